// compare_impl.hpp — the part of the packed-domain compare that does not depend on the predicate:
// the bitmap store rule (put_word) and the walk over the FastLanes blocks of one chunk
// (cmp_blocks), with the small helpers of the numeric predicates (cmp_op, CmpV, scalar_of,
// alp_factors, the patch position and bit assignment).  compare.hip tests op(epilogue(value),
// scalar); compare_range.hip tests a lower and an upper bound at once; compare_str.hip tests a bit
// of a dictionary's truth table.  filter_packed.hip takes the small helpers (alp_factors, patch_pos,
// cmp_table_index) for its own walk.  Included by those four units only.
#pragma once

#include <type_traits>

#include "compare.hpp"

namespace vxg {

namespace {

constexpr int kCmpThreads = 256;

template <int OP, class V>
__device__ __forceinline__ bool cmp_op(V v, V s) {
    if constexpr (OP == VXG_CMP_EQ) return v == s;
    else if constexpr (OP == VXG_CMP_NOT_EQ) return v != s;  // IEEE: true against NaN
    else if constexpr (OP == VXG_CMP_GT) return v > s;
    else if constexpr (OP == VXG_CMP_GTE) return v >= s;
    else if constexpr (OP == VXG_CMP_LT) return v < s;
    else return v <= s;
}

// The compared type of an epilogue output O: itself (unsigned, float) or its signed twin.
template <class O, int CK>
using CmpV = std::conditional_t<CK == kCmpSigned, std::make_signed_t<std::conditional_t<std::is_integral_v<O>, O, int>>, O>;

template <class V>
__device__ __forceinline__ V scalar_of(uint64_t bits) {
    V s;
    __builtin_memcpy(&s, &bits, sizeof(V));  // little-endian: the low bytes
    return s;
}

// ALP's factors F10[f] and IF10[e] from the chunk's exponents: the reference's tables
// (encodings/alp/src/alp/mod.rs:255-351; the same literals as capi.hip's, so the same bits).
template <Epi EPI>
__device__ __forceinline__ void alp_factors(uint32_t e, uint32_t f, double& a, double& b) {
    if constexpr (EPI == Epi::AlpF32) {
        constexpr float f10[11] = {1.0f, 10.0f, 100.0f, 1000.0f, 10000.0f, 100000.0f, 1000000.0f,
                                   10000000.0f, 100000000.0f, 1000000000.0f, 10000000000.0f};
        constexpr float if10[11] = {1.0f, 0.1f, 0.01f, 0.001f, 0.0001f, 0.00001f, 0.000001f,
                                    0.0000001f, 0.00000001f, 0.000000001f, 0.0000000001f};
        a = double(f10[f < 11 ? f : 0]);
        b = double(if10[e < 11 ? e : 0]);
    } else if constexpr (EPI == Epi::AlpF64) {
        constexpr double f10[24] = {
            1.0, 10.0, 100.0, 1000.0, 10000.0, 100000.0, 1000000.0, 10000000.0, 100000000.0,
            1000000000.0, 10000000000.0, 100000000000.0, 1000000000000.0, 10000000000000.0,
            100000000000000.0, 1000000000000000.0, 10000000000000000.0, 100000000000000000.0,
            1000000000000000000.0, 10000000000000000000.0, 100000000000000000000.0,
            1000000000000000000000.0, 10000000000000000000000.0, 100000000000000000000000.0};
        constexpr double if10[24] = {
            1.0, 0.1, 0.01, 0.001, 0.0001, 0.00001, 0.000001, 0.0000001, 0.00000001, 0.000000001,
            0.0000000001, 0.00000000001, 0.000000000001, 0.0000000000001, 0.00000000000001,
            0.000000000000001, 0.0000000000000001, 0.00000000000000001, 0.000000000000000001,
            0.0000000000000000001, 0.00000000000000000001, 0.000000000000000000001,
            0.0000000000000000000001, 0.00000000000000000000001};
        a = f10[f < 24 ? f : 0];
        b = if10[e < 24 ? e : 0];
    } else {
        a = b = 0.0;
    }
}

// Patch position i of a Sparse patches child, relative to the array (compare.hip's patch kernels).
__device__ __forceinline__ uint64_t patch_pos(const TakePatches& p, uint64_t i) {
    uint64_t v;
    switch (p.iw) {
    case 1: v = p.isg ? uint64_t(int64_t(gload(static_cast<const int8_t*>(p.idx) + i))) : gload(static_cast<const uint8_t*>(p.idx) + i); break;
    case 2: v = p.isg ? uint64_t(int64_t(gload(static_cast<const int16_t*>(p.idx) + i))) : gload(static_cast<const uint16_t*>(p.idx) + i); break;
    case 4: v = p.isg ? uint64_t(int64_t(gload(static_cast<const int32_t*>(p.idx) + i))) : gload(static_cast<const uint32_t*>(p.idx) + i); break;
    default: v = gload(static_cast<const uint64_t*>(p.idx) + i); break;
    }
    return v - p.off;
}

__device__ __forceinline__ void assign_bit(uint32_t* __restrict__ out, uint64_t bit, bool v) {
    const uint32_t m = 1u << (bit & 31);
    if (v) __hip_atomic_fetch_or(out + (bit >> 5), m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else __hip_atomic_fetch_and(out + (bit >> 5), ~m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

unsigned cmp_grid(uint64_t n_threads) {
    const uint64_t g = (n_threads + kCmpThreads - 1) / kCmpThreads;
    return unsigned(g > 32768 ? 32768 : (g ? g : 1));
}

// One bitmap word of a producer that covers bits [cb, ce): `own` = all 64 bits of the word are
// this producer's to write.
__device__ __forceinline__ void put_word(uint64_t* __restrict__ out, int64_t word, uint64_t bits, bool own, bool excl,
                                         int64_t cb, int64_t ce) {
    const int64_t lo = word * 64;
    if (lo >= ce || lo + 64 <= cb) return;  // no row of the producer in this word
    if (excl || (own && lo >= cb && lo + 64 <= ce))
        gstore(out + word, bits);
    else if (bits)
        __hip_atomic_fetch_or(out + word, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The blocks of chunk `c` that workgroup `g` takes (compare.hip's header describes the walk).
// `mk()` builds the predicate after the packed words are staged: P::test(raw) is the bit of one
// unpacked T-bit value; a predicate with P::kChecks is then told by P::check(in_range) whether the
// position it just tested is a row of the chunk (slack positions hold arbitrary bits).
// `c` lives in the kernel argument: its fields are read with scalar loads where they are used.
template <int T, class MK>
__device__ __forceinline__ void cmp_blocks(const CmpChunk& c, uint32_t g, uint64_t* __restrict__ out, uint8_t* lds, MK mk) {
    using E = typename Fl<T>::E;
    constexpr uint32_t LANES = 1024 / T;
    constexpr uint32_t LT = T == 64 ? 6 : (T == 32 ? 5 : (T == 16 ? 4 : 3));
    const uint32_t W = c.W, bpw = c.bpw(), offset = c.offset, tid = threadIdx.x, wave = tid >> 6, l = tid & 63;
    const uint64_t len = c.len(), n_blocks = c.n_blocks();
    const uint64_t blk0 = uint64_t(g - c.first_group) * bpw;
    if (blk0 >= n_blocks) return;  // workgroup-uniform
    const uint32_t nb = uint32_t(n_blocks - blk0 < uint64_t(bpw) ? n_blocks - blk0 : uint64_t(bpw));
    E* const s_packed = reinterpret_cast<E*>(lds);
    const uint32_t q16 = nb * 8 * W;
    for (uint32_t q = tid; q < q16; q += kCmpThreads)
        reinterpret_cast<uint4*>(s_packed)[q] = gload(reinterpret_cast<const uint4*>(c.packed + blk0 * (128ull * W)) + q);
    __syncthreads();

    auto pred = mk();
    using P = decltype(pred);
    const int64_t cb = int64_t(c.out_bit), ce = int64_t(c.out_bit + len);
    const int64_t base = cb - int64_t(offset);  // bitmap bit of packed position 0
    const uint32_t d = uint32_t(uint64_t(base) & 63u);
    const uint32_t j = (l - d) & 63u;
    // packed position 64 m + j of a block: its lane's word index and the bit offset of its row,
    // for even and odd m
    uint32_t lane_x[2], start_x[2];
#pragma unroll
    for (uint32_t x = 0; x < 2; x++) {
        const uint32_t idx = 64 * x + j;
        lane_x[x] = idx % LANES;
        const uint32_t fl = (idx - lane_x[x]) >> 4;
        start_x[x] = __umul24((((fl & 1) << 2) | (fl & 2) | (fl >> 2)) * 8, W);  // FL_ORDER[fl] * 8 * W
    }
    const E mask = W >= uint32_t(T) ? E(~E(0)) : E((E(1) << W) - E(1));
    const uint64_t low = d ? (1ull << d) - 1ull : 0ull;  // bits of a ballot that belong to the next word
    const bool excl = c.excl();

    // a wave takes consecutive blocks, so the bits a block leaves for the next word (d != 0) are
    // carried into the next block's word 0 instead of being ORed in: only the first and last word
    // of a wave's run are shared with another wave
    const uint32_t per = (nb + kCmpThreads / 64 - 1) / (kCmpThreads / 64);
    const uint32_t b_begin = wave * per, b_end = b_begin + per < nb ? b_begin + per : nb;
    uint64_t carry = 0;  // uniform
    for (uint32_t b = b_begin; b < b_end; b++) {  // wave-uniform
        const E* __restrict__ pw = s_packed + b * (LANES * W);
        const uint64_t p0 = (blk0 + b) * 1024;  // packed position of the block's first value
        const bool full = p0 >= offset && p0 + 1024 <= uint64_t(offset) + len;
        uint64_t cur = 0;  // lane m: ballot m
        auto steps = [&](auto full_c) {  // unswitched: a block inside the chunk checks no position
#pragma unroll
        for (uint32_t m = 0; m < 16; m++) {
            E raw = 0;
            if (W) {
                // word w0 + 1 may be the next block's first row or the slack row: a value that ends
                // inside word w0 masks those bits off
                const uint32_t start = start_x[m & 1] + (m >> 1) * W, w0 = start >> LT;
                const E* __restrict__ q = pw + (LANES * w0 + lane_x[m & 1]);
                const E lo = q[0], hi = q[LANES];
                if constexpr (T == 64) {
                    const uint32_t sh = start & 63;
                    raw = (sh ? (lo >> sh) | (hi << (64 - sh)) : lo) & mask;
                } else if constexpr (T == 32) {
                    raw = E(__builtin_amdgcn_alignbit(hi, lo, start) & mask);  // shifts by start % 32
                } else {
                    raw = E(((uint32_t(lo) | (uint32_t(hi) << T)) >> (start & (T - 1))) & mask);
                }
            }
            bool pr = pred.test(raw);
            if constexpr (!decltype(full_c)::value) {
                const uint64_t p = p0 + 64 * m + j;
                pr = pr && p >= offset && p < uint64_t(offset) + len;
                if constexpr (P::kChecks) pred.check(p >= offset && p < uint64_t(offset) + len);
            } else if constexpr (P::kChecks) {
                pred.check(true);
            }
            const uint64_t bal = __ballot(pr);
            if (l == m) cur = bal;
        }
        };
        if (full) steps(std::true_type{});
        else steps(std::false_type{});
        // lane i owns word i of the block: ballot i's bits >= d and ballot i - 1's bits < d
        uint64_t prev = 0;
        if (d) {  // uniform: the previous lane's ballot, once per block
            const uint64_t up = uint64_t(uint32_t(__shfl_up(int(uint32_t(cur)), 1))) |
                                uint64_t(uint32_t(__shfl_up(int(uint32_t(cur >> 32)), 1))) << 32;
            prev = l ? up : carry;
        }
        const uint64_t bits = (cur & ~low) | (prev & low);
        const bool last = b + 1 == b_end;
        if (l < 16 || (l == 16 && last)) {
            const int64_t word = ((base + int64_t(p0)) >> 6) + int64_t(l);  // floor: base may be negative
            put_word(out, word, bits, l < 16 && (d == 0 || l >= 1 || b != b_begin), excl && l < 16, cb, ce);
        }
        if (d)  // lane 16 holds the bits of the word this block shares with the next one
            carry = uint64_t(uint32_t(__builtin_amdgcn_readlane(int(uint32_t(bits)), 16))) |
                    uint64_t(uint32_t(__builtin_amdgcn_readlane(int(uint32_t(bits >> 32)), 16))) << 32;
    }
}

// Workgroup g's entry of a kernel-argument table sorted by first_group (uniform, scalar loads).
template <class TAB>
__device__ __forceinline__ uint32_t cmp_table_index(const TAB& tab, uint32_t g) {
    uint32_t lo = 0, hi = tab.n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tab.c[mid].first_group <= g) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace

}  // namespace vxg
