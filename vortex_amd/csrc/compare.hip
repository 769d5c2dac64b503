// compare.hip — compute::compare of an array with a scalar (vortex-array/src/compute/compare.rs:
// 81-124), in the packed domain where the tree is a BitPacked-rooted cascade.
//
// The reference scan builds its row mask with compare and then filters (vortex-serde/src/layouts/
// read/filtering.rs:27-43).  Canonicalizing first writes T bits per value only to read them back;
// the fused kernel here reads the W packed bits and writes 1 bit per value:
//   * a workgroup stages the packed words of `bpw` consecutive FastLanes blocks of one chunk into
//     LDS with coalesced 16-byte loads (every packed byte is read once);
//   * a wave takes whole blocks.  In step m (0..15) lane l extracts packed position 64 m + j of
//     the block, j = (l - d) mod 64 with d = the bitmap bit of the block's position 0 mod 64, so
//     the value's bit sits at bit l of its bitmap word: the 64-bit ballot of the compare IS that
//     word (bits >= d) and the next word (bits < d).  Lane and FL_ORDER group of position 64 m + j
//     depend only on the parity of m and the row advances by one every two steps, so the bit
//     offset is a per-lane constant plus a uniform term;
//   * the decoded value is apply_epi's (fl_unpack_impl.hpp), the arithmetic of canonicalize;
//   * lane m keeps ballot m (the previous lane's comes by one shuffle per block); lane i then owns
//     word i of the block: a word whose 64 bits all come from this block and lie
//     inside the chunk is one plain 8-byte store.  A wave takes consecutive blocks and carries
//     the bits a block leaves for the next word (d != 0) into the next block's word 0, so only
//     the first and last word of a wave's run, and the words cut by the chunk's start or end, are
//     ORed into the zeroed bitmap.
// Patched rows are re-compared afterwards (patch kernels); every other encoding is canonicalized
// by the planner and compared by the plain kernel, which writes bits with the same store rule.
#include "compare_impl.hpp"

namespace vxg {

namespace {

template <class V>
__device__ __forceinline__ bool cmp_rt(int op, V v, V s) {
    switch (op) {
    case VXG_CMP_EQ: return v == s;
    case VXG_CMP_NOT_EQ: return v != s;
    case VXG_CMP_GT: return v > s;
    case VXG_CMP_GTE: return v >= s;
    case VXG_CMP_LT: return v < s;
    default: return v <= s;
    }
}

// The predicate of cmp_blocks (compare_impl.hpp): op(epilogue(raw), scalar).
template <int T, Epi EPI, int CK, int OP>
struct EpiPred {
    using E = typename Fl<T>::E;
    using V = CmpV<typename EpiOut<T, EPI, 0>::type, CK>;
    static constexpr bool kChecks = false;
    EpiParams ep;
    V s;
    __device__ __forceinline__ bool test(E raw) const { return cmp_op<OP>(V(apply_epi<T, EPI, 0>(raw, ep)), s); }
    __device__ __forceinline__ void check(bool) const {}
};

template <int T, Epi EPI, int CK, int OP>
__device__ __forceinline__ void cmp_chunk(const CmpChunk& c, uint32_t g, uint64_t* __restrict__ out, uint64_t sbits,
                                          uint8_t* lds) {
    using P = EpiPred<T, EPI, CK, OP>;
    cmp_blocks<T>(c, g, out, lds, [&] {
        EpiParams ep{};
        ep.reference = c.reference;
        ep.shift = c.shift;
        alp_factors<EPI>(c.alp_e, c.alp_f, ep.alp_a, ep.alp_b);
        return P{ep, scalar_of<typename P::V>(sbits)};
    });
}

template <int T, Epi EPI, int CK>
__global__ __launch_bounds__(kCmpThreads) void cmp_packed_kernel(CmpTable tab, uint64_t* __restrict__ out,
                                                                 uint64_t sbits, int op) {
    extern __shared__ __attribute__((aligned(16))) uint8_t cmp_lds[];
    const uint32_t g = blockIdx.x;
    uint32_t lo = 0, hi = tab.n;
    while (hi - lo > 1) {  // uniform, on the kernel argument
        const uint32_t mid = (lo + hi) >> 1;
        if (tab.c[mid].first_group <= g) lo = mid; else hi = mid;
    }
    const CmpChunk& c = tab.c[lo];
    switch (op) {  // uniform: one straight-line body per operator
    case VXG_CMP_EQ: cmp_chunk<T, EPI, CK, VXG_CMP_EQ>(c, g, out, sbits, cmp_lds); break;
    case VXG_CMP_NOT_EQ: cmp_chunk<T, EPI, CK, VXG_CMP_NOT_EQ>(c, g, out, sbits, cmp_lds); break;
    case VXG_CMP_GT: cmp_chunk<T, EPI, CK, VXG_CMP_GT>(c, g, out, sbits, cmp_lds); break;
    case VXG_CMP_GTE: cmp_chunk<T, EPI, CK, VXG_CMP_GTE>(c, g, out, sbits, cmp_lds); break;
    case VXG_CMP_LT: cmp_chunk<T, EPI, CK, VXG_CMP_LT>(c, g, out, sbits, cmp_lds); break;
    default: cmp_chunk<T, EPI, CK, VXG_CMP_LTE>(c, g, out, sbits, cmp_lds); break;
    }
}

// ---- plain compare: one wave per bitmap word, lane l = bit l of the word ------------------
template <class V, int OP>
__device__ __forceinline__ void cmp_plain_body(const V* __restrict__ in, uint64_t n, uint64_t* __restrict__ out,
                                               uint64_t out_bit, V s, bool excl) {
    const uint32_t l = threadIdx.x & 63;
    const int64_t cb = int64_t(out_bit), ce = int64_t(out_bit + n);
    const int64_t first = cb >> 6, n_words = ((ce + 63) >> 6) - first;
    const int64_t waves = int64_t(gridDim.x) * (kCmpThreads / 64);
    for (int64_t w = int64_t(blockIdx.x) * (kCmpThreads / 64) + (threadIdx.x >> 6); w < n_words; w += waves) {
        const int64_t i = (first + w) * 64 + int64_t(l) - cb;
        const bool in_range = i >= 0 && uint64_t(i) < n;
        const V v = in_range ? gload(in + i) : V(0);
        const uint64_t bal = __ballot(in_range && cmp_op<OP>(v, s));
        if (l == 0) put_word(out, first + w, bal, true, excl, cb, ce);
    }
}

template <class V>
__global__ __launch_bounds__(kCmpThreads) void cmp_plain_kernel(const V* __restrict__ in, uint64_t n,
                                                                uint64_t* __restrict__ out, uint64_t out_bit,
                                                                uint64_t sbits, int op, int excl) {
    const V s = scalar_of<V>(sbits);
    switch (op) {
    case VXG_CMP_EQ: cmp_plain_body<V, VXG_CMP_EQ>(in, n, out, out_bit, s, excl != 0); break;
    case VXG_CMP_NOT_EQ: cmp_plain_body<V, VXG_CMP_NOT_EQ>(in, n, out, out_bit, s, excl != 0); break;
    case VXG_CMP_GT: cmp_plain_body<V, VXG_CMP_GT>(in, n, out, out_bit, s, excl != 0); break;
    case VXG_CMP_GTE: cmp_plain_body<V, VXG_CMP_GTE>(in, n, out, out_bit, s, excl != 0); break;
    case VXG_CMP_LT: cmp_plain_body<V, VXG_CMP_LT>(in, n, out, out_bit, s, excl != 0); break;
    default: cmp_plain_body<V, VXG_CMP_LTE>(in, n, out, out_bit, s, excl != 0); break;
    }
}

// ---- patches: re-compare the patched rows, set or clear their bits ------------------------
template <int T, Epi EPI, int CK>
__global__ __launch_bounds__(kCmpThreads) void cmp_patch_kernel(TakePatches p, uint64_t len, uint32_t* __restrict__ out,
                                                                uint64_t out_bit, EpiParams ep, uint64_t sbits, int op) {
    using E = typename Fl<T>::E;
    using V = CmpV<typename EpiOut<T, EPI, 0>::type, CK>;
    const V s = scalar_of<V>(sbits);
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < p.n; i += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t pos = patch_pos(p, i);
        if (pos >= len) {
            __hip_atomic_fetch_or(ep.err, kErrPatchOOB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
        const V v = V(apply_epi<T, EPI, 0>(gload(static_cast<const E*>(p.values) + i), ep));
        assign_bit(out, out_bit + pos, cmp_rt(op, v, s));
    }
}

template <class V>
__global__ __launch_bounds__(kCmpThreads) void cmp_patch_raw_kernel(TakePatches p, uint64_t len, uint32_t* __restrict__ out,
                                                                    uint64_t out_bit, uint64_t sbits, int op, uint32_t* err) {
    const V s = scalar_of<V>(sbits);
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < p.n; i += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t pos = patch_pos(p, i);
        if (pos >= len) {
            __hip_atomic_fetch_or(err, kErrPatchOOB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
        assign_bit(out, out_bit + pos, cmp_rt(op, gload(static_cast<const V*>(p.values) + i), s));
    }
}

__global__ __launch_bounds__(kCmpThreads) void and_words_kernel(uint64_t* __restrict__ bits, const uint64_t* __restrict__ mask,
                                                                uint64_t n) {
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += uint64_t(gridDim.x) * blockDim.x)
        bits[i] &= mask[i];
}

template <int T, Epi EPI, int CK>
vxg_status packed_launch(const CmpTable& tab, uint64_t groups, uint32_t lds_bytes, void* out, uint64_t sbits, int op,
                         hipStream_t s) {
    hipLaunchKernelGGL((cmp_packed_kernel<T, EPI, CK>), dim3(unsigned(groups)), dim3(kCmpThreads), lds_bytes, s, tab,
                       static_cast<uint64_t*>(out), sbits, op);
    return hip_check(hipGetLastError(), "cmp_packed_kernel");
}

}  // namespace

vxg_status launch_cmp_packed(int T, Epi epi, int ck, const CmpTable& tab, uint64_t groups, uint32_t lds_bytes, void* out,
                             uint64_t sbits, int op, hipStream_t s) {
    if (groups == 0 || groups > 0x7FFFFFFFull || lds_bytes > 64 * 1024)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "compare: bad launch shape");
#define VXG_CMP(TT, EE, CC)                                                                          \
    if (T == TT && epi == EE && ck == CC) return packed_launch<TT, EE, CC>(tab, groups, lds_bytes, out, sbits, op, s);
#define VXG_CMP_INT(TT)                                                                              \
    VXG_CMP(TT, Epi::Plain, kCmpUnsigned) VXG_CMP(TT, Epi::Plain, kCmpSigned) VXG_CMP(TT, Epi::For, kCmpUnsigned) \
    VXG_CMP(TT, Epi::For, kCmpSigned) VXG_CMP(TT, Epi::ForZigZag, kCmpSigned)
    VXG_CMP_INT(8) VXG_CMP_INT(16) VXG_CMP_INT(32) VXG_CMP_INT(64)
    VXG_CMP(32, Epi::AlpF32, kCmpFloat) VXG_CMP(64, Epi::AlpF64, kCmpFloat)
#undef VXG_CMP_INT
#undef VXG_CMP
    return set_error(VXG_ERR_NOT_IMPLEMENTED, "compare: unsupported BitPacked cascade");
}

vxg_status launch_cmp_plain(int ptype, const void* in, uint64_t n, void* out, uint64_t out_bit, uint64_t sbits, int op,
                            bool excl, hipStream_t s) {
    if (n == 0) return VXG_OK;
    const uint64_t words = ((out_bit + n + 63) >> 6) - (out_bit >> 6);
    const dim3 grid(cmp_grid(words * 64)), block(kCmpThreads);
#define VXG_CMP_PLAIN(PT, VV)                                                                        \
    case PT:                                                                                         \
        hipLaunchKernelGGL((cmp_plain_kernel<VV>), grid, block, 0, s, static_cast<const VV*>(in), n, \
                           static_cast<uint64_t*>(out), out_bit, sbits, op, int(excl));              \
        break;
    switch (ptype) {
        VXG_CMP_PLAIN(VXG_U8, uint8_t) VXG_CMP_PLAIN(VXG_U16, uint16_t) VXG_CMP_PLAIN(VXG_U32, uint32_t)
        VXG_CMP_PLAIN(VXG_U64, uint64_t) VXG_CMP_PLAIN(VXG_I8, int8_t) VXG_CMP_PLAIN(VXG_I16, int16_t)
        VXG_CMP_PLAIN(VXG_I32, int32_t) VXG_CMP_PLAIN(VXG_I64, int64_t) VXG_CMP_PLAIN(VXG_F32, float)
        VXG_CMP_PLAIN(VXG_F64, double)
    default: return set_error(VXG_ERR_NOT_IMPLEMENTED, "compare: unsupported ptype");
    }
#undef VXG_CMP_PLAIN
    return hip_check(hipGetLastError(), "cmp_plain_kernel");
}

vxg_status launch_cmp_patch(int T, Epi epi, int ck, const TakePatches& p, uint64_t len, void* out, uint64_t out_bit,
                            const EpiParams& ep, uint64_t sbits, int op, hipStream_t s) {
    if (p.n == 0) return VXG_OK;
    const dim3 grid(cmp_grid(p.n)), block(kCmpThreads);
#define VXG_CMPP(TT, EE, CC)                                                                         \
    if (T == TT && epi == EE && ck == CC) {                                                          \
        hipLaunchKernelGGL((cmp_patch_kernel<TT, EE, CC>), grid, block, 0, s, p, len,                \
                           static_cast<uint32_t*>(out), out_bit, ep, sbits, op);                     \
        return hip_check(hipGetLastError(), "cmp_patch_kernel");                                     \
    }
#define VXG_CMPP_INT(TT)                                                                             \
    VXG_CMPP(TT, Epi::Plain, kCmpUnsigned) VXG_CMPP(TT, Epi::Plain, kCmpSigned) VXG_CMPP(TT, Epi::For, kCmpUnsigned) \
    VXG_CMPP(TT, Epi::For, kCmpSigned) VXG_CMPP(TT, Epi::ForZigZag, kCmpSigned)
    VXG_CMPP_INT(8) VXG_CMPP_INT(16) VXG_CMPP_INT(32) VXG_CMPP_INT(64)
    VXG_CMPP(32, Epi::AlpF32, kCmpFloat) VXG_CMPP(64, Epi::AlpF64, kCmpFloat)
#undef VXG_CMPP_INT
#undef VXG_CMPP
    return set_error(VXG_ERR_NOT_IMPLEMENTED, "compare: unsupported BitPacked cascade");
}

vxg_status launch_cmp_patch_raw(int ptype, const TakePatches& p, uint64_t len, void* out, uint64_t out_bit,
                                uint64_t sbits, int op, uint32_t* err, hipStream_t s) {
    if (p.n == 0) return VXG_OK;
    const dim3 grid(cmp_grid(p.n)), block(kCmpThreads);
    if (ptype == VXG_F32)
        hipLaunchKernelGGL((cmp_patch_raw_kernel<float>), grid, block, 0, s, p, len, static_cast<uint32_t*>(out), out_bit,
                           sbits, op, err);
    else if (ptype == VXG_F64)
        hipLaunchKernelGGL((cmp_patch_raw_kernel<double>), grid, block, 0, s, p, len, static_cast<uint32_t*>(out), out_bit,
                           sbits, op, err);
    else
        return set_error(VXG_ERR_NOT_IMPLEMENTED, "compare: outer patches are f32 or f64");
    return hip_check(hipGetLastError(), "cmp_patch_raw_kernel");
}

vxg_status launch_and_words(void* bits, const void* mask, uint64_t n_words, hipStream_t s) {
    if (n_words == 0) return VXG_OK;
    hipLaunchKernelGGL(and_words_kernel, dim3(cmp_grid(n_words)), dim3(kCmpThreads), 0, s, static_cast<uint64_t*>(bits),
                       static_cast<const uint64_t*>(mask), n_words);
    return hip_check(hipGetLastError(), "and_words_kernel");
}

}  // namespace vxg
