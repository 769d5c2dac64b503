// compare_range.hip — the kernels of a scan's row filter (vxg_row_filter; RowFilter::evaluate,
// vortex-serde/src/layouts/read/filtering.rs:27-43) that a single compare does not have:
//   * K18r, the two-sided twins of compare.hip's kernels: a range on one column
//     (lo_op in {>, >=} AND hi_op in {<, <=}) tested on the value while it is in a register.  The
//     packed kernel is cmp_blocks (compare_impl.hpp) with a predicate of two tests, so the block
//     walk, the bitmap store rule, the CmpTable argument and the LDS size are compare.hip's; every
//     twin is bit for bit the AND of the two one-sided results (ordered compares with NaN are false
//     on either side);
//   * K21, the combine: out[w] = in_0[w] & ... & in_{k-1}[w] over 64-bit words, k <= 16 pointers in
//     the kernel argument, and optionally the number of set bits added to a device counter with one
//     atomic per workgroup.
#include <algorithm>

#include "compare_impl.hpp"

namespace vxg {

namespace {

// (lower, upper) operator pair -> 0..3: bit 0 = the lower bound is >=, bit 1 = the upper bound is <=.
__host__ __device__ constexpr int range_code(int lo_op, int hi_op) {
    return (lo_op == VXG_CMP_GTE ? 1 : 0) | (hi_op == VXG_CMP_LTE ? 2 : 0);
}

template <int RC, class V>
__device__ __forceinline__ bool range_op(V v, V lo, V hi) {
    constexpr int LO = (RC & 1) ? VXG_CMP_GTE : VXG_CMP_GT;
    constexpr int HI = (RC & 2) ? VXG_CMP_LTE : VXG_CMP_LT;
    return cmp_op<LO>(v, lo) && cmp_op<HI>(v, hi);
}

template <class V>
__device__ __forceinline__ bool range_rt(int rc, V v, V lo, V hi) {
    switch (rc) {
    case 0: return range_op<0>(v, lo, hi);
    case 1: return range_op<1>(v, lo, hi);
    case 2: return range_op<2>(v, lo, hi);
    default: return range_op<3>(v, lo, hi);
    }
}

// The two-sided predicate of cmp_blocks: lo_op(epilogue(raw), s_lo) && hi_op(epilogue(raw), s_hi).
template <int T, Epi EPI, int CK, int RC>
struct RangePred {
    using E = typename Fl<T>::E;
    using V = CmpV<typename EpiOut<T, EPI, 0>::type, CK>;
    static constexpr bool kChecks = false;
    EpiParams ep;
    V lo, hi;
    __device__ __forceinline__ bool test(E raw) const { return range_op<RC>(V(apply_epi<T, EPI, 0>(raw, ep)), lo, hi); }
    __device__ __forceinline__ void check(bool) const {}
};

template <int T, Epi EPI, int CK, int RC>
__device__ __forceinline__ void range_chunk(const CmpChunk& c, uint32_t g, uint64_t* __restrict__ out, uint64_t lo_bits,
                                            uint64_t hi_bits, uint8_t* lds) {
    using P = RangePred<T, EPI, CK, RC>;
    cmp_blocks<T>(c, g, out, lds, [&] {
        EpiParams ep{};
        ep.reference = c.reference;
        ep.shift = c.shift;
        alp_factors<EPI>(c.alp_e, c.alp_f, ep.alp_a, ep.alp_b);
        return P{ep, scalar_of<typename P::V>(lo_bits), scalar_of<typename P::V>(hi_bits)};
    });
}

template <int T, Epi EPI, int CK>
__global__ __launch_bounds__(kCmpThreads) void cmp_range_packed_kernel(CmpTable tab, uint64_t* __restrict__ out,
                                                                       uint64_t lo_bits, uint64_t hi_bits, int rc) {
    extern __shared__ __attribute__((aligned(16))) uint8_t cmp_lds[];
    const uint32_t g = blockIdx.x;
    const CmpChunk& c = tab.c[cmp_table_index(tab, g)];
    switch (rc) {  // uniform: one straight-line body per operator pair
    case 0: range_chunk<T, EPI, CK, 0>(c, g, out, lo_bits, hi_bits, cmp_lds); break;
    case 1: range_chunk<T, EPI, CK, 1>(c, g, out, lo_bits, hi_bits, cmp_lds); break;
    case 2: range_chunk<T, EPI, CK, 2>(c, g, out, lo_bits, hi_bits, cmp_lds); break;
    default: range_chunk<T, EPI, CK, 3>(c, g, out, lo_bits, hi_bits, cmp_lds); break;
    }
}

// ---- plain: one wave per bitmap word, lane l = bit l of the word ----------------------------
template <class V, int RC>
__device__ __forceinline__ void range_plain_body(const V* __restrict__ in, uint64_t n, uint64_t* __restrict__ out,
                                                 uint64_t out_bit, V lo, V hi, bool excl) {
    const uint32_t l = threadIdx.x & 63;
    const int64_t cb = int64_t(out_bit), ce = int64_t(out_bit + n);
    const int64_t first = cb >> 6, n_words = ((ce + 63) >> 6) - first;
    const int64_t waves = int64_t(gridDim.x) * (kCmpThreads / 64);
    for (int64_t w = int64_t(blockIdx.x) * (kCmpThreads / 64) + (threadIdx.x >> 6); w < n_words; w += waves) {
        const int64_t i = (first + w) * 64 + int64_t(l) - cb;
        const bool in_range = i >= 0 && uint64_t(i) < n;
        const V v = in_range ? gload(in + i) : V(0);
        const uint64_t bal = __ballot(in_range && range_op<RC>(v, lo, hi));
        if (l == 0) put_word(out, first + w, bal, true, excl, cb, ce);
    }
}

template <class V>
__global__ __launch_bounds__(kCmpThreads) void cmp_range_plain_kernel(const V* __restrict__ in, uint64_t n,
                                                                      uint64_t* __restrict__ out, uint64_t out_bit,
                                                                      uint64_t lo_bits, uint64_t hi_bits, int rc, int excl) {
    const V lo = scalar_of<V>(lo_bits), hi = scalar_of<V>(hi_bits);
    switch (rc) {
    case 0: range_plain_body<V, 0>(in, n, out, out_bit, lo, hi, excl != 0); break;
    case 1: range_plain_body<V, 1>(in, n, out, out_bit, lo, hi, excl != 0); break;
    case 2: range_plain_body<V, 2>(in, n, out, out_bit, lo, hi, excl != 0); break;
    default: range_plain_body<V, 3>(in, n, out, out_bit, lo, hi, excl != 0); break;
    }
}

// ---- patches: re-test the patched rows, set or clear their bits ------------------------------
template <int T, Epi EPI, int CK>
__global__ __launch_bounds__(kCmpThreads) void cmp_range_patch_kernel(TakePatches p, uint64_t len, uint32_t* __restrict__ out,
                                                                      uint64_t out_bit, EpiParams ep, uint64_t lo_bits,
                                                                      uint64_t hi_bits, int rc) {
    using E = typename Fl<T>::E;
    using V = CmpV<typename EpiOut<T, EPI, 0>::type, CK>;
    const V lo = scalar_of<V>(lo_bits), hi = scalar_of<V>(hi_bits);
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < p.n; i += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t pos = patch_pos(p, i);
        if (pos >= len) {
            __hip_atomic_fetch_or(ep.err, kErrPatchOOB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
        const V v = V(apply_epi<T, EPI, 0>(gload(static_cast<const E*>(p.values) + i), ep));
        assign_bit(out, out_bit + pos, range_rt(rc, v, lo, hi));
    }
}

template <class V>
__global__ __launch_bounds__(kCmpThreads) void cmp_range_patch_raw_kernel(TakePatches p, uint64_t len,
                                                                          uint32_t* __restrict__ out, uint64_t out_bit,
                                                                          uint64_t lo_bits, uint64_t hi_bits, int rc,
                                                                          uint32_t* err) {
    const V lo = scalar_of<V>(lo_bits), hi = scalar_of<V>(hi_bits);
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < p.n; i += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t pos = patch_pos(p, i);
        if (pos >= len) {
            __hip_atomic_fetch_or(err, kErrPatchOOB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
        assign_bit(out, out_bit + pos, range_rt(rc, gload(static_cast<const V*>(p.values) + i), lo, hi));
    }
}

// ---- K21: AND of bitmaps (+ the true count) ---------------------------------------------------
// `out` may alias an input: a thread reads index w of every input before it writes out[w], and no
// other thread touches index w.  COUNT: every thread popcounts the words it wrote, the workgroup
// sums through LDS and one thread adds the sum to *count (zeroed on the stream beforehand).
template <bool COUNT>
__global__ __launch_bounds__(kCmpThreads) void and_count_kernel(AndInputs in, uint64_t* out, uint64_t n_words,
                                                                uint64_t* count) {
    uint32_t ones = 0;  // (a thread's words hold far fewer than 2^32 bits: n_words <= 2^34 over >= 2^19 threads)
    for (uint64_t w = uint64_t(blockIdx.x) * kCmpThreads + threadIdx.x; w < n_words; w += uint64_t(gridDim.x) * kCmpThreads) {
        uint64_t v = gload(in.p[0] + w);
        for (uint32_t i = 1; i < in.k; i++) v &= gload(in.p[i] + w);  // uniform trip count
        gstore(out + w, v);
        if constexpr (COUNT) ones += uint32_t(__popcll(v));
    }
    if constexpr (COUNT) {
        __shared__ uint64_t wave_sum[kCmpThreads / 64];
        uint64_t s = ones;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            s += uint64_t(uint32_t(__shfl_down(int(uint32_t(s)), d))) | uint64_t(uint32_t(__shfl_down(int(uint32_t(s >> 32)), d))) << 32;
        }
        if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t t = 0;
#pragma unroll
            for (int i = 0; i < kCmpThreads / 64; i++) t += wave_sum[i];
            if (t) __hip_atomic_fetch_add(count, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <int T, Epi EPI, int CK>
vxg_status range_packed_launch(const CmpTable& tab, uint64_t groups, uint32_t lds_bytes, void* out, uint64_t lo_bits,
                               uint64_t hi_bits, int rc, hipStream_t s) {
    hipLaunchKernelGGL((cmp_range_packed_kernel<T, EPI, CK>), dim3(unsigned(groups)), dim3(kCmpThreads), lds_bytes, s, tab,
                       static_cast<uint64_t*>(out), lo_bits, hi_bits, rc);
    return hip_check(hipGetLastError(), "cmp_range_packed_kernel");
}

bool range_ops_ok(int lo_op, int hi_op) {
    return (lo_op == VXG_CMP_GT || lo_op == VXG_CMP_GTE) && (hi_op == VXG_CMP_LT || hi_op == VXG_CMP_LTE);
}

}  // namespace

vxg_status launch_cmp_range_packed(int T, Epi epi, int ck, const CmpTable& tab, uint64_t groups, uint32_t lds_bytes,
                                   void* out, const CmpRange& r, hipStream_t s) {
    if (groups == 0 || groups > 0x7FFFFFFFull || lds_bytes > 64 * 1024 || !range_ops_ok(r.lo_op, r.hi_op))
        return set_error(VXG_ERR_INVALID_ARGUMENT, "range compare: bad launch shape");
    const int rc = range_code(r.lo_op, r.hi_op);
#define VXG_CMP(TT, EE, CC)                                                                          \
    if (T == TT && epi == EE && ck == CC)                                                            \
        return range_packed_launch<TT, EE, CC>(tab, groups, lds_bytes, out, r.lo_bits, r.hi_bits, rc, s);
#define VXG_CMP_INT(TT)                                                                              \
    VXG_CMP(TT, Epi::Plain, kCmpUnsigned) VXG_CMP(TT, Epi::Plain, kCmpSigned) VXG_CMP(TT, Epi::For, kCmpUnsigned) \
    VXG_CMP(TT, Epi::For, kCmpSigned) VXG_CMP(TT, Epi::ForZigZag, kCmpSigned)
    VXG_CMP_INT(8) VXG_CMP_INT(16) VXG_CMP_INT(32) VXG_CMP_INT(64)
    VXG_CMP(32, Epi::AlpF32, kCmpFloat) VXG_CMP(64, Epi::AlpF64, kCmpFloat)
#undef VXG_CMP_INT
#undef VXG_CMP
    return set_error(VXG_ERR_NOT_IMPLEMENTED, "compare: unsupported BitPacked cascade");
}

vxg_status launch_cmp_range_plain(int ptype, const void* in, uint64_t n, void* out, uint64_t out_bit, const CmpRange& r,
                                  bool excl, hipStream_t s) {
    if (!range_ops_ok(r.lo_op, r.hi_op)) return set_error(VXG_ERR_INVALID_ARGUMENT, "range compare: bad operators");
    if (n == 0) return VXG_OK;
    const int rc = range_code(r.lo_op, r.hi_op);
    const uint64_t words = ((out_bit + n + 63) >> 6) - (out_bit >> 6);
    const dim3 grid(cmp_grid(words * 64)), block(kCmpThreads);
#define VXG_CMP_PLAIN(PT, VV)                                                                              \
    case PT:                                                                                               \
        hipLaunchKernelGGL((cmp_range_plain_kernel<VV>), grid, block, 0, s, static_cast<const VV*>(in), n, \
                           static_cast<uint64_t*>(out), out_bit, r.lo_bits, r.hi_bits, rc, int(excl));     \
        break;
    switch (ptype) {
        VXG_CMP_PLAIN(VXG_U8, uint8_t) VXG_CMP_PLAIN(VXG_U16, uint16_t) VXG_CMP_PLAIN(VXG_U32, uint32_t)
        VXG_CMP_PLAIN(VXG_U64, uint64_t) VXG_CMP_PLAIN(VXG_I8, int8_t) VXG_CMP_PLAIN(VXG_I16, int16_t)
        VXG_CMP_PLAIN(VXG_I32, int32_t) VXG_CMP_PLAIN(VXG_I64, int64_t) VXG_CMP_PLAIN(VXG_F32, float)
        VXG_CMP_PLAIN(VXG_F64, double)
    default: return set_error(VXG_ERR_NOT_IMPLEMENTED, "compare: unsupported ptype");
    }
#undef VXG_CMP_PLAIN
    return hip_check(hipGetLastError(), "cmp_range_plain_kernel");
}

vxg_status launch_cmp_range_patch(int T, Epi epi, int ck, const TakePatches& p, uint64_t len, void* out, uint64_t out_bit,
                                  const EpiParams& ep, const CmpRange& r, hipStream_t s) {
    if (!range_ops_ok(r.lo_op, r.hi_op)) return set_error(VXG_ERR_INVALID_ARGUMENT, "range compare: bad operators");
    if (p.n == 0) return VXG_OK;
    const int rc = range_code(r.lo_op, r.hi_op);
    const dim3 grid(cmp_grid(p.n)), block(kCmpThreads);
#define VXG_CMPP(TT, EE, CC)                                                                         \
    if (T == TT && epi == EE && ck == CC) {                                                          \
        hipLaunchKernelGGL((cmp_range_patch_kernel<TT, EE, CC>), grid, block, 0, s, p, len,          \
                           static_cast<uint32_t*>(out), out_bit, ep, r.lo_bits, r.hi_bits, rc);      \
        return hip_check(hipGetLastError(), "cmp_range_patch_kernel");                               \
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

vxg_status launch_cmp_range_patch_raw(int ptype, const TakePatches& p, uint64_t len, void* out, uint64_t out_bit,
                                      const CmpRange& r, uint32_t* err, hipStream_t s) {
    if (!range_ops_ok(r.lo_op, r.hi_op)) return set_error(VXG_ERR_INVALID_ARGUMENT, "range compare: bad operators");
    if (p.n == 0) return VXG_OK;
    const int rc = range_code(r.lo_op, r.hi_op);
    const dim3 grid(cmp_grid(p.n)), block(kCmpThreads);
    if (ptype == VXG_F32)
        hipLaunchKernelGGL((cmp_range_patch_raw_kernel<float>), grid, block, 0, s, p, len, static_cast<uint32_t*>(out),
                           out_bit, r.lo_bits, r.hi_bits, rc, err);
    else if (ptype == VXG_F64)
        hipLaunchKernelGGL((cmp_range_patch_raw_kernel<double>), grid, block, 0, s, p, len, static_cast<uint32_t*>(out),
                           out_bit, r.lo_bits, r.hi_bits, rc, err);
    else
        return set_error(VXG_ERR_NOT_IMPLEMENTED, "compare: outer patches are f32 or f64");
    return hip_check(hipGetLastError(), "cmp_range_patch_raw_kernel");
}

vxg_status launch_and_count(const AndInputs& in, void* out, uint64_t n_words, uint64_t* count, hipStream_t s) {
    if (in.k == 0 || in.k > uint32_t(kAndInputs)) return set_error(VXG_ERR_INVALID_ARGUMENT, "combine: 1..16 bitmaps per launch");
    if (n_words == 0) return VXG_OK;
    // memory-bound: at most 2048 workgroups, the rest by grid stride
    const unsigned grid = std::min(cmp_grid(n_words), 2048u);
    if (count)
        hipLaunchKernelGGL(and_count_kernel<true>, dim3(grid), dim3(kCmpThreads), 0, s, in, static_cast<uint64_t*>(out),
                           n_words, count);
    else
        hipLaunchKernelGGL(and_count_kernel<false>, dim3(grid), dim3(kCmpThreads), 0, s, in, static_cast<uint64_t*>(out),
                           n_words, count);
    return hip_check(hipGetLastError(), "and_count_kernel");
}

}  // namespace vxg
