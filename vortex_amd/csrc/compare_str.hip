// compare_str.hip — compute::compare of a string array (utf8 / binary) with a scalar
// (varbin/compute/compare.rs:16-67, varbinview/compute.rs:79, fsst/src/compute.rs:37-97), on the
// compressed forms.  Bytes are compared unsigned and lexicographically, a proper prefix is smaller:
// arrow's order for Utf8 and Binary.
//
//   * Row compare (cmpb_rows_kernel): one wave per bitmap word, lane l = bit l, one ballot, one
//     8-byte store or OR by put_word's rule.  An accessor reads the row where it lies -- VarBin
//     (offsets plain or packed), VarBinView (decided from the view alone wherever its length,
//     inline bytes or prefix suffice), FSST (the row's codes are walked against the scalar with the
//     piece's symbol table in LDS; no heap and no views are written).  For == and != a row whose
//     length differs from the scalar's is decided without touching its bytes.
//   * Dict: the dictionary's VALUES are compared by the row kernel into a truth table (one bit per
//     dictionary entry), then every row is one table lookup: BitPacked codes in the packed domain
//     (compare.hip's walk with the predicate replaced: W bits read, 1 bit written per row), other
//     codes by a plain kernel (one wave per word).
// Unlike the reference's compare_fsst_constant, which compresses the scalar and compares code
// bytes (right only when every row was compressed with the same choices as the scalar, == and !=
// only), FSST rows are compared as decoded bytes: all six operators, any valid code sequence.
#include "compare_str.hpp"

#include "compare_impl.hpp"
#include "intcol.hpp"

namespace vxg {

namespace {

template <int OP>
__device__ __forceinline__ bool ord_op(int ord) {  // ord: sign of (row - scalar)
    if constexpr (OP == VXG_CMP_EQ) return ord == 0;
    else if constexpr (OP == VXG_CMP_NOT_EQ) return ord != 0;
    else if constexpr (OP == VXG_CMP_GT) return ord > 0;
    else if constexpr (OP == VXG_CMP_GTE) return ord >= 0;
    else if constexpr (OP == VXG_CMP_LT) return ord < 0;
    else return ord <= 0;
}
template <int OP>
constexpr bool kEqOnly = OP == VXG_CMP_EQ || OP == VXG_CMP_NOT_EQ;

// The scalar as the row kernels see it: LDS (short) or global memory (long), so a generic pointer.
struct Scalar {
    const uint8_t* p;
    uint64_t len;
};

__device__ __forceinline__ void flag(uint32_t* err, uint32_t bit) {
    __hip_atomic_fetch_or(err, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int64_t ccol_get(const CCol& c, uint64_t i) {  // uniform branches only
    if (c.packed)
        return c.width == 4 ? fl_get<32>(c.p, c.W, c.shift, c.offset, c.reference, c.sgn != 0, i)
                            : fl_get<64>(c.p, c.W, c.shift, c.offset, c.reference, c.sgn != 0, i);
    switch (c.width) {
    case 1: return c.sgn ? ld<1, true>(c.p, i) : ld<1, false>(c.p, i);
    case 2: return c.sgn ? ld<2, true>(c.p, i) : ld<2, false>(c.p, i);
    case 4: return c.sgn ? ld<4, true>(c.p, i) : ld<4, false>(c.p, i);
    default: return ld<8, true>(c.p, i);
    }
}

// Sign of (row bytes - scalar) for a row that lies contiguously in global memory, its first `done`
// bytes already known to equal the scalar's.
__device__ __forceinline__ int cmp_tail(const uint8_t* __restrict__ rp, uint64_t rlen, const Scalar& sc, uint64_t done) {
    const uint64_t m = rlen < sc.len ? rlen : sc.len;
    for (uint64_t k = done; k < m; k++) {
        const uint8_t a = gload(rp + k), b = sc.p[k];
        if (a != b) return a < b ? -1 : 1;
    }
    return rlen < sc.len ? -1 : (rlen > sc.len ? 1 : 0);
}

// ---- accessors: bit of row i of a piece ----------------------------------------------------
struct NoLds {};

template <int OP>
__device__ __forceinline__ bool varbin_row(const uint8_t* bytes, uint64_t bytes_len, const CCol& offs, uint64_t i,
                                           const Scalar& sc, uint32_t* err) {
    const int64_t o0 = ccol_get(offs, i), o1 = ccol_get(offs, i + 1);
    if (o0 < 0 || o1 < o0 || uint64_t(o1) > bytes_len) {
        flag(err, kErrVarBin);
        return false;
    }
    const uint64_t rlen = uint64_t(o1 - o0);
    if (kEqOnly<OP> && rlen != sc.len) return OP == VXG_CMP_NOT_EQ;  // the bytes are not touched
    return ord_op<OP>(cmp_tail(bytes + o0, rlen, sc, 0));
}

struct VbDictAcc {
    using Piece = VbDictPiece;
    using Lds = NoLds;
    static __device__ __forceinline__ uint64_t out_bit(const Piece& p) { return uint64_t(p.out_word) * 64; }
    static __device__ __forceinline__ uint64_t n(const Piece& p) { return p.n; }
    static __device__ __forceinline__ bool excl(const Piece&) { return true; }
    static __device__ __forceinline__ void setup(const Piece&, Lds&) {}
    template <int OP>
    static __device__ __forceinline__ bool row(const Piece& p, const Lds&, uint64_t i, const Scalar& sc, uint32_t* err) {
        CCol c{};
        c.p = p.offs;
        c.width = p.width;
        c.sgn = p.sgn;
        return varbin_row<OP>(p.bytes, p.bytes_len, c, i, sc, err);
    }
};

struct VbAcc {
    using Piece = VbPiece;
    using Lds = NoLds;
    static __device__ __forceinline__ uint64_t out_bit(const Piece& p) { return p.out_bit; }
    static __device__ __forceinline__ uint64_t n(const Piece& p) { return p.n; }
    static __device__ __forceinline__ bool excl(const Piece& p) { return p.excl != 0; }
    static __device__ __forceinline__ void setup(const Piece&, Lds&) {}
    template <int OP>
    static __device__ __forceinline__ bool row(const Piece& p, const Lds&, uint64_t i, const Scalar& sc, uint32_t* err) {
        return varbin_row<OP>(p.bytes, p.bytes_len, p.offs, i, sc, err);
    }
};

// BinaryView (varbinview/mod.rs): u32 size, then 12 inlined bytes, or a 4-byte prefix, u32
// buffer_index and u32 offset.
struct ViewAcc {
    using Piece = ViewPiece;
    using Lds = NoLds;
    static __device__ __forceinline__ uint64_t out_bit(const Piece& p) { return p.out_bit; }
    static __device__ __forceinline__ uint64_t n(const Piece& p) { return p.n; }
    static __device__ __forceinline__ bool excl(const Piece& p) { return p.excl != 0; }
    static __device__ __forceinline__ void setup(const Piece&, Lds&) {}
    template <int OP>
    static __device__ __forceinline__ bool row(const Piece& p, const Lds&, uint64_t i, const Scalar& sc, uint32_t* err) {
        const uint4 v = gload(reinterpret_cast<const uint4*>(p.views) + i);
        const uint64_t rlen = v.x;
        if (kEqOnly<OP> && rlen != sc.len) return OP == VXG_CMP_NOT_EQ;
        // the bytes the view itself holds: the whole row (<= 12) or its prefix
        const uint32_t have = rlen <= 12 ? uint32_t(rlen) : 4u;
        const uint32_t m = uint64_t(have) < sc.len ? have : uint32_t(sc.len);
        for (uint32_t k = 0; k < m; k++) {
            const uint32_t w = k < 4 ? v.y : (k < 8 ? v.z : v.w);
            const uint8_t a = uint8_t(w >> (8 * (k & 3))), b = sc.p[k];
            if (a != b) return ord_op<OP>(a < b ? -1 : 1);
        }
        if (rlen <= 12 || sc.len <= 4) return ord_op<OP>(rlen < sc.len ? -1 : (rlen > sc.len ? 1 : 0));
        // longer than 12 bytes and the prefix ties: the data buffer
        StrBuf b = p.buf0;
        if (v.z >= p.n_buffers) {
            flag(err, kErrVarBin);
            return false;
        }
        if (p.n_buffers > 1) {
            b.p = gload(&p.bufs[v.z].p);
            b.len = gload(&p.bufs[v.z].len);
        }
        if (uint64_t(v.w) + rlen > b.len) {
            flag(err, kErrVarBin);
            return false;
        }
        return ord_op<OP>(cmp_tail(b.p + v.w, rlen, sc, 4));
    }
};

// FSST (fsst/src/array.rs): a row is a run of codes; code c < n_symbols stands for the 1..8
// bytes of symbol c, 255 escapes the next byte as a literal.
struct FsstLds {
    uint64_t sym[256];
    uint8_t len[256];
};
struct FsstAcc {
    using Piece = FsstPiece;
    using Lds = FsstLds;
    static __device__ __forceinline__ uint64_t out_bit(const Piece& p) { return p.out_bit; }
    static __device__ __forceinline__ uint64_t n(const Piece& p) { return p.n; }
    static __device__ __forceinline__ bool excl(const Piece& p) { return p.excl != 0; }
    static __device__ __forceinline__ void setup(const Piece& p, Lds& l) {  // 256 threads, then a barrier
        const uint32_t t = threadIdx.x;
        if (t < p.n_symbols) {
            l.sym[t] = gload(p.symbols + t);
            l.len[t] = gload(p.sym_lens + t);
        }
    }
    template <int OP>
    static __device__ __forceinline__ bool row(const Piece& p, const Lds& l, uint64_t i, const Scalar& sc, uint32_t* err) {
        const int64_t o0 = ccol_get(p.offs, i), o1 = ccol_get(p.offs, i + 1);
        if (o0 < 0 || o1 < o0 || uint64_t(o1) > p.codes_len) {
            flag(err, kErrFsst);
            return false;
        }
        uint64_t ulen = 0;
        if constexpr (kEqOnly<OP>) {
            ulen = uint64_t(ccol_get(p.lens, i));
            if (ulen != sc.len) return OP == VXG_CMP_NOT_EQ;  // most rows of a selective predicate
        }
        uint64_t pos = 0;  // decoded bytes so far, all equal to the scalar's
        for (int64_t c = o0; c < o1;) {
            const uint32_t code = gload(p.codes + c++);
            uint64_t sym;
            uint32_t sl;
            if (code == 255) {
                if (c >= o1) {  // an escape with no byte after it
                    flag(err, kErrFsst);
                    return false;
                }
                sym = gload(p.codes + c++);
                sl = 1;
            } else {
                if (code >= p.n_symbols) {
                    flag(err, kErrFsst);
                    return false;
                }
                sym = l.sym[code];
                sl = l.len[code];
                sl = sl > 8 ? 8 : sl;
            }
            for (uint32_t k = 0; k < sl; k++) {
                if (pos >= sc.len) return ord_op<OP>(1);  // the scalar is a proper prefix of the row
                const uint8_t a = uint8_t(sym >> (8 * k)), b = sc.p[pos];
                if (a != b) return ord_op<OP>(a < b ? -1 : 1);
                pos++;
            }
        }
        if constexpr (kEqOnly<OP>) {
            if (pos != ulen) {  // the codes do not decode to uncompressed_lengths
                flag(err, kErrFsst);
                return false;
            }
        }
        return ord_op<OP>(pos < sc.len ? -1 : 0);
    }
};

template <class ACC, int OP>
__device__ __forceinline__ void rows_body(const typename ACC::Piece& p, const typename ACC::Lds& lds, uint32_t g,
                                          const Scalar& sc, uint64_t* __restrict__ out, uint32_t* err) {
    const uint32_t l = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t n = ACC::n(p);
    const int64_t cb = int64_t(ACC::out_bit(p)), ce = cb + int64_t(n);
    const int64_t first = cb >> 6, n_words = ((ce + 63) >> 6) - first;
    const bool excl = ACC::excl(p);
    const int64_t w0 = int64_t(g - p.first_group) * kStrWordsPerGroup;
    for (uint32_t r = 0; r < kStrWordsPerGroup / (kCmpThreads / 64); r++) {
        const int64_t w = w0 + int64_t(r * (kCmpThreads / 64) + wave);  // wave-uniform
        if (w >= n_words) break;
        const int64_t i = (first + w) * 64 + int64_t(l) - cb;
        const bool in_range = i >= 0 && uint64_t(i) < n;
        const bool pr = in_range && ACC::template row<OP>(p, lds, uint64_t(i), sc, err);
        const uint64_t bal = __ballot(pr);
        if (l == 0) put_word(out, first + w, bal, true, excl, cb, ce);
    }
}

template <class ACC, class TAB>
__global__ __launch_bounds__(kCmpThreads) void cmpb_rows_kernel(TAB tab, StrScalar ss, uint64_t* __restrict__ out,
                                                                uint32_t* err, int op) {
    __shared__ uint64_t s_scalar[kStrInline / 8];
    __shared__ typename ACC::Lds s_acc;
    const uint32_t g = blockIdx.x;
    const typename ACC::Piece& p = tab.c[cmp_table_index(tab, g)];
    if (threadIdx.x == 0) {
#pragma unroll
        for (uint32_t k = 0; k < kStrInline / 8; k++) s_scalar[k] = ss.inl[k];
    }
    ACC::setup(p, s_acc);
    __syncthreads();
    Scalar sc;
    sc.len = ss.len;
    sc.p = ss.len <= kStrInline ? reinterpret_cast<const uint8_t*>(s_scalar) : ss.dev;
    switch (op) {  // uniform: one straight-line body per operator
    case VXG_CMP_EQ: rows_body<ACC, VXG_CMP_EQ>(p, s_acc, g, sc, out, err); break;
    case VXG_CMP_NOT_EQ: rows_body<ACC, VXG_CMP_NOT_EQ>(p, s_acc, g, sc, out, err); break;
    case VXG_CMP_GT: rows_body<ACC, VXG_CMP_GT>(p, s_acc, g, sc, out, err); break;
    case VXG_CMP_GTE: rows_body<ACC, VXG_CMP_GTE>(p, s_acc, g, sc, out, err); break;
    case VXG_CMP_LT: rows_body<ACC, VXG_CMP_LT>(p, s_acc, g, sc, out, err); break;
    default: rows_body<ACC, VXG_CMP_LTE>(p, s_acc, g, sc, out, err); break;
    }
}

// ---- Dict lookups ----------------------------------------------------------------------------
__global__ __launch_bounds__(kCmpThreads) void cmpb_dict_plain_kernel(DictPlainTab tab, uint64_t* __restrict__ out,
                                                                      const uint32_t* __restrict__ tt, uint32_t* err) {
    const uint32_t g = blockIdx.x, l = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const DictPlainPiece& p = tab.c[cmp_table_index(tab, g)];
    const int64_t cb = int64_t(p.out_bit), ce = cb + int64_t(p.n);
    const int64_t first = cb >> 6, n_words = ((ce + 63) >> 6) - first;
    const uint32_t* __restrict__ t32 = tt + 2ull * p.tword;
    const int64_t w0 = int64_t(g - p.first_group) * kStrWordsPerGroup;
    for (uint32_t r = 0; r < kStrWordsPerGroup / (kCmpThreads / 64); r++) {
        const int64_t w = w0 + int64_t(r * (kCmpThreads / 64) + wave);
        if (w >= n_words) break;
        const int64_t i = (first + w) * 64 + int64_t(l) - cb;
        bool pr = false;
        if (i >= 0 && uint64_t(i) < p.n) {
            int64_t c;
            switch (p.width) {  // uniform
            case 1: c = p.sgn ? ld<1, true>(p.codes, uint64_t(i)) : ld<1, false>(p.codes, uint64_t(i)); break;
            case 2: c = p.sgn ? ld<2, true>(p.codes, uint64_t(i)) : ld<2, false>(p.codes, uint64_t(i)); break;
            case 4: c = p.sgn ? ld<4, true>(p.codes, uint64_t(i)) : ld<4, false>(p.codes, uint64_t(i)); break;
            default: c = ld<8, true>(p.codes, uint64_t(i)); break;
            }
            if (uint64_t(c) < uint64_t(p.vlen)) pr = (gload(t32 + (uint32_t(c) >> 5)) >> (uint32_t(c) & 31)) & 1u;
            else flag(err, kErrTakeOOB);
        }
        const uint64_t bal = __ballot(pr);
        if (l == 0) put_word(out, first + w, bal, true, p.excl != 0, cb, ce);
    }
}

// The predicate of cmp_blocks for Dict codes: a truth-table bit; a code past the dictionary is
// reported (kErrTakeOOB) when its position is a row of the chunk, and its bit is 0.
template <int T, bool LDS>
struct DictPred {
    using E = typename Fl<T>::E;
    static constexpr bool kChecks = true;
    const uint32_t* tab;  // LDS or global
    uint64_t vlen;
    uint32_t* err;
    bool bad;
    __device__ __forceinline__ bool test(E raw) {
        const uint64_t c = uint64_t(raw);
        bad = c >= vlen;
        const uint32_t i = bad ? 0u : uint32_t(c);
        const uint32_t w = LDS ? lds_load(tab + (i >> 5)) : gload(tab + (i >> 5));
        return !bad && ((w >> (i & 31)) & 1u);
    }
    __device__ __forceinline__ void check(bool in_range) const {
        if (bad && in_range) flag(err, kErrTakeOOB);
    }
};

template <int T>
__global__ __launch_bounds__(kCmpThreads) void cmpb_dict_packed_kernel(CmpTable tab, uint64_t* __restrict__ out,
                                                                       const uint32_t* __restrict__ tt, uint32_t* err,
                                                                       uint32_t tt_lds_off) {
    extern __shared__ __attribute__((aligned(16))) uint8_t cmpb_lds[];
    const uint32_t g = blockIdx.x;
    const CmpChunk& c = tab.c[cmp_table_index(tab, g)];
    const uint32_t vlen = uint32_t(c.reference >> 32);
    const uint32_t* __restrict__ t32 = tt + 2ull * uint32_t(c.reference);
    if (vlen <= kDictLdsBits) {  // uniform
        uint32_t* s_tt = reinterpret_cast<uint32_t*>(cmpb_lds + tt_lds_off);
        for (uint32_t k = threadIdx.x; k < (vlen + 31) / 32; k += kCmpThreads) s_tt[k] = gload(t32 + k);
        // (cmp_blocks' barrier, after its own staging, covers these stores)
        cmp_blocks<T>(c, g, out, cmpb_lds, [&] { return DictPred<T, true>{s_tt, vlen, err, false}; });
    } else {
        cmp_blocks<T>(c, g, out, cmpb_lds, [&] { return DictPred<T, false>{t32, vlen, err, false}; });
    }
}

template <class ACC, class TAB>
vxg_status rows_launch(const TAB& t, uint64_t groups, const StrScalar& sc, void* out, uint32_t* err, int op, hipStream_t s,
                       const char* what) {
    if (t.n == 0 || groups == 0) return VXG_OK;
    if (groups > 0x7FFFFFFFull) return set_error(VXG_ERR_INVALID_ARGUMENT, "compare: bad launch shape");
    hipLaunchKernelGGL((cmpb_rows_kernel<ACC, TAB>), dim3(unsigned(groups)), dim3(kCmpThreads), 0, s, t, sc,
                       static_cast<uint64_t*>(out), err, op);
    return hip_check(hipGetLastError(), what);
}

}  // namespace

vxg_status launch_cmpb_varbin_dict(const VbDictTab& t, uint64_t groups, const StrScalar& sc, void* out, uint32_t* err,
                                   int op, hipStream_t s) {
    return rows_launch<VbDictAcc>(t, groups, sc, out, err, op, s, "cmpb_rows_kernel (VarBin dictionaries)");
}
vxg_status launch_cmpb_varbin(const VbTab& t, uint64_t groups, const StrScalar& sc, void* out, uint32_t* err, int op,
                              hipStream_t s) {
    return rows_launch<VbAcc>(t, groups, sc, out, err, op, s, "cmpb_rows_kernel (VarBin)");
}
vxg_status launch_cmpb_views(const ViewTab& t, uint64_t groups, const StrScalar& sc, void* out, uint32_t* err, int op,
                             hipStream_t s) {
    return rows_launch<ViewAcc>(t, groups, sc, out, err, op, s, "cmpb_rows_kernel (VarBinView)");
}
vxg_status launch_cmpb_fsst(const FsstTab& t, uint64_t groups, const StrScalar& sc, void* out, uint32_t* err, int op,
                            hipStream_t s) {
    return rows_launch<FsstAcc>(t, groups, sc, out, err, op, s, "cmpb_rows_kernel (FSST)");
}

vxg_status launch_cmpb_dict_plain(const DictPlainTab& t, uint64_t groups, void* out, const void* tt, uint32_t* err,
                                  hipStream_t s) {
    if (t.n == 0 || groups == 0) return VXG_OK;
    if (groups > 0x7FFFFFFFull) return set_error(VXG_ERR_INVALID_ARGUMENT, "compare: bad launch shape");
    hipLaunchKernelGGL(cmpb_dict_plain_kernel, dim3(unsigned(groups)), dim3(kCmpThreads), 0, s, t,
                       static_cast<uint64_t*>(out), static_cast<const uint32_t*>(tt), err);
    return hip_check(hipGetLastError(), "cmpb_dict_plain_kernel");
}

vxg_status launch_cmpb_dict_packed(int T, const CmpTable& tab, uint64_t groups, uint32_t lds_bytes, void* out,
                                   const void* tt, uint32_t* err, hipStream_t s) {
    const uint32_t tt_off = (lds_bytes + 15u) & ~15u, total = tt_off + kDictLdsBits / 8;
    if (groups == 0 || groups > 0x7FFFFFFFull || total > 64 * 1024)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "compare: bad launch shape");
#define VXG_CMPB(TT)                                                                                              \
    case TT:                                                                                                      \
        hipLaunchKernelGGL((cmpb_dict_packed_kernel<TT>), dim3(unsigned(groups)), dim3(kCmpThreads), total, s, tab, \
                           static_cast<uint64_t*>(out), static_cast<const uint32_t*>(tt), err, tt_off);           \
        break;
    switch (T) {
        VXG_CMPB(8) VXG_CMPB(16) VXG_CMPB(32) VXG_CMPB(64)
    default: return set_error(VXG_ERR_NOT_IMPLEMENTED, "compare: unsupported codes width");
    }
#undef VXG_CMPB
    return hip_check(hipGetLastError(), "cmpb_dict_packed_kernel");
}

}  // namespace vxg
