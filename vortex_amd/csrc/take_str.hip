// take_str.hip — compute::take of string arrays (utf8 / binary) on their compressed forms.
//
// Reference: varbin/compute/take.rs:11-83 appends the taken rows to a VarBinBuilder (a null row as
// an empty value), fsst/src/compute.rs:114-126 takes the codes and lengths, dict/compute.rs:44-52
// takes the codes; whatever the route, the canonical of the result (varbin/flatten.rs) is one heap
// of the taken rows' bytes in index order with views over it.  The GPU builds exactly that:
//   * VarBinView, Dict values and the fallback: take_views gathers 16-byte views at the indices
//     (or at the taken Dict codes), then filter.hip's heap rebuild copies each row's bytes;
//   * VarBin: take_varbin_views writes a source view per taken row over the array's own bytes
//     (offsets read in place, plain or packed), then the same heap rebuild;
//   * FSST: only the taken rows are decoded.  Sizing needs no decode (uncompressed_lengths at the
//     indices, summed per 1024-row tile, one scan); the decode kernel stages the symbol table in
//     LDS once per workgroup and gives every taken row to ONE LANE, which walks its codes and
//     writes bytes and the final view.  One lane per row, not one wave per row: a row's walk is a
//     dependent chain (each code's output position follows from the lengths before it), so 64 lanes
//     on one row would wait on one chain, while 64 rows per wave keep 64 chains in flight; string
//     columns hold rows of tens of bytes, far below what 64 lanes need to share a row usefully.
//     The cost is divergence: a wave runs as long as its longest row.  Lane l of round r takes row
//     tile * 1024 + r * 256 + l, so indices are read and views are written coalesced.
#include "take_str.hpp"

#include "filter.hpp"
#include "intcol.hpp"

namespace vxg {

namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kRounds = int(kTakeStrTileRows) / kThreads;

__device__ __forceinline__ void flag(uint32_t* err, uint32_t bit) {
    __hip_atomic_fetch_or(err, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint64_t ld_idx(const void* p, int width, bool sgn, uint64_t i) {
    switch (width) {  // uniform
    case 1: return uint64_t(sgn ? ld<1, true>(p, i) : ld<1, false>(p, i));
    case 2: return uint64_t(sgn ? ld<2, true>(p, i) : ld<2, false>(p, i));
    case 4: return uint64_t(sgn ? ld<4, true>(p, i) : ld<4, false>(p, i));
    default: return uint64_t(ld<8, true>(p, i));
    }
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

__device__ __forceinline__ bool is_null(const uint8_t* valid, uint64_t j) {
    return valid && !((gload(valid + (j >> 3)) >> (j & 7)) & 1u);
}

__device__ __forceinline__ uint64_t wave_incl_scan(uint64_t v, int lane) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint64_t o = __shfl_up(v, d, kWave);
        if (lane >= d) v += o;
    }
    return v;
}

__global__ __launch_bounds__(kThreads) void take_views_kernel(const uint4* __restrict__ src, uint64_t n_src,
                                                              const void* __restrict__ codes, int cw, bool csg, uint64_t n,
                                                              TakeIdx guard, const StrBuf* __restrict__ bufs,
                                                              uint32_t n_bufs, const uint8_t* __restrict__ valid,
                                                              uint4* __restrict__ out, uint32_t* err) {
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t j = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; j < n; j += stride) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (!is_null(valid, j)) {
            if (guard.idx && ld_idx(guard.idx, guard.iw, guard.isg != 0, j) >= guard.len) {
                flag(err, kErrTakeOOB);
            } else {
                const uint64_t c = ld_idx(codes, cw, csg, j);
                if (c >= n_src) {
                    flag(err, kErrTakeOOB);
                } else {
                    v = gload(src + c);
                    if (bufs && v.x > 12u && (v.z >= n_bufs || uint64_t(v.w) + v.x > gload(&bufs[v.z].len))) {
                        flag(err, kErrVarBin);
                        v = make_uint4(0u, 0u, 0u, 0u);
                    }
                }
            }
        }
        out[j] = v;
    }
}

// VarBin, step 1: a record per taken row -- {length, 0, 0, offset into the array's bytes}, all zero
// for a null, out-of-bounds or malformed row.  The bytes are not touched here: step 2 reads them once.
__global__ __launch_bounds__(kThreads) void take_varbin_rows_kernel(TakeIdx t, CCol offs, uint64_t bytes_len,
                                                                    const uint8_t* __restrict__ valid,
                                                                    uint4* __restrict__ out, uint32_t* err) {
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t j = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; j < t.n; j += stride) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (!is_null(valid, j)) {
            const uint64_t i = ld_idx(t.idx, t.iw, t.isg != 0, j);
            if (i >= t.len) {
                flag(err, kErrTakeOOB);
            } else {
                const int64_t o0 = ccol_get(offs, i), o1 = ccol_get(offs, i + 1);
                if (o0 < 0 || o1 < o0 || uint64_t(o1) > bytes_len) {
                    flag(err, kErrVarBin);
                } else {
                    v.x = uint32_t(o1 - o0);  // bytes_len < 2^32
                    v.w = o1 > o0 ? uint32_t(o0) : 0u;  // (an empty row's record is its final, all-zero view)
                }
            }
        }
        out[j] = v;
    }
}

// VarBin, step 2: filter.hip's heap-build tiling (a 4096-row tile per workgroup, 16 consecutive rows
// per thread, heap_off from launch_view_heap_sizes over the records) -- each row's bytes are copied
// from the array's own bytes to the new heap and its final view is made from the bytes just read.
constexpr int kBuildRowsPerThread = int(kFilterTileRows) / kThreads;

__global__ __launch_bounds__(kThreads) void take_varbin_build_kernel(uint4* __restrict__ views, uint64_t n,
                                                                     const uint64_t* __restrict__ heap_off,
                                                                     const uint8_t* __restrict__ bytes,
                                                                     uint8_t* __restrict__ heap) {
    __shared__ uint64_t part[kThreads / kWave];
    const int tid = threadIdx.x, lane = tid % kWave, wv = tid / kWave;
    const uint64_t r0 = uint64_t(blockIdx.x) * kFilterTileRows + uint64_t(tid) * kBuildRowsPerThread;
    uint64_t s = 0;
    for (int k = 0; k < kBuildRowsPerThread; ++k)
        if (r0 + k < n) s += gload(reinterpret_cast<const uint32_t*>(views + r0 + k));
    const uint64_t incl = wave_incl_scan(s, lane);
    if (lane == kWave - 1) part[wv] = incl;
    __syncthreads();
    uint64_t off = gload(heap_off + blockIdx.x) + incl - s;
    for (int i = 0; i < wv; ++i) off += part[i];
    for (int k = 0; k < kBuildRowsPerThread; ++k) {
        const uint64_t r = r0 + k;
        if (r >= n) break;
        uint4 v = gload(views + r);
        const uint32_t len = v.x;
        if (len == 0u) continue;  // (the record is already the all-zero view)
        const uint8_t* __restrict__ src = bytes + v.w;
        uint8_t* __restrict__ dst = heap + off;
        uint64_t lo = 0;  // the first 12 bytes: the inline view, or its prefix
        uint32_t hi = 0;
        uint32_t j = 0;
        for (; j + 8 <= len; j += 8) {
            uint64_t x;
            __builtin_memcpy(&x, src + j, 8);
            __builtin_memcpy(dst + j, &x, 8);
            if (j == 0) lo = x;
            if (j == 8) hi = uint32_t(x);
        }
        for (; j < len; ++j) {
            const uint8_t b = src[j];
            dst[j] = b;
            if (j < 8) lo |= uint64_t(b) << (8 * j);
            else if (j < 12) hi |= uint32_t(b) << (8 * (j - 8));
        }
        v.y = uint32_t(lo);
        if (len <= 12u) {
            v.z = uint32_t(lo >> 32);
            v.w = len > 8u ? hi : 0u;
        } else {
            v.z = 0u;
            v.w = uint32_t(off);
        }
        views[r] = v;
        off += len;
    }
}

// Bytes of taken row j (0 for a row past n, a null row, an index out of bounds or a length outside
// u32); *i its source row, *live: the row's codes are to be walked.
__device__ __forceinline__ uint32_t fsst_row_len(const TakeFsst& f, uint64_t j, uint64_t* i, bool* live, uint32_t* err) {
    *live = false;
    *i = 0;
    if (j >= f.t.n || is_null(f.valid, j)) return 0u;
    const uint64_t r = ld_idx(f.t.idx, f.t.iw, f.t.isg != 0, j);
    if (r >= f.t.len) {
        flag(err, kErrTakeOOB);
        return 0u;
    }
    const int64_t l = ccol_get(f.lens, r);
    if (l < 0 || l > int64_t(0xFFFFFFFFll)) {
        flag(err, kErrFsst);
        return 0u;
    }
    *i = r;
    *live = true;
    return uint32_t(l);
}

__global__ __launch_bounds__(kThreads) void take_fsst_sizes_kernel(TakeFsst f, uint64_t* __restrict__ tile_off,
                                                                   uint32_t* err) {
    __shared__ uint64_t part[kThreads / kWave];
    const int tid = threadIdx.x, lane = tid % kWave;
    uint64_t s = 0;
    for (int r = 0; r < kRounds; r++) {
        uint64_t i;
        bool live;
        s += fsst_row_len(f, uint64_t(blockIdx.x) * kTakeStrTileRows + uint64_t(r * kThreads + tid), &i, &live, err);
    }
    s = wave_incl_scan(s, lane);
    if (lane == kWave - 1) part[tid / kWave] = s;
    __syncthreads();
    if (tid == 0) {
        uint64_t tot = 0;
        for (int k = 0; k < kThreads / kWave; k++) tot += part[k];
        tile_off[blockIdx.x] = tot;
    }
}

__global__ __launch_bounds__(kThreads) void take_fsst_decode_kernel(TakeFsst f, const uint64_t* __restrict__ tile_off,
                                                                    uint8_t* __restrict__ heap, uint4* __restrict__ views,
                                                                    uint32_t* err) {
    __shared__ uint64_t s_sym[256];
    __shared__ uint8_t s_len[256];
    __shared__ uint64_t part[kRounds][kThreads / kWave];
    const int tid = threadIdx.x, lane = tid % kWave, wv = tid / kWave;
    if (uint32_t(tid) < f.n_symbols) {  // n_symbols <= 255
        s_sym[tid] = gload(f.symbols + tid);
        s_len[tid] = gload(f.sym_lens + tid);
    }
    uint64_t run = gload(tile_off + blockIdx.x);
    for (int r = 0; r < kRounds; r++) {  // every thread takes every round: the barrier is uniform
        const uint64_t j = uint64_t(blockIdx.x) * kTakeStrTileRows + uint64_t(r * kThreads + tid);
        uint64_t i;
        bool live;
        const uint32_t len = fsst_row_len(f, j, &i, &live, err);
        const uint64_t incl = wave_incl_scan(len, lane);
        if (lane == kWave - 1) part[r][wv] = incl;
        __syncthreads();  // (round 0: also the symbol table's)
        uint64_t off = run + incl - len;
        for (int k = 0; k < kThreads / kWave; k++) {
            const uint64_t p = part[r][k];
            if (k < wv) off += p;
            run += p;
        }
        if (j >= f.t.n) continue;
        uint64_t lo = 0;   // the row's first 12 bytes: the inline view, or its prefix
        uint32_t hi = 0;
        if (live) {
            bool bad = false;
            uint64_t pos = 0;
            const int64_t o0 = ccol_get(f.offs, i), o1 = ccol_get(f.offs, i + 1);
            if (o0 < 0 || o1 < o0 || uint64_t(o1) > f.codes_len) {  // before any code is read
                bad = true;
                pos = len;
            } else {
                uint8_t* __restrict__ dst = heap + off;
                for (int64_t c = o0; c < o1;) {
                    const uint32_t code = gload(f.codes + c++);
                    uint64_t sym;
                    uint32_t sl;
                    if (code == 255u) {
                        if (c >= o1) {  // an escape with no byte after it
                            bad = true;
                            break;
                        }
                        sym = gload(f.codes + c++);
                        sl = 1u;
                    } else {
                        if (code >= f.n_symbols) {
                            bad = true;
                            break;
                        }
                        sym = s_sym[code];
                        sl = s_len[code];
                        sl = sl > 8u ? 8u : sl;
                    }
                    if (pos + 8 <= uint64_t(len)) {
                        // all 8 bytes lie in the row's slot: one store, the symbols after this one
                        // overwrite the bytes past sl
                        __builtin_memcpy(dst + pos, &sym, 8);
                    } else {
                        for (uint32_t k = 0; k < sl; k++)
                            if (pos + k < uint64_t(len)) dst[pos + k] = uint8_t(sym >> (8 * k));
                    }
                    if (pos < 12) {
                        const uint64_t m = sl >= 8u ? sym : (sym & ((1ull << (8 * sl)) - 1ull));
                        if (pos < 8) {
                            lo |= m << (8 * pos);
                            if (pos > 0 && pos + sl > 8) hi |= uint32_t(m >> (8 * (8 - pos)));
                        } else {
                            hi |= uint32_t(m << (8 * (pos - 8)));
                        }
                    }
                    pos += sl;
                }
            }
            if (bad || pos != uint64_t(len)) flag(err, kErrFsst);  // the codes do not decode to uncompressed_lengths
        }
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (len != 0u) {
            v.x = len;
            v.y = uint32_t(lo);
            if (len <= 12u) {
                // (a well-formed row decodes to exactly len bytes: the bytes past it stay zero)
                v.z = uint32_t(lo >> 32);
                v.w = hi;
            } else {
                v.w = uint32_t(off);  // heap <= 2^32 - 1
            }
        }
        views[j] = v;
    }
}

unsigned grid_for(uint64_t n) {
    const uint64_t g = (n + kThreads - 1) / kThreads;
    return unsigned(g > 65536 ? 65536 : (g ? g : 1));
}

}  // namespace

vxg_status launch_take_views(const uint8_t* src, uint64_t n_src, const void* codes, int cw, bool csg, uint64_t n,
                             const TakeIdx& guard, const StrBuf* bufs, uint32_t n_bufs, const uint8_t* valid,
                             uint8_t* out, uint32_t* err, hipStream_t s) {
    if (n == 0) return VXG_OK;
    if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(out)) & 15)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "take: views must be 16-byte aligned");
    hipLaunchKernelGGL(take_views_kernel, dim3(grid_for(n)), dim3(kThreads), 0, s, reinterpret_cast<const uint4*>(src),
                       n_src, codes, cw, csg, n, guard, bufs, n_bufs, valid, reinterpret_cast<uint4*>(out), err);
    return hip_check(hipGetLastError(), "take_views_kernel");
}

vxg_status launch_take_varbin_rows(const TakeIdx& t, const CCol& offs, uint64_t bytes_len, const uint8_t* valid,
                                   uint8_t* out, uint32_t* err, hipStream_t s) {
    if (t.n == 0) return VXG_OK;
    if (bytes_len > 0xFFFFFFFFull) return set_error(VXG_ERR_INVALID_ARGUMENT, "take: VarBin bytes exceed u32 view offsets");
    if (reinterpret_cast<uintptr_t>(out) & 15)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "take: views must be 16-byte aligned");
    hipLaunchKernelGGL(take_varbin_rows_kernel, dim3(grid_for(t.n)), dim3(kThreads), 0, s, t, offs, bytes_len, valid,
                       reinterpret_cast<uint4*>(out), err);
    return hip_check(hipGetLastError(), "take_varbin_rows_kernel");
}

vxg_status launch_take_varbin_build(uint8_t* views, uint64_t n, const uint64_t* heap_off, const uint8_t* bytes,
                                    uint8_t* heap, hipStream_t s) {
    const uint64_t tiles = filter_tiles(n);
    if (!tiles) return VXG_OK;
    if (tiles > 0x7FFFFFFFull) return set_error(VXG_ERR_INVALID_ARGUMENT, "take: too many indices");
    hipLaunchKernelGGL(take_varbin_build_kernel, dim3(unsigned(tiles)), dim3(kThreads), 0, s,
                       reinterpret_cast<uint4*>(views), n, heap_off, bytes, heap);
    return hip_check(hipGetLastError(), "take_varbin_build_kernel");
}

vxg_status launch_take_fsst_sizes(const TakeFsst& f, uint64_t* tile_off, uint32_t* err, hipStream_t s) {
    const uint64_t tiles = take_str_tiles(f.t.n);
    if (tiles > 0x7FFFFFFFull) return set_error(VXG_ERR_INVALID_ARGUMENT, "take: too many indices");
    if (tiles) {
        hipLaunchKernelGGL(take_fsst_sizes_kernel, dim3(unsigned(tiles)), dim3(kThreads), 0, s, f, tile_off, err);
        if (vxg_status st = hip_check(hipGetLastError(), "take_fsst_sizes_kernel"); st != VXG_OK) return st;
    }
    return launch_scan_tiles(tile_off, tiles, s);
}

vxg_status launch_take_fsst_decode(const TakeFsst& f, const uint64_t* tile_off, uint8_t* heap, uint8_t* views,
                                   uint32_t* err, hipStream_t s) {
    const uint64_t tiles = take_str_tiles(f.t.n);
    if (!tiles) return VXG_OK;
    if (tiles > 0x7FFFFFFFull) return set_error(VXG_ERR_INVALID_ARGUMENT, "take: too many indices");
    if (f.n_symbols > 255u) return set_error(VXG_ERR_INVALID_ARGUMENT, "FSST symbol table > 255 entries");
    if (reinterpret_cast<uintptr_t>(views) & 15)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "take: views must be 16-byte aligned");
    hipLaunchKernelGGL(take_fsst_decode_kernel, dim3(unsigned(tiles)), dim3(kThreads), 0, s, f, tile_off, heap,
                       reinterpret_cast<uint4*>(views), err);
    return hip_check(hipGetLastError(), "take_fsst_decode_kernel");
}

}  // namespace vxg
