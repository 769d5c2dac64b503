// filter_packed.hip — K22: compute::filter of BitPacked-rooted cascades in the packed domain, for a
// batch whose row mask was counted and scanned once (Planner::filter_batch; the scan's
// filter(batch, mask), vortex-serde layouts/read/stream.rs:143-149 over array/struct_/compute.rs:
// 80-99).  Canonicalize-then-compact writes T bits per row into a temporary and reads them back;
// here the W packed bits are read and only the selected rows are written:
//   * a workgroup stages the packed words of `bpw` consecutive FastLanes blocks of one chunk into
//     LDS exactly as the compare does (cmp_blocks, compare_impl.hpp): 16-byte loads, every packed
//     byte read once;
//   * a wave takes whole blocks.  In step m (0..15) lane l extracts packed position 64 m + j of the
//     block, j = (l - d) mod 64 with d = the column row of the block's position 0 mod 64 -- the
//     compare's rotation -- so the row's mask bit is bit l of its mask word: the step covers bits
//     >= d of mask word A and bits < d of word A + 1, in row order;
//   * the value is apply_epi's (fl_unpack_impl.hpp), the arithmetic of canonicalize;
//   * row r goes to slot tile_off[r / 4096] + popcount(the tile's mask words before r's word) +
//     popcount(word & lanes below l).  The per-word bases are a wave scan of the tile's 64 words
//     (tile_words, filter_impl.hpp), kept in registers while the wave's blocks stay in the tile and
//     moved into lanes 0..16 once per block (the 17 words a block touches), so a step reads them
//     with readlane.  No atomics: every slot has exactly one writer;
//   * a step whose 64 mask bits are zero unpacks nothing, and a block with no set bit runs no step.
//     (The block is still staged: staging is the workgroup's, decided before the mask is read.)
// Patched rows are rewritten afterwards (patch kernels: one thread per patch finds its row's slot
// by counting the tile's words before it).  Primitive buffers are compacted by the range kernel,
// the plain filter kernel over a row range of the column (a chunk's first row falls anywhere).
#include "compare_impl.hpp"
#include "filter_impl.hpp"
#include "filter_packed.hpp"

namespace vxg {

namespace {

// The words of tile t (a signed index: the rows before a sliced chunk's first one may lie before
// row 0) and their output bases; outside the mask every word is 0.
__device__ __forceinline__ TileWords filt_tile(const FiltMask& fm, int64_t t, int lane) {
    if (t < 0 || uint64_t(t) * kFilterTileRows >= fm.n) return TileWords{0, 0};  // uniform
    return tile_words(fm.mask, fm.n, fm.tile_off, uint64_t(t), lane);
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
    const uint32_t lo = uint32_t(__shfl(int(uint32_t(v)), src, kWave));
    const uint32_t hi = uint32_t(__shfl(int(uint32_t(v >> 32)), src, kWave));
    return (uint64_t(hi) << 32) | lo;
}

template <int T, Epi EPI>
__global__ __launch_bounds__(kCmpThreads) void filter_packed_kernel(CmpTable tab, FiltMask fm,
                                                                    typename EpiOut<T, EPI, 0>::type* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t filt_lds[];
    using E = typename Fl<T>::E;
    using O = typename EpiOut<T, EPI, 0>::type;
    constexpr uint32_t LANES = 1024 / T;
    constexpr uint32_t LT = T == 64 ? 6 : (T == 32 ? 5 : (T == 16 ? 4 : 3));
    const uint32_t g = blockIdx.x;
    const CmpChunk& c = tab.c[cmp_table_index(tab, g)];  // the kernel argument: scalar loads
    const uint32_t W = c.W, bpw = c.bpw(), offset = c.offset, tid = threadIdx.x, wave = tid >> 6, l = tid & 63;
    const uint64_t len = c.len(), n_blocks = c.n_blocks();
    const uint64_t blk0 = uint64_t(g - c.first_group) * bpw;
    if (blk0 >= n_blocks) return;  // workgroup-uniform
    const uint32_t nb = uint32_t(n_blocks - blk0 < uint64_t(bpw) ? n_blocks - blk0 : uint64_t(bpw));
    E* const s_packed = reinterpret_cast<E*>(filt_lds);
    const uint32_t q16 = nb * 8 * W;
    for (uint32_t q = tid; q < q16; q += kCmpThreads)
        reinterpret_cast<uint4*>(s_packed)[q] = gload(reinterpret_cast<const uint4*>(c.packed + blk0 * (128ull * W)) + q);
    __syncthreads();

    EpiParams ep{};
    ep.reference = c.reference;
    ep.shift = c.shift;
    alp_factors<EPI>(c.alp_e, c.alp_f, ep.alp_a, ep.alp_b);

    const int64_t base = int64_t(c.out_bit) - int64_t(offset);  // column row of packed position 0
    const uint32_t d = uint32_t(uint64_t(base) & 63u);
    const uint32_t j = (l - d) & 63u;
    // packed position 64 m + j of a block: its lane's word index and the bit offset of its row,
    // for even and odd m (cmp_blocks' arithmetic)
    uint32_t lane_x[2], start_x[2];
#pragma unroll
    for (uint32_t x = 0; x < 2; x++) {
        const uint32_t idx = 64 * x + j;
        lane_x[x] = idx % LANES;
        const uint32_t fl = (idx - lane_x[x]) >> 4;
        start_x[x] = __umul24((((fl & 1) << 2) | (fl & 2) | (fl >> 2)) * 8, W);  // FL_ORDER[fl] * 8 * W
    }
    const E vmask = W >= uint32_t(T) ? E(~E(0)) : E((E(1) << W) - E(1));
    const uint64_t low = d ? (1ull << d) - 1ull : 0ull;  // bits of a step that lie in its second mask word
    const uint64_t below = lanes_below(int(l));
    const bool second = l < d;  // this lane's rows lie in the step's second word

    const uint32_t per = (nb + kCmpThreads / 64 - 1) / (kCmpThreads / 64);
    const uint32_t b_begin = wave * per, b_end = b_begin + per < nb ? b_begin + per : nb;
    // the tiles held in registers: tile t0 in tw0 and, once a block reaches into it, t0 + 1 in tw1
    int64_t t0 = 0;
    bool have0 = false, have1 = false;  // uniform
    TileWords tw0{0, 0}, tw1{0, 0};
    for (uint32_t b = b_begin; b < b_end; b++) {  // wave-uniform
        const E* __restrict__ pw = s_packed + b * (LANES * W);
        const uint64_t p0 = (blk0 + b) * 1024;  // packed position of the block's first value
        const bool full = p0 >= offset && p0 + 1024 <= uint64_t(offset) + len;
        const int64_t gw0 = (base + int64_t(p0)) >> 6;  // mask word of step 0's first part (floor: may be negative)
        const int64_t t = gw0 >> 6;
        if (!have0 || t != t0) {
            if (have0 && have1 && t == t0 + 1) {
                tw0 = tw1;
            } else {
                tw0 = filt_tile(fm, t, int(l));
            }
            t0 = t;
            have0 = true;
            have1 = false;
        }
        const uint32_t i0 = uint32_t(uint64_t(gw0) & 63u);
        if (i0 + 16 >= 64 && !have1) {
            tw1 = filt_tile(fm, t0 + 1, int(l));
            have1 = true;
        }
        // lane i (0..16) takes word gw0 + i of the mask and its base
        const uint32_t wi = i0 + l;
        uint64_t wm = shfl64(tw0.m, int(wi & 63u)), wb = shfl64(tw0.base, int(wi & 63u));
        if (have1) {  // uniform
            const uint64_t m1 = shfl64(tw1.m, int(wi & 63u)), b1 = shfl64(tw1.base, int(wi & 63u));
            if (wi >= 64) {
                wm = m1;
                wb = b1;
            }
        } else if (wi >= 64) {
            wm = 0;
        }
        // the block's rows: bits >= d of word 0, words 1..15, bits < d of word 16
        const uint64_t mine = l == 0 ? ~low : (l < 16 ? ~0ull : (l == 16 ? low : 0ull));
        if (__ballot((wm & mine) != 0) == 0) continue;  // nothing selected: the block is not unpacked

        auto steps = [&](auto full_c) {  // unswitched: a block inside the chunk checks no position
#pragma unroll
            for (uint32_t m = 0; m < 16; m++) {
                const uint64_t mA = readlane64(wm, int(m)), mB = readlane64(wm, int(m + 1));
                const uint64_t selw = (mA & ~low) | (mB & low);  // bit l: the mask bit of this lane's row
                if (selw != 0) {                                 // uniform: an empty step unpacks nothing
                    E raw = 0;
                    if (W) {
                        const uint32_t start = start_x[m & 1] + (m >> 1) * W, w0 = start >> LT;
                        const E* __restrict__ q = pw + (LANES * w0 + lane_x[m & 1]);
                        const E lo = q[0], hi = q[LANES];
                        if constexpr (T == 64) {
                            const uint32_t sh = start & 63;
                            raw = (sh ? (lo >> sh) | (hi << (64 - sh)) : lo) & vmask;
                        } else if constexpr (T == 32) {
                            raw = E(__builtin_amdgcn_alignbit(hi, lo, start) & vmask);  // shifts by start % 32
                        } else {
                            raw = E(((uint32_t(lo) | (uint32_t(hi) << T)) >> (start & (T - 1))) & vmask);
                        }
                    }
                    bool oob = false;  // (no Dict epilogue here: never set)
                    const O v = apply_epi<T, EPI, 0>(raw, ep, oob);
                    bool sel = ((selw >> l) & 1ull) != 0;
                    if constexpr (!decltype(full_c)::value) {
                        const uint64_t p = p0 + 64 * m + j;
                        sel = sel && p >= offset && p < uint64_t(offset) + len;
                    }
                    const uint64_t bA = readlane64(wb, int(m)), bB = readlane64(wb, int(m + 1));
                    const uint64_t slot = second ? bB + uint64_t(__popcll(mB & below)) : bA + uint64_t(__popcll(mA & below));
                    if (sel && slot < fm.k) gstore(out + slot, v);
                }
            }
        };
        if (full) steps(std::true_type{});
        else steps(std::false_type{});
    }
}

// The slot of `row` if its mask bit is set (one thread: the tile's words before it are counted).
__device__ __forceinline__ bool filt_slot(const FiltMask& fm, uint64_t row, uint64_t* slot) {
    const uint64_t wi = row >> 6;
    const uint64_t w = filter_mask_word(fm.mask, fm.n, wi);
    if (!((w >> (row & 63)) & 1ull)) return false;
    uint64_t r = gload(fm.tile_off + row / kFilterTileRows);
    for (uint64_t x = wi & ~63ull; x < wi; x++) r += uint64_t(__popcll(filter_mask_word(fm.mask, fm.n, x)));
    r += uint64_t(__popcll(w & lanes_below(int(row & 63))));
    *slot = r;
    return r < fm.k;
}

template <int T, Epi EPI>
__global__ __launch_bounds__(kCmpThreads) void filter_patch_kernel(TakePatches p, uint64_t len, uint64_t first_row,
                                                                   EpiParams ep, FiltMask fm,
                                                                   typename EpiOut<T, EPI, 0>::type* __restrict__ out) {
    using E = typename Fl<T>::E;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < p.n; i += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t pos = patch_pos(p, i);
        if (pos >= len) {
            __hip_atomic_fetch_or(ep.err, kErrTakeOOB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
        uint64_t slot;
        if (!filt_slot(fm, first_row + pos, &slot)) continue;
        bool oob = false;
        gstore(out + slot, apply_epi<T, EPI, 0>(gload(static_cast<const E*>(p.values) + i), ep, oob));
    }
}

template <class V>
__global__ __launch_bounds__(kCmpThreads) void filter_patch_raw_kernel(TakePatches p, uint64_t len, uint64_t first_row,
                                                                       FiltMask fm, V* __restrict__ out, uint32_t* err) {
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < p.n; i += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t pos = patch_pos(p, i);
        if (pos >= len) {
            __hip_atomic_fetch_or(err, kErrTakeOOB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
        uint64_t slot;
        if (!filt_slot(fm, first_row + pos, &slot)) continue;
        gstore(out + slot, gload(static_cast<const V*>(p.values) + i));
    }
}

// filter_values_kernel (filter.hip) over the column rows [first_row, first_row + len) that `in` holds:
// one wave per tile the range touches.
template <class V>
__global__ __launch_bounds__(kCmpThreads) void filter_range_kernel(const V* __restrict__ in, uint64_t first_row,
                                                                   uint64_t len, FiltMask fm, V* __restrict__ out) {
    const int lane = threadIdx.x % kWave;
    const uint64_t t = first_row / kFilterTileRows + uint64_t(blockIdx.x) * (kCmpThreads / kWave) + threadIdx.x / kWave;
    if (t > (first_row + len - 1) / kFilterTileRows) return;  // (len >= 1)
    const TileWords tw = tile_words(fm.mask, fm.n, fm.tile_off, t, lane);
    const uint64_t below = lanes_below(lane);
    const uint64_t row0 = t * kFilterTileRows + uint64_t(lane);
    for (int w = 0; w < 64; ++w) {
        const uint64_t mw = readlane64(tw.m, w);
        if (mw == 0) continue;
        const uint64_t bw = readlane64(tw.base, w);
        const uint64_t row = row0 + uint64_t(w) * 64;
        if (((mw >> lane) & 1ull) && row >= first_row && row - first_row < len) {
            const uint64_t slot = bw + uint64_t(__popcll(mw & below));
            if (slot < fm.k) gstore(out + slot, gload(in + (row - first_row)));
        }
    }
}

}  // namespace

vxg_status launch_filter_packed(int T, Epi epi, const CmpTable& tab, uint64_t groups, uint32_t lds_bytes,
                                const FiltMask& fm, void* out, hipStream_t s) {
    if (groups == 0 || groups > 0x7FFFFFFFull || lds_bytes > 64 * 1024)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "filter: bad launch shape");
#define VXG_FILT(TT, EE)                                                                                         \
    if (T == TT && epi == EE) {                                                                                  \
        hipLaunchKernelGGL((filter_packed_kernel<TT, EE>), dim3(unsigned(groups)), dim3(kCmpThreads), lds_bytes, s, tab, \
                           fm, static_cast<typename EpiOut<TT, EE, 0>::type*>(out));                             \
        return hip_check(hipGetLastError(), "filter_packed_kernel");                                             \
    }
#define VXG_FILT_INT(TT) VXG_FILT(TT, Epi::Plain) VXG_FILT(TT, Epi::For) VXG_FILT(TT, Epi::ForZigZag)
    VXG_FILT_INT(8) VXG_FILT_INT(16) VXG_FILT_INT(32) VXG_FILT_INT(64)
    VXG_FILT(32, Epi::AlpF32) VXG_FILT(64, Epi::AlpF64)
#undef VXG_FILT_INT
#undef VXG_FILT
    return set_error(VXG_ERR_NOT_IMPLEMENTED, "filter: unsupported BitPacked cascade");
}

vxg_status launch_filter_patch(int T, Epi epi, const TakePatches& p, uint64_t len, uint64_t first_row,
                               const EpiParams& ep, const FiltMask& fm, void* out, hipStream_t s) {
    if (p.n == 0) return VXG_OK;
    const dim3 grid(cmp_grid(p.n)), block(kCmpThreads);
#define VXG_FILTP(TT, EE)                                                                                  \
    if (T == TT && epi == EE) {                                                                            \
        hipLaunchKernelGGL((filter_patch_kernel<TT, EE>), grid, block, 0, s, p, len, first_row, ep, fm,    \
                           static_cast<typename EpiOut<TT, EE, 0>::type*>(out));                           \
        return hip_check(hipGetLastError(), "filter_patch_kernel");                                        \
    }
#define VXG_FILTP_INT(TT) VXG_FILTP(TT, Epi::Plain) VXG_FILTP(TT, Epi::For) VXG_FILTP(TT, Epi::ForZigZag)
    VXG_FILTP_INT(8) VXG_FILTP_INT(16) VXG_FILTP_INT(32) VXG_FILTP_INT(64)
    VXG_FILTP(32, Epi::AlpF32) VXG_FILTP(64, Epi::AlpF64)
#undef VXG_FILTP_INT
#undef VXG_FILTP
    return set_error(VXG_ERR_NOT_IMPLEMENTED, "filter: unsupported BitPacked cascade");
}

vxg_status launch_filter_patch_raw(int width, const TakePatches& p, uint64_t len, uint64_t first_row, const FiltMask& fm,
                                   void* out, uint32_t* err, hipStream_t s) {
    if (p.n == 0) return VXG_OK;
    const dim3 grid(cmp_grid(p.n)), block(kCmpThreads);
    if (width == 4)
        hipLaunchKernelGGL((filter_patch_raw_kernel<uint32_t>), grid, block, 0, s, p, len, first_row, fm,
                           static_cast<uint32_t*>(out), err);
    else if (width == 8)
        hipLaunchKernelGGL((filter_patch_raw_kernel<uint64_t>), grid, block, 0, s, p, len, first_row, fm,
                           static_cast<uint64_t*>(out), err);
    else
        return set_error(VXG_ERR_NOT_IMPLEMENTED, "filter: outer patches are f32 or f64");
    return hip_check(hipGetLastError(), "filter_patch_raw_kernel");
}

vxg_status launch_filter_range(int width, const void* in, uint64_t first_row, uint64_t len, const FiltMask& fm,
                               void* out, hipStream_t s) {
    if (len == 0) return VXG_OK;
    const uint64_t tiles = (first_row + len - 1) / kFilterTileRows - first_row / kFilterTileRows + 1;
    const uint64_t groups = (tiles + kCmpThreads / kWave - 1) / (kCmpThreads / kWave);
    if (groups > 0x7FFFFFFFull) return set_error(VXG_ERR_INVALID_ARGUMENT, "filter: array too long");
    const dim3 grid{unsigned(groups)}, block(kCmpThreads);
#define VXG_FILTR(WW, VV)                                                                                     \
    case WW:                                                                                                  \
        hipLaunchKernelGGL((filter_range_kernel<VV>), grid, block, 0, s, static_cast<const VV*>(in), first_row, len, fm, \
                           static_cast<VV*>(out));                                                            \
        break;
    switch (width) {
        VXG_FILTR(1, uint8_t) VXG_FILTR(2, uint16_t) VXG_FILTR(4, uint32_t) VXG_FILTR(8, uint64_t)
    default: return set_error(VXG_ERR_INVALID_ARGUMENT, "filter: unsupported value width");
    }
#undef VXG_FILTR
    return hip_check(hipGetLastError(), "filter_range_kernel");
}

}  // namespace vxg
