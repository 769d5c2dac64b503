// filter_packed.hpp — arguments of the packed-domain filter kernels (filter_packed.hip, K22);
// internal, not the C ABI.
#pragma once

#include "compare.hpp"  // CmpChunk / CmpTable: the chunk table of a launch, out_bit = the chunk's first row
#include "filter.hpp"

namespace vxg {

// The row mask of a batch, counted and scanned once (launch_filter_count): bits at and beyond n
// are ignored, tile_off holds filter_tiles(n) + 1 entries and k = tile_off[tiles], the true count
// the host read back.  No kernel below writes a slot at or past k.
struct FiltMask {
    const uint64_t* mask;
    uint64_t n;
    const uint64_t* tile_off;
    uint64_t k;
};

// The selected rows of BitPacked-rooted cascades, unpacked through the epilogue of (T, epi) and
// written to their slots of `out` (values of the epilogue's output type).  Chunk c of the table
// covers column rows [c.out_bit, c.out_bit + c.len()).  lds_bytes = max over the chunks of
// bpw * 128 * W, + 128 of slack.
vxg_status launch_filter_packed(int T, Epi epi, const CmpTable& tab, uint64_t groups, uint32_t lds_bytes,
                                const FiltMask& fm, void* out, hipStream_t s);
// Patched rows, after the launch above: each patch whose row (first_row + position) is selected
// overwrites its slot.  Inner BitPacked patches: raw T-bit values through the epilogue.
vxg_status launch_filter_patch(int T, Epi epi, const TakePatches& p, uint64_t len, uint64_t first_row,
                               const EpiParams& ep, const FiltMask& fm, void* out, hipStream_t s);
// Outer ALP patches: values of `width` bytes as they are.
vxg_status launch_filter_patch_raw(int width, const TakePatches& p, uint64_t len, uint64_t first_row, const FiltMask& fm,
                                   void* out, uint32_t* err, hipStream_t s);
// The selected rows of a primitive buffer that holds column rows [first_row, first_row + len)
// (a Primitive array, or one Primitive chunk), `width` bytes each (1, 2, 4, 8).
vxg_status launch_filter_range(int width, const void* in, uint64_t first_row, uint64_t len, const FiltMask& fm,
                               void* out, hipStream_t s);

}  // namespace vxg
