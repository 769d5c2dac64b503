// compare.hpp — arguments of the compare-with-a-scalar kernels (compare.hip); internal, not the C ABI.
#pragma once

#include "take.hpp"  // EpiParams, Epi, TakePatches

namespace vxg {

// How the decoded value is compared: in the ptype's signedness, or as an IEEE float.
enum : int { kCmpUnsigned = 0, kCmpSigned = 1, kCmpFloat = 2 };

// One BitPacked-rooted cascade (a whole array or one chunk of a ChunkedArray) of a fused compare
// launch: bit i of the chunk lands at bit out_bit + i of the launch's bitmap.  40 bytes, so the
// table of a whole C5 column (92 chunks) travels as the kernel argument: no upload, no host state.
struct CmpChunk {
    const uint8_t* packed;
    uint64_t reference;    // FoR reference bits
    uint64_t out_bit;      // bitmap bit of value 0
    uint32_t len_lo;       // values compared: len_lo | len_hi << 32
    uint32_t first_group;  // first workgroup of this chunk in the launch
    uint16_t offset;       // values to skip in block 0 (< 1024)
    uint8_t len_hi;
    uint8_t W;             // bit width (0..T)
    uint8_t shift;         // FoR shift
    // blocks per workgroup (multiple of 4, <= 32) | 0x80: no other producer writes a bitmap word
    // this chunk touches (out_bit, offset and the end fall on word boundaries, or the end is the
    // end of the bitmap), so every word is a plain store
    uint8_t bpw_excl;
    uint8_t alp_e, alp_f;  // ALP exponents (the kernel holds the reference's tables)
    __host__ __device__ uint64_t len() const { return uint64_t(len_lo) | uint64_t(len_hi) << 32; }
    __host__ __device__ uint64_t n_blocks() const { return len() ? (len() + offset + 1023) / 1024 : 0; }
    __host__ __device__ uint32_t bpw() const { return bpw_excl & 0x7Fu; }
    __host__ __device__ bool excl() const { return (bpw_excl & 0x80u) != 0; }
};
static_assert(sizeof(CmpChunk) == 40, "CmpChunk is packed to 40 bytes");
constexpr uint64_t kCmpMaxLen = (uint64_t(1) << 40) - 1;
constexpr int kCmpArgChunks = 100;
struct CmpTable {
    CmpChunk c[kCmpArgChunks];
    uint32_t n;
};

// Blocks per workgroup the staging LDS (32 KiB) allows at bit width W.
inline uint32_t cmp_bpw_max(uint32_t W) {
    const uint32_t b = ((32u * 1024u) / (128u * (W ? W : 1u))) & ~3u;
    return b < 4 ? 4 : (b > 32 ? 32 : b);
}

// Fused packed-domain compare: out (64-bit words) gets op(epilogue(unpacked), scalar) per value.
// Whole words inside a chunk are plain stores; a chunk's edge words are ORed in (zeroed bitmap)
// unless the chunk is `excl`.  lds_bytes = max over the chunks of bpw * 128 * W, + 128 of slack.
vxg_status launch_cmp_packed(int T, Epi epi, int ck, const CmpTable& tab, uint64_t groups, uint32_t lds_bytes,
                             void* out, uint64_t scalar_bits, int op, hipStream_t s);
// Compare a primitive buffer of `ptype` and write n bits at bit out_bit (same store rule).
vxg_status launch_cmp_plain(int ptype, const void* in, uint64_t n, void* out, uint64_t out_bit, uint64_t scalar_bits,
                            int op, bool excl, hipStream_t s);
// Re-compare patched rows and set or clear their bits (32-bit atomics), after the launches above.
// Inner BitPacked patches: raw T-bit values through the epilogue.
vxg_status launch_cmp_patch(int T, Epi epi, int ck, const TakePatches& p, uint64_t len, void* out, uint64_t out_bit,
                            const EpiParams& ep, uint64_t scalar_bits, int op, hipStream_t s);
// Outer ALP patches: values of `ptype` as they are.
vxg_status launch_cmp_patch_raw(int ptype, const TakePatches& p, uint64_t len, void* out, uint64_t out_bit,
                                uint64_t scalar_bits, int op, uint32_t* err, hipStream_t s);
// bits[w] &= mask[w] over n_words 64-bit words (values AND validity).
vxg_status launch_and_words(void* bits, const void* mask, uint64_t n_words, hipStream_t s);

// ---- the row filter's kernels (compare_range.hip) ---------------------------------------------
// A range on one column as one test: lo_op (GT or GTE) against lo_bits AND hi_op (LT or LTE)
// against hi_bits, the scalars as the little-endian bits of the compared type.
struct CmpRange {
    uint64_t lo_bits, hi_bits;
    int lo_op, hi_op;
};
// The two-sided twins of the four launches above: the same arguments, bitmap store rules and launch
// shapes, bit for bit the AND of the two one-sided results.
vxg_status launch_cmp_range_packed(int T, Epi epi, int ck, const CmpTable& tab, uint64_t groups, uint32_t lds_bytes,
                                   void* out, const CmpRange& r, hipStream_t s);
vxg_status launch_cmp_range_plain(int ptype, const void* in, uint64_t n, void* out, uint64_t out_bit, const CmpRange& r,
                                  bool excl, hipStream_t s);
vxg_status launch_cmp_range_patch(int T, Epi epi, int ck, const TakePatches& p, uint64_t len, void* out, uint64_t out_bit,
                                  const EpiParams& ep, const CmpRange& r, hipStream_t s);
vxg_status launch_cmp_range_patch_raw(int ptype, const TakePatches& p, uint64_t len, void* out, uint64_t out_bit,
                                      const CmpRange& r, uint32_t* err, hipStream_t s);
// out[w] = p[0][w] & ... & p[k-1][w] over n_words 64-bit words (out may alias an input); with
// `count`, the set bits of out are ADDED to *count (a device uint64 the caller zeroed on `s`).
constexpr int kAndInputs = 16;
struct AndInputs {
    const uint64_t* p[kAndInputs];
    uint32_t k;
};
vxg_status launch_and_count(const AndInputs& in, void* out, uint64_t n_words, uint64_t* count, hipStream_t s);

}  // namespace vxg
