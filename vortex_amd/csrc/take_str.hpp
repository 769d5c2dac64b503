// take_str.hpp — arguments of the string take kernels (take_str.hip); internal, not the C ABI.
#pragma once

#include "compare_str.hpp"  // CCol, StrBuf

namespace vxg {

// The indices of a take: n integers of iw bytes (signed if isg) into an array of `len` rows.  A
// negative index sign-extends to a huge one, so it counts as >= len.
struct TakeIdx {
    const void* idx;
    uint64_t n, len;
    int iw, isg;
};

// Rows per workgroup of the FSST take kernels: 256 threads, four rounds of one row per lane, so the
// symbol table's stage into LDS is paid once per 1024 taken rows.
constexpr uint64_t kTakeStrTileRows = 1024;
inline uint64_t take_str_tiles(uint64_t n) { return (n + kTakeStrTileRows - 1) / kTakeStrTileRows; }

// out view j = src view codes[j] (16 bytes each).  A code >= n_src gives a zero view and
// kErrTakeOOB.  `guard` (optional, guard.idx != null): the take's own indices when `codes` are
// values taken at them (Dict) -- row j is a zero view when guard index j is out of bounds.
// `bufs` (optional): the buffer table of the views; a view longer than 12 bytes whose buffer index
// or byte range lies outside it gives a zero view and kErrVarBin.  valid: the OUTPUT rows' LSB
// validity or null; a null row gets a zero view and its source view is not read.
vxg_status launch_take_views(const uint8_t* src, uint64_t n_src, const void* codes, int cw, bool csg, uint64_t n,
                             const TakeIdx& guard, const StrBuf* bufs, uint32_t n_bufs, const uint8_t* valid,
                             uint8_t* out, uint32_t* err, hipStream_t s);

// VarBin, step 1: out record j = {length, 0, 0, offset} of row idx[j] inside the array's own bytes
// (16 bytes, in the views buffer).  Offsets: len + 1 integers, plain or packed.  Malformed offsets
// of a taken row give a zero record and kErrVarBin; an index >= len a zero record and kErrTakeOOB;
// a null row (valid, as above) a zero record without reading its offsets.  bytes_len <= 2^32 - 1.
// The bytes are not read.  launch_view_heap_sizes (filter.hpp, valid = null) sizes the heap from
// the records' lengths.
vxg_status launch_take_varbin_rows(const TakeIdx& t, const CCol& offs, uint64_t bytes_len, const uint8_t* valid,
                                   uint8_t* out, uint32_t* err, hipStream_t s);
// Step 2: every row's bytes copied to heap + its offset (heap_off: launch_view_heap_sizes' scan),
// read once, and its record replaced by the final view over the new heap (buffer 0).
vxg_status launch_take_varbin_build(uint8_t* views, uint64_t n, const uint64_t* heap_off, const uint8_t* bytes,
                                    uint8_t* heap, hipStream_t s);

// FSST rows at indices, decoded in place.
struct TakeFsst {
    const uint64_t* symbols;
    const uint8_t* sym_lens;
    const uint8_t* codes;
    uint64_t codes_len;
    CCol offs;  // codes VarBin offsets (len + 1)
    CCol lens;  // uncompressed lengths (len)
    uint32_t n_symbols;
    TakeIdx t;
    const uint8_t* valid;  // the OUTPUT rows' LSB validity, or null
};
// Sizing: tile_off[tile] = bytes of the tile's taken rows (uncompressed_lengths at the indices; 0
// for a null row or an index >= len), then scanned in place: take_str_tiles(n) + 1 u64,
// tile_off[tiles] = heap bytes.
vxg_status launch_take_fsst_sizes(const TakeFsst& f, uint64_t* tile_off, uint32_t* err, hipStream_t s);
// Decode: every taken row's bytes to heap + its offset (tile_off scanned, heap <= 2^32 - 1 bytes)
// and its final view (buffer 0).  Malformed codes of a taken row give kErrFsst; the row keeps its
// declared length and nothing is written outside its slot.  An index >= len gives kErrTakeOOB.
vxg_status launch_take_fsst_decode(const TakeFsst& f, const uint64_t* tile_off, uint8_t* heap, uint8_t* views,
                                   uint32_t* err, hipStream_t s);

}  // namespace vxg
