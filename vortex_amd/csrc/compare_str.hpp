// compare_str.hpp — arguments of the string compare-with-a-scalar kernels (compare_str.hip);
// internal, not the C ABI.
#pragma once

#include "compare.hpp"

namespace vxg {

// The scalar of a string compare: up to kStrInline bytes ride in the kernel argument (staged into
// LDS by every workgroup), longer ones are read from `dev` (a planner temporary).
constexpr uint32_t kStrInline = 64;
struct StrScalar {
    const uint8_t* dev;  // len > kStrInline
    uint64_t len;
    uint64_t inl[kStrInline / 8];
};

// IntCol (vxg_internal.hpp) packed to 24 bytes, so that 32 FSST pieces fit the kernel argument.
struct CCol {
    const void* p;
    uint64_t reference;
    uint16_t offset;
    uint8_t width, sgn, packed, W, shift, pad;
};
static_assert(sizeof(CCol) == 24, "CCol is packed to 24 bytes");
inline CCol to_ccol(const IntCol& c) {
    CCol r{};
    r.p = c.p;
    r.reference = c.reference;
    r.offset = uint16_t(c.offset);
    r.width = uint8_t(c.width);
    r.sgn = c.sgn;
    r.packed = c.packed;
    r.W = uint8_t(c.W);
    r.shift = uint8_t(c.shift);
    return r;
}

// A workgroup of the row kernels takes kStrWordsPerGroup consecutive bitmap words of one piece
// (one wave per word, four rounds), so a piece's set-up -- FSST's symbol table in LDS -- is paid
// once per 1024 rows.
constexpr uint32_t kStrWordsPerGroup = 16;

// Row i of a piece lands at bit out_bit + i of the launch's bitmap; `excl`: no other producer
// writes a word this piece touches (plain stores only).
// A VarBin whose offsets are a Primitive array and whose bitmap starts on a word: 40 bytes, so the
// dictionaries of a whole C5 column (92 chunks) are one launch.  Every word is exclusive.
struct VbDictPiece {
    const uint8_t* bytes;
    const void* offs;
    uint32_t bytes_len, out_word, n, first_group;
    uint8_t width, sgn;
};
static_assert(sizeof(VbDictPiece) == 40, "VbDictPiece is packed to 40 bytes");
struct VbPiece {
    const uint8_t* bytes;
    uint64_t bytes_len;
    CCol offs;  // n + 1 offsets, any integer ptype, plain or packed
    uint64_t out_bit, n;
    uint32_t first_group, excl;
};
struct StrBuf {
    const uint8_t* p;
    uint64_t len;
};
struct ViewPiece {
    const uint8_t* views;  // 16 B per row, 16-byte aligned
    StrBuf buf0;           // n_buffers <= 1: the buffer itself
    const StrBuf* bufs;    // n_buffers > 1: device table
    uint64_t out_bit, n;
    uint32_t n_buffers, first_group, excl, pad;
};
struct FsstPiece {
    const uint64_t* symbols;
    const uint8_t* sym_lens;
    const uint8_t* codes;
    uint64_t codes_len;
    CCol offs;  // codes VarBin offsets (n + 1)
    CCol lens;  // uncompressed lengths (n)
    uint64_t out_bit, n;
    uint32_t first_group, excl, n_symbols, pad;
};
// Dict codes read in place (a Primitive array or a temporary): bit i = table[codes[i]].
struct DictPlainPiece {
    const void* codes;
    uint64_t out_bit, n;
    uint32_t first_group, tword, vlen;  // truth table: 64-bit word index, entries
    uint8_t width, sgn, excl;
};
static_assert(sizeof(DictPlainPiece) == 40, "DictPlainPiece is packed to 40 bytes");

constexpr int kStrArgPieces = 32;   // VarBin / VarBinView / FSST pieces per launch
constexpr int kStrArgPieces40 = 96; // 40-byte pieces per launch
template <class P, int N>
struct PieceTab {
    P c[N];
    uint32_t n;
};
using VbDictTab = PieceTab<VbDictPiece, kStrArgPieces40>;
using VbTab = PieceTab<VbPiece, kStrArgPieces>;
using ViewTab = PieceTab<ViewPiece, kStrArgPieces>;
using FsstTab = PieceTab<FsstPiece, kStrArgPieces>;
using DictPlainTab = PieceTab<DictPlainPiece, kStrArgPieces40>;
// the 4 KiB kernel-argument limit: table + scalar + two pointers + op
static_assert(sizeof(VbDictTab) + sizeof(StrScalar) + 24 <= 4096, "kernel argument");
static_assert(sizeof(VbTab) + sizeof(StrScalar) + 24 <= 4096, "kernel argument");
static_assert(sizeof(ViewTab) + sizeof(StrScalar) + 24 <= 4096, "kernel argument");
static_assert(sizeof(FsstTab) + sizeof(StrScalar) + 24 <= 4096, "kernel argument");
static_assert(sizeof(DictPlainTab) + 32 <= 4096, "kernel argument");
static_assert(sizeof(CmpTable) + 40 <= 4096, "kernel argument");

inline uint64_t piece_words(uint64_t out_bit, uint64_t n) { return n ? ((out_bit + n + 63) >> 6) - (out_bit >> 6) : 0; }
inline uint64_t piece_groups(uint64_t out_bit, uint64_t n) {
    return (piece_words(out_bit, n) + kStrWordsPerGroup - 1) / kStrWordsPerGroup;
}

// Row compare: out bit = op(bytes of row, scalar), unsigned lexicographic, a proper prefix is
// smaller.  `groups` = sum of piece_groups (first_group filled in).  Malformed offsets or views
// set kErrVarBin, malformed FSST codes kErrFsst; such a row's bit is 0.
vxg_status launch_cmpb_varbin_dict(const VbDictTab& t, uint64_t groups, const StrScalar& sc, void* out, uint32_t* err,
                                   int op, hipStream_t s);
vxg_status launch_cmpb_varbin(const VbTab& t, uint64_t groups, const StrScalar& sc, void* out, uint32_t* err, int op,
                              hipStream_t s);
vxg_status launch_cmpb_views(const ViewTab& t, uint64_t groups, const StrScalar& sc, void* out, uint32_t* err, int op,
                             hipStream_t s);
vxg_status launch_cmpb_fsst(const FsstTab& t, uint64_t groups, const StrScalar& sc, void* out, uint32_t* err, int op,
                            hipStream_t s);

// Dict lookup: out bit i = bit codes[i] of the piece's truth table (64-bit words of `tt`); a code
// >= the dictionary's length sets kErrTakeOOB and gives 0.
// A dictionary of at most kDictLdsBits entries (1 KiB of truth table) is staged into LDS by the
// packed-domain kernel; a longer one is read from global memory.
constexpr uint32_t kDictLdsBits = 8192;
vxg_status launch_cmpb_dict_plain(const DictPlainTab& t, uint64_t groups, void* out, const void* tt, uint32_t* err,
                                  hipStream_t s);
// BitPacked unsigned codes in the packed domain (compare.hip's walk): CmpChunk::reference holds
// the truth-table word index (low 32 bits) and the dictionary's length (high 32 bits).
// lds_bytes: the staging area of the packed words, as for launch_cmp_packed.
vxg_status launch_cmpb_dict_packed(int T, const CmpTable& tab, uint64_t groups, uint32_t lds_bytes, void* out,
                                   const void* tt, uint32_t* err, hipStream_t s);

}  // namespace vxg
