// planner_compute.hip — compute on compressed arrays: take (vortex-array/src/compute/take.rs:10-34,
// take.hip), filter (compute/filter.rs:23-52, filter.hip), compare with a scalar
// (compute/compare.rs:81-124, compare.hip) and compare of strings with a scalar (compare_str.hip).
// Each reads the compressed tree where a kernel serves it and falls back to the canonical values.
#include <algorithm>
#include <cstring>
#include <tuple>

#include "filter.hpp"
#include "filter_packed.hpp"
#include "planner.hpp"

namespace vxg {

// ---- compute::take on compressed arrays (vortex-array/src/compute/take.rs:10-34) ---------
vxg_status Planner::take_patches(const vxg_array& sp, TakePatches& p) {
    if (sp.encoding != VXG_ENC_SPARSE) return set_error(VXG_ERR_INVALID_ARGUMENT, "Can't patch with a non-Sparse array");
    const vxg_array* idx = child(sp, 0);
    const vxg_array* val = child(sp, 1);
    if (!idx || !val || idx->len != val->len)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "Sparse patches need indices and values of equal length");
    if (!ptype_is_int(idx->ptype)) return set_error(VXG_ERR_MISMATCHED_TYPES, "Sparse indices must be integers");
    VXG_TRY(view_primitive(*idx, &p.idx));
    VXG_TRY(view_primitive(*val, &p.values));
    p.n = idx->len;
    p.off = sp.meta.sparse.indices_offset;
    p.iw = width(*idx);
    p.isg = ptype_is_signed(idx->ptype);
    return VXG_OK;
}

vxg_status Planner::take_values(const vxg_array& a, const void* idx, int iw, bool isg, uint64_t n, void* dst) {
    if (n == 0) return VXG_OK;
    auto via_canonical = [&]() -> vxg_status {  // canonicalize, then take the primitive
        if (tinfo_) tinfo_->fallback_arrays++;
        const void* pv;
        VXG_TRY(view_primitive(a, &pv));
        return launch_take(width(a), pv, a.len, iw, isg, idx, n, dst, ctx_->c.err_word, s_);
    };
    const vxg_array* bp = nullptr;
    Epi epi = Epi::Plain;
    EpiParams ep{};
    TakePatches outer;
    auto fl_child = [&](const vxg_array* c) -> const vxg_array* {  // FoR(BitPacked) or BitPacked
        if (c && c->encoding == VXG_ENC_FL_FOR && child(*c, 0) && child(*c, 0)->encoding == VXG_ENC_FL_BITPACKED) {
            ep.reference = c->meta.for_.reference;
            ep.shift = c->meta.for_.shift;
            return child(*c, 0);
        }
        return c && c->encoding == VXG_ENC_FL_BITPACKED ? c : nullptr;
    };
    switch (a.encoding) {
    case VXG_ENC_FL_BITPACKED: bp = &a; break;  // bitpacking/compute/take.rs:21-125
    case VXG_ENC_FL_FOR:                          // for/compute.rs:39-48: take the child, keep the FoR
        bp = fl_child(&a);
        epi = Epi::For;
        break;
    case VXG_ENC_ZIGZAG:  // zigzag/compute.rs: take the encoded child, decode
        bp = fl_child(child(a, 0));
        epi = Epi::ForZigZag;
        break;
    case VXG_ENC_ALP: {  // alp/compute.rs: take the encoded child and the patches
        const bool f32 = a.ptype == VXG_F32;
        const unsigned e = a.meta.alp.e, f = a.meta.alp.f;
        if ((f32 && (e > 10 || f > 10)) || (!f32 && (a.ptype != VXG_F64 || e > 23 || f > 23))) return via_canonical();
        bp = fl_child(child(a, 0));
        epi = f32 ? Epi::AlpF32 : Epi::AlpF64;
        ep.alp_a = f32 ? double(kF10f[f]) : kF10d[f];
        ep.alp_b = f32 ? double(kIF10f[e]) : kIF10d[e];
        if (bp && a.meta.alp.has_patches) {
            if (!child(a, 1)) return set_error(VXG_ERR_INVALID_ARGUMENT, "ALPArray: patches child missing");
            VXG_TRY(take_patches(*child(a, 1), outer));
        }
        break;
    }
    case VXG_ENC_DICT: {  // dict/compute.rs:44-52: take the codes, then the values at them
        const vxg_array* values = child(a, 0);
        const vxg_array* codes = child(a, 1);
        if (!values || !codes || values->dtype != VXG_DTYPE_PRIMITIVE || !ptype_is_int(codes->ptype))
            return via_canonical();
        if (tinfo_) tinfo_->dict_arrays++;
        void* tc;
        VXG_TRY(temp(n * width(*codes), &tc));
        VXG_TRY(take_codes(*codes, idx, iw, isg, n, tc));
        const void* pv;
        VXG_TRY(view_primitive(*values, &pv));
        return launch_take(width(*values), pv, values->len, width(*codes), false, tc, n, dst, ctx_->c.err_word, s_);
    }
    default: return via_canonical();
    }
    const int T = bp ? 8 * width(*bp) : 0;
    const bool t_ok = bp && (epi == Epi::AlpF32 ? T == 32 : epi == Epi::AlpF64 ? T == 64 : T == 8 * width(a));
    // bitpacking/compute/take.rs:23-31: many indices -> canonicalize and take the primitive
    if (!t_ok || bp->len != a.len || n * 8 > a.len) return via_canonical();
    const vxg_buffer* pb = buf(*bp, 0);
    const unsigned W = bp->meta.bitpacked.bit_width, off = bp->meta.bitpacked.offset;
    if (off > 1023) return set_error(VXG_ERR_INVALID_ARGUMENT, "Offset must be less than full block, i.e. 1024");
    if (W > unsigned(T)) return set_error(VXG_ERR_INVALID_ARGUMENT, "Unsupported bit width");
    const uint64_t nblk = (bp->len + off + 1023) / 1024, have = pb ? pb->len : 0;
    if (W > 0 && have != nblk * 128ull * W)  // bitpacking/mod.rs:80-88
        return set_error(VXG_ERR_INVALID_ARGUMENT, "Expected " + std::to_string(nblk * 128ull * W) +
                                                       " packed bytes, got " + std::to_string(have));
    TakePacked t{};
    t.packed = pb ? static_cast<const uint8_t*>(pb->ptr) : nullptr;
    t.W = W;
    t.offset = off;
    t.len = a.len;
    t.idx = idx;
    t.iw = iw;
    t.isg = isg;
    t.n = n;
    t.out = dst;
    t.ep = ep;
    t.outer = outer;
    t.err = ctx_->c.err_word;
    if (bp->meta.bitpacked.has_patches) {  // take.rs:127-200: patches of the taken positions
        if (!child(*bp, 0)) return set_error(VXG_ERR_INVALID_ARGUMENT, "BitPacked patches child missing");
        VXG_TRY(take_patches(*child(*bp, 0), t.inner));
    }
    if (tinfo_) tinfo_->packed_launches++;
    return launch_take_packed(T, epi, t, s_);
}

// The codes of a Dict at the indices: the Dict is what the counters name (dict_arrays), so codes
// that go through their canonical values do not count as a fallback of their own.
vxg_status Planner::take_codes(const vxg_array& codes, const void* idx, int iw, bool isg, uint64_t n, void* dst) {
    const uint32_t fb = tinfo_ ? tinfo_->fallback_arrays : 0;
    const vxg_status st = take_values(codes, idx, iw, isg, n, dst);
    if (tinfo_) tinfo_->fallback_arrays = fb;
    return st;
}

// validity.take(indices): the array's validity into a temporary, then the bit gather.
vxg_status Planner::take_validity(const vxg_array& a, const void* idx, int iw, bool isg, uint64_t n, vxg_canonical& out) {
    const vxg_array* node;
    int kind;
    VXG_TRY(validity_source(a, &node, &kind));
    if (kind == 0) {  // validity.take of NonNullable / AllValid: no nulls
        out.validity = nullptr;
        return VXG_OK;
    }
    void* src = nullptr;  // the array's validity, then taken at the indices
    VXG_TRY(temp(((a.len + 31) / 32) * 4, &src));
    VXG_TRY(validity_into(a, &src));
    const uint64_t bytes = ((n + 31) / 32) * 4;
    if (!out.validity) VXG_TRY(hip_check(hipMalloc(&out.validity, bytes ? bytes : 4), "take validity alloc"));
    return launch_gather_bits(out.validity, idx, iw, isg, n, static_cast<const uint8_t*>(src), a.len, ctx_->c.err_word,
                              s_);
}

vxg_status Planner::take(const vxg_array& a, const void* idx, int iw, bool isg, uint64_t n, uint32_t flags,
                         vxg_canonical& out, vxg_take_info& info) {
    if (flags & ~uint32_t(VXG_TAKE_CANONICALIZE)) return set_error(VXG_ERR_INVALID_ARGUMENT, "unknown take flags");
    const bool force = (flags & VXG_TAKE_CANONICALIZE) != 0;
    tinfo_ = &info;
    if (is_string(a)) return take_strings(a, idx, iw, isg, n, force, out, info);
    out.len = n;
    out.dtype = a.dtype;
    out.ptype = a.ptype;
    if (a.dtype == VXG_DTYPE_BOOL) {  // bool/compute/take.rs: the canonical bits, gathered
        out.kind = VXG_ENC_BOOL;
        out.values_bytes = ((n + 31) / 32) * 4;
        const uint64_t src_bytes = ((a.len + 31) / 32) * 4;
        void* bits;
        VXG_TRY(temp(src_bytes, &bits));
        VXG_TRY(launch_copy_bytes(bits, nullptr, src_bytes ? src_bytes : 4, s_));
        VXG_TRY(bools_into(a, bits, 0));
        info.fallback_arrays++;
        if (!out.values)
            VXG_TRY(hip_check(hipMalloc(&out.values, out.values_bytes ? out.values_bytes : 4), "take bool alloc"));
        VXG_TRY(launch_gather_bits(out.values, idx, iw, isg, n, static_cast<const uint8_t*>(bits), a.len,
                                   ctx_->c.err_word, s_));
        return take_validity(a, idx, iw, isg, n, out);
    }
    if (a.dtype != VXG_DTYPE_PRIMITIVE)
        return set_error(VXG_ERR_NOT_IMPLEMENTED, "take supports primitive, bool and utf8/binary dtypes");
    out.kind = VXG_ENC_PRIMITIVE;
    out.values_bytes = n * width(a);
    if (!out.values)
        VXG_TRY(hip_check(hipMalloc(&out.values, out.values_bytes ? out.values_bytes : 16), "take values alloc"));
    if (force) {  // VXG_TAKE_CANONICALIZE: the canonical values, then the gather
        if (n) {
            info.fallback_arrays++;
            const void* pv;
            VXG_TRY(view_primitive(a, &pv));
            VXG_TRY(launch_take(width(a), pv, a.len, iw, isg, idx, n, out.values, ctx_->c.err_word, s_));
        }
    } else {
        VXG_TRY(take_values(a, idx, iw, isg, n, out.values));
    }
    return take_validity(a, idx, iw, isg, n, out);
}

// take of a utf8 / binary array (take_str.hip): one new heap of the taken rows in index order, views
// over it.  Dict takes its codes and gathers the dictionary's views; VarBin, VarBinView and FSST rows
// are read where they lie; everything else (Chunked, a Dict of Chunked values, `force`) canonicalizes
// the whole array into temporaries first.  Synchronous: the heap size is read back.
vxg_status Planner::take_strings(const vxg_array& a, const void* idx, int iw, bool isg, uint64_t n, bool force,
                                 vxg_canonical& out, vxg_take_info& info) {
    uint32_t* err = ctx_->c.err_word;
    const TakeIdx tix{idx, n, a.len, iw, int(isg)};
    auto bytes_of = [&](const vxg_array& b, const void** p) -> vxg_status {
        if (b.dtype != VXG_DTYPE_PRIMITIVE || width(b) != 1)
            return set_error(VXG_ERR_MISMATCHED_TYPES, "string bytes must be a u8 array");
        return view_primitive(b, p);
    };
    // canonical views of `s` in temporaries + the base of each of their data buffers
    auto canonical_views = [&](const vxg_array& s, const uint8_t** views, std::vector<const uint8_t*>& bases) -> vxg_status {
        vxg_canonical src{};
        std::vector<vxg_data_buffer> lay;
        uint64_t extent;
        VXG_TRY(string_layout(s, lay, extent));
        const vxg_array* vnode;
        int vkind;
        VXG_TRY(validity_source(s, &vnode, &vkind));
        if (vkind != 0) VXG_TRY(temp(((s.len + 31) / 32) * 4, &src.validity));
        VXG_TRY(temp(16 * s.len, &src.views));
        VXG_TRY(temp(extent + 16, &src.data));
        src.data_bytes = extent;
        src.data_buffers = lay.data();
        src.n_data_buffers = src.data_buffers_cap = uint32_t(lay.size());
        VXG_TRY(string_canonical(s, src));
        *views = static_cast<const uint8_t*>(src.views);
        bases.resize(lay.size());
        for (size_t b = 0; b < lay.size(); b++) bases[b] = static_cast<const uint8_t*>(src.data) + lay[b].offset;
        return VXG_OK;
    };

    // ---- classify and validate before any output is allocated ----
    enum class Kind { Fallback, Dict, View, VarBin, Fsst } kind = Kind::Fallback;
    const vxg_array *dvalues = nullptr, *dcodes = nullptr;
    const void* src_views = nullptr;   // View
    std::vector<StrBuf> vbufs;         // View: its buffers
    CCol vb_offs{};                    // VarBin
    const void* vb_bytes = nullptr;
    uint64_t vb_bytes_len = 0;
    TakeFsst fs{};
    if (!force) switch (a.encoding) {
    case VXG_ENC_DICT: {
        dvalues = child(a, 0);
        dcodes = child(a, 1);
        if (!dvalues || !dcodes) return set_error(VXG_ERR_INVALID_ARGUMENT, "DictArray needs values and codes");
        if (!ptype_is_int(dcodes->ptype) || dcodes->dtype != VXG_DTYPE_PRIMITIVE)
            return set_error(VXG_ERR_MISMATCHED_TYPES, "Dict codes must be integers");
        if (dcodes->len != a.len) return set_error(VXG_ERR_INVALID_ARGUMENT, "Dict codes length != array length");
        // Density rule (profiles/take_strings_bench.json, dict_shipmode): taking the codes first wins
        // up to len / 4 (1.03-2.35x), ties at len / 2 and loses from n = len (0.96x, both index orders:
        // as many codes are taken as the array holds, and they pass through a temporary that the
        // fused codes -> views decode of the canonical path never writes): n >= len canonicalizes.
        if (is_string(*dvalues) && dvalues->encoding != VXG_ENC_CHUNKED && n < a.len) kind = Kind::Dict;
        break;
    }
    case VXG_ENC_VARBINVIEW: {
        const vxg_array* vw = child(a, 0);
        const uint32_t nb = a.meta.varbinview.n_buffers;
        if (!vw || a.n_children < 1 + nb)
            return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBinViewArray: missing views/data buffers");
        VXG_TRY(bytes_of(*vw, &src_views));
        if (vw->len < 16 * a.len) return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBinView views shorter than 16 * len");
        if (reinterpret_cast<uintptr_t>(src_views) & 15)
            return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBinView views must be 16-byte aligned");
        vbufs.resize(nb);
        for (uint32_t b = 0; b < nb; b++) {
            const void* pb;
            VXG_TRY(bytes_of(a.children[1 + b], &pb));
            vbufs[b] = StrBuf{static_cast<const uint8_t*>(pb), a.children[1 + b].len};
        }
        kind = Kind::View;
        break;
    }
    case VXG_ENC_VARBIN: {
        const vxg_array* offs = child(a, 0);
        const vxg_array* bytes = child(a, 1);
        if (!offs || !bytes) return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBinArray needs offsets and bytes");
        if (!ptype_is_int(offs->ptype) || offs->dtype != VXG_DTYPE_PRIMITIVE)
            return set_error(VXG_ERR_MISMATCHED_TYPES, "VarBin offsets must be integers");
        if (offs->len < a.len + 1) return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBin offsets shorter than len + 1");
        if (bytes->len > 0xFFFFFFFFull) break;  // a view's offset is a u32: the canonical's several buffers
        VXG_TRY(bytes_of(*bytes, &vb_bytes));
        vb_bytes_len = bytes->len;
        IntCol oc;
        VXG_TRY(int_column(*offs, oc));
        if (reinterpret_cast<uintptr_t>(oc.p) % uint64_t(oc.packed ? 16 : oc.width))
            return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBin offsets must be aligned to their width");
        vb_offs = to_ccol(oc);
        kind = Kind::VarBin;
        break;
    }
    case VXG_ENC_FSST: {
        const vxg_array* sym = child(a, 0);
        const vxg_array* slen = child(a, 1);
        const vxg_array* codes = child(a, 2);
        const vxg_array* ulen = child(a, 3);
        if (!sym || !slen || !codes || !ulen || codes->encoding != VXG_ENC_VARBIN || !child(*codes, 0) || !child(*codes, 1))
            return set_error(VXG_ERR_INVALID_ARGUMENT, "FSSTArray needs symbols, lengths, VarBin codes, lengths");
        if (sym->len > 255 || slen->len < sym->len || width(*sym) != 8 || width(*slen) != 1)
            return set_error(VXG_ERR_INVALID_ARGUMENT, "FSST symbol table must hold at most 255 u64 symbols and their u8 lengths");
        if (codes->len != a.len || ulen->len < a.len || child(*codes, 0)->len < a.len + 1)
            return set_error(VXG_ERR_INVALID_ARGUMENT, "FSST codes / lengths do not cover the array");
        if (!ptype_is_int(child(*codes, 0)->ptype) || !ptype_is_int(ulen->ptype))
            return set_error(VXG_ERR_MISMATCHED_TYPES, "FSST offsets and lengths must be integers");
        const void *psym, *pslen, *pcb;
        VXG_TRY(view_primitive(*sym, &psym));
        VXG_TRY(view_primitive(*slen, &pslen));
        VXG_TRY(bytes_of(*child(*codes, 1), &pcb));
        if (reinterpret_cast<uintptr_t>(psym) & 7) return set_error(VXG_ERR_INVALID_ARGUMENT, "FSST symbols must be 8-byte aligned");
        IntCol oc, lc;
        VXG_TRY(int_column(*child(*codes, 0), oc));
        VXG_TRY(int_column(*ulen, lc));
        if (reinterpret_cast<uintptr_t>(oc.p) % uint64_t(oc.packed ? 16 : oc.width) ||
            reinterpret_cast<uintptr_t>(lc.p) % uint64_t(lc.packed ? 16 : lc.width))
            return set_error(VXG_ERR_INVALID_ARGUMENT, "FSST offsets / lengths must be aligned to their width");
        fs.symbols = static_cast<const uint64_t*>(psym);
        fs.sym_lens = static_cast<const uint8_t*>(pslen);
        fs.codes = static_cast<const uint8_t*>(pcb);
        fs.codes_len = child(*codes, 1)->len;
        fs.offs = to_ccol(oc);
        fs.lens = to_ccol(lc);
        fs.n_symbols = uint32_t(sym->len);
        fs.t = tix;
        kind = Kind::Fsst;
        break;
    }
    default: break;
    }
    if (reinterpret_cast<uintptr_t>(out.views) & 15)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "take: views must be 16-byte aligned");
    (kind == Kind::Dict ? info.dict_arrays : kind == Kind::Fallback ? info.fallback_arrays : info.direct_arrays)++;

    out.kind = VXG_ENC_VARBINVIEW;
    out.len = n;
    out.dtype = a.dtype;
    out.ptype = a.ptype;

    // ---- validity.take(indices), before the rows: a null row keeps no bytes ----
    void* tcodes = nullptr;  // Dict: the codes at the indices
    const int cw = dcodes ? width(*dcodes) : 0;
    if (kind == Kind::Dict) {
        VXG_TRY(temp(n * cw, &tcodes));
        VXG_TRY(take_codes(*dcodes, idx, iw, isg, n, tcodes));
        // values.validity().take(codes) (validity_into's Dict rule) from the codes already taken:
        // work by n and the dictionary's size, not by len
        const vxg_array* vnode;
        int vkind;
        VXG_TRY(validity_source(*dvalues, &vnode, &vkind));
        if (vkind == 0) {
            out.validity = nullptr;
        } else {
            void* vbits = nullptr;
            VXG_TRY(temp(((dvalues->len + 31) / 32) * 4, &vbits));
            VXG_TRY(validity_into(*dvalues, &vbits));
            const uint64_t bytes = ((n + 31) / 32) * 4;
            if (!out.validity) VXG_TRY(hip_check(hipMalloc(&out.validity, bytes ? bytes : 4), "take validity alloc"));
            VXG_TRY(launch_gather_bits(out.validity, tcodes, cw, false, n, static_cast<const uint8_t*>(vbits),
                                       dvalues->len, err, s_));
        }
    } else {
        VXG_TRY(take_validity(a, idx, iw, isg, n, out));
    }
    const uint8_t* valid = static_cast<const uint8_t*>(out.validity);
    if (!out.views) VXG_TRY(hip_check(hipMalloc(&out.views, n ? 16 * n : 16), "take views alloc"));
    uint8_t* views = static_cast<uint8_t*>(out.views);

    // the heap's size is known: check it against the caller's buffer, or allocate
    auto size_heap = [&](uint64_t heap) -> vxg_status {
        if (heap > 0xFFFFFFFFull) return set_error(VXG_ERR_INVALID_ARGUMENT, "taken string heap exceeds u32 view offsets");
        if (out.data && out.data_bytes < heap)
            return set_error(VXG_ERR_INVALID_ARGUMENT, "caller-provided data holds " + std::to_string(out.data_bytes) +
                                                           " bytes, the taken heap needs " + std::to_string(heap));
        if (!out.data) VXG_TRY(hip_check(hipMalloc(&out.data, heap + 16), "take heap alloc"));
        out.data_bytes = heap;
        out.n_data_buffers = 1;
        if (out.data_buffers && out.data_buffers_cap >= 1) out.data_buffers[0] = vxg_data_buffer{0, heap};
        return VXG_OK;
    };
    auto read_total = [&](const uint64_t* p, uint64_t* v) -> vxg_status {
        VXG_TRY(hip_check(hipMemcpyAsync(v, p, 8, hipMemcpyDeviceToHost, s_), "take heap readback"));
        return hip_check(hipStreamSynchronize(s_), "take heap sync");
    };

    if (kind == Kind::Fsst) {  // sizes from uncompressed_lengths, then decode only the taken rows
        fs.valid = valid;
        const uint64_t tiles = take_str_tiles(n);
        void* toff;
        VXG_TRY(temp((tiles + 1) * 8, &toff));
        VXG_TRY(launch_take_fsst_sizes(fs, static_cast<uint64_t*>(toff), err, s_));
        uint64_t heap = 0;
        VXG_TRY(read_total(static_cast<uint64_t*>(toff) + tiles, &heap));
        VXG_TRY(size_heap(heap));
        VXG_TRY(launch_take_fsst_decode(fs, static_cast<const uint64_t*>(toff), static_cast<uint8_t*>(out.data), views, err,
                                        s_));
        return hip_check(hipStreamSynchronize(s_), "take sync");
    }

    // ---- source views of the taken rows, then filter's heap rebuild over their buffers ----
    // The small host tables (`vbufs`, `bases`) are uploaded stream-ordered; the heap-size readback's
    // sync drains those copies, so they cost no sync of their own.
    std::vector<const uint8_t*> bases;
    auto rows = [&]() -> vxg_status {
        const uint64_t ktiles = filter_tiles(n);
        void* hoff;
        VXG_TRY(temp((ktiles + 1) * 8, &hoff));
        uint64_t heap = 0;
        if (kind == Kind::VarBin) {  // records, sizes, then one pass over the taken rows' bytes
            VXG_TRY(launch_take_varbin_rows(tix, vb_offs, vb_bytes_len, valid, views, err, s_));
            VXG_TRY(launch_view_heap_sizes(views, n, nullptr, static_cast<uint64_t*>(hoff), s_));
            VXG_TRY(read_total(static_cast<uint64_t*>(hoff) + ktiles, &heap));
            VXG_TRY(size_heap(heap));
            return launch_take_varbin_build(views, n, static_cast<const uint64_t*>(hoff), static_cast<const uint8_t*>(vb_bytes),
                                            static_cast<uint8_t*>(out.data), s_);
        }
        if (kind == Kind::Dict) {
            const uint8_t* vviews;
            VXG_TRY(canonical_views(*dvalues, &vviews, bases));
            VXG_TRY(launch_take_views(vviews, dvalues->len, tcodes, cw, false, n, tix, nullptr, 0, valid, views, err, s_));
        } else if (kind == Kind::View) {
            void* dbufs;
            VXG_TRY(temp(vbufs.size() * sizeof(StrBuf), &dbufs));
            if (!vbufs.empty())
                VXG_TRY(hip_check(hipMemcpyAsync(dbufs, vbufs.data(), vbufs.size() * sizeof(StrBuf), hipMemcpyHostToDevice, s_),
                                  "take buffer table upload"));
            for (const StrBuf& b : vbufs) bases.push_back(b.p);
            VXG_TRY(launch_take_views(static_cast<const uint8_t*>(src_views), a.len, idx, iw, isg, n, TakeIdx{},
                                      static_cast<const StrBuf*>(dbufs), uint32_t(vbufs.size()), valid, views, err, s_));
        } else {
            const uint8_t* cviews;
            VXG_TRY(canonical_views(a, &cviews, bases));
            VXG_TRY(launch_take_views(cviews, a.len, idx, iw, isg, n, TakeIdx{}, nullptr, 0, valid, views, err, s_));
        }
        void* dbases;
        VXG_TRY(temp(bases.size() * sizeof(void*) + 8, &dbases));
        if (!bases.empty())
            VXG_TRY(hip_check(hipMemcpyAsync(dbases, bases.data(), bases.size() * sizeof(void*), hipMemcpyHostToDevice, s_),
                              "take buffer table upload"));
        VXG_TRY(launch_view_heap_sizes(views, n, valid, static_cast<uint64_t*>(hoff), s_));
        VXG_TRY(read_total(static_cast<uint64_t*>(hoff) + ktiles, &heap));
        VXG_TRY(size_heap(heap));
        return launch_view_heap_build(views, n, valid, static_cast<const uint64_t*>(hoff),
                                      static_cast<const uint8_t* const*>(dbases), uint32_t(bases.size()),
                                      static_cast<uint8_t*>(out.data), err, s_);
    };
    const vxg_status st = rows();
    // complete on return -- and, on an error too, nothing still reads `vbufs` / `bases`
    const vxg_status sync = hip_check(hipStreamSynchronize(s_), "take sync");
    return st != VXG_OK ? st : sync;
}

// ---- compute::compare with a scalar (vortex-array/src/compute/compare.rs:81-124) ----------
// Is `a` a cascade the fused kernel serves -- BitPacked, FoR(BitPacked), ZigZag or ALP over
// either?  Then validate its packed buffer exactly like take_values and describe it.
vxg_status Planner::compare_shape(const vxg_array& a, uint64_t out_bit, CmpFused& f, bool* fused) {
    *fused = false;
    f = CmpFused{};
    f.arr = &a;
    f.epi = Epi::Plain;
    f.ck = ptype_is_signed(a.ptype) ? kCmpSigned : kCmpUnsigned;
    auto fl_child = [&](const vxg_array* c) -> const vxg_array* {  // FoR(BitPacked) or BitPacked
        if (c && c->encoding == VXG_ENC_FL_FOR && child(*c, 0) && child(*c, 0)->encoding == VXG_ENC_FL_BITPACKED) {
            f.ep.reference = c->meta.for_.reference;
            f.ep.shift = c->meta.for_.shift;
            return child(*c, 0);
        }
        return c && c->encoding == VXG_ENC_FL_BITPACKED ? c : nullptr;
    };
    switch (a.encoding) {
    case VXG_ENC_FL_BITPACKED: f.bp = &a; break;
    case VXG_ENC_FL_FOR:
        f.bp = fl_child(&a);
        f.epi = Epi::For;
        break;
    case VXG_ENC_ZIGZAG:
        if (!ptype_is_signed(a.ptype)) return VXG_OK;  // the fallback reports it
        f.bp = fl_child(child(a, 0));
        f.epi = Epi::ForZigZag;
        break;
    case VXG_ENC_ALP: {
        const bool f32 = a.ptype == VXG_F32;
        const unsigned e = a.meta.alp.e, fx = a.meta.alp.f;
        if ((f32 && (e > 10 || fx > 10)) || (!f32 && (a.ptype != VXG_F64 || e > 23 || fx > 23))) return VXG_OK;
        f.bp = fl_child(child(a, 0));
        f.epi = f32 ? Epi::AlpF32 : Epi::AlpF64;
        f.ck = kCmpFloat;
        f.ep.alp_a = f32 ? double(kF10f[fx]) : kF10d[fx];
        f.ep.alp_b = f32 ? double(kIF10f[e]) : kIF10d[e];
        if (f.bp && a.meta.alp.has_patches) {
            if (!child(a, 1)) return set_error(VXG_ERR_INVALID_ARGUMENT, "ALPArray: patches child missing");
            f.outer = child(a, 1);
        }
        break;
    }
    default: return VXG_OK;
    }
    if (!f.bp || !ptype_is_int(f.bp->ptype) || !(ptype_is_int(a.ptype) || f.ck == kCmpFloat)) return VXG_OK;
    f.T = 8 * width(*f.bp);
    if (f.T != 8 * width(a) || f.bp->len != a.len) return VXG_OK;
    const vxg_buffer* pb = buf(*f.bp, 0);
    const unsigned W = f.bp->meta.bitpacked.bit_width, off = f.bp->meta.bitpacked.offset;
    if (off > 1023) return set_error(VXG_ERR_INVALID_ARGUMENT, "Offset must be less than full block, i.e. 1024");
    if (W > unsigned(f.T)) return set_error(VXG_ERR_INVALID_ARGUMENT, "Unsupported bit width");
    const uint64_t nblk = (a.len + off + 1023) / 1024, have = pb ? pb->len : 0;
    if (W > 0 && have != nblk * 128ull * W)  // bitpacking/mod.rs:80-88
        return set_error(VXG_ERR_INVALID_ARGUMENT, "Expected " + std::to_string(nblk * 128ull * W) +
                                                       " packed bytes, got " + std::to_string(have));
    if (W > 0 && (reinterpret_cast<uintptr_t>(pb->ptr) & 15))
        return set_error(VXG_ERR_INVALID_ARGUMENT, "packed buffer must be 16-byte aligned");
    if (a.len > kCmpMaxLen) return set_error(VXG_ERR_INVALID_ARGUMENT, "array too long for one compare launch");
    // patch children are checked here, before the caller allocates or launches anything
    auto patch_values = [&](const vxg_array& sp) -> const vxg_array* {
        return sp.encoding == VXG_ENC_SPARSE && child(sp, 0) && child(sp, 1) ? child(sp, 1) : nullptr;
    };
    if (f.bp->meta.bitpacked.has_patches) {
        if (!child(*f.bp, 0)) return set_error(VXG_ERR_INVALID_ARGUMENT, "BitPacked patches child missing");
        const vxg_array* pv = patch_values(*child(*f.bp, 0));
        if (pv && width(*pv) != f.T / 8)
            return set_error(VXG_ERR_MISMATCHED_TYPES, "BitPacked patch values must have the array's width");
    }
    if (f.outer) {
        const vxg_array* pv = patch_values(*f.outer);
        if (pv && pv->ptype != a.ptype)
            return set_error(VXG_ERR_MISMATCHED_TYPES, "ALP patch values must have the array's ptype");
    }
    f.ep.err = ctx_->c.err_word;
    f.d.packed = pb ? static_cast<const uint8_t*>(pb->ptr) : nullptr;
    f.d.len_lo = uint32_t(a.len);
    f.d.len_hi = uint8_t(a.len >> 32);
    f.d.out_bit = out_bit;
    f.d.reference = f.ep.reference;
    f.d.alp_e = a.encoding == VXG_ENC_ALP ? a.meta.alp.e : 0;
    f.d.alp_f = a.encoding == VXG_ENC_ALP ? a.meta.alp.f : 0;
    f.d.offset = uint16_t(off);
    f.d.shift = uint8_t(f.ep.shift);
    f.d.W = uint8_t(W);
    *fused = true;
    return VXG_OK;
}

// The chunks of one kernel instantiation (T, epilogue, compared type; at most kCmpArgChunks) in one
// launch: the table is the kernel argument -- nothing is uploaded and no host state outlives the call.
vxg_status Planner::launch_compare_group(std::vector<CmpFused*>& group, void* out, uint64_t scalar_bits, int op,
                                         const CmpRange* range) {
    uint64_t blocks = 0;
    for (const CmpFused* f : group) blocks += f->d.n_blocks();
    // small launches take fewer blocks per workgroup (>= 4: one per wave), like K1w's rule
    uint32_t pick = uint32_t(std::min<uint64_t>(32, blocks / 1024)) & ~3u;
    if (pick < 4) pick = 4;
    CmpTable tab{};
    uint64_t groups = 0;
    uint32_t lds = 0;
    for (const CmpFused* f : group) {
        CmpChunk& c = tab.c[tab.n++];
        c = f->d;
        const uint32_t bpw = std::min(cmp_bpw_max(c.W), pick);
        c.bpw_excl = uint8_t(bpw | (f->excl ? 0x80u : 0u));
        c.first_group = uint32_t(groups);
        groups += (c.n_blocks() + bpw - 1) / bpw;
        lds = std::max(lds, bpw * 128u * c.W);
    }
    if (groups == 0) groups = 1;  // an empty array: one workgroup that finds no block
    const CmpFused& f0 = *group[0];
    // (+ one word row of slack: a value's second word is read unconditionally)
    if (range) return launch_cmp_range_packed(f0.T, f0.epi, f0.ck, tab, groups, lds + 128, out, *range, s_);
    return launch_cmp_packed(f0.T, f0.epi, f0.ck, tab, groups, lds + 128, out, scalar_bits, op, s_);
}

vxg_status Planner::compare(const vxg_array& a, int op, uint64_t scalar_bits, uint32_t flags, vxg_canonical& out,
                            vxg_compare_info& info) {
    return compare_impl(a, op, scalar_bits, nullptr, flags, out, info);
}

// compare(), or with `range` the two tests of a range on one column in the same walk (row_filter):
// every launch is then the two-sided twin of the one a single compare issues (op and scalar_bits
// are not looked at).
vxg_status Planner::compare_impl(const vxg_array& a, int op, uint64_t scalar_bits, const CmpRange* range, uint32_t flags,
                                 vxg_canonical& out, vxg_compare_info& info) {
    if (a.dtype != VXG_DTYPE_PRIMITIVE) return set_error(VXG_ERR_NOT_IMPLEMENTED, "compare supports primitive arrays");
    if (width(a) == 0 || a.ptype == VXG_F16) return set_error(VXG_ERR_NOT_IMPLEMENTED, "compare does not support f16");
    if (!range && (op < VXG_CMP_EQ || op > VXG_CMP_LTE))
        return set_error(VXG_ERR_INVALID_ARGUMENT, "unknown compare operator " + std::to_string(op));
    if (flags & ~uint32_t(VXG_CMP_NULL_AS_FALSE)) return set_error(VXG_ERR_INVALID_ARGUMENT, "unknown compare flags");
    const uint64_t n = a.len, words = (n + 63) / 64, bytes = words * 8;

    // the pieces: the array itself, or the chunks of a top-level ChunkedArray at their bit offsets
    std::vector<std::pair<const vxg_array*, uint64_t>> pieces;
    if (a.encoding == VXG_ENC_CHUNKED) {
        if (a.n_children != a.meta.chunked.nchunks + 1)
            return set_error(VXG_ERR_INVALID_ARGUMENT, "Chunked child count != nchunks + 1");
        uint64_t off = 0;
        for (uint32_t i = 1; i < a.n_children; i++) {
            const vxg_array& c = a.children[i];
            if (c.dtype != a.dtype || c.ptype != a.ptype)
                return set_error(VXG_ERR_MISMATCHED_TYPES, "Chunks must have the same dtype");
            pieces.emplace_back(&c, off);
            off += c.len;
        }
        if (off != n) return set_error(VXG_ERR_INVALID_ARGUMENT, "Chunked chunk lengths do not sum to len");
    } else {
        pieces.emplace_back(&a, 0);
    }
    // classify and validate every piece before anything is allocated or launched
    std::vector<CmpFused> fused;
    std::vector<std::pair<const vxg_array*, uint64_t>> plain;
    fused.reserve(pieces.size());
    bool zero = false;  // some word is ORed in: the bitmap starts zeroed
    auto word_edges = [&](uint64_t ob, uint64_t len) { return ob % 64 == 0 && ((ob + len) % 64 == 0 || ob + len == n); };
    for (const auto& [p, ob] : pieces) {
        CmpFused f;
        bool is_fused;
        VXG_TRY(compare_shape(*p, ob, f, &is_fused));
        if (is_fused) {
            f.excl = word_edges(ob, p->len) && f.d.offset % 64 == 0;
            if (p->len == 0 && p != &a) {  // an empty chunk: counted, nothing to launch
                info.fused_chunks++;
                continue;
            }
            zero = zero || (p->len && !f.excl);
            fused.push_back(f);
        } else {
            zero = zero || (p->len && !word_edges(ob, p->len));
            plain.emplace_back(p, ob);
        }
    }

    out.kind = VXG_ENC_BOOL;
    out.len = n;
    out.dtype = VXG_DTYPE_BOOL;
    out.ptype = VXG_U8;
    out.values_bytes = bytes;
    if (!out.values) VXG_TRY(hip_check(hipMalloc(&out.values, bytes ? bytes : 8), "compare values alloc"));
    if (reinterpret_cast<uintptr_t>(out.values) & 7)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "compare output must be 8-byte aligned");
    if (zero) VXG_TRY(launch_copy_bytes(out.values, nullptr, bytes, s_));

    // fused launches, one per kernel instantiation
    std::vector<CmpFused*> order;
    for (CmpFused& f : fused) order.push_back(&f);
    std::stable_sort(order.begin(), order.end(), [](const CmpFused* x, const CmpFused* y) {
        return std::make_tuple(x->T, int(x->epi), x->ck) < std::make_tuple(y->T, int(y->epi), y->ck);
    });
    for (size_t i = 0; i < order.size();) {
        size_t j = i;
        while (j < order.size() && j - i < size_t(kCmpArgChunks) && order[j]->T == order[i]->T &&
               order[j]->epi == order[i]->epi && order[j]->ck == order[i]->ck)
            j++;
        std::vector<CmpFused*> group(order.begin() + i, order.begin() + j);
        VXG_TRY(launch_compare_group(group, out.values, scalar_bits, op, range));
        info.fused_launches++;
        info.fused_chunks += uint32_t(j - i);
        i = j;
    }
    // patched rows are compared again: BitPacked's raw values through the epilogue, then ALP's
    for (const CmpFused& f : fused) {
        if (f.bp->meta.bitpacked.has_patches) {
            TakePatches tp;
            VXG_TRY(take_patches(*child(*f.bp, 0), tp));
            if (range) VXG_TRY(launch_cmp_range_patch(f.T, f.epi, f.ck, tp, f.d.len(), out.values, f.d.out_bit, f.ep, *range, s_));
            else VXG_TRY(launch_cmp_patch(f.T, f.epi, f.ck, tp, f.d.len(), out.values, f.d.out_bit, f.ep, scalar_bits, op, s_));
            info.patch_launches += tp.n != 0;
        }
        if (f.outer) {
            TakePatches tp;
            VXG_TRY(take_patches(*f.outer, tp));
            if (range)
                VXG_TRY(launch_cmp_range_patch_raw(a.ptype, tp, f.d.len(), out.values, f.d.out_bit, *range, ctx_->c.err_word, s_));
            else
                VXG_TRY(launch_cmp_patch_raw(a.ptype, tp, f.d.len(), out.values, f.d.out_bit, scalar_bits, op, ctx_->c.err_word,
                                             s_));
            info.patch_launches += tp.n != 0;
        }
    }
    // every other encoding: the canonical values (a Primitive array in place), then the plain kernel
    for (const auto& [p, ob] : plain) {
        const void* pv;
        VXG_TRY(view_primitive(*p, &pv));
        if (reinterpret_cast<uintptr_t>(pv) % uint64_t(width(a)))
            return set_error(VXG_ERR_INVALID_ARGUMENT, "primitive buffer must be aligned to the value width");
        if (range) VXG_TRY(launch_cmp_range_plain(a.ptype, pv, p->len, out.values, ob, *range, word_edges(ob, p->len), s_));
        else VXG_TRY(launch_cmp_plain(a.ptype, pv, p->len, out.values, ob, scalar_bits, op, word_edges(ob, p->len), s_));
        info.fallback_arrays++;
    }

    // value bits of null rows are 0; null_as_false drops the validity (filtering.rs:42)
    const vxg_array* vnode;
    int vkind;
    VXG_TRY(validity_source(a, &vnode, &vkind));
    const bool null_as_false = (flags & VXG_CMP_NULL_AS_FALSE) != 0;
    if (vkind == 0) {
        out.validity = nullptr;
        return VXG_OK;
    }
    void* vbits = nullptr;
    if (null_as_false) VXG_TRY(temp(bytes, &vbits));
    else if (out.validity) vbits = out.validity;
    else {
        VXG_TRY(hip_check(hipMalloc(&vbits, bytes ? bytes : 8), "compare validity alloc"));
        out.validity = vbits;  // (the entry point releases it if a later step fails)
    }
    if (reinterpret_cast<uintptr_t>(vbits) & 7)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "compare validity must be 8-byte aligned");
    if (n) {  // (an empty array's bitmaps hold no bytes: nothing is written)
        VXG_TRY(launch_copy_bytes(vbits, nullptr, bytes, s_));
        VXG_TRY(validity_into(a, &vbits));
        VXG_TRY(launch_and_words(out.values, vbits, words, s_));
    }
    out.validity = null_as_false ? nullptr : vbits;
    return VXG_OK;
}

// ---- RowFilter::evaluate (vortex-serde/src/layouts/read/filtering.rs:27-43) ----------------
// One pass per conjunct -- or per range pair -- each into its own bitmap with null_as_false, then
// the AND of the bitmaps (K21, compare_range.hip), which also takes the true count.  Nothing is
// read back: the reference's early return at a zero count gives the same bits.
vxg_status Planner::row_filter(const vxg_predicate* preds, uint32_t n_preds, uint32_t flags, vxg_canonical& out,
                               uint64_t* count_dev, vxg_row_filter_info& info) {
    const uint64_t n = preds[0].column->len, words = (n + 63) / 64, bytes = words * 8;
    info.predicates = n_preds;

    // pairing: per primitive column node, the i-th lower bound with the i-th upper bound in list order
    struct Pass { uint32_t a, b; };  // conjunct a alone (b == a), or the range (lower a, upper b)
    constexpr uint32_t kNone = ~0u;
    std::vector<uint32_t> mate(n_preds, kNone);
    if (!(flags & VXG_ROWF_NO_FUSE_RANGES)) {  // (flags 0: the default is to pair)
        auto lower = [&](uint32_t i) { return preds[i].op == VXG_CMP_GT || preds[i].op == VXG_CMP_GTE; };
        auto upper = [&](uint32_t i) { return preds[i].op == VXG_CMP_LT || preds[i].op == VXG_CMP_LTE; };
        for (uint32_t i = 0; i < n_preds; i++) {
            if (mate[i] != kNone || preds[i].column->dtype != VXG_DTYPE_PRIMITIVE || !(lower(i) || upper(i))) continue;
            for (uint32_t j = i + 1; j < n_preds; j++) {  // the first unpaired bound of the other side
                if (mate[j] != kNone || preds[j].column != preds[i].column) continue;
                if (lower(i) ? !upper(j) : !lower(j)) continue;
                // i is the first unpaired bound of its side: an earlier one would have taken j
                mate[i] = j;
                mate[j] = i;
                break;
            }
        }
    }
    std::vector<Pass> passes;
    for (uint32_t i = 0; i < n_preds; i++) {
        if (mate[i] == kNone) passes.push_back({i, i});
        else if (mate[i] > i) {
            const bool lo_first = preds[i].op == VXG_CMP_GT || preds[i].op == VXG_CMP_GTE;
            passes.push_back(lo_first ? Pass{i, mate[i]} : Pass{mate[i], i});
        }
    }
    info.range_pairs = n_preds - uint32_t(passes.size());
    info.compare_passes = uint32_t(passes.size());

    out.kind = VXG_ENC_BOOL;
    out.len = n;
    out.dtype = VXG_DTYPE_BOOL;
    out.ptype = VXG_U8;
    out.values_bytes = bytes;
    out.validity = nullptr;
    if (!out.values) VXG_TRY(hip_check(hipMalloc(&out.values, bytes ? bytes : 8), "row filter values alloc"));
    if (reinterpret_cast<uintptr_t>(out.values) & 7)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "row filter output must be 8-byte aligned");

    auto scalar_bits = [](const vxg_predicate& p) {
        uint64_t bits = 0;
        std::memcpy(&bits, p.scalar_host, size_t(ptype_width(p.column->ptype)));
        return bits;
    };
    // the passes' bitmaps: one temporary for all of them, each on a 16-byte boundary
    const uint64_t slot = (bytes + 15) & ~15ull;
    void* slab = nullptr;
    if (passes.size() > 1) VXG_TRY(temp(slot * passes.size(), &slab));
    std::vector<void*> bitmaps;
    for (const Pass& ps : passes) {
        const vxg_predicate& p = preds[ps.a];
        vxg_canonical c{};
        // (a single pass: its bitmap is the output)
        c.values = slab ? static_cast<uint8_t*>(slab) + slot * bitmaps.size() : out.values;
        bitmaps.push_back(c.values);
        if (is_string(*p.column)) {
            vxg_compare_bytes_info bi{};
            VXG_TRY(compare_bytes(*p.column, p.op, p.scalar_host, p.scalar_len, VXG_CMP_NULL_AS_FALSE, c, bi));
            info.fused_launches += bi.dict_launches;
            info.fallback_arrays += bi.fallback_arrays;
            continue;
        }
        vxg_compare_info ci{};
        if (ps.b != ps.a) {
            const CmpRange r{scalar_bits(p), scalar_bits(preds[ps.b]), p.op, preds[ps.b].op};
            VXG_TRY(compare_impl(*p.column, 0, 0, &r, VXG_CMP_NULL_AS_FALSE, c, ci));
            info.range_launches += ci.fused_launches;
        } else {
            VXG_TRY(compare_impl(*p.column, p.op, scalar_bits(p), nullptr, VXG_CMP_NULL_AS_FALSE, c, ci));
        }
        info.fused_launches += ci.fused_launches;
        info.fallback_arrays += ci.fallback_arrays;
    }
    if (bitmaps.size() == 1 && !count_dev) return VXG_OK;

    if (count_dev) VXG_TRY(launch_copy_bytes(count_dev, nullptr, 8, s_));
    // up to 16 bitmaps per launch, the running output among them from the second launch on; only
    // the last launch counts (an earlier one would count rows a later bitmap still clears)
    for (size_t i = 0; i < bitmaps.size();) {
        AndInputs in{};
        if (i) in.p[in.k++] = static_cast<const uint64_t*>(out.values);
        while (in.k < uint32_t(kAndInputs) && i < bitmaps.size()) in.p[in.k++] = static_cast<const uint64_t*>(bitmaps[i++]);
        VXG_TRY(launch_and_count(in, out.values, words, i == bitmaps.size() ? count_dev : nullptr, s_));
        info.combine_launches += words != 0;
    }
    return VXG_OK;
}

// ---- compute::compare of strings with a scalar (compare_str.hip) ---------------------------
// The rows of string array `s` (a piece, or the values of a Dict piece) as a piece of the row
// kernels, at bit out_bit of their target.  VarBin, VarBinView and FSST are read where they lie;
// anything else is canonicalized into temporaries and compared as a VarBinView (*fell_back).
// `table`: the target is a truth table (out_bit on a word, every word exclusive), so a VarBin
// with plain offsets takes the 40-byte form.
vxg_status Planner::compare_rows_of(const vxg_array& s, uint64_t out_bit, bool excl, bool table, StrRows& rows,
                                    bool* fell_back) {
    *fell_back = false;
    if (!is_string(s)) return set_error(VXG_ERR_MISMATCHED_TYPES, "compare: expected a utf8 or binary array");
    if (s.len == 0) return VXG_OK;
    auto bytes_of = [&](const vxg_array& b, const void** p) -> vxg_status {
        if (b.dtype != VXG_DTYPE_PRIMITIVE || width(b) != 1)
            return set_error(VXG_ERR_MISMATCHED_TYPES, "string bytes must be a u8 array");
        return view_primitive(b, p);
    };
    auto view_piece = [&](const void* views, const std::vector<StrBuf>& bufs) -> vxg_status {
        if (reinterpret_cast<uintptr_t>(views) & 15)
            return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBinView views must be 16-byte aligned");
        ViewPiece p{};
        p.views = static_cast<const uint8_t*>(views);
        p.n_buffers = uint32_t(bufs.size());
        if (bufs.size() == 1) p.buf0 = bufs[0];
        if (bufs.size() > 1) {  // a device table of the buffers, like Planner::filter's
            void* d;
            VXG_TRY(temp(bufs.size() * sizeof(StrBuf), &d));
            VXG_TRY(hip_check(hipMemcpyAsync(d, bufs.data(), bufs.size() * sizeof(StrBuf), hipMemcpyHostToDevice, s_),
                              "compare buffer table upload"));
            VXG_TRY(hip_check(hipStreamSynchronize(s_), "compare buffer table sync"));  // `bufs` is read by the upload
            p.bufs = static_cast<const StrBuf*>(d);
        }
        p.out_bit = out_bit;
        p.n = s.len;
        p.excl = excl;
        rows.vw.push_back(p);
        return VXG_OK;
    };
    switch (s.encoding) {
    case VXG_ENC_VARBIN: {
        const vxg_array* offs = child(s, 0);
        const vxg_array* bytes = child(s, 1);
        if (!offs || !bytes) return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBinArray needs offsets and bytes");
        if (!ptype_is_int(offs->ptype) || offs->dtype != VXG_DTYPE_PRIMITIVE)
            return set_error(VXG_ERR_MISMATCHED_TYPES, "VarBin offsets must be integers");
        if (offs->len < s.len + 1) return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBin offsets shorter than len + 1");
        const void* pb;
        VXG_TRY(bytes_of(*bytes, &pb));
        if (table && offs->encoding == VXG_ENC_PRIMITIVE && bytes->len <= 0xFFFFFFFFull && s.len <= 0xFFFFFFFFull &&
            out_bit % 64 == 0 && out_bit / 64 <= 0xFFFFFFFFull) {
            const void* po;
            VXG_TRY(view_primitive(*offs, &po));
            if (reinterpret_cast<uintptr_t>(po) % uint64_t(width(*offs)))
                return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBin offsets must be aligned to their width");
            VbDictPiece p{};
            p.bytes = static_cast<const uint8_t*>(pb);
            p.offs = po;
            p.bytes_len = uint32_t(bytes->len);
            p.out_word = uint32_t(out_bit / 64);
            p.n = uint32_t(s.len);
            p.width = uint8_t(width(*offs));
            p.sgn = ptype_is_signed(offs->ptype);
            rows.vbd.push_back(p);
            return VXG_OK;
        }
        IntCol oc;
        VXG_TRY(int_column(*offs, oc));
        if (reinterpret_cast<uintptr_t>(oc.p) % uint64_t(oc.packed ? 16 : oc.width))
            return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBin offsets must be aligned to their width");
        VbPiece p{};
        p.bytes = static_cast<const uint8_t*>(pb);
        p.bytes_len = bytes->len;
        p.offs = to_ccol(oc);
        p.out_bit = out_bit;
        p.n = s.len;
        p.excl = excl;
        rows.vb.push_back(p);
        return VXG_OK;
    }
    case VXG_ENC_VARBINVIEW: {
        const vxg_array* vw = child(s, 0);
        const uint32_t nb = s.meta.varbinview.n_buffers;
        if (!vw || s.n_children < 1 + nb)
            return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBinViewArray: missing views/data buffers");
        const void* pv;
        VXG_TRY(bytes_of(*vw, &pv));
        if (vw->len < 16 * s.len) return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBinView views shorter than 16 * len");
        std::vector<StrBuf> bufs(nb);
        for (uint32_t b = 0; b < nb; b++) {
            const void* pb;
            VXG_TRY(bytes_of(s.children[1 + b], &pb));
            bufs[b] = StrBuf{static_cast<const uint8_t*>(pb), s.children[1 + b].len};
        }
        return view_piece(pv, bufs);
    }
    case VXG_ENC_FSST: {
        const vxg_array* sym = child(s, 0);
        const vxg_array* slen = child(s, 1);
        const vxg_array* codes = child(s, 2);
        const vxg_array* ulen = child(s, 3);
        if (!sym || !slen || !codes || !ulen || codes->encoding != VXG_ENC_VARBIN || !child(*codes, 0) || !child(*codes, 1))
            return set_error(VXG_ERR_INVALID_ARGUMENT, "FSSTArray needs symbols, lengths, VarBin codes, lengths");
        if (sym->len > 255 || slen->len < sym->len || width(*sym) != 8 || width(*slen) != 1)
            return set_error(VXG_ERR_INVALID_ARGUMENT, "FSST symbol table must hold at most 255 u64 symbols and their u8 lengths");
        if (codes->len != s.len || ulen->len < s.len || child(*codes, 0)->len < s.len + 1)
            return set_error(VXG_ERR_INVALID_ARGUMENT, "FSST codes / lengths do not cover the array");
        if (!ptype_is_int(child(*codes, 0)->ptype) || !ptype_is_int(ulen->ptype))
            return set_error(VXG_ERR_MISMATCHED_TYPES, "FSST offsets and lengths must be integers");
        const void *psym, *pslen, *pcb;
        VXG_TRY(view_primitive(*sym, &psym));
        VXG_TRY(view_primitive(*slen, &pslen));
        VXG_TRY(bytes_of(*child(*codes, 1), &pcb));
        if (reinterpret_cast<uintptr_t>(psym) & 7) return set_error(VXG_ERR_INVALID_ARGUMENT, "FSST symbols must be 8-byte aligned");
        IntCol oc, lc;
        VXG_TRY(int_column(*child(*codes, 0), oc));
        VXG_TRY(int_column(*ulen, lc));
        if (reinterpret_cast<uintptr_t>(oc.p) % uint64_t(oc.packed ? 16 : oc.width) ||
            reinterpret_cast<uintptr_t>(lc.p) % uint64_t(lc.packed ? 16 : lc.width))
            return set_error(VXG_ERR_INVALID_ARGUMENT, "FSST offsets / lengths must be aligned to their width");
        FsstPiece p{};
        p.symbols = static_cast<const uint64_t*>(psym);
        p.sym_lens = static_cast<const uint8_t*>(pslen);
        p.codes = static_cast<const uint8_t*>(pcb);
        p.codes_len = child(*codes, 1)->len;
        p.offs = to_ccol(oc);
        p.lens = to_ccol(lc);
        p.out_bit = out_bit;
        p.n = s.len;
        p.excl = excl;
        p.n_symbols = uint32_t(sym->len);
        rows.fs.push_back(p);
        return VXG_OK;
    }
    default: {
        // canonical views + data in temporaries (as Planner::filter builds its source)
        *fell_back = true;
        vxg_canonical src{};
        std::vector<vxg_data_buffer> lay;
        uint64_t extent;
        VXG_TRY(string_layout(s, lay, extent));
        const vxg_array* vnode;
        int vkind;
        VXG_TRY(validity_source(s, &vnode, &vkind));
        if (vkind != 0) VXG_TRY(temp(((s.len + 31) / 32) * 4, &src.validity));
        VXG_TRY(temp(16 * s.len, &src.views));
        VXG_TRY(temp(extent + 16, &src.data));
        src.data_bytes = extent;
        src.data_buffers = lay.data();
        src.n_data_buffers = src.data_buffers_cap = uint32_t(lay.size());
        VXG_TRY(string_canonical(s, src));
        std::vector<StrBuf> bufs(lay.size());
        for (size_t b = 0; b < lay.size(); b++)
            bufs[b] = StrBuf{static_cast<const uint8_t*>(src.data) + lay[b].offset, lay[b].len};
        return view_piece(src.views, bufs);
    }
    }
}

// Every piece of `rows` into `out`: one launch per kind and per kernel-argument table.
vxg_status Planner::launch_str_rows(StrRows& rows, const StrScalar& sc, void* out, int op, uint32_t& launches) {
    uint32_t* err = ctx_->c.err_word;
    auto run = [&](auto& v, auto tab, auto groups_of, auto launch) -> vxg_status {
        constexpr size_t cap = sizeof(tab.c) / sizeof(tab.c[0]);
        for (size_t i = 0; i < v.size(); i += cap) {
            tab.n = 0;
            uint64_t groups = 0;
            for (size_t k = i; k < v.size() && k < i + cap; k++) {
                v[k].first_group = uint32_t(groups);
                groups += groups_of(v[k]);
                tab.c[tab.n++] = v[k];
            }
            VXG_TRY(launch(tab, groups));
            launches++;
        }
        return VXG_OK;
    };
    VXG_TRY(run(rows.vbd, VbDictTab{}, [](const VbDictPiece& p) { return piece_groups(0, p.n); },
                [&](const VbDictTab& t, uint64_t g) { return launch_cmpb_varbin_dict(t, g, sc, out, err, op, s_); }));
    VXG_TRY(run(rows.vb, VbTab{}, [](const VbPiece& p) { return piece_groups(p.out_bit, p.n); },
                [&](const VbTab& t, uint64_t g) { return launch_cmpb_varbin(t, g, sc, out, err, op, s_); }));
    VXG_TRY(run(rows.vw, ViewTab{}, [](const ViewPiece& p) { return piece_groups(p.out_bit, p.n); },
                [&](const ViewTab& t, uint64_t g) { return launch_cmpb_views(t, g, sc, out, err, op, s_); }));
    VXG_TRY(run(rows.fs, FsstTab{}, [](const FsstPiece& p) { return piece_groups(p.out_bit, p.n); },
                [&](const FsstTab& t, uint64_t g) { return launch_cmpb_fsst(t, g, sc, out, err, op, s_); }));
    return VXG_OK;
}

vxg_status Planner::compare_bytes(const vxg_array& a, int op, const void* scalar_host, uint64_t scalar_len, uint32_t flags,
                                  vxg_canonical& out, vxg_compare_bytes_info& info) {
    if (!is_string(a)) return set_error(VXG_ERR_MISMATCHED_TYPES, "compare_bytes needs a utf8 or binary array");
    if (op < VXG_CMP_EQ || op > VXG_CMP_LTE)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "unknown compare operator " + std::to_string(op));
    if (flags & ~uint32_t(VXG_CMP_NULL_AS_FALSE)) return set_error(VXG_ERR_INVALID_ARGUMENT, "unknown compare flags");
    if (a.len > kCmpMaxLen) return set_error(VXG_ERR_INVALID_ARGUMENT, "array too long for one compare launch");
    const uint64_t n = a.len, words = (n + 63) / 64, bytes = words * 8;

    // the pieces: the array itself, or the chunks of a top-level ChunkedArray at their bit offsets
    std::vector<std::pair<const vxg_array*, uint64_t>> pieces;
    if (a.encoding == VXG_ENC_CHUNKED) {
        if (a.n_children != a.meta.chunked.nchunks + 1)
            return set_error(VXG_ERR_INVALID_ARGUMENT, "Chunked child count != nchunks + 1");
        uint64_t off = 0;
        for (uint32_t i = 1; i < a.n_children; i++) {
            const vxg_array& c = a.children[i];
            if (c.dtype != a.dtype) return set_error(VXG_ERR_MISMATCHED_TYPES, "Chunks must have the same dtype");
            pieces.emplace_back(&c, off);
            off += c.len;
        }
        if (off != n) return set_error(VXG_ERR_INVALID_ARGUMENT, "Chunked chunk lengths do not sum to len");
    } else {
        pieces.emplace_back(&a, 0);
    }

    // classify and validate every piece before the output is allocated or a compare is launched
    struct DictPacked {
        int T;
        CmpChunk d;
        bool excl;
    };
    StrRows table_rows, out_rows;
    std::vector<DictPacked> packed;
    std::vector<DictPlainPiece> plain;
    uint64_t tt_words = 0;
    bool zero = false;  // some word is ORed in: the bitmap starts zeroed
    auto word_edges = [&](uint64_t ob, uint64_t len) { return ob % 64 == 0 && ((ob + len) % 64 == 0 || ob + len == n); };
    for (const auto& [p, ob] : pieces) {
        const bool edges = word_edges(ob, p->len);
        bool fell = false;
        if (p->encoding != VXG_ENC_DICT) {
            VXG_TRY(compare_rows_of(*p, ob, edges, false, out_rows, &fell));
            if (fell) info.fallback_arrays++;
            else info.direct_chunks++;
            zero = zero || (p->len && !edges);
            continue;
        }
        const vxg_array* values = child(*p, 0);
        const vxg_array* codes = child(*p, 1);
        if (!values || !codes) return set_error(VXG_ERR_INVALID_ARGUMENT, "DictArray needs values and codes");
        if (!ptype_is_int(codes->ptype) || codes->dtype != VXG_DTYPE_PRIMITIVE)
            return set_error(VXG_ERR_MISMATCHED_TYPES, "Dict codes must be integers");
        if (codes->len != p->len) return set_error(VXG_ERR_INVALID_ARGUMENT, "Dict codes length != array length");
        if (values->len > 0xFFFFFFFFull) return set_error(VXG_ERR_NOT_IMPLEMENTED, "compare: dictionary of 2^32 or more values");
        info.dict_chunks++;
        if (p->len == 0) continue;  // an empty chunk: counted, nothing to launch
        const uint64_t tword = tt_words;
        if (tword > 0xFFFFFFFFull) return set_error(VXG_ERR_NOT_IMPLEMENTED, "compare: truth tables exceed 2^32 words");
        tt_words += std::max<uint64_t>(1, (values->len + 63) / 64);
        // (a) the truth table: the dictionary's values, compared like any string array
        VXG_TRY(compare_rows_of(*values, tword * 64, true, true, table_rows, &fell));
        if (fell) info.fallback_arrays++;
        // (b) the lookup
        const int T = 8 * width(*codes);
        if (codes->encoding == VXG_ENC_FL_BITPACKED && ptype_is_unsigned(codes->ptype) && !codes->meta.bitpacked.has_patches) {
            const vxg_buffer* pb = buf(*codes, 0);
            const unsigned W = codes->meta.bitpacked.bit_width, off = codes->meta.bitpacked.offset;
            if (off > 1023) return set_error(VXG_ERR_INVALID_ARGUMENT, "Offset must be less than full block, i.e. 1024");
            if (W > unsigned(T)) return set_error(VXG_ERR_INVALID_ARGUMENT, "Unsupported bit width");
            const uint64_t nblk = (p->len + off + 1023) / 1024, have = pb ? pb->len : 0;
            if (W > 0 && have != nblk * 128ull * W)  // bitpacking/mod.rs:80-88
                return set_error(VXG_ERR_INVALID_ARGUMENT, "Expected " + std::to_string(nblk * 128ull * W) +
                                                               " packed bytes, got " + std::to_string(have));
            if (W > 0 && (reinterpret_cast<uintptr_t>(pb->ptr) & 15))
                return set_error(VXG_ERR_INVALID_ARGUMENT, "packed buffer must be 16-byte aligned");
            DictPacked dp{};
            dp.T = T;
            dp.d.packed = pb ? static_cast<const uint8_t*>(pb->ptr) : nullptr;
            dp.d.reference = tword | uint64_t(values->len) << 32;
            dp.d.out_bit = ob;
            dp.d.len_lo = uint32_t(p->len);
            dp.d.len_hi = uint8_t(p->len >> 32);
            dp.d.offset = uint16_t(off);
            dp.d.W = uint8_t(W);
            dp.excl = edges && off % 64 == 0;
            zero = zero || !dp.excl;
            packed.push_back(dp);
        } else {  // a Primitive array in place; any other encoding through a temporary
            const void* pc;
            VXG_TRY(view_primitive(*codes, &pc));
            if (reinterpret_cast<uintptr_t>(pc) % uint64_t(width(*codes)))
                return set_error(VXG_ERR_INVALID_ARGUMENT, "primitive buffer must be aligned to the value width");
            DictPlainPiece d{};
            d.codes = pc;
            d.out_bit = ob;
            d.n = p->len;
            d.tword = uint32_t(tword);
            d.vlen = uint32_t(values->len);
            d.width = uint8_t(width(*codes));
            d.sgn = ptype_is_signed(codes->ptype);
            d.excl = edges;
            zero = zero || !edges;
            plain.push_back(d);
        }
    }

    // the scalar: short ones ride in the kernel argument, long ones go to a temporary
    StrScalar sc{};
    sc.len = scalar_len;
    if (scalar_len <= kStrInline) {
        if (scalar_len) std::memcpy(sc.inl, scalar_host, size_t(scalar_len));
    } else {
        void* d;
        VXG_TRY(temp(scalar_len, &d));
        VXG_TRY(hip_check(hipMemcpyAsync(d, scalar_host, scalar_len, hipMemcpyHostToDevice, s_), "compare scalar upload"));
        VXG_TRY(hip_check(hipStreamSynchronize(s_), "compare scalar sync"));  // the caller may free its bytes
        sc.dev = static_cast<const uint8_t*>(d);
    }

    out.kind = VXG_ENC_BOOL;
    out.len = n;
    out.dtype = VXG_DTYPE_BOOL;
    out.ptype = VXG_U8;
    out.values_bytes = bytes;
    if (!out.values) VXG_TRY(hip_check(hipMalloc(&out.values, bytes ? bytes : 8), "compare values alloc"));
    if (reinterpret_cast<uintptr_t>(out.values) & 7)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "compare output must be 8-byte aligned");
    if (zero) VXG_TRY(launch_copy_bytes(out.values, nullptr, bytes, s_));

    // truth tables: every dictionary starts on a 64-bit word of one temporary
    void* tt = nullptr;
    if (tt_words) {
        VXG_TRY(temp(tt_words * 8, &tt));
        VXG_TRY(launch_str_rows(table_rows, sc, tt, op, info.table_launches));
    }
    // lookups of the BitPacked codes, one launch per code width T
    std::stable_sort(packed.begin(), packed.end(), [](const DictPacked& x, const DictPacked& y) { return x.T < y.T; });
    for (size_t i = 0; i < packed.size();) {
        size_t j = i;
        uint64_t blocks = 0;
        while (j < packed.size() && j - i < size_t(kCmpArgChunks) && packed[j].T == packed[i].T) blocks += packed[j++].d.n_blocks();
        uint32_t pick = uint32_t(std::min<uint64_t>(32, blocks / 1024)) & ~3u;  // launch_compare_group's rule
        if (pick < 4) pick = 4;
        CmpTable tab{};
        uint64_t groups = 0;
        uint32_t lds = 0;
        for (size_t k = i; k < j; k++) {
            CmpChunk& c = tab.c[tab.n++];
            c = packed[k].d;
            const uint32_t bpw = std::min(cmp_bpw_max(c.W), pick);
            c.bpw_excl = uint8_t(bpw | (packed[k].excl ? 0x80u : 0u));
            c.first_group = uint32_t(groups);
            groups += (c.n_blocks() + bpw - 1) / bpw;
            lds = std::max(lds, bpw * 128u * c.W);
        }
        VXG_TRY(launch_cmpb_dict_packed(packed[i].T, tab, groups, lds + 128, out.values, tt, ctx_->c.err_word, s_));
        info.dict_launches++;
        i = j;
    }
    for (size_t i = 0; i < plain.size(); i += size_t(kStrArgPieces40)) {
        DictPlainTab tab{};
        uint64_t groups = 0;
        for (size_t k = i; k < plain.size() && k < i + size_t(kStrArgPieces40); k++) {
            plain[k].first_group = uint32_t(groups);
            groups += piece_groups(plain[k].out_bit, plain[k].n);
            tab.c[tab.n++] = plain[k];
        }
        VXG_TRY(launch_cmpb_dict_plain(tab, groups, out.values, tt, ctx_->c.err_word, s_));
        info.dict_launches++;
    }
    // VarBin / VarBinView / FSST pieces in place, and the canonicalized ones
    VXG_TRY(launch_str_rows(out_rows, sc, out.values, op, info.direct_launches));

    // value bits of null rows are 0; null_as_false drops the validity (filtering.rs:42)
    const vxg_array* vnode;
    int vkind;
    VXG_TRY(validity_source(a, &vnode, &vkind));
    const bool null_as_false = (flags & VXG_CMP_NULL_AS_FALSE) != 0;
    if (vkind == 0) {
        out.validity = nullptr;
        return VXG_OK;
    }
    void* vbits = nullptr;
    if (null_as_false) VXG_TRY(temp(bytes, &vbits));
    else if (out.validity) vbits = out.validity;
    else {
        VXG_TRY(hip_check(hipMalloc(&vbits, bytes ? bytes : 8), "compare validity alloc"));
        out.validity = vbits;  // (the entry point releases it if a later step fails)
    }
    if (reinterpret_cast<uintptr_t>(vbits) & 7)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "compare validity must be 8-byte aligned");
    if (n) {  // (an empty array's bitmaps hold no bytes: nothing is written)
        VXG_TRY(launch_copy_bytes(vbits, nullptr, bytes, s_));
        VXG_TRY(validity_into(a, &vbits));
        VXG_TRY(launch_and_words(out.values, vbits, words, s_));
    }
    out.validity = null_as_false ? nullptr : vbits;
    return VXG_OK;
}

// compute::filter (compute/filter.rs:23-52).  The predicate (any Bool encoding) becomes a bit
// buffer padded to whole u64 words; one sync reads the true count (the filtered length the
// reference's Array carries); the array is canonicalized into temporaries and compacted.
// Strings get a new single heap of the selected rows' bytes (VarBin/FSST filter, then
// varbin/flatten.rs), null rows as empty values.
vxg_status Planner::filter(const vxg_array& a, const vxg_array& pred, vxg_canonical& out) {
    if (pred.dtype != VXG_DTYPE_BOOL || pred.nullable)  // filter.rs:27-32
        return set_error(VXG_ERR_INVALID_ARGUMENT, "predicate must be non-nullable bool");
    if (pred.len != a.len)  // filter.rs:33-39
        return set_error(VXG_ERR_INVALID_ARGUMENT, "predicate.len() is " + std::to_string(pred.len) +
                                                       ", does not equal array.len() of " + std::to_string(a.len));
    const bool is_str = is_string(a);
    if (!is_str && a.dtype != VXG_DTYPE_BOOL && a.dtype != VXG_DTYPE_PRIMITIVE)
        return set_error(VXG_ERR_NOT_IMPLEMENTED, "filter supports primitive, bool and utf8/binary dtypes");
    const uint64_t n = a.len, tiles = filter_tiles(n);
    void* mask;
    VXG_TRY(temp(((n + 63) / 64) * 8, &mask));
    VXG_TRY(launch_copy_bytes(mask, nullptr, ((n + 63) / 64) * 8, s_));
    VXG_TRY(bools_into(pred, mask, 0));
    void* toff;
    VXG_TRY(temp((tiles + 1) * 8, &toff));
    const uint64_t* m = static_cast<const uint64_t*>(mask);
    uint64_t* to = static_cast<uint64_t*>(toff);
    VXG_TRY(launch_filter_count(m, n, to, s_));
    uint64_t k = 0;
    VXG_TRY(hip_check(hipMemcpyAsync(&k, to + tiles, 8, hipMemcpyDeviceToHost, s_), "filter count readback"));
    VXG_TRY(hip_check(hipStreamSynchronize(s_), "filter count sync"));
    VXG_TRY(filter_selected(a, m, to, k, out, nullptr));
    // strings: complete on return, like the reference's compute::filter
    return is_str ? hip_check(hipStreamSynchronize(s_), "filter sync") : VXG_OK;
}

// The part of compute::filter after the count: `a` canonicalized into temporaries and compacted by
// the mask `m` (whole u64 words; bits past len are ignored) with its scanned tile offsets `to` and
// true count `k`.  A string array waits once for its heap size (*syncs counts it); the heap's bytes
// are enqueued like every other output.
vxg_status Planner::filter_selected(const vxg_array& a, const uint64_t* m, const uint64_t* to, uint64_t k,
                                    vxg_canonical& out, uint32_t* syncs) {
    const bool is_str = is_string(a);
    const uint64_t n = a.len;
    // canonical source in temporaries
    vxg_canonical src{};
    const vxg_array* vnode;
    int vkind;
    VXG_TRY(validity_source(a, &vnode, &vkind));
    if (vkind != 0) VXG_TRY(temp(((n + 31) / 32) * 4, &src.validity));
    std::vector<vxg_data_buffer> bufs;
    if (is_str) {
        uint64_t extent;
        VXG_TRY(string_layout(a, bufs, extent));
        VXG_TRY(temp(16 * n, &src.views));
        VXG_TRY(temp(extent + 16, &src.data));
        src.data_bytes = extent;
        src.data_buffers = bufs.data();
        src.n_data_buffers = src.data_buffers_cap = uint32_t(bufs.size());
    } else if (a.dtype == VXG_DTYPE_BOOL) {
        VXG_TRY(temp(((n + 31) / 32) * 4, &src.values));
    } else {
        VXG_TRY(temp(n * width(a), &src.values));
    }
    VXG_TRY(canonical(a, src));

    out.kind = src.kind;
    out.len = k;
    out.dtype = a.dtype;
    out.ptype = a.ptype;
    const uint64_t vbits = ((k + 31) / 32) * 4;
    if (src.validity) {  // validity.filter(predicate)
        if (!out.validity) VXG_TRY(hip_check(hipMalloc(&out.validity, vbits ? vbits : 4), "filter validity alloc"));
        VXG_TRY(launch_copy_bytes(out.validity, nullptr, vbits ? vbits : 4, s_));
        VXG_TRY(launch_filter_bits(m, n, to, static_cast<const uint8_t*>(src.validity), out.validity, s_));
    } else {
        out.validity = nullptr;
    }
    if (a.dtype == VXG_DTYPE_PRIMITIVE) {
        out.values_bytes = k * width(a);
        if (!out.values)
            VXG_TRY(hip_check(hipMalloc(&out.values, out.values_bytes ? out.values_bytes : 16), "filter values alloc"));
        return launch_filter_values(m, n, to, src.values, width(a), out.values, s_);
    }
    if (a.dtype == VXG_DTYPE_BOOL) {
        out.values_bytes = vbits;
        if (!out.values) VXG_TRY(hip_check(hipMalloc(&out.values, vbits ? vbits : 4), "filter bool alloc"));
        VXG_TRY(launch_copy_bytes(out.values, nullptr, vbits ? vbits : 4, s_));
        return launch_filter_bits(m, n, to, static_cast<const uint8_t*>(src.values), out.values, s_);
    }
    // strings: compact the views, then rebuild one heap of the selected rows
    if (!out.views) VXG_TRY(hip_check(hipMalloc(&out.views, k ? 16 * k : 16), "filter views alloc"));
    VXG_TRY(launch_filter_values(m, n, to, src.views, 16, out.views, s_));
    const uint64_t ktiles = filter_tiles(k);
    void* hoff;
    VXG_TRY(temp((ktiles + 1) * 8, &hoff));
    uint8_t* views = static_cast<uint8_t*>(out.views);
    const uint8_t* valid = static_cast<const uint8_t*>(out.validity);
    VXG_TRY(launch_view_heap_sizes(views, k, valid, static_cast<uint64_t*>(hoff), s_));
    // the table of the source buffers goes up before the heap-size readback, whose sync drains
    // the copy: `bases` is not read after it
    std::vector<const uint8_t*> bases(bufs.size());
    for (size_t i = 0; i < bufs.size(); ++i) bases[i] = static_cast<const uint8_t*>(src.data) + bufs[i].offset;
    void* dbases;
    VXG_TRY(temp(bases.size() * sizeof(void*) + 8, &dbases));
    if (!bases.empty())
        VXG_TRY(hip_check(hipMemcpyAsync(dbases, bases.data(), bases.size() * sizeof(void*), hipMemcpyHostToDevice, s_),
                          "filter buffer table upload"));
    uint64_t heap = 0;
    const vxg_status rb = hip_check(hipMemcpyAsync(&heap, static_cast<uint64_t*>(hoff) + ktiles, 8, hipMemcpyDeviceToHost, s_),
                                    "filter heap readback");
    VXG_TRY(hip_check(hipStreamSynchronize(s_), "filter heap sync"));
    VXG_TRY(rb);
    if (syncs) ++*syncs;
    if (heap > 0xFFFFFFFFull) return set_error(VXG_ERR_INVALID_ARGUMENT, "filtered string heap exceeds u32 view offsets");
    if (out.data && out.data_bytes < heap)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "caller-provided data holds " + std::to_string(out.data_bytes) +
                                                       " bytes, the filtered heap needs " + std::to_string(heap));
    if (!out.data) VXG_TRY(hip_check(hipMalloc(&out.data, heap + 16), "filter heap alloc"));
    out.data_bytes = heap;
    out.n_data_buffers = 1;
    if (out.data_buffers && out.data_buffers_cap >= 1) out.data_buffers[0] = vxg_data_buffer{0, heap};
    return launch_view_heap_build(views, k, valid, static_cast<uint64_t*>(hoff),
                                  static_cast<const uint8_t* const*>(dbases), uint32_t(bases.size()),
                                  static_cast<uint8_t*>(out.data), ctx_->c.err_word, s_);
}

// ---- filter(batch, mask): the scan's last step (vortex-serde layouts/read/stream.rs:143-149) ----
// One mask for every column of the batch: counted and scanned once, k read back once.  Per column
// (classified and validated before the first launch):
//   Packed    BitPacked / FoR(BitPacked) / ZigZag / ALP over either (compare_shape), or a top-level
//             Chunked whose non-empty chunks all have such a shape: K22 reads the packed words and
//             writes only the selected rows; chunks of one (T, epilogue) share a launch;
//   InPlace   a Primitive array, or a Chunked of Primitive chunks: compacted from its own buffers;
//   Fallback  everything else, and VXG_FILTB_CANONICALIZE: filter_selected (canonicalize, compact).
// The validity of every route is validity_into a temporary, then launch_filter_bits.
vxg_status Planner::filter_batch(const vxg_array* const* cols, uint32_t n_cols, const void* mask, uint64_t n,
                                 uint32_t flags, vxg_canonical* outs, uint64_t* true_count, vxg_filter_batch_info& info) {
    enum class Route { Packed, InPlace, Fallback };
    struct Col {
        Route route = Route::Fallback;
        std::vector<CmpFused> fused;                              // Packed: the non-empty arrays/chunks
        std::vector<std::pair<const void*, uint64_t>> prims;      // InPlace: buffer, first row
        std::vector<uint64_t> prim_len;
        int vkind = 0;
    };
    const bool force = (flags & VXG_FILTB_CANONICALIZE) != 0;
    info.columns = n_cols;
    std::vector<Col> plan(n_cols);
    for (uint32_t ci = 0; ci < n_cols; ci++) {
        const vxg_array& a = *cols[ci];
        Col& col = plan[ci];
        const vxg_array* vnode;
        VXG_TRY(validity_source(a, &vnode, &col.vkind));
        if (a.dtype != VXG_DTYPE_PRIMITIVE || width(a) == 0 || n == 0) continue;  // Bool, strings: Fallback
        // the pieces: the array itself, or the non-empty chunks of a top-level Chunked at their first rows
        std::vector<std::pair<const vxg_array*, uint64_t>> pieces;
        if (a.encoding == VXG_ENC_CHUNKED) {
            if (a.n_children != a.meta.chunked.nchunks + 1)
                return set_error(VXG_ERR_INVALID_ARGUMENT, "Chunked child count != nchunks + 1");
            uint64_t off = 0;
            for (uint32_t i = 1; i < a.n_children; i++) {
                const vxg_array& c = a.children[i];
                if (c.dtype != a.dtype || c.ptype != a.ptype)
                    return set_error(VXG_ERR_MISMATCHED_TYPES, "Chunks must have the same dtype");
                if (c.len) pieces.emplace_back(&c, off);
                off += c.len;
            }
            if (off != n) return set_error(VXG_ERR_INVALID_ARGUMENT, "Chunked chunk lengths do not sum to len");
        } else {
            pieces.emplace_back(&a, 0);
        }
        // compare_shape's checks run for every piece, whatever route the column then takes
        size_t n_fused = 0, n_prim = 0;
        bool misaligned = false;
        for (const auto& [p, row] : pieces) {
            CmpFused f;
            bool is_fused;
            VXG_TRY(compare_shape(*p, row, f, &is_fused));
            if (is_fused) {
                col.fused.push_back(f);
                n_fused++;
            } else if (p->encoding == VXG_ENC_PRIMITIVE) {
                const void* pv;
                VXG_TRY(view_primitive(*p, &pv));  // (a Primitive array: its own buffer, nothing is decoded)
                misaligned = misaligned || reinterpret_cast<uintptr_t>(pv) % uint64_t(width(a));
                col.prims.emplace_back(pv, row);
                col.prim_len.push_back(p->len);
                n_prim++;
            }
        }
        if (force) continue;
        if (n_fused == pieces.size()) col.route = Route::Packed;
        else if (n_prim == pieces.size()) col.route = Route::InPlace;
        if (col.route == Route::InPlace && misaligned)  // (as compare_impl checks the buffers it reads in place)
            return set_error(VXG_ERR_INVALID_ARGUMENT, "primitive buffer must be aligned to the value width");
        if (col.route != Route::Fallback && (reinterpret_cast<uintptr_t>(outs[ci].values) % uint64_t(width(a))))
            return set_error(VXG_ERR_INVALID_ARGUMENT, "filter output must be aligned to the value width");
    }

    // the one count + scan of the mask, and the one readback of k
    const uint64_t tiles = filter_tiles(n);
    const uint64_t* m = static_cast<const uint64_t*>(mask);
    uint64_t* to = nullptr;
    uint64_t k = 0;
    if (n) {
        void* toff;
        VXG_TRY(temp((tiles + 1) * 8, &toff));
        to = static_cast<uint64_t*>(toff);
        VXG_TRY(launch_filter_count(m, n, to, s_));
        info.mask_scans = 1;
        const vxg_status rb = hip_check(hipMemcpyAsync(&k, to + tiles, 8, hipMemcpyDeviceToHost, s_), "filter count readback");
        VXG_TRY(hip_check(hipStreamSynchronize(s_), "filter count sync"));
        VXG_TRY(rb);
        info.syncs++;
    }
    if (true_count) *true_count = k;
    const FiltMask fm{m, n, to, k};

    for (uint32_t ci = 0; ci < n_cols; ci++) {
        const vxg_array& a = *cols[ci];
        Col& col = plan[ci];
        vxg_canonical& out = outs[ci];
        if (k == 0) {  // the scan's skip (stream.rs:144-146): nothing is launched or allocated
            out.kind = is_string(a) ? VXG_ENC_VARBINVIEW : a.dtype == VXG_DTYPE_BOOL ? VXG_ENC_BOOL : VXG_ENC_PRIMITIVE;
            out.len = 0;
            out.dtype = a.dtype;
            out.ptype = a.ptype;
            out.values_bytes = 0;
            if (col.vkind == 0) out.validity = nullptr;
            if (is_string(a)) {
                out.data_bytes = 0;
                out.n_data_buffers = 1;
                if (out.data_buffers && out.data_buffers_cap >= 1) out.data_buffers[0] = vxg_data_buffer{0, 0};
            }
            continue;
        }
        if (col.route == Route::Fallback) {
            info.fallback_arrays++;
            VXG_TRY(filter_selected(a, m, to, k, out, &info.syncs));
            continue;
        }
        out.kind = VXG_ENC_PRIMITIVE;
        out.len = k;
        out.dtype = a.dtype;
        out.ptype = a.ptype;
        out.values_bytes = k * width(a);
        const uint64_t vbits = ((k + 31) / 32) * 4;
        if (col.vkind != 0) {  // validity.filter(mask)
            void* src = nullptr;
            VXG_TRY(temp(((n + 31) / 32) * 4, &src));
            VXG_TRY(validity_into(a, &src));
            if (!out.validity) VXG_TRY(hip_check(hipMalloc(&out.validity, vbits), "filter validity alloc"));
            VXG_TRY(launch_copy_bytes(out.validity, nullptr, vbits, s_));
            VXG_TRY(launch_filter_bits(m, n, to, static_cast<const uint8_t*>(src), out.validity, s_));
        } else {
            out.validity = nullptr;
        }
        if (!out.values) VXG_TRY(hip_check(hipMalloc(&out.values, out.values_bytes), "filter values alloc"));
        if (col.route == Route::InPlace) {
            for (size_t i = 0; i < col.prims.size(); i++) {
                VXG_TRY(launch_filter_range(width(a), col.prims[i].first, col.prims[i].second, col.prim_len[i], fm,
                                            out.values, s_));
                info.inplace_arrays++;
            }
            continue;
        }
        // Packed: one launch per (T, epilogue) and kCmpArgChunks chunks, the table as the argument
        std::vector<CmpFused*> order;
        for (CmpFused& f : col.fused) order.push_back(&f);
        std::stable_sort(order.begin(), order.end(), [](const CmpFused* x, const CmpFused* y) {
            return std::make_tuple(x->T, int(x->epi)) < std::make_tuple(y->T, int(y->epi));
        });
        for (size_t i = 0; i < order.size();) {
            size_t j = i;
            uint64_t blocks = 0;
            while (j < order.size() && j - i < size_t(kCmpArgChunks) && order[j]->T == order[i]->T &&
                   order[j]->epi == order[i]->epi)
                blocks += order[j++]->d.n_blocks();
            // small launches take fewer blocks per workgroup (>= 4: one per wave), the compare's rule
            uint32_t pick = uint32_t(std::min<uint64_t>(32, blocks / 1024)) & ~3u;
            if (pick < 4) pick = 4;
            CmpTable tab{};
            uint64_t groups = 0;
            uint32_t lds = 0;
            for (size_t x = i; x < j; x++) {
                CmpChunk& c = tab.c[tab.n++];
                c = order[x]->d;
                const uint32_t bpw = std::min(cmp_bpw_max(c.W), pick);
                c.bpw_excl = uint8_t(bpw);
                c.first_group = uint32_t(groups);
                groups += (c.n_blocks() + bpw - 1) / bpw;
                lds = std::max(lds, bpw * 128u * c.W);
            }
            // (+ one word row of slack: a value's second word is read unconditionally)
            VXG_TRY(launch_filter_packed(order[i]->T, order[i]->epi, tab, groups, lds + 128, fm, out.values, s_));
            info.packed_launches++;
            info.packed_chunks += uint32_t(j - i);
            i = j;
        }
        // patched rows: BitPacked's raw values through the epilogue, then ALP's values as they are
        for (const CmpFused& f : col.fused) {
            if (f.bp->meta.bitpacked.has_patches) {
                TakePatches tp;
                VXG_TRY(take_patches(*child(*f.bp, 0), tp));
                VXG_TRY(launch_filter_patch(f.T, f.epi, tp, f.d.len(), f.d.out_bit, f.ep, fm, out.values, s_));
                info.patch_launches += tp.n != 0;
            }
            if (f.outer) {
                TakePatches tp;
                VXG_TRY(take_patches(*f.outer, tp));
                VXG_TRY(launch_filter_patch_raw(width(a), tp, f.d.len(), f.d.out_bit, fm, out.values, ctx_->c.err_word, s_));
                info.patch_launches += tp.n != 0;
            }
        }
    }
    return VXG_OK;
}

}  // namespace vxg
