// planner_take.hip — take on compressed arrays (vortex-array/src/compute/take.rs:10-34; take.hip,
// take_str.hip): the rows at the indices, read from the compressed tree where a kernel serves it
// (classify_cascade, the string readers) and from the canonical values elsewhere.
#include "filter.hpp"
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
    if (a.encoding == VXG_ENC_DICT) {  // dict/compute.rs:44-52: take the codes, then the values at them
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
    Cascade c;  // (single values are unpacked: the buffer's alignment is not asked for)
    VXG_TRY(classify_cascade(a, false, c));
    TakePacked t{};
    if (c.outer) VXG_TRY(take_patches(*c.outer, t.outer));
    // take's own gate, bitpacking/compute/take.rs:23-31: many indices -> canonicalize and take the primitive
    if (!c.bp || n * 8 > a.len) return via_canonical();
    t.packed = c.packed;
    t.W = c.W;
    t.offset = c.offset;
    t.len = a.len;
    t.idx = idx;
    t.iw = iw;
    t.isg = isg;
    t.n = n;
    t.out = dst;
    t.ep = c.ep;
    t.err = ctx_->c.err_word;
    if (c.bp->meta.bitpacked.has_patches) {  // take.rs:127-200: patches of the taken positions
        if (!child(*c.bp, 0)) return set_error(VXG_ERR_INVALID_ARGUMENT, "BitPacked patches child missing");
        VXG_TRY(take_patches(*child(*c.bp, 0), t.inner));
    }
    if (tinfo_) tinfo_->packed_launches++;
    return launch_take_packed(c.T, c.epi, t, s_);
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
    // canonical views of `s` in temporaries + the base of each of their data buffers
    auto canonical_views = [&](const vxg_array& s, const uint8_t** views, std::vector<const uint8_t*>& bases) -> vxg_status {
        vxg_canonical src;
        std::vector<vxg_data_buffer> lay;
        VXG_TRY(string_canonical_temp(s, src, lay));
        *views = static_cast<const uint8_t*>(src.views);
        bases.resize(lay.size());
        for (size_t b = 0; b < lay.size(); b++) bases[b] = static_cast<const uint8_t*>(src.data) + lay[b].offset;
        return VXG_OK;
    };

    // ---- classify and validate before any output is allocated ----
    enum class Kind { Fallback, Dict, View, VarBin, Fsst } kind = Kind::Fallback;
    const vxg_array *dvalues = nullptr, *dcodes = nullptr;
    ViewSrc vw{};
    VarBinSrc vb{};
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
    case VXG_ENC_VARBINVIEW:
        VXG_TRY(read_varbinview(a, vw));
        kind = Kind::View;
        break;
    case VXG_ENC_VARBIN:
        // take's own gate: a view's offset is a u32, so more bytes than that go to the canonical's
        // several buffers (whose decode checks the children)
        if (child(a, 1) && child(a, 1)->len > 0xFFFFFFFFull) break;
        VXG_TRY(read_varbin(a, vb));
        kind = Kind::VarBin;
        break;
    case VXG_ENC_FSST: {
        FsstSrc f;
        VXG_TRY(read_fsst(a, f));
        fs = TakeFsst{f.symbols, f.sym_lens, f.codes, f.codes_len, f.offs, f.lens, f.n_symbols, tix, nullptr};
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

    // the heap's size, read back, is checked against the caller's buffer, or the heap allocated
    auto size_heap = [&](const uint64_t* total) -> vxg_status {
        uint64_t heap = 0;
        VXG_TRY(read_u64(total, "take heap", &heap));
        return size_string_heap(out, heap, "take", "taken");
    };

    if (kind == Kind::Fsst) {  // sizes from uncompressed_lengths, then decode only the taken rows
        fs.valid = valid;
        const uint64_t tiles = take_str_tiles(n);
        void* toff;
        VXG_TRY(temp((tiles + 1) * 8, &toff));
        VXG_TRY(launch_take_fsst_sizes(fs, static_cast<uint64_t*>(toff), err, s_));
        VXG_TRY(size_heap(static_cast<uint64_t*>(toff) + tiles));
        VXG_TRY(launch_take_fsst_decode(fs, static_cast<const uint64_t*>(toff), static_cast<uint8_t*>(out.data), views, err,
                                        s_));
        return hip_check(hipStreamSynchronize(s_), "take sync");
    }

    // ---- source views of the taken rows, then filter's heap rebuild over their buffers ----
    // The small host tables (`vw.bufs`, `bases`) are uploaded stream-ordered; the heap-size readback's
    // sync drains those copies, so they cost no sync of their own.
    std::vector<const uint8_t*> bases;
    auto rows = [&]() -> vxg_status {
        const uint64_t ktiles = filter_tiles(n);
        void* hoff;
        VXG_TRY(temp((ktiles + 1) * 8, &hoff));
        if (kind == Kind::VarBin) {  // records, sizes, then one pass over the taken rows' bytes
            VXG_TRY(launch_take_varbin_rows(tix, vb.offs, vb.bytes_len, valid, views, err, s_));
            VXG_TRY(launch_view_heap_sizes(views, n, nullptr, static_cast<uint64_t*>(hoff), s_));
            VXG_TRY(size_heap(static_cast<uint64_t*>(hoff) + ktiles));
            return launch_take_varbin_build(views, n, static_cast<const uint64_t*>(hoff), vb.bytes,
                                            static_cast<uint8_t*>(out.data), s_);
        }
        if (kind == Kind::Dict) {
            const uint8_t* vviews;
            VXG_TRY(canonical_views(*dvalues, &vviews, bases));
            VXG_TRY(launch_take_views(vviews, dvalues->len, tcodes, cw, false, n, tix, nullptr, 0, valid, views, err, s_));
        } else if (kind == Kind::View) {
            void* dbufs;
            VXG_TRY(temp(vw.bufs.size() * sizeof(StrBuf), &dbufs));
            if (!vw.bufs.empty())
                VXG_TRY(hip_check(hipMemcpyAsync(dbufs, vw.bufs.data(), vw.bufs.size() * sizeof(StrBuf), hipMemcpyHostToDevice, s_),
                                  "take buffer table upload"));
            for (const StrBuf& b : vw.bufs) bases.push_back(b.p);
            VXG_TRY(launch_take_views(vw.views, a.len, idx, iw, isg, n, TakeIdx{},
                                      static_cast<const StrBuf*>(dbufs), uint32_t(vw.bufs.size()), valid, views, err, s_));
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
        VXG_TRY(size_heap(static_cast<uint64_t*>(hoff) + ktiles));
        return launch_view_heap_build(views, n, valid, static_cast<const uint64_t*>(hoff),
                                      static_cast<const uint8_t* const*>(dbases), uint32_t(bases.size()),
                                      static_cast<uint8_t*>(out.data), err, s_);
    };
    const vxg_status st = rows();
    // complete on return -- and, on an error too, nothing still reads `vw.bufs` / `bases`
    const vxg_status sync = hip_check(hipStreamSynchronize(s_), "take sync");
    return st != VXG_OK ? st : sync;
}

}  // namespace vxg
