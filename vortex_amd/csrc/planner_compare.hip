// planner_compare.hip — compare with a scalar on compressed arrays (compute/compare.rs:81-124;
// compare.hip), of strings with a scalar (compare_str.hip), and a scan's conjunctive row filter
// over both (filtering.rs:27-43; compare_range.hip).  Each reads the compressed tree where a kernel
// serves it and falls back to the canonical values.
#include <cstring>

#include "planner.hpp"

namespace vxg {

// ---- compute::compare with a scalar (vortex-array/src/compute/compare.rs:81-124) ----------
// Is `a` a cascade the fused kernel serves -- BitPacked, FoR(BitPacked), ZigZag or ALP over
// either (classify_cascade)?  Then describe it for the kernel's table.
vxg_status Planner::compare_shape(const vxg_array& a, uint64_t out_bit, CmpFused& f, bool* fused) {
    *fused = false;
    f = CmpFused{};
    f.arr = &a;
    // compare's own gate: ZigZag decodes to a signed type, and the kernel compares the array's ptype
    // (take gathers the bits as they are); the fallback reports an unsigned one
    if (a.encoding == VXG_ENC_ZIGZAG && !ptype_is_signed(a.ptype)) return VXG_OK;
    Cascade c;
    VXG_TRY(classify_cascade(a, true, c));
    const bool alp = c.epi == Epi::AlpF32 || c.epi == Epi::AlpF64;
    // compare's own gate: values are ordered as the integers or floats their ptypes name
    if (!c.bp || !ptype_is_int(c.bp->ptype) || !(ptype_is_int(a.ptype) || alp)) return VXG_OK;
    // compare's own gate: CmpChunk holds a 40-bit length
    if (a.len > kCmpMaxLen) return set_error(VXG_ERR_INVALID_ARGUMENT, "array too long for one compare launch");
    f.bp = c.bp;
    f.outer = c.outer;
    f.T = c.T;
    f.epi = c.epi;
    f.ck = alp ? kCmpFloat : ptype_is_signed(a.ptype) ? kCmpSigned : kCmpUnsigned;
    f.ep = c.ep;
    // compare's own gate: the patch kernels read values of the array's width / ptype.  Patch children
    // are checked here, before the caller allocates or launches anything
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
    f.d.packed = c.packed;
    f.d.len_lo = uint32_t(a.len);
    f.d.len_hi = uint8_t(a.len >> 32);
    f.d.out_bit = out_bit;
    f.d.reference = f.ep.reference;
    f.d.alp_e = a.encoding == VXG_ENC_ALP ? a.meta.alp.e : 0;
    f.d.alp_f = a.encoding == VXG_ENC_ALP ? a.meta.alp.f : 0;
    f.d.offset = uint16_t(c.offset);
    f.d.shift = uint8_t(f.ep.shift);
    f.d.W = uint8_t(c.W);
    *fused = true;
    return VXG_OK;
}

// The header and value bitmap of a Bool result.
vxg_status Planner::bool_output(uint64_t n, const char* what, vxg_canonical& out) {
    const uint64_t bytes = ((n + 63) / 64) * 8;
    out.kind = VXG_ENC_BOOL;
    out.len = n;
    out.dtype = VXG_DTYPE_BOOL;
    out.ptype = VXG_U8;
    out.values_bytes = bytes;
    if (!out.values)
        VXG_TRY(hip_check(hipMalloc(&out.values, bytes ? bytes : 8), (std::string(what) + " values alloc").c_str()));
    if (reinterpret_cast<uintptr_t>(out.values) & 7)
        return set_error(VXG_ERR_INVALID_ARGUMENT, std::string(what) + " output must be 8-byte aligned");
    return VXG_OK;
}

// value bits of null rows are 0; null_as_false drops the validity (filtering.rs:42)
vxg_status Planner::compare_validity(const vxg_array& a, uint32_t flags, vxg_canonical& out) {
    const uint64_t n = a.len, words = (n + 63) / 64, bytes = words * 8;
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
    const uint64_t n = a.len, bytes = ((n + 63) / 64) * 8;

    // the pieces: the array itself, or the chunks of a top-level ChunkedArray at their bit offsets
    Pieces pieces;
    VXG_TRY(chunk_pieces(a, true, false, pieces));
    // classify and validate every piece before anything is allocated or launched
    std::vector<CmpFused> fused;
    Pieces plain;
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

    VXG_TRY(bool_output(n, "compare", out));
    if (zero) VXG_TRY(launch_copy_bytes(out.values, nullptr, bytes, s_));

    // fused launches, one per kernel instantiation (T, epilogue, compared type)
    std::vector<const CmpJob*> jobs;
    jobs.reserve(fused.size());
    for (const CmpFused& f : fused) jobs.push_back(&f);
    VXG_TRY(for_each_cmp_launch(
        std::move(jobs), [&](const CmpJob& k, const CmpTable& tab, uint64_t groups, uint32_t lds, uint32_t chunks) -> vxg_status {
            info.fused_launches++;
            info.fused_chunks += chunks;
            if (range) return launch_cmp_range_packed(k.T, k.epi, k.ck, tab, groups, lds, out.values, *range, s_);
            return launch_cmp_packed(k.T, k.epi, k.ck, tab, groups, lds, out.values, scalar_bits, op, s_);
        }));
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
    return compare_validity(a, flags, out);
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

    out.validity = nullptr;
    VXG_TRY(bool_output(n, "row filter", out));

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
    auto view_piece = [&](const void* views, const std::vector<StrBuf>& bufs) -> vxg_status {
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
        VarBinSrc v;
        VXG_TRY(read_varbin(s, v));
        // a truth table's VarBin with plain offsets: the 40-byte piece
        if (table && child(s, 0)->encoding == VXG_ENC_PRIMITIVE && v.bytes_len <= 0xFFFFFFFFull && s.len <= 0xFFFFFFFFull &&
            out_bit % 64 == 0 && out_bit / 64 <= 0xFFFFFFFFull) {
            VbDictPiece p{};
            p.bytes = v.bytes;
            p.offs = v.offs.p;
            p.bytes_len = uint32_t(v.bytes_len);
            p.out_word = uint32_t(out_bit / 64);
            p.n = uint32_t(s.len);
            p.width = v.offs.width;
            p.sgn = v.offs.sgn;
            rows.vbd.push_back(p);
            return VXG_OK;
        }
        VbPiece p{};
        p.bytes = v.bytes;
        p.bytes_len = v.bytes_len;
        p.offs = v.offs;
        p.out_bit = out_bit;
        p.n = s.len;
        p.excl = excl;
        rows.vb.push_back(p);
        return VXG_OK;
    }
    case VXG_ENC_VARBINVIEW: {
        ViewSrc v;
        VXG_TRY(read_varbinview(s, v));
        return view_piece(v.views, v.bufs);
    }
    case VXG_ENC_FSST: {
        FsstSrc f;
        VXG_TRY(read_fsst(s, f));
        FsstPiece p{};
        p.symbols = f.symbols;
        p.sym_lens = f.sym_lens;
        p.codes = f.codes;
        p.codes_len = f.codes_len;
        p.offs = f.offs;
        p.lens = f.lens;
        p.out_bit = out_bit;
        p.n = s.len;
        p.excl = excl;
        p.n_symbols = f.n_symbols;
        rows.fs.push_back(p);
        return VXG_OK;
    }
    default: {
        // canonical views + data in temporaries (as Planner::filter builds its source)
        *fell_back = true;
        vxg_canonical src;
        std::vector<vxg_data_buffer> lay;
        VXG_TRY(string_canonical_temp(s, src, lay));
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
    const uint64_t n = a.len, bytes = ((n + 63) / 64) * 8;

    // the pieces: the array itself, or the chunks of a top-level ChunkedArray at their bit offsets
    Pieces pieces;
    VXG_TRY(chunk_pieces(a, false, false, pieces));

    // classify and validate every piece before the output is allocated or a compare is launched
    StrRows table_rows, out_rows;
    std::vector<CmpJob> packed;  // the lookups of BitPacked codes (no epilogue, nothing compared)
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
            uint64_t nblk;
            VXG_TRY(check_bitpacked(T, W, off, p->len, pb ? pb->ptr : nullptr, pb ? pb->len : 0, true, &nblk));
            CmpJob dp{};
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

    VXG_TRY(bool_output(n, "compare", out));
    if (zero) VXG_TRY(launch_copy_bytes(out.values, nullptr, bytes, s_));

    // truth tables: every dictionary starts on a 64-bit word of one temporary
    void* tt = nullptr;
    if (tt_words) {
        VXG_TRY(temp(tt_words * 8, &tt));
        VXG_TRY(launch_str_rows(table_rows, sc, tt, op, info.table_launches));
    }
    // lookups of the BitPacked codes, one launch per code width T
    std::vector<const CmpJob*> jobs;
    jobs.reserve(packed.size());
    for (const CmpJob& dp : packed) jobs.push_back(&dp);
    VXG_TRY(for_each_cmp_launch(
        std::move(jobs), [&](const CmpJob& k, const CmpTable& tab, uint64_t groups, uint32_t lds, uint32_t) -> vxg_status {
            info.dict_launches++;
            return launch_cmpb_dict_packed(k.T, tab, groups, lds, out.values, tt, ctx_->c.err_word, s_);
        }));
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
    return compare_validity(a, flags, out);
}

}  // namespace vxg
