// planner_strings.hip — the Planner's string canonicalize: every utf8/binary array becomes a
// VarBinView (canonical.rs:56-63) from VarBin (varbin/flatten.rs:10-17), VarBinView, FSST
// (fsst/canonical.rs:7-57), Dict over strings (varbinview/compute.rs:68-76) and Chunked
// (pack_views, chunked/canonical.rs:194-236), plus the layout of its data buffers.
#include <algorithm>

#include "k1g.hpp"
#include "planner.hpp"

namespace vxg {

// VXG_PLAN_VB_K1G=0 (read at every plan recording): an unbatched plan canonicalizes chunked
// Dict(VarBin) string columns with a views launch + K14 instead of one K1g launch (A/B).
static bool plan_vb_k1g() { return env_flag("VXG_PLAN_VB_K1G", true); }

// ---- strings: VarBin, VarBinView, FSST, Dict(strings), Chunked (pack_views) -------------
// Every string canonical is a VarBinView (canonical.rs:56-63).  Its data buffers: one per
// VarBin / FSST leaf (the bytes buffer / the decoded heap), a Dict's are its values', a
// VarBinView input keeps its own, and a ChunkedArray concatenates its chunks' lists with each
// chunk's buffer_index rebased by the buffers before it (chunked/canonical.rs:194-236).
vxg_status Planner::string_buffer_count(const vxg_array& a, uint32_t& n) {
    switch (a.encoding) {
    case VXG_ENC_VARBIN:
    case VXG_ENC_FSST: n = 1; return VXG_OK;
    case VXG_ENC_VARBINVIEW: n = a.meta.varbinview.n_buffers; return VXG_OK;
    case VXG_ENC_DICT:
        if (a.n_children < 1) return set_error(VXG_ERR_INVALID_ARGUMENT, "DictArray needs values and codes");
        return string_buffer_count(a.children[0], n);
    case VXG_ENC_CHUNKED: {
        uint32_t t = 0;
        for (uint32_t i = 1; i < a.n_children; i++) {
            uint32_t k;
            VXG_TRY(string_buffer_count(a.children[i], k));
            t += k;
        }
        n = t;
        return VXG_OK;
    }
    default:
        return set_error(VXG_ERR_NOT_IMPLEMENTED, "string canonicalize for encoding id " + std::to_string(a.encoding));
    }
}

// Buffer lengths in order; FSST heap sizes (sum of uncompressed lengths) are device sums
// recorded in `fsst` as (slot, node) and resolved by string_layout with one readback.
vxg_status Planner::string_lens(const vxg_array& a, std::vector<uint64_t>& lens,
                                std::vector<std::pair<size_t, const vxg_array*>>& fsst) const {
    switch (a.encoding) {
    case VXG_ENC_VARBIN: {
        const vxg_array* bytes = child(a, 1);
        if (!bytes) return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBinArray needs offsets and bytes");
        lens.push_back(bytes->len);
        return VXG_OK;
    }
    case VXG_ENC_VARBINVIEW:
        if (a.n_children < 1 + a.meta.varbinview.n_buffers)
            return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBinViewArray: missing views/data buffers");
        for (uint32_t b = 0; b < a.meta.varbinview.n_buffers; b++) lens.push_back(a.children[1 + b].len);
        return VXG_OK;
    case VXG_ENC_FSST:
        if (!child(a, 3)) return set_error(VXG_ERR_INVALID_ARGUMENT, "FSST lengths child missing");
        fsst.emplace_back(lens.size(), &a);
        lens.push_back(0);
        return VXG_OK;
    case VXG_ENC_DICT:
        if (!child(a, 0)) return set_error(VXG_ERR_INVALID_ARGUMENT, "DictArray needs values and codes");
        return string_lens(a.children[0], lens, fsst);
    case VXG_ENC_CHUNKED:
        for (uint32_t i = 1; i < a.n_children; i++) VXG_TRY(string_lens(a.children[i], lens, fsst));
        return VXG_OK;
    default:
        return set_error(VXG_ERR_NOT_IMPLEMENTED, "string canonicalize for encoding id " + std::to_string(a.encoding));
    }
}

vxg_status Planner::string_layout(const vxg_array& a, std::vector<vxg_data_buffer>& bufs, uint64_t& extent) {
    std::vector<uint64_t> lens;
    std::vector<std::pair<size_t, const vxg_array*>> fsst;
    VXG_TRY(string_lens(a, lens, fsst));
    if (!fsst.empty()) {  // fsst/canonical.rs:29-42: heap size = sum of uncompressed lengths
        // a query runs on the legacy default stream, which a non-blocking stream's uploads are not
        // ordered with: every upload enqueued so far (any stream) lands before the sums read it
        // (as vxg_plan_create_ex(VXG_PLAN_MEASURE) does before it runs the decode)
        if (query_) VXG_TRY(hip_check(hipDeviceSynchronize(), "layout query: device synchronize"));
        void* d;
        VXG_TRY(temp(8 * fsst.size(), &d));
        for (size_t k = 0; k < fsst.size(); k++) {
            const vxg_array& ul = *child(*fsst[k].second, 3);
            const void* pul;
            VXG_TRY(view_primitive(ul, &pul));
            VXG_TRY(launch_sum(pul, width(ul), ptype_is_signed(ul.ptype), ul.len, static_cast<uint64_t*>(d) + k, s_));
        }
        std::vector<uint64_t> h(fsst.size());
        VXG_TRY(hip_check(hipMemcpyAsync(h.data(), d, 8 * h.size(), hipMemcpyDeviceToHost, s_), "sum readback"));
        VXG_TRY(hip_check(hipStreamSynchronize(s_), "sum sync"));
        for (size_t k = 0; k < fsst.size(); k++) lens[fsst[k].first] = h[k];
    }
    bufs.resize(lens.size());
    uint64_t off = 0;
    for (size_t b = 0; b < lens.size(); b++) {
        bufs[b] = vxg_data_buffer{off, lens[b]};
        off = (off + lens[b] + 15) & ~15ull;
    }
    extent = lens.empty() ? 0 : bufs.back().offset + bufs.back().len;
    return VXG_OK;
}

// Canonical views of `a` into `views`, its data buffers into `data` at bufs[0..k), non-inlined
// views carrying buffer_index bidx + (buffer within a).  `validity`: a's LSB bitmap or NULL.
// `fsst_sink`: `a` is an FSST chunk of a chunked array, decoded with that array's other FSST
// chunks (the chunk loop's list); null: decoded now.  Never handed on to a child.
vxg_status Planner::strings_into(const vxg_array& a, uint8_t* views, uint8_t* data, const vxg_data_buffer* bufs,
                                 uint32_t bidx, const uint8_t* validity, std::vector<FsstChunk>* fsst_sink) {
    switch (a.encoding) {
    case VXG_ENC_VARBIN: {
        // varbin/flatten.rs:10-17: views over the whole bytes buffer (arrow-cast Utf8 -> Utf8View)
        const vxg_array* offs = child(a, 0);
        const vxg_array* bytes = child(a, 1);
        const void *po, *pb;
        VXG_TRY(view_primitive(*offs, &po));
        VXG_TRY(view_primitive(*bytes, &pb));
        uint8_t* heap = data + bufs[0].offset;
        if (bufs[0].len)
            VXG_TRY(launch_copy_bytes(heap, pb, bufs[0].len, s_));
        return launch_varbin_views(heap, bufs[0].len, width(*offs), po, a.len, validity, bidx, views, ctx_->c.err_word, s_);
    }
    case VXG_ENC_VARBINVIEW: {
        // already canonical: views (rebased) and buffers copied into the output layout
        const vxg_array* vw = child(a, 0);
        const void* pv;
        VXG_TRY(view_primitive(*vw, &pv));
        if (vw->len < 16 * a.len) return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBinView views shorter than 16 * len");
        VXG_TRY(launch_views_rebase(static_cast<const uint8_t*>(pv), a.len, bidx, views, s_));
        for (uint32_t b = 0; b < a.meta.varbinview.n_buffers; b++) {
            const void* pb;
            VXG_TRY(view_primitive(a.children[1 + b], &pb));
            if (bufs[b].len)
                VXG_TRY(launch_copy_bytes(data + bufs[b].offset, pb, bufs[b].len, s_));
        }
        return VXG_OK;
    }
    case VXG_ENC_FSST: {
        // fsst/canonical.rs:7-57
        const vxg_array* sym = child(a, 0);
        const vxg_array* slen = child(a, 1);
        const vxg_array* codes = child(a, 2);
        const vxg_array* ulen = child(a, 3);
        if (!sym || !slen || !codes || !ulen || codes->encoding != VXG_ENC_VARBIN)
            return set_error(VXG_ERR_INVALID_ARGUMENT, "FSSTArray needs symbols, lengths, VarBin codes, lengths");
        const void *psym, *pslen, *pcb;
        VXG_TRY(view_primitive(*sym, &psym));
        VXG_TRY(view_primitive(*slen, &pslen));
        VXG_TRY(view_primitive(*child(*codes, 1), &pcb));
        FsstChunk f{};
        f.symbols = static_cast<const uint64_t*>(psym);
        f.sym_lens = static_cast<const uint8_t*>(pslen);
        f.n_symbols = unsigned(sym->len);
        f.codes = static_cast<const uint8_t*>(pcb);
        VXG_TRY(int_column(*child(*codes, 0), f.offs));  // read in place by the FSST kernels
        VXG_TRY(int_column(*ulen, f.lens));              // (packed columns stay packed)
        f.n = a.len;
        f.validity = validity;
        f.heap = data + bufs[0].offset;
        f.heap_len = bufs[0].len;
        f.views = views;
        f.bidx = bidx;
        if (fsst_sink) {  // a chunk: decoded with the other FSST chunks
            fsst_sink->push_back(f);
            return VXG_OK;
        }
        std::vector<FsstChunk> one{f};
        void* scratch;
        VXG_TRY(temp(fsst_chunks_scratch_bytes(one.data(), 1), &scratch));
        return launch_fsst_batch(one, scratch, ctx_->c.err_word, s_, plan_);
    }
    case VXG_ENC_DICT: {
        // Dict over string values: take on the values' views (varbinview/compute.rs:68-76); the
        // values' buffers are the result's buffers, so they decode straight into the output
        const vxg_array* values = child(a, 0);
        const vxg_array* codes = child(a, 1);
        if (!values || !codes) return set_error(VXG_ERR_INVALID_ARGUMENT, "DictArray needs values and codes");
        const vxg_array* vn;
        int vk;
        VXG_TRY(validity_source(*values, &vn, &vk));
        void* vbits = nullptr;  // nullable values: their null rows get zero views before the take
        if (vk != 0) {
            VXG_TRY(temp(((values->len + 31) / 32) * 4, &vbits));
            VXG_TRY(validity_into(*values, &vbits));
        }
        void* vviews;
        VXG_TRY(temp(16 * values->len, &vviews));
        VXG_TRY(strings_into(*values, static_cast<uint8_t*>(vviews), data, bufs, bidx,
                             static_cast<const uint8_t*>(vbits), nullptr));
        if (codes->encoding == VXG_ENC_FL_BITPACKED && codes->meta.bitpacked.bit_width <= kDictFusedMaxW) {
            UnpackArgs ua{};
            ua.dict = vviews;
            ua.dict_len = values->len;
            return decode_bitpacked(*codes, Epi::Dict, 16, ua, views, nullptr);
        }
        const void* pc;
        VXG_TRY(view_primitive(*codes, &pc));
        return launch_take(16, vviews, values->len, width(*codes), false, pc, a.len, views, ctx_->c.err_word, s_);
    }
    case VXG_ENC_CHUNKED: {
        // pack_views (chunked/canonical.rs:194-236): each chunk's views go to its slice of the
        // output, its buffers after the preceding chunks', buffer_index rebased accordingly.
        // Dict(VarBin values, BitPacked codes) chunks share launches: one batched
        // views-and-bytes launch for all their dictionaries, one grouped K1 gather.
        const uint64_t n = a.meta.chunked.nchunks;
        if (a.n_children != n + 1) return set_error(VXG_ERR_INVALID_ARGUMENT, "Chunked child count != nchunks + 1");
        auto dict_batchable = [&](const vxg_array& c) {
            if (c.encoding != VXG_ENC_DICT || c.n_children < 2) return false;
            const vxg_array& v = c.children[0];
            const vxg_array& k = c.children[1];
            return v.encoding == VXG_ENC_VARBIN && v.validity != VXG_VALIDITY_ARRAY &&
                   v.validity != VXG_VALIDITY_ALL_INVALID && v.n_children >= 2 &&
                   v.children[0].encoding == VXG_ENC_PRIMITIVE && v.children[1].encoding == VXG_ENC_PRIMITIVE &&
                   k.encoding == VXG_ENC_FL_BITPACKED && ptype_is_unsigned(k.ptype) && !k.nullable &&
                   k.meta.bitpacked.bit_width <= kDictFusedMaxW;
        };
        uint64_t dict_rows = 0;
        for (uint64_t i = 0; i < n; i++)
            if (dict_batchable(a.children[i + 1])) dict_rows += a.children[i + 1].children[0].len;
        uint8_t* dviews = nullptr;
        if (dict_rows) {
            void* t;
            VXG_TRY(temp(16 * dict_rows, &t));
            dviews = static_cast<uint8_t*>(t);
        }
        std::vector<VarBinChunk> dicts;
        std::vector<K1Job> jobs;
        std::vector<PatchJob> patches;
        K1Sink sink{jobs, patches};
        std::vector<FsstChunk> fssts;
        uint64_t row = 0;
        uint32_t b = 0;
        for (uint64_t i = 0; i < n; i++) {
            const vxg_array& c = a.children[i + 1];
            if (c.dtype != a.dtype) return set_error(VXG_ERR_MISMATCHED_TYPES, "Chunks must have the ChunkedArray's dtype");
            uint32_t k;
            VXG_TRY(string_buffer_count(c, k));
            if (dict_batchable(c)) {
                const vxg_array& v = c.children[0];
                const void *po, *pb;
                VXG_TRY(view_primitive(v.children[0], &po));
                VXG_TRY(view_primitive(v.children[1], &pb));
                VarBinChunk d{};
                d.src = static_cast<const uint8_t*>(pb);
                d.dst = data + bufs[b].offset;
                d.offsets = po;
                d.views = dviews;
                d.bytes = bufs[b].len;
                d.n = v.len;
                d.offs_width = uint32_t(width(v.children[0]));
                d.bidx = bidx + b;
                // a plan batch with a small dictionary: K1g builds its views in LDS (no views
                // launch); otherwise the views are built into dviews first
                const vxg_array& codes = c.children[1];
                // also in an unbatched plan (its own K1g launch per column instead of a views
                // launch + K14: VXG_PLAN_VB_K1G=0 restores those)
                const bool vb = (defer(a) || (plan_ && plan_vb_k1g())) && v.len <= kGenVarBinDictMax && v.len > 0 &&
                                codes.len > 0 && !codes.meta.bitpacked.has_patches;
                if (!vb) dicts.push_back(d);
                UnpackArgs ua{};
                ua.dict = vb ? nullptr : dviews;
                ua.dict_len = v.len;
                dviews += 16 * v.len;
                K1Job j;
                const vxg_array* p;  // (null with vb)
                VXG_TRY(describe_bitpacked(codes, Epi::Dict, 16, ua, views + 16 * row, j, &p));
                j.vb = vb;
                if (vb) j.vbc = d;
                VXG_TRY(submit_k1(j, p, ua, &sink, nullptr));
            } else {
                void* cv = nullptr;  // the chunk's own validity (null views are all-zero)
                const vxg_array* vn;
                int vk;
                VXG_TRY(validity_source(c, &vn, &vk));
                if (vk != 0) {
                    VXG_TRY(temp(((c.len + 31) / 32) * 4, &cv));
                    VXG_TRY(validity_into(c, &cv));
                }
                VXG_TRY(strings_into(c, views + 16 * row, data, bufs + b, bidx + b, static_cast<const uint8_t*>(cv),
                                     c.encoding == VXG_ENC_FSST ? &fssts : nullptr));
            }
            row += c.len;
            b += k;
        }
        if (row != a.len) return set_error(VXG_ERR_INVALID_ARGUMENT, "Chunked len != sum of chunk lens");
        if (!fssts.empty() && defer(a)) {  // a plan's root: decoded at the batch's flush
            batch_->fssts.insert(batch_->fssts.end(), fssts.begin(), fssts.end());
        } else if (!fssts.empty()) {
            void* scratch;
            VXG_TRY(temp(fsst_chunks_scratch_bytes(fssts.data(), fssts.size()), &scratch));
            VXG_TRY(launch_fsst_batch(fssts, scratch, ctx_->c.err_word, s_, plan_));
        }
        if (defer(a) && patches.empty()) {  // a plan's root: launched with the other arrays' jobs (PlanBatch)
            batch_->dicts.insert(batch_->dicts.end(), dicts.begin(), dicts.end());
            batch_->jobs.insert(batch_->jobs.end(), jobs.begin(), jobs.end());
            return VXG_OK;
        }
        VXG_TRY(launch_varbin_dicts(dicts, ctx_->c.err_word, s_, plan_));
        VXG_TRY(launch_k1_jobs(jobs, ctx_->c.err_word, s_, plan_, nullptr));
        for (const PatchJob& p : patches) VXG_TRY(apply_sparse_patches(*p.sp, p.T, p.epi, p.vw, p.a, p.dst, p.out_len));
        return VXG_OK;
    }
    default:
        return set_error(VXG_ERR_NOT_IMPLEMENTED, "string canonicalize for encoding id " + std::to_string(a.encoding));
    }
}

vxg_status Planner::string_canonical(const vxg_array& a, vxg_canonical& out) {
    out.kind = VXG_ENC_VARBINVIEW;
    out.len = a.len;
    out.dtype = a.dtype;
    uint32_t nb;
    VXG_TRY(string_buffer_count(a, nb));
    std::vector<vxg_data_buffer> bufs;
    if (out.views && out.data) {
        // caller-allocated (sized with vxg_canonical_layout / _size): no device sum + sync on
        // the decode path
        if (nb == 1) {
            bufs.push_back(vxg_data_buffer{0, out.data_bytes});
        } else {
            if (!out.data_buffers || out.n_data_buffers != nb)
                return set_error(VXG_ERR_INVALID_ARGUMENT, "caller-provided data needs the vxg_canonical_layout buffer table (" +
                                                               std::to_string(nb) + " buffers)");
            bufs.assign(out.data_buffers, out.data_buffers + nb);
        }
    } else {
        uint64_t extent;
        VXG_TRY(string_layout(a, bufs, extent));
        if (nb > 1 && (!out.data_buffers || out.data_buffers_cap < nb))
            return set_error(VXG_ERR_INVALID_ARGUMENT, "data_buffers must have room for " + std::to_string(nb) + " buffers");
        if (!out.views) VXG_TRY(hip_check(hipMalloc(&out.views, a.len ? 16 * a.len : 16), "views alloc"));
        if (!out.data) VXG_TRY(hip_check(hipMalloc(&out.data, extent + 16), "data alloc"));
        out.data_bytes = extent;
    }
    out.n_data_buffers = nb;
    if (out.data_buffers && out.data_buffers_cap >= nb && out.data_buffers != bufs.data())
        std::copy(bufs.begin(), bufs.end(), out.data_buffers);
    VXG_TRY(validity_into(a, &out.validity));
    return strings_into(a, static_cast<uint8_t*>(out.views), static_cast<uint8_t*>(out.data), bufs.data(), 0,
                        static_cast<const uint8_t*>(out.validity), nullptr);
}

vxg_status Planner::string_canonical_temp(const vxg_array& s, vxg_canonical& src, std::vector<vxg_data_buffer>& lay) {
    src = vxg_canonical{};
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
    return string_canonical(s, src);
}

// ---- string arrays read where they lie (take_str.hip, compare_str.hip) ----------------------
vxg_status Planner::string_bytes(const vxg_array& b, const void** p) {
    if (b.dtype != VXG_DTYPE_PRIMITIVE || width(b) != 1)
        return set_error(VXG_ERR_MISMATCHED_TYPES, "string bytes must be a u8 array");
    return view_primitive(b, p);
}

vxg_status Planner::read_varbin(const vxg_array& s, VarBinSrc& v) {
    const vxg_array* offs = child(s, 0);
    const vxg_array* bytes = child(s, 1);
    if (!offs || !bytes) return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBinArray needs offsets and bytes");
    if (!ptype_is_int(offs->ptype) || offs->dtype != VXG_DTYPE_PRIMITIVE)
        return set_error(VXG_ERR_MISMATCHED_TYPES, "VarBin offsets must be integers");
    if (offs->len < s.len + 1) return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBin offsets shorter than len + 1");
    const void* pb;
    VXG_TRY(string_bytes(*bytes, &pb));
    IntCol oc;
    VXG_TRY(int_column(*offs, oc));
    if (reinterpret_cast<uintptr_t>(oc.p) % uint64_t(oc.packed ? 16 : oc.width))
        return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBin offsets must be aligned to their width");
    v = VarBinSrc{static_cast<const uint8_t*>(pb), bytes->len, to_ccol(oc)};
    return VXG_OK;
}

vxg_status Planner::read_varbinview(const vxg_array& s, ViewSrc& v) {
    const vxg_array* vw = child(s, 0);
    const uint32_t nb = s.meta.varbinview.n_buffers;
    if (!vw || s.n_children < 1 + nb)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBinViewArray: missing views/data buffers");
    const void* pv;
    VXG_TRY(string_bytes(*vw, &pv));
    if (vw->len < 16 * s.len) return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBinView views shorter than 16 * len");
    if (reinterpret_cast<uintptr_t>(pv) & 15)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBinView views must be 16-byte aligned");
    v.views = static_cast<const uint8_t*>(pv);
    v.bufs.resize(nb);
    for (uint32_t b = 0; b < nb; b++) {
        const void* pb;
        VXG_TRY(string_bytes(s.children[1 + b], &pb));
        v.bufs[b] = StrBuf{static_cast<const uint8_t*>(pb), s.children[1 + b].len};
    }
    return VXG_OK;
}

vxg_status Planner::read_fsst(const vxg_array& s, FsstSrc& f) {
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
    VXG_TRY(string_bytes(*child(*codes, 1), &pcb));
    if (reinterpret_cast<uintptr_t>(psym) & 7) return set_error(VXG_ERR_INVALID_ARGUMENT, "FSST symbols must be 8-byte aligned");
    IntCol oc, lc;
    VXG_TRY(int_column(*child(*codes, 0), oc));
    VXG_TRY(int_column(*ulen, lc));
    if (reinterpret_cast<uintptr_t>(oc.p) % uint64_t(oc.packed ? 16 : oc.width) ||
        reinterpret_cast<uintptr_t>(lc.p) % uint64_t(lc.packed ? 16 : lc.width))
        return set_error(VXG_ERR_INVALID_ARGUMENT, "FSST offsets / lengths must be aligned to their width");
    f = FsstSrc{static_cast<const uint64_t*>(psym), static_cast<const uint8_t*>(pslen), static_cast<const uint8_t*>(pcb),
                child(*codes, 1)->len, to_ccol(oc), to_ccol(lc), uint32_t(sym->len)};
    return VXG_OK;
}

// ---- the one new heap of a string take / filter ----------------------------------------------
vxg_status Planner::size_string_heap(vxg_canonical& out, uint64_t heap, const char* op, const char* rows) {
    const std::string r(rows);
    if (heap > 0xFFFFFFFFull) return set_error(VXG_ERR_INVALID_ARGUMENT, r + " string heap exceeds u32 view offsets");
    if (out.data && out.data_bytes < heap)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "caller-provided data holds " + std::to_string(out.data_bytes) +
                                                       " bytes, the " + r + " heap needs " + std::to_string(heap));
    if (!out.data) VXG_TRY(hip_check(hipMalloc(&out.data, heap + 16), (std::string(op) + " heap alloc").c_str()));
    out.data_bytes = heap;
    out.n_data_buffers = 1;
    if (out.data_buffers && out.data_buffers_cap >= 1) out.data_buffers[0] = vxg_data_buffer{0, heap};
    return VXG_OK;
}

vxg_status Planner::read_u64(const uint64_t* dev, const char* what, uint64_t* v) {
    const hipError_t rb = hipMemcpyAsync(v, dev, 8, hipMemcpyDeviceToHost, s_);
    const hipError_t sync = hipStreamSynchronize(s_);  // (also after a failed copy: nothing is left in flight)
    if (sync != hipSuccess) return hip_check(sync, (std::string(what) + " sync").c_str());
    return rb == hipSuccess ? VXG_OK : hip_check(rb, (std::string(what) + " readback").c_str());
}

}  // namespace vxg
