// planner_decode.hip — the Planner's decode of primitive arrays, validity and bools, and
// canonical() itself: Array::into_canonical (vortex-array/src/canonical.rs:353-357) ->
// ArrayEncoding::canonicalize (encoding/mod.rs:53) -> per-encoding IntoCanonical (cited at each
// case).  A BitPacked-rooted cascade (ALP -> FoR -> BitPacked: 3-4 passes in the reference,
// SURVEY.md §3 stack B) is ONE fused K1 launch (+ tiny patch scatters); anything else is decoded
// child-first into temporaries exactly like the reference.
#include <algorithm>
#include <cstring>

#include "planner.hpp"

namespace vxg {

// VXG_FUSED_PATCHES=0 (read at every decode): ALP's outer patches take the separate scatter
// launch instead of the K1w launch (A/B measurements, parity tests of both paths).
static bool fused_patches_enabled() { return env_flag("VXG_FUSED_PATCHES", true); }

vxg_status Planner::view_primitive(const vxg_array& a, const void** p) {
    if (a.encoding == VXG_ENC_PRIMITIVE) {
        const vxg_buffer* b = buf(a, 0);
        if (!b && a.len) return set_error(VXG_ERR_INVALID_ARGUMENT, "Primitive array without buffer");
        if (b && b->len < a.len * width(a))
            return set_error(VXG_ERR_INVALID_ARGUMENT, "Primitive buffer shorter than len * width");
        *p = b ? b->ptr : nullptr;
        return VXG_OK;
    }
    void* t;
    VXG_TRY(temp(a.len * width(a), &t));
    VXG_TRY(decode_into(a, t));
    *p = t;
    return VXG_OK;
}

vxg_status Planner::int_column(const vxg_array& a, IntCol& c) {
    // An integer child read in place by a consumer kernel: a patch-free 32/64-bit
    // [FoR](BitPacked) column stays packed (elements unpacked where used); anything else is
    // canonicalized to a primitive buffer first.
    if (!ptype_is_int(a.ptype)) return set_error(VXG_ERR_MISMATCHED_TYPES, "expected an integer array");
    bool packed = false;
    VXG_TRY(packed_column(a, c, &packed));
    return packed ? VXG_OK : view_primitive(a, &c.p);
}

vxg_status Planner::runend_column(const vxg_array& a, bool in_place, IntCol& c) {
    // RunEnd ends/values: read in place by the short-run kernel when packable, else a plain
    // buffer (canonicalized child-first).  Non-integer values (floats) are plain bits.
    bool packed = false;
    if (in_place && ptype_is_int(a.ptype)) VXG_TRY(packed_column(a, c, &packed));
    if (packed) return VXG_OK;
    c = IntCol{};
    c.width = width(a);
    c.sgn = ptype_is_signed(a.ptype);
    return view_primitive(a, &c.p);
}

vxg_status Planner::packed_column(const vxg_array& a, IntCol& c, bool* packed) {
    *packed = false;
    c = IntCol{};
    c.width = width(a);
    c.sgn = ptype_is_signed(a.ptype);
    const vxg_array* bp = fl_leaf(&a, &c.reference, &c.shift);
    if (bp && !bp->meta.bitpacked.has_patches && width(*bp) == c.width && (c.width == 4 || c.width == 8) &&
        bp->len == a.len) {
        const vxg_buffer* pk = buf(*bp, 0);
        uint64_t nblk;  // (elements are unpacked one by one: no alignment is asked for)
        VXG_TRY(check_bitpacked(8 * c.width, bp->meta.bitpacked.bit_width, bp->meta.bitpacked.offset, bp->len,
                                pk ? pk->ptr : nullptr, pk ? pk->len : 0, false, &nblk));
        c.packed = true;
        c.p = pk ? pk->ptr : nullptr;
        c.W = bp->meta.bitpacked.bit_width;
        c.offset = bp->meta.bitpacked.offset;
        *packed = true;
    }
    return VXG_OK;
}

const vxg_array* Planner::fl_leaf(const vxg_array* c, uint64_t* reference, uint32_t* shift) const {
    if (c && c->encoding == VXG_ENC_FL_FOR && child(*c, 0) && child(*c, 0)->encoding == VXG_ENC_FL_BITPACKED) {
        *reference = c->meta.for_.reference;
        *shift = c->meta.for_.shift;
        return child(*c, 0);
    }
    return c && c->encoding == VXG_ENC_FL_BITPACKED ? c : nullptr;
}

bool Planner::alp_factors(const vxg_array& a, double* alp_a, double* alp_b) {
    const bool f32 = a.ptype == VXG_F32;
    const unsigned e = a.meta.alp.e, f = a.meta.alp.f, top = f32 ? 10 : 23;
    if ((!f32 && a.ptype != VXG_F64) || e > top || f > top) return false;
    *alp_a = f32 ? double(kF10f[f]) : kF10d[f];
    *alp_b = f32 ? double(kIF10f[e]) : kIF10d[e];
    return true;
}

vxg_status Planner::classify_cascade(const vxg_array& a, bool aligned, Cascade& c) {
    c = Cascade{};
    const vxg_array* bp = nullptr;
    switch (a.encoding) {
    case VXG_ENC_FL_BITPACKED: bp = &a; break;  // bitpacking/compute/take.rs:21-125
    case VXG_ENC_FL_FOR:                          // for/compute.rs:39-48: the child, under the FoR
        bp = fl_leaf(&a, &c.ep.reference, &c.ep.shift);
        c.epi = Epi::For;
        break;
    case VXG_ENC_ZIGZAG:  // zigzag/compute.rs: the encoded child, decoded
        bp = fl_leaf(child(a, 0), &c.ep.reference, &c.ep.shift);
        c.epi = Epi::ForZigZag;
        break;
    case VXG_ENC_ALP:  // alp/compute.rs: the encoded child and the patches
        if (!alp_factors(a, &c.ep.alp_a, &c.ep.alp_b)) return VXG_OK;
        bp = fl_leaf(child(a, 0), &c.ep.reference, &c.ep.shift);
        c.epi = a.ptype == VXG_F32 ? Epi::AlpF32 : Epi::AlpF64;
        if (bp && a.meta.alp.has_patches) {
            if (!child(a, 1)) return set_error(VXG_ERR_INVALID_ARGUMENT, "ALPArray: patches child missing");
            c.outer = child(a, 1);
        }
        break;
    default: return VXG_OK;
    }
    if (!bp || width(*bp) != width(a) || bp->len != a.len) return VXG_OK;
    const vxg_buffer* pb = buf(*bp, 0);
    c.T = 8 * width(*bp);
    c.W = bp->meta.bitpacked.bit_width;
    c.offset = bp->meta.bitpacked.offset;
    uint64_t nblk;
    VXG_TRY(check_bitpacked(c.T, c.W, c.offset, bp->len, pb ? pb->ptr : nullptr, pb ? pb->len : 0, aligned, &nblk));
    c.packed = pb ? static_cast<const uint8_t*>(pb->ptr) : nullptr;
    c.bp = bp;
    return VXG_OK;
}

vxg_status Planner::chunk_pieces(const vxg_array& a, bool check_ptype, bool skip_empty, Pieces& pieces) {
    if (a.encoding != VXG_ENC_CHUNKED) {
        pieces.emplace_back(&a, 0);
        return VXG_OK;
    }
    if (a.n_children != a.meta.chunked.nchunks + 1)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "Chunked child count != nchunks + 1");
    pieces.reserve(a.n_children);
    uint64_t off = 0;
    for (uint32_t i = 1; i < a.n_children; i++) {
        const vxg_array& c = a.children[i];
        if (c.dtype != a.dtype || (check_ptype && c.ptype != a.ptype))
            return set_error(VXG_ERR_MISMATCHED_TYPES, "Chunks must have the same dtype");
        if (c.len || !skip_empty) pieces.emplace_back(&c, off);
        off += c.len;
    }
    if (off != a.len) return set_error(VXG_ERR_INVALID_ARGUMENT, "Chunked chunk lengths do not sum to len");
    return VXG_OK;
}

vxg_status Planner::apply_sparse_patches(const vxg_array& sp, int T, Epi epi, int vw, const UnpackArgs& a,
                                         void* dst, uint64_t out_len) {
    // bitpacking/compress.rs:191-207 / alp/compress.rs:80-96: only SparseArray patches.
    if (sp.encoding != VXG_ENC_SPARSE)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "Can't patch with a non-Sparse array");
    const vxg_array* idx = child(sp, 0);
    const vxg_array* val = child(sp, 1);
    if (!idx || !val) return set_error(VXG_ERR_INVALID_ARGUMENT, "Sparse patches need indices and values");
    if (idx->len != val->len) return set_error(VXG_ERR_INVALID_ARGUMENT, "Sparse indices/values length mismatch");
    PatchCol pc;  // a packed index column is unpacked by the scatter itself (no temporary)
    VXG_TRY(int_column(*idx, pc.idx));
    VXG_TRY(view_primitive(*val, &pc.vals));
    return launch_patch(vw, pc.idx, epi, T, dst, out_len, sp.meta.sparse.indices_offset, pc.vals, idx->len, a, s_);
}

bool Planner::patch_fusable(const vxg_array& sp, int value_width) const {
    const vxg_array* idx = child(sp, 0);
    const vxg_array* val = child(sp, 1);
    return sp.encoding == VXG_ENC_SPARSE && idx && val && idx->len == val->len && idx->len > 0 &&
           width(*val) == value_width && width(*idx) == 8 && ptype_is_int(idx->ptype);
}

vxg_status Planner::sparse_patch_col(const vxg_array& sp, PatchCol& pc) {
    // patch_fusable(sp) holds
    const vxg_array* idx = child(sp, 0);
    VXG_TRY(int_column(*idx, pc.idx));
    VXG_TRY(view_primitive(*child(sp, 1), &pc.vals));
    pc.n = idx->len;
    pc.idx_off = sp.meta.sparse.indices_offset;
    return VXG_OK;
}

vxg_status Planner::describe_bitpacked(const vxg_array& bp, Epi epi, int vw, UnpackArgs& a, void* dst, K1Job& j,
                                       const vxg_array** patches) {
    // bitpacking/mod.rs:215-219 -> compress.rs:167-189 (patches: child 0 when has_patches)
    if (!ptype_is_int(bp.ptype)) return set_error(VXG_ERR_MISMATCHED_TYPES, "BitPacked needs an integer ptype");
    const vxg_buffer* packed = buf(bp, 0);
    a.err = ctx_->c.err_word;
    VXG_TRY(make_k1_job(8 * width(bp), bp.meta.bitpacked.bit_width, bp.meta.bitpacked.offset, bp.len,
                        packed ? packed->ptr : nullptr, packed ? packed->len : 0, epi, vw, a, dst, j));
    *patches = bp.meta.bitpacked.has_patches ? child(bp, 0) : nullptr;
    if (bp.meta.bitpacked.has_patches && !*patches)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "BitPackedArray: patches child missing");
    return VXG_OK;
}

vxg_status Planner::submit_k1(const K1Job& j, const vxg_array* patches, const UnpackArgs& a, K1Sink* sink,
                              const PatchCol* fused) {
    if (sink) {  // a chunk of a ChunkedArray: launched with the other chunks
        sink->jobs.push_back(j);
        if (patches) sink->patches.push_back(PatchJob{patches, j.T, j.epi, j.vw, a, j.d.out, j.d.len});
        return VXG_OK;
    }
    std::vector<K1Job> one{j};
    VXG_TRY(launch_k1_jobs(one, ctx_->c.err_word, s_, plan_, fused));
    if (patches) VXG_TRY(apply_sparse_patches(*patches, j.T, j.epi, j.vw, a, j.d.out, j.d.len));
    return VXG_OK;
}

vxg_status Planner::decode_bitpacked(const vxg_array& bp, Epi epi, int vw, UnpackArgs a, void* dst, K1Sink* sink) {
    K1Job j;
    const vxg_array* p;
    VXG_TRY(describe_bitpacked(bp, epi, vw, a, dst, j, &p));
    return submit_k1(j, p, a, sink, nullptr);
}

vxg_status Planner::decode_alp(const vxg_array& a, void* dst, K1Sink* sink) {
    // alp/array.rs:269 -> alp/compress.rs:61-78 (+ patch_decoded :80-96)
    const vxg_array* enc = child(a, 0);
    if (!enc) return set_error(VXG_ERR_INVALID_ARGUMENT, "ALPArray: encoded child missing");
    const bool f32 = a.ptype == VXG_F32;
    if (!f32 && a.ptype != VXG_F64) return set_error(VXG_ERR_MISMATCHED_TYPES, "ALP can only encode f32 and f64");
    UnpackArgs ua{};
    if (!alp_factors(a, &ua.alp_a, &ua.alp_b)) return set_error(VXG_ERR_INVALID_ARGUMENT, "ALP exponents out of range");
    const Epi epi = f32 ? Epi::AlpF32 : Epi::AlpF64;
    const vxg_array* bp = fl_leaf(enc, &ua.reference, &ua.shift);
    bool fused = false;  // the outer patches written by the K1w launch itself
    if (bp && width(*bp) == (f32 ? 4 : 8)) {
        PatchCol pc{};
        const vxg_array* p = a.meta.alp.has_patches ? child(a, 1) : nullptr;
        if (p && !sink && !bp->meta.bitpacked.has_patches && bp->len == a.len && patch_fusable(*p, f32 ? 4 : 8) &&
            fused_patches_enabled()) {
            // the launch submit_k1 makes: one kernel-argument table of this array's blocks
            const uint64_t nblk = (bp->len + bp->meta.bitpacked.offset + 1023) / 1024;
            if (k1_choose(f32 ? 32 : 64, int(bp->meta.bitpacked.bit_width), epi, false, (nblk + 31) / 32, false,
                          k1_wave_mode(), split_below_groups()).kind == K1Kind::Wave) {
                VXG_TRY(sparse_patch_col(*p, pc));
                fused = !pc.idx.packed || pc.idx.W > 0;  // K1w reads 8-byte index words directly
            }
        }
        K1Job j;
        const vxg_array* inner;
        VXG_TRY(describe_bitpacked(*bp, epi, 0, ua, dst, j, &inner));
        fused = fused && j.d.n_blocks;  // (an empty array launches nothing)
        VXG_TRY(submit_k1(j, inner, ua, sink, fused ? &pc : nullptr));  // fused unpack+FoR+ALP (+patches)
    } else {
        const void* penc;
        VXG_TRY(view_primitive(*enc, &penc));
        VXG_TRY(launch_alp(a.ptype, penc, a.len, ua.alp_a, ua.alp_b, dst, s_));
    }
    if (a.meta.alp.has_patches && !fused) {
        const vxg_array* p = child(a, 1);
        if (!p) return set_error(VXG_ERR_INVALID_ARGUMENT, "ALPArray: patches child missing");
        UnpackArgs plain{};
        plain.err = ctx_->c.err_word;
        if (sink) {  // after the chunk's K1 decode and its inner patches
            sink->patches.push_back(PatchJob{p, f32 ? 32 : 64, Epi::Plain, 0, plain, dst, a.len});
            return VXG_OK;
        }
        VXG_TRY(apply_sparse_patches(*p, f32 ? 32 : 64, Epi::Plain, 0, plain, dst, a.len));
    }
    return VXG_OK;
}

vxg_status Planner::decode_dict_primitive(const vxg_array& a, void* dst, K1Sink* sink) {
    // dict/array.rs:68-73: take(canonical(values), codes)
    const vxg_array* values = child(a, 0);
    const vxg_array* codes = child(a, 1);
    if (!values || !codes) return set_error(VXG_ERR_INVALID_ARGUMENT, "DictArray needs values and codes");
    if (!ptype_is_unsigned(codes->ptype) || codes->nullable)
        return set_error(VXG_ERR_MISMATCHED_TYPES, "Dict codes must be non-nullable unsigned int");
    const void* pv;
    VXG_TRY(view_primitive(*values, &pv));
    const int vw = width(*values);
    if (codes->encoding == VXG_ENC_FL_BITPACKED && codes->meta.bitpacked.bit_width <= kDictFusedMaxW) {
        UnpackArgs ua{};
        ua.dict = pv;
        ua.dict_len = values->len;
        return decode_bitpacked(*codes, Epi::Dict, vw, ua, dst, sink);
    }
    const void* pc;
    VXG_TRY(view_primitive(*codes, &pc));
    return launch_take(vw, pv, values->len, width(*codes), false, pc, a.len, dst, ctx_->c.err_word, s_);
}

// Chunks whose whole decode is one K1 launch (+ patch scatters): BitPacked, FoR/ZigZag/ALP over
// BitPacked of the same width, Dict(Primitive values, BitPacked codes).  Their decodes are
// deferred and grouped across chunks; nothing in them reads another deferred output.
bool Planner::k1_fusable(const vxg_array& c) const {
    auto bp_of_width = [&](const vxg_array* x, int w) {
        return x && x->encoding == VXG_ENC_FL_BITPACKED && width(*x) == w && ptype_is_int(x->ptype);
    };
    const int w = width(c);
    switch (c.encoding) {
    case VXG_ENC_FL_BITPACKED: return ptype_is_int(c.ptype);
    case VXG_ENC_FL_FOR: return ptype_is_int(c.ptype) && bp_of_width(child(c, 0), w);
    case VXG_ENC_ZIGZAG: return ptype_is_signed(c.ptype) && bp_of_width(child(c, 0), w);
    case VXG_ENC_ALP: {
        if (c.ptype != VXG_F32 && c.ptype != VXG_F64) return false;
        const vxg_array* e = child(c, 0);
        if (e && e->encoding == VXG_ENC_FL_FOR) e = child(*e, 0);
        return bp_of_width(e, w);
    }
    case VXG_ENC_DICT: {
        const vxg_array* v = child(c, 0);
        const vxg_array* k = child(c, 1);
        return v && k && v->encoding == VXG_ENC_PRIMITIVE && k->encoding == VXG_ENC_FL_BITPACKED &&
               ptype_is_unsigned(k->ptype) && !k->nullable && k->meta.bitpacked.bit_width <= kDictFusedMaxW;
    }
    default: return false;
    }
}

vxg_status Planner::decode_chunked_primitive(const vxg_array& a, void* dst) {
    // chunked/canonical.rs:27-122 / pack_primitives :170-187 -- every chunk decodes straight
    // into its slice of the output (no per-chunk materialisation + memcpy).  Launches are
    // shared across chunks, level by level:
    //   level 0  K1 decodes: chunks that are one K1 decode, and the ends/values children of
    //            RunEnd chunks (into one temporary)      -> grouped by kernel, 32 per launch
    //   level 1  their patch scatters
    //   level 2  RunEnd expansions                         -> 48 chunks per launch
    // Other chunks decode one by one.
    const uint64_t n = a.meta.chunked.nchunks;
    if (a.n_children != n + 1) return set_error(VXG_ERR_INVALID_ARGUMENT, "Chunked child count != nchunks + 1");
    const int w = width(a);
    std::vector<K1Job> jobs;
    std::vector<PatchJob> patches;
    K1Sink sink{jobs, patches};
    std::vector<RunEndChunk> runs;
    std::vector<uint8_t> runs_indep;  // the run's children are read in place (no level-0 decode)
    // RunEnd chunks whose ends/values are primitive or one K1 decode: their temporaries
    auto child_ok = [&](const vxg_array* x) {
        return x && ptype_is_int(x->ptype) && (x->encoding == VXG_ENC_PRIMITIVE || k1_fusable(*x));
    };
    auto batch_runend = [&](const vxg_array& c) {
        const vxg_array* e = child(c, 0);
        const vxg_array* v = child(c, 1);
        return c.encoding == VXG_ENC_RUN_END && child_ok(e) && v && width(*v) == w && e->len == v->len &&
               (v->encoding == VXG_ENC_PRIMITIVE || k1_fusable(*v)) && e->len > 0;
    };
    // short-run chunks read packed ends/values in place (no temporary, no level-0 launch)
    std::vector<IntCol> inplace(2 * n);
    std::vector<uint8_t> is_inplace(2 * n, 0);
    uint64_t tmp_bytes = 0;
    for (uint64_t i = 0; i < n; i++) {
        const vxg_array& c = a.children[i + 1];
        if (!batch_runend(c)) continue;
        const vxg_array* e = child(c, 0);
        const vxg_array* v = child(c, 1);
        const bool short_runs = c.len <= kRunEndShortRun * e->len;
        const vxg_array* xs[2] = {e, v};
        for (int k = 0; k < 2; k++) {
            bool pk = false;
            if (short_runs && ptype_is_int(xs[k]->ptype)) VXG_TRY(packed_column(*xs[k], inplace[2 * i + k], &pk));
            is_inplace[2 * i + k] = pk;
            if (!pk && xs[k]->encoding != VXG_ENC_PRIMITIVE) tmp_bytes += (xs[k]->len * width(*xs[k]) + 15) & ~15ull;
        }
    }
    uint8_t* tmp = nullptr;
    if (tmp_bytes) {
        void* t;
        VXG_TRY(temp(tmp_bytes, &t));
        tmp = static_cast<uint8_t*>(t);
    }
    // decode `x` (primitive or one K1 decode) for a RunEnd chunk: pointer into the temporary
    auto level0 = [&](const vxg_array& x, const void** p) -> vxg_status {
        if (x.encoding == VXG_ENC_PRIMITIVE) return view_primitive(x, p);
        *p = tmp;
        tmp += (x.len * width(x) + 15) & ~15ull;
        return decode_into(x, const_cast<void*>(*p), &sink);
    };
    uint64_t off = 0;
    for (uint64_t i = 0; i < n; i++) {
        const vxg_array& c = a.children[i + 1];
        if (c.ptype != a.ptype || c.dtype != a.dtype)
            return set_error(VXG_ERR_MISMATCHED_TYPES, "Chunks must have the ChunkedArray's dtype");
        uint8_t* slice = static_cast<uint8_t*>(dst) + off * w;
        if (k1_fusable(c)) {
            VXG_TRY(decode_into(c, slice, &sink));
        } else if (batch_runend(c)) {
            // runend/compress.rs:115-148 (runend/array.rs:191-197)
            const vxg_array& e = *child(c, 0);
            const vxg_array& v = *child(c, 1);
            RunEndChunk r{};
            IntCol* cols[2] = {&r.ends, &r.values};
            const vxg_array* xs[2] = {&e, &v};
            for (int k = 0; k < 2; k++) {
                if (is_inplace[2 * i + k]) {
                    *cols[k] = inplace[2 * i + k];
                } else {
                    cols[k]->width = width(*xs[k]);
                    cols[k]->sgn = ptype_is_signed(xs[k]->ptype);
                    VXG_TRY(level0(*xs[k], &cols[k]->p));
                }
            }
            r.out = slice;
            r.n_runs = e.len;
            r.offset = c.meta.runend.offset;
            r.len = c.len;
            runs.push_back(r);
            runs_indep.push_back(uint8_t((is_inplace[2 * i] || e.encoding == VXG_ENC_PRIMITIVE) &&
                                         (is_inplace[2 * i + 1] || v.encoding == VXG_ENC_PRIMITIVE)));
        } else if ((reinterpret_cast<uintptr_t>(slice) & 15) == 0) {
            VXG_TRY(decode_into(c, slice));
        } else {
            const void* p;
            VXG_TRY(view_primitive(c, &p));
            VXG_TRY(launch_copy_bytes(slice, p, c.len * w, s_));
        }
        off += c.len;
    }
    if (off != a.len) return set_error(VXG_ERR_INVALID_ARGUMENT, "Chunked len != sum of chunk lens");
    if (defer(a) && patches.empty()) {  // a plan's root: launched with the other arrays' jobs (PlanBatch)
        batch_->jobs.insert(batch_->jobs.end(), jobs.begin(), jobs.end());
        for (size_t k = 0; k < runs.size(); k++) batch_->runs.push_back(PlanBatch::Run{w, runs[k], runs_indep[k] != 0});
        return VXG_OK;
    }
    VXG_TRY(launch_k1_jobs(jobs, ctx_->c.err_word, s_, plan_, nullptr));
    for (const PatchJob& p : patches) VXG_TRY(apply_sparse_patches(*p.sp, p.T, p.epi, p.vw, p.a, p.dst, p.out_len));
    return launch_runs(runs, w, ctx_->c.err_word, s_, plan_);
}

vxg_status Planner::decode_alprd(const vxg_array& a, void* dst) {
    // alp_rd/array.rs:179-235 -> alp_rd/mod.rs:260-301
    const vxg_array* left = child(a, 0);
    const vxg_array* right = child(a, 1);
    if (!left || !right) return set_error(VXG_ERR_INVALID_ARGUMENT, "ALPRDArray needs left/right parts");
    if (left->ptype != VXG_U16) return set_error(VXG_ERR_MISMATCHED_TYPES, "ALP-RD left parts must be u16");
    const void *pl, *pr;
    VXG_TRY(view_primitive(*left, &pl));
    VXG_TRY(view_primitive(*right, &pr));
    const void* pos = nullptr;
    const void* exc = nullptr;
    uint64_t n_exc = 0, pos_off = 0;
    int pw = 8;
    bool psg = false;
    if (a.meta.alprd.has_exceptions) {
        const vxg_array* sp = child(a, 2);
        if (!sp || sp->encoding != VXG_ENC_SPARSE)
            return set_error(VXG_ERR_INVALID_ARGUMENT, "left_parts_exceptions must be SparseArray encoded");
        const vxg_array* si = child(*sp, 0);
        const vxg_array* sv = child(*sp, 1);
        VXG_TRY(view_primitive(*si, &pos));
        VXG_TRY(view_primitive(*sv, &exc));
        n_exc = si->len;
        pos_off = sp->meta.sparse.indices_offset;
        pw = width(*si);
        psg = ptype_is_signed(si->ptype);
    }
    return launch_alprd(a.ptype, static_cast<const uint16_t*>(pl), a.meta.alprd.dict, a.meta.alprd.dict_len,
                        a.meta.alprd.right_bit_width, pr, a.len, pos, pw, psg, pos_off,
                        static_cast<const uint16_t*>(exc), n_exc, dst, ctx_->c.err_word, s_);
}

vxg_status Planner::decode_sparse_values(const vxg_array& a, void* dst) {
    // array/sparse/flatten.rs:68-98: fill (null fill -> default 0), then scatter values.
    uint8_t fill[16] = {0};
    if (!a.meta.sparse.fill_is_null) std::memcpy(fill, a.meta.sparse.fill, 16);
    VXG_TRY(launch_fill(width(a), fill, a.len, dst, s_));
    UnpackArgs plain{};
    plain.err = ctx_->c.err_word;
    return apply_sparse_patches(a, 8 * width(a), Epi::Plain, 0, plain, dst, a.len);
}

vxg_status Planner::decode_into(const vxg_array& a, void* dst, K1Sink* sink) {
    if (!is_primitive_dtype(a)) return set_error(VXG_ERR_MISMATCHED_TYPES, "expected a primitive dtype");
    const int w = width(a);
    if (w == 0) return set_error(VXG_ERR_NOT_IMPLEMENTED, "unsupported ptype");
    switch (a.encoding) {
    case VXG_ENC_PRIMITIVE: {
        const void* p;
        VXG_TRY(view_primitive(a, &p));
        if (p != dst && a.len)
            VXG_TRY(launch_copy_bytes(dst, p, a.len * w, s_));
        return VXG_OK;
    }
    case VXG_ENC_FL_BITPACKED:
        return decode_bitpacked(a, Epi::Plain, 0, UnpackArgs{}, dst, sink);
    case VXG_ENC_FL_FOR: {
        // for/mod.rs:105-109 -> for/compress.rs:86-98
        const vxg_array* enc = child(a, 0);
        if (!enc) return set_error(VXG_ERR_INVALID_ARGUMENT, "FoRArray is missing encoded child array");
        if (!ptype_is_int(a.ptype)) return set_error(VXG_ERR_MISMATCHED_TYPES, "FoR needs an integer ptype");
        if (enc->encoding == VXG_ENC_FL_BITPACKED && width(*enc) == w) {
            UnpackArgs ua{};
            ua.reference = a.meta.for_.reference;
            ua.shift = a.meta.for_.shift;
            return decode_bitpacked(*enc, Epi::For, 0, ua, dst, sink);
        }
        VXG_TRY(decode_into(*enc, dst));
        return launch_for(w, dst, a.len, a.meta.for_.reference, a.meta.for_.shift, false, dst, s_);
    }
    case VXG_ENC_ZIGZAG: {
        const vxg_array* enc = child(a, 0);
        if (!enc) return set_error(VXG_ERR_INVALID_ARGUMENT, "ZigZagArray is missing encoded child");
        if (!ptype_is_signed(a.ptype)) return set_error(VXG_ERR_MISMATCHED_TYPES, "ZigZag decodes to signed ints");
        if (enc->encoding == VXG_ENC_FL_BITPACKED && width(*enc) == w)
            return decode_bitpacked(*enc, Epi::ForZigZag, 0, UnpackArgs{}, dst, sink);
        VXG_TRY(decode_into(*enc, dst));
        return launch_zigzag(w, dst, a.len, dst, s_);
    }
    case VXG_ENC_ALP:
        return decode_alp(a, dst, sink);
    case VXG_ENC_ALP_RD:
        return decode_alprd(a, dst);
    case VXG_ENC_DICT:
        return decode_dict_primitive(a, dst, sink);
    case VXG_ENC_FL_DELTA: {
        // delta/mod.rs:237 -> delta/compress.rs:100-166
        const vxg_array* bases = child(a, 0);
        const vxg_array* deltas = child(a, 1);
        if (!bases || !deltas) return set_error(VXG_ERR_INVALID_ARGUMENT, "DeltaArray needs bases and deltas");
        const int T = 8 * w, lanes = 1024 / T;
        const uint64_t nd = deltas->len;
        if (bases->len != (nd / 1024) * lanes + (nd % 1024 ? 1 : 0))
            return set_error(VXG_ERR_INVALID_ARGUMENT, "DeltaArray: bases.len() != expected_bases_len");
        if (a.meta.delta.offset >= 1024 || a.meta.delta.offset + a.len > nd)
            return set_error(VXG_ERR_INVALID_ARGUMENT, "DeltaArray: offset/len out of range");
        const void *pb, *pd;
        VXG_TRY(view_primitive(*bases, &pb));
        VXG_TRY(view_primitive(*deltas, &pd));
        return launch_delta(w, pb, pd, nd, a.meta.delta.offset, a.len, dst, s_);
    }
    case VXG_ENC_RUN_END: {
        // runend/array.rs:191-197 -> runend/compress.rs:95-148
        const vxg_array* ends = child(a, 0);
        const vxg_array* values = child(a, 1);
        if (!ends || !values) return set_error(VXG_ERR_INVALID_ARGUMENT, "RunEndArray needs ends and values");
        if (ends->len != values->len) return set_error(VXG_ERR_INVALID_ARGUMENT, "RunEnd ends/values length mismatch");
        RunEndChunk c{};
        c.out = dst;
        c.n_runs = ends->len;
        c.offset = a.meta.runend.offset;
        c.len = a.len;
        VXG_TRY(runend_column(*ends, a.len <= kRunEndShortRun * ends->len, c.ends));
        VXG_TRY(runend_column(*values, a.len <= kRunEndShortRun * ends->len, c.values));
        return launch_runend(w, c, ctx_->c.err_word, s_);
    }
    case VXG_ENC_SPARSE:
        return decode_sparse_values(a, dst);
    case VXG_ENC_CONSTANT: {
        uint8_t sc[16] = {0};
        if (!a.meta.constant.is_null) std::memcpy(sc, a.meta.constant.scalar, 16);
        return launch_fill(w, sc, a.len, dst, s_);
    }
    case VXG_ENC_CHUNKED:
        return decode_chunked_primitive(a, dst);
    default:
        return set_error(VXG_ERR_NOT_IMPLEMENTED,
                         "no GPU canonicalize for encoding id " + std::to_string(a.encoding));
    }
}

// Where does the validity of `a` come from?  kind: 0 = no nulls, 1 = all invalid,
// 2 = Bool child array `node` (canonical bitmap buffer 0).
vxg_status Planner::validity_source(const vxg_array& a, const vxg_array** node, int* kind) {
    *node = nullptr;
    *kind = 0;
    auto from_meta = [&](uint32_t child_idx) -> vxg_status {
        switch (a.validity) {
        case VXG_VALIDITY_NON_NULLABLE:
        case VXG_VALIDITY_ALL_VALID: return VXG_OK;
        case VXG_VALIDITY_ALL_INVALID: *kind = 1; return VXG_OK;
        default: {
            const vxg_array* v = child(a, child_idx);
            if (!v || v->dtype != VXG_DTYPE_BOOL)
                return set_error(VXG_ERR_INVALID_ARGUMENT, "validity child must be a Bool array");
            *node = v;
            *kind = v->encoding == VXG_ENC_BOOL ? 2 : 5;  // 5: compressed bools, decoded
            return VXG_OK;
        }
        }
    };
    switch (a.encoding) {
    case VXG_ENC_PRIMITIVE:
    case VXG_ENC_BOOL:
    case VXG_ENC_BYTE_BOOL: return from_meta(0);
    case VXG_ENC_RUN_END_BOOL: return from_meta(1);
    case VXG_ENC_FL_BITPACKED: return from_meta(a.meta.bitpacked.has_patches ? 1 : 0);
    case VXG_ENC_FL_DELTA: return from_meta(2);
    case VXG_ENC_RUN_END: return from_meta(2);
    case VXG_ENC_VARBIN: return from_meta(2);
    case VXG_ENC_VARBINVIEW: return from_meta(1 + a.meta.varbinview.n_buffers);
    case VXG_ENC_FL_FOR:
    case VXG_ENC_ZIGZAG:
    case VXG_ENC_ALP: return child(a, 0) ? validity_source(*child(a, 0), node, kind) : VXG_OK;
    case VXG_ENC_ALP_RD: return child(a, 0) ? validity_source(*child(a, 0), node, kind) : VXG_OK;
    case VXG_ENC_FSST: return child(a, 2) ? validity_source(*child(a, 2), node, kind) : VXG_OK;
    case VXG_ENC_CONSTANT: *kind = a.meta.constant.is_null ? 1 : 0; return VXG_OK;
    case VXG_ENC_DICT: {
        const vxg_array* v = child(a, 0);
        if (!v) return VXG_OK;
        // take(values, codes) carries values.validity().take(codes) (primitive/compute/take.rs:
        // 58-67, varbinview/compute.rs:68-76): gathered from the values' bitmap by code
        VXG_TRY(validity_source(*v, node, kind));
        if (*kind != 0) {
            *kind = 6;
            *node = &a;
        }
        return VXG_OK;
    }
    case VXG_ENC_SPARSE:
        // primitives: valid exactly at the indices when the fill is null; bools: always
        // (canonicalize_sparse_bools builds its validity from the indices alone,
        // sparse/flatten.rs:41-61)
        if (a.meta.sparse.fill_is_null || a.dtype == VXG_DTYPE_BOOL) { *kind = 3; *node = &a; }
        return VXG_OK;
    case VXG_ENC_CHUNKED: {
        for (uint32_t i = 1; i < a.n_children; i++) {
            const vxg_array* n2;
            int k2;
            VXG_TRY(validity_source(a.children[i], &n2, &k2));
            if (k2 != 0) { *kind = 4; *node = &a; return VXG_OK; }
        }
        return VXG_OK;
    }
    default: return VXG_OK;
    }
}

vxg_status Planner::validity_into(const vxg_array& a, void** bitmap) {
    const vxg_array* node;
    int kind;
    VXG_TRY(validity_source(a, &node, &kind));
    if (kind == 0) {  // no nulls: validity NULL (a caller-provided bitmap is left untouched)
        *bitmap = nullptr;
        return VXG_OK;
    }
    const uint64_t bytes = ((a.len + 31) / 32) * 4;
    if (!*bitmap) VXG_TRY(hip_check(hipMalloc(bitmap, bytes ? bytes : 4), "validity alloc"));
    VXG_TRY(launch_copy_bytes(*bitmap, nullptr, bytes ? bytes : 4, s_));
    if (kind == 1) return VXG_OK;
    if (kind == 2) {
        const vxg_buffer* b = buf(*node, 0);
        if (!b) return set_error(VXG_ERR_INVALID_ARGUMENT, "BoolArray without buffer");
        return launch_copy_bits(*bitmap, 0, static_cast<const uint8_t*>(b->ptr),
                                node->meta.boolean.first_byte_bit_offset, a.len, false, s_);
    }
    if (kind == 5) return bools_into(*node, *bitmap, 0);
    // kinds 6, 3 and 4 name the Dict / Sparse / Chunked node itself: `a`, or the node a FoR / ZigZag /
    // ALP / ALP-RD / FSST array inherits its validity from (validity_source's recursion)
    const vxg_array& src = *node;
    if (kind == 6) {  // Dict with nullable values: bit i = values_valid[codes[i]]
        const vxg_array* vals = child(src, 0);
        const vxg_array* codes = child(src, 1);
        if (!vals || !codes) return set_error(VXG_ERR_INVALID_ARGUMENT, "DictArray needs values and codes");
        if (!ptype_is_int(codes->ptype)) return set_error(VXG_ERR_MISMATCHED_TYPES, "Dict codes must be integers");
        void* vbits = nullptr;
        VXG_TRY(temp(((vals->len + 31) / 32) * 4, &vbits));
        VXG_TRY(validity_into(*vals, &vbits));
        const void* pc;
        VXG_TRY(view_primitive(*codes, &pc));
        return launch_gather_bits(*bitmap, pc, width(*codes), false, a.len, static_cast<const uint8_t*>(vbits), vals->len,
                                  ctx_->c.err_word, s_);
    }
    if (kind == 3) {  // Sparse with null fill: valid exactly at the indices (flatten.rs:82-93)
        const vxg_array* idx = child(src, 0);
        const void* pi;
        VXG_TRY(view_primitive(*idx, &pi));
        return launch_set_bits_at(*bitmap, pi, width(*idx), ptype_is_signed(idx->ptype),
                                  src.meta.sparse.indices_offset, idx->len, a.len, s_);
    }
    // kind 4: chunked concatenation of chunk validities
    uint64_t off = 0;
    for (uint32_t i = 1; i < src.n_children; i++) {
        const vxg_array& c = src.children[i];
        const vxg_array* n2;
        int k2;
        VXG_TRY(validity_source(c, &n2, &k2));
        if (k2 == 0) {
            VXG_TRY(launch_copy_bits(*bitmap, off, nullptr, 0, c.len, true, s_));
        } else if (k2 == 2) {
            VXG_TRY(launch_copy_bits(*bitmap, off, static_cast<const uint8_t*>(n2->buffers[0].ptr),
                                     n2->meta.boolean.first_byte_bit_offset, c.len, false, s_));
        } else if (k2 == 5) {
            VXG_TRY(bools_into(*n2, *bitmap, off));
        } else if (k2 != 1) {
            void* sub = nullptr;
            VXG_TRY(temp(((c.len + 31) / 32) * 4, &sub));
            VXG_TRY(validity_into(c, &sub));
            VXG_TRY(launch_copy_bits(*bitmap, off, static_cast<const uint8_t*>(sub), 0, c.len, false, s_));
        }
        off += c.len;
    }
    return VXG_OK;
}

// ---- bools: canonical BoolArray = LSB bit buffer (bool/mod.rs), from every Bool encoding ----
vxg_status Planner::bools_into(const vxg_array& a, void* bits, uint64_t off) {
    if (a.dtype != VXG_DTYPE_BOOL) return set_error(VXG_ERR_MISMATCHED_TYPES, "expected a Bool array");
    if (a.len == 0) return VXG_OK;
    switch (a.encoding) {
    case VXG_ENC_BOOL: {  // bool/mod.rs:25-28: bits from first_byte_bit_offset
        const vxg_buffer* b = buf(a, 0);
        const uint64_t fbo = a.meta.boolean.first_byte_bit_offset;
        if (!b || b->len * 8 < fbo + a.len) return set_error(VXG_ERR_INVALID_ARGUMENT, "BoolArray buffer too short");
        return launch_copy_bits(bits, off, static_cast<const uint8_t*>(b->ptr), fbo, a.len, false, s_);
    }
    case VXG_ENC_BYTE_BOOL: {  // bytebool/src/array.rs:138-146
        const vxg_buffer* b = buf(a, 0);
        if (!b || b->len < a.len) return set_error(VXG_ERR_INVALID_ARGUMENT, "ByteBoolArray buffer too short");
        return launch_bytebool(static_cast<const uint8_t*>(b->ptr), a.len, bits, off, s_);
    }
    case VXG_ENC_RUN_END_BOOL: {  // runend-bool/src/array.rs:152-163 -> compress.rs:46-93
        const vxg_array* e = child(a, 0);
        if (!e || e->len == 0) return set_error(VXG_ERR_INVALID_ARGUMENT, "Ends array must have at least one element");
        if (!ptype_is_unsigned(e->ptype))
            return set_error(VXG_ERR_INVALID_ARGUMENT, "Ends array must be an unsigned integer type");
        const void* pe;
        VXG_TRY(view_primitive(*e, &pe));
        return launch_runend_bool(pe, width(*e), e->len, a.meta.runendbool.offset, a.meta.runendbool.start != 0,
                                  a.len, bits, off, ctx_->c.err_word, s_);
    }
    case VXG_ENC_ROARING_BOOL: {  // roaring/src/boolean/mod.rs:127-147 (K16, roaring.hip)
        const vxg_buffer* b = buf(a, 0);
        if (!b) return set_error(VXG_ERR_INVALID_ARGUMENT, "RoaringBoolArray without buffer");
        return launch_roaring_bool(static_cast<const uint8_t*>(b->ptr), b->len, a.len, bits, off, ctx_->c.err_word, s_);
    }
    case VXG_ENC_CONSTANT:  // constant/canonical.rs:26-33: new_set / new_unset
        if (!a.meta.constant.is_null && a.meta.constant.scalar[0])
            return launch_copy_bits(bits, off, nullptr, 0, a.len, true, s_);
        return VXG_OK;
    case VXG_ENC_SPARSE: {  // sparse/flatten.rs:41-61 canonicalize_sparse_bools
        const vxg_array* idx = child(a, 0);
        const vxg_array* val = child(a, 1);
        if (!idx || !val || idx->len != val->len)
            return set_error(VXG_ERR_INVALID_ARGUMENT, "Sparse needs indices and values of equal length");
        if (!a.meta.sparse.fill_is_null && a.meta.sparse.fill[0])
            VXG_TRY(launch_copy_bits(bits, off, nullptr, 0, a.len, true, s_));
        if (idx->len == 0) return VXG_OK;
        void* vb;
        const uint64_t vbytes = ((val->len + 31) / 32) * 4;
        VXG_TRY(temp(vbytes, &vb));
        VXG_TRY(launch_copy_bytes(vb, nullptr, vbytes, s_));
        VXG_TRY(bools_into(*val, vb, 0));
        const void* pi;
        VXG_TRY(view_primitive(*idx, &pi));
        return launch_assign_bits_at(bits, off, pi, width(*idx), ptype_is_signed(idx->ptype),
                                     a.meta.sparse.indices_offset, idx->len, a.len, static_cast<const uint8_t*>(vb), s_);
    }
    case VXG_ENC_CHUNKED: {  // chunked/canonical.rs:154-163 pack_bools
        uint64_t o = 0;
        for (uint32_t i = 1; i < a.n_children; i++) {
            VXG_TRY(bools_into(a.children[i], bits, off + o));
            o += a.children[i].len;
        }
        if (o != a.len) return set_error(VXG_ERR_INVALID_ARGUMENT, "Chunked len != sum of chunk lens");
        return VXG_OK;
    }
    default:
        return set_error(VXG_ERR_NOT_IMPLEMENTED, "bool canonicalize for encoding id " + std::to_string(a.encoding));
    }
}

vxg_status Planner::canonical_size(const vxg_array& a, uint64_t& vb, uint64_t& db) {
    vb = db = 0;
    if (a.dtype == VXG_DTYPE_PRIMITIVE) {
        vb = a.len * width(a);
        return VXG_OK;
    }
    if (a.dtype == VXG_DTYPE_BOOL) {  // whole 32-bit words
        vb = ((a.len + 31) / 32) * 4;
        return VXG_OK;
    }
    if (!is_string(a)) return set_error(VXG_ERR_NOT_IMPLEMENTED, "canonical size for this dtype");
    vb = a.len * 16;
    std::vector<vxg_data_buffer> bufs;
    return string_layout(a, bufs, db);
}

vxg_status Planner::canonical(const vxg_array& a, vxg_canonical& out) {
    root_ = &a;
    out.len = a.len;
    out.dtype = a.dtype;
    out.ptype = a.ptype;
    if (is_string(a)) return string_canonical(a, out);
    if (a.dtype == VXG_DTYPE_BOOL) {  // Canonical::Bool: LSB bit buffer + validity
        out.kind = VXG_ENC_BOOL;
        out.values_bytes = ((a.len + 31) / 32) * 4;
        if (!out.values)
            VXG_TRY(hip_check(hipMalloc(&out.values, out.values_bytes ? out.values_bytes : 4), "bool values alloc"));
        if (out.values_bytes)
            VXG_TRY(launch_copy_bytes(out.values, nullptr, out.values_bytes, s_));
        VXG_TRY(bools_into(a, out.values, 0));
        return validity_into(a, &out.validity);
    }
    if (a.dtype != VXG_DTYPE_PRIMITIVE)
        return set_error(VXG_ERR_NOT_IMPLEMENTED, "canonicalize supports primitive, bool and utf8/binary dtypes");
    out.kind = VXG_ENC_PRIMITIVE;
    out.values_bytes = a.len * width(a);
    if (!out.values)
        VXG_TRY(hip_check(hipMalloc(&out.values, out.values_bytes ? out.values_bytes : 16), "values alloc"));
    VXG_TRY(decode_into(a, out.values));
    return validity_into(a, &out.validity);
}

}  // namespace vxg
