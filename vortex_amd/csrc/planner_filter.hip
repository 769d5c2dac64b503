// planner_filter.hip — filter by a predicate (vortex-array/src/compute/filter.rs:23-52; filter.hip)
// and a scan batch by its row mask (filter_packed.hip): packed cascades are filtered where they lie
// (compare_shape), everything else from its canonical values.
#include "filter.hpp"
#include "filter_packed.hpp"
#include "planner.hpp"

namespace vxg {

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
    VXG_TRY(read_u64(to + tiles, "filter count", &k));
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
    std::vector<vxg_data_buffer> bufs;
    if (is_str) {
        VXG_TRY(string_canonical_temp(a, src, bufs));
    } else {
        const vxg_array* vnode;
        int vkind;
        VXG_TRY(validity_source(a, &vnode, &vkind));
        if (vkind != 0) VXG_TRY(temp(((n + 31) / 32) * 4, &src.validity));
        VXG_TRY(temp(a.dtype == VXG_DTYPE_BOOL ? ((n + 31) / 32) * 4 : n * width(a), &src.values));
        VXG_TRY(canonical(a, src));
    }

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
    VXG_TRY(read_u64(static_cast<uint64_t*>(hoff) + ktiles, "filter heap", &heap));
    if (syncs) ++*syncs;
    VXG_TRY(size_string_heap(out, heap, "filter", "filtered"));
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
        Pieces pieces;
        VXG_TRY(chunk_pieces(a, true, true, pieces));
        // compare_shape's checks run for every piece, whatever route the column then takes
        size_t n_fused = 0, n_prim = 0;
        bool misaligned = false;
        col.fused.reserve(pieces.size());
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
        VXG_TRY(read_u64(to + tiles, "filter count", &k));
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
        // (the compared type follows the column's ptype and the epilogue: it splits no group)
        std::vector<const CmpJob*> jobs;
        jobs.reserve(col.fused.size());
        for (const CmpFused& f : col.fused) jobs.push_back(&f);
        VXG_TRY(for_each_cmp_launch(
            std::move(jobs), [&](const CmpJob& g, const CmpTable& tab, uint64_t groups, uint32_t lds, uint32_t chunks) -> vxg_status {
                info.packed_launches++;
                info.packed_chunks += chunks;
                return launch_filter_packed(g.T, g.epi, tab, groups, lds, fm, out.values, s_);
            }));
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
