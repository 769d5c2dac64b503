// planner.hpp — what the units of the canonicalize planner share: the Planner class, the K1 job and
// plan-batch records, the launch-grouping functions and the small helpers of every entry point.
//
// The planner is the host-side mirror of the reference's dispatch: Array::into_canonical
// (vortex-array/src/canonical.rs:353-357) -> ArrayEncoding::canonicalize (encoding/mod.rs:53)
// -> per-encoding IntoCanonical.  Where the reference materialises one buffer per cascade
// level (e.g. ALP -> FoR -> BitPacked is 3-4 passes, SURVEY.md §3 stack B) the planner
// recognises the cascade and issues ONE fused K1 launch (+ tiny patch scatters); anything it
// does not recognise is decoded child-first into temporaries exactly like the reference.
//
// No decode decision travels in Planner state.  A decode function launches at once unless its
// caller hands it a sink (K1Sink below; strings_into's FSST chunk list): only the chunk loop of a
// ChunkedArray makes one, and it reaches only the BitPacked leaf of a chunk that is one K1 decode.
// Which K1 kernel a launch takes is one rule, k1_choose (vxg_internal.hpp): launch_one switches on
// it and decode_alp asks it beforehand whether the launch will write its outer patches.
//
// Units: planner_launch.hip (launch grouping, K1 dispatch, the BitPacked buffer check),
// planner_decode.hip (primitives, validity, bools, canonical(), the cascade classifier),
// planner_strings.hip (string canonicalize, the string readers), planner_take.hip,
// planner_compare.hip (compare, compare_bytes, row_filter), planner_filter.hip (filter,
// filter_batch), plan.hip (the plan recorder), capi.hip (the context and the C entry points).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "chunk_pack.hpp"
#include "compare.hpp"
#include "compare_str.hpp"
#include "env.hpp"
#include "k1g.hpp"
#include "take.hpp"
#include "take_str.hpp"
#include "vxg_internal.hpp"

struct vxg_ctx {
    vxg::Ctx c;
};

#define VXG_TRY(expr)                         \
    do {                                      \
        vxg_status _s = (expr);               \
        if (_s != VXG_OK) return _s;          \
    } while (0)

namespace vxg {

inline hipStream_t S(void* s) { return static_cast<hipStream_t>(s); }

// Every entry point that takes a context starts here: its launches follow ctx's device and
// options (g_cur_ctx, vxg_internal.hpp).  The error text of a failed call is this host thread's
// (set_error; read back by vxg_last_error).
vxg_status use_device(vxg_ctx* ctx);
// The device error word's bits -> the VortexError variant each one stands for.
vxg_status status_of_err_word(uint32_t err);

inline bool is_string(const vxg_array& a) { return a.dtype == VXG_DTYPE_UTF8 || a.dtype == VXG_DTYPE_BINARY; }

// A recorded plan's deferred launches, shared by the planners of all its arrays: the K1 decodes,
// RunEnd expansions and string-dictionary views of every chunked column, launched together at
// the end of recording on one graph branch (dictionary views, then one launch per large K1 kernel
// group + one K1g launch for all the small ones, then the expansions), instead of per column.
struct PlanBatch {
    struct Run {
        int w;             // value width
        RunEndChunk c;
        bool indep;        // ends/values read in place (no K1 decode of this batch feeds it)
    };
    std::vector<VarBinChunk> dicts;
    std::vector<K1Job> jobs;
    std::vector<Run> runs;
    std::vector<FsstChunk> fssts;  // FSST chunks of chunked columns
    bool empty() const { return dicts.empty() && jobs.empty() && runs.empty() && fssts.empty(); }
};

// ---- launch grouping (planner_launch.hip) ---------------------------------------------------
// Validate one BitPacked buffer (bitpacking/mod.rs:54-130): the slice offset, the bit width against
// the type's T bits, the byte count of the 1024-row blocks and, for the kernels that read 16-byte
// words (`aligned`), the pointer.  *nblk: the blocks that len + offset rows cover.
vxg_status check_bitpacked(int T, unsigned W, unsigned offset, uint64_t len, const void* packed, uint64_t packed_bytes,
                           bool aligned, uint64_t* nblk);
// check_bitpacked (aligned), then describe the buffer's K1 decode.
vxg_status make_k1_job(int T, unsigned W, unsigned offset, uint64_t len, const void* packed, uint64_t packed_bytes,
                       Epi epi, int vw, const UnpackArgs& a, void* out, K1Job& j);
// K1 jobs launched now, grouped by kernel; dt: the plan being recorded, or null; patch: the outer
// patches of the single array that `jobs` decodes, written by its K1w launch (k1_choose), or null.
vxg_status launch_k1_jobs(std::vector<K1Job>& jobs, uint32_t* err, hipStream_t s, DevTables* dt, const PatchCol* patch);
vxg_status launch_runs(std::vector<RunEndChunk> runs, int w, uint32_t* err, hipStream_t s, DevTables* dt);
vxg_status launch_varbin_dicts(const std::vector<VarBinChunk>& dicts, uint32_t* err, hipStream_t s, DevTables* dt);
vxg_status flush_plan_batch(PlanBatch& b, uint32_t* err, hipStream_t s, DevTables* dt);

// ---- decode sinks ----------------------------------------------------------------------------
// A patch scatter that must follow a queued K1 decode.
struct PatchJob {
    const vxg_array* sp;
    int T;
    Epi epi;
    int vw;
    UnpackArgs a;
    void* dst;
    uint64_t out_len;
};
// Where the K1 decode of a single-K1 cascade (Planner::k1_fusable) goes instead of its own launch:
// into the chunk loop's shared launches, its patch scatters after them in queue order.  A decode
// function launches at once unless it is handed a sink, and hands it on only to the BitPacked
// leaf of that cascade -- never to a child it decodes into a temporary -- so no nested array can
// queue into a loop that does not know of it.  The FSST chunks of a chunked string array travel
// the same way (strings_into's std::vector<FsstChunk>*).
struct K1Sink { std::vector<K1Job>& jobs; std::vector<PatchJob>& patches; };

// ===================================================================================
// Planner
// ===================================================================================
class Planner {
  public:
    Planner(vxg_ctx* ctx, hipStream_t s, DevTables* plan = nullptr, PlanBatch* batch = nullptr)
        : ctx_(ctx), s_(s), plan_(plan), batch_(batch) {}
    ~Planner() {
        for (void* p : temps_) (void)hipFreeAsync(p, s_);
    }

    vxg_status canonical(const vxg_array& a, vxg_canonical& out);
    // compute::take on the compressed tree (take.hip, take_str.hip): the rows at the indices +
    // validity.take(indices); flags: VXG_TAKE_*; info: what ran
    vxg_status take(const vxg_array& a, const void* idx, int iw, bool isg, uint64_t n, uint32_t flags, vxg_canonical& out,
                    vxg_take_info& info);
    // compute::filter (filter.hip): the rows whose predicate bit is set + validity.filter
    vxg_status filter(const vxg_array& a, const vxg_array& pred, vxg_canonical& out);
    // filter(batch, mask) (filter_packed.hip): every column by one device mask, counted and scanned
    // once; packed cascades are filtered where they lie.  The arguments are the entry point's,
    // checked there.
    vxg_status filter_batch(const vxg_array* const* cols, uint32_t n_cols, const void* mask, uint64_t n, uint32_t flags,
                            vxg_canonical* outs, uint64_t* true_count, vxg_filter_batch_info& info);
    // compute::compare with a scalar (compare.hip): a Bool canonical, bit i = op(value i, scalar)
    vxg_status compare(const vxg_array& a, int op, uint64_t scalar_bits, uint32_t flags, vxg_canonical& out,
                       vxg_compare_info& info);
    // compute::compare of a utf8/binary array with a scalar (compare_str.hip)
    vxg_status compare_bytes(const vxg_array& a, int op, const void* scalar_host, uint64_t scalar_len, uint32_t flags,
                             vxg_canonical& out, vxg_compare_bytes_info& info);
    // RowFilter::evaluate (filtering.rs:27-43): the AND of the conjuncts' null_as_false compares and,
    // with count_dev, its true count; a range on one column node is one two-sided compare
    // (compare_range.hip).  The arguments are the entry point's, checked there.
    vxg_status row_filter(const vxg_predicate* preds, uint32_t n_preds, uint32_t flags, vxg_canonical& out,
                          uint64_t* count_dev, vxg_row_filter_info& info);
    vxg_status canonical_size(const vxg_array& a, uint64_t& vb, uint64_t& db);
    // A size / layout query (vxg_canonical_size, vxg_canonical_layout): it is handed no stream, so
    // where it has to read the device (string_layout's FSST sums) it first waits for the whole
    // device -- the caller's uploads may be enqueued on any stream.
    void as_query() { query_ = true; }
    // Data buffers of a string canonical, placed 16-byte aligned in one allocation.
    vxg_status string_layout(const vxg_array& a, std::vector<vxg_data_buffer>& bufs, uint64_t& extent);
    static vxg_status string_buffer_count(const vxg_array& a, uint32_t& n);

  private:
    vxg_ctx* ctx_;
    hipStream_t s_;
    std::vector<void*> temps_;
    bool query_ = false;  // as_query()
    // Recording a plan: temporaries are plain allocations owned by the plan (alive for all its
    // replays) instead of stream-ordered ones, and chunk tables longer than a kernel argument
    // holds become device tables (one launch per kernel group).
    DevTables* plan_ = nullptr;
    PlanBatch* batch_ = nullptr;  // a plan's deferred launches (all its arrays), or null
    // The array canonical() was called on.  Only a ChunkedArray that IS this root defers its
    // launches into batch_: its chunks write straight into the caller's output and nothing
    // recorded after it reads them.  A nested ChunkedArray (Dict values, FoR/ZigZag/ALP child,
    // Sparse/RunEnd children, views of a string dictionary) feeds a consumer recorded right
    // after it, so it launches immediately.
    const vxg_array* root_ = nullptr;
    bool defer(const vxg_array& a) const { return batch_ && &a == root_; }
    // `c` decodes as one K1 launch (+ patch scatters): what a K1Sink may be handed to.
    bool k1_fusable(const vxg_array& c) const;

    vxg_status temp(uint64_t bytes, void** p) {
        if (bytes == 0) bytes = 16;
        if (plan_) {
            VXG_TRY(hip_check(hipMalloc(p, (bytes + 15) & ~15ull), "hipMalloc (plan temporary)"));
            plan_->allocs.push_back(*p);
            return VXG_OK;
        }
        VXG_TRY(hip_check(hipMallocAsync(p, (bytes + 15) & ~15ull, s_), "hipMallocAsync"));
        temps_.push_back(*p);
        return VXG_OK;
    }

    static bool is_primitive_dtype(const vxg_array& a) { return a.dtype == VXG_DTYPE_PRIMITIVE; }
    static int width(const vxg_array& a) { return ptype_width(a.ptype); }

    const vxg_buffer* buf(const vxg_array& a, uint32_t i) const {
        return i < a.n_buffers ? &a.buffers[i] : nullptr;
    }
    const vxg_array* child(const vxg_array& a, uint32_t i) const {
        return i < a.n_children ? &a.children[i] : nullptr;
    }

    // Decode a primitive-typed array into dst (len * width bytes, 16-B aligned).  With a sink, `a`
    // is k1_fusable and its one K1 decode is queued (K1Sink).
    vxg_status decode_into(const vxg_array& a, void* dst, K1Sink* sink = nullptr);
    // Canonical primitive values of `a` as a device pointer (aliases PRIMITIVE buffers).
    vxg_status view_primitive(const vxg_array& a, const void** p);
    vxg_status int_column(const vxg_array& a, IntCol& c);
    // a patch-free 32/64-bit [FoR](BitPacked) integer column as a packed IntCol (*packed = true),
    // validated; otherwise *packed = false and nothing is decoded
    vxg_status packed_column(const vxg_array& a, IntCol& c, bool* packed);
    vxg_status runend_column(const vxg_array& a, bool in_place, IntCol& c);
    // `c` is FoR(BitPacked) or BitPacked: the BitPacked leaf, with the FoR's reference and shift
    // (left as they are for a bare BitPacked); anything else: null.
    const vxg_array* fl_leaf(const vxg_array* c, uint64_t* reference, uint32_t* shift) const;
    // ALP's decode factors F10[f] and IF10[e] of an f32 / f64 array (alp/compress.rs:61-78); false
    // when an exponent lies outside the ptype's table.
    static bool alp_factors(const vxg_array& a, double* alp_a, double* alp_b);
    // A BitPacked-rooted cascade that one fused kernel serves -- BitPacked, FoR(BitPacked), ZigZag or
    // ALP over either, the leaf of the array's own width and length -- with its packed buffer
    // validated (check_bitpacked).  take, compare and filter_batch build their kernel arguments
    // from it.
    struct Cascade {
        const vxg_array* bp = nullptr;     // the BitPacked leaf; null: not a served shape
        const vxg_array* outer = nullptr;  // ALP's patches, named even where the shape is not served
        int T = 0;                         // bits of the leaf's type
        Epi epi = Epi::Plain;
        EpiParams ep{};                    // reference, shift, alp_a, alp_b
        const uint8_t* packed = nullptr;
        unsigned W = 0, offset = 0;
    };
    // `aligned`: the kernel reads the packed buffer in 16-byte words
    vxg_status classify_cascade(const vxg_array& a, bool aligned, Cascade& c);

    // A BitPacked array under the epilogue of its parents: validate it and describe its K1 decode
    // (*patches: its patches child, or null), then queue the decode into `sink` or, without one,
    // launch it (+ the patch scatter) now -- `fused`: outer patches the launch itself writes.
    vxg_status describe_bitpacked(const vxg_array& bp, Epi epi, int vw, UnpackArgs& a, void* dst, K1Job& j,
                                  const vxg_array** patches);
    vxg_status submit_k1(const K1Job& j, const vxg_array* patches, const UnpackArgs& a, K1Sink* sink, const PatchCol* fused);
    vxg_status decode_bitpacked(const vxg_array& bp, Epi epi, int vw, UnpackArgs a, void* dst, K1Sink* sink);
    bool patch_fusable(const vxg_array& sparse, int value_width) const;
    vxg_status sparse_patch_col(const vxg_array& sparse, PatchCol& pc);
    vxg_status apply_sparse_patches(const vxg_array& sparse, int T, Epi epi, int vw, const UnpackArgs& a,
                                    void* dst, uint64_t out_len);
    vxg_status decode_alp(const vxg_array& a, void* dst, K1Sink* sink);
    vxg_status decode_dict_primitive(const vxg_array& a, void* dst, K1Sink* sink);
    vxg_status decode_chunked_primitive(const vxg_array& a, void* dst);
    vxg_status decode_alprd(const vxg_array& a, void* dst);
    vxg_status decode_sparse_values(const vxg_array& a, void* dst);

    // filter() after the count: canonicalize `a` into temporaries, compact by the counted mask
    vxg_status filter_selected(const vxg_array& a, const uint64_t* m, const uint64_t* to, uint64_t k, vxg_canonical& out,
                               uint32_t* syncs);

    vxg_take_info* tinfo_ = nullptr;  // take(): the counters of the call under way
    vxg_status take_values(const vxg_array& a, const void* idx, int iw, bool isg, uint64_t n, void* dst);
    vxg_status take_codes(const vxg_array& codes, const void* idx, int iw, bool isg, uint64_t n, void* dst);
    vxg_status take_validity(const vxg_array& a, const void* idx, int iw, bool isg, uint64_t n, vxg_canonical& out);
    vxg_status take_strings(const vxg_array& a, const void* idx, int iw, bool isg, uint64_t n, bool force,
                            vxg_canonical& out, vxg_take_info& info);
    vxg_status take_patches(const vxg_array& sp, TakePatches& p);
    // A cascade the fused compare kernel serves (compare, filter_batch): the launch's share
    // (CmpJob, chunk_pack.hpp) and what the patch launches after it need.
    struct CmpFused : CmpJob {
        const vxg_array* arr;    // the array or chunk
        const vxg_array* bp;     // its BitPacked leaf
        const vxg_array* outer;  // ALP patches, or null
        EpiParams ep;
    };
    vxg_status compare_shape(const vxg_array& a, uint64_t out_bit, CmpFused& f, bool* fused);
    // compare(); with `range`, both tests of a range in the same walk and launches
    vxg_status compare_impl(const vxg_array& a, int op, uint64_t scalar_bits, const CmpRange* range, uint32_t flags,
                            vxg_canonical& out, vxg_compare_info& info);
    // The pieces of a compute call with their first rows: `a` itself, or the chunks of a top-level
    // Chunked (check_ptype: of a's ptype as well as its dtype; skip_empty: only those with rows).
    using Pieces = std::vector<std::pair<const vxg_array*, uint64_t>>;
    vxg_status chunk_pieces(const vxg_array& a, bool check_ptype, bool skip_empty, Pieces& pieces);
    // The header and value bitmap (whole u64 words, 8-byte aligned) of an n-row Bool result;
    // `what` names the call in the error texts.
    vxg_status bool_output(uint64_t n, const char* what, vxg_canonical& out);
    // The end of a compare: the value bits of null rows cleared and, unless null_as_false, the
    // validity handed out.
    vxg_status compare_validity(const vxg_array& a, uint32_t flags, vxg_canonical& out);
    // The children of a VarBin / VarBinView / FSST array, checked and read where they lie.
    struct VarBinSrc {
        const uint8_t* bytes;
        uint64_t bytes_len;
        CCol offs;
    };
    struct ViewSrc {
        const uint8_t* views;  // 16-byte aligned
        std::vector<StrBuf> bufs;
    };
    struct FsstSrc {
        const uint64_t* symbols;
        const uint8_t* sym_lens;
        const uint8_t* codes;
        uint64_t codes_len;
        CCol offs, lens;
        uint32_t n_symbols;
    };
    vxg_status string_bytes(const vxg_array& b, const void** p);
    vxg_status read_varbin(const vxg_array& s, VarBinSrc& v);
    vxg_status read_varbinview(const vxg_array& s, ViewSrc& v);
    vxg_status read_fsst(const vxg_array& s, FsstSrc& f);
    // The canonical of string array `s` in temporaries: src.views, src.data under the layout `lay`
    // (src.data_buffers points into it) and src.validity (null: no nulls).
    vxg_status string_canonical_temp(const vxg_array& s, vxg_canonical& src, std::vector<vxg_data_buffer>& lay);
    // The one heap of a take's or filter's string result, its size known: checked against the
    // caller's buffer or allocated.  op / rows name the call in the error texts ("take" / "taken").
    vxg_status size_string_heap(vxg_canonical& out, uint64_t heap, const char* op, const char* rows);
    // One u64 from device memory, waited for; `what` names it in the error texts.
    vxg_status read_u64(const uint64_t* dev, const char* what, uint64_t* v);
    // The string pieces of one row-compare target (the output bitmap, or the truth tables of the
    // Dict pieces), by kernel.
    struct StrRows {
        std::vector<VbDictPiece> vbd;
        std::vector<VbPiece> vb;
        std::vector<ViewPiece> vw;
        std::vector<FsstPiece> fs;
    };
    vxg_status compare_rows_of(const vxg_array& s, uint64_t out_bit, bool excl, bool table, StrRows& rows, bool* fell_back);
    vxg_status launch_str_rows(StrRows& rows, const StrScalar& sc, void* out, int op, uint32_t& launches);
    vxg_status validity_into(const vxg_array& a, void** bitmap);
    // OR the values of a Bool-dtype array into the zeroed bit buffer `bits` at bit `off`.
    vxg_status bools_into(const vxg_array& a, void* bits, uint64_t off);
    vxg_status validity_source(const vxg_array& a, const vxg_array** node, int* kind);
    vxg_status string_canonical(const vxg_array& a, vxg_canonical& out);
    vxg_status string_lens(const vxg_array& a, std::vector<uint64_t>& lens,
                           std::vector<std::pair<size_t, const vxg_array*>>& fsst) const;
    vxg_status strings_into(const vxg_array& a, uint8_t* views, uint8_t* data, const vxg_data_buffer* bufs,
                            uint32_t bidx, const uint8_t* validity, std::vector<FsstChunk>* fsst_sink);
};

}  // namespace vxg
