// planner_launch.hip — launch grouping and K1 dispatch: which kernel a FastLanes decode takes
// (launch_fl_unpack over the instantiation units, fl_inst.hip), and how the K1 decodes, RunEnd
// expansions and VarBin dictionaries of many chunks share launches -- chunk tables as kernel
// arguments, or device tables and the one K1g launch (k1g.hpp) while a plan is recorded
// (chunk_pack.hpp holds the table rule; chunked/canonical.rs:27-122 is what the launches compute).
#include <algorithm>
#include <tuple>

#include "chunk_pack.hpp"
#include "k1g.hpp"
#include "planner.hpp"

// Chunk tables travel as kernel arguments: they must fit the 4 KiB kernarg segment.
static_assert(sizeof(vxg::ChunkTable) <= 4096, "ChunkTable exceeds the kernarg limit");
static_assert(sizeof(vxg::FsstTable) <= 4096, "FsstTable exceeds the kernarg limit");
static_assert(sizeof(vxg::RunEndTable) <= 4096, "RunEndTable exceeds the kernarg limit");
static_assert(sizeof(vxg::VarBinTable) <= 4096, "VarBinTable exceeds the kernarg limit");
static_assert(sizeof(vxg::CmpTable) + 32 <= 4096, "CmpTable and the compare arguments exceed the kernarg limit");

namespace vxg {

void note_k1w_launch(uint32_t bpw, uint32_t bpw_max, uint64_t groups) {
    if (!g_cur_ctx) return;
    std::lock_guard<std::mutex> lk(g_cur_ctx->mu);
    LaunchStats& st = g_cur_ctx->st;
    st.k1w_min_bpw = st.k1w_launches == 0 ? bpw : std::min(st.k1w_min_bpw, bpw);
    st.k1w_max_bpw = st.k1w_launches == 0 ? bpw : std::max(st.k1w_max_bpw, bpw);
    st.k1w_launches++;
    st.k1w_last_bpw = bpw;
    st.k1w_last_bpw_max = bpw_max;
    st.k1w_last_groups = groups;
}

// K1 dispatch over the instantiation units.
vxg_status launch_fl_unpack(int T, int W, Epi epi, int vw, const ChunkTable& t, uint64_t g, hipStream_t s) {
    if (W < 0 || W > T) return set_error(VXG_ERR_INVALID_ARGUMENT, "bit width out of range");
    switch (epi) {
    case Epi::Plain:
    case Epi::For:
    case Epi::ForZigZag:
        switch (T) {
        case 8: return fl_plain_8(W, epi, t, g, s);
        case 16: return fl_plain_16(W, epi, t, g, s);
        case 32: return fl_plain_32(W, epi, t, g, s);
        case 64: return fl_plain_64(W, epi, t, g, s);
        }
        return set_error(VXG_ERR_INVALID_ARGUMENT, "bad FastLanes width");
    case Epi::AlpF32:
    case Epi::AlpF64:
        return fl_alp(T, W, epi, t, g, s);
    case Epi::Dict:
        if (W > kDictFusedMaxW) return VXG_ERR_NOT_IMPLEMENTED;
        switch (vw) {
        case 1: return fl_dict_1(T, W, t, g, s);
        case 2: return fl_dict_2(T, W, t, g, s);
        case 4: return fl_dict_4(T, W, t, g, s);
        // 8-byte values stay on K1 (C3, 8 KiB dictionaries: K1 4 % faster, profiles/r02_*)
        case 8: return fl_dict_8(T, W, t, g, s);
        // K14 for 16-byte values (the views of a string dictionary): 2.2-2.4x K1 on the
        // lineitem columns
        case 16: return launch_dict_rows(T, W, t, s);
        }
        return set_error(VXG_ERR_INVALID_ARGUMENT, "bad dictionary value width");
    }
    return VXG_ERR_INVALID_ARGUMENT;
}

static bool same_kernel(const K1Job& a, const K1Job& b) {
    return a.T == b.T && a.W == b.W && a.epi == b.epi && a.vw == b.vw && a.vb == b.vb;
}

// Output bytes below which a plan batch's kernel group goes to the one K1g launch instead of its
// own K1 launch (VXG_K1G_MAX_BYTES overrides; 0 disables K1g).  Round 5, C5 (same box, ms per
// step): 1 GPU 0.289 with 64 MiB (every numeric column in K1g: unbatched kept) vs 0.272 with
// 16 MiB (batched kept); 2-GPU shard 0.163 vs 0.145; 4-GPU shard 0.0715 vs 0.0784 (its 18 MB
// date-column group then leaves K1g); 8-GPU shard equal.  20 MiB sits between.
static uint64_t k1g_max_bytes() {
    static const uint64_t v = env_u64("VXG_K1G_MAX_BYTES", uint64_t(20) << 20);
    return v;
}

// Bytes of one output value of a K1 decode.
static int k1_out_width(int T, Epi epi, int vw) {
    return epi == Epi::Dict ? vw : (epi == Epi::AlpF32 ? 4 : (epi == Epi::AlpF64 ? 8 : T / 8));
}

// Sort `jobs` by kernel (T, W, epilogue, value width) and call group(i, j, out_bytes) for every
// run [i, j) of jobs with the same kernel, at most max_group jobs long; out_bytes = its output.
template <class Group>
static vxg_status for_each_kernel_group(std::vector<K1Job>& jobs, size_t max_group, Group group) {
    std::stable_sort(jobs.begin(), jobs.end(), [](const K1Job& a, const K1Job& b) {
        return std::make_tuple(a.T, a.W, int(a.epi), a.vw, a.vb) < std::make_tuple(b.T, b.W, int(b.epi), b.vw, b.vb);
    });
    for (size_t i = 0, j; i < jobs.size(); i = j) {
        uint64_t out_bytes = 0;
        for (j = i; j < jobs.size() && j - i < max_group && same_kernel(jobs[i], jobs[j]); j++)
            out_bytes += jobs[j].d.len * uint64_t(k1_out_width(jobs[j].T, jobs[j].epi, jobs[j].vw));
        VXG_TRY(group(i, j, out_bytes));
    }
    return VXG_OK;
}

// One kernel group's own launches: the chunk table as the kernel argument, kArgChunks jobs per
// launch (no device table, no upload, no host sync), or -- dt set, a longer group -- one launch
// over a device table.  Empty jobs take no part.  `patch`: the outer patches of a single array,
// written by its K1w launch.
static vxg_status launch_kernel_group(const K1Job* it, const K1Job* end, uint32_t* err, hipStream_t s, DevTables* dt,
                                      const PatchCol* patch) {
    const K1Job& k = *it;
    while (it != end) {
        ChunkTable tab{};
        tab.err = err;
        if (patch) tab.patch = *patch;
        uint64_t groups;
        VXG_TRY(pack_chunk_table(
            tab, it, end, dt, [](const K1Job& jb) { return jb.d.n_blocks ? &jb.d : nullptr; },
            [](const ChunkDev& c) { return (c.n_blocks + 31) / 32; }, &groups));
        if (tab.n) VXG_TRY(launch_fl_unpack(k.T, k.W, k.epi, k.vw, tab, groups, s));
    }
    return VXG_OK;
}

static void add_nonempty(std::vector<const K1Job*>& gen, const K1Job* it, const K1Job* end) {
    for (; it != end; ++it)
        if (it->d.n_blocks) gen.push_back(it);
}

// Launch K1 jobs now, grouped by kernel.  While a plan is recorded (dt set) a group of any size
// is one launch, and Dict-over-VarBin jobs (K1Job::vb, made for plans only) share one K1g launch.
// `patch` (one job only): see launch_kernel_group.
vxg_status launch_k1_jobs(std::vector<K1Job>& jobs, uint32_t* err, hipStream_t s, DevTables* dt, const PatchCol* patch) {
    if (patch && jobs.size() != 1) return set_error(VXG_ERR_INVALID_ARGUMENT, "internal: fused patches need a single K1 job");
    std::vector<const K1Job*> gen;
    VXG_TRY(for_each_kernel_group(jobs, dt ? jobs.size() : size_t(kArgChunks), [&](size_t i, size_t j, uint64_t) -> vxg_status {
        if (!jobs[i].vb) return launch_kernel_group(jobs.data() + i, jobs.data() + j, err, s, dt, patch);
        if (!dt) return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBin-dictionary K1 jobs need a plan");
        add_nonempty(gen, jobs.data() + i, jobs.data() + j);
        return VXG_OK;
    }));
    return gen.empty() ? VXG_OK : launch_k1g_jobs(gen, {}, FsstFused{}, err, s, *dt);
}

// A plan batch's K1 jobs: one launch over a device table per large kernel group, and ONE K1g
// launch (k1g.hpp) for all the groups whose output is small, gen_runs and the fused FSST group: a
// sharded scan's many small per-column kernels cost more in ramp, drain and graph edges than in
// data.
static vxg_status launch_plan_k1_jobs(std::vector<K1Job>& jobs, const std::vector<std::pair<int, RunEndChunk>>& gen_runs,
                                      const FsstFused& fuse, uint32_t* err, hipStream_t s, DevTables& dt) {
    std::vector<const K1Job*> gen;  // jobs for the shared K1g launch
    VXG_TRY(for_each_kernel_group(jobs, jobs.size(), [&](size_t i, size_t j, uint64_t out_bytes) -> vxg_status {
        if (const K1Job& k = jobs[i]; !k.vb && (out_bytes >= k1g_max_bytes() || gen_kind(k.T, int(k.epi), k.vw) < 0))
            return launch_kernel_group(jobs.data() + i, jobs.data() + j, err, s, &dt, nullptr);
        add_nonempty(gen, jobs.data() + i, jobs.data() + j);
        return VXG_OK;
    }));
    return launch_k1g_jobs(gen, gen_runs, fuse, err, s, dt);
}

// Validate one BitPacked buffer (bitpacking/mod.rs:54-130).
vxg_status check_bitpacked(int T, unsigned W, unsigned offset, uint64_t len, const void* packed, uint64_t packed_bytes,
                           bool aligned, uint64_t* nblk) {
    if (offset > 1023) return set_error(VXG_ERR_INVALID_ARGUMENT, "Offset must be less than full block, i.e. 1024");
    if (W > unsigned(T)) return set_error(VXG_ERR_INVALID_ARGUMENT, "Unsupported bit width");
    *nblk = (len + offset + 1023) / 1024;
    if (W > 0 && packed_bytes != *nblk * 128ull * W)  // bitpacking/mod.rs:80-88
        return set_error(VXG_ERR_INVALID_ARGUMENT, "Expected " + std::to_string(*nblk * 128ull * W) +
                                                       " packed bytes, got " + std::to_string(packed_bytes));
    if (aligned && W > 0 && (reinterpret_cast<uintptr_t>(packed) & 15))
        return set_error(VXG_ERR_INVALID_ARGUMENT, "packed buffer must be 16-byte aligned");
    return VXG_OK;
}

// Validate one BitPacked buffer and describe its K1 decode.
vxg_status make_k1_job(int T, unsigned W, unsigned offset, uint64_t len, const void* packed, uint64_t packed_bytes,
                       Epi epi, int vw, const UnpackArgs& a, void* out, K1Job& j) {
    uint64_t nblk;
    VXG_TRY(check_bitpacked(T, W, offset, len, packed, packed_bytes, true, &nblk));
    const int ow = k1_out_width(T, epi, vw);
    if (ow != 1 && ow != 2 && ow != 4 && ow != 8 && ow != 16)  // (a Dict value width of 0 would divide by zero below)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "value width must be 1, 2, 4, 8 or 16");
    if (reinterpret_cast<uintptr_t>(out) % uint64_t(ow))
        return set_error(VXG_ERR_INVALID_ARGUMENT, "output buffer must be aligned to the value width");
    if (epi == Epi::Dict && W > unsigned(kDictFusedMaxW)) return VXG_ERR_NOT_IMPLEMENTED;
    // every code is out of bounds of an empty dictionary (whose buffer may be null)
    if (epi == Epi::Dict && a.dict_len == 0 && len > 0)
        return set_error(VXG_ERR_OUT_OF_BOUNDS, "take: index out of bounds");
    j.T = T;
    j.W = int(W);
    j.epi = epi;
    j.vw = epi == Epi::Dict ? vw : 0;
    j.d = ChunkDev{};
    j.d.packed = static_cast<const uint8_t*>(packed);
    j.d.out = out;
    j.d.n_blocks = len ? nblk : 0;
    j.d.len = len;
    j.d.reference = a.reference;
    j.d.alp_a = a.alp_a;
    j.d.alp_b = a.alp_b;
    j.d.dict = a.dict;
    j.d.dict_len = a.dict_len;
    j.d.offset = offset;
    j.d.shift = a.shift;
    return VXG_OK;
}

// RunEnd expansions of one value width: short runs thread-per-run (K8r), long runs workgroup
// per kRunEndSpan outputs (K8), kRunEndArgChunks chunks per launch (a plan: one launch per kind
// over a device table).  Empty chunks are dropped up front.
vxg_status launch_runs(std::vector<RunEndChunk> runs, int w, uint32_t* err, hipStream_t s, DevTables* dt) {
    runs.erase(std::remove_if(runs.begin(), runs.end(), [](const RunEndChunk& r) { return r.len == 0; }), runs.end());
    std::vector<RunEndChunk> short_runs, long_runs;
    for (const RunEndChunk& r : runs) (r.len <= kRunEndShortRun * r.n_runs ? short_runs : long_runs).push_back(r);
    for (int pass = 0; pass < 2; pass++) {
        const std::vector<RunEndChunk>& rs = pass == 0 ? short_runs : long_runs;
        for (const RunEndChunk* it = rs.data(), * const end = rs.data() + rs.size(); it != end;) {
            RunEndTable tab{};
            tab.err = err;
            uint64_t groups;
            VXG_TRY(pack_chunk_table(
                tab, it, end, dt, [](const RunEndChunk& r) { return &r; },
                [pass](const RunEndChunk& r) {
                    return pass == 0 ? (r.n_runs + kRunEndRunsPerGroup - 1) / kRunEndRunsPerGroup
                                     : (r.len + kRunEndSpan - 1) / kRunEndSpan;
                },
                &groups));
            VXG_TRY(pass == 0 ? launch_runend_runs(w, tab, groups, s) : launch_runend_chunks(w, tab, groups, s));
        }
    }
    return VXG_OK;
}

// VXG_PLAN_FUSE=0 (read at every flush): a batched plan's FSST decode keeps its own launch
// instead of running inside the K1g launch (A/B).
static bool plan_fuse_enabled() { return env_flag("VXG_PLAN_FUSE", true); }

// Views (+ byte copies) of VarBin dictionaries, kVarBinArgChunks per launch (a plan: one launch
// over a device table).  An empty dictionary still gets one workgroup.
vxg_status launch_varbin_dicts(const std::vector<VarBinChunk>& dicts, uint32_t* err, hipStream_t s, DevTables* dt) {
    for (const VarBinChunk* it = dicts.data(), * const end = dicts.data() + dicts.size(); it != end;) {
        VarBinTable tab{};
        tab.err = err;
        uint64_t groups;
        VXG_TRY(pack_chunk_table(
            tab, it, end, dt, [](const VarBinChunk& d) { return &d; },
            [](const VarBinChunk& d) { return d.n ? (d.n + 255) / 256 : uint64_t(1); }, &groups));
        VXG_TRY(launch_varbin_chunks(tab, groups, s));
    }
    return VXG_OK;
}

vxg_status flush_plan_batch(PlanBatch& b, uint32_t* err, hipStream_t s, DevTables* dt) {
    // FSST chunks: pre-passes first; one accessor group's decode tiles then run inside the K1g
    // launch (fsst_k1g_kernel), beside the K1 jobs, the other groups' decodes here
    FsstFused ff;
    if (!b.fssts.empty()) {
        void* scratch = nullptr;
        VXG_TRY(hip_check(hipMalloc(&scratch, (fsst_chunks_scratch_bytes(b.fssts.data(), b.fssts.size()) + 15) & ~15ull),
                            "hipMalloc (plan FSST scratch)"));
        dt->allocs.push_back(scratch);
        VXG_TRY(launch_fsst_batch(b.fssts, scratch, err, s, dt, plan_fuse_enabled() ? &ff : nullptr));
    }
    VXG_TRY(launch_varbin_dicts(b.dicts, err, s, dt));
    // short-run expansions that read their children in place join the K1g launch; the others
    // follow the K1 decodes that produce their children
    std::vector<std::pair<int, RunEndChunk>> gen_runs;
    std::vector<PlanBatch::Run> rest;
    for (const PlanBatch::Run& r : b.runs) {
        if (r.c.len == 0) continue;
        if (r.indep && r.c.len <= kRunEndShortRun * r.c.n_runs && gen_runs_kind(r.w) >= 0) gen_runs.emplace_back(r.w, r.c);
        else rest.push_back(r);
    }
    VXG_TRY(launch_plan_k1_jobs(b.jobs, gen_runs, ff, err, s, *dt));
    std::vector<int> widths;
    for (const auto& r : rest) widths.push_back(r.w);
    std::sort(widths.begin(), widths.end());
    widths.erase(std::unique(widths.begin(), widths.end()), widths.end());
    for (int w : widths) {
        std::vector<RunEndChunk> rs;
        for (const auto& r : rest)
            if (r.w == w) rs.push_back(r.c);
        VXG_TRY(launch_runs(rs, w, err, s, dt));
    }
    return VXG_OK;
}

}  // namespace vxg
