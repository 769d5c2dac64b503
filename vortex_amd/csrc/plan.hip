// plan.hip — the plan recorder (prepared canonicalize): vxg_plan_create records the canonicalize
// of several arrays once into a HIP graph -- the arrays on parallel branches, the deferrable
// launches of chunked columns in one PlanBatch (planner.hpp) -- optionally as two candidates that
// are timed against each other, and vxg_plan_launch replays it (as direct kernel launches when the
// graph is one short chain).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <memory>

#include "k1g.hpp"
#include "planner.hpp"

using namespace vxg;

// Bytes a canonicalize of `a` moves (every buffer of the tree read once + the canonical
// output written): the plan's branch-balancing weight.
static uint64_t tree_bytes(const vxg_array& a) {
    uint64_t b = 0;
    for (uint32_t i = 0; i < a.n_buffers; i++) b += a.buffers[i].len;
    for (uint32_t i = 0; i < a.n_children; i++) b += tree_bytes(a.children[i]);
    return b;
}

// Encoding that decides an array's decode kernel: the first non-Chunked node of its tree.
static uint16_t leading_encoding(const vxg_array& a) {
    return a.encoding == VXG_ENC_CHUNKED && a.n_children ? leading_encoding(a.children[0]) : a.encoding;
}

// Bytes of the canonical values (or views) of `a`.
static uint64_t canonical_out_bytes(const vxg_array& a) {
    return a.dtype == VXG_DTYPE_BOOL ? a.len / 8 : a.len * (is_string(a) ? 16 : ptype_width(a.ptype));
}

// Branch-balancing weight: estimated device time ~ bytes moved / the kernel's measured fraction
// of the HBM roofline (round 3, each lineitem column alone, profiles/r03_c5_columns_w1.jsonl):
// FSST 0.45, string dictionaries (16-byte views) 0.55, short-run RunEnd 0.34, other decodes ~0.7.
static uint64_t plan_cost(const vxg_array& a) {
    const uint64_t bytes = tree_bytes(a) + canonical_out_bytes(a);
    const uint16_t e = leading_encoding(a);
    const uint64_t pct = e == VXG_ENC_FSST ? 45 : e == VXG_ENC_RUN_END ? 34 : is_string(a) ? 55 : 70;
    return bytes * 100 / pct;
}

// Parallel graph branches of a plan (VXG_PLAN_BRANCHES overrides, 1..16; 0 = unset).
static uint32_t plan_branches_env() {
    static const uint32_t nb = uint32_t(env_int("VXG_PLAN_BRANCHES", 1, 16, 0));
    return nb;
}

// Plan batching (PlanBatch + K1g).  Whether it pays depends on the table (round 4: C5 per GPU at
// 8 / 4 GPUs measured 0.060 / 0.095 ms batched vs 0.120 / 0.131 unbatched, but 0.200 vs 0.180 at
// 2 GPUs; mixing batched and unbatched arrays was slower than either).  So VXG_PLAN_MEASURE
// records the plan both ways (unbatched on 2 graph branches, batched on 1) and keeps one by
// vxg_plan_select (3 interleaved timed replays each after one warm-up).  The knob
// VXG_PLAN_BATCH (read at every create) is a diagnostic: "0" unbatched, "1" batched, "mixed"
// (arrays whose output is <= VXG_PLAN_BATCH_MAX_BYTES batched, the others not), unset = measured.
// "s" batches only the string-dictionary columns (one K1g launch for all of them on a branch
// of its own, the other columns unbatched).
enum class BatchMode { Auto, Off, On, Mixed, Strings };
static BatchMode plan_batch_mode() {
    const char* e = env_str("VXG_PLAN_BATCH");
    if (!e || !*e) return BatchMode::Auto;
    if (e[0] == '0') return BatchMode::Off;
    if (e[0] == '1') return BatchMode::On;
    if (e[0] == 'm') return BatchMode::Mixed;
    if (e[0] == 's') return BatchMode::Strings;
    return BatchMode::Auto;
}
// A string column whose leading encoding is Dict (C5's four Dict(VarBin) columns).
static bool dict_string_column(const vxg_array& a) {
    if (!is_string(a)) return false;
    if (a.encoding == VXG_ENC_CHUNKED) {
        for (uint32_t i = 1; i < a.n_children; i++)
            if (a.children[i].encoding != VXG_ENC_DICT) return false;
        return a.n_children > 1;
    }
    return a.encoding == VXG_ENC_DICT;
}
static uint64_t plan_batch_max_bytes() { return env_u64("VXG_PLAN_BATCH_MAX_BYTES", uint64_t(64) << 20); }
// vxg_plan_create without VXG_PLAN_MEASURE records one candidate: batched.  (Round 4 kept
// unbatched plans above 400 MB of output: then every small-enough numeric column went to K1g's
// runtime-width body.  With K1g limited to groups below 20 MiB and the FSST decode inside the
// K1g launch, batched measured faster at every C5 size in round 5: 1 GPU 0.272 vs 0.289 ms,
// 2-GPU shard 0.145 vs 0.173, 4 0.072 vs 0.125, 8 0.042 vs 0.104.)

// A batched plan's fused FSST+K1g launch with the in-grid pre-pass (fsst.hip): its arguments live
// here so that every replay can give it a new record tag (FsstFusedArgs::tag).
struct FusedNode {
    FsstFusedArgs fa;
    const GenChunk* gtab;
    uint32_t gn, dict_off;
    bool dict_lds;
    uint32_t* err;
    uint64_t gpe;
    void* args[7];
    hipGraphNode_t node = nullptr;
    hipKernelNodeParams p{};
    explicit FusedNode(void** a) {
        fa = *static_cast<const FsstFusedArgs*>(a[0]);
        gtab = *static_cast<const GenChunk* const*>(a[1]);
        gn = *static_cast<const uint32_t*>(a[2]);
        dict_off = *static_cast<const uint32_t*>(a[3]);
        dict_lds = *static_cast<const bool*>(a[4]);
        err = *static_cast<uint32_t* const*>(a[5]);
        gpe = *static_cast<const uint64_t*>(a[6]);
        void* const mine[7] = {&fa, &gtab, &gn, &dict_off, &dict_lds, &err, &gpe};
        std::copy(mine, mine + 7, args);
    }
};

struct vxg_plan {
    vxg_ctx* ctx = nullptr;
    std::vector<std::unique_ptr<FusedNode>> fused;  // in-grid pre-pass launches (tag per replay)
    uint64_t launches = 0;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    DevTables store;  // the recorded launches' temporaries and device chunk tables
    // A recorded graph that is one short chain of kernels (a sharded scan after batching:
    // FSST pre-pass -> decode -> K1g) replays as direct launches of its kernel nodes: one stream,
    // no graph-to-graph dependency (a graph replay boundary cost ~14 us on the C5 shard).
    std::vector<hipKernelNodeParams> direct;
    bool batched = false;  // recorded with a PlanBatch (diagnostics)
    uint32_t branches = 0;
    vxg_plan_info info{};  // filled by vxg_plan_create_ex
};

// Direct replay of short kernel chains (VXG_PLAN_DIRECT=0 disables; at most
// VXG_PLAN_DIRECT_MAX nodes, default 16: C5's 1-GPU batched chain is 9 kernels, 0.2745 ms per
// step as a graph vs 0.2719 direct).  Read at every plan recording.
static size_t plan_direct_max() { return size_t(env_u64("VXG_PLAN_DIRECT_MAX", 16)); }
static bool plan_direct_enabled() { return env_flag("VXG_PLAN_DIRECT", true); }

// The kernel nodes of `g` in order if g is a chain of <= plan_direct_max() kernel nodes, else empty.
static std::vector<hipKernelNodeParams> kernel_chain(hipGraph_t g) {
    std::vector<hipKernelNodeParams> out;
    size_t nn = 0;
    if (hipGraphGetNodes(g, nullptr, &nn) != hipSuccess || nn == 0 || nn > plan_direct_max()) return out;
    std::vector<hipGraphNode_t> nodes(nn);
    if (hipGraphGetNodes(g, nodes.data(), &nn) != hipSuccess) return out;
    std::vector<hipGraphNode_t> dep(nn, nullptr);
    size_t roots = 0, root = 0;
    for (size_t i = 0; i < nn; i++) {
        hipGraphNodeType t{};
        if (hipGraphNodeGetType(nodes[i], &t) != hipSuccess || t != hipGraphNodeTypeKernel) {
            if (env_str("VXG_PLAN_DEBUG")) std::fprintf(stderr, "plan: node %zu of %zu has type %d\n", i, nn, int(t));
            return out;
        }
        size_t nd = 0;
        if (hipGraphNodeGetDependencies(nodes[i], nullptr, &nd) != hipSuccess || nd > 1) return out;
        if (nd == 1 && hipGraphNodeGetDependencies(nodes[i], &dep[i], &nd) != hipSuccess) return out;
        if (nd == 0) {
            roots++;
            root = i;
        }
    }
    if (roots != 1) return out;
    std::vector<size_t> order{root};
    while (order.size() < nn) {  // the unique node depending on the last one
        size_t next = nn, cnt = 0;
        for (size_t i = 0; i < nn; i++)
            if (dep[i] == nodes[order.back()]) {
                next = i;
                cnt++;
            }
        if (cnt != 1) return out;
        order.push_back(next);
    }
    for (size_t i : order) {
        hipKernelNodeParams p{};
        if (hipGraphKernelNodeGetParams(nodes[i], &p) != hipSuccess || p.extra || !p.kernelParams || !p.func) {
            out.clear();
            return out;
        }
        out.push_back(p);
    }
    return out;
}

// The plan's fused launches with an in-grid pre-pass: arguments copied into the plan (the direct
// chain's entry repointed at them; graph replays set them on the executable graph).
static vxg_status bind_fused_nodes(vxg_plan* pl, hipGraph_t g) {
    size_t nn = 0;
    if (hipGraphGetNodes(g, nullptr, &nn) != hipSuccess) return set_error(VXG_ERR_ASSERTION_FAILED, "graph nodes");
    std::vector<hipGraphNode_t> nodes(nn);
    if (nn && hipGraphGetNodes(g, nodes.data(), &nn) != hipSuccess) return set_error(VXG_ERR_ASSERTION_FAILED, "graph nodes");
    for (hipGraphNode_t nd : nodes) {
        hipGraphNodeType t{};
        if (hipGraphNodeGetType(nd, &t) != hipSuccess || t != hipGraphNodeTypeKernel) continue;
        hipKernelNodeParams p{};
        if (hipGraphKernelNodeGetParams(nd, &p) != hipSuccess || !p.kernelParams || !is_fsst_fused_kernel(p.func)) continue;
        if (static_cast<const FsstFusedArgs*>(p.kernelParams[0])->prepass == 0) continue;
        auto f = std::make_unique<FusedNode>(p.kernelParams);
        f->node = nd;
        f->p = p;
        f->p.kernelParams = f->args;
        for (hipKernelNodeParams& d : pl->direct)
            if (d.func == p.func) d.kernelParams = f->args;  // (one fused launch per plan)
        pl->fused.push_back(std::move(f));
    }
    return VXG_OK;
}

// Record one candidate plan: arrays with batched[i] defer their deferrable launches into one
// PlanBatch flushed at the end; `branches` parallel graph branches (arrays spread longest-first).
static vxg_status record_plan(vxg_ctx* ctx, const vxg_array* arrays, vxg_canonical* outs, uint32_t n,
                              const std::vector<bool>& batched, uint32_t branches, vxg_plan** plan) {
    *plan = nullptr;
    const bool batching = std::find(batched.begin(), batched.end(), true) != batched.end();
    // Record on an origin stream forked into `branches` streams: the arrays are independent, so
    // their launches become parallel graph branches (the graph runs them on several hardware
    // queues, overlapping the ramp and drain of the many small kernels of a chunked scan), joined
    // back into the origin stream.  The batched arrays' deferrable launches (K1 decodes, RunEnd
    // expansions, dictionary views of chunked columns) go to one more branch -- or, with one
    // branch, follow the arrays on it (a single-stream graph) -- recorded after every array.
    const bool own = batching && branches > 1;
    const uint32_t nb = (n < branches ? (n ? n : 1) : branches) + (own ? 1 : 0);
    const uint32_t na = own ? nb - 1 : nb;  // branches the arrays are spread over
    PlanBatch batch;
    hipStream_t cs;
    VXG_TRY(hip_check(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking), "plan stream"));
    std::vector<hipStream_t> br(nb, nullptr);
    std::vector<hipEvent_t> ev(nb + 1, nullptr);
    vxg_status st = VXG_OK;
    for (uint32_t b = 0; b < nb && st == VXG_OK; b++)
        st = hip_check(hipStreamCreateWithFlags(&br[b], hipStreamNonBlocking), "plan branch stream");
    for (uint32_t b = 0; b <= nb && st == VXG_OK; b++)
        st = hip_check(hipEventCreateWithFlags(&ev[b], hipEventDisableTiming), "plan event");
    auto* pl = new vxg_plan();
    pl->ctx = ctx;
    pl->batched = batching;
    pl->branches = na;
    if (st == VXG_OK) st = hip_check(hipStreamBeginCapture(cs, hipStreamCaptureModeRelaxed), "hipStreamBeginCapture");
    if (st == VXG_OK) {
        st = hip_check(hipEventRecord(ev[nb], cs), "fork");
        for (uint32_t b = 0; b < nb && st == VXG_OK; b++)
            st = hip_check(hipStreamWaitEvent(br[b], ev[nb], 0), "fork wait");
        // longest-processing-time-first: arrays in decreasing order of the bytes their decode
        // moves, each onto the branch with the least work so far, so one heavy column (C5's
        // l_comment) does not queue behind others on its branch
        std::vector<uint32_t> order(n);
        std::vector<uint64_t> cost(n), load(na, 0);
        for (uint32_t i = 0; i < n; i++) {
            order[i] = i;
            cost[i] = plan_cost(arrays[i]);
        }
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return cost[x] > cost[y]; });
        for (uint32_t k = 0; k < n && st == VXG_OK; k++) {
            const uint32_t i = order[k];
            const uint32_t b = uint32_t(std::min_element(load.begin(), load.end()) - load.begin());
            if (!(own && batched[i])) load[b] += cost[i];  // (a batched array's launches run on the batch branch)
            Planner p(ctx, br[b], &pl->store, batched[i] ? &batch : nullptr);
            st = p.canonical(arrays[i], outs[i]);
        }
        // A batch on its own branch waits for every array branch first: deferred
        // launches read what those branches wrote -- a chunked FSST column's per-chunk validity
        // bitmaps, a Dict chunk's decoded values -- and nothing else orders the two streams.
        for (uint32_t b = 0; own && b < na && st == VXG_OK; b++) {
            st = hip_check(hipEventRecord(ev[b], br[b]), "batch join");
            if (st == VXG_OK) st = hip_check(hipStreamWaitEvent(br[nb - 1], ev[b], 0), "batch join wait");
        }
        if (batching && st == VXG_OK) st = flush_plan_batch(batch, ctx->c.err_word, br[nb - 1], &pl->store);
        for (uint32_t b = 0; b < nb && st == VXG_OK; b++) {
            st = hip_check(hipEventRecord(ev[b], br[b]), "join");
            if (st == VXG_OK) st = hip_check(hipStreamWaitEvent(cs, ev[b], 0), "join wait");
        }
        hipGraph_t g = nullptr;
        const hipError_t e = hipStreamEndCapture(cs, &g);
        if (st == VXG_OK) st = hip_check(e, "hipStreamEndCapture");
        pl->graph = g;
        if (st == VXG_OK && env_str("VXG_PLAN_DOT")) {  // diagnostics: PREFIX_<n>.dot per recorded graph
            static int cnt = 0;
            const std::string path = std::string(env_str("VXG_PLAN_DOT")) + "_" + std::to_string(cnt++) + ".dot";
            (void)hipGraphDebugDotPrint(g, path.c_str(), 0);
        }
        if (st == VXG_OK)
            st = hip_check(hipGraphInstantiate(&pl->exec, g, nullptr, nullptr, 0), "hipGraphInstantiate");
        if (st == VXG_OK) st = pl->store.upload();  // device chunk tables, once for all replays
        if (st == VXG_OK && plan_direct_enabled()) pl->direct = kernel_chain(g);
        if (st == VXG_OK) st = bind_fused_nodes(pl, g);
    }
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    for (hipStream_t b : br)
        if (b) (void)hipStreamDestroy(b);
    (void)hipStreamDestroy(cs);
    if (st == VXG_OK) *plan = pl;
    else vxg_plan_destroy(pl);
    return st;
}

// Median device time of `reps` interleaved replays of each candidate (after one warm-up each).
static vxg_status time_plans(const std::vector<vxg_plan*>& cands, int reps, std::vector<float>* ms) {
    hipStream_t s;
    VXG_TRY(hip_check(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "plan timing stream"));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    vxg_status st = hip_check(hipEventCreate(&e0), "plan timing event");
    if (st == VXG_OK) st = hip_check(hipEventCreate(&e1), "plan timing event");
    std::vector<std::vector<float>> t(cands.size());
    for (vxg_plan* p : cands)
        if (st == VXG_OK) st = vxg_plan_launch(p, s);
    for (int r = 0; r < reps && st == VXG_OK; r++) {
        for (size_t c = 0; c < cands.size() && st == VXG_OK; c++) {
            st = hip_check(hipEventRecord(e0, s), "plan timing");
            if (st == VXG_OK) st = vxg_plan_launch(cands[c], s);
            if (st == VXG_OK) st = hip_check(hipEventRecord(e1, s), "plan timing");
            if (st == VXG_OK) st = hip_check(hipEventSynchronize(e1), "plan timing");
            float x = 0;
            if (st == VXG_OK) st = hip_check(hipEventElapsedTime(&x, e0, e1), "plan timing");
            t[c].push_back(x);
        }
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
    ms->clear();
    for (auto& v : t) {
        std::sort(v.begin(), v.end());
        ms->push_back(v.empty() ? 0.f : v[v.size() / 2]);
    }
    return st;
}

// Graph nodes + dependency edges: what a replay pays beyond its kernels (each cross-branch edge
// is a queue synchronisation; a direct chain replays with no graph at all).
static uint32_t graph_cost(hipGraph_t g) {
    size_t nn = 0, ne = 0;
    if (!g || hipGraphGetNodes(g, nullptr, &nn) != hipSuccess) return 0;
    if (hipGraphGetEdges(g, nullptr, nullptr, &ne) != hipSuccess) ne = 0;
    return uint32_t(nn + ne);
}

extern "C" {

uint32_t vxg_plan_select(const float* ms, const uint32_t* cost, uint32_t n, uint32_t* selection) {
    uint32_t sel = VXG_PLAN_SEL_SINGLE, best = 0;
    if (n > 1 && !ms) {  // unmeasured: the smallest graph
        sel = VXG_PLAN_SEL_UNMEASURED;
        for (uint32_t c = 1; c < n; c++)
            if (cost && cost[c] < cost[best]) best = c;
    } else if (n > 1) {
        uint32_t fastest = 0;
        for (uint32_t c = 1; c < n; c++)
            if (ms[c] < ms[fastest]) fastest = c;
        best = fastest;
        sel = VXG_PLAN_SEL_FASTER;
        // candidates within 3 % of the fastest are equal: the smallest graph among them, the
        // lowest index on equal cost
        for (uint32_t c = 0; c < n; c++) {
            if (c == fastest || !(ms[c] <= ms[fastest] * 1.03f)) continue;
            sel = VXG_PLAN_SEL_TIE_COST;
            if (!cost) continue;
            if (cost[c] < cost[best] || (cost[c] == cost[best] && c < best)) best = c;
        }
    }
    if (selection) *selection = sel;
    return best;
}

vxg_status vxg_plan_create(vxg_ctx* ctx, const vxg_array* arrays, vxg_canonical* outs, uint32_t n, vxg_plan** plan) {
    return vxg_plan_create_ex(ctx, arrays, outs, n, 0, plan);
}

vxg_status vxg_plan_create_ex(vxg_ctx* ctx, const vxg_array* arrays, vxg_canonical* outs, uint32_t n,
                              uint32_t flags, vxg_plan** plan) {
    const auto t0 = std::chrono::steady_clock::now();
    VXG_TRY(use_device(ctx));
    if (!plan || (n && (!arrays || !outs))) return set_error(VXG_ERR_INVALID_ARGUMENT, "null plan/arrays/outs");
    if (flags & ~uint32_t(VXG_PLAN_MEASURE)) return set_error(VXG_ERR_INVALID_ARGUMENT, "unknown plan flags");
    *plan = nullptr;
    for (uint32_t i = 0; i < n; i++) {  // nothing may allocate or synchronise while recording
        const vxg_array& a = arrays[i];
        const vxg_canonical& o = outs[i];
        if (is_string(a) ? (!o.views || !o.data) : !o.values)
            return set_error(VXG_ERR_INVALID_ARGUMENT, "a plan needs caller-allocated outputs");
        if (a.nullable && !o.validity)
            return set_error(VXG_ERR_INVALID_ARGUMENT, "a plan needs caller-allocated validity for nullable arrays");
    }
    // candidates: (batched mask, branches); 2 branches unbatched (C5 at 1 GPU 322.6 us/replay vs
    // 362 with 1 and 348 with 3), 1 batched (each cross-branch edge costs a replay several
    // microseconds of queue synchronisation: C5 shard 82 -> 68 us)
    const uint32_t env_br = plan_branches_env();
    const std::vector<bool> none(n, false), all(n, true);
    std::vector<bool> mixed(n);
    for (uint32_t i = 0; i < n; i++) mixed[i] = canonical_out_bytes(arrays[i]) <= plan_batch_max_bytes();
    std::vector<std::pair<std::vector<bool>, uint32_t>> cand;
    const bool measure = (flags & VXG_PLAN_MEASURE) != 0;
    switch (plan_batch_mode()) {
    case BatchMode::Off: cand.emplace_back(none, env_br ? env_br : 2u); break;
    case BatchMode::On: cand.emplace_back(all, env_br ? env_br : 1u); break;
    case BatchMode::Mixed: cand.emplace_back(mixed, env_br ? env_br : 2u); break;
    case BatchMode::Strings: {
        std::vector<bool> strs(n);
        for (uint32_t i = 0; i < n; i++) strs[i] = dict_string_column(arrays[i]);
        cand.emplace_back(strs, env_br ? env_br : 2u);
        break;
    }
    case BatchMode::Auto:
        if (measure) {
            cand.emplace_back(none, env_br ? env_br : 2u);
            if (n) cand.emplace_back(all, env_br ? env_br : 1u);
        } else {
            cand.emplace_back(all, env_br ? env_br : 1u);
        }
        break;
    }
    std::vector<vxg_plan*> plans;
    vxg_status st = VXG_OK;
    for (const auto& [mask, branches] : cand) {
        vxg_plan* p = nullptr;
        st = record_plan(ctx, arrays, outs, n, mask, branches, &p);
        if (st != VXG_OK) break;
        plans.push_back(p);
    }
    size_t best = 0;
    uint32_t selection = VXG_PLAN_SEL_SINGLE;
    std::vector<float> ms(plans.size(), 0.f);
    std::vector<uint32_t> cost(plans.size(), 0);
    for (size_t c = 0; c < plans.size(); c++) cost[c] = graph_cost(plans[c]->graph);
    if (st == VXG_OK && measure && plans.size() > 1) {
        // the candidates read the inputs now: every upload the caller enqueued (any stream) first
        st = hip_check(hipDeviceSynchronize(), "plan create: device synchronize");
        uint32_t pending = 0;  // an error of the caller's earlier work: theirs to sync, not ours
        if (st == VXG_OK)
            st = hip_check(hipMemcpy(&pending, ctx->c.err_word, 4, hipMemcpyDeviceToHost), "error word readback");
        if (st == VXG_OK && pending) {
            best = vxg_plan_select(nullptr, cost.data(), uint32_t(plans.size()), &selection);
        } else if (st == VXG_OK) {
            st = time_plans(plans, 3, &ms);
            if (st == VXG_OK) best = vxg_plan_select(ms.data(), cost.data(), uint32_t(plans.size()), &selection);
            if (st == VXG_OK) {  // errors the measured runs found belong to create, not the next sync
                uint32_t err = 0;
                st = hip_check(hipMemcpy(&err, ctx->c.err_word, 4, hipMemcpyDeviceToHost), "error word readback");
                if (st == VXG_OK && err) {
                    st = hip_check(hipMemset(ctx->c.err_word, 0, 4), "error word reset");
                    if (st == VXG_OK) st = status_of_err_word(err);
                }
            }
        }
        if (env_str("VXG_PLAN_DEBUG"))
            for (size_t c = 0; c < ms.size(); c++)
                std::fprintf(stderr, "plan candidate %zu (%s, %u branches, %zu kernel-chain nodes): %.4f ms%s\n", c,
                             plans[c]->batched ? "batched" : "unbatched", cand[c].second, plans[c]->direct.size(),
                             ms[c], c == best ? "  <- kept" : "");
    }
    if (st == VXG_OK && !plans.empty()) {
        vxg_plan_info& in = plans[best]->info;
        in.batched = plans[best]->batched;
        in.branches = plans[best]->branches;
        in.direct_nodes = uint32_t(plans[best]->direct.size());
        in.n_candidates = uint32_t(std::min<size_t>(plans.size(), 2));
        for (size_t c = 0; c < plans.size() && c < 2; c++) {
            in.candidate_batched[c] = plans[c]->batched;
            in.candidate_ms[c] = ms[c];
        }
        in.selection = selection;
        for (size_t c = 0; c < plans.size() && c < 2; c++) in.candidate_cost[c] = cost[c];
        in.create_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    for (size_t c = 0; c < plans.size(); c++)
        if (st != VXG_OK || c != best) vxg_plan_destroy(plans[c]);
    if (st == VXG_OK && !plans.empty()) *plan = plans[best];
    return st;
}

vxg_status vxg_plan_get_info(const vxg_plan* plan, vxg_plan_info* info) {
    if (!plan || !info) return set_error(VXG_ERR_INVALID_ARGUMENT, "null plan/info");
    *info = plan->info;
    return VXG_OK;
}

vxg_status vxg_plan_launch(vxg_plan* plan, void* stream) {
    if (!plan || !plan->exec) return set_error(VXG_ERR_INVALID_ARGUMENT, "null plan");
    VXG_TRY(use_device(plan->ctx));
    // a new record tag per launch for the in-grid pre-pass (the previous launch's records carry
    // the previous tag)
    const uint32_t tag = uint32_t(++plan->launches % 65535u) + 1u;
    for (auto& f : plan->fused) f->fa.tag = tag;
    if (!plan->direct.empty()) {
        for (const hipKernelNodeParams& p : plan->direct)
            VXG_TRY(hip_check(hipLaunchKernel(p.func, p.gridDim, p.blockDim, p.kernelParams, p.sharedMemBytes, S(stream)),
                              "plan kernel"));
        return VXG_OK;
    }
    for (auto& f : plan->fused)
        VXG_TRY(hip_check(hipGraphExecKernelNodeSetParams(plan->exec, f->node, &f->p), "plan fused launch tag"));
    return hip_check(hipGraphLaunch(plan->exec, S(stream)), "hipGraphLaunch");
}

vxg_status vxg_plan_destroy(vxg_plan* plan) {
    if (!plan) return VXG_OK;
    if (plan->ctx) (void)hipSetDevice(plan->ctx->c.device);
    if (plan->exec) (void)hipGraphExecDestroy(plan->exec);
    if (plan->graph) (void)hipGraphDestroy(plan->graph);
    if (!plan->store.allocs.empty()) (void)hipDeviceSynchronize();  // no replay may still use them
    for (void* p : plan->store.allocs) (void)hipFree(p);
    delete plan;
    return VXG_OK;
}

}  // extern "C"
