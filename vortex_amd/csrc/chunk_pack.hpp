// chunk_pack.hpp — the one place that fills a launch's chunk table (vxg_internal.hpp: ChunkTable,
// RunEndTable, VarBinTable; compare.hpp: CmpTable, at the end).
//
// The rule: up to the table's capacity the entries travel in the kernel argument (tab.c); while a
// plan is recorded (dt set) a longer list becomes ONE device table of any length (tab.ext, built
// in a host mirror that DevTables uploads when the plan is finalised).  Outside a plan a longer
// list is split: each call takes the next launch's share.
#pragma once

#include <algorithm>
#include <tuple>
#include <type_traits>
#include <vector>

#include "compare.hpp"
#include "vxg_internal.hpp"

namespace vxg {

// Fill `tab` (zeroed but for the caller's own fields) with the next launch's entries of [it, end)
// and advance `it` past them.  entry(*it) is the element's table entry, or null for an element
// that takes no part in the launch (the caller's rule for empty chunks); groups_of(entry) its
// workgroup count.  Sets tab.n, tab.ext (and tab.host where the table has one) and every
// first_group; *groups is the launch's workgroup total.  tab.n == 0: nothing to launch.
template <class Tab, class It, class Entry, class Groups>
vxg_status pack_chunk_table(Tab& tab, It& it, It end, DevTables* dt, Entry entry, Groups groups_of, uint64_t* groups) {
    using E = std::remove_reference_t<decltype(tab.c[0])>;
    constexpr size_t cap = sizeof(tab.c) / sizeof(tab.c[0]);
    size_t take = 0;
    for (It k = it; k != end; ++k) take += entry(*k) != nullptr;
    E* cs = tab.c;
    if (dt && take > cap) {
        if (take > 0xFFFFFFFFull) return set_error(VXG_ERR_INVALID_ARGUMENT, "too many chunks");
        E* host;
        const vxg_status st = dt->table(take, &host, &tab.ext);
        if (st != VXG_OK) return st;
        if constexpr (requires { tab.host; }) tab.host = host;
        cs = host;
    } else {
        take = std::min(take, cap);
    }
    tab.n = 0;
    *groups = 0;
    for (; it != end && tab.n < take; ++it) {
        const E* e = entry(*it);
        if (!e) continue;
        E& c = cs[tab.n++];
        c = *e;
        c.first_group = *groups;
        *groups += groups_of(c);
    }
    while (it != end && !entry(*it)) ++it;  // (they never start a launch of their own)
    if (*groups > 0xFFFFFFFFull) return set_error(VXG_ERR_INVALID_ARGUMENT, "array too long for one launch");
    return VXG_OK;
}

// ---- the packed-domain kernels' table (CmpTable: compare, the Dict lookup, filter_batch) ----
// One chunk of such a launch: the kernel it takes (T, epilogue, compared type) and its entry.
struct CmpJob {
    int T;
    Epi epi;
    int ck;
    CmpChunk d;
    bool excl;  // no other producer writes a bitmap word the chunk touches (CmpChunk::bpw_excl)
};

// Fill `tab` with the chunks [it, end) (at most kCmpArgChunks) of one launch: blocks per workgroup,
// every first_group, the launch's workgroups and its LDS bytes.
inline void pack_cmp_table(const CmpJob* const* it, const CmpJob* const* end, CmpTable& tab, uint64_t* groups,
                           uint32_t* lds) {
    uint64_t blocks = 0;
    for (const CmpJob* const* k = it; k != end; ++k) blocks += (*k)->d.n_blocks();
    // small launches take fewer blocks per workgroup (>= 4: one per wave), like K1w's rule
    uint32_t pick = uint32_t(std::min<uint64_t>(32, blocks / 1024)) & ~3u;
    if (pick < 4) pick = 4;
    tab.n = 0;
    *groups = 0;
    *lds = 0;
    for (; it != end; ++it) {
        CmpChunk& c = tab.c[tab.n++];
        c = (*it)->d;
        const uint32_t bpw = std::min(cmp_bpw_max(c.W), pick);
        c.bpw_excl = uint8_t(bpw | ((*it)->excl ? 0x80u : 0u));
        c.first_group = uint32_t(*groups);
        *groups += (c.n_blocks() + bpw - 1) / bpw;
        *lds = std::max(*lds, bpw * 128u * c.W);
    }
    if (*groups == 0) *groups = 1;  // an empty array: one workgroup that finds no block
    *lds += 128;                    // one word row of slack: a value's second word is read unconditionally
}

// Sort `jobs` by kernel and call launch(first job, table, groups, lds, chunks) for every run of at
// most kCmpArgChunks jobs of one kernel: the table is the kernel argument -- nothing is uploaded
// and no host state outlives the call.
template <class Launch>
vxg_status for_each_cmp_launch(std::vector<const CmpJob*> jobs, Launch launch) {
    auto key = [](const CmpJob* j) { return std::make_tuple(j->T, int(j->epi), j->ck); };
    std::stable_sort(jobs.begin(), jobs.end(), [&](const CmpJob* x, const CmpJob* y) { return key(x) < key(y); });
    for (size_t i = 0, j; i < jobs.size(); i = j) {
        for (j = i; j < jobs.size() && j - i < size_t(kCmpArgChunks) && key(jobs[j]) == key(jobs[i]);) j++;
        CmpTable tab{};
        uint64_t groups;
        uint32_t lds;
        pack_cmp_table(jobs.data() + i, jobs.data() + j, tab, &groups, &lds);
        const vxg_status st = launch(*jobs[i], tab, groups, lds, uint32_t(j - i));
        if (st != VXG_OK) return st;
    }
    return VXG_OK;
}

}  // namespace vxg
