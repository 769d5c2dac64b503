// chunk_pack.hpp — the one place that fills a launch's chunk table (vxg_internal.hpp: ChunkTable,
// RunEndTable, VarBinTable).
//
// The rule: up to the table's capacity the entries travel in the kernel argument (tab.c); while a
// plan is recorded (dt set) a longer list becomes ONE device table of any length (tab.ext, built
// in a host mirror that DevTables uploads when the plan is finalised).  Outside a plan a longer
// list is split: each call takes the next launch's share.
#pragma once

#include <algorithm>
#include <type_traits>

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

}  // namespace vxg
