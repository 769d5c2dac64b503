// env.hpp — the one reader of the engine's VXG_* environment knobs (INTEGRATION.md lists them).
// A reader parses the variable each time it is called; a knob that is read once per process
// keeps the result in a function-local static at its call site.
#pragma once

#include <cstdint>
#include <cstdlib>

namespace vxg {

// The variable's text, or null when it is unset (knobs with a parse of their own, diagnostics
// that only ask whether the variable is there).
inline const char* env_str(const char* name) { return std::getenv(name); }

// An on/off knob: `dflt` when unset, off when the text starts with '0', on otherwise.
inline bool env_flag(const char* name, bool dflt) {
    const char* e = env_str(name);
    return e ? e[0] != '0' : dflt;
}

// An unsigned decimal: `dflt` when unset.
inline uint64_t env_u64(const char* name, uint64_t dflt) {
    const char* e = env_str(name);
    return e ? uint64_t(std::strtoull(e, nullptr, 10)) : dflt;
}

// A decimal integer within [lo, hi]: `dflt` when unset or out of range.
inline long long env_int(const char* name, long long lo, long long hi, long long dflt) {
    const char* e = env_str(name);
    if (!e) return dflt;
    const long long v = std::strtoll(e, nullptr, 10);
    return v >= lo && v <= hi ? v : dflt;
}

}  // namespace vxg
