// filter_impl.hpp — the device helpers the filter kernels share: the wave scans, the one read of a
// mask word (filter_mask_word) and a tile's words with their output bases (tile_words).  Included
// by filter.hip and filter_packed.hip only.
#pragma once

#include "filter.hpp"

namespace vxg {

namespace {

constexpr int kWave = 64;

// Word wi of an n-row LSB mask: 0 past the last word, and the bits at and beyond n cleared in the
// last one -- every read of a mask word goes through here, so a caller's mask may hold anything
// past its length.
__device__ __forceinline__ uint64_t filter_mask_word(const uint64_t* __restrict__ mask, uint64_t n, uint64_t wi) {
    const uint64_t nw = (n + 63) / 64;
    if (wi >= nw) return 0;
    const uint64_t w = mask[wi];
    return (wi + 1 == nw && (n & 63)) ? w & ((1ull << (n & 63)) - 1ull) : w;
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int lane) {
    const uint32_t lo = __builtin_amdgcn_readlane(uint32_t(v), lane);
    const uint32_t hi = __builtin_amdgcn_readlane(uint32_t(v >> 32), lane);
    return (uint64_t(hi) << 32) | lo;
}

__device__ __forceinline__ uint64_t wave_incl_scan(uint64_t v, int lane) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint64_t o = __shfl_up(v, d, kWave);
        if (lane >= d) v += o;
    }
    return v;
}

__device__ __forceinline__ uint64_t wave_or(uint64_t v) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) v |= __shfl_xor(v, d, kWave);
    return v;
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) v += __shfl_xor(v, d, kWave);
    return v;
}

__device__ __forceinline__ uint64_t lanes_below(int lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }

// Per wavefront: the mask word of this lane and the output base of its first selected row.
struct TileWords {
    uint64_t m, base;
};

__device__ __forceinline__ TileWords tile_words(const uint64_t* __restrict__ mask, uint64_t n,
                                                const uint64_t* __restrict__ tile_off, uint64_t t, int lane) {
    TileWords r;
    r.m = filter_mask_word(mask, n, t * 64 + lane);
    const uint64_t c = uint64_t(__popcll(r.m));
    r.base = tile_off[t] + wave_incl_scan(c, lane) - c;
    return r;
}

}  // namespace

}  // namespace vxg
