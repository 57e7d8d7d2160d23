// The appearance list's addressing, defined once.
//
// A march kernel appends its appearance samples to kLists sub-lists (one per XCD run). Sub-list l owns the slots
// [l * list_cap, l * list_cap + live_l) of every per-entry array (app_pos, app_ray, app_rgb, ...), live_l = min(counters[l * kCounterStride],
// list_cap): a counter may run past the capacity (a budgeted launch that overflowed), the slots never do. The consumers take the entries as
// ROWS, handed out in tiles of 32, sub-list by sub-list: sub-list l has ceil(live_l / 32) tiles, its first one is tile t[l] of the launch
// (TilePrefix: the exclusive prefix sum, t[kLists] the total), row r = 32 * tile + j is slot j' = r - 32 * t[l] of that sub-list and is
// live when j' < live_l; the rows behind a sub-list's last entry, up to the tile's end, are padding.
//
// Three forms of the same arithmetic: plain functions for the host and for a thread that handles one row (a TilePrefix in memory), the
// wave-resident form for kernels whose waves walk tiles (counts and prefix in lanes 0 .. nlists - 1, nothing in memory), and the
// read-lane variant of the latter for k_mlp_ss3. Nothing here calls into the HIP runtime: a host program can include this file alone and
// run the first form on the CPU (tests/test_list_tiles_cpu.py).
#pragma once
#include <hip/hip_runtime.h>   // (the wave intrinsics' declarations)

namespace t2n {

constexpr int kLists = 8;            // appearance sub-lists per sub-launch
constexpr int kCounterStride = 64;   // unsigned words between sub-list counters: one 256-B line each (same-line atomics serialise)

struct TilePrefix { unsigned t[kLists + 1]; };   // tiles before each sub-list; t[kLists] = all tiles

// ---- host and device: a counter block and a TilePrefix in memory ------------------------------------------------------------------------
// live entries of sub-list l, from a counter block as the march kernels leave it
__host__ __device__ inline unsigned list_live(const unsigned* raw, int l, unsigned list_cap) {
    const unsigned n = raw[l * kCounterStride];
    return n < list_cap ? n : list_cap;
}
// counter block -> *tp (may be NULL); returns the tile total
__host__ __device__ inline unsigned tile_prefix(const unsigned* raw, unsigned list_cap, TilePrefix* tp) {
    unsigned t = 0;
    for (int l = 0; l < kLists; ++l) {
        if (tp) tp->t[l] = t;
        t += (list_live(raw, l, list_cap) + 31u) / 32u;
    }
    if (tp) tp->t[kLists] = t;
    return t;
}
// row -> slot idx of its entry; false for a padding row. tp is read THROUGH the reference (one load at a computed address): a caller that
// picks between two prefixes binds a reference to one of them and never copies it — a private copy becomes a dynamically indexed
// register array (k_app_bin<1>: 33 us instead of 12). Where one of the two is a by-value kernel argument, two calls, one per prefix, keep
// its reads scalar loads (k_head_in, k_dense3_sigmoid).
__host__ __device__ inline bool row_to_entry(long long row, const TilePrefix& tp, const unsigned* counters, unsigned list_cap, unsigned& idx) {
    const unsigned tile = (unsigned)(row >> 5);
    int l = 0;
#pragma unroll
    for (int q = 1; q < kLists; ++q) l += (tp.t[q] <= tile) ? 1 : 0;
    const unsigned slot = (unsigned)(row - (long long)tp.t[l] * 32);
    const unsigned live = list_live(counters, l, list_cap);
    idx = (unsigned)l * list_cap + slot;
    return slot < live;
}
// and back (slot: of a live entry)
__host__ __device__ inline unsigned slot_to_row(unsigned slot, unsigned list_cap, const TilePrefix& tp) {
    const unsigned l = slot / list_cap;
    return tp.t[l] * 32u + (slot - l * list_cap);
}

// ---- wave-resident: every lane of a wave calls these together ---------------------------------------------------------------------------
// Leaves in lane l < nlists the live count of sub-list l (cnt) and the INCLUSIVE tile prefix (incl); returns the tile total in every lane.
// OR_MAX (the one-kernel shade paths): counters may be NULL, every sub-list then holds count_max entries, unclipped.
template <bool OR_MAX = false>
__device__ __forceinline__ unsigned list_tiles(const unsigned* counters, unsigned list_cap, int nlists, int lane, unsigned& cnt, unsigned& incl,
                                               unsigned count_max = 0u) {
    unsigned c = 0u;
    if (lane < nlists) c = (!OR_MAX || counters) ? list_live(counters, lane, list_cap) : count_max;
    unsigned in = (c + 31u) / 32u;
#pragma unroll
    for (int o = 1; o < kLists; o <<= 1) {
        const unsigned t = __shfl_up(in, o);
        if (lane >= o) in += t;
    }
    cnt = c;
    incl = in;
    return __shfl(in, nlists - 1);
}
// wave-uniform tile (below the total) -> first slot of the tile and one past the last live slot of its sub-list
// SBASE: base comes back in a scalar register. The kernels that want it there get it HERE, in front of count: taken at the call site,
// behind count, the compiler regroups their `count - base` from one scalar and one vector operation into two vector ones.
template <bool SBASE = false>
__device__ __forceinline__ void list_locate(unsigned tile, unsigned cnt, unsigned incl, unsigned list_cap, int nlists, int lane, unsigned& base,
                                            unsigned& count) {
    const int li = (int)__popcll(__ballot((lane < nlists) & (incl <= tile)));
    const unsigned before = li ? __shfl(incl, li - 1) : 0u;
    const unsigned lbase = (unsigned)li * list_cap;
    base = lbase + (tile - before) * 32u;
    if (SBASE) base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
    count = lbase + __shfl(cnt, li);
}
// The same for k_mlp_ss3, which has no scalar registers to spare: the tile index is a scalar, the table stays in lanes 0 .. 7 of cnt and
// incl_m and is read with v_readlane (one compare, two read-lanes, scalar results) instead of __shfl's per-lane permutes. incl_m = incl
// with the lanes from nlists on set to 0xffffffff, so that the ballot needs no lane test.
__device__ __forceinline__ void list_locate_readlane(unsigned tile, unsigned cnt, unsigned incl_m, unsigned list_cap, unsigned& base,
                                                     unsigned& count) {
    const int li = (int)__popcll(__ballot(incl_m <= tile));   // (tile < the last prefix sum: li <= kLists - 1)
    const unsigned before = li ? (unsigned)__builtin_amdgcn_readlane((int)incl_m, li - 1) : 0u;
    const unsigned lbase = (unsigned)li * list_cap;
    base = lbase + (tile - before) * 32u;
    count = lbase + (unsigned)__builtin_amdgcn_readlane((int)cnt, li);
}
}  // namespace t2n
