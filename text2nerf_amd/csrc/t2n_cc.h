// The device pieces that the two connected-component stages share (t2n_mesh.hip: components of a face list; t2n_volume.hip: components
// of a dense volume): the workgroup scan, the lock-free union-find over a global parent array whose roots are the smallest index of
// each component.
#pragma once
#include "t2n_internal.h"

namespace t2n {

constexpr int kMcScanChunk = 1024;   // workgroup sums per step of the one-workgroup scans (k_mc_scan, k_cc_scan, k_vol_scan)
constexpr int kCcRun = 256;          // elements per workgroup of the per-element component kernels

// exclusive prefix of v over the workgroup (NT threads, every one of them calls); total = the workgroup's sum. wsum: NT / 64 words of LDS
template <int NT>
__device__ __forceinline__ int block_scan_excl(int v, int* wsum, int& total) {
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const int up = __shfl_up(inc, o, kWave);
        if (lane >= o) inc += up;
    }
    if (lane == kWave - 1) wsum[w] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int q = 0; q < NT / kWave; ++q) {
        const int s = wsum[q];
        if (q < w) before += s;
        all += s;
    }
    __syncthreads();      // wsum may be reused by the next call
    total = all;
    return before + inc - v;
}

// kScope: agent for a parent array in global memory that many workgroups unite in (the default), workgroup for one in LDS
template <int kScope = __HIP_MEMORY_SCOPE_AGENT>
__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, kScope); }

// Chase the parents from x to a vertex that reads as its own parent. Every value read was stored in parent[] at some time (a relaxed
// load; at agent scope: served by memory, not by this CU's L1), which is all the callers rely on; a stale one costs a retry in cc_unite.
// On the way parent[x] is lowered to its grandparent (atomicMin: it can only decrease, and to a vertex of the same tree).
template <int kScope = __HIP_MEMORY_SCOPE_AGENT>
__device__ __forceinline__ int cc_find(int* parent, int x) {
    int p = cc_load<kScope>(parent + x);
    while (p != x) {
        const int g = cc_load<kScope>(parent + p);
        if (g != p) atomicMin(parent + x, g);
        x = p;
        p = g;
    }
    return x;
}

// Link the larger root under the smaller. Only what atomicMin returns decides: `hi` back = hi was a root and now hangs under lo; anything
// else = hi had a parent `old` already (parent[hi] is now min(old, lo), both of hi's component once this call is through), and the pair
// (old, lo) is still to unite. The pair decreases every round, so this terminates.
template <int kScope = __HIP_MEMORY_SCOPE_AGENT>
__device__ __forceinline__ void cc_unite(int* parent, int a, int b) {
    while (true) {
        a = cc_find<kScope>(parent, a);
        b = cc_find<kScope>(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = atomicMin(parent + hi, lo);
        if (old == hi) return;
        a = old;
        b = lo;
    }
}

}  // namespace t2n
