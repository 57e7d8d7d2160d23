// Connected components of a dense fp32 volume [n0][n1][n2] (last index fastest: the layout t2n_alpha_volume writes) on the device, in the
// place of scipy.ndimage.label on a host copy: block-based union-find, all integer, the labels a function of the volume alone.
// A voxel is foreground iff volume > level (strict: NaN is background); connectivity 6 / 18 / 26 = neighbours that differ in at most
// 1 / 2 / 3 coordinates, each by one. Six launches on one stream label a volume (t2n_volume_components):
//   k_vol_local    a workgroup owns a tile of kVolT0 x kVolT1 x kVolT2 = 4 x 8 x 64 voxels: 32 rows of 64 along n2, a row = one wave-wide
//                  load of 256 contiguous bytes. Per row one __ballot gives the foreground mask, and bit arithmetic on it gives every
//                  voxel the first voxel of its run: the runs along n2 cost no union. Runs of neighbouring rows (the row before in the
//                  slice, and the three rows of the slice before; which of them, and whether a run reaches one voxel sideways, depends
//                  on the connectivity) are united in an LDS parent array: for a pair of touching runs exactly ONE lane unites, the
//                  first voxel of the row's run that touches the other run (vol_row_links). Links go larger root under smaller
//                  (atomicMin), so a tile's roots are the smallest voxels of its pieces. Flatten, and write every voxel's parent as
//                  the GLOBAL linear index of its tile-local root, -1 on background, into `labels` (which serves as the parent array).
//   k_vol_border   one thread per foreground voxel on a tile face unites it with its foreground neighbours in OTHER tiles (a diagonal
//                  neighbour may sit in a tile that shares only an edge or a corner), each unordered pair once, from its larger end:
//                  cc_find / cc_unite of t2n_cc.h on the global parents. Tile order inside a tile = linear order, so parent[x] <= x
//                  holds from the start and only ever decreases: a component's final root is its smallest voxel whatever order the
//                  threads ran in.
//   k_vol_flatten  root of every voxel into the workspace (a separate launch: the kernel boundary is the fence), per-256 sums of the root
//                  flags; k_vol_scan: their exclusive scan by one workgroup with a running carry, the total = K; k_vol_rank: the rank of
//                  every root into its own labels slot; k_vol_label: every other foreground voxel reads its root's slot.
// Labels are therefore dense, 0 .. K-1, in the order of each component's smallest linear index, and -1 on background.
// Behind it: t2n_volume_component_stats (voxel counts and index boxes: integer atomics, equal labels combined inside a wave first) and
// t2n_volume_filter (out = keep[label] ? volume : fill on foreground). No float atomics, no host read.
#include "t2n_internal.h"
#include "t2n_cc.h"

#include <limits.h>
#include <math.h>

namespace t2n {

constexpr int kVolT0 = 4, kVolT1 = 8, kVolT2 = 64;      // the local stage's tile; kVolT2 = one wave
constexpr int kVolRows = kVolT0 * kVolT1;               // rows of a tile
constexpr int kVolTile = kVolRows * kVolT2;             // voxels of a tile
constexpr int kVolThreads = 256;
constexpr int kVolRowsPerWave = kVolRows / (kVolThreads / kWave);
static_assert(kVolT2 == kWave, "a row of a tile is one wave-wide access");
static_assert(kVolRows % (kVolThreads / kWave) == 0, "every wave owns the same number of rows");
static_assert((kVolT1 & (kVolT1 - 1)) == 0, "rows are split by shifts");
constexpr int kVolT1Log = 3;
static_assert((1 << kVolT1Log) == kVolT1, "kVolT1Log");

typedef unsigned long long vol_mask;

struct VolDims { int n0, n1, n2, n; int b1, b2; };      // b1, b2: tiles along n1 and n2

// union-find inside a tile: cc_find / cc_unite of t2n_cc.h over an LDS parent array, its loads at workgroup scope
constexpr int kVolLds = __HIP_MEMORY_SCOPE_WORKGROUP;

// bit j of m, 0 outside 0 .. 63
__device__ __forceinline__ bool vol_bit(vol_mask m, int j) { return (unsigned)j < 64u && ((m >> j) & 1ull); }
// first voxel of the run of m that holds the set bit j
__device__ __forceinline__ int vol_run_start(vol_mask m, int j) {
    const vol_mask below = ~m & ((1ull << j) - 1ull);
    return below ? 64 - __clzll((long long)below) : 0;
}

// Unite the runs of this row (mask `mine`, this lane's voxel k in a run that starts at `start`, `fg`: k is foreground) with the runs
// of the row `other` (mask `theirs`) that they touch; reach = 0: voxel k touches voxel k only, reach = 1: k-1, k, k+1. Runs [s,e] and
// [s',e'] touch iff s' <= e + reach and e' >= s - reach; the ONE lane that unites them is k* = max(s, s' - reach), the first voxel of
// [s,e] that touches [s',e']:
//   s' - reach > s   lane k* sees the other run begin at the far end of its reach: bit k + reach set, bit k + reach - 1 clear
//   otherwise        lane s: the other run holds s - reach or, where that bit is clear and reach = 1, begins at s (a run that begins
//                    at s + 1 is the first case)
__device__ __forceinline__ void vol_row_links(int* par, int row, int other, vol_mask theirs, int k, int start, bool fg, int reach) {
    if (!fg || !theirs) return;
    const int a = row * kVolT2 + start, b = other * kVolT2;
    if (reach == 0) {
        if (vol_bit(theirs, k) && (k == start || !vol_bit(theirs, k - 1))) cc_unite<kVolLds>(par, a, b + vol_run_start(theirs, k));
        return;
    }
    if (vol_bit(theirs, k + 1) && !vol_bit(theirs, k)) cc_unite<kVolLds>(par, a, b + k + 1);
    if (k == start) {
        if (vol_bit(theirs, k - 1)) cc_unite<kVolLds>(par, a, b + vol_run_start(theirs, k - 1));
        else if (vol_bit(theirs, k)) cc_unite<kVolLds>(par, a, b + k);
    }
}

// reach of a neighbour row that differs in `nz` (1 or 2) of the two slow coordinates, -1 = not a neighbour at this connectivity
__device__ __forceinline__ int vol_reach(int conn, int nz) {
    if (nz == 1) return conn == 6 ? 0 : 1;
    return conn == 6 ? -1 : conn == 18 ? 0 : 1;
}

__global__ __launch_bounds__(kVolThreads) void k_vol_local(const float* __restrict__ volume, VolDims d, float level, int conn,
                                                           int* __restrict__ parent_out) {
    __shared__ int par[kVolTile];
    __shared__ vol_mask rowmask[kVolRows];
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    int tb = blockIdx.x;
    const int o2 = (tb % d.b2) * kVolT2;
    tb /= d.b2;
    const int o1 = (tb % d.b1) * kVolT1, o0 = (tb / d.b1) * kVolT0;
    const int i2 = o2 + lane;

    // classify, runs along n2
#pragma unroll
    for (int q = 0; q < kVolRowsPerWave; ++q) {
        const int r = w * kVolRowsPerWave + q;
        const int i0 = o0 + (r >> kVolT1Log), i1 = o1 + (r & (kVolT1 - 1));
        const bool in = i0 < d.n0 && i1 < d.n1 && i2 < d.n2;
        const float v = in ? volume[((size_t)i0 * d.n1 + i1) * d.n2 + i2] : 0.0f;
        const bool fg = in && v > level;
        const vol_mask m = __ballot(fg);
        par[r * kVolT2 + lane] = fg ? r * kVolT2 + vol_run_start(m, lane) : -1;
        if (lane == 0) rowmask[r] = m;
    }
    __syncthreads();

    // unite the runs of every row with those of the rows before it that it touches
    const int r1 = vol_reach(conn, 1), r2 = vol_reach(conn, 2);
    for (int q = 0; q < kVolRowsPerWave; ++q) {
        const int r = w * kVolRowsPerWave + q;
        const vol_mask mine = rowmask[r];
        if (!mine) continue;
        const bool fg = (mine >> lane) & 1ull;
        const int start = vol_run_start(mine, lane);
        const int l0 = r >> kVolT1Log, l1 = r & (kVolT1 - 1);
        if (l1 > 0) vol_row_links(par, r, r - 1, rowmask[r - 1], lane, start, fg, r1);
        if (l0 > 0) {
            vol_row_links(par, r, r - kVolT1, rowmask[r - kVolT1], lane, start, fg, r1);
            if (r2 >= 0 && l1 > 0) vol_row_links(par, r, r - kVolT1 - 1, rowmask[r - kVolT1 - 1], lane, start, fg, r2);
            if (r2 >= 0 && l1 < kVolT1 - 1) vol_row_links(par, r, r - kVolT1 + 1, rowmask[r - kVolT1 + 1], lane, start, fg, r2);
        }
    }
    __syncthreads();

    // flatten; the parent of a voxel = the global linear index of its root in this tile
#pragma unroll
    for (int q = 0; q < kVolRowsPerWave; ++q) {
        const int r = w * kVolRowsPerWave + q;
        const int i0 = o0 + (r >> kVolT1Log), i1 = o1 + (r & (kVolT1 - 1));
        if (i0 >= d.n0 || i1 >= d.n1 || i2 >= d.n2) continue;
        int x = par[r * kVolT2 + lane];
        if (x >= 0) {
            int p = cc_load<kVolLds>(par + x);
            while (p != x) { x = p; p = cc_load<kVolLds>(par + x); }
            const int rr = x >> 6;
            x = ((o0 + (rr >> kVolT1Log)) * d.n1 + o1 + (rr & (kVolT1 - 1))) * d.n2 + o2 + (x & (kVolT2 - 1));
        }
        parent_out[((size_t)i0 * d.n1 + i1) * d.n2 + i2] = x;
    }
}

// this thread's voxel, or n for the threads beyond
__device__ __forceinline__ int vol_item(int n) {
    const long long t = (long long)blockIdx.x * kCcRun + threadIdx.x;
    return t < n ? (int)t : n;
}

// One thread per voxel; the foreground voxels on a tile face go on. Of the 26 offsets the 13 that lead to a SMALLER linear index are
// walked (the pair is then united once, from its larger end), those the connectivity admits, those that leave the tile.
__global__ __launch_bounds__(kCcRun) void k_vol_border(VolDims d, int conn, int* parent) {
    const int v = vol_item(d.n);
    if (v >= d.n || parent[v] < 0) return;              // -1 is final: background is never written again
    const int i2 = v % d.n2, t = v / d.n2;
    const int i1 = t % d.n1, i0 = t / d.n1;
    const int l0 = i0 % kVolT0, l1 = i1 % kVolT1, l2 = i2 % kVolT2;
    if (l0 != 0 && l1 != 0 && l1 != kVolT1 - 1 && l2 != 0 && l2 != kVolT2 - 1) return;
    const int most = conn == 6 ? 1 : conn == 18 ? 2 : 3;
#pragma unroll
    for (int c = 0; c < 13; ++c) {
        const int e0 = c < 9 ? -1 : 0;
        const int e1 = c < 9 ? c / 3 - 1 : c < 12 ? -1 : 0;
        const int e2 = c < 12 ? c % 3 - 1 : -1;
        if ((e0 != 0) + (e1 != 0) + (e2 != 0) > most) continue;
        const bool leaves = (e0 < 0 && l0 == 0) || (e1 < 0 && l1 == 0) || (e1 > 0 && l1 == kVolT1 - 1) || (e2 < 0 && l2 == 0) ||
                            (e2 > 0 && l2 == kVolT2 - 1);
        const int j0 = i0 + e0, j1 = i1 + e1, j2 = i2 + e2;
        if (!leaves || j0 < 0 || j1 < 0 || j1 >= d.n1 || j2 < 0 || j2 >= d.n2) continue;
        const int u = (j0 * d.n1 + j1) * d.n2 + j2;
        if (cc_load(parent + u) >= 0) cc_unite(parent, v, u);
    }
}

// k_cc_flatten with a background: root -1, no flag
__global__ __launch_bounds__(kCcRun) void k_vol_flatten(const int* __restrict__ parent, int n, int* __restrict__ root, int* __restrict__ bsum) {
    __shared__ int wsum[kCcRun / kWave];
    const int v = vol_item(n);
    int flag = 0;
    if (v < n) {
        int x = v, p = parent[v];
        if (p < 0) x = -1;
        else while (p != x) { x = p; p = parent[x]; }
        root[v] = x;
        flag = x == v;
    }
    int all;
    block_scan_excl<kCcRun>(flag, wsum, all);
    if (threadIdx.x == 0) bsum[blockIdx.x] = all;
}

// exclusive scan in place of a[0..nb) by one workgroup with a running carry (k_cc_scan's steps); the total to total[0]
__global__ __launch_bounds__(kMcScanChunk) void k_vol_scan(int* __restrict__ a, int nb, long long* __restrict__ total) {
    __shared__ int wsum[kMcScanChunk / kWave];
    long long carry = 0;
    for (int base = 0; base < nb; base += kMcScanChunk) {
        const int i = base + (int)threadIdx.x;
        const int own = i < nb ? a[i] : 0;
        int all;
        const int ex = block_scan_excl<kMcScanChunk>(own, wsum, all);
        if (i < nb) a[i] = (int)(carry + ex);
        carry += all;
    }
    if (threadIdx.x == 0) total[0] = carry;
}

// the rank of every root, into the root's own slot of labels
__global__ __launch_bounds__(kCcRun) void k_vol_rank(const int* __restrict__ root, int n, const int* __restrict__ bsum, int* __restrict__ labels) {
    __shared__ int wsum[kCcRun / kWave];
    const int v = vol_item(n);
    const int flag = v < n && root[v] == v;
    int all;
    const int r = bsum[blockIdx.x] + block_scan_excl<kCcRun>(flag, wsum, all);
    if (flag) labels[v] = r;
}

// every other foreground voxel reads its root's slot (roots' slots are not written here, the others' are not read)
__global__ __launch_bounds__(kCcRun) void k_vol_label(const int* __restrict__ root, int n, int* labels) {
    const int v = vol_item(n);
    if (v >= n) return;
    const int x = root[v];
    if (x >= 0 && x != v) labels[v] = labels[x];
}

__global__ __launch_bounds__(kCcRun) void k_vol_box_init(int* __restrict__ boxes, int K) {
    const int c = vol_item(K);
    if (c >= K) return;
#pragma unroll
    for (int a = 0; a < 3; ++a) { boxes[(size_t)c * 6 + a] = INT_MAX; boxes[(size_t)c * 6 + 3 + a] = -1; }
}

// box[a] = min(box[a], lo[a]), box[3 + a] = max(box[3 + a], hi[a]). A box only ever grows, so a value that does not grow the box as a
// relaxed load shows it cannot grow the box as it is now: the atomic is skipped. All but the first few voxels of a component end here.
__device__ __forceinline__ void vol_box_grow(int* b, int lo0, int lo1, int lo2, int hi0, int hi1, int hi2) {
    if (lo0 < cc_load(b + 0)) atomicMin(b + 0, lo0);
    if (lo1 < cc_load(b + 1)) atomicMin(b + 1, lo1);
    if (lo2 < cc_load(b + 2)) atomicMin(b + 2, lo2);
    if (hi0 > cc_load(b + 3)) atomicMax(b + 3, hi0);
    if (hi1 > cc_load(b + 4)) atomicMax(b + 4, hi1);
    if (hi2 > cc_load(b + 5)) atomicMax(b + 5, hi2);
}

constexpr int kVolStatSteps = 16;      // a wave of k_vol_stats walks 16 x 64 consecutive voxels

// counts[label] += voxels and, where boxes are asked for, the index box of every label: integer atomics, equal labels combined inside a
// wave first (the ballot loop of the mesh stage's cc_count), and across the wave's steps for ONE label at a time: the count of a label that holds eight lanes and
// more of a step is carried in registers until another such label takes its place, so a component that fills the volume costs an add
// per 1024 voxels, not one per 64 on one word. A wave step that lies inside one row holds its voxels in i2 order with i0, i1 fixed:
// per distinct label the first and the last of its lanes carry the box. A step that spans rows (n2 < 64, or a row's end) lets every
// lane grow the box by its own voxel.
__global__ __launch_bounds__(kCcRun) void k_vol_stats(const int* __restrict__ labels, VolDims d, int K, int* __restrict__ counts,
                                                      int* boxes) {
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const long long first = ((long long)blockIdx.x * (kCcRun / kWave) + w) * (kVolStatSteps * kWave);
    int held = -1, held_count = 0;      // wave-uniform
    for (int step = 0; step < kVolStatSteps; ++step) {
        const long long at = first + step * kWave;
        if (at >= d.n) break;
        const long long v = at + lane;
        int l = -1;
        if (v < d.n) l = labels[v];
        const bool ok = (unsigned)l < (unsigned)K;
        const int vv = (int)(v < d.n ? v : d.n - 1);
        const int i2 = vv % d.n2, t = vv / d.n2;
        const int i1 = t % d.n1, i0 = t / d.n1;
        const bool one_row = __shfl(t, 0, kWave) == __shfl(t, kWave - 1, kWave);
        vol_mask todo = __ballot(ok);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int ll = __shfl(l, leader, kWave);
            const vol_mask same = __ballot(ok && l == ll);
            const int cnt = __popcll(same);
            if (ll == held) held_count += cnt;
            else if (cnt >= 8) {
                if (lane == 0 && held_count) atomicAdd(counts + held, held_count);
                held = ll;
                held_count = cnt;
            } else if (lane == leader) atomicAdd(counts + ll, cnt);
            if (boxes && one_row) {
                const int hi2 = __shfl(i2, 63 - __clzll((long long)same), kWave);
                if (lane == leader) vol_box_grow(boxes + (size_t)ll * 6, i0, i1, i2, i0, i1, hi2);
            }
            todo &= ~same;
        }
        if (boxes && !one_row && ok) vol_box_grow(boxes + (size_t)l * 6, i0, i1, i2, i0, i1, i2);
    }
    if (lane == 0 && held_count) atomicAdd(counts + held, held_count);
}

// volume_out may be volume: every thread reads and writes its own voxel only
__global__ __launch_bounds__(kCcRun) void k_vol_filter(const float* volume, const int* __restrict__ labels, int n,
                                                       const uint8_t* __restrict__ keep, int K, float fill, float* volume_out) {
    const int v = vol_item(n);
    if (v >= n) return;
    const int l = labels[v];
    const float x = volume[v];
    volume_out[v] = ((unsigned)l < (unsigned)K && !keep[l]) ? fill : x;
}

static bool vol_shape_ok(int n0, int n1, int n2) {
    return n0 >= 1 && n1 >= 1 && n2 >= 1 && (int64_t)n0 * n1 * n2 < (1ll << 31);
}
static VolDims vol_dims(int n0, int n1, int n2) {
    VolDims d;
    d.n0 = n0; d.n1 = n1; d.n2 = n2; d.n = n0 * n1 * n2;
    d.b1 = (n1 + kVolT1 - 1) / kVolT1;
    d.b2 = (n2 + kVolT2 - 1) / kVolT2;
    return d;
}
// workspace: root [n] int32 | bsum [nb] int32, each region rounded up to 256 bytes
struct VolCarve { size_t root, bsum, total; int nb; };
static VolCarve vol_carve(int64_t n) {
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    VolCarve c;
    c.nb = (int)((n + kCcRun - 1) / kCcRun);
    c.root = 0;
    c.bsum = c.root + up((size_t)n * 4);
    c.total = c.bsum + up((size_t)c.nb * 4);
    return c;
}

}  // namespace t2n

using namespace t2n;

extern "C" size_t t2n_volume_components_workspace_bytes(int n0, int n1, int n2) {
    if (!vol_shape_ok(n0, n1, n2)) return 0;
    return vol_carve((int64_t)n0 * n1 * n2).total;
}

extern "C" int t2n_volume_components_tile(int tile3[3]) {
    if (!tile3) {
        set_error("t2n_volume_components_tile: NULL pointer");
        return T2N_ERR_INVALID;
    }
    tile3[0] = kVolT0; tile3[1] = kVolT1; tile3[2] = kVolT2;
    return T2N_OK;
}

extern "C" int t2n_volume_components(const float* volume, int n0, int n1, int n2, float level, int connectivity, int32_t* labels,
                                     int64_t* n_components_out, void* workspace, size_t workspace_bytes, t2n_stream stream) {
    if (!volume || !labels || !n_components_out || !workspace || !vol_shape_ok(n0, n1, n2) ||
        (connectivity != 6 && connectivity != 18 && connectivity != 26) || !isfinite(level) ||
        workspace_bytes < vol_carve((int64_t)n0 * n1 * n2).total) {
        set_error("t2n_volume_components: bad argument (NULL pointer, a dimension < 1, 2^31 voxels and more, a connectivity other than 6, "
                  "18 or 26, a level that is not finite, or a workspace smaller than t2n_volume_components_workspace_bytes)");
        return T2N_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const VolDims d = vol_dims(n0, n1, n2);
    const VolCarve c = vol_carve(d.n);
    char* ws = (char*)workspace;
    int* root = (int*)(ws + c.root);
    int* bsum = (int*)(ws + c.bsum);
    const int64_t tiles = (int64_t)((n0 + kVolT0 - 1) / kVolT0) * d.b1 * d.b2;      // <= n < 2^31
    const dim3 gv((unsigned)c.nb), nt(kCcRun);
    hipLaunchKernelGGL(k_vol_local, dim3((unsigned)tiles), dim3(kVolThreads), 0, s, volume, d, level, connectivity, labels);
    hipLaunchKernelGGL(k_vol_border, gv, nt, 0, s, d, connectivity, labels);
    hipLaunchKernelGGL(k_vol_flatten, gv, nt, 0, s, (const int*)labels, d.n, root, bsum);
    hipLaunchKernelGGL(k_vol_scan, dim3(1), dim3(kMcScanChunk), 0, s, bsum, c.nb, (long long*)n_components_out);
    hipLaunchKernelGGL(k_vol_rank, gv, nt, 0, s, (const int*)root, d.n, (const int*)bsum, labels);
    hipLaunchKernelGGL(k_vol_label, gv, nt, 0, s, (const int*)root, d.n, labels);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" int t2n_volume_component_stats(const int32_t* labels, int n0, int n1, int n2, int64_t n_components, int32_t* voxel_counts,
                                          int32_t* boxes_or_null, t2n_stream stream) {
    if (!labels || !vol_shape_ok(n0, n1, n2) || n_components < 0 || n_components > (int64_t)n0 * n1 * n2 ||
        (n_components > 0 && !voxel_counts)) {
        set_error("t2n_volume_component_stats: bad argument (NULL pointer, a dimension < 1, 2^31 voxels and more, or a component count "
                  "outside [0, n0 * n1 * n2])");
        return T2N_ERR_INVALID;
    }
    if (n_components == 0) return T2N_OK;
    hipStream_t s = (hipStream_t)stream;
    const VolDims d = vol_dims(n0, n1, n2);
    const int K = (int)n_components;
    T2N_HIP(hipMemsetAsync(voxel_counts, 0, (size_t)K * 4, s));
    if (boxes_or_null) hipLaunchKernelGGL(k_vol_box_init, dim3((unsigned)((K + kCcRun - 1) / kCcRun)), dim3(kCcRun), 0, s, boxes_or_null, K);
    const int64_t per = (int64_t)kCcRun * kVolStatSteps;
    hipLaunchKernelGGL(k_vol_stats, dim3((unsigned)((d.n + per - 1) / per)), dim3(kCcRun), 0, s, labels, d, K, voxel_counts, boxes_or_null);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" int t2n_volume_filter(const float* volume, const int32_t* labels, int n0, int n1, int n2, const uint8_t* keep,
                                 int64_t n_components, float fill, float* volume_out, t2n_stream stream) {
    if (!volume || !labels || !volume_out || !vol_shape_ok(n0, n1, n2) || n_components < 0 || n_components > (int64_t)n0 * n1 * n2 ||
        (n_components > 0 && !keep)) {
        set_error("t2n_volume_filter: bad argument (NULL pointer, a dimension < 1, 2^31 voxels and more, or a component count outside "
                  "[0, n0 * n1 * n2])");
        return T2N_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const int n = n0 * n1 * n2;
    hipLaunchKernelGGL(k_vol_filter, dim3((unsigned)((n + kCcRun - 1) / kCcRun)), dim3(kCcRun), 0, s, volume, labels, n, keep,
                       (int)n_components, fill, volume_out);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}
