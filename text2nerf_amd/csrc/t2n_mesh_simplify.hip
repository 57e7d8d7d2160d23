// Mesh export, the stage behind floater removal and smoothing: simplification by vertex clustering on a uniform grid with quadric-optimal
// representatives (Lindstrom's out-of-core simplification). Every stage is keys -> sort -> rows -> one thread per row, as in
// t2n_mesh_smooth.hip, and every output is a function of the input alone: integer keys, float64 sums in a fixed order, no float atomics.
//   clusters   k_sp_vertex_keys writes cell id << 32 | vertex per vertex; the caller sorts; t2n_mesh_cluster_rows flags where the high word
//              changes (k_sp_flags + k_sp_scan + k_sp_rows_fill): clusters are the occupied cells in ascending id, a cluster's members
//              its vertices in ascending index.
//   placement  one thread per cluster walks its member row (the mean) and its face row (the quadric; the cluster -> face CSR comes from
//              k_sp_face_keys, a sort and t2n_mesh_csr with n_rows = K), solves the regularised 3 x 3 system by cofactors and keeps the
//              solution when it lies in the cluster's cell. The sums are sequential by definition (ascending index, one rounding per
//              operation), so a row is one thread's loop: a wave takes as long as its longest row.
//   faces      k_sp_face_map sends every index through vertex_map, marks faces that collapsed, rotates the rest (smallest index first)
//              and writes the two sort keys of the rotated triple; the caller's two stable sorts bring equal triples together in
//              ascending face index; k_sp_face_first keeps the first of every group; flags + scan + k_sp_faces_fill compact the kept
//              faces in their original order.
// Rows are clipped to the array lengths and an index outside its range is skipped: no memory is touched through a bad array.
#include "t2n_internal.h"
#include "t2n_cc.h"      // block_scan_excl, kMcScanChunk, kCcRun

namespace t2n {

constexpr long long kSpNone = 0x7fffffffffffffffll;     // a face key that t2n_mesh_csr drops; a triple key behind every real one
constexpr long long kSpNoCell = 0x7fffffffll;           // the high word of a vertex outside the grid: above every cell id (< 2^31 - 1)

struct SpGrid { double o[3], h[3]; int n[3]; };

// this thread's element of n (n < 2^31), or n for the threads beyond
__device__ __forceinline__ int sp_item(int n) {
    const long long t = (long long)blockIdx.x * kCcRun + threadIdx.x;
    return t < n ? (int)t : n;
}

__device__ __forceinline__ bool sp_finite(double x) { return x - x == 0.0; }

__global__ __launch_bounds__(kCcRun) void k_sp_vertex_keys(const float* __restrict__ verts, int V, SpGrid g, long long* __restrict__ keys) {
    const int v = sp_item(V);
    if (v >= V) return;
    long long c[3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double q = floor(((double)verts[(size_t)v * 3 + k] - g.o[k]) / g.h[k]);
        ok = ok && q >= 0.0 && q < (double)g.n[k];      // false for a NaN
        c[k] = ok ? (long long)q : 0;
    }
    const long long id = ok ? (c[0] * g.n[1] + c[1]) * g.n[2] + c[2] : kSpNoCell;
    keys[v] = id << 32 | (long long)v;
}

// ---- flags -> per-workgroup sums -> scan: the count / scan / emit shape of t2n_mesh_smooth.hip -----------------------------------------
// 1 where a sorted vertex key opens a cluster
struct SpRowFlag {
    const long long* keys; int n, V;
    __device__ bool valid(int i) const { return i < n && keys[i] >= 0 && (keys[i] >> 32) < kSpNoCell && (keys[i] & 0xffffffffll) < V; }
    __device__ int operator()(int i) const { return valid(i) && (i == 0 || (keys[i - 1] >> 32) != (keys[i] >> 32)) ? 1 : 0; }
};
struct SpKeepFlag {
    const uint8_t* keep; int n;
    __device__ int operator()(int i) const { return i < n && keep[i] ? 1 : 0; }
};

template <class Flag>
__global__ __launch_bounds__(kCcRun) void k_sp_flags(Flag flag, int n, int* __restrict__ bsum) {
    __shared__ int wsum[kCcRun / kWave];
    int all;
    block_scan_excl<kCcRun>(flag(sp_item(n)), wsum, all);
    if (threadIdx.x == 0) bsum[blockIdx.x] = all;
}

// exclusive scan of a[0..nb) in place by one workgroup with a running carry (k_mc_scan's steps); the total to total[0]
__global__ __launch_bounds__(kMcScanChunk) void k_sp_scan(int* __restrict__ a, int nb, long long* __restrict__ total) {
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

// sorted position i holds vertex v of cluster `to`: vertex_map[v] = to, members[i] = v; the opener writes offsets[to] and cells[to]; the
// last valid position writes offsets[K] (the valid keys are a prefix: kSpNoCell sorts behind every cell)
__global__ __launch_bounds__(kCcRun) void k_sp_rows_fill(SpRowFlag flag, int n, SpGrid g, const int* __restrict__ bsum, int* __restrict__ vertex_map,
                                                         long long* __restrict__ offsets, int* __restrict__ members, int* __restrict__ cells) {
    __shared__ int wsum[kCcRun / kWave];
    const int i = sp_item(n);
    const int fl = flag(i);
    int all;
    const int before = bsum[blockIdx.x] + block_scan_excl<kCcRun>(fl, wsum, all);
    if (i >= n) return;
    const long long k = flag.keys[i];
    const int v = (int)(k & 0xffffffffll);
    members[i] = v;
    if (!flag.valid(i)) {
        if ((unsigned)v < (unsigned)flag.V) vertex_map[v] = -1;
        if (i == 0) offsets[0] = 0;
        return;
    }
    const int to = before + fl - 1;             // clusters opened up to and including i, minus one: 0 <= to <= i < V
    vertex_map[v] = to;
    if (fl) {
        const long long id = k >> 32;
        offsets[to] = i;
        cells[(size_t)to * 3] = (int)(id / ((long long)g.n[1] * g.n[2]));
        cells[(size_t)to * 3 + 1] = (int)(id / g.n[2] % g.n[1]);
        cells[(size_t)to * 3 + 2] = (int)(id % g.n[2]);
    }
    if (!flag.valid(i + 1)) offsets[to + 1] = (long long)i + 1;
}

// ---- cluster -> face keys ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool sp_face(const int* __restrict__ faces, int t, int V, int f[3]) {
    const int* p = faces + (size_t)t * 3;
    f[0] = p[0]; f[1] = p[1]; f[2] = p[2];
    return (unsigned)f[0] < (unsigned)V && (unsigned)f[1] < (unsigned)V && (unsigned)f[2] < (unsigned)V;
}

// keys [3 F]: face t writes (vertex_map[corner], t) per corner; two corners in one cluster give one key twice, which t2n_mesh_csr keeps once
__global__ __launch_bounds__(kCcRun) void k_sp_face_keys(const int* __restrict__ faces, int F, int V, const int* __restrict__ vertex_map, int K,
                                                         long long* __restrict__ keys) {
    const int t = sp_item(F);
    if (t >= F) return;
    int f[3];
    const bool ok = sp_face(faces, t, V, f);
    long long* o = keys + (size_t)t * 3;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const int c = ok ? vertex_map[f[e]] : -1;
        o[e] = (unsigned)c < (unsigned)K ? ((long long)c << 32 | (long long)t) : kSpNone;
    }
}

// ---- placement ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCcRun) void k_sp_place(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                     const long long* __restrict__ offsets, const int* __restrict__ members, long long M,
                                                     const int* __restrict__ cells, int K, const long long* __restrict__ foffsets,
                                                     const int* __restrict__ frows, long long E, SpGrid g, double reg, int quadric,
                                                     float* __restrict__ out) {
    const int c = sp_item(K);
    if (c >= K) return;
    long long b = offsets[c], e = offsets[c + 1];
    b = b < 0 ? 0 : b;
    e = e > M ? M : e;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    long long cnt = 0;
    for (long long q = b; q < e; ++q) {
        const int v = members[q];
        if ((unsigned)v >= (unsigned)V) continue;
        const float* p = verts + (size_t)v * 3;
        s0 = s0 + (double)p[0];
        s1 = s1 + (double)p[1];
        s2 = s2 + (double)p[2];
        ++cnt;
    }
    float* o = out + (size_t)c * 3;
    if (cnt == 0) { o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f; return; }       // no cluster of t2n_mesh_cluster_rows is empty
    const double d = (double)cnt;
    const double m0 = s0 / d, m1 = s1 / d, m2 = s2 / d;
    o[0] = (float)m0; o[1] = (float)m1; o[2] = (float)m2;
    if (!quadric) return;
    b = foffsets[c]; e = foffsets[c + 1];
    b = b < 0 ? 0 : b;
    e = e > E ? E : e;
    double A00 = 0.0, A01 = 0.0, A02 = 0.0, A11 = 0.0, A12 = 0.0, A22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    for (long long q = b; q < e; ++q) {
        const int t = frows[q];
        int f[3];
        if ((unsigned)t >= (unsigned)F || !sp_face(faces, t, V, f)) continue;
        // the corners rotated so that the smallest vertex index (the first of equal ones) comes first: index rotation does not matter
        const int k = f[1] < f[0] ? (f[2] < f[1] ? 2 : 1) : (f[2] < f[0] ? 2 : 0);
        const float* pa = verts + (size_t)f[k] * 3;
        const float* pb = verts + (size_t)f[(k + 1) % 3] * 3;
        const float* pc = verts + (size_t)f[(k + 2) % 3] * 3;
        const double a0 = pa[0], a1 = pa[1], a2 = pa[2];
        const double u0 = (double)pb[0] - a0, u1 = (double)pb[1] - a1, u2 = (double)pb[2] - a2;
        const double w0 = (double)pc[0] - a0, w1 = (double)pc[1] - a1, w2 = (double)pc[2] - a2;
        const double n0 = u1 * w2 - u2 * w1, n1 = u2 * w0 - u0 * w2, n2 = u0 * w1 - u1 * w0;
        if (!(sp_finite(n0) && sp_finite(n1) && sp_finite(n2)) || (n0 == 0.0 && n1 == 0.0 && n2 == 0.0)) continue;
        const double r = (n0 * (a0 - m0) + n1 * (a1 - m1)) + n2 * (a2 - m2);
        A00 = A00 + n0 * n0; A01 = A01 + n0 * n1; A02 = A02 + n0 * n2;
        A11 = A11 + n1 * n1; A12 = A12 + n1 * n2; A22 = A22 + n2 * n2;
        b0 = b0 + n0 * r; b1 = b1 + n1 * r; b2 = b2 + n2 * r;
    }
    const double t = (A00 + A11) + A22;
    if (!(t > 0.0) || !sp_finite(t)) return;
    const double eps = reg * t;
    const double M00 = A00 + eps, M11 = A11 + eps, M22 = A22 + eps;
    const double C00 = M11 * M22 - A12 * A12;
    const double C01 = A02 * A12 - A01 * M22;
    const double C02 = A01 * A12 - A02 * M11;
    const double C11 = M00 * M22 - A02 * A02;
    const double C12 = A01 * A02 - M00 * A12;
    const double C22 = M00 * M11 - A01 * A01;
    const double det = (M00 * C00 + A01 * C01) + A02 * C02;
    const double p0 = m0 + ((C00 * b0 + C01 * b1) + C02 * b2) / det;
    const double p1 = m1 + ((C01 * b0 + C11 * b1) + C12 * b2) / det;
    const double p2 = m2 + ((C02 * b0 + C12 * b1) + C22 * b2) / det;
    const double p[3] = {p0, p1, p2};
    bool inside = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int ck = cells[(size_t)c * 3 + k];
        const double lo = g.o[k] + (double)ck * g.h[k], hi = g.o[k] + ((double)ck + 1.0) * g.h[k];      // ck + 1 is exact
        inside = inside && p[k] >= lo && p[k] <= hi;        // false for a p that is not finite
    }
    if (inside) { o[0] = (float)p0; o[1] = (float)p1; o[2] = (float)p2; }
}

// per channel (sum of the members + count / 2) / count in integers
__global__ __launch_bounds__(kCcRun) void k_sp_colors(const uint8_t* __restrict__ colors, int V, const long long* __restrict__ offsets,
                                                      const int* __restrict__ members, long long M, int K, uint8_t* __restrict__ out) {
    const int c = sp_item(K);
    if (c >= K) return;
    long long b = offsets[c], e = offsets[c + 1];
    b = b < 0 ? 0 : b;
    e = e > M ? M : e;
    unsigned long long s0 = 0, s1 = 0, s2 = 0, cnt = 0;
    for (long long q = b; q < e; ++q) {
        const int v = members[q];
        if ((unsigned)v >= (unsigned)V) continue;
        const uint8_t* p = colors + (size_t)v * 3;
        s0 += p[0]; s1 += p[1]; s2 += p[2];
        ++cnt;
    }
    uint8_t* o = out + (size_t)c * 3;
    if (cnt == 0) { o[0] = 0; o[1] = 0; o[2] = 0; return; }
    o[0] = (uint8_t)((s0 + cnt / 2) / cnt);
    o[1] = (uint8_t)((s1 + cnt / 2) / cnt);
    o[2] = (uint8_t)((s2 + cnt / 2) / cnt);
}

// ---- faces ------------------------------------------------------------------------------------------------------------------------------------------
// rot [F][3]: the mapped triple, smallest index first in its cyclic order, or (-1, -1, -1) for a face that collapsed (two corners in one
// cluster) or holds a bad index; key_hi = the first index (K for a dropped face: behind every real one), key_lo = second << 32 | third
__global__ __launch_bounds__(kCcRun) void k_sp_face_map(const int* __restrict__ faces, int F, int V, const int* __restrict__ vertex_map, int K,
                                                        int* __restrict__ rot, long long* __restrict__ key_hi, long long* __restrict__ key_lo) {
    const int t = sp_item(F);
    if (t >= F) return;
    int f[3];
    bool ok = sp_face(faces, t, V, f);
    int m[3] = {-1, -1, -1};
    if (ok) {
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            m[e] = vertex_map[f[e]];
            ok = ok && (unsigned)m[e] < (unsigned)K;
        }
    }
    ok = ok && m[0] != m[1] && m[1] != m[2] && m[2] != m[0];
    const int k = m[1] < m[0] ? (m[2] < m[1] ? 2 : 1) : (m[2] < m[0] ? 2 : 0);
    const int a = ok ? m[k] : -1, b = ok ? m[(k + 1) % 3] : -1, c = ok ? m[(k + 2) % 3] : -1;
    rot[(size_t)t * 3] = a; rot[(size_t)t * 3 + 1] = b; rot[(size_t)t * 3 + 2] = c;
    key_hi[t] = ok ? (long long)a : (long long)K;
    key_lo[t] = ok ? ((long long)b << 32 | (long long)c) : kSpNone;
}

// order [F]: the faces sorted by rotated triple, equal triples in ascending face index. keep[f] = 1 for the first face of every group of
// live faces (keep is zero beforehand; an entry of `order` outside [0, F) is skipped)
__global__ __launch_bounds__(kCcRun) void k_sp_face_first(const int* __restrict__ rot, const long long* __restrict__ order, int F,
                                                          uint8_t* __restrict__ keep) {
    const int i = sp_item(F);
    if (i >= F) return;
    const long long f = order[i];
    if (f < 0 || f >= F) return;
    const int* r = rot + (size_t)f * 3;
    if (r[0] < 0) return;
    bool first = true;
    if (i > 0) {
        const long long g = order[i - 1];
        if (g >= 0 && g < F) {
            const int* s = rot + (size_t)g * 3;
            first = s[0] != r[0] || s[1] != r[1] || s[2] != r[2];
        }
    }
    if (first) keep[f] = 1;
}

__global__ __launch_bounds__(kCcRun) void k_sp_faces_fill(SpKeepFlag flag, int F, const int* __restrict__ bsum, const int* __restrict__ rot,
                                                          int* __restrict__ out) {
    __shared__ int wsum[kCcRun / kWave];
    const int t = sp_item(F);
    const int fl = flag(t);
    int all;
    const int to = bsum[blockIdx.x] + block_scan_excl<kCcRun>(fl, wsum, all);
    if (!fl) return;                // to < the total <= F: inside out
    out[(size_t)to * 3] = rot[(size_t)t * 3];
    out[(size_t)to * 3 + 1] = rot[(size_t)t * 3 + 1];
    out[(size_t)to * 3 + 2] = rot[(size_t)t * 3 + 2];
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------
static bool sp_count_ok(int64_t n) { return n >= 0 && n < (1ll << 31); }
static bool sp_faces_ok(int64_t F) { return F >= 0 && F <= ((1ll << 31) - 1) / 3; }

// false for a grid the kernels must not see: a cell that is not finite and positive, an origin that is not finite, a dimension < 1,
// 2^31 cells and more
static bool sp_grid(const double* origin3, const double* cell3, const int32_t* dims3, SpGrid& g) {
    if (!origin3 || !cell3 || !dims3) return false;
    long long cells = 1;
    for (int k = 0; k < 3; ++k) {
        g.o[k] = origin3[k]; g.h[k] = cell3[k]; g.n[k] = dims3[k];
        if (!(g.h[k] > 0.0) || g.h[k] - g.h[k] != 0.0 || g.o[k] - g.o[k] != 0.0 || g.n[k] < 1) return false;
        cells *= g.n[k];
        if (cells >= (1ll << 31)) return false;
    }
    return true;
}

// workspace of the two compactions: per-workgroup sums [nb] int32 | (faces only) keep [n] uint8, each region rounded up to 256 bytes
struct SpCarve { size_t bsum, keep, total; int nb; };
static SpCarve sp_carve(int64_t n, bool with_keep) {
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    SpCarve c;
    c.nb = (int)((n + kCcRun - 1) / kCcRun);
    c.bsum = 0;
    c.keep = c.bsum + up((size_t)c.nb * 4) + 256;       // never 0 for a good argument
    c.total = c.keep + (with_keep ? up((size_t)n) : 0);
    return c;
}

static dim3 sp_blocks(int64_t n) { return dim3((unsigned)((n + kCcRun - 1) / kCcRun)); }

}  // namespace t2n

using namespace t2n;

extern "C" int t2n_mesh_cluster_keys(const float* verts, int64_t n_verts, const double* origin3, const double* cell3, const int32_t* dims3,
                                     int64_t* keys, t2n_stream stream) {
    SpGrid g;
    if (!sp_count_ok(n_verts) || !sp_grid(origin3, cell3, dims3, g) || (n_verts > 0 && (!verts || !keys))) {
        set_error("t2n_mesh_cluster_keys: bad argument (NULL pointer, a negative count, 2^31 vertices and more, a cell that is not finite and "
                  "positive, an origin that is not finite, a dimension < 1, or 2^31 cells and more)");
        return T2N_ERR_INVALID;
    }
    if (n_verts == 0) return T2N_OK;
    hipLaunchKernelGGL(k_sp_vertex_keys, sp_blocks(n_verts), dim3(kCcRun), 0, (hipStream_t)stream, verts, (int)n_verts, g, (long long*)keys);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" size_t t2n_mesh_cluster_rows_workspace_bytes(int64_t n_verts) {
    if (!sp_count_ok(n_verts)) return 0;
    return sp_carve(n_verts, false).total;
}

extern "C" int t2n_mesh_cluster_rows(const int64_t* sorted_keys, int64_t n_verts, const int32_t* dims3, int32_t* vertex_map, int64_t* offsets,
                                     int32_t* members, int32_t* cells, int64_t* n_clusters_out, void* workspace, size_t workspace_bytes,
                                     t2n_stream stream) {
    SpGrid g;
    const double zero[3] = {0.0, 0.0, 0.0}, one[3] = {1.0, 1.0, 1.0};
    if (!sp_count_ok(n_verts) || !sp_grid(zero, one, dims3, g) || !offsets || !n_clusters_out || !workspace ||
        (n_verts > 0 && (!sorted_keys || !vertex_map || !members || !cells)) || workspace_bytes < sp_carve(n_verts, false).total) {
        set_error("t2n_mesh_cluster_rows: bad argument (NULL pointer, a negative count, 2^31 vertices and more, a dimension < 1, 2^31 cells and "
                  "more, or a workspace smaller than t2n_mesh_cluster_rows_workspace_bytes)");
        return T2N_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const SpCarve c = sp_carve(n_verts, false);
    const int n = (int)n_verts;
    int* bsum = (int*)((char*)workspace + c.bsum);
    if (n == 0) {               // K = 0 and offsets[0] = 0, by the scan of no sums and one memset
        T2N_HIP(hipMemsetAsync(offsets, 0, sizeof(int64_t), s));
        T2N_HIP(hipMemsetAsync(n_clusters_out, 0, sizeof(int64_t), s));
        return T2N_OK;
    }
    const SpRowFlag flag{(const long long*)sorted_keys, n, n};
    hipLaunchKernelGGL(k_sp_flags<SpRowFlag>, dim3((unsigned)c.nb), dim3(kCcRun), 0, s, flag, n, bsum);
    hipLaunchKernelGGL(k_sp_scan, dim3(1), dim3(kMcScanChunk), 0, s, bsum, c.nb, (long long*)n_clusters_out);
    hipLaunchKernelGGL(k_sp_rows_fill, dim3((unsigned)c.nb), dim3(kCcRun), 0, s, flag, n, g, (const int*)bsum, vertex_map, (long long*)offsets,
                       members, cells);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" int t2n_mesh_cluster_face_keys(const int32_t* faces, int64_t n_faces, int64_t n_verts, const int32_t* vertex_map, int64_t n_clusters,
                                          int64_t* keys, t2n_stream stream) {
    if (!sp_count_ok(n_verts) || !sp_faces_ok(n_faces) || n_clusters < 0 || n_clusters > n_verts ||
        (n_faces > 0 && (!faces || !keys || (n_verts > 0 && !vertex_map)))) {
        set_error("t2n_mesh_cluster_face_keys: bad argument (NULL pointer, a negative count, 2^31 vertices and more, 3 * n_faces >= 2^31, or "
                  "n_clusters outside [0, n_verts])");
        return T2N_ERR_INVALID;
    }
    if (n_faces == 0) return T2N_OK;
    hipLaunchKernelGGL(k_sp_face_keys, sp_blocks(n_faces), dim3(kCcRun), 0, (hipStream_t)stream, faces, (int)n_faces, (int)n_verts, vertex_map,
                       (int)n_clusters, (long long*)keys);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" int t2n_mesh_cluster_place(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const int64_t* offsets,
                                      const int32_t* members, int64_t n_members, const int32_t* cells, int64_t n_clusters,
                                      const int64_t* face_offsets, const int32_t* face_rows, int64_t n_entries, const double* origin3,
                                      const double* cell3, double regularisation, int quadric, float* out, t2n_stream stream) {
    SpGrid g;
    const int32_t any[3] = {1, 1, 1};
    const bool q = quadric != 0;
    if (!sp_count_ok(n_verts) || !sp_faces_ok(n_faces) || n_clusters < 0 || n_clusters > n_verts || n_members < 0 || n_entries < 0 ||
        !sp_grid(origin3, cell3, any, g) || !(regularisation >= 0.0) || regularisation - regularisation != 0.0 || (quadric != 0 && quadric != 1) ||
        (n_clusters > 0 && (!verts || !offsets || !out || (n_members > 0 && !members))) ||
        (q && n_clusters > 0 && (!cells || !face_offsets || (n_entries > 0 && (!face_rows || !faces))))) {
        set_error("t2n_mesh_cluster_place: bad argument (NULL pointer, a negative count, 2^31 vertices and more, 3 * n_faces >= 2^31, n_clusters "
                  "outside [0, n_verts], a cell that is not finite and positive, an origin or a regularisation that is not finite, a negative "
                  "regularisation, or quadric outside {0, 1})");
        return T2N_ERR_INVALID;
    }
    if (n_clusters == 0) return T2N_OK;
    hipLaunchKernelGGL(k_sp_place, sp_blocks(n_clusters), dim3(kCcRun), 0, (hipStream_t)stream, verts, (int)n_verts, faces, (int)n_faces,
                       (const long long*)offsets, members, (long long)n_members, cells, (int)n_clusters, (const long long*)face_offsets, face_rows,
                       (long long)n_entries, g, regularisation, q ? 1 : 0, out);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" int t2n_mesh_cluster_colors(const uint8_t* colors, int64_t n_verts, const int64_t* offsets, const int32_t* members, int64_t n_members,
                                       int64_t n_clusters, uint8_t* out, t2n_stream stream) {
    if (!sp_count_ok(n_verts) || n_clusters < 0 || n_clusters > n_verts || n_members < 0 ||
        (n_clusters > 0 && (!colors || !offsets || !out || (n_members > 0 && !members)))) {
        set_error("t2n_mesh_cluster_colors: bad argument (NULL pointer, a negative count, 2^31 vertices and more, or n_clusters outside [0, n_verts])");
        return T2N_ERR_INVALID;
    }
    if (n_clusters == 0) return T2N_OK;
    hipLaunchKernelGGL(k_sp_colors, sp_blocks(n_clusters), dim3(kCcRun), 0, (hipStream_t)stream, colors, (int)n_verts, (const long long*)offsets,
                       members, (long long)n_members, (int)n_clusters, out);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" int t2n_mesh_simplify_face_map(const int32_t* faces, int64_t n_faces, int64_t n_verts, const int32_t* vertex_map, int64_t n_clusters,
                                          int32_t* rotated, int64_t* key_hi, int64_t* key_lo, t2n_stream stream) {
    if (!sp_count_ok(n_verts) || !sp_faces_ok(n_faces) || n_clusters < 0 || n_clusters > n_verts ||
        (n_faces > 0 && (!faces || !rotated || !key_hi || !key_lo || (n_verts > 0 && !vertex_map)))) {
        set_error("t2n_mesh_simplify_face_map: bad argument (NULL pointer, a negative count, 2^31 vertices and more, 3 * n_faces >= 2^31, or "
                  "n_clusters outside [0, n_verts])");
        return T2N_ERR_INVALID;
    }
    if (n_faces == 0) return T2N_OK;
    hipLaunchKernelGGL(k_sp_face_map, sp_blocks(n_faces), dim3(kCcRun), 0, (hipStream_t)stream, faces, (int)n_faces, (int)n_verts, vertex_map,
                       (int)n_clusters, rotated, (long long*)key_hi, (long long*)key_lo);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" size_t t2n_mesh_simplify_faces_workspace_bytes(int64_t n_faces) {
    if (!sp_faces_ok(n_faces)) return 0;
    return sp_carve(n_faces, true).total;
}

extern "C" int t2n_mesh_simplify_faces(const int32_t* rotated, const int64_t* order, int64_t n_faces, int32_t* faces_out, int64_t* count_out,
                                       void* workspace, size_t workspace_bytes, t2n_stream stream) {
    if (!sp_faces_ok(n_faces) || !count_out || !workspace || (n_faces > 0 && (!rotated || !order || !faces_out)) ||
        workspace_bytes < sp_carve(n_faces, true).total) {
        set_error("t2n_mesh_simplify_faces: bad argument (NULL pointer, a negative count, 3 * n_faces >= 2^31, or a workspace smaller than "
                  "t2n_mesh_simplify_faces_workspace_bytes)");
        return T2N_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    if (n_faces == 0) {
        T2N_HIP(hipMemsetAsync(count_out, 0, sizeof(int64_t), s));
        return T2N_OK;
    }
    const SpCarve c = sp_carve(n_faces, true);
    const int F = (int)n_faces;
    int* bsum = (int*)((char*)workspace + c.bsum);
    uint8_t* keep = (uint8_t*)workspace + c.keep;
    T2N_HIP(hipMemsetAsync(keep, 0, (size_t)F, s));
    const dim3 grid((unsigned)c.nb), nt(kCcRun);
    hipLaunchKernelGGL(k_sp_face_first, grid, nt, 0, s, rotated, (const long long*)order, F, keep);
    const SpKeepFlag flag{keep, F};
    hipLaunchKernelGGL(k_sp_flags<SpKeepFlag>, grid, nt, 0, s, flag, F, bsum);
    hipLaunchKernelGGL(k_sp_scan, dim3(1), dim3(kMcScanChunk), 0, s, bsum, c.nb, (long long*)count_out);
    hipLaunchKernelGGL(k_sp_faces_fill, grid, nt, 0, s, flag, F, (const int*)bsum, rotated, faces_out);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}
