// Mesh export, the stage behind marching cubes and floater removal: vertex adjacency and vertex->face rows of a triangle list as CSR
// arrays, Taubin (lambda | mu) smoothing of the positions in float64, area-weighted vertex normals. Every output is a function of the
// face SET and the positions alone: no float atomics, no dependence on the order the threads ran in.
//   rows      both CSR arrays come from 64-bit keys (row << 32 | value), one launch to write them (k_csr_edge_keys: the six directed
//             edges of a face, a -> b for a != b; k_csr_face_keys: (vertex, face) for the three corners), the caller's radix sort, and
//             t2n_mesh_csr over the SORTED keys: a key that differs from its predecessor is kept (k_csr_flags + k_csr_scan + k_csr_fill,
//             the count / scan / emit shape of t2n_mesh.hip), row v starts at the lower bound of v << 32 among the kept keys
//             (k_csr_offsets). So every row is ascending and unique, whatever the face order was. Keys of skipped edges (both ends
//             equal) and of faces with an index outside [0, V) are kCsrNone, which sorts behind every real key.
//   smoothing one thread per vertex walks its row in its ascending order: sum from 0.0, / degree, - x, * s, + x, each operation rounded
//             on its own in float64 (the library is built without floating-point contraction). Ping-pong buffers are the caller's.
//   normals   one thread per vertex walks its faces in ascending face index: n += (x_b - x_a) x (x_c - x_a) in float64 from the
//             float32 positions, prescaled by the largest |component|, divided by the norm, rounded to float32 once.
#include "t2n_internal.h"
#include "t2n_cc.h"      // block_scan_excl, kMcScanChunk, kCcRun

namespace t2n {

constexpr long long kCsrNone = 0x7fffffffffffffffll;

// this thread's element of n (n < 2^31), or n for the threads beyond
__device__ __forceinline__ int csr_item(int n) {
    const long long t = (long long)blockIdx.x * kCcRun + threadIdx.x;
    return t < n ? (int)t : n;
}

__device__ __forceinline__ bool csr_face(const int* __restrict__ faces, int t, int V, int f[3]) {
    const int* p = faces + (size_t)t * 3;
    f[0] = p[0]; f[1] = p[1]; f[2] = p[2];
    return (unsigned)f[0] < (unsigned)V && (unsigned)f[1] < (unsigned)V && (unsigned)f[2] < (unsigned)V;
}

__device__ __forceinline__ long long csr_key(int row, int value) { return (long long)row << 32 | (long long)(unsigned)value; }

// keys [6 F]: face t writes a->b, b->a, b->c, c->b, c->a, a->c
__global__ __launch_bounds__(kCcRun) void k_csr_edge_keys(const int* __restrict__ faces, int F, int V, long long* __restrict__ keys) {
    const int t = csr_item(F);
    if (t >= F) return;
    int f[3];
    const bool ok = csr_face(faces, t, V, f);
    long long* o = keys + (size_t)t * 6;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const int a = f[e], b = f[(e + 1) % 3];
        const bool keep = ok && a != b;
        o[2 * e] = keep ? csr_key(a, b) : kCsrNone;
        o[2 * e + 1] = keep ? csr_key(b, a) : kCsrNone;
    }
}

// keys [3 F]: face t writes (f0, t), (f1, t), (f2, t); a vertex twice in a face gives one key twice, which t2n_mesh_csr keeps once
__global__ __launch_bounds__(kCcRun) void k_csr_face_keys(const int* __restrict__ faces, int F, int V, long long* __restrict__ keys) {
    const int t = csr_item(F);
    if (t >= F) return;
    int f[3];
    const bool ok = csr_face(faces, t, V, f);
    long long* o = keys + (size_t)t * 3;
#pragma unroll
    for (int e = 0; e < 3; ++e) o[e] = ok ? csr_key(f[e], t) : kCsrNone;
}

__device__ __forceinline__ int csr_flag(const long long* __restrict__ keys, int i, int n, int V) {
    if (i >= n) return 0;
    const long long k = keys[i];
    // a row outside [0, V) (kCsrNone among them) is dropped: the rows below never index past V
    if (k < 0 || (k >> 32) >= V) return 0;
    return i == 0 || keys[i - 1] != k ? 1 : 0;
}

__global__ __launch_bounds__(kCcRun) void k_csr_flags(const long long* __restrict__ keys, int n, int V, int* __restrict__ bsum) {
    __shared__ int wsum[kCcRun / kWave];
    int all;
    block_scan_excl<kCcRun>(csr_flag(keys, csr_item(n), n, V), wsum, all);
    if (threadIdx.x == 0) bsum[blockIdx.x] = all;
}

// exclusive scan of a[0..nb) in place by one workgroup with a running carry (k_mc_scan's steps); the total to total[0]
__global__ __launch_bounds__(kMcScanChunk) void k_csr_scan(int* __restrict__ a, int nb, long long* __restrict__ total) {
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

__global__ __launch_bounds__(kCcRun) void k_csr_fill(const long long* __restrict__ keys, int n, int V, const int* __restrict__ bsum,
                                                     long long* __restrict__ ukeys, int* __restrict__ values) {
    __shared__ int wsum[kCcRun / kWave];
    const int i = csr_item(n);
    const int flag = csr_flag(keys, i, n, V);
    int all;
    const int to = bsum[blockIdx.x] + block_scan_excl<kCcRun>(flag, wsum, all);
    if (!flag) return;              // to < the total <= n: inside both arrays
    const long long k = keys[i];
    ukeys[to] = k;
    values[to] = (int)(k & 0xffffffffll);
}

// offsets[v] = the number of kept keys below v << 32, v = 0 .. V (offsets[V] = the total)
__global__ __launch_bounds__(kCcRun) void k_csr_offsets(const long long* __restrict__ ukeys, const long long* __restrict__ total, int V,
                                                        long long* __restrict__ offsets) {
    const long long v = (long long)blockIdx.x * kCcRun + threadIdx.x;
    if (v > V) return;
    const long long want = v << 32;
    long long lo = 0, hi = total[0];
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (ukeys[mid] < want) lo = mid + 1; else hi = mid;
    }
    offsets[v] = lo;
}

// y_v = x_v + s * (mean of x_u over row v - x_v); a vertex with an empty row or a set `fixed` byte keeps its position. Rows are clipped
// to [0, E) and a neighbour outside [0, V) is skipped (the Python layer refuses such arrays; no memory is touched through them).
__global__ __launch_bounds__(kCcRun) void k_smooth_pass(const double* __restrict__ x, double* __restrict__ y, const long long* __restrict__ offsets,
                                                        const int* __restrict__ nbr, long long E, const uint8_t* __restrict__ fixed, int V,
                                                        double s) {
    const int v = csr_item(V);
    if (v >= V) return;
    const double x0 = x[(size_t)v * 3], x1 = x[(size_t)v * 3 + 1], x2 = x[(size_t)v * 3 + 2];
    long long b = offsets[v], e = offsets[v + 1];
    b = b < 0 ? 0 : b;
    e = e > E ? E : e;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    long long deg = 0;
    if (!(fixed && fixed[v])) {
        for (long long q = b; q < e; ++q) {
            const int u = nbr[q];
            if ((unsigned)u >= (unsigned)V) continue;
            const double* p = x + (size_t)u * 3;
            s0 = s0 + p[0];
            s1 = s1 + p[1];
            s2 = s2 + p[2];
            ++deg;
        }
    }
    double* o = y + (size_t)v * 3;
    if (deg == 0) { o[0] = x0; o[1] = x1; o[2] = x2; return; }
    const double d = (double)deg;
    o[0] = x0 + s * (s0 / d - x0);
    o[1] = x1 + s * (s1 / d - x1);
    o[2] = x2 + s * (s2 / d - x2);
}

__global__ __launch_bounds__(kCcRun) void k_vertex_normals(const float* __restrict__ verts, const int* __restrict__ faces, int F,
                                                           const long long* __restrict__ offsets, const int* __restrict__ rows, long long E,
                                                           int V, float* __restrict__ normals) {
    const int v = csr_item(V);
    if (v >= V) return;
    long long b = offsets[v], e = offsets[v + 1];
    b = b < 0 ? 0 : b;
    e = e > E ? E : e;
    double n0 = 0.0, n1 = 0.0, n2 = 0.0;
    for (long long q = b; q < e; ++q) {
        const int t = rows[q];
        int f[3];
        if ((unsigned)t >= (unsigned)F || !csr_face(faces, t, V, f)) continue;
        const float* pa = verts + (size_t)f[0] * 3;
        const float* pb = verts + (size_t)f[1] * 3;
        const float* pc = verts + (size_t)f[2] * 3;
        const double a0 = pa[0], a1 = pa[1], a2 = pa[2];
        const double u0 = (double)pb[0] - a0, u1 = (double)pb[1] - a1, u2 = (double)pb[2] - a2;
        const double w0 = (double)pc[0] - a0, w1 = (double)pc[1] - a1, w2 = (double)pc[2] - a2;
        n0 = n0 + (u1 * w2 - u2 * w1);
        n1 = n1 + (u2 * w0 - u0 * w2);
        n2 = n2 + (u0 * w1 - u1 * w0);
    }
    const double m = fmax(fmax(fabs(n0), fabs(n1)), fabs(n2));
    float* o = normals + (size_t)v * 3;
    // zero stays zero; so does a sum that is not finite (fmax drops a NaN operand: the components are tested themselves)
    if (!(m > 0.0 && m < (double)INFINITY) || n0 != n0 || n1 != n1 || n2 != n2) { o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f; return; }
    const double h0 = n0 / m, h1 = n1 / m, h2 = n2 / m;
    const double len = sqrt(h0 * h0 + h1 * h1 + h2 * h2);
    o[0] = (float)(h0 / len);
    o[1] = (float)(h1 / len);
    o[2] = (float)(h2 / len);
}

// workspace of t2n_mesh_csr: kept keys [n] int64 | per-workgroup sums [nb] int32, each region rounded up to 256 bytes
struct CsrCarve { size_t ukeys, bsum, total; int nb; };
static bool csr_keys_ok(int64_t n) { return n >= 0 && n < (1ll << 31); }
static bool csr_counts_ok(int64_t V, int64_t F) { return V >= 0 && F >= 0 && V < (1ll << 31) && F <= ((1ll << 31) - 1) / 6; }
static CsrCarve csr_carve(int64_t n) {
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    CsrCarve c;
    c.nb = (int)((n + kCcRun - 1) / kCcRun);
    c.ukeys = 0;
    c.bsum = c.ukeys + up((size_t)n * 8);
    c.total = c.bsum + up((size_t)c.nb * 4) + 256;      // never 0 for a good argument
    return c;
}

}  // namespace t2n

using namespace t2n;

extern "C" size_t t2n_mesh_csr_workspace_bytes(int64_t n_keys) {
    if (!csr_keys_ok(n_keys)) return 0;
    return csr_carve(n_keys).total;
}

static int csr_keys_call(const char* who, bool edges, const int32_t* faces, int64_t n_faces, int64_t n_verts, int64_t* keys, t2n_stream stream) {
    if (!csr_counts_ok(n_verts, n_faces) || (n_faces > 0 && (!faces || !keys))) {
        set_error("%s: bad argument (NULL pointer, a negative count, 2^31 vertices and more, or 6 * n_faces >= 2^31)", who);
        return T2N_ERR_INVALID;
    }
    if (n_faces == 0) return T2N_OK;
    const dim3 grid((unsigned)((n_faces + kCcRun - 1) / kCcRun)), nt(kCcRun);
    if (edges) hipLaunchKernelGGL(k_csr_edge_keys, grid, nt, 0, (hipStream_t)stream, faces, (int)n_faces, (int)n_verts, (long long*)keys);
    else hipLaunchKernelGGL(k_csr_face_keys, grid, nt, 0, (hipStream_t)stream, faces, (int)n_faces, (int)n_verts, (long long*)keys);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" int t2n_mesh_edge_keys(const int32_t* faces, int64_t n_faces, int64_t n_verts, int64_t* keys, t2n_stream stream) {
    return csr_keys_call("t2n_mesh_edge_keys", true, faces, n_faces, n_verts, keys, stream);
}

extern "C" int t2n_mesh_face_keys(const int32_t* faces, int64_t n_faces, int64_t n_verts, int64_t* keys, t2n_stream stream) {
    return csr_keys_call("t2n_mesh_face_keys", false, faces, n_faces, n_verts, keys, stream);
}

extern "C" int t2n_mesh_csr(const int64_t* sorted_keys, int64_t n_keys, int64_t n_rows, int64_t* offsets, int32_t* values, int64_t* count_out,
                            void* workspace, size_t workspace_bytes, t2n_stream stream) {
    if (!csr_keys_ok(n_keys) || n_rows < 0 || n_rows >= (1ll << 31) || (n_keys > 0 && (!sorted_keys || !values)) || !offsets || !count_out ||
        !workspace || workspace_bytes < csr_carve(n_keys).total) {
        set_error("t2n_mesh_csr: bad argument (NULL pointer, a negative count, 2^31 keys or rows and more, or a workspace smaller than "
                  "t2n_mesh_csr_workspace_bytes)");
        return T2N_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const CsrCarve c = csr_carve(n_keys);
    const int n = (int)n_keys, V = (int)n_rows;
    char* ws = (char*)workspace;
    long long* ukeys = (long long*)(ws + c.ukeys);
    int* bsum = (int*)(ws + c.bsum);
    const dim3 gk((unsigned)c.nb), nt(kCcRun);
    if (n > 0) hipLaunchKernelGGL(k_csr_flags, gk, nt, 0, s, (const long long*)sorted_keys, n, V, bsum);
    hipLaunchKernelGGL(k_csr_scan, dim3(1), dim3(kMcScanChunk), 0, s, bsum, c.nb, (long long*)count_out);
    if (n > 0) hipLaunchKernelGGL(k_csr_fill, gk, nt, 0, s, (const long long*)sorted_keys, n, V, (const int*)bsum, ukeys, values);
    hipLaunchKernelGGL(k_csr_offsets, dim3((unsigned)((n_rows + 1 + kCcRun - 1) / kCcRun)), nt, 0, s, (const long long*)ukeys,
                       (const long long*)count_out, V, (long long*)offsets);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" int t2n_mesh_smooth_pass(const double* pos_in, double* pos_out, const int64_t* offsets, const int32_t* neighbours, int64_t n_entries,
                                    const uint8_t* fixed_or_null, int64_t n_verts, double s, t2n_stream stream) {
    if (n_verts < 0 || n_verts >= (1ll << 31) || n_entries < 0 || (n_verts > 0 && (!pos_in || !pos_out || !offsets)) ||
        (n_entries > 0 && !neighbours) || pos_in == pos_out || !(s == s) || s - s != 0.0) {
        set_error("t2n_mesh_smooth_pass: bad argument (NULL pointer, a negative count, 2^31 vertices and more, pos_out == pos_in, or a "
                  "factor that is not finite)");
        return T2N_ERR_INVALID;
    }
    if (n_verts == 0) return T2N_OK;
    hipLaunchKernelGGL(k_smooth_pass, dim3((unsigned)((n_verts + kCcRun - 1) / kCcRun)), dim3(kCcRun), 0, (hipStream_t)stream, pos_in, pos_out,
                       (const long long*)offsets, neighbours, (long long)n_entries, fixed_or_null, (int)n_verts, s);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" int t2n_mesh_vertex_normals(const float* verts, const int32_t* faces, int64_t n_faces, const int64_t* vf_offsets,
                                       const int32_t* vf_faces, int64_t n_entries, int64_t n_verts, float* normals, t2n_stream stream) {
    if (!csr_counts_ok(n_verts, n_faces) || n_entries < 0 || (n_verts > 0 && (!verts || !vf_offsets || !normals)) || (n_faces > 0 && !faces) ||
        (n_entries > 0 && !vf_faces)) {
        set_error("t2n_mesh_vertex_normals: bad argument (NULL pointer, a negative count, 2^31 vertices and more, or 6 * n_faces >= 2^31)");
        return T2N_ERR_INVALID;
    }
    if (n_verts == 0) return T2N_OK;
    hipLaunchKernelGGL(k_vertex_normals, dim3((unsigned)((n_verts + kCcRun - 1) / kCcRun)), dim3(kCcRun), 0, (hipStream_t)stream, verts, faces,
                       (int)n_faces, (const long long*)vf_offsets, vf_faces, (long long)n_entries, (int)n_verts, normals);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}
