// Mesh export: TSDF fusion of depth views into a dense volume [n0][n1][n2] (last index fastest, node (a,b,c) at origin + (a,b,c) *
// spacing: t2n_mc_emit's frame), the stage users of depth-supervised scenes run on the host after dumping depth maps. Definitions in
// include/t2n.h; every float64 operation below is one IEEE operation in the written order (the library is built without contraction),
// double divide and sqrt are correctly rounded, so the state is a function of the inputs alone: no atomics, a node is owned by one thread.
//   k_tsdf_integrate      one thread per node, node-linear (consecutive lanes along n2: state loads and stores coalesce). The view loop
//                         is inside the kernel with the node's state in registers: the state is read once and written once per call (and
//                         not written at all by a node that no view updated), rounded to float32 after every view as the definition
//                         asks. The matrices are indexed by the loop's (uniform) view index: scalar loads. Gates in the order of their
//                         cost: p_2 > near (three products), a division-free frustum test that can only pass what the exact test may
//                         pass (below), then the two divides, the pixel, and only for a valid pixel the square root.
//   k_tsdf_face_flags     one thread per face: the observed-cells rule on the cell of the face's centroid
//   k_tsdf_sample_colors  one thread per vertex: trilinear colour over the observed corners of the vertex's cell
#include "t2n_internal.h"

namespace t2n {

constexpr int kTsdfRun = 256;        // nodes / faces / vertices per workgroup

struct TsdfFrame { double o[3], s[3]; int n0, n1, n2, n; };
struct TsdfViews {
    const float* depth; const float* rgb; const float* pw; const double* w2c;
    int V, H, W, kind;
    double fx, fy, cx, cy, trunc, near, max_weight;
    double bu, bv;        // |fx p_0| > bu p_2 (|fy p_1| > bv p_2) proves u (v) outside [0, W) ([0, H)): see k_tsdf_integrate
};

__global__ __launch_bounds__(kTsdfRun) void k_tsdf_integrate(float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ color,
                                                             TsdfFrame f, TsdfViews in) {
    const long long t = (long long)blockIdx.x * kTsdfRun + threadIdx.x;
    if (t >= f.n) return;
    const int c = (int)(t % f.n2), r = (int)(t / f.n2);
    const int b = r % f.n1, a = r / f.n1;
    const double x0 = f.o[0] + (double)a * f.s[0], x1 = f.o[1] + (double)b * f.s[1], x2 = f.o[2] + (double)c * f.s[2];
    float T = tsdf[t], Wt = weight[t];
    float C0 = 0.f, C1 = 0.f, C2 = 0.f;
    if (color) { C0 = color[t * 3]; C1 = color[t * 3 + 1]; C2 = color[t * 3 + 2]; }
    bool touched = false;
    const size_t plane = (size_t)in.H * in.W;
    for (int v = 0; v < in.V; ++v) {
        const double* __restrict__ M = in.w2c + (size_t)v * 12;
        const double p2 = ((M[8] * x0 + M[9] * x1) + M[10] * x2) + M[11];
        if (!(p2 > in.near)) continue;
        const double p0 = ((M[0] * x0 + M[1] * x1) + M[2] * x2) + M[3];
        const double p1 = ((M[4] * x0 + M[5] * x1) + M[6] * x2) + M[7];
        const double a0 = in.fx * p0, a1 = in.fy * p1;
        // Without a divide: bu = (W + |cx| + 2) (1 + 2^-40). For p_2 > 0, |a0| > bu p_2 (the product rounded, 2^-53) puts |a0 / p_2|
        // above W + |cx| + 2, so does its rounded value, and adding cx leaves u >= W + 1 or u <= -1: the exact test below skips the
        // view too. Everything else (a NaN compares false; p_2 <= 0 under a negative `near`) goes on to the exact test.
        if (p2 > 0.0 && (fabs(a0) > in.bu * p2 || fabs(a1) > in.bv * p2)) continue;
        const double u = a0 / p2 + in.cx, w = a1 / p2 + in.cy;
        if (!(u >= 0.0 && u < (double)in.W && w >= 0.0 && w < (double)in.H)) continue;
        const int i = (int)u, j = (int)w;               // floor of a value in [0, W): the nearest pixel, pixel i spans [i, i + 1)
        const size_t px = (size_t)v * plane + (size_t)j * in.W + i;
        const float df = in.depth[px];
        if (!(df > 0.0f && df < INFINITY)) continue;    // 0, negatives, NaN and +inf are no measurement
        double pw = 1.0;
        if (in.pw) {
            const float q = in.pw[px];
            if (!(q > 0.0f && q < INFINITY)) continue;
            pw = (double)q;
        }
        const double rr = in.kind == 0 ? sqrt((p0 * p0 + p1 * p1) + p2 * p2) : p2;
        const double sdf = (double)df - rr;
        if (sdf < -in.trunc) continue;
        const double s = fmin(1.0, sdf / in.trunc);
        const double Wo = (double)Wt, Wn = Wo + pw;
        T = (float)((Wo * (double)T + pw * s) / Wn);
        if (in.rgb) {
            const float* __restrict__ q = in.rgb + px * 3;
            C0 = (float)((Wo * (double)C0 + pw * (double)q[0]) / Wn);
            C1 = (float)((Wo * (double)C1 + pw * (double)q[1]) / Wn);
            C2 = (float)((Wo * (double)C2 + pw * (double)q[2]) / Wn);
        }
        Wt = (float)fmin(Wn, in.max_weight);
        touched = true;
    }
    if (!touched) return;
    tsdf[t] = T;
    weight[t] = Wt;
    if (color && in.rgb) { color[t * 3] = C0; color[t * 3 + 1] = C1; color[t * 3 + 2] = C2; }
}

// cell_k = clamp((int)floor(g), 0, n - 2), the clamp taken in double (a NaN gives 0)
__device__ __forceinline__ int tsdf_cell(double g, int n) {
    const double fl = floor(g);
    return fl >= (double)(n - 2) ? n - 2 : (fl > 0.0 ? (int)fl : 0);
}

__device__ __forceinline__ bool tsdf_seen(const float* __restrict__ weight, const TsdfFrame& f, int c0, int c1, int c2, double min_weight) {
    return (double)weight[((size_t)c0 * f.n1 + c1) * f.n2 + c2] > min_weight;
}

__global__ __launch_bounds__(kTsdfRun) void k_tsdf_face_flags(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                              const float* __restrict__ weight, TsdfFrame f, double min_weight,
                                                              uint8_t* __restrict__ keep) {
    const long long t = (long long)blockIdx.x * kTsdfRun + threadIdx.x;
    if (t >= F) return;
    const int* p = faces + (size_t)t * 3;
    const int ia = p[0], ib = p[1], ic = p[2];
    if ((unsigned)ia >= (unsigned)V || (unsigned)ib >= (unsigned)V || (unsigned)ic >= (unsigned)V) { keep[t] = 0; return; }
    int cell[3];
    const int n[3] = {f.n0, f.n1, f.n2};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double ck = (((double)verts[(size_t)ia * 3 + k] + (double)verts[(size_t)ib * 3 + k]) + (double)verts[(size_t)ic * 3 + k]) / 3.0;
        cell[k] = tsdf_cell((ck - f.o[k]) / f.s[k], n[k]);
    }
    bool all = true;
#pragma unroll
    for (int q = 0; q < 8; ++q) all = all && tsdf_seen(weight, f, cell[0] + (q >> 2 & 1), cell[1] + (q >> 1 & 1), cell[2] + (q & 1), min_weight);
    keep[t] = all ? 1 : 0;
}

__global__ __launch_bounds__(kTsdfRun) void k_tsdf_sample_colors(const float* __restrict__ verts, int V, const float* __restrict__ weight,
                                                                 const float* __restrict__ color, TsdfFrame f, double min_weight,
                                                                 uint8_t* __restrict__ out) {
    const long long t = (long long)blockIdx.x * kTsdfRun + threadIdx.x;
    if (t >= V) return;
    int cell[3];
    double fr[3];
    const int n[3] = {f.n0, f.n1, f.n2};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double g = ((double)verts[(size_t)t * 3 + k] - f.o[k]) / f.s[k];
        cell[k] = tsdf_cell(g, n[k]);
        fr[k] = fmin(fmax(g - (double)cell[k], 0.0), 1.0);      // (a NaN becomes 0)
    }
    double sw = 0.0, sc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 8; ++q) {                                // (0,0,0), (0,0,1), (0,1,0), ...: axis 2 fastest
        const int d0 = q >> 2 & 1, d1 = q >> 1 & 1, d2 = q & 1;
        const size_t node = ((size_t)(cell[0] + d0) * f.n1 + (cell[1] + d1)) * f.n2 + (cell[2] + d2);
        if (!((double)weight[node] > min_weight)) continue;
        const double wq = ((d0 ? fr[0] : 1.0 - fr[0]) * (d1 ? fr[1] : 1.0 - fr[1])) * (d2 ? fr[2] : 1.0 - fr[2]);
        sw = sw + wq;
#pragma unroll
        for (int k = 0; k < 3; ++k) sc[k] = sc[k] + wq * (double)color[node * 3 + k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double col = sw > 0.0 ? sc[k] / sw : 0.0;
        out[(size_t)t * 3 + k] = (uint8_t)rint(fmin(fmax(col, 0.0), 1.0) * 255.0);    // round half to even
    }
}

static bool tsdf_frame(int n0, int n1, int n2, int least, const float* origin3, const float* spacing3, TsdfFrame& f) {
    if (n0 < least || n1 < least || n2 < least || !origin3 || !spacing3) return false;
    for (int a = 0; a < 3; ++a) {
        if (!(spacing3[a] > 0.0f && spacing3[a] < INFINITY) || !(fabsf(origin3[a]) < INFINITY)) return false;
        f.o[a] = (double)origin3[a];
        f.s[a] = (double)spacing3[a];
    }
    f.n0 = n0; f.n1 = n1; f.n2 = n2;
    f.n = 0;
    return true;
}
static bool tsdf_nodes_fit(int n0, int n1, int n2) { return (long long)n0 * n1 * n2 < (1ll << 31); }

}  // namespace t2n

using namespace t2n;

extern "C" int t2n_tsdf_integrate(float* tsdf, float* weight, float* color_or_null, int n0, int n1, int n2, const float* depth,
                                  const float* rgb_or_null, const float* pixel_weight_or_null, const double* w2c, int n_views, int H, int W,
                                  double fx, double fy, double cx, double cy, const float* origin3, const float* spacing3, double trunc,
                                  double near, double max_weight, int kind, t2n_stream stream) {
    TsdfFrame f;
    const bool finite4 = fabs(fx) < INFINITY && fabs(fy) < INFINITY && fabs(cx) < INFINITY && fabs(cy) < INFINITY;
    if (!tsdf || !weight || !tsdf_frame(n0, n1, n2, 1, origin3, spacing3, f) || n_views < 0 || H < 1 || W < 1 ||
        (n_views > 0 && (!depth || !w2c)) || !rgb_or_null != !color_or_null || !finite4 || fx == 0.0 || fy == 0.0 ||
        !(trunc > 0.0 && trunc < INFINITY) || !(fabs(near) < INFINITY) || !(max_weight > 0.0) || (kind != 0 && kind != 1)) {
        set_error("t2n_tsdf_integrate: bad argument (NULL pointer, a dimension < 1, rgb and colour state on one side only, intrinsics that "
                  "are not finite or a zero focal length, a truncation or spacing that is not finite and positive, a max_weight that is "
                  "not > 0, or an unknown kind)");
        return T2N_ERR_INVALID;
    }
    if (!tsdf_nodes_fit(n0, n1, n2)) {
        set_error("t2n_tsdf_integrate: unsupported: a grid of 2^31 nodes and more");
        return T2N_ERR_UNSUPPORTED;
    }
    if (n_views == 0) return T2N_OK;
    f.n = n0 * n1 * n2;
    TsdfViews in{depth, rgb_or_null, pixel_weight_or_null, w2c, n_views, H, W, kind, fx, fy, cx, cy, trunc, near, max_weight, 0.0, 0.0};
    const double slack = 1.0 + 1.0 / 1099511627776.0;      // 1 + 2^-40
    in.bu = ((double)W + fabs(cx) + 2.0) * slack;
    in.bv = ((double)H + fabs(cy) + 2.0) * slack;
    const unsigned nb = (unsigned)(((long long)f.n + kTsdfRun - 1) / kTsdfRun);
    hipLaunchKernelGGL(k_tsdf_integrate, dim3(nb), dim3(kTsdfRun), 0, (hipStream_t)stream, tsdf, weight, color_or_null, f, in);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" int t2n_tsdf_face_flags(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* weight, int n0,
                                   int n1, int n2, const float* origin3, const float* spacing3, double min_weight, uint8_t* keep,
                                   t2n_stream stream) {
    TsdfFrame f;
    if (n_verts < 0 || n_faces < 0 || n_verts >= (1ll << 31) || n_faces > ((1ll << 31) - 1) / 3 || !weight ||
        !tsdf_frame(n0, n1, n2, 2, origin3, spacing3, f) || (n_faces > 0 && (!faces || !keep || !verts)) || min_weight != min_weight) {
        set_error("t2n_tsdf_face_flags: bad argument (NULL pointer, a negative count, 2^31 vertices or face indices and more, a dimension "
                  "< 2, a spacing that is not finite and positive, or a min_weight that is NaN)");
        return T2N_ERR_INVALID;
    }
    if (!tsdf_nodes_fit(n0, n1, n2)) {
        set_error("t2n_tsdf_face_flags: unsupported: a grid of 2^31 nodes and more");
        return T2N_ERR_UNSUPPORTED;
    }
    if (n_faces == 0) return T2N_OK;
    f.n = n0 * n1 * n2;
    hipLaunchKernelGGL(k_tsdf_face_flags, dim3((unsigned)((n_faces + kTsdfRun - 1) / kTsdfRun)), dim3(kTsdfRun), 0, (hipStream_t)stream, verts,
                       (int)n_verts, faces, (int)n_faces, weight, f, min_weight, keep);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" int t2n_tsdf_sample_colors(const float* verts, int64_t n_verts, const float* weight, const float* color, int n0, int n1, int n2,
                                      const float* origin3, const float* spacing3, double min_weight, uint8_t* colors_out, t2n_stream stream) {
    TsdfFrame f;
    if (n_verts < 0 || n_verts >= (1ll << 31) || !weight || !color || !tsdf_frame(n0, n1, n2, 2, origin3, spacing3, f) ||
        (n_verts > 0 && (!verts || !colors_out)) || min_weight != min_weight) {
        set_error("t2n_tsdf_sample_colors: bad argument (NULL pointer, a negative count, 2^31 vertices and more, a dimension < 2, a spacing "
                  "that is not finite and positive, or a min_weight that is NaN)");
        return T2N_ERR_INVALID;
    }
    if (!tsdf_nodes_fit(n0, n1, n2)) {
        set_error("t2n_tsdf_sample_colors: unsupported: a grid of 2^31 nodes and more");
        return T2N_ERR_UNSUPPORTED;
    }
    if (n_verts == 0) return T2N_OK;
    f.n = n0 * n1 * n2;
    hipLaunchKernelGGL(k_tsdf_sample_colors, dim3((unsigned)((n_verts + kTsdfRun - 1) / kTsdfRun)), dim3(kTsdfRun), 0, (hipStream_t)stream, verts,
                       (int)n_verts, weight, color, f, min_weight, colors_out);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}
