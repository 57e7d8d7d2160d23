// Shared declarations of the general-shape path: its argument blocks, the workspace carves and the inline device helpers that both
// directions use (t2n_generic.hip: forward and the plain backward; t2n_generic_bwd.hip: the backward as kernels).
#pragma once
#include "t2n_device.h"

namespace t2n {

constexpr int kGenDimMax = 64, kGenHidMax = 256, kGenInMax = 4096;

struct GenArgs {
    FieldDev F;                       // scalars only (aabb, step, thresholds, activation); the factor sets of F are unused here
    int grid[3], Cd[3], Ca[3], app_dim, shading, fea_pe, view_pe, fC, in0;
    const float* dp[3]; const float* dl[3]; const float* ap[3]; const float* al[3];
    const float* basis; const float* w0; const float* b0; const float* w1; const float* b1; const float* w2; const float* b2;
    float* g_dp[3]; float* g_dl[3]; float* g_ap[3]; float* g_al[3];
    float* g_basis; float* g_w0; float* g_b0; float* g_w1; float* g_b1; float* g_w2; float* g_b2;
    const float* rays; long long n_rays; int ray_stride; int N; int train; int add_bg;
    const float* jitter;
    float* rgb; float* depth;         // outputs
    float* w; float* z;               // [R, N] rows (the caller's tensors or workspace)
    float* sigma; float* T;           // [R, N] context: density and transmittance in front of every sample
    float* rgb_s;                     // [R, N, 3] colours of the appearance samples (context)
    float* acc; float* raw;           // [R] opacity, [R, 3] colour before the clamp
    const float* d_rgb; const float* d_depth; const float* d_w;   // upstream gradients
    float* go;                        // [R, N, 3] dL/d colour of the appearance samples (backward scratch)
    unsigned long long* stats;
};

struct Tap3 { Axis a[3]; };
__device__ __forceinline__ Tap3 gen_taps(const GenArgs& a, float xn, float yn, float zn) {
    Tap3 t;
    t.a[0] = axis_taps(xn, a.grid[0]); t.a[1] = axis_taps(yn, a.grid[1]); t.a[2] = axis_taps(zn, a.grid[2]);
    return t;
}
// plane k of a factor set in the reference layout: value(c, y, x) = P[(c * H + y) * W + x], H = grid[mat1(k)], W = grid[mat0(k)]
__device__ __forceinline__ float gen_plane(const float* __restrict__ P, int c, int H, int W, const Axis& ax, const Axis& ay) {
    const float* __restrict__ p = P + (size_t)c * H * W;
    float v = p[(size_t)ay.i0 * W + ax.i0] * (ay.w0 * ax.w0);
    v = fmaf(p[(size_t)ay.i0 * W + ax.i1], ay.w0 * ax.w1, v);
    v = fmaf(p[(size_t)ay.i1 * W + ax.i0], ay.w1 * ax.w0, v);
    v = fmaf(p[(size_t)ay.i1 * W + ax.i1], ay.w1 * ax.w1, v);
    return v;
}
__device__ __forceinline__ float gen_line(const float* __restrict__ Ln, int c, int Lsz, const Axis& al) {
    const float* __restrict__ p = Ln + (size_t)c * Lsz;
    return fmaf(p[al.i1], al.w1, p[al.i0] * al.w0);
}
__device__ __forceinline__ void gen_plane_add(float* __restrict__ G, int c, int H, int W, const Axis& ax, const Axis& ay, float g) {
    float* __restrict__ p = G + (size_t)c * H * W;
    atomicAdd(p + (size_t)ay.i0 * W + ax.i0, g * (ay.w0 * ax.w0));
    atomicAdd(p + (size_t)ay.i0 * W + ax.i1, g * (ay.w0 * ax.w1));
    atomicAdd(p + (size_t)ay.i1 * W + ax.i0, g * (ay.w1 * ax.w0));
    atomicAdd(p + (size_t)ay.i1 * W + ax.i1, g * (ay.w1 * ax.w1));
}
__device__ __forceinline__ void gen_line_add(float* __restrict__ G, int c, int Lsz, const Axis& al, float g) {
    float* __restrict__ p = G + (size_t)c * Lsz;
    atomicAdd(p + al.i0, g * al.w0);
    atomicAdd(p + al.i1, g * al.w1);
}

__device__ __forceinline__ float gen_density_feature(const GenArgs& a, const Tap3& t) {
    float feat = 0.f;
    for (int k = 0; k < 3; ++k) {
        const int W = a.grid[mat0(k)], H = a.grid[mat1(k)], Lz = a.grid[vecm(k)];
        const Axis& ax = t.a[mat0(k)]; const Axis& ay = t.a[mat1(k)]; const Axis& al = t.a[vecm(k)];
        for (int c = 0; c < a.Cd[k]; ++c) feat = fmaf(gen_plane(a.dp[k], c, H, W, ax, ay), gen_line(a.dl[k], c, Lz, al), feat);
    }
    return feat;
}

// box test, eval z gate and — when the field carries one — the AlphaGridMask (models/tensorBase.py:451-456): a masked sample is not
// evaluated and gets no density gradient. MASK = false: coordinates of a sample already known to be valid (the appearance kernels)
template <bool MASK = true>
__device__ __forceinline__ bool gen_point(const GenArgs& a, const Ray& ray, float z, float& xn, float& yn, float& zn) {
    bool ok = a.train ? sample_point<true>(a.F, ray, z, xn, yn, zn) : sample_point<false>(a.F, ray, z, xn, yn, zn);
    if (MASK && a.F.alpha && ok) ok = alpha_pass(a.F, ray, z);
    return ok;
}
// z_i: t_min + step (i [+ u]), or the NDC depth table (F.ztab) shared by all rays
__device__ __forceinline__ float gen_z(const GenArgs& a, const Ray& ray, int i, float u) {
    return a.train ? sample_z<true>(a.F, ray, i, u) : sample_z<false>(a.F, ray, i, 0.f);
}
// the ray's jitter draw (train mode; on the NDC path `jitter` is the [N] depth table instead)
__device__ __forceinline__ float gen_u(const GenArgs& a, long long r) { return (a.train && !a.F.ztab) ? a.jitter[r] : 0.f; }
// the heads' view direction: the ray's d, divided by |d| on the NDC path (models/tensorBase.py:445)
__device__ __forceinline__ void gen_dir(const GenArgs& a, const Ray& ray, float* dir) {
    dir[0] = ray.dx; dir[1] = ray.dy; dir[2] = ray.dz;
    if (a.F.ztab) { dir[0] = dir[0] / ray.norm; dir[1] = dir[1] / ray.norm; dir[2] = dir[2] / ray.norm; }
}

__device__ __forceinline__ void gen_sh9(const float* dir, float* sh) {   // models/sh.py:4-14,87-112 (degree 2)
    const float dx = dir[0], dy = dir[1], dz = dir[2];
    const float C0 = 0.28209479177387814f, C1 = 0.4886025119029199f;
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz, xy = dx * dy, yz = dy * dz, xz = dx * dz;
    sh[0] = C0; sh[1] = -C1 * dy; sh[2] = C1 * dz; sh[3] = -C1 * dx;
    sh[4] = 1.0925484305920792f * xy; sh[5] = -1.0925484305920792f * yz; sh[6] = 0.31539156525252005f * (2.0f * zz - xx - yy);
    sh[7] = -1.0925484305920792f * xz; sh[8] = 0.5462742152960396f * (xx - yy);
}

struct GenFast {
    const float* dp[3]; const float* dl[3]; const float* ap[3]; const float* al[3];   // channel-last copies
    int* list; unsigned* count; unsigned cap;
    int ncol;
    const float* w0p; const float* w1p; int ld0, ld1;   // MLP weights with rows padded to multiples of 16 floats (64-byte aligned rows: s_load_dwordx16)
    // MLP layers on the matrix cores (k_dense of t2n_heads.hip, exact-fp32 MFMA): the head kernel then only WRITES the input rows of
    // one pass of the list — entries [row0, row0 + rows_cap) — to x0 [rows_cap][ldx]; k_gen_out finishes from h1
    float* x0; int ldx; unsigned row0, rows_cap; HeadPlanDev* plan;
    int hbc;   // columns of Hb (a multiple of 16): the head kernel's LDS staging of the input rows
};
struct GenStageArgs { const float* src[12]; float* dst[12]; int C[12]; long long HW[12]; unsigned block0[13]; };

struct GenCarve { size_t w, z, sigma, T, rgb_s, acc, raw, go, total; };
// staged (channel-last) factor copies + the appearance list behind the plain carve
struct GenStageCarve { size_t t[12], list, count, w0p, w1p, plan, x0, h0, h1, total; unsigned rows_cap; int ldx, ldh; };
constexpr long long kGenPassRows = 262144;   // list entries per pass of the matrix-core head (x0 + h0 + h1: 3.4 KB per row at 351 / 256 / 256)

// host side (t2n_generic.hip)
int gen_field(FieldDev& F, const t2n_generic_desc* d, const char* who);
int gen_fill(GenArgs& a, const t2n_generic_desc* d, const t2n_field_params* p, const char* who);
int gen_bind(GenArgs& a, const float* rays, int64_t n_rays, int ray_stride, int n_samples, uint32_t flags, const float* jitter,
             float* weights, float* z_vals, void* workspace, size_t workspace_bytes, const char* who);
GenCarve gen_carve(int64_t R, int N, bool own_wz);
GenStageCarve gen_stage_carve(const t2n_generic_desc* d, int64_t R, int N, size_t base);
size_t gen_head_lds(const t2n_generic_desc* d, bool rows_only = false);
bool gen_forward_staged(const t2n_generic_desc* d);   // the forward's predicate for its kernel form (workspace room aside)
// the staged copies, the list and its count as the forward placed them in `ws`
void gen_fast_bind(GenFast& fa, const GenArgs& a, const GenStageCarve& sc, char* ws, long long tot);
// one pass of the matrix-core head up to h1: rows [row0, row0 + rows) of the list -> x0, h0, h1 of the forward's carve (rows <= sc.rows_cap,
// a multiple of 64), by the forward's own kernels (k_gen_head_rows + two k_dense), clipped to the device-side count
int launch_gen_head_pass(const GenArgs& a, GenFast fa, const t2n_generic_desc* desc, const GenStageCarve& sc, char* ws, long long row0,
                         unsigned rows, hipStream_t s);

}  // namespace t2n
