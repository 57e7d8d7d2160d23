// TensoRF's two other parameter regularisers (models/tensoRF.py:173-191) as device kernels, beside the TV term of t2n_optim.hip:
//   density_L1          sum_k mean|density_plane[k]| + mean|density_line[k]|: per tensor T under weight w the gradient is
//                       float32(w / numel(T)) * sign(t), sign(+-0) = 0 (torch.abs's backward)
//   vector_comp_diffs   per line tensor [1,C,n,1] read as M [C,n]: D = M M^T, value = sum_{i != j} |D_ij| / (C (C - 1)),
//                       gradient = 2 / (C (C - 1)) * S M with S_ij = sign(D_ij) off the diagonal, S_ii = 0
// D and every value sum are taken in float64 from the float32 inputs, in a fixed order, without atomics (the rule of
// t2n_depth_loss.hip): sign(D_ij) of a nearly orthogonal pair is the one place where the order of a float32 sum would change a
// gradient by its whole magnitude. The products of two float32 are exact in float64, so D carries the error of its additions only.
// Two calls give the same bits. weight * 2 / (C (C - 1)) * S M is summed over j = 0 .. C - 1 in that order in both layouts and scaled in
// float64, then rounded to float32 once.
#include "t2n_device.h"

namespace t2n {

// s with the sign of v, 0 for v = +-0: on the bits, so that denormal inputs count whatever the float mode of the comparison
__device__ __forceinline__ float signed_scale(float v, float s) {
    const unsigned u = __float_as_uint(v);
    return (u << 1) == 0u ? 0.f : __uint_as_float(__float_as_uint(s) ^ (u & 0x80000000u));
}

// ---- L1, any tensor of n floats ------------------------------------------------------------------------------------------------
template <bool SET>
__global__ __launch_bounds__(256) void k_l1_grad(const float* __restrict__ x, float* __restrict__ g, long long n, float s,
                                                 const float* __restrict__ upstream) {
    const float sc = (SET && upstream) ? s * *upstream : s;
    const bool vec = ((((uintptr_t)x) | ((uintptr_t)g)) & 15u) == 0;     // (slices of a stacked tensor may start anywhere)
    const long long n4 = vec ? n / 4 : 0;
    const long long stride = (long long)gridDim.x * 256, t0 = (long long)blockIdx.x * 256 + threadIdx.x;
    const float4* __restrict__ X = reinterpret_cast<const float4*>(x);
    float4* __restrict__ G = reinterpret_cast<float4*>(g);
    for (long long i = t0; i < n4; i += stride) {
        const float4 v = X[i];
        float4 r = make_float4(signed_scale(v.x, sc), signed_scale(v.y, sc), signed_scale(v.z, sc), signed_scale(v.w, sc));
        if (!SET) { const float4 o = G[i]; r.x += o.x; r.y += o.y; r.z += o.z; r.w += o.w; }
        G[i] = r;
    }
    for (long long i = n4 * 4 + t0; i < n; i += stride) {
        const float r = signed_scale(x[i], sc);
        g[i] = SET ? r : g[i] + r;
    }
}

// mean |x| as T2N_REG_SLOTS partial sums, each already divided by n (one workgroup each, written, not added to): float64 from the
// first addition on
__global__ __launch_bounds__(256) void k_l1_value(const float* __restrict__ x, long long n, double* __restrict__ out) {
    __shared__ double part[4];
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) acc += (double)fabsf(x[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = ((part[0] + part[1]) + (part[2] + part[3])) / (double)n;
}

// ---- ortho: the Gram matrix. Element (i, k) of M at x[i * si + k * sk]: reference layout si = n, sk = 1; channel-last si = 1, sk = C
// One wave per pair i <= j: lanes stride k, partial sums folded by the xor butterfly (every lane ends with the same bits); the
// order depends on n alone, so both layouts give the same D. The upper triangle is indexed directly: row a (C - a pairs) and row
// C - 1 - a (a + 1 pairs) share one run of C + 1 waves, ceil(C / 2) such runs (gram_waves); an odd C's middle row stands alone.
__host__ __device__ __forceinline__ long long gram_waves(int C) { return (long long)((C + 1) / 2) * (C + 1); }
__device__ __forceinline__ void gram_wave(const float* __restrict__ x, long long si, long long sk, int C, int n, long long w, double* __restrict__ D) {
    if (w >= gram_waves(C)) return;
    const int a = (int)(w / (C + 1)), b = (int)(w - (long long)a * (C + 1));
    int i, j;
    if (b < C - a) { i = a; j = a + b; }
    else { i = C - 1 - a; j = i + (b - (C - a)); if (i == a) return; }     // (the middle row of an odd C: counted in the first branch)
    const int lane = threadIdx.x & 63;
    const float* __restrict__ xi = x + i * si;
    const float* __restrict__ xj = x + j * si;
    double acc = 0.0;
    for (int k = lane; k < n; k += 64) acc += (double)xi[k * sk] * (double)xj[k * sk];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) { D[(size_t)i * C + j] = acc; D[(size_t)j * C + i] = acc; }
}
__global__ __launch_bounds__(256) void k_ortho_gram(const float* __restrict__ x, int C, int n, double* __restrict__ D) {
    gram_wave(x, n, 1, C, n, (long long)blockIdx.x * 4 + (threadIdx.x >> 6), D);
}
// sum_{i != j} |D_ij| / (C (C - 1)): one workgroup, fixed order
__global__ __launch_bounds__(256) void k_ortho_value(const double* __restrict__ D, int C, double* __restrict__ out) {
    __shared__ double part[4];
    const long long cc = (long long)C * C;
    double acc = 0.0;
    for (long long e = threadIdx.x; e < cc; e += 256) {
        const long long i = e / C;
        if (e - i * C != i) acc += fabs(D[e]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = ((part[0] + part[1]) + (part[2] + part[3])) / ((double)C * (double)(C - 1));
}
// gradient element e: (a, b) = (e / n, e % n) on the reference layout, (e % C, e / C) channel-last; a pair with D_aj = 0 adds nothing
template <bool SET, bool CL>
__device__ __forceinline__ void ortho_grad_elem(const float* __restrict__ x, float* __restrict__ g, const double* __restrict__ D, int C, int n,
                                                long long e, double scale) {
    if (e >= (long long)C * n) return;
    int a, b;
    if (CL) { b = (int)(e / C); a = (int)(e - (long long)b * C); } else { a = (int)(e / n); b = (int)(e - (long long)a * n); }
    const double* __restrict__ Da = D + (size_t)a * C;
    // (sum and scale in float64, rounded to float32 once: half an ulp of the term whatever C is, so that a training step's gradients with
    // and without the term differ by the term to the roundings of the float32 additions around it)
    double acc = 0.0;
    for (int j = 0; j < C; ++j) {
        if (j == a) continue;
        const double d = Da[j];
        const double m = (double)(CL ? x[(size_t)b * C + j] : x[(size_t)j * n + b]);
        if (d > 0.0) acc += m; else if (d < 0.0) acc -= m;
    }
    const float r = (float)(scale * acc);
    g[e] = SET ? r : g[e] + r;
}
template <bool SET>
__global__ __launch_bounds__(256) void k_ortho_grad(const float* __restrict__ x, float* __restrict__ g, const double* __restrict__ D, int C, int n,
                                                    double scale, const float* __restrict__ upstream) {
    const double sc = (SET && upstream) ? scale * (double)*upstream : scale;
    ortho_grad_elem<SET, false>(x, g, D, C, n, (long long)blockIdx.x * 256 + threadIdx.x, sc);
}

// ---- the six line tensors of a field (channel-last [n][C]) in two launches: Gram, then gradient added to the gradient buffer --------
struct OrthoLines {
    const float* x[6]; float* g[6]; double* D[6];
    int C[6], n[6];
    double scale[6];
    unsigned gram0[7], grad0[7];     // first workgroup of line t in the two launches (zero-width where the weight is 0)
    const float* w_dev;              // fused training step: the two weights (density, appearance lines) of this step in device memory
};
__global__ __launch_bounds__(256) void k_ortho_gram_lines(const OrthoLines a) {
    int t = 0;
#pragma unroll 1
    for (int q = 1; q < 6; ++q) t += (a.gram0[q] <= blockIdx.x) ? 1 : 0;
    if (a.w_dev && a.w_dev[t < 3 ? 0 : 1] == 0.f) return;
    gram_wave(a.x[t], 1, a.C[t], a.C[t], a.n[t], (long long)(blockIdx.x - a.gram0[t]) * 4 + (threadIdx.x >> 6), a.D[t]);
}
__global__ __launch_bounds__(256) void k_ortho_grad_lines(const OrthoLines a) {
    int t = 0;
#pragma unroll 1
    for (int q = 1; q < 6; ++q) t += (a.grad0[q] <= blockIdx.x) ? 1 : 0;
    double scale = a.scale[t];
    if (a.w_dev) {     // the host's expression (ortho_scale), on this step's weight
        const float w = a.w_dev[t < 3 ? 0 : 1];
        if (w == 0.f) return;
        scale = (double)w * 2.0 / ((double)a.C[t] * (double)(a.C[t] - 1));
    }
    ortho_grad_elem<false, true>(a.x[t], a.g[t], a.D[t], a.C[t], a.n[t], (long long)(blockIdx.x - a.grad0[t]) * 256 + threadIdx.x, scale);
}

// the six lines' Gram matrices: allocated once by the field's first upload (t2n_api.hip), never inside a step
size_t reg_ws_bytes(const t2n_field* f) {
    const size_t Cd = (size_t)f->dev.den.C, Ca = (size_t)f->dev.app.C;
    return 3 * (Cd * Cd + Ca * Ca) * sizeof(double);
}
static double ortho_scale(float weight, int C) { return (double)weight * 2.0 / ((double)C * (double)(C - 1)); }
static bool ortho_shape_ok(int C, int n) { return C >= 2 && n >= 1 && (gram_waves(C) + 3) / 4 < 0x7fffffffll && ((long long)C * n + 255) / 256 < 0x7fffffffll; }

// g of the six lines += ortho gradient of the field's channel-last line copies (w_dev: both weights from device memory, else by value; a
// zero weight leaves its three lines out of both launches). D lives in a buffer the field owns (61 KB at 16 + 48 components).
int launch_ortho_lines(t2n_field* f, float w_den, float w_app, const float* w_dev, hipStream_t s) {
    const int* gr = f->desc.grid;
    const int Cd = f->dev.den.C, Ca = f->dev.app.C;
    if (Cd < 2 || Ca < 2) { set_error("ortho term: needs at least two components per line tensor"); return T2N_ERR_INVALID; }
    if (!f->reg_ws || f->reg_ws_bytes < reg_ws_bytes(f)) { set_error("ortho term: the field holds no Gram buffer for %d + %d components (allocated by t2n_field_upload)", Cd, Ca); return T2N_ERR_STATE; }
    OrthoLines A;
    memset(&A, 0, sizeof(A));
    unsigned gb = 0, rb = 0;
    double* D = (double*)f->reg_ws;
    for (int q = 0; q < 2; ++q)
        for (int k = 0; k < 3; ++k) {
            const int t = q * 3 + k, C = q ? Ca : Cd, n = gr[vecm(k)];
            const float w = q ? w_app : w_den;
            A.x[t] = q ? f->buf_app_line[k] : f->buf_den_line[k];
            A.g[t] = q ? f->gbuf_app_line[k] : f->gbuf_den_line[k];
            A.D[t] = D; D += (size_t)C * C;
            A.C[t] = C; A.n[t] = n; A.scale[t] = ortho_scale(w, C);
            A.gram0[t] = gb; A.grad0[t] = rb;
            if (w_dev || w != 0.f) { gb += (unsigned)((gram_waves(C) + 3) / 4); rb += (unsigned)(((long long)C * n + 255) / 256); }
        }
    A.gram0[6] = gb; A.grad0[6] = rb; A.w_dev = w_dev;
    if (!gb) return T2N_OK;
    hipLaunchKernelGGL(k_ortho_gram_lines, dim3(gb), dim3(256), 0, s, A);
    hipLaunchKernelGGL(k_ortho_grad_lines, dim3(rb), dim3(256), 0, s, A);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

}  // namespace t2n

using namespace t2n;

static unsigned l1_blocks(int64_t n) { const long long b = (n / 4 + 255) / 256; return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b)); }

extern "C" int t2n_l1_value(const float* param, int64_t n, double* sums, t2n_stream stream) {
    if (!param || !sums || n < 1) { set_error("t2n_l1_value: bad argument"); return T2N_ERR_INVALID; }
    hipLaunchKernelGGL(k_l1_value, dim3(T2N_REG_SLOTS), dim3(256), 0, (hipStream_t)stream, param, (long long)n, sums);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" int t2n_l1_grad_add(const float* param, float* grad, int64_t n, float weight, t2n_stream stream) {
    if (!param || !grad || n < 1) { set_error("t2n_l1_grad_add: bad argument"); return T2N_ERR_INVALID; }
    hipLaunchKernelGGL(k_l1_grad<false>, dim3(l1_blocks(n)), dim3(256), 0, (hipStream_t)stream, param, grad, (long long)n,
                       (float)((double)weight / (double)n), (const float*)nullptr);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" int t2n_l1_grad_set(const float* param, float* grad, int64_t n, float weight, const float* upstream, t2n_stream stream) {
    if (!param || !grad || n < 1) { set_error("t2n_l1_grad_set: bad argument"); return T2N_ERR_INVALID; }
    hipLaunchKernelGGL(k_l1_grad<true>, dim3(l1_blocks(n)), dim3(256), 0, (hipStream_t)stream, param, grad, (long long)n,
                       (float)((double)weight / (double)n), upstream);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" size_t t2n_ortho_workspace_bytes(int C) { return C < 2 ? 0 : (size_t)C * (size_t)C * sizeof(double); }

static int ortho_gram(const char* who, const float* param, int C, int64_t n, void* ws, size_t ws_bytes, hipStream_t s) {
    if (!param || !ws || C < 2 || n < 1 || n > 0x7fffffff || (((uintptr_t)ws) & 7u)) { set_error("%s: bad argument (C >= 2, n >= 1, an 8-byte aligned workspace)", who); return T2N_ERR_INVALID; }
    if (!ortho_shape_ok(C, (int)n)) { set_error("%s: C %d x n %lld out of range", who, C, (long long)n); return T2N_ERR_UNSUPPORTED; }
    if (ws_bytes < t2n_ortho_workspace_bytes(C)) { set_error("%s: workspace %zu B < %zu B", who, ws_bytes, t2n_ortho_workspace_bytes(C)); return T2N_ERR_WORKSPACE; }
    hipLaunchKernelGGL(k_ortho_gram, dim3((unsigned)((gram_waves(C) + 3) / 4)), dim3(256), 0, s, param, C, (int)n, (double*)ws);
    return T2N_OK;
}

extern "C" int t2n_ortho_value(const float* param, int C, int64_t n, double* value, void* workspace, size_t workspace_bytes, t2n_stream stream) {
    if (!value) { set_error("t2n_ortho_value: bad argument"); return T2N_ERR_INVALID; }
    int rc;
    if ((rc = ortho_gram("t2n_ortho_value", param, C, n, workspace, workspace_bytes, (hipStream_t)stream))) return rc;
    hipLaunchKernelGGL(k_ortho_value, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, C, value);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" int t2n_ortho_grad_add(const float* param, float* grad, int C, int64_t n, float weight, void* workspace, size_t workspace_bytes,
                                  t2n_stream stream) {
    if (!grad) { set_error("t2n_ortho_grad_add: bad argument"); return T2N_ERR_INVALID; }
    int rc;
    if ((rc = ortho_gram("t2n_ortho_grad_add", param, C, n, workspace, workspace_bytes, (hipStream_t)stream))) return rc;
    hipLaunchKernelGGL(k_ortho_grad<false>, dim3((unsigned)(((long long)C * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, param, grad,
                       (const double*)workspace, C, (int)n, ortho_scale(weight, C), (const float*)nullptr);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" int t2n_ortho_grad_set(const float* param, float* grad, int C, int64_t n, float weight, const float* upstream, void* workspace,
                                  size_t workspace_bytes, t2n_stream stream) {
    if (!grad) { set_error("t2n_ortho_grad_set: bad argument"); return T2N_ERR_INVALID; }
    int rc;
    if ((rc = ortho_gram("t2n_ortho_grad_set", param, C, n, workspace, workspace_bytes, (hipStream_t)stream))) return rc;
    hipLaunchKernelGGL(k_ortho_grad<true>, dim3((unsigned)(((long long)C * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, param, grad,
                       (const double*)workspace, C, (int)n, ortho_scale(weight, C), upstream);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}
