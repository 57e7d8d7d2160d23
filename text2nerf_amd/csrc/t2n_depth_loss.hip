// ---- the reference's other depth losses (utils.py:301-342) as the depth term of the driver's loss ---------------------------------------
// kind 1 "gnll":   compute_depth_loss (:306-320) with is_not_in_expected_distribution (:301-304): |mean over the K applying rays of
//                  1/2 (log v + (mu - y)^2 / v)|, var = sum_n (z - mu)^2 w + 1e-8, v = max(var, 1e-3) (nn.GaussianNLLLoss(eps=0.001)),
//                  a ray applies when |mu - y| - std > 0 or std^2 < var.
// kind 2 "si_log": compute_depth_loss_scale_invariant (:324-331): mean |d + alpha|, d = log mu - log y, alpha = -mean d.
// kind 3 "ssi":    scale_shift_invariant_loss (:333-342): the weighted least-squares fit y ~ s z + t over all R x N samples (upstream:
//                  statsmodels on the host, every step), then mean(w (s z + t - y)^2); the gradient goes to the weights alone.
// Laid out like t2n_loss.hip: one wave per ray, four rays per workgroup, per-workgroup partial sums, ONE finishing workgroup that adds
// them in a fixed order, no atomics: two calls give the same bits. Three launches:
//   pass 1  per ray: (full form) the rgb error, d_rgb and the masked transmittance mean of k_train_loss, and the kind's statistics;
//   finish  the scalars that couple the rays, all on the device: K and the signed mean NLL | alpha, mean sign | s, t (2 x 2 normal
//           equations); the four reported losses; aux;
//   pass 2  per ray: d_depth, and d_weights = transmittance term + depth term, written once (exact zeros where neither contributes).
// Precision: everything of the depth term is float64 from the first operation (the moments of ssi cancel in S0 S2 - S1^2; what the
// float64 arithmetic costs against a float32 form was not measured: no float32 form was built); the rgb and transmittance terms keep
// k_train_loss's float32 arithmetic. weights is read once and z_vals twice per call.
#include "t2n_device.h"

namespace t2n {
namespace {
constexpr int DL_SLOTS = 8;      // doubles per workgroup partial: e_rgb, e_trans, then up to six of the kind's
constexpr int DL_RAY = 3;        // doubles per ray kept between the passes: m_r, then two of the kind's
constexpr int DL_FIN = 8;        // doubles the finish leaves for pass 2

struct DepthLossArgs {
    const float* rgb; const float* depth; const float* w; const float* z; const float* rgb_t; const float* depth_t;
    long long R; int N; float w_depth, w_trans, delta; double sigma;
    float* d_rgb; float* d_depth; float* d_w; float* losses; double* aux;
    double* part; double* ray; double* fin; unsigned nblocks;
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ bool gnll_applies(double e, double var, double sigma) { return (fabs(e) - sigma > 0.0) || (sigma * sigma < var); }

// FULL: the driver's whole loss (t2n_train_loss_ex: rgb + depth term + transmittance, NaN depths count as 0); else the depth term alone.
template <int KIND, bool FULL>
__global__ __launch_bounds__(256) void k_depth_loss_rays(const DepthLossArgs a) {
    __shared__ double red[4][DL_SLOTS];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long long r = (long long)blockIdx.x * 4 + wid;
    double s[DL_SLOTS];
#pragma unroll
    for (int i = 0; i < DL_SLOTS; ++i) s[i] = 0.0;
    if (r < a.R) {
        const float dt = a.depth_t[r];
        const float* wr = a.w ? a.w + r * a.N : nullptr;
        const float* zr = a.z ? a.z + r * a.N : nullptr;
        float dep = a.depth ? a.depth[r] : 0.f;      // (ssi has no depth input)
        if (FULL && dep != dep) dep = 0.f;
        const double mu = (double)dep, y = (double)dt;
        float m = 0.f;
        double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0, q4 = 0.0, q5 = 0.0;
        if (FULL || KIND != 2) {
            for (int n = lane; n < a.N; n += 64) {
                const float wf = wr[n], zf = zr[n];
                if (FULL) m += ((zf - dt) + a.delta < 0.f) ? wf : 0.f;
                const double wd = (double)wf, zd = (double)zf;
                if (KIND == 1) {
                    const double dz = zd - mu;
                    q0 += (dz * dz) * wd;
                    q1 += dz * wd;
                } else if (KIND == 3) {
                    const double wz = wd * zd;
                    q0 += wd; q1 += wz; q2 += wz * zd; q3 += wd * y; q4 += wz * y; q5 += (wd * y) * y;
                }
            }
        }
        double* ray = a.ray + r * DL_RAY;
        if (FULL) {
            m = wave_sum(m) / (float)a.N;
            float e_rgb = 0.f;
            if (lane < 3) {
                const float d = a.rgb[r * 3 + lane] - a.rgb_t[r * 3 + lane];
                a.d_rgb[r * 3 + lane] = 2.f * d / (3.f * (float)a.R);
                e_rgb = d * d;
            }
            s[0] = (double)wave_sum(e_rgb);
            s[1] = (double)(m * m);
            if (lane == 0) ray[0] = (double)m;
        }
        if (KIND == 1) {
            const double var = wave_sum_f64(q0) + 1e-8, c = wave_sum_f64(q1), e = mu - y;
            if (gnll_applies(e, var, a.sigma)) {
                const double v = fmax(var, 1e-3);
                s[2] = 1.0;
                s[3] = 0.5 * (log(v) + (e * e) / v);
            }
            if (lane == 0) { ray[1] = var; ray[2] = c; }
        } else if (KIND == 2) {
            const double d = log(mu) - log(y);
            s[2] = d;
            if (lane == 0) ray[1] = d;
        } else {
            s[2] = wave_sum_f64(q0); s[3] = wave_sum_f64(q1); s[4] = wave_sum_f64(q2);
            s[5] = wave_sum_f64(q3); s[6] = wave_sum_f64(q4); s[7] = wave_sum_f64(q5);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < DL_SLOTS; ++i) red[wid][i] = s[i];
    }
    __syncthreads();
    if (threadIdx.x < DL_SLOTS)
        a.part[(size_t)blockIdx.x * DL_SLOTS + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// sum of `v` over the 256 threads of the workgroup in a fixed order; every thread gets the result
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

template <int KIND, bool FULL>
__global__ __launch_bounds__(256) void k_depth_loss_finish(const DepthLossArgs a) {
    __shared__ double red[256];
    double S[DL_SLOTS];
#pragma unroll
    for (int i = 0; i < DL_SLOTS; ++i) {
        double v = 0.0;
        for (unsigned b = threadIdx.x; b < a.nblocks; b += 256) v += a.part[(size_t)b * DL_SLOTS + i];
        S[i] = block_sum_f64(v, red);
    }
    const double Rd = (double)a.R;
    double term = 0.0, f0 = 0.0, f1 = 0.0, x0 = 0.0, x1 = 0.0;      // the depth term, two scalars for pass 2, two for aux
    if (KIND == 1) {
        const double K = S[2], mean = K > 0.0 ? S[3] / K : 0.0;
        term = fabs(mean);
        f0 = K > 0.0 ? (mean > 0.0 ? 1.0 : (mean < 0.0 ? -1.0 : 0.0)) / K : 0.0;      // g: d|mean| / d(a ray's term)
        x0 = K; x1 = mean;
    } else if (KIND == 2) {
        const double alpha = -(S[2] / Rd);
        double l = 0.0, sg = 0.0;
        for (long long r = threadIdx.x; r < a.R; r += 256) {
            const double u = a.ray[r * DL_RAY + 1] + alpha;
            l += fabs(u);
            sg += u > 0.0 ? 1.0 : (u < 0.0 ? -1.0 : 0.0);
        }
        l = block_sum_f64(l, red);
        sg = block_sum_f64(sg, red);
        term = l / Rd;
        f0 = alpha; f1 = sg / Rd;
        x0 = alpha;
    } else {
        // y ~ s z + t by weighted least squares; rank-deficient systems follow the pseudo-inverse (statsmodels' default fit)
        const double S0 = S[2], S1 = S[3], S2 = S[4], Sy = S[5], Szy = S[6], Syy = S[7];
        double sc = 0.0, sh = 0.0;
        if (S0 > 0.0) {
            const double zb = S1 / S0, yb = Sy / S0, varz = S2 / S0 - zb * zb;
            if (varz <= 1e-12 * (S2 / S0)) {
                sh = yb / (1.0 + zb * zb);
                sc = sh * zb;
            } else {
                sc = (Szy / S0 - zb * yb) / varz;
                sh = yb - sc * zb;
            }
        }
        x0 = sc; x1 = sh;
        f0 = (double)(float)sc; f1 = (double)(float)sh;       // upstream multiplies float32 tensors by s and t
        term = ((f0 * f0) * S2 + 2.0 * (f0 * f1) * S1 + (f1 * f1) * S0 - 2.0 * f0 * Szy - 2.0 * f1 * Sy + Syy) / (Rd * (double)a.N);
        if (term < 0.0) term = 0.0;
    }
    if (threadIdx.x == 0) {
        a.fin[0] = f0; a.fin[1] = f1;
        a.aux[0] = x0; a.aux[1] = x1; a.aux[2] = 0.0; a.aux[3] = 0.0;
        if (FULL) {
            const float mse = (float)(S[0] / (3.0 * Rd)), dl = (float)term, tl = (float)(S[1] / Rd);
            a.losses[0] = mse; a.losses[1] = dl; a.losses[2] = tl; a.losses[3] = mse + a.w_depth * dl + a.w_trans * tl;
        } else {
            a.losses[0] = (float)term;
        }
    }
}

template <int KIND, bool FULL>
__global__ __launch_bounds__(256) void k_depth_loss_grads(const DepthLossArgs a) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long long r = (long long)blockIdx.x * 4 + wid;
    if (r >= a.R) return;
    const float dt = a.depth_t[r];
    float dep = a.depth ? a.depth[r] : 0.f;      // (ssi has no depth input)
    const bool bad = FULL && dep != dep;
    if (bad) dep = 0.f;
    const double mu = (double)dep, y = (double)dt, up = FULL ? (double)a.w_depth : 1.0;
    const double f0 = a.fin[0], f1 = a.fin[1];
    const double* ray = a.ray + r * DL_RAY;
    float gw = 0.f;
    if (FULL) gw = (2.f * a.w_trans * (float)ray[0] / (float)a.R) / (float)a.N;
    double dd = 0.0, dv = 0.0;
    if (KIND == 1) {
        const double var = ray[1], c = ray[2], e = mu - y;
        if (gnll_applies(e, var, a.sigma)) {
            const double v = fmax(var, 1e-3);
            dv = 0.5 * f0 * (1.0 / v - (e * e) / (v * v));       // the clamp passes the gradient through, evaluated at v
            dd = f0 * e / v - 2.0 * dv * c;
        }
    } else if (KIND == 2) {
        const double u = ray[1] + f0;
        dd = ((u > 0.0 ? 1.0 : (u < 0.0 ? -1.0 : 0.0)) - f1) / ((double)a.R * mu);
    }
    if (a.d_depth && lane == 0) a.d_depth[r] = bad ? 0.f : (float)(up * dd);
    if (!a.d_w) return;
    float* dwr = a.d_w + r * a.N;
    const float* zr = a.z ? a.z + r * a.N : nullptr;
    const double inv_rn = 1.0 / ((double)a.R * (double)a.N);
    for (int n = lane; n < a.N; n += 64) {
        float g = 0.f;
        double t = 0.0;
        if (FULL || KIND != 2) {
            const float zf = zr[n];
            if (FULL) g = ((zf - dt) + a.delta < 0.f) ? gw : 0.f;
            if (KIND == 1) {
                const double dz = (double)zf - mu;
                t = dv * (dz * dz);
            } else if (KIND == 3) {
                const double res = (f0 * (double)zf + f1) - y;
                t = (res * res) * inv_rn;
            }
        }
        dwr[n] = FULL ? g + (float)(up * t) : (float)t;
    }
}

template <int KIND, bool FULL>
int launch_depth_loss_kind(const DepthLossArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((k_depth_loss_rays<KIND, FULL>), dim3(a.nblocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL((k_depth_loss_finish<KIND, FULL>), dim3(1), dim3(256), 0, s, a);
    if (a.d_depth || a.d_w) hipLaunchKernelGGL((k_depth_loss_grads<KIND, FULL>), dim3(a.nblocks), dim3(256), 0, s, a);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}
template <bool FULL>
int launch_depth_loss(int kind, const DepthLossArgs& a, hipStream_t s) {
    return kind == 1 ? launch_depth_loss_kind<1, FULL>(a, s) : kind == 2 ? launch_depth_loss_kind<2, FULL>(a, s) : launch_depth_loss_kind<3, FULL>(a, s);
}
size_t depth_loss_doubles(int64_t n_rays) { return (size_t)((n_rays + 3) / 4) * DL_SLOTS + (size_t)n_rays * DL_RAY + DL_FIN; }
void carve(DepthLossArgs& a, void* workspace) {
    a.nblocks = (unsigned)((a.R + 3) / 4);
    a.part = (double*)workspace;
    a.ray = a.part + (size_t)a.nblocks * DL_SLOTS;
    a.fin = a.ray + (size_t)a.R * DL_RAY;
}
}  // namespace
}  // namespace t2n

using namespace t2n;

extern "C" size_t t2n_train_loss_ex_workspace_bytes(int64_t n_rays) {
    if (n_rays <= 0) return 0;
    const size_t own = depth_loss_doubles(n_rays) * sizeof(double), base = t2n_train_loss_workspace_bytes(n_rays);
    return own > base ? own : base;
}

extern "C" int t2n_train_loss_ex(const float* rgb, const float* depth, const float* weights, const float* z_vals, const float* rgb_t,
                                 const float* depth_t, int64_t n_rays, int n_samples, float w_depth, float w_trans, float delta,
                                 int depth_kind, float target_std, float* d_rgb, float* d_depth, float* d_weights, float* losses, double* aux,
                                 void* workspace, size_t workspace_bytes, t2n_stream stream) {
    if (!rgb || !depth || !weights || !z_vals || !rgb_t || !depth_t || !d_rgb || !d_depth || !d_weights || !losses || !aux || !workspace ||
        n_rays <= 0 || n_samples <= 0) {
        set_error("t2n_train_loss_ex: bad argument");
        return T2N_ERR_INVALID;
    }
    if (depth_kind < 0 || depth_kind > 3) { set_error("t2n_train_loss_ex: depth_kind %d is none of 0 (mse), 1 (gnll), 2 (si_log), 3 (ssi)", depth_kind); return T2N_ERR_INVALID; }
    if (depth_kind == 1 && !(target_std > 0.f)) { set_error("t2n_train_loss_ex: gnll needs target_std > 0"); return T2N_ERR_INVALID; }
    if (((uintptr_t)workspace & 7) != 0) { set_error("t2n_train_loss_ex: the workspace must be 8-byte aligned"); return T2N_ERR_INVALID; }
    if (workspace_bytes < t2n_train_loss_ex_workspace_bytes(n_rays)) { set_error("t2n_train_loss_ex: workspace too small"); return T2N_ERR_WORKSPACE; }
    if (depth_kind == 0) {
        // today's loss: the same kernels on the same arguments (bit-equal outputs); aux has nothing to report
        T2N_HIP(hipMemsetAsync(aux, 0, 4 * sizeof(double), (hipStream_t)stream));
        return t2n_train_loss(rgb, depth, weights, z_vals, rgb_t, depth_t, n_rays, n_samples, w_depth, w_trans, delta, d_rgb, d_depth, d_weights,
                              losses, workspace, workspace_bytes, stream);
    }
    DepthLossArgs a;
    a.rgb = rgb; a.depth = depth; a.w = weights; a.z = z_vals; a.rgb_t = rgb_t; a.depth_t = depth_t; a.R = n_rays; a.N = n_samples;
    a.w_depth = w_depth; a.w_trans = w_trans; a.delta = delta; a.sigma = (double)target_std;
    a.d_rgb = d_rgb; a.d_depth = d_depth; a.d_w = d_weights; a.losses = losses; a.aux = aux;
    carve(a, workspace);
    return launch_depth_loss<true>(depth_kind, a, (hipStream_t)stream);
}

extern "C" size_t t2n_depth_loss_workspace_bytes(int64_t n_rays) { return n_rays > 0 ? depth_loss_doubles(n_rays) * sizeof(double) : 0; }

extern "C" int t2n_depth_loss(int kind, const float* depth, const float* weights, const float* z_vals, const float* depth_t, int64_t n_rays,
                              int n_samples, float target_std, float* loss, double* aux, float* d_depth, float* d_weights, void* workspace,
                              size_t workspace_bytes, t2n_stream stream) {
    if (kind < 1 || kind > 3) { set_error("t2n_depth_loss: kind %d is none of 1 (gnll), 2 (si_log), 3 (ssi)", kind); return T2N_ERR_INVALID; }
    if ((!depth && kind != 3) || !depth_t || !loss || !aux || !workspace || n_rays <= 0 || n_samples <= 0 || (kind != 2 && (!weights || !z_vals))) {
        set_error("t2n_depth_loss: bad argument");
        return T2N_ERR_INVALID;
    }
    if (kind == 1 && !(target_std > 0.f)) { set_error("t2n_depth_loss: gnll needs target_std > 0"); return T2N_ERR_INVALID; }
    if (((uintptr_t)workspace & 7) != 0) { set_error("t2n_depth_loss: the workspace must be 8-byte aligned"); return T2N_ERR_INVALID; }
    if (workspace_bytes < t2n_depth_loss_workspace_bytes(n_rays)) { set_error("t2n_depth_loss: workspace too small"); return T2N_ERR_WORKSPACE; }
    DepthLossArgs a;
    a.rgb = nullptr; a.depth = depth; a.w = kind == 2 ? nullptr : weights; a.z = kind == 2 ? nullptr : z_vals; a.rgb_t = nullptr; a.depth_t = depth_t;
    a.R = n_rays; a.N = n_samples; a.w_depth = 1.f; a.w_trans = 0.f; a.delta = 0.f; a.sigma = (double)target_std;
    a.d_rgb = nullptr; a.d_depth = d_depth; a.d_w = d_weights; a.losses = loss; a.aux = aux;
    carve(a, workspace);
    return launch_depth_loss<false>(kind, a, (hipStream_t)stream);
}
