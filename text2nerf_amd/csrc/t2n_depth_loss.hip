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
//
// ---- the distortion regulariser on a ray's weights (mip-NeRF 360, eq. 15; the reference has no such term) -------------------------------
// Per ray, with rho = inv_range, dz_n = z[n+1] - z[n] (0 for the last sample), delta_n = dz_n rho, m_n = ((z[n] - z[0]) + dz_n / 2) rho:
//   L_r = sum_i sum_j w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 delta_i,   dL_r/dw_i = 2 sum_j w_j |m_i - m_j| + 2/3 w_i delta_i,   D = mean_r L_r,
// in O(N) by the sorted-order identity (z_vals ascend along a ray): with the exclusive prefix sums W, WM of w and w m,
//   sum_j w_j |m_i - m_j| = (m_i W_<i - WM_<i) + (WM_>i - m_i W_>i),   suffix = total - prefix - self,   sum_i sum_j = 2 sum_i w_i (m_i W_<i - WM_<i).
// Same mapping (wave per ray, four rays per workgroup, lanes strided over the samples); the prefix sums run over tiles of 64 consecutive
// samples: a wave inclusive scan of the pair (w, w m) by DPP (row shifts and row broadcasts: VALU moves, no LDS crossbar) plus a
// running carry. z[n+1] is a second, still coalesced load. float64 from the first operation (z[n+1] - z[n] and z[n] - z[0] are exact), fixed order, no atomics; the stored gradient and
// the reported loss are rounded to float32 once.
//   t2n_distortion_loss: ONE pass (per ray: the two totals by plain wave sums, then one scan that gives L_r and the gradient; the ray's
//                        2 N floats were just read by the same wave) + the finishing workgroup.
//   t2n_train_loss_dist: kind 0: k_train_loss's arithmetic with the same totals + one scan inside its pass, then its reduce; kinds 1..3: the
//                        scan for L_r rides in pass 1, the finish adds up D, the gradient scan rides in pass 2, where d_weights is
//                        written once as float32(old value + w_dist / R dL_r/dw). The same launch counts as without the term.
//   Kinds 1..3: the ray's two totals (sum w, sum w m) travel from pass 1 to pass 2 in two ray slots of their own (DIST_RAY, 16 B per
//   ray) instead of being recomputed in pass 2 (-DT2N_DIST_RECOMPUTE_TOTALS: one more read of the ray's 2 N floats). Measured at
//   16 384 x 259 (profiles/distortion_timing.txt): kept 80.4 / 98.5 / 82.5 us per call for gnll / si_log / ssi, recomputed 87.7 / 105.7 /
//   89.6 us. The __shfl_up form of the scan (ds_bpermute) with two scans per ray cost 57 us over t2n_train_loss_ex where this one costs 27.
#include "t2n_device.h"

namespace t2n {
namespace {
constexpr int DL_SLOTS = 8;      // doubles per workgroup partial: e_rgb, e_trans, then up to six of the kind's
constexpr int DL_RAY = 3;        // doubles per ray kept between the passes: m_r, then two of the kind's
constexpr int DL_FIN = 8;        // doubles the finish leaves for pass 2
constexpr int DIST_RAY = 2;      // doubles per ray of the distortion term between the passes: sum w, sum w m

struct DepthLossArgs {
    const float* rgb; const float* depth; const float* w; const float* z; const float* rgb_t; const float* depth_t;
    long long R; int N; float w_depth, w_trans, delta; double sigma;
    float* d_rgb; float* d_depth; float* d_w; float* losses; double* aux;
    double* part; double* ray; double* fin; unsigned nblocks;
    // the distortion term (DIST kernels only): weight, 1 / z_range, w_dist / R (1 / R for the term alone), per-workgroup partial sums of
    // L_r, the ray slots, D (device double, may be NULL), the term alone: its float32 loss (may be NULL); kind 0: k_train_loss's partials
    double w_dist, rho, gscale; double* dpart; double* dray; double* dist; float* dist_f; float* fpart;
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ bool gnll_applies(double e, double var, double sigma) { return (fabs(e) - sigma > 0.0) || (sigma * sigma < var); }

// ---- distortion term: one tile of 64 consecutive samples of a ray ----------------------------------------------------------------------
// A double moved across lanes by DPP (two 32-bit moves, VALU; no LDS crossbar as __shfl_up's ds_bpermute takes): 0.0 arrives where the
// control names no source lane or the row mask excludes the row, so `v += dpp_f64<...>(v)` leaves those lanes as they are.
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ double dpp_f64(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROW_MASK, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}
// inclusive sum scan over the 64 lanes (lane 0 first): row_shr 1, 2, 4, 8 inside each row of 16, then row_bcast15 into rows 1 and 3,
// row_bcast31 into rows 2 and 3. A fixed order.
__device__ __forceinline__ double wave_scan_add_f64(double v) {
    v += dpp_f64<0x111>(v);
    v += dpp_f64<0x112>(v);
    v += dpp_f64<0x114>(v);
    v += dpp_f64<0x118>(v);
    v += dpp_f64<0x142, 0xa>(v);
    v += dpp_f64<0x143, 0xc>(v);
    return v;
}
__device__ __forceinline__ double lane63_f64(double v) {       // (wave-uniform: a scalar register pair)
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)b, 63), hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), 63);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// This lane's sample n = base + lane (w = 0 past the ray's end) and its exclusive prefix sums over the whole ray so far; the carries
// advance by the tile's sums. Called by all 64 lanes of the wave.
struct DistTile { double w, m, delta, W_lt, WM_lt; };
struct DistCarry { double W, WM; };
__device__ __forceinline__ void dist_sample(const float* __restrict__ wr, const float* __restrict__ zr, int N, int n, double z0, double rho,
                                            double& w, double& m, double& delta) {
    const double zn = (double)zr[n];
    const double dz = n + 1 < N ? (double)zr[n + 1] - zn : 0.0;
    w = (double)wr[n];
    delta = dz * rho;
    m = ((zn - z0) + dz * 0.5) * rho;
}
__device__ __forceinline__ DistTile dist_tile(const float* __restrict__ wr, const float* __restrict__ zr, int N, int base, int lane, double z0,
                                              double rho, DistCarry& c) {
    DistTile t;
    t.w = 0.0; t.m = 0.0; t.delta = 0.0;
    const int n = base + lane;
    if (n < N) dist_sample(wr, zr, N, n, z0, rho, t.w, t.m, t.delta);
    const double iw = wave_scan_add_f64(t.w), iwm = wave_scan_add_f64(t.w * t.m);
    t.W_lt = c.W + dpp_f64<0x138>(iw);           // wave_shr 1: the inclusive sums one lane down, 0 into lane 0
    t.WM_lt = c.WM + dpp_f64<0x138>(iwm);
    c.W += lane63_f64(iw);
    c.WM += lane63_f64(iwm);
    return t;
}
// this lane's share of L_r's two sums
__device__ __forceinline__ void dist_loss_terms(const DistTile& t, double& cross, double& self) {
    cross += t.w * (t.m * t.W_lt - t.WM_lt);
    self += (t.w * t.w) * t.delta;
}
__device__ __forceinline__ double dist_loss_value(double cross, double self) { return 2.0 * wave_sum_f64(cross) + wave_sum_f64(self) / 3.0; }
// L_r of one ray (every lane gets it); `tot` leaves with the ray's totals sum w, sum w m
__device__ __forceinline__ double dist_ray_loss(const float* __restrict__ wr, const float* __restrict__ zr, int N, int lane, double rho, DistCarry& tot) {
    const double z0 = (double)zr[0];
    tot.W = 0.0; tot.WM = 0.0;
    double cross = 0.0, self = 0.0;
    for (int base = 0; base < N; base += 64) {
        const DistTile t = dist_tile(wr, zr, N, base, lane, z0, rho, tot);
        dist_loss_terms(t, cross, self);
    }
    return dist_loss_value(cross, self);
}
// the ray's totals alone: lanes strided over the samples, one wave sum each (no scan)
__device__ __forceinline__ DistCarry dist_ray_totals(const float* __restrict__ wr, const float* __restrict__ zr, int N, int lane, double rho) {
    const double z0 = (double)zr[0];
    double sw = 0.0, swm = 0.0;
    for (int n = lane; n < N; n += 64) {
        double w, m, delta;
        dist_sample(wr, zr, N, n, z0, rho, w, m, delta);
        sw += w;
        swm += w * m;
    }
    return DistCarry{wave_sum_f64(sw), wave_sum_f64(swm)};
}
// dL_r/dw of this lane's sample of a tile, given the ray's totals
__device__ __forceinline__ double dist_grad(const DistTile& t, const DistCarry& tot) {
    const double wm = t.w * t.m;
    const double before = t.m * t.W_lt - t.WM_lt;
    const double after = ((tot.WM - t.WM_lt) - wm) - t.m * ((tot.W - t.W_lt) - t.w);
    return 2.0 * (before + after) + ((2.0 / 3.0) * t.w) * t.delta;
}
// L_r and the gradient of one ray in ONE scan (the totals first, by dist_ray_totals): store(n, dL_r/dw_n) for every sample
template <class Store>
__device__ __forceinline__ double dist_ray_loss_and_grad(const float* __restrict__ wr, const float* __restrict__ zr, int N, int lane, double rho,
                                                         Store store) {
    const DistCarry tot = dist_ray_totals(wr, zr, N, lane, rho);
    const double z0 = (double)zr[0];
    DistCarry c{0.0, 0.0};
    double cross = 0.0, self = 0.0;
    for (int base = 0; base < N; base += 64) {
        const DistTile t = dist_tile(wr, zr, N, base, lane, z0, rho, c);
        dist_loss_terms(t, cross, self);
        if (base + lane < N) store(base + lane, dist_grad(t, tot));
    }
    return dist_loss_value(cross, self);
}

// FULL: the driver's whole loss (t2n_train_loss_ex: rgb + depth term + transmittance, NaN depths count as 0); else the depth term alone.
// DIST (FULL only): the distortion term rides along (t2n_train_loss_dist).
template <int KIND, bool FULL, bool DIST = false>
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
    if constexpr (DIST) {
        __shared__ double dred[4];
        double L = 0.0;
        if (r < a.R) {
            DistCarry tot;
            L = dist_ray_loss(a.w + r * a.N, a.z + r * a.N, a.N, lane, a.rho, tot);
            if (lane == 0) { a.dray[r * DIST_RAY] = tot.W; a.dray[r * DIST_RAY + 1] = tot.WM; }
        }
        if (lane == 0) dred[wid] = L;
        __syncthreads();
        if (threadIdx.x == 0) a.dpart[blockIdx.x] = (dred[0] + dred[1]) + (dred[2] + dred[3]);
    } else {
        __syncthreads();
    }
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

// D = mean_r L_r from the per-workgroup partial sums (every thread gets it)
__device__ __forceinline__ double dist_mean(const DepthLossArgs& a, double* red) {
    double v = 0.0;
    for (unsigned b = threadIdx.x; b < a.nblocks; b += 256) v += a.dpart[b];
    return block_sum_f64(v, red) / (double)a.R;
}

template <int KIND, bool FULL, bool DIST = false>
__global__ __launch_bounds__(256) void k_depth_loss_finish(const DepthLossArgs a) {
    __shared__ double red[256];
    double S[DL_SLOTS];
#pragma unroll
    for (int i = 0; i < DL_SLOTS; ++i) {
        double v = 0.0;
        for (unsigned b = threadIdx.x; b < a.nblocks; b += 256) v += a.part[(size_t)b * DL_SLOTS + i];
        S[i] = block_sum_f64(v, red);
    }
    double D = 0.0;
    if constexpr (DIST) D = dist_mean(a, red);
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
            if constexpr (DIST) {
                a.losses[3] = (float)((double)(mse + a.w_depth * dl + a.w_trans * tl) + a.w_dist * D);
                a.dist[0] = D;
            }
        } else {
            a.losses[0] = (float)term;
        }
    }
}

template <int KIND, bool FULL, bool DIST = false>
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
    // the value without the distortion term
    auto sample = [&](int n) -> float {
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
        return FULL ? g + (float)(up * t) : (float)t;
    };
    if constexpr (DIST) {
        const float* wr = a.w + r * a.N;
#ifdef T2N_DIST_RECOMPUTE_TOTALS      // the measured alternative (see the file header): one more read of the ray instead of the two slots
        const DistCarry tot = dist_ray_totals(wr, zr, a.N, lane, a.rho);
#else
        const DistCarry tot{a.dray[r * DIST_RAY], a.dray[r * DIST_RAY + 1]};
#endif
        const double z0 = (double)zr[0];
        DistCarry c{0.0, 0.0};
        for (int base = 0; base < a.N; base += 64) {
            const DistTile t = dist_tile(wr, zr, a.N, base, lane, z0, a.rho, c);
            const int n = base + lane;
            if (n < a.N) dwr[n] = (float)((double)sample(n) + a.gscale * dist_grad(t, tot));
        }
    } else {
        for (int n = lane; n < a.N; n += 64) dwr[n] = sample(n);
    }
}

template <int KIND, bool FULL, bool DIST = false>
int launch_depth_loss_kind(const DepthLossArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((k_depth_loss_rays<KIND, FULL, DIST>), dim3(a.nblocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL((k_depth_loss_finish<KIND, FULL, DIST>), dim3(1), dim3(256), 0, s, a);
    if (a.d_depth || a.d_w) hipLaunchKernelGGL((k_depth_loss_grads<KIND, FULL, DIST>), dim3(a.nblocks), dim3(256), 0, s, a);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}
template <bool FULL, bool DIST = false>
int launch_depth_loss(int kind, const DepthLossArgs& a, hipStream_t s) {
    return kind == 1 ? launch_depth_loss_kind<1, FULL, DIST>(a, s) : kind == 2 ? launch_depth_loss_kind<2, FULL, DIST>(a, s)
                                                                                : launch_depth_loss_kind<3, FULL, DIST>(a, s);
}
size_t depth_loss_doubles(int64_t n_rays) { return (size_t)((n_rays + 3) / 4) * DL_SLOTS + (size_t)n_rays * DL_RAY + DL_FIN; }
void carve(DepthLossArgs& a, void* workspace) {
    a.nblocks = (unsigned)((a.R + 3) / 4);
    a.part = (double*)workspace;
    a.ray = a.part + (size_t)a.nblocks * DL_SLOTS;
    a.fin = a.ray + (size_t)a.R * DL_RAY;
    a.w_dist = 0.0; a.rho = 0.0; a.gscale = 0.0;
    a.dpart = nullptr; a.dray = nullptr; a.dist = nullptr; a.dist_f = nullptr; a.fpart = nullptr;
}

// ---- the distortion term alone, and inside the driver's loss with the "mse" depth term -------------------------------------------------
// GRAD: also d_w = gscale dL_r/dw (the ray's totals stay in registers between the two scans)
template <bool GRAD>
__global__ __launch_bounds__(256) void k_distortion_rays(const DepthLossArgs a) {
    __shared__ double dred[4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long long r = (long long)blockIdx.x * 4 + wid;
    double L = 0.0;
    if (r < a.R) {
        const float* wr = a.w + r * a.N;
        const float* zr = a.z + r * a.N;
        if (GRAD) {
            float* dwr = a.d_w + r * a.N;
            L = dist_ray_loss_and_grad(wr, zr, a.N, lane, a.rho, [&](int n, double g) { dwr[n] = (float)(a.gscale * g); });
        } else {
            DistCarry tot;
            L = dist_ray_loss(wr, zr, a.N, lane, a.rho, tot);
        }
    }
    if (lane == 0) dred[wid] = L;
    __syncthreads();
    if (threadIdx.x == 0) a.dpart[blockIdx.x] = (dred[0] + dred[1]) + (dred[2] + dred[3]);
}
__global__ __launch_bounds__(256) void k_distortion_finish(const DepthLossArgs a) {
    __shared__ double red[256];
    const double D = dist_mean(a, red);
    if (threadIdx.x == 0) {
        if (a.dist) a.dist[0] = D;
        if (a.dist_f) a.dist_f[0] = (float)D;
    }
}
int launch_distortion(const DepthLossArgs& a, hipStream_t s) {
    if (a.d_w) hipLaunchKernelGGL(k_distortion_rays<true>, dim3(a.nblocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_distortion_rays<false>, dim3(a.nblocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_distortion_finish, dim3(1), dim3(256), 0, s, a);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

// k_train_loss (t2n_loss.hip) with the distortion term: the same float32 operations in the same order for everything k_train_loss
// computes (bit-equal d_rgb, d_depth, partial sums), d_w = float32(k_train_loss's value + gscale dL_r/dw), and the partial sum of L_r.
__global__ __launch_bounds__(256) void k_train_loss_dist(const DepthLossArgs a) {
    __shared__ float red[4][3];
    __shared__ double dred[4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long long r = (long long)blockIdx.x * 4 + wid;
    float e_rgb = 0.f, e_dep = 0.f, e_tr = 0.f;
    double L = 0.0;
    if (r < a.R) {
        const float dt = a.depth_t[r];
        const float* wr = a.w + r * a.N;
        const float* zr = a.z + r * a.N;
        float m = 0.f;
        for (int n = lane; n < a.N; n += 64) m += ((zr[n] - dt) + a.delta < 0.f) ? wr[n] : 0.f;
        m = wave_sum(m) / (float)a.N;
        const float gw = (2.f * a.w_trans * m / (float)a.R) / (float)a.N;
        float* dwr = a.d_w + r * a.N;
        L = dist_ray_loss_and_grad(wr, zr, a.N, lane, a.rho, [&](int n, double g) {
            const float old = ((zr[n] - dt) + a.delta < 0.f) ? gw : 0.f;
            dwr[n] = (float)((double)old + a.gscale * g);
        });
        if (lane < 3) {
            const float d = a.rgb[r * 3 + lane] - a.rgb_t[r * 3 + lane];
            a.d_rgb[r * 3 + lane] = 2.f * d / (3.f * (float)a.R);
            e_rgb = d * d;
        }
        e_rgb = wave_sum(e_rgb);
        float dep = a.depth[r];
        const bool bad = dep != dep;
        if (bad) dep = 0.f;
        const float dd = dep - dt;
        if (lane == 0) a.d_depth[r] = bad ? 0.f : 2.f * a.w_depth * dd / (float)a.R;
        e_dep = dd * dd;
        e_tr = m * m;
    }
    if (lane == 0) { red[wid][0] = e_rgb; red[wid][1] = e_dep; red[wid][2] = e_tr; dred[wid] = L; }
    __syncthreads();
    if (threadIdx.x < 3) a.fpart[(size_t)blockIdx.x * 3 + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    if (threadIdx.x == 3) a.dpart[blockIdx.x] = (dred[0] + dred[1]) + (dred[2] + dred[3]);
}
__global__ __launch_bounds__(256) void k_train_loss_dist_reduce(const DepthLossArgs a) {
    __shared__ float red[256][3];
    __shared__ double dsum[256];
    const LossReduceArgs lr{a.fpart, a.nblocks, a.losses, a.R, a.w_depth, a.w_trans};
    loss_reduce_rows(lr, red);          // k_train_loss_reduce's losses[4]; thread 0 wrote them
    const double D = dist_mean(a, dsum);
    if (threadIdx.x == 0) {
        a.losses[3] = (float)((double)a.losses[3] + a.w_dist * D);
        a.dist[0] = D;
    }
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

// ---- the distortion regulariser ---------------------------------------------------------------------------------------------------------
static size_t dist_doubles(int64_t n_rays) { return (size_t)((n_rays + 3) / 4) + (size_t)n_rays * DIST_RAY; }
static bool positive_finite(double v) { return v > 0.0 && v <= 1.79769313486231570e308; }

extern "C" size_t t2n_distortion_loss_workspace_bytes(int64_t n_rays) { return n_rays > 0 ? (size_t)((n_rays + 3) / 4) * sizeof(double) : 0; }

extern "C" int t2n_distortion_loss(const float* weights, const float* z_vals, int64_t n_rays, int n_samples, float inv_range, float* loss,
                                   float* d_weights, void* workspace, size_t workspace_bytes, t2n_stream stream) {
    if (!weights || !z_vals || !loss || !workspace || n_rays <= 0 || n_samples <= 0) {
        set_error("t2n_distortion_loss: bad argument");
        return T2N_ERR_INVALID;
    }
    if (!positive_finite((double)inv_range)) { set_error("t2n_distortion_loss: inv_range must be finite and > 0"); return T2N_ERR_INVALID; }
    if (((uintptr_t)workspace & 7) != 0) { set_error("t2n_distortion_loss: the workspace must be 8-byte aligned"); return T2N_ERR_INVALID; }
    if (workspace_bytes < t2n_distortion_loss_workspace_bytes(n_rays)) { set_error("t2n_distortion_loss: workspace too small"); return T2N_ERR_WORKSPACE; }
    DepthLossArgs a;
    a.rgb = nullptr; a.depth = nullptr; a.w = weights; a.z = z_vals; a.rgb_t = nullptr; a.depth_t = nullptr; a.R = n_rays; a.N = n_samples;
    a.w_depth = 0.f; a.w_trans = 0.f; a.delta = 0.f; a.sigma = 0.0;
    a.d_rgb = nullptr; a.d_depth = nullptr; a.d_w = d_weights; a.losses = nullptr; a.aux = nullptr;
    carve(a, workspace);
    a.part = a.ray = a.fin = nullptr;
    a.dpart = (double*)workspace;
    a.w_dist = 1.0; a.rho = (double)inv_range; a.gscale = 1.0 / (double)n_rays; a.dist_f = loss;
    return launch_distortion(a, (hipStream_t)stream);
}

extern "C" size_t t2n_train_loss_dist_workspace_bytes(int64_t n_rays) {
    if (n_rays <= 0) return 0;
    return ((t2n_train_loss_ex_workspace_bytes(n_rays) + 7) & ~(size_t)7) + dist_doubles(n_rays) * sizeof(double);
}

extern "C" int t2n_train_loss_dist(const float* rgb, const float* depth, const float* weights, const float* z_vals, const float* rgb_t,
                                   const float* depth_t, int64_t n_rays, int n_samples, float w_depth, float w_trans, float delta,
                                   int depth_kind, float target_std, float w_dist, float inv_range, float* d_rgb, float* d_depth,
                                   float* d_weights, float* losses, double* aux, double* dist, void* workspace, size_t workspace_bytes,
                                   t2n_stream stream) {
    if (!rgb || !depth || !weights || !z_vals || !rgb_t || !depth_t || !d_rgb || !d_depth || !d_weights || !losses || !aux || !dist || !workspace ||
        n_rays <= 0 || n_samples <= 0) {
        set_error("t2n_train_loss_dist: bad argument");
        return T2N_ERR_INVALID;
    }
    if (depth_kind < 0 || depth_kind > 3) { set_error("t2n_train_loss_dist: depth_kind %d is none of 0 (mse), 1 (gnll), 2 (si_log), 3 (ssi)", depth_kind); return T2N_ERR_INVALID; }
    if (depth_kind == 1 && !(target_std > 0.f)) { set_error("t2n_train_loss_dist: gnll needs target_std > 0"); return T2N_ERR_INVALID; }
    if (!positive_finite((double)inv_range)) { set_error("t2n_train_loss_dist: inv_range must be finite and > 0"); return T2N_ERR_INVALID; }
    if (!(w_dist == 0.f || positive_finite((double)w_dist))) { set_error("t2n_train_loss_dist: w_dist must be finite and >= 0"); return T2N_ERR_INVALID; }
    if (((uintptr_t)workspace & 7) != 0) { set_error("t2n_train_loss_dist: the workspace must be 8-byte aligned"); return T2N_ERR_INVALID; }
    if (workspace_bytes < t2n_train_loss_dist_workspace_bytes(n_rays)) { set_error("t2n_train_loss_dist: workspace too small"); return T2N_ERR_WORKSPACE; }
    const size_t base_bytes = (t2n_train_loss_ex_workspace_bytes(n_rays) + 7) & ~(size_t)7;
    DepthLossArgs a;
    a.rgb = rgb; a.depth = depth; a.w = weights; a.z = z_vals; a.rgb_t = rgb_t; a.depth_t = depth_t; a.R = n_rays; a.N = n_samples;
    a.w_depth = w_depth; a.w_trans = w_trans; a.delta = delta; a.sigma = (double)target_std;
    a.d_rgb = d_rgb; a.d_depth = d_depth; a.d_w = d_weights; a.losses = losses; a.aux = aux;
    carve(a, workspace);
    a.dpart = (double*)((char*)workspace + base_bytes);
    a.dray = a.dpart + a.nblocks;
    a.w_dist = (double)w_dist; a.rho = (double)inv_range; a.gscale = (double)w_dist / (double)n_rays; a.dist = dist;
    const hipStream_t s = (hipStream_t)stream;
    if (w_dist == 0.f) {
        // t2n_train_loss_ex itself (bit-equal outputs); D is still reported
        const int rc = t2n_train_loss_ex(rgb, depth, weights, z_vals, rgb_t, depth_t, n_rays, n_samples, w_depth, w_trans, delta, depth_kind,
                                         target_std, d_rgb, d_depth, d_weights, losses, aux, workspace, workspace_bytes, stream);
        if (rc != T2N_OK) return rc;
        a.d_w = nullptr;
        return launch_distortion(a, s);
    }
    if (depth_kind == 0) {
        T2N_HIP(hipMemsetAsync(aux, 0, 4 * sizeof(double), s));
        a.fpart = (float*)workspace;
        hipLaunchKernelGGL(k_train_loss_dist, dim3(a.nblocks), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_train_loss_dist_reduce, dim3(1), dim3(256), 0, s, a);
        T2N_HIP(hipGetLastError());
        return T2N_OK;
    }
    return launch_depth_loss<true, true>(depth_kind, a, s);
}
