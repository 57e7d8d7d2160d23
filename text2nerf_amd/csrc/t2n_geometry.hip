// Geometry outputs of a view beside the render: the density feature's analytic gradient at points (k_density_grad_at) and, per ray
// of an EVAL march, acc / expected depth / the depth at a quantile of the weight distribution / the depth variance / the
// weight-averaged field normal (k_geometry). Siblings of k_density_at and k_march (t2n_march.hip): same sample positions, box mask,
// z gate, alpha-mask test and last-interval-0 rule as t2n_render_forward without T2N_FLAG_TRAIN; early termination never applies.
// Nothing of the render path is touched: no workspace, no atomics, no host read.
//
// Gradient: f = sum over pairs k and channels c of P_kc(u, v) L_kc(t) (models/tensoRF.py:205-220), P bilinear and L linear in the
// index coordinates of axis_taps. Inside the cell the float32 coordinate falls into, dP/du is the difference of the two taps along u
// weighted by the other axis, dL/dt the difference of the two line taps (clamped indices: 0 on the exact upper face), and the world
// gradient is the index gradient times inv_aabb_size[a] (grid[a] - 1) / 2.
#include <float.h>

#include "t2n_device.h"

namespace t2n {

__device__ __forceinline__ float4 f4_sub(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float f4_dot_acc(float4 a, float4 b, float s) {
    s = fmaf(a.x, b.x, s); s = fmaf(a.y, b.y, s); s = fmaf(a.z, b.z, s); s = fmaf(a.w, b.w, s);
    return s;
}

// One lane's share (channel quad q of the 16 density channels) of f and of its gradient in INDEX coordinates, g[a] along grid axis a.
// `part` runs k_density_at's multiply / fma chain: the quad sum of it is that kernel's feature bit for bit.
template <int K, bool HALF>
__device__ __forceinline__ void pair_grad(const FactorSet& S, int q, const Axes3& A, float& part, float (&g)[3]) {
    QuadTaps t;
    issue_taps_ax<K, HALF>(S, 4, q, A, t);
    const Axis& ax = A.a[mat0(K)];
    const Axis& ay = A.a[mat1(K)];
    const float4 p = taps_plane(t), l = taps_line(t);
    if constexpr (K == 0) { part = p.x * l.x; part = fmaf(p.y, l.y, part); part = fmaf(p.z, l.z, part); part = fmaf(p.w, l.w, part); }
    else part = f4_dot_acc(p, l, part);
    const float4 du = f4_fma(f4_sub(t.se, t.sw), ay.w1, f4_mul(f4_sub(t.ne, t.nw), ay.w0));   // dP / d(index along mat0)
    const float4 dv = f4_fma(f4_sub(t.se, t.ne), ax.w1, f4_mul(f4_sub(t.sw, t.nw), ax.w0));   // dP / d(index along mat1)
    const float4 dl = f4_sub(t.l1, t.l0);                                                     // dL / d(index along vec)
    g[mat0(K)] = f4_dot_acc(du, l, g[mat0(K)]);
    g[mat1(K)] = f4_dot_acc(dv, l, g[mat1(K)]);
    g[vecm(K)] = f4_dot_acc(p, dl, g[vecm(K)]);
}

// f and the WORLD gradient of the density feature at one point, from the four lanes of its quad (all four return the sums)
template <bool HALF>
__device__ __forceinline__ void density_grad_quad(const FieldDev& F, int q, const Axes3& A, bool ok, float& feat, float& gx, float& gy,
                                                  float& gz) {
    float part = 0.f, g[3] = {0.f, 0.f, 0.f};
    if (ok) {
        pair_grad<0, HALF>(F.den, q, A, part, g);
        pair_grad<1, HALF>(F.den, q, A, part, g);
        pair_grad<2, HALF>(F.den, q, A, part, g);
    }
    feat = group_sum<4>(part);
    // d(index a) / d(world a) = inv_aabb_size[a] (grid[a] - 1) / 2   (normalisation :245-246, then axis_taps' ((g + 1) / 2) (size - 1))
    gx = group_sum<4>(g[0]) * ((F.inv[0] * (float)(F.den.W[0] - 1)) * 0.5f);
    gy = group_sum<4>(g[1]) * ((F.inv[1] * (float)(F.den.H[0] - 1)) * 0.5f);
    gz = group_sum<4>(g[2]) * ((F.inv[2] * (float)(F.den.H[1] - 1)) * 0.5f);
}

// Point-wise: 4 lanes per point, the six loads per factor pair of k_density_at.
__global__ __launch_bounds__(256) void k_density_grad_at(const FieldDev F, const float* __restrict__ xyz, long long n, float* feat_out,
                                                         float* grad_out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long p = t >> 2;
    const int q = (int)(t & 3);
    const bool ok = p < n;
    Axes3 A = {};
    if (ok) A = sample_axes(F.den, xyz[p * 3 + 0], xyz[p * 3 + 1], xyz[p * 3 + 2]);
    float feat, gx, gy, gz;
    density_grad_quad<false>(F, q, A, ok, feat, gx, gy, gz);
    if (ok && q == 0) {
        if (feat_out) feat_out[p] = feat;
        if (grad_out) { grad_out[p * 3 + 0] = gx; grad_out[p * 3 + 1] = gy; grad_out[p * 3 + 2] = gz; }
    }
}

__device__ __forceinline__ float wave_scan_add(float v, int lane) {   // inclusive sum scan over the 64 lanes (lane 0 first)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}
// (t2n_depth_loss.hip keeps the same four lines in its own anonymous namespace; the shared header is read by the render path's
// kernels, whose sources this file's addition leaves byte for byte as they were)
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// k_march's pass A for an eval ray: first / last sample that passes the box test and the z gate (the mask is an interval). A copy of
// that pass (t2n_march.hip), not a shared function: the render path's kernels stay exactly as they are. Windows of more than 64
// samples take the wide form (tests/test_geometry_gpu.py, the multi-block cases); the exact scan is the fallback for a range that
// does not bracket the window, which the +-3 sample margin of ray_interval leaves no eval ray to reach.
__device__ __forceinline__ void valid_interval(const FieldDev& F, const Ray& ray, int N, int lane, int& first, int& last) {
    first = N; last = -1;
    int lo, hi;
    ray_interval<false>(F, ray, N, lo, hi);
    bool done = hi < lo;
    if (!done) {
        const bool narrow = hi - lo < 64;
        const int i = narrow ? lo + lane : (lane < 32 ? lo + lane : hi - (lane - 32));
        bool ok = false;
        if (i >= lo && i <= hi) {
            float xn, yn, zn;
            ok = sample_point<false>(F, ray, sample_z<false>(F, ray, i, 0.f), xn, yn, zn);
        }
        const unsigned long long m = __ballot(ok);
        if (narrow) {
            if (m) { first = lo + (int)__ffsll((long long)m) - 1; last = lo + 63 - (int)__clzll((long long)m); }
            const bool lo_ok = !(m & 1ull) || lo == 0;
            const bool hi_ok = !((m >> (hi - lo)) & 1ull) || hi == N - 1;
            done = lo_ok && hi_ok;
            if (!done) { first = N; last = -1; }
        } else {
            const unsigned mlo = (unsigned)m, mhi = (unsigned)(m >> 32);
            const bool lo_ok = !(mlo & 1u) || lo == 0, hi_ok = !(mhi & 1u) || hi == N - 1;
            if (mlo && mhi && lo_ok && hi_ok) {
                first = lo + (int)__ffs((int)mlo) - 1;
                last = hi - ((int)__ffs((int)mhi) - 1);
                done = true;
            }
        }
    }
    if (!done) {   // exact scan over all samples
        for (int base = 0; base < N; base += 64) {
            const int i = base + lane;
            bool ok = false;
            if (i < N) {
                float xn, yn, zn;
                ok = sample_point<false>(F, ray, sample_z<false>(F, ray, i, 0.f), xn, yn, zn);
            }
            const unsigned long long m = __ballot(ok);
            if (m) {
                if (first == N) first = base + (int)__ffsll((long long)m) - 1;
                last = base + 63 - (int)__clzll((long long)m);
            }
        }
    }
}

struct GeometryArgs {
    FieldDev F;
    const float* rays; long long n_rays; int ray_stride; int n_samples;
    float quantile, miss_depth;
    float* acc; float* depth; float* median; float* var; float* normal;
    unsigned nblocks;
};

// One wave per ray, four waves per workgroup; the ray's window in blocks of 64 samples, so LDS use (1 KB per wave) does not depend
// on N. A ray's arithmetic involves its own wave only: its outputs depend neither on n_rays nor on its place in the batch, and no
// atomics are used: two calls give the same bits.
template <bool HALF>
__global__ __launch_bounds__(256) void k_geometry(const GeometryArgs a) {
    __shared__ __attribute__((aligned(16))) float4 win[4][64];   // (sigma, n_x, n_y, n_z) of the block's samples, per wave
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const FieldDev& F = a.F;
    const long long r = (long long)xcd_tile(blockIdx.x, a.nblocks) * 4 + wid;
    if (r >= a.n_rays) return;
    const int N = a.n_samples;
    const Ray ray = load_ray(F, a.rays + r * a.ray_stride, a.ray_stride);

    int first, last;
    valid_interval(F, ray, N, lane, first, last);
    const int Lw = last - first + 1;   // window length (<= 0: empty ray)

    float acc = 0.f, dep = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
    // variance: float64 moments about the first window sample's depth (sum w z^2 - D^2 in float32 cancels completely)
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    const float zp = Lw > 0 ? sample_z<false>(F, ray, first, 0.f) : 0.f;
    float carry = 1.f, ccum = 0.f;     // transmittance / cumulative weight in front of the block
    bool found = false;
    float med = a.miss_depth;
    const int q = lane & 3, sl = lane >> 2;
    for (int b0 = 0; b0 < Lw; b0 += 64) {
        const int b1 = min(Lw, b0 + 64);
        // ---- gather: 16 samples per step, 4 lanes each -> sigma and the unit normal into the window
        for (int base = b0; base < b1; base += 16) {
            const int j = base + sl;
            float xn = 0.f, yn = 0.f, zn = 0.f;
            bool ok = false;
            if (j < b1) {
                const float z = sample_z<false>(F, ray, first + j, 0.f);
                ok = sample_point<false>(F, ray, z, xn, yn, zn);
                if (F.alpha && ok) ok = alpha_pass(F, ray, z);      // models/tensorBase.py:451-456
            }
            Axes3 A = {};
            if (ok) A = sample_axes_inbox(F.den, xn, yn, zn);
            float feat, gx, gy, gz;
            density_grad_quad<HALF>(F, q, A, ok, feat, gx, gy, gz);
            if (q == 0 && j < b1) {
                float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ok) {
                    // softplus' > 0 and relu' >= 0: -grad f / |grad f| is the direction of steepest density decrease
                    // -g / max(|g|, FLT_MIN) without squaring g itself (components below 1e-19 have squares that underflow):
                    // h = g / max(largest |component|, FLT_MIN) has |h| in [1, sqrt 3] unless |g| < FLT_MIN, where h is g / FLT_MIN
                    const float s = fmaxf(fmaxf(fabsf(gx), fabsf(gy)), fmaxf(fabsf(gz), FLT_MIN));
                    const float hx = gx / s, hy = gy / s, hz = gz / s;
                    const float d = fmaxf(sqrtf((hx * hx + hy * hy) + hz * hz), 1.f);
                    e = make_float4(feature2density(F, feat), (-hx) / d, (-hy) / d, (-hz) / d);
                }
                win[wid][j - b0] = e;
            }
        }
        // LDS window written by lanes of this wave only; a wave is in lock-step, but the compiler needs the fence.
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();

        // ---- scan: alpha, transmittance, weights (k_march's pass C), sums, first crossing of the quantile
        {
            const int j = b0 + lane;
            const int i = first + j;
            const bool in = j < b1;
            float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
            float z = 0.f, dist = 0.f;
            if (in) {
                e = win[wid][lane];
                z = sample_z<false>(F, ray, i, 0.f);
                if (i < N - 1) dist = sample_z<false>(F, ray, i + 1, 0.f) - z;   // :448, last sample gets 0
            }
            const float d = scaled_dist(F, ray, dist);
            const float nsd = (-e.x) * d;
            const float alpha = 1.f - exp_finite(nsd);   // (nsd <= 0)
            const float f = (1.f - alpha) + 1e-10f;
            const float incl = wave_scan_mul(f, lane);
            float excl = __shfl_up(incl, 1);
            if (lane == 0) excl = 1.f;
            const float T = carry * excl;
            const float w = in ? alpha * T : 0.f;
            carry = carry * __shfl(incl, 63);
            acc += w;
            dep = fmaf(w, z, dep);
            nx = fmaf(w, e.y, nx); ny = fmaf(w, e.z, ny); nz = fmaf(w, e.w, nz);
            const double wd = (double)w, dz = (double)z - (double)zp;
            s0 += wd; s1 = fma(wd, dz, s1); s2 = fma(wd * dz, dz, s2);
            // cumulative weight: C_i = ccum + (inclusive sum inside the block); the first sample with C_i >= quantile
            const float cin = wave_scan_add(w, lane);
            float cex = __shfl_up(cin, 1);
            if (lane == 0) cex = 0.f;
            const float cprev = ccum + cex, ccur = ccum + cin;
            const unsigned long long hit = __ballot(in & (ccur >= a.quantile));
            if (!found && hit) {
                const int k = (int)__ffsll((long long)hit) - 1;
                const float zk = __shfl(z, k), dk = __shfl(dist, k), ck = __shfl(cprev, k), wk = __shfl(w, k);
                // w_k spread over the interval that produced it (dist_k unscaled): continuous and monotone in the quantile
                float t = wk > 0.f ? (a.quantile - ck) / wk : 0.f;
                t = fminf(fmaxf(t, 0.f), 1.f);
                med = fmaf(dk, t, zk);
                found = true;
            }
            ccum = ccum + __shfl(cin, 63);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    acc = wave_sum(acc); dep = wave_sum(dep);
    nx = wave_sum(nx); ny = wave_sum(ny); nz = wave_sum(nz);
    s0 = wave_sum_f64(s0); s1 = wave_sum_f64(s1); s2 = wave_sum_f64(s2);
    if (lane == 0) {
        const float D = dep + (1.f - acc) * ray.last;   // :504-505
        if (a.acc) a.acc[r] = acc;
        if (a.depth) a.depth[r] = D;
        if (a.median) a.median[r] = med;
        if (a.var) {
            const double m = (double)D - (double)zp;
            const double v = fma(m * m, s0, fma(-2.0 * m, s1, s2));   // sum w (z - D)^2
            a.var[r] = (float)fmax(v, 0.0);
        }
        if (a.normal) { a.normal[r * 3 + 0] = nx; a.normal[r * 3 + 1] = ny; a.normal[r * 3 + 2] = nz; }
    }
}

}  // namespace t2n

using namespace t2n;

extern "C" int t2n_density_grad_at(const t2n_field* f, const float* xyz_norm, int64_t n, float* feat, float* grad_world,
                                   t2n_stream stream) {
    if (!f || !xyz_norm || n < 0 || n > 0x7fffffffll * 16) { set_error("t2n_density_grad_at: bad argument"); return T2N_ERR_INVALID; }
    if (!f->uploaded) { set_error("t2n_density_grad_at: field has no uploaded parameters"); return T2N_ERR_STATE; }
    if (n == 0 || (!feat && !grad_world)) return T2N_OK;
    const long long threads = (long long)n * 4;
    hipLaunchKernelGGL(k_density_grad_at, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, f->dev, xyz_norm,
                       (long long)n, feat, grad_world);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" int t2n_render_geometry(const t2n_field* f, const float* rays, int64_t n_rays, int ray_stride, int n_samples, float quantile,
                                   float miss_depth, float* acc, float* depth, float* depth_median, float* depth_var, float* normal,
                                   t2n_stream stream) {
    if (!f || !rays || n_rays < 0 || n_rays > 0x7fffffffll * 4 || ray_stride < 6 || n_samples <= 0) {
        set_error("t2n_render_geometry: bad argument");
        return T2N_ERR_INVALID;
    }
    if (!(quantile > 0.f && quantile < 1.f)) {
        set_error("t2n_render_geometry: quantile %g is not inside (0, 1)", (double)quantile);
        return T2N_ERR_INVALID;
    }
    if (!f->uploaded) { set_error("t2n_render_geometry: field has no uploaded parameters"); return T2N_ERR_STATE; }
    if (n_rays == 0 || (!acc && !depth && !depth_median && !depth_var && !normal)) return T2N_OK;
    GeometryArgs a;
    a.F = f->dev;
    a.rays = rays; a.n_rays = n_rays; a.ray_stride = ray_stride; a.n_samples = n_samples;
    a.quantile = quantile; a.miss_depth = miss_depth;
    a.acc = acc; a.depth = depth; a.median = depth_median; a.var = depth_var; a.normal = normal;
    a.nblocks = (unsigned)((n_rays + 3) / 4);
    const bool half = f->factor_bf16 && f->dev.den.plane_h[0];
    if (half) hipLaunchKernelGGL((k_geometry<true>), dim3(a.nblocks), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((k_geometry<false>), dim3(a.nblocks), dim3(256), 0, (hipStream_t)stream, a);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}
