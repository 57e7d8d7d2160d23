// General-shape render path, the backward as kernels (t2n_generic_backward_staged; the plain form t2n_generic_backward in
// t2n_generic.hip stays the fallback and the A/B partner). Built like the forward's kernel form and on what that forward left in the
// caller's workspace: the channel-last factor copies, the appearance list with its device-side count, sigma / T / rgb_s / acc / raw and
// the go scratch are reused, nothing of them is rebuilt.
//   k_genb_scan      a wave per ray, 64-sample rounds from the far end: dL/dw of every sample, the suffix sum S = sum_{j>i} G_j w_j by a
//                    wave scan with a carry, d alpha -> d sigma -> dfeat[t] (0 where the density has no gradient), go[t] for list entries.
//                    k_gen_bwd_march's arithmetic term by term (closed-interval clamp gate, `common`, fct = e + 1e-10, softplus's
//                    threshold of 20, the ReLU gate, scaled_dist with the ray's norm on NDC rays); S is summed in scan order.
//   k_genb_density   a wave per 64 samples, one sample with a gradient at a time: box / mask test (gen_point: masked and out-of-box samples
//                    add nothing), then lanes run along the COMPONENTS of each tap row of the channel-last gradient copies — a wave
//                    instruction adds contiguous floats instead of one lane per [1, C, H, W] row.
//   head, per pass of pass_rows list entries (issued for the worst case, clipped to the count on the device; nothing depends on row0
//   beyond addressing):
//     MLP heads      k_gen_head_rows + two k_dense (the forward's kernels: the same x0 / h0 / h1, hence the forward's ReLU decisions),
//                    k_genb_l2 (d2 = go c (1 - c), G1 = (d2 W2) [h1 > 0]), dW2 / dW1 / dW0 as k_gemm_tn (exact-fp32 MFMA over row chunks,
//                    partial slabs, k_gemm_tn_reduce; 128 rows of M per launch, two launches for 129..256 units), the bias sums as
//                    k_genb_colsum slabs + a fixed-order reduce, G0 = (G1 W1) [h0 > 0] and GX = G0 W0 as k_dense on transposed weight
//                    copies (the mask as one elementwise pass), k_genb_gfeat (raw column + sum_o 2^o (cos g_sin - sin g_cos) with the
//                    octaves read back from x0, i.e. as the forward built them; view-direction columns carry no gradient)
//     SH / RGB       k_genb_simple_gf (gfeat[c 9 + b] = go[c] sh[b] where the pre-ReLU colour is positive; gfeat = go)
//     all heads      k_genb_app<2> writes X[col] = plane x line per row, d basis = gfeat^T X (k_gemm_tn), GXapp = gfeat B (k_dense),
//                    k_genb_app<1> scatters GXapp[col] line w_tap into the plane rows and GXapp[col] plane into the line rows (as k_genb_density)
//   k_genb_unstage   the channel-last gradient copies, transposed through an LDS tile (k_gen_stage's mirror), ADDED into the caller's
//                    [1, C, H, W] / [1, C, L, 1] tensors; a NULL gradient pointer skips that tensor.
// Exact fp32 throughout (no f16 splits). No atomic on any weight, bias or basis gradient: they are deterministic; the factor gradients
// carry float-atomic arrival order, as in the plain form. No host read, no allocation, no synchronisation; every argument is checked
// before the first launch. LDS: 16.6 KB (k_genb_unstage), the reused kernels keep theirs (k_dense <= 133 KB, k_gen_head_rows <= 160 KB).
// Kept on the plain form: MLP heads with more than 512 inputs (k_dense stages a K x 64 weight slab in LDS) and shapes whose staged head
// does not fit 160 KB of LDS (their forward runs plain, so there are no staged copies and no list to reuse).
// Replaces: the autograd of models/tensorBase.py:436-507, :19-26, :406-410, :11-17, :29-39, :62-159 and models/tensoRF.py:205-239.
#include <stdlib.h>

#include "t2n_generic.h"

namespace t2n {

struct GenBwd {
    float* gdp[3]; float* gdl[3]; float* gap[3]; float* gal[3];   // channel-last gradient copies (the staged factors' shapes)
    float* dfeat;                 // [R N] dL/d density feature
    unsigned* pcnt;               // [max_passes] list entries of each pass
    unsigned pass_rows, max_passes;
    float* d2; float* g1; float* g0; float* gx; float* gf; float* X; float* gxa;   // one pass's rows
    const float* x0; const float* h0; const float* h1;                             // (the forward's carve)
    int ldd2, ldg, ldx, ldh, ldgf, ldX;
};

// dst [cols][rows] = src [rows][cols]^T (the head's matrices: a few hundred KB at most)
__global__ __launch_bounds__(256) void k_genb_transpose(const float* __restrict__ src, int rows, int cols, float* __restrict__ dst) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)rows * cols) return;
    const int c = (int)(t / rows), r = (int)(t - (long long)c * rows);
    dst[t] = src[(size_t)r * cols + c];
}
__global__ __launch_bounds__(256) void k_genb_plan(const unsigned* __restrict__ count, HeadPlanDev* __restrict__ plan, unsigned* __restrict__ pcnt,
                                                   unsigned pass_rows, unsigned max_passes) {
    const unsigned cnt = *count;
    if (blockIdx.x == 0 && threadIdx.x == 0) plan->rows = cnt;
    for (unsigned p = blockIdx.x * blockDim.x + threadIdx.x; p < max_passes; p += gridDim.x * blockDim.x) {
        const unsigned long long lo = (unsigned long long)p * pass_rows;
        pcnt[p] = cnt > lo ? (unsigned)((cnt - lo) < pass_rows ? (cnt - lo) : pass_rows) : 0u;
    }
}

// ---- reverse scan: one wave per ray ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_genb_scan(const GenArgs a, const GenBwd b) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long long r = (long long)blockIdx.x * 4 + wid;
    if (r >= a.n_rays) return;
    const int N = a.N;
    const Ray ray = load_ray(a.F, a.rays + r * a.ray_stride, a.ray_stride);
    float dc[3];
    float dbg = 0.f;
    for (int k = 0; k < 3; ++k) {
        const float raw = a.raw[r * 3 + k];
        dc[k] = (raw >= 0.f && raw <= 1.f) ? a.d_rgb[r * 3 + k] : 0.f;        // clamp(0, 1): the gradient passes on the CLOSED interval
        dbg += dc[k];
    }
    const float dd = a.d_depth[r];
    const float common = (a.add_bg ? -dbg : 0.f) - dd * ray.last;
    float carry = 0.f;                                                         // sum of G_j w_j over the rounds behind this one
    for (int base = ((N - 1) / 64) * 64; base >= 0; base -= 64) {
        const int i = base + lane;
        const bool in = i < N;
        const long long t = r * N + (in ? i : N - 1);
        const float w = in ? a.w[t] : 0.f, z = a.z[t], sg = in ? a.sigma[t] : 0.f, T = a.T[t];
        float G = common + dd * z + (a.d_w ? a.d_w[t] : 0.f);
        if (in && w > a.F.thres) {
            for (int k = 0; k < 3; ++k) {
                G = fmaf(dc[k], a.rgb_s[t * 3 + k], G);
                a.go[t * 3 + k] = dc[k] * w;
            }
        }
        const float gw = in ? G * w : 0.f;
        float incl = gw;                                                       // inclusive SUFFIX sum over the lanes (lane 63 first)
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float tv = __shfl_down(incl, o);
            if (lane + o < 64) incl += tv;
        }
        float excl = __shfl_down(incl, 1);
        if (lane == 63) excl = 0.f;
        const float S = carry + excl;
        carry += __shfl(incl, 0);
        const float dist = (in && i < N - 1) ? a.z[t + 1] - z : 0.f;
        const float sd = scaled_dist(a.F, ray, dist);
        const float e = expf((-sg) * sd);                      // 1 - alpha
        const float fct = e + 1e-10f;
        const float dalpha = G * T - S / fct;
        const float dsg = dalpha * sd * e;
        float df = 0.f;
        if (in && !(dsg == 0.f || (sg == 0.f && a.F.act == T2N_ACT_RELU)))
            df = (a.F.act == T2N_ACT_RELU || sg > 20.f) ? dsg : dsg * (-expm1f(-sg));
        if (in) b.dfeat[t] = df;
    }
}

// ---- one factor set at one sample, lanes along the components ---------------------------------------------------------------------
// MODE 0: density scatter (the same gradient gu for every component), 1: appearance scatter (grow[col]), 2: X[col] = plane x line -> xrow
template <int MODE>
__device__ __forceinline__ void genb_set(const GenArgs& a, const float* const* __restrict__ P, const float* const* __restrict__ L,
                                         float* const* GP, float* const* GL, const int* Cn, const Tap3& tp, int lane, float gu,
                                         const float* __restrict__ grow, float* __restrict__ xrow) {
    int col0 = 0;
#pragma unroll 1
    for (int k = 0; k < 3; ++k) {
        const int W = a.grid[mat0(k)], C = Cn[k];
        const Axis& ax = tp.a[mat0(k)]; const Axis& ay = tp.a[mat1(k)]; const Axis& al = tp.a[vecm(k)];
        const size_t o00 = ((size_t)ay.i0 * W + ax.i0) * C, o01 = ((size_t)ay.i0 * W + ax.i1) * C;
        const size_t o10 = ((size_t)ay.i1 * W + ax.i0) * C, o11 = ((size_t)ay.i1 * W + ax.i1) * C;
        const size_t q0 = (size_t)al.i0 * C, q1 = (size_t)al.i1 * C;
        const float w00 = ay.w0 * ax.w0, w01 = ay.w0 * ax.w1, w10 = ay.w1 * ax.w0, w11 = ay.w1 * ax.w1;
        for (int c = lane; c < C; c += 64) {
            float pv = P[k][o00 + c] * w00;
            pv = fmaf(P[k][o01 + c], w01, pv); pv = fmaf(P[k][o10 + c], w10, pv); pv = fmaf(P[k][o11 + c], w11, pv);
            const float lv = fmaf(L[k][q1 + c], al.w1, L[k][q0 + c] * al.w0);
            if (MODE == 2) xrow[col0 + c] = pv * lv;
            else {
                const float g = MODE == 0 ? gu : grow[col0 + c];
                const float gp = g * lv, gl = g * pv;
                atomicAdd(GP[k] + o00 + c, gp * w00); atomicAdd(GP[k] + o01 + c, gp * w01);
                atomicAdd(GP[k] + o10 + c, gp * w10); atomicAdd(GP[k] + o11 + c, gp * w11);
                atomicAdd(GL[k] + q0 + c, gl * al.w0); atomicAdd(GL[k] + q1 + c, gl * al.w1);
            }
        }
        col0 += C;
    }
}

// ---- density scatter: a wave per 64 samples, the samples with a gradient one after the other ---------------------------------------
__global__ __launch_bounds__(256) void k_genb_density(const GenArgs a, const GenFast fa, const GenBwd b) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long long tot = a.n_rays * a.N;
    const long long t0 = ((long long)blockIdx.x * 4 + wid) * 64;
    if (t0 >= tot) return;
    const float dfv = t0 + lane < tot ? b.dfeat[t0 + lane] : 0.f;
    unsigned long long bal = __ballot(dfv != 0.f);
    while (bal) {
        const int sl = __ffsll((long long)bal) - 1;
        bal &= bal - 1ull;
        const float df = __shfl(dfv, sl);
        const long long t = t0 + sl;
        const long long r = t / a.N;
        const Ray ray = load_ray(a.F, a.rays + r * a.ray_stride, a.ray_stride);
        float xn, yn, zn;
        if (!gen_point(a, ray, a.z[t], xn, yn, zn)) continue;       // (sigma is 0 and constant outside the box and under the mask)
        const Tap3 tp = gen_taps(a, xn, yn, zn);
        genb_set<0>(a, fa.dp, fa.dl, b.gdp, b.gdl, a.Cd, tp, lane, df, nullptr, nullptr);
    }
}

// ---- appearance factors of one pass: a wave per list entry (MODE 2: X rows, MODE 1: scatter of GXapp) -------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void k_genb_app(const GenArgs a, const GenFast fa, const GenBwd b, unsigned pass) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const unsigned cnt = b.pcnt[pass];
    const unsigned row0 = pass * b.pass_rows;
    for (unsigned lrow = blockIdx.x * 4 + wid; lrow < cnt; lrow += gridDim.x * 4) {
        const long long t = fa.list[row0 + lrow];
        const long long r = t / a.N;
        const int i = (int)(t - r * a.N);
        const Ray ray = load_ray(a.F, a.rays + r * a.ray_stride, a.ray_stride);
        float xn, yn, zn;
        gen_point<false>(a, ray, gen_z(a, ray, i, gen_u(a, r)), xn, yn, zn);       // (the forward's coordinates of a sample known to be valid)
        const Tap3 tp = gen_taps(a, xn, yn, zn);
        genb_set<MODE>(a, fa.ap, fa.al, b.gap, b.gal, a.Ca, tp, lane, 0.f, b.gxa + (size_t)lrow * b.ldX, b.X + (size_t)lrow * b.ldX);
    }
}

// ---- layer 2: d2 = go c (1 - c) -> D2 [rows][32] (zero beyond 3), G1 = (d2 W2) [h1 > 0] -> [rows][ldg] (zero from fC to fC rounded up to 4)
__global__ __launch_bounds__(256) void k_genb_l2(const GenArgs a, const GenFast fa, const GenBwd b, unsigned pass) {
    const unsigned cnt = b.pcnt[pass];
    const unsigned row0 = pass * b.pass_rows;
    const int fC = a.fC, f4 = (fC + 3) & ~3;
    const int per = f4 > 32 ? f4 : 32;                           // threads per row: the G1 columns, and the 32 of D2
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < (long long)cnt * per; q += (long long)gridDim.x * blockDim.x) {
        const unsigned lrow = (unsigned)(q / per);
        const int v = (int)(q - (long long)lrow * per);
        const long long t = fa.list[row0 + lrow];
        float d2[3];
        for (int c = 0; c < 3; ++c) { const float c3 = a.rgb_s[t * 3 + c]; d2[c] = a.go[t * 3 + c] * c3 * (1.f - c3); }
        if (v < 32) b.d2[(size_t)lrow * b.ldd2 + v] = v == 0 ? d2[0] : (v == 1 ? d2[1] : (v == 2 ? d2[2] : 0.f));
        if (v < f4) {
            float g = 0.f;
            if (v < fC && b.h1[(size_t)lrow * b.ldh + v] > 0.f)
                for (int c = 0; c < 3; ++c) g = fmaf(a.w2[(size_t)c * fC + v], d2[c], g);
            b.g1[(size_t)lrow * b.ldg + v] = g;
        }
    }
}
// G [rows][ldg] *= [H > 0] over the first n columns
__global__ __launch_bounds__(256) void k_genb_mask(float* __restrict__ G, int ldg, const float* __restrict__ H, int ldh, int n,
                                                   const unsigned* __restrict__ pcnt) {
    const unsigned cnt = *pcnt;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < (long long)cnt * n; q += (long long)gridDim.x * blockDim.x) {
        const unsigned lrow = (unsigned)(q / n);
        const int v = (int)(q - (long long)lrow * n);
        if (!(H[(size_t)lrow * ldh + v] > 0.f)) G[(size_t)lrow * ldg + v] = 0.f;
    }
}
// bias gradients: column sums of G over row chunks -> part [kColChunks][N], then one thread per column adds the chunks up in order
constexpr int kColChunks = 128;
__global__ __launch_bounds__(256) void k_genb_colsum(const float* __restrict__ G, int ld, int N, const unsigned* __restrict__ pcnt, float* __restrict__ part) {
    const unsigned cnt = *pcnt;
    const unsigned per = (cnt + kColChunks - 1) / kColChunks;
    const unsigned r0 = blockIdx.x * per, r1 = r0 + per < cnt ? r0 + per : cnt;
    for (int n = threadIdx.x; n < N; n += 256) {
        float s = 0.f;
        for (unsigned r = r0; r < r1; ++r) s += G[(size_t)r * ld + n];
        part[(size_t)blockIdx.x * N + n] = s;
    }
}
__global__ __launch_bounds__(256) void k_genb_colsum_reduce(const float* __restrict__ part, int N, float* db) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float s = 0.f;
    for (int c = 0; c < kColChunks; ++c) s += part[(size_t)c * N + n];
    db[n] += s;
}

// ---- dL/d features of the MLP heads from GX = dL/d input row: thread per (row, feature column of gf) ----------------------------------
__global__ __launch_bounds__(256) void k_genb_gfeat(const GenArgs a, const GenBwd b, unsigned pass) {
    const unsigned cnt = b.pcnt[pass];
    const int D = a.app_dim, ld = b.ldgf;
    const int fpe = a.shading == T2N_SHADE_MLP ? 0 : a.fea_pe;
    const int pe0 = D + (a.shading != T2N_SHADE_MLP_FEA_NOVIEW ? 3 : 0);
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < (long long)cnt * ld; q += (long long)gridDim.x * blockDim.x) {
        const unsigned lrow = (unsigned)(q / ld);
        const int f = (int)(q - (long long)lrow * ld);
        float g = 0.f;
        if (f < D) {
            const float* __restrict__ gr = b.gx + (size_t)lrow * b.ldx;
            const float* __restrict__ xr = b.x0 + (size_t)lrow * b.ldx;
            g = gr[f];
            const int js = pe0 + f * fpe, jc = js + fpe * D;
            for (int o = 0; o < fpe; ++o) {
                const float sc = (float)(1 << o);
                g = fmaf(gr[js + o] * sc, xr[jc + o], g);          // d sin(2^o f) = 2^o cos
                g = fmaf(-(gr[jc + o] * sc), xr[js + o], g);       // d cos(2^o f) = -2^o sin
            }
        }
        b.gf[(size_t)lrow * ld + f] = g;
    }
}
// SH / RGB: gfeat straight from go
__global__ __launch_bounds__(256) void k_genb_simple_gf(const GenArgs a, const GenFast fa, const GenBwd b, unsigned pass) {
    const unsigned cnt = b.pcnt[pass];
    const unsigned row0 = pass * b.pass_rows;
    const int ld = b.ldgf;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < (long long)cnt * ld; q += (long long)gridDim.x * blockDim.x) {
        const unsigned lrow = (unsigned)(q / ld);
        const int f = (int)(q - (long long)lrow * ld);
        const long long t = fa.list[row0 + lrow];
        float g = 0.f;
        if (a.shading == T2N_SHADE_RGB) { if (f < 3) g = a.go[t * 3 + f]; }
        else if (f < 27) {
            const int c = f / 9, bb = f - 9 * c;
            if (a.rgb_s[t * 3 + c] > 0.f) {                        // relu(q + 0.5) > 0 exactly where q + 0.5 > 0
                const long long r = t / a.N;
                const Ray ray = load_ray(a.F, a.rays + r * a.ray_stride, a.ray_stride);
                float dir[3], sh[9];
                gen_dir(a, ray, dir);
                gen_sh9(dir, sh);
                float shv = 0.f;
#pragma unroll
                for (int q = 0; q < 9; ++q) shv = q == bb ? sh[q] : shv;      // (a select chain: a dynamic index would put sh[] in scratch)
                g = a.go[t * 3 + c] * shv;
            }
        }
        b.gf[(size_t)lrow * ld + f] = g;
    }
}

// ---- unstage: dst [C][HW] += src [HW][C]^T (k_gen_stage's tile, the other way round) -----------------------------------------------
__global__ __launch_bounds__(256) void k_genb_unstage(const GenStageArgs a) {
    __shared__ float tile[64][65];
    int t = 0;
#pragma unroll 1
    for (int q = 1; q < 12; ++q) t += (a.block0[q] <= blockIdx.x) ? 1 : 0;
    float* dst = a.dst[t];
    if (!dst) return;                                   // (uniform over the workgroup)
    const int C = a.C[t];
    const long long HW = a.HW[t];
    const int cb = (C + 63) / 64;
    const unsigned bk = blockIdx.x - a.block0[t];
    const long long p0 = (long long)(bk / cb) * 64;
    const int c0 = (int)(bk % cb) * 64;
    const int lp = threadIdx.x & 63, q4 = threadIdx.x >> 6;
    for (int pp = q4; pp < 64; pp += 4)
        tile[pp][lp] = (c0 + lp < C && p0 + pp < HW) ? a.src[t][(p0 + pp) * C + c0 + lp] : 0.f;
    __syncthreads();
    for (int c = q4; c < 64; c += 4)
        if (c0 + c < C && p0 + lp < HW) dst[(long long)(c0 + c) * HW + p0 + lp] += tile[lp][c];
}

// ---- plan and carve ------------------------------------------------------------------------------------------------------------------
static int genb_in0(const t2n_generic_desc* d) {
    const int fpe = d->shading == T2N_SHADE_MLP ? 0 : (d->fea_pe > 0 ? d->fea_pe : 0);
    return d->app_dim * (1 + 2 * fpe) + (d->shading != T2N_SHADE_MLP_FEA_NOVIEW ? 3 + 6 * (d->view_pe > 0 ? d->view_pe : 0) : 0);
}
static bool genb_is_mlp(const t2n_generic_desc* d) {
    return d->shading == T2N_SHADE_MLP_FEA_NOVIEW || d->shading == T2N_SHADE_MLP_FEA || d->shading == T2N_SHADE_MLP;
}
static bool genb_kernel_form(const t2n_generic_desc* d) {
    static const bool plain_bwd = getenv("T2N_GENERIC_PLAIN_BWD") && atoi(getenv("T2N_GENERIC_PLAIN_BWD")) != 0;
    if (plain_bwd || !gen_forward_staged(d)) return false;
    if (genb_is_mlp(d)) return genb_in0(d) <= 512 && d->feature_c >= 1 && d->feature_c <= 512;
    return d->shading == T2N_SHADE_SH || d->shading == T2N_SHADE_RGB;
}
static uint32_t genb_pass_rows(int64_t R, int N, uint32_t req) {
    const unsigned long long tot64 = ((unsigned long long)R * (unsigned long long)N + 63) / 64 * 64;
    unsigned long long pr = req ? ((unsigned long long)req + 63) / 64 * 64 : (unsigned long long)kGenPassRows;
    if (pr > tot64) pr = tot64;
    return (uint32_t)pr;
}
struct GenBwdCarve { size_t g[12], zb, zero_end, dfeat, pcnt, w1t, w0t, bt, d2, g1, g0, gx, gf, X, gxa, part, csum, total;
                     int ldg, ldgf, ldX, in0, ncol; uint32_t pass_rows, max_passes; };
static GenBwdCarve genb_carve(const t2n_generic_desc* d, int64_t R, int N, uint32_t req) {
    GenBwdCarve c;
    memset(&c, 0, sizeof(c));
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = (o + bytes + 255) / 256 * 256; return at; };
    for (int q = 0; q < 4; ++q)
        for (int k = 0; k < 3; ++k) {
            const size_t HW = (size_t)d->grid[mat1(k)] * d->grid[mat0(k)], L = (size_t)d->grid[vecm(k)];
            const size_t C = q < 2 ? (size_t)d->density_n_comp[k] : (size_t)d->app_n_comp[k];
            c.g[q * 3 + k] = take(((q & 1) ? L : HW) * C * 4);
        }
    const bool mlp = genb_is_mlp(d);
    const size_t fc = mlp ? (size_t)d->feature_c : 0, D = (size_t)d->app_dim;
    c.in0 = mlp ? genb_in0(d) : 0;
    c.ncol = d->app_n_comp[0] + d->app_n_comp[1] + d->app_n_comp[2];
    size_t zn = (size_t)c.ncol > fc ? (size_t)c.ncol : fc;
    if ((size_t)c.in0 > zn) zn = (size_t)c.in0;
    c.zb = take(zn * 4);                                  // a zero bias for the k_dense launches (zeroed with the gradient copies)
    c.zero_end = o;
    c.pass_rows = genb_pass_rows(R, N, req);
    c.max_passes = (uint32_t)(((unsigned long long)R * (unsigned long long)N + c.pass_rows - 1) / c.pass_rows);
    c.dfeat = take((size_t)R * N * 4);
    c.pcnt = take((size_t)c.max_passes * 4);
    c.ldg = (int)((fc + 127) / 128 * 128); c.ldgf = D <= 32 ? 32 : 128; c.ldX = (c.ncol + 15) / 16 * 16;
    const size_t pr = c.pass_rows;
    if (mlp) {
        c.w1t = take(fc * fc * 4); c.w0t = take(fc * (size_t)c.in0 * 4);
        c.d2 = take(pr * 32 * 4); c.g1 = take(pr * c.ldg * 4); c.g0 = take(pr * c.ldg * 4);
        c.gx = take(pr * (size_t)((c.in0 + 15) / 16 * 16) * 4);
    }
    c.bt = take((size_t)c.ncol * D * 4);
    c.gf = take(pr * c.ldgf * 4); c.X = take(pr * c.ldX * 4); c.gxa = take(pr * c.ldX * 4);
    size_t part = 0;                                      // the largest partial-slab set of the GEMMs (128 rows of M each)
    const int Ns[3] = {(int)fc, c.in0, c.ncol};
    for (int q = 0; q < 3; ++q) {
        if (Ns[q] <= 0) continue;
        const TnPlan p = tn_plan((int64_t)pr, Ns[q]);
        const size_t bytes = (size_t)p.chunks * 128 * p.ldp * 4;
        if (bytes > part) part = bytes;
    }
    c.part = take(part);
    c.csum = take((size_t)kColChunks * (fc > 32 ? fc : 32) * 4);
    c.total = o;
    return c;
}
static int genb_check_desc(const t2n_generic_desc* d, const char* who) {
    if (!d) { set_error("%s: NULL descriptor", who); return T2N_ERR_INVALID; }
    for (int k = 0; k < 3; ++k)
        if (d->grid[k] < 2 || d->density_n_comp[k] < 1 || d->app_n_comp[k] < 1) { set_error("%s: bad grid / component counts", who); return T2N_ERR_INVALID; }
    if (d->app_dim < 1 || d->app_dim > kGenDimMax) { set_error("%s: app_dim %d outside [1, %d]", who, d->app_dim, kGenDimMax); return T2N_ERR_UNSUPPORTED; }
    return T2N_OK;
}

}  // namespace t2n

using namespace t2n;

extern "C" int t2n_generic_backward_plan(const t2n_generic_desc* desc, int64_t n_rays, int n_samples, uint32_t pass_rows, t2n_generic_bwd_plan* out) {
    if (!out) { set_error("t2n_generic_backward_plan: NULL argument"); return T2N_ERR_INVALID; }
    memset(out, 0, sizeof(*out));
    if (int rc = genb_check_desc(desc, "t2n_generic_backward_plan")) return rc;
    if (n_rays <= 0 || n_samples < 1 || (uint64_t)n_rays * (uint64_t)n_samples > 0x7fffffffull) {
        set_error("t2n_generic_backward_plan: %lld rays x %d samples", (long long)n_rays, n_samples);
        return T2N_ERR_INVALID;
    }
    out->pass_rows = genb_pass_rows(n_rays, n_samples, pass_rows);
    out->max_passes = (uint32_t)(((unsigned long long)n_rays * (unsigned long long)n_samples + out->pass_rows - 1) / out->pass_rows);
    out->kernel_form = genb_kernel_form(desc) ? 1 : 0;
    out->workspace_bytes = out->kernel_form ? genb_carve(desc, n_rays, n_samples, pass_rows).total : 0;
    return T2N_OK;
}

extern "C" int t2n_generic_backward_staged(const t2n_generic_desc* desc, const t2n_field_params* params, const float* rays, int64_t n_rays,
                                           int ray_stride, int n_samples, uint32_t flags, const float* jitter, const float* weights,
                                           const float* z_vals, const float* d_rgb, const float* d_depth, const float* d_weights,
                                           const t2n_field_grads* g, void* workspace, size_t workspace_bytes, void* bwd_workspace,
                                           size_t bwd_bytes, uint32_t pass_rows, t2n_stream stream) {
    const char* who = "t2n_generic_backward_staged";
    hipStream_t s = (hipStream_t)stream;
    if (n_rays == 0) return T2N_OK;
    GenArgs a;
    int rc = gen_fill(a, desc, params, who);
    if (rc) return rc;
    if (!g || !d_rgb || !d_depth) { set_error("%s: NULL argument", who); return T2N_ERR_INVALID; }
    if ((rc = gen_bind(a, rays, n_rays, ray_stride, n_samples, flags, jitter, const_cast<float*>(weights), const_cast<float*>(z_vals), workspace,
                       workspace_bytes, who))) return rc;
    const long long tot = (long long)n_rays * n_samples;
    const GenStageCarve sc = gen_stage_carve(desc, n_rays, n_samples, gen_carve(n_rays, n_samples, true).total);
    const bool mlp = genb_is_mlp(desc);
    if (!genb_kernel_form(desc) || sc.total > workspace_bytes || (mlp && !sc.x0)) {
        set_error("%s: this shape (or T2N_GENERIC_PLAIN / T2N_GENERIC_PLAIN_BWD) takes the plain form: call t2n_generic_backward", who);
        return T2N_ERR_UNSUPPORTED;
    }
    const GenBwdCarve c = genb_carve(desc, n_rays, n_samples, pass_rows);
    if (!bwd_workspace || c.total > bwd_bytes) { set_error("%s: backward workspace %zu B < %zu B", who, bwd_bytes, c.total); return T2N_ERR_WORKSPACE; }
    if (c.pass_rows > sc.rows_cap && mlp) { set_error("%s: pass of %u rows beyond the forward's %u", who, c.pass_rows, sc.rows_cap); return T2N_ERR_INVALID; }
    a.d_rgb = d_rgb; a.d_depth = d_depth; a.d_w = d_weights;
    char* ws = (char*)workspace;
    char* bw = (char*)bwd_workspace;
    GenFast fa;
    gen_fast_bind(fa, a, sc, ws, tot);
    GenBwd b;
    memset(&b, 0, sizeof(b));
    for (int k = 0; k < 3; ++k) {
        b.gdp[k] = (float*)(bw + c.g[k]); b.gdl[k] = (float*)(bw + c.g[3 + k]); b.gap[k] = (float*)(bw + c.g[6 + k]); b.gal[k] = (float*)(bw + c.g[9 + k]);
    }
    b.dfeat = (float*)(bw + c.dfeat); b.pcnt = (unsigned*)(bw + c.pcnt); b.pass_rows = c.pass_rows; b.max_passes = c.max_passes;
    b.d2 = (float*)(bw + c.d2); b.g1 = (float*)(bw + c.g1); b.g0 = (float*)(bw + c.g0); b.gx = (float*)(bw + c.gx);
    b.gf = (float*)(bw + c.gf); b.X = (float*)(bw + c.X); b.gxa = (float*)(bw + c.gxa);
    b.x0 = (const float*)(ws + sc.x0); b.h0 = (const float*)(ws + sc.h0); b.h1 = (const float*)(ws + sc.h1);
    b.ldd2 = 32; b.ldg = c.ldg; b.ldx = sc.ldx; b.ldh = sc.ldh; b.ldgf = c.ldgf; b.ldX = c.ldX;
    const float* zb = (const float*)(bw + c.zb);
    float* w1t = (float*)(bw + c.w1t); float* w0t = (float*)(bw + c.w0t); float* bt = (float*)(bw + c.bt);
    float* part = (float*)(bw + c.part); float* csum = (float*)(bw + c.csum);
    HeadPlanDev* plan = (HeadPlanDev*)(ws + sc.plan);
    const int fC = a.fC, in0 = a.in0, D = a.app_dim, ncol = c.ncol;
    auto grid1 = [](long long n) { const long long q = (n + 255) / 256; return dim3((unsigned)(q < 1 ? 1 : (q > 4096 ? 4096 : q))); };

    // ---- everything below only queues work on `s` ----
    T2N_HIP(hipMemsetAsync(bw + c.g[0], 0, c.zero_end - c.g[0], s));
    hipLaunchKernelGGL(k_genb_plan, dim3(1), dim3(256), 0, s, (const unsigned*)fa.count, plan, b.pcnt, c.pass_rows, c.max_passes);
    hipLaunchKernelGGL(k_genb_transpose, grid1((long long)D * ncol), dim3(256), 0, s, a.basis, D, ncol, bt);
    if (mlp) {
        hipLaunchKernelGGL(k_genb_transpose, grid1((long long)fC * fC), dim3(256), 0, s, a.w1, fC, fC, w1t);
        hipLaunchKernelGGL(k_genb_transpose, grid1((long long)fC * in0), dim3(256), 0, s, a.w0, fC, in0, w0t);
    }
    hipLaunchKernelGGL(k_genb_scan, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, s, a, b);
    hipLaunchKernelGGL(k_genb_density, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, a, fa, b);
    const unsigned pr = c.pass_rows;
    const unsigned wgrid = (unsigned)((pr + 3) / 4 < 2048 ? (pr + 3) / 4 : 2048);           // a wave per row, four per workgroup
    // dW [M][N] += A^T B in launches of 128 rows of M (k_gemm_tn<4>), or one of 32 (k_gemm_tn<1>) where M <= 32 and lda == 32
    auto wgrad = [&](const float* A, int lda, int M, const float* B, int ldb, int N, float* Cw, const unsigned* rows_dev) {
        if (!Cw) return;
        if (lda == 32) { launch_gemm_tn(1, true, A, lda, B, ldb, pr, M, N, Cw, N, part, s, nullptr, nullptr, rows_dev); return; }
        for (int m0 = 0; m0 < M; m0 += 128)
            launch_gemm_tn(4, true, A + m0, lda, B, ldb, pr, (M - m0 < 128 ? M - m0 : 128), N, Cw + (size_t)m0 * N, N, part, s, nullptr, nullptr, rows_dev);
    };
    auto bias = [&](const float* G, int ld, int N, float* db, const unsigned* rows_dev) {
        if (!db) return;
        hipLaunchKernelGGL(k_genb_colsum, dim3(kColChunks), dim3(256), 0, s, G, ld, N, rows_dev, csum);
        hipLaunchKernelGGL(k_genb_colsum_reduce, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, (const float*)csum, N, db);
    };
    for (unsigned p = 0; p < c.max_passes; ++p) {
        const long long row0 = (long long)p * pr;
        const unsigned* pc = b.pcnt + p;
        if (mlp) {
            if ((rc = launch_gen_head_pass(a, fa, desc, sc, ws, row0, pr, s))) return rc;
            hipLaunchKernelGGL(k_genb_l2, grid1((long long)pr * (fC > 32 ? fC : 32)), dim3(256), 0, s, a, fa, b, p);
            wgrad(b.d2, 32, 3, b.h1, sc.ldh, fC, g->mlp_w2, pc);
            bias(b.d2, 32, 3, g->mlp_b2, pc);
            wgrad(b.g1, c.ldg, fC, b.h0, sc.ldh, fC, g->mlp_w1, pc);
            bias(b.g1, c.ldg, fC, g->mlp_b1, pc);
            if ((rc = launch_dense_rows(b.g1, c.ldg, w1t, fC, fC, zb, 0, pr, b.g0, c.ldg, s, plan, row0))) return rc;
            hipLaunchKernelGGL(k_genb_mask, grid1((long long)pr * fC), dim3(256), 0, s, b.g0, c.ldg, b.h0, sc.ldh, fC, pc);
            wgrad(b.g0, c.ldg, fC, b.x0, sc.ldx, in0, g->mlp_w0, pc);
            bias(b.g0, c.ldg, fC, g->mlp_b0, pc);
            if ((rc = launch_dense_rows(b.g0, c.ldg, w0t, fC, in0, zb, 0, pr, b.gx, sc.ldx, s, plan, row0))) return rc;
            hipLaunchKernelGGL(k_genb_gfeat, grid1((long long)pr * c.ldgf), dim3(256), 0, s, a, b, p);
        } else
            hipLaunchKernelGGL(k_genb_simple_gf, grid1((long long)pr * c.ldgf), dim3(256), 0, s, a, fa, b, p);
        hipLaunchKernelGGL((k_genb_app<2>), dim3(wgrid), dim3(256), 0, s, a, fa, b, p);
        wgrad(b.gf, c.ldgf, D, b.X, c.ldX, ncol, g->basis_weight, pc);
        if ((rc = launch_dense_rows(b.gf, c.ldgf, bt, D, ncol, zb, 0, pr, b.gxa, c.ldX, s, plan, row0))) return rc;
        hipLaunchKernelGGL((k_genb_app<1>), dim3(wgrid), dim3(256), 0, s, a, fa, b, p);
    }
    GenStageArgs sa;
    unsigned blocks = 0;
    for (int q = 0; q < 4; ++q)
        for (int k = 0; k < 3; ++k) {
            const int idx = q * 3 + k;
            float* dst[4] = {g->density_plane[k], g->density_line[k], g->app_plane[k], g->app_line[k]};
            const long long HW = (long long)desc->grid[mat1(k)] * desc->grid[mat0(k)], L = desc->grid[vecm(k)];
            sa.src[idx] = (const float*)(bw + c.g[idx]); sa.dst[idx] = dst[q]; sa.C[idx] = q < 2 ? a.Cd[k] : a.Ca[k]; sa.HW[idx] = (q & 1) ? L : HW;
            sa.block0[idx] = blocks;
            blocks += (unsigned)(((sa.HW[idx] + 63) / 64) * ((sa.C[idx] + 63) / 64));
        }
    sa.block0[12] = blocks;
    hipLaunchKernelGGL(k_genb_unstage, dim3(blocks), dim3(256), 0, s, sa);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}
