// The support-set builder: what the driver does between inpainting a view and handing training rays to the optimiser
// (text2nerf_main.py:380-392, dataLoader/scene_gen.py:305-316).
//   one-to-many forward warp     utils.py:122-163 (gt_warping, bilinear_splat branch) over scripts/Warper.py:21-180: ONE source
//                                frame splatted to V target poses, every target an independent output (no merge). The arithmetic
//                                is that of k_warp_points / k_warp_splat / k_warp_resolve (t2n_image.hip) in fp64; here the view
//                                index is a grid axis, the V transforms travel by value, the projection is recomputed by the splat
//                                instead of stored, and resolve + white background + / 255 are one kernel.
//   many-to-one forward warp     utils.py:83-119 (bilinear_splat_warping_multiview), for the inpaint-view builder (text2nerf_main.py:129):
//                                V source frames splatted by the same two kernels, the SOURCE on the grid axis and each on its own
//                                canvas, then one resolve per target pixel in which the earliest source wins.
//   formatter                    dataLoader/scene_gen.py:31-98 (produce_formatted_data): rays of N poses and the `mask > 0.5` row
//                                selection in the reference's order (view-major, raster order inside a view): count -> exclusive
//                                scan -> scatter.
#include "t2n_device.h"

namespace t2n {

// ---- one-to-many forward warp -----------------------------------------------------------------------------------------------------
constexpr int kSvViews = 8;            // target views per launch set (the driver's support set has 8)
struct SvMats { double Ki[9], K2[9], T[kSvViews][12]; };

// Warper.py:64-95: X = depth * Ki (x, y, 1); X' = T (X, 1); p = K2 X'  ->  (u, v, z). Called by both passes with the same inputs:
// the library is compiled without contraction, so both see the same bits.
__device__ __forceinline__ void sv_project(const double* Ki, const double* T, const double* K2, int xi, int yi, double d, double& u,
                                           double& v, double& z) {
    const double x = (double)xi, y = (double)yi;
    double cam[3], w2[3], p[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) cam[r] = d * (Ki[r * 3] * x + Ki[r * 3 + 1] * y + Ki[r * 3 + 2] * 1.0);
#pragma unroll
    for (int r = 0; r < 3; ++r) w2[r] = T[r * 4] * cam[0] + T[r * 4 + 1] * cam[1] + T[r * 4 + 2] * cam[2] + T[r * 4 + 3] * 1.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) p[r] = K2[r * 3] * w2[0] + K2[r * 3 + 1] * w2[1] + K2[r * 3 + 2] * w2[2];
    u = p[0] / p[2]; v = p[1] / p[2]; z = p[2];
}

// Both warps below put the view on blockIdx.y with its transform in M.T[view]: one source to V targets (src_stride = 0: every view
// reads the same frame) and V sources to one target (src_stride = H W: view v reads frame v of the stacks; no mask_aux).
// Warper.py:141-143: max over the frame of log(1 + clip(z, 0, 1000)), one value PER VIEW (blockIdx.y). Few workgroups per
// view, each striding over the frame and posting ONE atomic: thousands of atomics on one word serialise (~90 per microsecond).
constexpr int kSvLogmaxBlocks = 128;
__global__ __launch_bounds__(256) void k_sv_logmax(const float* __restrict__ depth, size_t src_stride, int H, int W, const SvMats M,
                                                   unsigned long long* logmax_bits) {
    __shared__ double sm[4];
    const int view = blockIdx.y, n = H * W;
    depth += (size_t)view * src_stride;
    double lg = 0.0;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < n; t += gridDim.x * 256) {
        const int yi = t / W, xi = t - yi * W;
        double u, v, z;
        sv_project(M.Ki, M.T[view], M.K2, xi, yi, (double)depth[t], u, v, z);
        lg = fmax(lg, log(1.0 + fmin(fmax(z, 0.0), 1000.0)));      // fmax drops a NaN operand
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lg = fmax(lg, __shfl_xor(lg, o));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = lg;
    __syncthreads();
    if (threadIdx.x == 0) {
        lg = fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3]));
        if (lg > 0.0) atomicMax(logmax_bits + view, (unsigned long long)__double_as_longlong(lg));   // lg >= 0: bit order = value order
    }
}

// Warper.py:97-166: inverse-bilinear splat of (r, g, b, z) and the weight into the view's (H+2, W+2) canvas with fp64 atomics.
// The canvas is planar — planes of (H+2)(W+2) doubles: r, g, b, z, weight[, aux weight] — so that the lanes of a wave, which hold
// neighbouring source pixels and mostly land on neighbouring target pixels, add to neighbouring doubles of one plane (with an
// interleaved texel every lane's add is a 64-B memory request of its own; DESIGN.md has the measured difference). mask1 scales
// every weight (the reference's mask_gt); mask_aux only feeds the sixth plane: the weight this pixel WOULD carry under
// mask1 = mask_aux, so that `aux weight > 0` is the coverage of a second, masked warp decided as the reference decides it.
__global__ __launch_bounds__(256) void k_sv_splat(const float* __restrict__ rgb, const float* __restrict__ depth,
                                                  const unsigned char* __restrict__ mask1, const unsigned char* __restrict__ mask_aux,
                                                  size_t src_stride, int H, int W, const SvMats M,
                                                  const unsigned long long* __restrict__ logmax_bits, double* canvas, size_t canvas_stride) {
    const int t = blockIdx.x * 256 + threadIdx.x, view = blockIdx.y;
    if (t >= H * W) return;
    rgb += (size_t)view * src_stride * 3; depth += (size_t)view * src_stride;
    if (mask1) mask1 += (size_t)view * src_stride;
    const int yi = t / W, xi = t - yi * W;
    double u, v, z;
    sv_project(M.Ki, M.T[view], M.K2, xi, yi, (double)depth[t], u, v, z);
    const double logmax = __longlong_as_double((long long)logmax_bits[view]);
    double ox = u + 1.0, oy = v + 1.0;
    // floor / ceil -> integer -> clip, in the reference's order (a NaN / huge coordinate clips to the canvas ring)
    const double fxd = floor(ox), fyd = floor(oy), cxd = ceil(ox), cyd = ceil(oy);
    auto to_idx = [](double a, int hi) { if (!(a > 0.0)) return 0; if (a > (double)hi) return hi; return (int)a; };
    const int fx = to_idx(fxd, W + 1), cx = to_idx(cxd, W + 1), fy = to_idx(fyd, H + 1), cy = to_idx(cyd, H + 1);
    ox = fmin(fmax(ox, 0.0), (double)(W + 1)); oy = fmin(fmax(oy, 0.0), (double)(H + 1));
    const double logd = log(1.0 + fmin(fmax(z, 0.0), 1000.0));
    const double dw = exp(logd / logmax * 50.0);
    const double mk = mask1 ? (mask1[t] ? 1.0 : 0.0) : 1.0;
    const double ma = mask_aux ? (mask_aux[t] ? 1.0 : 0.0) : 0.0;
    double val[4];
#pragma unroll
    for (int k = 0; k < 3; ++k) val[k] = (double)(unsigned char)(int)(rgb[(size_t)t * 3 + k] * 255.f);   // (rgb * 255).astype(uint8)
    val[3] = z;
    const int iy[4] = {fy, cy, fy, cy}, ix[4] = {fx, fx, cx, cx};
    const double py[4] = {1.0 - (oy - fy), 1.0 - (cy - oy), 1.0 - (oy - fy), 1.0 - (cy - oy)};
    const double px[4] = {1.0 - (ox - fx), 1.0 - (ox - fx), 1.0 - (cx - ox), 1.0 - (cx - ox)};
    double* cv = canvas + (size_t)view * canvas_stride;
    const size_t plane = (size_t)(H + 2) * (W + 2);
    const bool finite_z = isfinite(z);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double wt = py[q] * px[q] * mk / dw;
        double* c = cv + (size_t)iy[q] * (W + 2) + ix[q];               // iy <= H + 1, ix <= W + 1: inside the plane
        // a zero weight with finite values adds +-0 to sums that start at +0: no bit changes, so the masked-out pixels are skipped
        if (wt != 0.0 || !finite_z) {
#pragma unroll
            for (int k = 0; k < 4; ++k) atomicAdd(c + k * plane, val[k] * wt);
            atomicAdd(c + 4 * plane, wt);
        }
        if (mask_aux) {
            const double wa = py[q] * px[q] * (mk * ma) / dw;
            if (wa != 0.0) atomicAdd(c + 5 * plane, wa);                 // only `> 0` is read from this plane; a NaN weight (dw NaN) is != 0 and is added
        }
    }
}

// Warper.py:168-180 + utils.py:149-155: crop the ring, normalise, clip, round half to even to a uint8 level, white where nothing
// landed, / 255 -> fp32; the mask as integers; the depth in fp64 (0 where nothing landed) and, when asked, rounded to fp32 (what
// produce_formatted_data makes of it). Every output may be NULL except the image.
__global__ __launch_bounds__(256) void k_sv_resolve(const double* __restrict__ canvas, size_t canvas_stride, int nch, int H, int W,
                                                    float* __restrict__ image, long long* __restrict__ mask, double* __restrict__ depth,
                                                    float* __restrict__ depth32, long long* __restrict__ aux) {
    const int t = blockIdx.x * 256 + threadIdx.x, view = blockIdx.y;
    if (t >= H * W) return;
    const int y = t / W, x = t - y * W;
    const size_t plane = (size_t)(H + 2) * (W + 2);
    const double* c = canvas + (size_t)view * canvas_stride + (size_t)(y + 1) * (W + 2) + (x + 1);
    const double w = c[4 * plane];
    const bool known = w > 0.0;
    const size_t o = (size_t)view * H * W + t;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int level = known ? (int)(unsigned char)(int)rint(fmin(fmax(c[k * plane] / w, 0.0), 255.0)) : 255;
        image[o * 3 + k] = (float)((double)level / 255.0);
    }
    const double d = known ? c[3 * plane] / w : 0.0;
    if (mask) mask[o] = known ? 1 : 0;
    if (depth) depth[o] = d;
    if (depth32) depth32[o] = (float)d;
    if (aux) aux[o] = (nch > 5 && c[5 * plane] > 0.0) ? 1 : 0;
}

// ---- many-to-one forward warp: utils.py:83-119 (bilinear_splat_warping_multiview) -----------------------------------------------------
// Every source of the chunk has been splatted into its own planar canvas (k_sv_logmax / k_sv_splat with src_stride = H W). Per
// target pixel: the first source, in ascending order, whose weight is > 0 wins (utils.py:106-113); pixels an earlier chunk filled
// are left alone. `filled` / `image_u8` carry the state between chunks (untouched when one chunk holds every source), `depth` is
// the output itself. The last chunk writes the white background, / 255 -> fp32 and the int64 mask (utils.py:115-118).
__global__ __launch_bounds__(256) void k_ms_resolve(const double* __restrict__ canvas, size_t canvas_stride, int nv, int H, int W,
                                                    int first, int last, unsigned char* filled, unsigned char* image_u8,
                                                    float* __restrict__ image, long long* __restrict__ mask, double* __restrict__ depth) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= H * W) return;
    const int y = t / W, x = t - y * W;
    const size_t plane = (size_t)(H + 2) * (W + 2);
    const double* c0 = canvas + (size_t)(y + 1) * (W + 2) + (x + 1);
    bool known = first ? false : filled[t] != 0;
    bool fresh = false;
    int level[3] = {255, 255, 255};
    if (known && last) {
#pragma unroll
        for (int k = 0; k < 3; ++k) level[k] = image_u8[(size_t)t * 3 + k];
    }
    if (!known) {
        for (int v = 0; v < nv; ++v) {
            const double* c = c0 + (size_t)v * canvas_stride;
            const double w = c[4 * plane];
            if (!(w > 0.0)) continue;
#pragma unroll
            for (int k = 0; k < 3; ++k) level[k] = (int)(unsigned char)(int)rint(fmin(fmax(c[k * plane] / w, 0.0), 255.0));
            depth[t] = c[3 * plane] / w;
            known = fresh = true;
            break;
        }
    }
    if (first && !known) depth[t] = 0.0;
    if (!last) {
        if (first || fresh) {
            filled[t] = known ? 1 : 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) image_u8[(size_t)t * 3 + k] = (unsigned char)level[k];
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) image[(size_t)t * 3 + k] = (float)((double)level[k] / 255.0);
    mask[t] = known ? 1 : 0;
}

// ---- formatter --------------------------------------------------------------------------------------------------------------------
constexpr int kFmtViews = 32;          // poses per launch (by value)
struct FmtPoses { float m[kFmtViews][12]; };

// `mask > 0.5` (scene_gen.py:64) on the dtypes a mask arrives in; for the integer ones that is `>= 1`
__device__ __forceinline__ bool fmt_keep(const void* m, int dtype, size_t i) {
    switch (dtype) {
        case T2N_MASK_U8: return ((const unsigned char*)m)[i] > 0;
        case T2N_MASK_I32: return ((const int*)m)[i] > 0;
        case T2N_MASK_I64: return ((const long long*)m)[i] > 0;
        case T2N_MASK_F32: return ((const float*)m)[i] > 0.5f;
        default: return ((const double*)m)[i] > 0.5;
    }
}

// exclusive prefix of `keep` over the 256 threads of the workgroup in thread order, and the workgroup's total
__device__ __forceinline__ unsigned block_prefix256(bool keep, unsigned* sm4, unsigned& total) {
    const unsigned long long bal = __ballot(keep);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sm4[wave] = (unsigned)__popcll(bal);
    __syncthreads();
    unsigned before = 0;
    for (int w = 0; w < wave; ++w) before += sm4[w];
    total = sm4[0] + sm4[1] + sm4[2] + sm4[3];
    return before + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
}

// pass 1: every view's rays (all_rays_split) and the kept-pixel count of each 256-pixel tile. grid = (tiles, views of this launch)
__global__ __launch_bounds__(256) void k_fmt_rays_count(const void* __restrict__ masks, int mask_dtype, int H, int W, float fx, float fy,
                                                        float cx, float cy, const FmtPoses P, int view0, float* __restrict__ rays_split,
                                                        unsigned* __restrict__ tile_count) {
    __shared__ unsigned sm4[4];
    const int n = H * W, t = blockIdx.x * 256 + threadIdx.x, lv = blockIdx.y, view = view0 + lv;
    if (rays_split && t < n) {
        const int y = t / W, x = t - y * W;
        float rx, ry, rz;
        pixel_ray(P.m[lv], x, y, fx, fy, cx, cy, rx, ry, rz);
        float* r = rays_split + ((size_t)view * n + t) * 6;
        r[0] = P.m[lv][3]; r[1] = P.m[lv][7]; r[2] = P.m[lv][11]; r[3] = rx; r[4] = ry; r[5] = rz;
    }
    if (!tile_count) return;                       // mode 'test': rays only (uniform over the grid)
    const bool keep = t < n && fmt_keep(masks, mask_dtype, (size_t)view * n + t);
    unsigned total;
    block_prefix256(keep, sm4, total);
    if (threadIdx.x == 0) tile_count[(size_t)view * gridDim.x + blockIdx.x] = total;
}

// pass 2: exclusive scan of the tile counts (view-major, tile order = raster order) in one workgroup; record = {K, count per view}
__global__ __launch_bounds__(1024) void k_fmt_scan(const unsigned* __restrict__ tile_count, int n_views, int tiles, long long* tile_off,
                                                   long long* record) {
    __shared__ unsigned ws[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long total = (long long)n_views * tiles;
    long long carry = 0;
    for (long long base = 0; base < total; base += 1024) {
        const long long i = base + tid;
        const unsigned c = i < total ? tile_count[i] : 0u;
        unsigned incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        if (lane == 63) ws[wave] = incl;
        __syncthreads();
        unsigned before = 0, chunk = 0;
        for (int w = 0; w < 16; ++w) { if (w < wave) before += ws[w]; chunk += ws[w]; }
        if (i < total) tile_off[i] = carry + (long long)before + (long long)(incl - c);
        carry += (long long)chunk;
        __syncthreads();
    }
    if (tid == 0) { tile_off[total] = carry; record[0] = carry; }
    __syncthreads();
    for (int v = tid; v < n_views; v += 1024) record[1 + v] = tile_off[(long long)(v + 1) * tiles] - tile_off[(long long)v * tiles];
}

// pass 3: kept pixels to their rows. The ray is recomputed by the function pass 1 used (same bits as all_rays_split[mask]).
__global__ __launch_bounds__(256) void k_fmt_scatter(const float* __restrict__ images, const float* __restrict__ depths,
                                                     const void* __restrict__ masks, int mask_dtype, int H, int W, float fx, float fy,
                                                     float cx, float cy, const FmtPoses P, int view0, const long long* __restrict__ tile_off,
                                                     float* __restrict__ all_rays, float* __restrict__ all_rgbs,
                                                     float* __restrict__ all_depths) {
    __shared__ unsigned sm4[4];
    const int n = H * W, t = blockIdx.x * 256 + threadIdx.x, lv = blockIdx.y, view = view0 + lv;
    const size_t src = (size_t)view * n + t;
    const bool keep = t < n && fmt_keep(masks, mask_dtype, src);
    unsigned total;
    const unsigned before = block_prefix256(keep, sm4, total);
    if (!keep) return;
    const size_t row = (size_t)tile_off[(size_t)view * gridDim.x + blockIdx.x] + before;     // < K <= N H W = the buffers' capacity
    const int y = t / W, x = t - y * W;
    float rx, ry, rz;
    pixel_ray(P.m[lv], x, y, fx, fy, cx, cy, rx, ry, rz);
    float* r = all_rays + row * 6;
    r[0] = P.m[lv][3]; r[1] = P.m[lv][7]; r[2] = P.m[lv][11]; r[3] = rx; r[4] = ry; r[5] = rz;
#pragma unroll
    for (int k = 0; k < 3; ++k) all_rgbs[row * 3 + k] = images[src * 3 + k];
    all_depths[row] = depths[src];
}

}  // namespace t2n

using namespace t2n;

static size_t al256s(size_t x) { return (x + 255) / 256 * 256; }
static size_t sv_canvas_bytes(int H, int W) { return al256s((size_t)(H + 2) * (W + 2) * 6 * sizeof(double)); }

extern "C" size_t t2n_warp_views_workspace_bytes(int H, int W, int V) {
    if (H < 1 || W < 1 || V < 1 || (long long)H * W > (1ll << 30)) return 0;
    return sv_canvas_bytes(H, W) * (size_t)(V < kSvViews ? V : kSvViews) + 256;
}

extern "C" int t2n_warp_views(const float* rgb, const float* depth, const uint8_t* mask1, const uint8_t* mask_aux, int H, int W, int V,
                              const double* Ki9_host, const double* T12_host, const double* K9_host, float* image_out, int64_t* mask_out,
                              double* depth_out, float* depth32_out, int64_t* aux_out, void* workspace, size_t workspace_bytes,
                              t2n_stream stream) {
    if (!rgb || !depth || !Ki9_host || !T12_host || !K9_host || !image_out || !workspace || H < 1 || W < 1 || V < 1 ||
        (long long)H * W > (1ll << 30)) {
        set_error("t2n_warp_views: bad argument");
        return T2N_ERR_INVALID;
    }
    if (aux_out && !mask_aux) { set_error("t2n_warp_views: aux_out without mask_aux"); return T2N_ERR_INVALID; }
    if (workspace_bytes < t2n_warp_views_workspace_bytes(H, W, V)) { set_error("t2n_warp_views: workspace too small"); return T2N_ERR_WORKSPACE; }
    hipStream_t s = (hipStream_t)stream;
    const int n = H * W, nch = mask_aux ? 6 : 5;
    const size_t cbytes = sv_canvas_bytes(H, W), cstride = cbytes / sizeof(double);
    const unsigned nb = (unsigned)((n + 255) / 256);
    SvMats M;
    memcpy(M.Ki, Ki9_host, sizeof(M.Ki)); memcpy(M.K2, K9_host, sizeof(M.K2));
    for (int v0 = 0; v0 < V; v0 += kSvViews) {
        const int nv = V - v0 < kSvViews ? V - v0 : kSvViews;
        memset(M.T, 0, sizeof(M.T));
        memcpy(M.T, T12_host + (size_t)v0 * 12, (size_t)nv * 12 * sizeof(double));
        double* canvas = (double*)workspace;
        unsigned long long* logmax = (unsigned long long*)((char*)workspace + cbytes * nv);
        T2N_HIP(hipMemsetAsync(workspace, 0, cbytes * nv + 256, s));
        const size_t o = (size_t)v0 * n;
        hipLaunchKernelGGL(k_sv_logmax, dim3(nb < (unsigned)kSvLogmaxBlocks ? nb : (unsigned)kSvLogmaxBlocks, (unsigned)nv), dim3(256), 0, s, depth, (size_t)0, H, W, M, logmax);
        hipLaunchKernelGGL(k_sv_splat, dim3(nb, (unsigned)nv), dim3(256), 0, s, rgb, depth, mask1, mask_aux, (size_t)0, H, W, M,
                           (const unsigned long long*)logmax, canvas, cstride);
        hipLaunchKernelGGL(k_sv_resolve, dim3(nb, (unsigned)nv), dim3(256), 0, s, (const double*)canvas, cstride, nch, H, W,
                           image_out + o * 3, (long long*)(mask_out ? mask_out + o : nullptr), depth_out ? depth_out + o : nullptr,
                           depth32_out ? depth32_out + o : nullptr, (long long*)(aux_out ? aux_out + o : nullptr));
    }
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

static size_t ms_canvas_bytes(int H, int W) { return al256s((size_t)(H + 2) * (W + 2) * 5 * sizeof(double)); }

extern "C" size_t t2n_warp_sources_workspace_bytes(int H, int W, int V) {
    if (H < 1 || W < 1 || V < 1 || (long long)H * W > (1ll << 30)) return 0;
    const size_t n = (size_t)H * W;      // canvases of one chunk | per-source log-depth maxima | filled | image_u8
    return ms_canvas_bytes(H, W) * (size_t)(V < kSvViews ? V : kSvViews) + 256 + al256s(n) + al256s(n * 3);
}

extern "C" int t2n_warp_sources(const float* rgb, const float* depth, const uint8_t* mask1, int H, int W, int V, const double* Ki9_host,
                                const double* T12_host, const double* K9_host, float* image_out, int64_t* mask_out, double* depth_out,
                                void* workspace, size_t workspace_bytes, t2n_stream stream) {
    if (!rgb || !depth || !Ki9_host || !T12_host || !K9_host || !image_out || !mask_out || !depth_out || !workspace || H < 1 || W < 1 ||
        V < 1 || (long long)H * W > (1ll << 30)) {
        set_error("t2n_warp_sources: bad argument");
        return T2N_ERR_INVALID;
    }
    if (workspace_bytes < t2n_warp_sources_workspace_bytes(H, W, V)) { set_error("t2n_warp_sources: workspace too small"); return T2N_ERR_WORKSPACE; }
    hipStream_t s = (hipStream_t)stream;
    const int n = H * W, chunk = V < kSvViews ? V : kSvViews;
    const size_t cbytes = ms_canvas_bytes(H, W), cstride = cbytes / sizeof(double);
    const unsigned nb = (unsigned)((n + 255) / 256);
    double* canvas = (double*)workspace;
    unsigned long long* logmax = (unsigned long long*)((char*)workspace + cbytes * chunk);
    unsigned char* filled = (unsigned char*)workspace + cbytes * chunk + 256;
    unsigned char* image_u8 = filled + al256s((size_t)n);
    SvMats M;
    memcpy(M.Ki, Ki9_host, sizeof(M.Ki)); memcpy(M.K2, K9_host, sizeof(M.K2));
    for (int v0 = 0; v0 < V; v0 += kSvViews) {
        const int nv = V - v0 < kSvViews ? V - v0 : kSvViews;
        memset(M.T, 0, sizeof(M.T));
        memcpy(M.T, T12_host + (size_t)v0 * 12, (size_t)nv * 12 * sizeof(double));
        T2N_HIP(hipMemsetAsync(workspace, 0, cbytes * chunk + 256, s));      // canvases and maxima (contiguous)
        const size_t o = (size_t)v0 * n;
        hipLaunchKernelGGL(k_sv_logmax, dim3(nb < (unsigned)kSvLogmaxBlocks ? nb : (unsigned)kSvLogmaxBlocks, (unsigned)nv), dim3(256), 0, s,
                           depth + o, (size_t)n, H, W, M, logmax);
        hipLaunchKernelGGL(k_sv_splat, dim3(nb, (unsigned)nv), dim3(256), 0, s, rgb + o * 3, depth + o, mask1 ? mask1 + o : nullptr,
                           (const unsigned char*)nullptr, (size_t)n, H, W, M, (const unsigned long long*)logmax, canvas, cstride);
        hipLaunchKernelGGL(k_ms_resolve, dim3(nb), dim3(256), 0, s, (const double*)canvas, cstride, nv, H, W, v0 == 0 ? 1 : 0,
                           v0 + nv == V ? 1 : 0, filled, image_u8, image_out, (long long*)mask_out, depth_out);
    }
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" size_t t2n_format_views_workspace_bytes(int H, int W, int N) {
    if (H < 1 || W < 1 || N < 1 || (long long)H * W > (1ll << 30)) return 0;
    const size_t tiles = ((size_t)H * W + 255) / 256;
    return al256s(tiles * N * sizeof(unsigned)) + al256s((tiles * N + 1) * sizeof(long long));
}

extern "C" int t2n_format_views(const float* images, const float* depths, const void* masks, int mask_dtype, int N, int H, int W,
                                const float* c2w_host, float fx, float fy, float cx, float cy, float* rays_split, float* all_rays,
                                float* all_rgbs, float* all_depths, int64_t capacity_rows, int64_t* record, void* workspace,
                                size_t workspace_bytes, t2n_stream stream) {
    if (!c2w_host || N < 1 || H < 1 || W < 1 || (long long)H * W > (1ll << 30) || (!masks && !rays_split)) {
        set_error("t2n_format_views: bad argument");
        return T2N_ERR_INVALID;
    }
    const bool select = masks != nullptr;
    if (select) {
        if (!images || !depths || !all_rays || !all_rgbs || !all_depths || !record || !workspace) {
            set_error("t2n_format_views: the row selection needs images, depths, the three row buffers, the record and a workspace");
            return T2N_ERR_INVALID;
        }
        if (mask_dtype < T2N_MASK_U8 || mask_dtype > T2N_MASK_F64) { set_error("t2n_format_views: unknown mask dtype %d", mask_dtype); return T2N_ERR_INVALID; }
        if (capacity_rows < (int64_t)N * H * W) { set_error("t2n_format_views: row buffers must hold N*H*W rows"); return T2N_ERR_INVALID; }
        if (workspace_bytes < t2n_format_views_workspace_bytes(H, W, N)) { set_error("t2n_format_views: workspace too small"); return T2N_ERR_WORKSPACE; }
    }
    hipStream_t s = (hipStream_t)stream;
    const unsigned tiles = (unsigned)(((size_t)H * W + 255) / 256);
    unsigned* tile_count = select ? (unsigned*)workspace : nullptr;
    long long* tile_off = select ? (long long*)((char*)workspace + al256s((size_t)tiles * N * sizeof(unsigned))) : nullptr;
    FmtPoses P;
    for (int pass = 0; pass < (select ? 2 : 1); ++pass) {
        for (int v0 = 0; v0 < N; v0 += kFmtViews) {
            const int nv = N - v0 < kFmtViews ? N - v0 : kFmtViews;
            memset(&P, 0, sizeof(P));
            memcpy(P.m, c2w_host + (size_t)v0 * 12, (size_t)nv * 12 * sizeof(float));
            if (pass == 0)
                hipLaunchKernelGGL(k_fmt_rays_count, dim3(tiles, (unsigned)nv), dim3(256), 0, s, masks, mask_dtype, H, W, fx, fy, cx, cy, P,
                                   v0, rays_split, tile_count);
            else
                hipLaunchKernelGGL(k_fmt_scatter, dim3(tiles, (unsigned)nv), dim3(256), 0, s, images, depths, masks, mask_dtype, H, W, fx,
                                   fy, cx, cy, P, v0, (const long long*)tile_off, all_rays, all_rgbs, all_depths);
        }
        if (pass == 0 && select)
            hipLaunchKernelGGL(k_fmt_scan, dim3(1), dim3(1024), 0, s, (const unsigned*)tile_count, N, (int)tiles, tile_off,
                               (long long*)record);
    }
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}
