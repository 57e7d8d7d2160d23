// Image metrics of the evaluation loops on the device.
//   rgb_ssim   utils.py:436-482 (used by renderer.py:103-109 and extra/compute_metrics.py:34-80,151-162): five Gaussian-windowed
//              moments per pixel and channel (30 scipy.signal.convolve2d calls per frame on the host in the reference), the SSIM
//              formula, the mean of the map. Optionally the squared-error sum of the PSNR (renderer.py:98) from the same loads.
// Arithmetic contract: scipy widens a float32 image to float64 when it convolves it with the float64 filter, so every window sum and
// everything after it is float64 here; the products a*a, b*b, a*b (and the difference of the squared error) are formed in the INPUT's
// dtype first, as `img0**2` / `img0 * img1` are in the reference, and widened afterwards. Two instantiations: float32 and float64 inputs.
// No floating-point atomics: a tile's sum is reduced in a fixed tree, the tiles of a view by a second one-workgroup launch in a
// fixed order, so the result is bit-repeatable and a view inside a stack is bit-equal to the same view alone.
#include "t2n_internal.h"

namespace t2n {

constexpr int kSsimT = 16;                         // output pixels per tile edge (metrics._TILE)
constexpr int kSsimMaxF = 33;                      // filter taps (compile-time cap: sizes the LDS stage and the by-value tap array)
constexpr int kSsimS = kSsimT + kSsimMaxF - 1;     // 48: halo tile edge at the cap AND the stage's row pitch for every filter size
struct SsimTaps { double w[kSsimMaxF]; };          // w[j] = filt[fs-1-j]: the "valid" convolution as a correlation

template <typename T> __device__ __forceinline__ T ssim_clamp01(T x) { return x < (T)0 ? (T)0 : (x > (T)1 ? (T)1 : x); }   // keeps NaN, like torch.clamp

// fixed-order tree over the 256 lanes' values; the result is valid in thread 0. `buf` holds 256 doubles.
__device__ __forceinline__ double ssim_block_sum(double v, double* buf) {
    __syncthreads();
    buf[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) buf[threadIdx.x] += buf[threadIdx.x + s];
        __syncthreads();
    }
    return buf[0];
}

// One workgroup = one 16x16 tile of output pixels of one view (blockIdx.z), channel by channel:
//   stage   the (16+fs-1)^2 halo of both images in the input dtype, row pitch 48 elements (zero outside the image; clamp and the
//           squared-error sum happen here: a pixel is summed by the tile whose 16x16 origin block holds it, edge tiles own through the
//           image border)
//   rows    the horizontal pass of the five quantities a, b, a*a, b*b, a*b: (16+fs-1) rows x 16 columns, <= 3 positions per thread,
//           kept in registers until every lane has finished reading the stage, then written over it as [5][rows][16] doubles
//   columns the vertical pass, one output pixel per thread, then the formula
// LDS: max(2 * 48 * 48 * sizeof(T), 5 * 48 * 16 * 8) = 36 KiB (the float64 stage), so four workgroups fit a CU's 160 KiB.
// Banks: a 32-lane group reads two tile rows of 16 consecutive elements; with the pitch of 48 elements the second row starts 16 (4-byte
// banks of 32) resp. 32 dwords (8-byte reads, banks of 64) after the first: conflict-free in both dtypes. The [.][16] double rows
// of the second image are contiguous for the 32 lanes.
template <typename T>
__global__ __launch_bounds__(256) void k_ssim_tiles(const T* __restrict__ img0, const T* __restrict__ img1, int H, int W, int fs,
                                                     const SsimTaps taps, double c1, double c2, int clamp0, double* __restrict__ map,
                                                     double* __restrict__ part_ssim, double* __restrict__ part_sq) {
    __shared__ double smem[2 * kSsimS * kSsimS];
    T* sa = (T*)smem;
    T* sb = sa + kSsimS * kSsimS;
    const int S = kSsimT + fs - 1, OH = H - fs + 1, OW = W - fs + 1;
    const int bx = blockIdx.x * kSsimT, by = blockIdx.y * kSsimT;
    const bool last_x = blockIdx.x == gridDim.x - 1, last_y = blockIdx.y == gridDim.y - 1;
    const size_t view = blockIdx.z;
    img0 += view * (size_t)H * W * 3;
    img1 += view * (size_t)H * W * 3;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const bool live = bx + tx < OW && by + ty < OH;
    double sum = 0.0, sq = 0.0;
    for (int c = 0; c < 3; ++c) {
        __syncthreads();                                     // the previous channel's column pass has read the LDS
        for (int i = tid; i < S * S; i += 256) {
            const int ly = i / S, lx = i - ly * S;
            const int y = by + ly, x = bx + lx;
            T a = (T)0, b = (T)0;
            if (y < H && x < W) {
                const size_t o = ((size_t)y * W + x) * 3 + c;
                a = img0[o]; b = img1[o];
                if (clamp0) a = ssim_clamp01(a);
                if (part_sq && (lx < kSsimT || last_x) && (ly < kSsimT || last_y)) {
                    const T d = a - b;
                    const T d2 = d * d;
                    sq += (double)d2;
                }
            }
            sa[ly * kSsimS + lx] = a; sb[ly * kSsimS + lx] = b;
        }
        __syncthreads();
        double acc[3][5];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int p = tid + k * 256;                     // row p / 16 of the halo, output column p % 16
            for (int q = 0; q < 5; ++q) acc[k][q] = 0.0;
            if (p < S * kSsimT) {
                const int o = (p >> 4) * kSsimS + (p & 15);
                for (int j = 0; j < fs; ++j) {
                    const T a = sa[o + j], b = sb[o + j];
                    const T aa = a * a, bb = b * b, ab = a * b;          // in the input dtype, then widened
                    const double w = taps.w[j];
                    acc[k][0] += w * (double)a;  acc[k][1] += w * (double)b;
                    acc[k][2] += w * (double)aa; acc[k][3] += w * (double)bb; acc[k][4] += w * (double)ab;
                }
            }
        }
        __syncthreads();                                     // every lane is done with the stage: the row sums go over it
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int p = tid + k * 256;
            if (p < S * kSsimT)
                for (int q = 0; q < 5; ++q) smem[q * (kSsimS * kSsimT) + p] = acc[k][q];
        }
        __syncthreads();
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j < fs; ++j) {
            const double w = taps.w[j];
            const int o = (ty + j) * kSsimT + tx;
            for (int q = 0; q < 5; ++q) m[q] += w * smem[q * (kSsimS * kSsimT) + o];
        }
        if (live) {
            const double mu00 = m[0] * m[0], mu11 = m[1] * m[1], mu01 = m[0] * m[1];
            double s00 = m[2] - mu00, s11 = m[3] - mu11, s01 = m[4] - mu01;
            s00 = s00 < 0.0 ? 0.0 : s00;                     // np.maximum(0., .): NaN stays NaN
            s11 = s11 < 0.0 ? 0.0 : s11;
            const double lim = sqrt(s00 * s11), mag = fabs(s01);
            const double sgn = s01 > 0.0 ? 1.0 : (s01 < 0.0 ? -1.0 : s01);
            s01 = sgn * (lim < mag ? lim : mag);
            const double numer = (2.0 * mu01 + c1) * (2.0 * s01 + c2);
            const double denom = (mu00 + mu11 + c1) * (s00 + s11 + c2);
            const double val = numer / denom;
            sum += val;
            if (map) map[((view * OH + (by + ty)) * (size_t)OW + (bx + tx)) * 3 + c] = val;
        }
    }
    const size_t tile = (view * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const double s = ssim_block_sum(sum, smem);
    if (tid == 0) part_ssim[tile] = s;
    if (part_sq) {
        const double e = ssim_block_sum(sq, smem);
        if (tid == 0) part_sq[tile] = e;
    }
}

// The tiles of one view (blockIdx.x) in a fixed order: lane l sums tiles l, l + 256, ..., then the tree.
__global__ __launch_bounds__(256) void k_ssim_reduce(const double* __restrict__ part_ssim, const double* __restrict__ part_sq, int tiles,
                                                      double count, double* __restrict__ ssim, double* __restrict__ sq_err) {
    __shared__ double buf[256];
    const size_t base = (size_t)blockIdx.x * tiles;
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < tiles; i += 256) {
        a += part_ssim[base + i];
        if (part_sq) b += part_sq[base + i];
    }
    const double s = ssim_block_sum(a, buf);
    if (threadIdx.x == 0) ssim[blockIdx.x] = s / count;
    if (part_sq) {
        const double e = ssim_block_sum(b, buf);
        if (threadIdx.x == 0) sq_err[blockIdx.x] = e;
    }
}

}  // namespace t2n

using namespace t2n;

constexpr int kSsimMaxViews = 65535;      // the view is grid axis z
constexpr int kSsimMaxEdge = 32768;       // image edge: keeps tiles per view and every grid axis in int range

static bool ssim_shape_ok(int V, int H, int W, int fs) {
    return V >= 1 && V <= kSsimMaxViews && fs >= 1 && fs <= kSsimMaxF && H >= fs && W >= fs && H <= kSsimMaxEdge && W <= kSsimMaxEdge;
}
static size_t ssim_tiles(int H, int W, int fs) {
    return (size_t)((W - fs + 1 + kSsimT - 1) / kSsimT) * (size_t)((H - fs + 1 + kSsimT - 1) / kSsimT);
}
static size_t ssim_al256(size_t x) { return (x + 255) / 256 * 256; }

extern "C" size_t t2n_ssim_views_workspace_bytes(int V, int H, int W, int filter_size) {
    if (!ssim_shape_ok(V, H, W, filter_size)) return 0;
    return 2 * ssim_al256((size_t)V * ssim_tiles(H, W, filter_size) * sizeof(double));
}

extern "C" int t2n_ssim_views(const void* img0, const void* img1, int dtype, int V, int H, int W, const double* filter_host, int filter_size,
                              double c1, double c2, int clamp01_img0, double* ssim, double* ssim_map, double* sq_err, void* workspace,
                              size_t workspace_bytes, t2n_stream stream) {
    if (!img0 || !img1 || !filter_host || !ssim || !workspace) { set_error("t2n_ssim_views: NULL argument"); return T2N_ERR_INVALID; }
    if (dtype != 0 && dtype != 1) { set_error("t2n_ssim_views: dtype %d is neither 0 (float32) nor 1 (float64)", dtype); return T2N_ERR_INVALID; }
    if (filter_size < 1 || filter_size > kSsimMaxF) {
        set_error("t2n_ssim_views: filter_size %d outside 1..%d", filter_size, kSsimMaxF);
        return T2N_ERR_INVALID;
    }
    if (!ssim_shape_ok(V, H, W, filter_size)) {
        set_error("t2n_ssim_views: V %d, H %d, W %d with a %d-tap filter (needs V >= 1, H and W >= filter_size, V <= %d, H and W <= %d)", V, H, W,
                  filter_size, kSsimMaxViews, kSsimMaxEdge);
        return T2N_ERR_INVALID;
    }
    if (workspace_bytes < t2n_ssim_views_workspace_bytes(V, H, W, filter_size)) {
        set_error("t2n_ssim_views: workspace of %zu bytes, needs %zu", workspace_bytes, t2n_ssim_views_workspace_bytes(V, H, W, filter_size));
        return T2N_ERR_INVALID;
    }
    SsimTaps taps;
    for (int j = 0; j < kSsimMaxF; ++j) taps.w[j] = j < filter_size ? filter_host[filter_size - 1 - j] : 0.0;
    const int OH = H - filter_size + 1, OW = W - filter_size + 1;
    const int tiles = (int)ssim_tiles(H, W, filter_size);
    double* part_ssim = (double*)workspace;
    double* part_sq = sq_err ? (double*)((char*)workspace + ssim_al256((size_t)V * tiles * sizeof(double))) : nullptr;
    const dim3 grid((unsigned)((OW + kSsimT - 1) / kSsimT), (unsigned)((OH + kSsimT - 1) / kSsimT), (unsigned)V);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == 0)
        hipLaunchKernelGGL(k_ssim_tiles<float>, grid, dim3(256), 0, s, (const float*)img0, (const float*)img1, H, W, filter_size, taps, c1, c2,
                           clamp01_img0, ssim_map, part_ssim, part_sq);
    else
        hipLaunchKernelGGL(k_ssim_tiles<double>, grid, dim3(256), 0, s, (const double*)img0, (const double*)img1, H, W, filter_size, taps, c1,
                           c2, clamp01_img0, ssim_map, part_ssim, part_sq);
    hipLaunchKernelGGL(k_ssim_reduce, dim3((unsigned)V), dim3(256), 0, s, (const double*)part_ssim, (const double*)part_sq, tiles,
                       (double)OH * (double)OW * 3.0, ssim, sq_err);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}
