// The depth stage of a new view, between the inpainter and the support set of `render_warping_inapinting`
// (text2nerf_main.py:147-162 and :230-299): everything there that is not a network, as small index / elementwise / stencil kernels:
//   filled-pixel list      :233-239   the column-major list of the pixels with myMap_filt > 0, addressed by rank (count, scan, select)
//   merge-network inputs   :275-276   depth_ref (float64 arithmetic, rounded once), depth_src (float32 arithmetic), the float32 mask
//   after the network      :278-299   depth_new, img_new, current_mask_inpainted
//   mask expansion         :147-162   the update_known_views=True erosion of myMap_filt (cv2.blur 5x5 > 0.99 = a 25-tap AND)
// The library is built without floating-point contraction: every product and sum below rounds on its own, as numpy's do.
#include "t2n_internal.h"

namespace t2n {

// ---- filled pixels ----------------------------------------------------------------------------------------------------------------
// Order of the list (:234-237): column ascending, inside a column row ascending; entries are (row, col). Workspace: int32 offsets
// [W + 1], offsets[c] = number of filled pixels in the columns before c, offsets[W] = the total.
constexpr int kFpCols = 64, kFpSlices = 4;

// 64 columns per workgroup, the rows dealt to four slices: reads are coalesced along a row; the slice sums meet in LDS
__global__ __launch_bounds__(256) void k_fp_count(const int* __restrict__ known, int H, int W, int* __restrict__ counts) {
    __shared__ int part[kFpSlices][kFpCols];
    const int lc = threadIdx.x & (kFpCols - 1), sl = threadIdx.x >> 6;
    const int c = blockIdx.x * kFpCols + lc;
    int n = 0;
    if (c < W)
        for (int y = sl; y < H; y += kFpSlices) n += known[(size_t)y * W + c] > 0 ? 1 : 0;
    part[sl][lc] = n;
    __syncthreads();
    if (sl == 0 && c < W) counts[c] = part[0][lc] + part[1][lc] + part[2][lc] + part[3][lc];
}

// exclusive scan of counts[0..W) in place, in chunks of 1024 with a running carry; counts[W] and *total receive the sum
__global__ __launch_bounds__(1024) void k_fp_scan(int* __restrict__ counts, int W, long long* __restrict__ total) {
    __shared__ int sm[1024];
    const int t = threadIdx.x;
    int carry = 0;
    for (int base = 0; base < W; base += 1024) {
        const int i = base + t;
        const int own = i < W ? counts[i] : 0;
        sm[t] = own;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int add = t >= o ? sm[t - o] : 0;
            __syncthreads();
            sm[t] += add;
            __syncthreads();
        }
        if (i < W) counts[i] = carry + sm[t] - own;
        carry += sm[1023];
        __syncthreads();
    }
    if (t == 0) { counts[W] = carry; *total = carry; }
}

// one wave per rank: the column by binary search in the offsets, then a ballot / popcount walk down that column, 64 rows a step.
// A rank outside [0, total) writes (-1, -1).
__global__ __launch_bounds__(256) void k_fp_select(const int* __restrict__ known, int H, int W, const int* __restrict__ offsets,
                                                   const int* __restrict__ ranks, int K, int* __restrict__ pixel_yx) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= K) return;                                       // wave-uniform
    const int r = ranks[k];
    if (r < 0 || r >= offsets[W]) {
        if (lane == 0) { pixel_yx[2 * k] = -1; pixel_yx[2 * k + 1] = -1; }
        return;
    }
    int lo = 0, hi = W;                                       // the column c with offsets[c] <= r < offsets[c + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= r) lo = mid; else hi = mid;
    }
    const int c = lo;
    int rem = r - offsets[c];                                 // set pixels of the column above the one looked for
    for (int y0 = 0; y0 < H; y0 += 64) {
        const int y = y0 + lane;
        const bool set = y < H && known[(size_t)y * W + c] > 0;
        const unsigned long long m = __ballot(set);
        const int n = __popcll(m);
        if (rem < n) {
            if (set && __popcll(m & ((1ull << lane) - 1ull)) == rem) { pixel_yx[2 * k] = y; pixel_yx[2 * k + 1] = c; }
            return;
        }
        rem -= n;
    }
}

// ---- the merge network's inputs (:275-276) ---------------------------------------------------------------------------------------
// depth_ref: float64 throughout (depth_rendered is float64, the mask an integer map), rounded to float32 once; the product with the
// mask is a product, so that a masked-out pixel keeps the sign numpy gives its zero. depth_src: float32 operation by operation
// (numpy keeps float32 against Python scalars).
__global__ __launch_bounds__(256) void k_depth_merge_inputs(const double* __restrict__ depth_rendered, const int* __restrict__ known,
                                                            const float* __restrict__ depth_shift, long long n, double push,
                                                            float* __restrict__ depth_ref, float* __restrict__ depth_src,
                                                            float* __restrict__ mask) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int m = known[i] != 0 ? 1 : 0;
    const double a = (depth_rendered[i] - push) * 12000.0;
    const double b = a / 32768.0;
    depth_ref[i] = (float)((b - 1.0) * (double)m);
    const float pf = (float)push;
    const float s0 = (depth_shift[i] - pf) * 12000.f;
    const float s1 = s0 / 32768.f;
    depth_src[i] = s1 - 1.f;
    mask[i] = (float)m;
}

// ---- after the merge network (:278, :282, :285, :296) --------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_view_finish(const float* __restrict__ depth_merged, const unsigned char* __restrict__ img_u8,
                                                     const int* __restrict__ known, long long n, float push, float* __restrict__ depth_new,
                                                     float* __restrict__ img_new, long long* __restrict__ mask_inpainted) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float a = depth_merged[i] + 1.f;
    const float b = a * 32768.f;
    const float c = b / 12000.f;
    depth_new[i] = c + push;
#pragma unroll
    for (int k = 0; k < 3; ++k) img_new[i * 3 + k] = (float)((double)img_u8[i * 3 + k] / 255.0);
    mask_inpainted[i] = known[i] != 0 ? 0 : 1;
}

// ---- mask expansion (:147-162) ------------------------------------------------------------------------------------------------------
// cv2.blur(float32 map, (5,5)) > 0.99 with the default border (BORDER_REFLECT_101): 25/25 is >= 0.9999 and 24/25 is 0.96 in any
// summation order, so the pixel survives iff all 25 taps are set. 16x16 pixels per workgroup, the (16+4)^2 tile in LDS, loaded
// through the reflected indices. mask_ex = the removed ring (map - eroded) on three channels.
constexpr int kExT = 16, kExHalo = 2, kExS = kExT + 2 * kExHalo;
__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }
__global__ __launch_bounds__(256) void k_mask_expand(const int* __restrict__ known, int H, int W, int* __restrict__ eroded,
                                                     long long* __restrict__ mask_ex) {
    __shared__ unsigned char tile[kExS * kExS];
    const int bx = blockIdx.x * kExT, by = blockIdx.y * kExT;
    for (int i = threadIdx.x; i < kExS * kExS; i += 256) {
        const int ly = i / kExS, lx = i - ly * kExS;
        // a tile that overhangs the image reads clamped positions there; no pixel inside the image uses them
        const int y = reflect101(min(by + ly - kExHalo, H + 1), H), x = reflect101(min(bx + lx - kExHalo, W + 1), W);
        tile[i] = known[(size_t)y * W + x] != 0 ? 1 : 0;
    }
    __syncthreads();
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int x = bx + tx, y = by + ty;
    if (x >= W || y >= H) return;
    int all = 1;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy)
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) all &= tile[(ty + dy) * kExS + tx + dx];
    const int self = tile[(ty + kExHalo) * kExS + tx + kExHalo];
    const size_t o = (size_t)y * W + x;
    eroded[o] = all;
    const long long ring = self - all;
#pragma unroll
    for (int k = 0; k < 3; ++k) mask_ex[o * 3 + k] = ring;
}

}  // namespace t2n

using namespace t2n;

static bool fp_shape_ok(int H, int W) { return H >= 1 && W >= 1 && (long long)H * W < (1ll << 31); }

extern "C" size_t t2n_filled_pixels_workspace_bytes(int H, int W) {
    if (!fp_shape_ok(H, W)) return 0;
    return ((size_t)(W + 1) * 4 + 255) / 256 * 256;
}

extern "C" int t2n_filled_pixels_count(const int32_t* known, int H, int W, void* workspace, int64_t* count_out, t2n_stream stream) {
    if (!known || !workspace || !count_out || !fp_shape_ok(H, W)) { set_error("t2n_filled_pixels_count: bad argument"); return T2N_ERR_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    int* offsets = (int*)workspace;
    hipLaunchKernelGGL(k_fp_count, dim3((unsigned)((W + kFpCols - 1) / kFpCols)), dim3(256), 0, s, known, H, W, offsets);
    hipLaunchKernelGGL(k_fp_scan, dim3(1), dim3(1024), 0, s, offsets, W, (long long*)count_out);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" int t2n_filled_pixels_select(const int32_t* known, int H, int W, const void* workspace, const int32_t* ranks, int K,
                                        int32_t* pixel_yx, t2n_stream stream) {
    if (!known || !workspace || K < 0 || (K > 0 && (!ranks || !pixel_yx)) || !fp_shape_ok(H, W)) {
        set_error("t2n_filled_pixels_select: bad argument");
        return T2N_ERR_INVALID;
    }
    if (K == 0) return T2N_OK;
    hipLaunchKernelGGL(k_fp_select, dim3((unsigned)((K + 3) / 4)), dim3(256), 0, (hipStream_t)stream, known, H, W, (const int*)workspace,
                       ranks, K, pixel_yx);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" int t2n_depth_merge_inputs(const double* depth_rendered, const int32_t* known, const float* depth_shift, int H, int W,
                                      double push_depth, float* depth_ref, float* depth_src, float* mask, t2n_stream stream) {
    if (!depth_rendered || !known || !depth_shift || !depth_ref || !depth_src || !mask || !fp_shape_ok(H, W)) {
        set_error("t2n_depth_merge_inputs: bad argument");
        return T2N_ERR_INVALID;
    }
    const long long n = (long long)H * W;
    hipLaunchKernelGGL(k_depth_merge_inputs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, depth_rendered, known,
                       depth_shift, n, push_depth, depth_ref, depth_src, mask);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" int t2n_view_finish(const float* depth_merged, const uint8_t* img_u8, const int32_t* known, int H, int W, double push_depth,
                               float* depth_new, float* img_new, int64_t* mask_inpainted, t2n_stream stream) {
    if (!depth_merged || !img_u8 || !known || !depth_new || !img_new || !mask_inpainted || !fp_shape_ok(H, W)) {
        set_error("t2n_view_finish: bad argument");
        return T2N_ERR_INVALID;
    }
    const long long n = (long long)H * W;
    hipLaunchKernelGGL(k_view_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, depth_merged, img_u8, known, n,
                       (float)push_depth, depth_new, img_new, (long long*)mask_inpainted);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" int t2n_mask_expand(const int32_t* known, int H, int W, int32_t* eroded, int64_t* mask_ex, t2n_stream stream) {
    if (!known || !eroded || !mask_ex || known == eroded || H < 3 || W < 3 || !fp_shape_ok(H, W)) {   // reflect-101 of a 5x5 window needs 3 pixels
        set_error("t2n_mask_expand: bad argument");
        return T2N_ERR_INVALID;
    }
    hipLaunchKernelGGL(k_mask_expand, dim3((unsigned)((W + kExT - 1) / kExT), (unsigned)((H + kExT - 1) / kExT)), dim3(256), 0,
                       (hipStream_t)stream, known, H, W, eroded, (long long*)mask_ex);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}
