// Appearance feature volume of the tile-marcher frames (gfx950).
//
// Feature j of a sample is sum_k sum_c B[j, 48 k + c] * (bilinear tap of plane k)[c] * (linear tap of line k)[c]. In every plane / line
// pair the four plane taps times the two line taps are the eight corners of the sample's cell, so the 27 features are the TRILINEAR
// interpolation of a per-corner volume
//     F_j(ix, iy, iz) = sum_k sum_c B[j, 48 k + c] * P_k[corner's plane texel][c] * L_k[corner's line texel][c]
// which depends on the appearance factors and basis_mat alone (the identity behind the cached summed density table, with 27 channels).
// k_app_volume_build computes F for the whole grid once per version of those tensors; k_app_features_vol is the second form of the
// feature stage (t2n_shade.hip: k_app_features_p is the direct one): same lists in, same feature rows out, 8 corners x 7 quads of
// loads and 64 multiply-adds per sample instead of the blend, the split products and the LDS staging. Frames of one version before and
// after the build differ by rounding only (tests/test_app_volume_gpu.py).
//
// Layout: corner-major, [gz + 1][gy + 1][gx + 1][32] floats, x fastest — channels 0..26 the features, 27..31 zero; one 128-B line per
// corner. One entry past the last texel per axis (a copy of the clamped corner, as in the density table): a cell at the grid's last
// texel reads it with weight 0, so the eight corners of a cell are always (x, x + 1) x (y, y + 1) x (z, z + 1) without a clamp.
#include "t2n_internal.h"
#include "t2n_device.h"
#include "t2n_app_rows.h"

namespace t2n {

constexpr int kAvK = 144;                  // 3 x 48 plane x line products per corner

// ---- build ------------------------------------------------------------------------------------------------------------------------
// One thread per corner (x fastest: the 64 corners of a wave share their z and mostly their y, so line 0 / line 1 and the plane rows are
// broadcast or contiguous reads). The 144 products are formed from the channel-last fp32 factors (under bf16 storage: the rounded
// values as fp32, what every form of the feature stage multiplies) and contracted with basis_mat in fp32 multiply-adds, channel by
// channel in index order; basis_mat comes from the packed fp32 operand the exact path reads (FieldDev::basisA: [144][32], features
// contiguous, zero past app_dim), copied to LDS once per workgroup and read there at wave-uniform addresses.
struct AvBuildArgs { FactorSet app; const float* Bt; float* out; int n[3]; long long corners; };

template <int K>
__device__ __forceinline__ void av_pair(const AvBuildArgs& a, const float* __restrict__ Bs, const int c[3], float (&acc)[28]) {
    const float4* __restrict__ P = reinterpret_cast<const float4*>(a.app.plane[K]) + ((size_t)c[mat1(K)] * a.app.W[K] + c[mat0(K)]) * 12;
    const float4* __restrict__ L = reinterpret_cast<const float4*>(a.app.line[K]) + (size_t)c[vecm(K)] * 12;
#pragma unroll 1
    for (int q = 0; q < 12; ++q) {
        const float4 p = P[q], l = L[q];
        const float x[4] = {p.x * l.x, p.y * l.y, p.z * l.z, p.w * l.w};
        const float4* __restrict__ b = reinterpret_cast<const float4*>(Bs + (48 * K + 4 * q) * 32);
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
#pragma unroll
            for (int jq = 0; jq < 7; ++jq) {
                const float4 bv = b[ch * 8 + jq];
                acc[4 * jq] = fmaf(bv.x, x[ch], acc[4 * jq]); acc[4 * jq + 1] = fmaf(bv.y, x[ch], acc[4 * jq + 1]);
                acc[4 * jq + 2] = fmaf(bv.z, x[ch], acc[4 * jq + 2]); acc[4 * jq + 3] = fmaf(bv.w, x[ch], acc[4 * jq + 3]);
            }
    }
}

__global__ __launch_bounds__(256) void k_app_volume_build(const AvBuildArgs a) {
    __shared__ __attribute__((aligned(16))) float Bs[kAvK * 32];
    for (int i = threadIdx.x; i < kAvK * 32 / 4; i += 256) reinterpret_cast<float4*>(Bs)[i] = reinterpret_cast<const float4*>(a.Bt)[i];
    __syncthreads();
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.corners) return;
    const int nx = a.n[0] + 1, ny = a.n[1] + 1;
    const int x = (int)(idx % nx), y = (int)((idx / nx) % ny), z = (int)(idx / ((long long)nx * ny));
    const int c[3] = {min(x, a.n[0] - 1), min(y, a.n[1] - 1), min(z, a.n[2] - 1)};   // the entry past the last texel: the clamped corner again
    float acc[28];
#pragma unroll
    for (int j = 0; j < 28; ++j) acc[j] = 0.f;
    av_pair<0>(a, Bs, c, acc);
    av_pair<1>(a, Bs, c, acc);
    av_pair<2>(a, Bs, c, acc);
    float4* __restrict__ o = reinterpret_cast<float4*>(a.out + (size_t)idx * kAvStride);
#pragma unroll
    for (int jq = 0; jq < 7; ++jq) o[jq] = make_float4(acc[4 * jq], acc[4 * jq + 1], acc[4 * jq + 2], jq == 6 ? 0.f : acc[4 * jq + 3]);
    if constexpr (kAvStride == 32) o[7] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---- read -------------------------------------------------------------------------------------------------------------------------
// Four lanes per entry, sixteen entries per pass, two passes per 32-entry tile. Lane (e, q) owns quads q and q + 4 of the row: for each
// of the cell's eight corners it loads those two quads (lanes of one entry read 64 contiguous bytes per load; quad 7 is the volume's
// zero padding), sixteen 16-B loads issued together off one scalar base and four 32-bit byte offsets, then 64 multiply-adds in a fixed
// corner order. Tap indices and weights are sample_axes_inbox's, as in the direct form. Dead entries of a partial tile read corner 0
// with weight 0. The row layout is k_app_features_p's: 27 features, the entry's compositing weight in column 27, zeros.
struct AvReadArgs {
    FactorSet app;                 // sizes only
    const float* avol; unsigned row, slice, ny1;   // bytes between y / z neighbours, gy + 1
    const float4* app_pos; const unsigned* counters; unsigned list_cap; int nlists; unsigned tile_hi;
    float* feat;
};

__global__ __launch_bounds__(256) void k_app_features_vol(const AvReadArgs a) {
    // lanes per entry: 4 (quads q and q + 4 of a corner per lane). 8 lanes (one quad each, 79 VGPRs against 110) and 4 to 16 workgroups
    // per CU all run the C2 frame's rows in 0.27 ms: the texture addresser is busy for 0.78 - 0.87 of the kernel's cycles with the
    // 34 wave-wide 16-B loads per tile, whatever the lane mapping; the vector L1 serves four fifths of their line accesses and the
    // volume's touched part stays in L2 / Infinity Cache (counters: profiles/appearance_volume_ab.txt, section 9)
    // (the per-entry body is av_feature_row, t2n_app_rows.h: the tile marcher's tail runs it with eight lanes per entry)
    constexpr int LPE = 4, EPP = 64 / LPE, PASSES = 32 / EPP;   // entries per pass, passes per tile
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    unsigned cnt_l, incl;
    unsigned ntiles = (unsigned)__builtin_amdgcn_readfirstlane((int)list_tiles(a.counters, a.list_cap, a.nlists, lane, cnt_l, incl));
    if (ntiles > a.tile_hi) ntiles = a.tile_hi;
    const unsigned wave_stride = gridDim.x * 4u;
    const int e = lane / LPE, q = lane % LPE;
    const AvVolume vol{a.avol, a.row, a.slice, a.ny1};
    for (unsigned tile = blockIdx.x * 4u + wid; tile < ntiles; tile += wave_stride) {
        // tile -> (first entry, live entries), in scalar registers
        unsigned base, count;
        list_locate<true>(tile, cnt_l, incl, a.list_cap, a.nlists, lane, base, count);
        const unsigned nlive = (unsigned)__builtin_amdgcn_readfirstlane((int)(count - base < 32u ? count - base : 32u));
        const float4* __restrict__ pb = a.app_pos + base;
        asm volatile("" : "+s"(pb));
        float* __restrict__ rb = a.feat + (size_t)tile * 1024;
        asm volatile("" : "+s"(rb));
        float4 pos[PASSES];
#pragma unroll
        for (int p = 0; p < PASSES; ++p) pos[p] = (unsigned)(EPP * p + e) < nlive ? pb[EPP * p + e] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const bool live = (unsigned)(EPP * p + e) < nlive;
            const float4 mine = pos[p];
            av_feature_row<LPE>(a.app, vol, mine, live, q, rb + (unsigned)((EPP * p + e) * 32 + 4 * q), true);
        }
    }
}

int launch_app_features_vol(t2n_field* f, const float4* app_pos, const unsigned* counters_dev, unsigned list_cap, unsigned tile_hi, float* feat,
                            hipStream_t s) {
    AvReadArgs a;
    a.app = f->dev.app;
    a.avol = f->dev.avol; a.row = f->dev.av_row; a.slice = f->dev.av_slice; a.ny1 = (unsigned)f->desc.grid[1] + 1u;
    a.app_pos = app_pos; a.counters = counters_dev; a.list_cap = list_cap; a.nlists = kLists; a.tile_hi = tile_hi; a.feat = feat;
    const unsigned long long wg = ((unsigned long long)tile_hi + 3u) / 4u;
    const unsigned wg_max = 256u * 8u;   // eight workgroups of four waves per CU
    const dim3 grid((unsigned)(wg < wg_max ? (wg ? wg : 1u) : wg_max));
    hipLaunchKernelGGL(k_app_features_vol, grid, dim3(256), 0, s, a);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

// ---- lifetime ---------------------------------------------------------------------------------------------------------------------
size_t appearance_volume_bytes(const t2n_field* f) {
    const int* g = f->desc.grid;
    return (size_t)(g[0] + 1) * (g[1] + 1) * (g[2] + 1) * kAvCornerBytes;
}

int launch_app_volume_build(const t2n_field* f, float* out, hipStream_t s) {
    AvBuildArgs a;
    a.app = f->dev.app; a.Bt = f->dev.basisA; a.out = out;
    a.corners = 1;
    for (int k = 0; k < 3; ++k) { a.n[k] = f->desc.grid[k]; a.corners *= a.n[k] + 1; }
    hipLaunchKernelGGL(k_app_volume_build, dim3((unsigned)((a.corners + 255) / 256)), dim3(256), 0, s, a);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

void appearance_volume_release(t2n_field* f) {
    if (f->avol) { (void)hipDeviceSynchronize(); (void)hipFree(f->avol); }
    f->avol = nullptr; f->avol_bytes = 0; f->avol_version = 0; f->avol_seen = 0; f->avol_run = 0; f->avol_alloc_failed = false;
    f->dev.avol = nullptr;
}

// Once per tile-marcher frame (t2n_render_forward), next to density_cache_prepare: f->dev.avol = the volume when it is current, else NULL
// (the frame's feature stage then runs the direct form). The volume is built by the avol_min_frames-th CONSECUTIVE tile-marcher frame
// that finds the appearance factors and basis_mat unchanged — a build costs as much as that many frames save, so a loop that alternates
// optimiser steps and single frames never builds — on that frame's stream in front of its launches; frames on other streams wait for
// the event behind the build. A rebuild overwrites the buffer in place, ordered like the density table's.
int appearance_volume_prepare(t2n_field* f, hipStream_t s) {
    f->dev.avol = nullptr;
    if (f->avol_seen == f->app_version) ++f->avol_run; else { f->avol_seen = f->app_version; f->avol_run = 1; }
    const auto direct = [&]() { ++f->avol_counts[1]; return (int)T2N_OK; };
    if (!f->avol_on) return direct();
    // the frames whose feature stage is k_app_features_p (launch_shade_list): the fused MLP_Fea_noview head on split products
    if (f->desc.shading != T2N_SHADE_MLP_FEA_NOVIEW || !f->mlp_split || f->desc.app_n_comp != 48 || f->desc.app_dim != 27) return direct();
    const int* g = f->desc.grid;
    const size_t bytes = appearance_volume_bytes(f);
    size_t cap = f->avol_cap;
    if (!cap) {
        static size_t dev_total[64] = {};   // per device: asked once
        int d = 0;
        if (hipGetDevice(&d) != hipSuccess) { (void)hipGetLastError(); d = 0; }
        size_t& total = dev_total[(unsigned)d % 64u];
        if (!total) { size_t fr = 0, tot = 0; if (hipMemGetInfo(&fr, &tot) == hipSuccess) total = tot; else (void)hipGetLastError(); }
        cap = total / 64;
    }
    // (k_app_features_vol: 24-bit row counts and row bytes, 32-bit byte offsets — the last load of a cell reaches 256 B past its offset)
    const bool addressable = (size_t)(g[1] + 1) * (g[2] + 1) < (1u << 24) && (size_t)(g[0] + 1) * kAvCornerBytes < (1u << 24) &&
                             bytes + 256 < (1ull << 32);
    if ((size_t)g[0] * g[1] * g[2] * kAvCornerBytes > cap || !addressable) return direct();
    if (f->avol && f->avol_version == f->app_version) {
        if (f->avol_stream != (void*)s) T2N_HIP(hipStreamWaitEvent(s, (hipEvent_t)f->avol_ev, 0));
    } else {
        if (f->avol_run < (unsigned long long)(f->avol_min_frames > 1 ? f->avol_min_frames : 1)) return direct();
        if (!f->avol) {
            if (f->avol_alloc_failed) return direct();
            if (hipMalloc((void**)&f->avol, bytes + 256) != hipSuccess) {   // no room: the frames keep the direct form
                (void)hipGetLastError();
                f->avol = nullptr; f->avol_alloc_failed = true;
                return direct();
            }
            f->avol_bytes = bytes + 256;
        }
        if (!f->avol_ev) T2N_HIP(hipEventCreateWithFlags((hipEvent_t*)&f->avol_ev, hipEventDisableTiming));
        const int rc = launch_app_volume_build(f, f->avol, s);
        if (rc) return rc;
        T2N_HIP(hipEventRecord((hipEvent_t)f->avol_ev, s));
        f->avol_stream = (void*)s;
        f->avol_version = f->app_version;
        ++f->avol_counts[2];
    }
    f->dev.avol = f->avol;
    f->dev.av_row = (unsigned)(g[0] + 1) * kAvCornerBytes;
    f->dev.av_slice = f->dev.av_row * (unsigned)(g[1] + 1);
    ++f->avol_counts[0];
    return T2N_OK;
}

}  // namespace t2n
