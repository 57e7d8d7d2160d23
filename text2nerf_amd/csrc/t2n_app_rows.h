// One feature row from the cached appearance feature volume (t2n_app_volume.hip), shared by the read kernel (k_app_features_vol, four
// lanes per entry, dense [tile * 32 + s] rows) and the tile marcher's tail / k_compact_list (t2n_march_tiles.hip: eight lanes per entry,
// rows addressed by list slot). Both mappings run the same multiply-adds per channel in the same corner order: the rows are the same bits.
#pragma once
#include "t2n_internal.h"
#include "t2n_device.h"

namespace t2n {

struct AvVolume { const float* avol; unsigned row, slice, ny1; };   // bytes between y / z neighbours, gy + 1

// LPE lanes per entry; lane q of an entry owns quads q, q + LPE, .. of the row. `mine` = the entry's (x, y, z, w); a dead entry (!live)
// reads corner 0 with weight 0. `row` = the entry's row + 4 q floats; stored when `store`.
template <int LPE>
__device__ __forceinline__ void av_feature_row(const FactorSet& app, const AvVolume& v, const float4 mine, const bool live, const int q,
                                               float* __restrict__ row, const bool store) {
    constexpr int NQ = 8 / LPE;   // quads per lane
    const char* __restrict__ V = reinterpret_cast<const char*>(v.avol);
    const Axes3 A = sample_axes_inbox(app, mine.x, mine.y, mine.z);
    // (list slots a failed reservation left unwritten decode to anything: the cell stays inside the grid, as in the direct form)
    const unsigned ix = (unsigned)min(max(A.a[0].i0, 0), app.W[0] - 1), iy = (unsigned)min(max(A.a[1].i0, 0), app.H[0] - 1);
    const unsigned iz = (unsigned)min(max(A.a[2].i0, 0), app.H[1] - 1);
    // (24-bit multiplies, as in the cached density read: appearance_volume_prepare refuses grids that leave their range)
    const unsigned cell = umad24(umad24(iz, v.ny1, iy), v.row, ix * kAvCornerBytes);
    const unsigned o00 = (live ? cell : 0u) + (unsigned)q * 16u;
    const unsigned o01 = o00 + v.row, o10 = o00 + v.slice, o11 = o10 + v.row;
    const unsigned off[4] = {o00, o01, o10, o11};   // (z, y), (z, y + 1), (z + 1, y), (z + 1, y + 1)
    float4 c[4][2][NQ];   // [(z, y)][x, x + 1][quad]
#pragma unroll
    for (int zy = 0; zy < 4; ++zy)
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int i = 0; i < NQ; ++i)   // (scalar base + 32-bit offset + immediate)
                c[zy][x][i] = *reinterpret_cast<const float4*>(V + (size_t)off[zy] + ((int)kAvCornerBytes * x + 16 * LPE * i));
    __builtin_amdgcn_sched_barrier(0);   // all of the entry's loads are on their way before the first one is used
    const float wx0 = live ? A.a[0].w0 : 0.f, wx1 = live ? A.a[0].w1 : 0.f;
    const float wyx[2][2] = {{A.a[1].w0 * wx0, A.a[1].w0 * wx1}, {A.a[1].w1 * wx0, A.a[1].w1 * wx1}};
    const float wz[2] = {A.a[2].w0, A.a[2].w1};
    float4 r[NQ];
#pragma unroll
    for (int zy = 0; zy < 4; ++zy)
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            const float w = wyx[zy & 1][x] * wz[zy >> 1];
#pragma unroll
            for (int i = 0; i < NQ; ++i) r[i] = (zy == 0 && x == 0) ? f4_mul(c[0][0][i], w) : f4_fma(c[zy][x][i], w, r[i]);
        }
    // quad 6 carries the entry's compositing weight in column 27, quad 7 is zeros
    if (q == 6 % LPE) r[6 / LPE].w = live ? mine.w : 0.f;
    if (q == 7 % LPE) r[7 / LPE] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (store) {
#pragma unroll
        for (int i = 0; i < NQ; ++i) *reinterpret_cast<float4*>(row + 4 * LPE * i) = r[i];
    }
}

// The rows of `count` consecutive list slots whose entries THIS wave has just written (`pos` = the first slot's entry, `feat` = its row;
// both wave-uniform): eight lanes per entry, eight entries per pass. The entries are read back 64 at a time, one per lane, by loads that
// bypass the vector L1 — a line of the list is shared with the neighbouring waves' regions, and a copy of it this CU fetched before
// this wave's stores must not be what the wave reads — and handed to the passes across lanes. The caller has waited for its stores.
__device__ __forceinline__ void av_slot_rows(const FactorSet& app, const AvVolume& v, const float4* pos, float* feat, unsigned count, int lane) {
    typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
    const int e = lane >> 3, q = lane & 7;
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float4*>(pos), 0, (int)(count * 16u), 0x00020000);
#pragma unroll 1
    for (unsigned c0 = 0; c0 < count; c0 += 64u) {
        const unsigned left = count - c0;
        const unsigned mine_i = (unsigned)lane < left ? c0 + (unsigned)lane : count - 1u;
        const u32x4_t p = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(mine_i * 16u), 0, 16);   // (aux 16 = sc1: served by L2)
        const unsigned npass = left < 64u ? (left + 7u) >> 3 : 8u;
#pragma unroll 1
        for (unsigned s = 0; s < npass; ++s) {
            const int src = (int)(8u * s) + e;
            const float4 mine = make_float4(__uint_as_float(__shfl(p.x, src)), __uint_as_float(__shfl(p.y, src)),
                                            __uint_as_float(__shfl(p.z, src)), __uint_as_float(__shfl(p.w, src)));
            const bool live = (unsigned)src < left;
            av_feature_row<8>(app, v, mine, live, q, feat + (size_t)(c0 + (unsigned)src) * 32u + 4u * (unsigned)q, live);
        }
    }
}

}  // namespace t2n
