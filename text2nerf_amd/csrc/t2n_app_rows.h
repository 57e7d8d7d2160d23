// One feature row from the cached appearance feature volume (t2n_app_volume.hip), shared by the read kernel (k_app_features_vol, four
// lanes per entry, dense [tile * 32 + s] rows) and the tile marcher's tail / k_compact_list (t2n_march_tiles.hip: eight lanes per entry,
// rows addressed by list slot). Both mappings run the same multiply-adds per channel in the same corner order: the rows are the same bits.
#pragma once
#include "t2n_internal.h"
#include "t2n_device.h"

namespace t2n {

struct AvVolume { const float* avol; unsigned row, slice, ny1; };   // bytes between y / z neighbours, gy + 1

// A 4 x 4 x 4 box of the volume's corners copied to LDS (the tile marcher's staged tail): corner (x, y, z) of the box = corner
// min(origin + (x, y, z), last padded index) of the volume, quads 0..6 of it (quad 7 of a row is zeros whatever the corner holds) at
// ((z * 4 + y) * 4 + x) * kAvBoxCornerBytes. A cell read there must lie inside the box: low taps within origin .. origin + 2 per axis.
constexpr unsigned kAvBoxCornerBytes = 112;
struct AvBox { const char* lds; int ox, oy, oz; };
struct AvNoBox {};

// LPE lanes per entry; lane q of an entry owns quads q, q + LPE, .. of the row. `mine` = the entry's (x, y, z, w); a dead entry (!live)
// reads corner 0 with weight 0. `row` = the entry's row + 4 q floats; stored when `store`. BOX = AvBox: the eight corners come from the
// staged box instead of the volume (LPE = 8 only) — the only difference; positions, corner order, weight products and multiply-adds are
// the one statement below, so the rows are the same bits.
template <int LPE, typename BOX = AvNoBox>
__device__ __forceinline__ void av_feature_row(const FactorSet& app, const AvVolume& v, const float4 mine, const bool live, const int q,
                                               float* __restrict__ row, const bool store, const BOX box = BOX()) {
    constexpr int NQ = 8 / LPE;   // quads per lane
    constexpr bool kBox = !__is_same(BOX, AvNoBox);
    static_assert(!kBox || LPE == 8, "the staged box is read eight lanes per entry");
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
    const char* __restrict__ B = nullptr;
    if constexpr (kBox) {
        // (one LDS address + immediates; lane 7's quad does not exist in the box: it reads quad 6 and writes zeros below)
        const unsigned bcell = (unsigned)((((int)iz - box.oz) * 4 + ((int)iy - box.oy)) * 4 + ((int)ix - box.ox)) * kAvBoxCornerBytes;
        B = box.lds + ((live ? bcell : 0u) + (unsigned)min(q, 6) * 16u);
    } else {
#pragma unroll
        for (int zy = 0; zy < 4; ++zy)
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int i = 0; i < NQ; ++i)   // (scalar base + 32-bit offset + immediate)
                    c[zy][x][i] = *reinterpret_cast<const float4*>(V + (size_t)off[zy] + ((int)kAvCornerBytes * x + 16 * LPE * i));
    }
    if constexpr (!kBox) __builtin_amdgcn_sched_barrier(0);   // all of the entry's loads are on their way before the first one is used
    const float wx0 = live ? A.a[0].w0 : 0.f, wx1 = live ? A.a[0].w1 : 0.f;
    const float wyx[2][2] = {{A.a[1].w0 * wx0, A.a[1].w0 * wx1}, {A.a[1].w1 * wx0, A.a[1].w1 * wx1}};
    const float wz[2] = {A.a[2].w0, A.a[2].w1};
    float4 r[NQ];
#pragma unroll
    for (int zy = 0; zy < 4; ++zy)
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            if constexpr (kBox) {
                // the box's corners one z plane at a time (LDS latency is short; eight corners at once would not fit the marcher's
                // allocation beside what its tail keeps across a pass)
                if ((zy & 1) == 0 && x == 0) {
                    if (zy) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        c[zy + (j >> 1)][j & 1][0] = *reinterpret_cast<const float4*>(B + (int)kAvBoxCornerBytes * (((zy >> 1) * 4 + (j >> 1)) * 4 + (j & 1)));
                }
            }
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
