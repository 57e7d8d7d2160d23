// Tile marcher (eval frames in image order): 8x8-pixel tiles, ONE LANE PER RAY, all 64 rays of a tile advance through the
// same sample index together. At a given depth the 64 rays lie within a few texels of each other (pixel pitch t/f is far
// below the texel size), so per factor pair the union of their bilinear footprints is a small rectangle of R texels and a
// short segment of S line rows. The density feature of a sample is
//     sum_k sum_c (sum_t w_t P_k[t][c]) * (sum_l w_l L_k[l][c])  =  sum_k sum_t sum_l w_t w_l D_k[t][l],
//     D_k[t][l] = sum_c P_k[t][c] * L_k[l][c]      (t over the rectangle, l over the segment, c over the 16 components)
// so the wave computes the small table D_k = P_k L_k^T ONCE per step on the matrix cores (v_mfma_f32_16x16x4_f32, exact
// f32: one 16-B load per lane supplies the A operand of four k-steps, lane l holding texel l&15, components 4(l>>4)..+3),
// parks it in LDS (<= 64 x 16 floats per plane), adds the three tables into ONE 4 x 4 x 4 table S[z][y][x] (one entry per lane:
// the 4 x 2 entries per plane a lane would read are the terms of the 8 corner values of its cell, table_sum) and every lane
// reads just the 8 corners of its cell from S — 32 B per sample instead of the 1152 B of factor data the per-lane interpolation
// reads (and of the 96 B and three interpolations of reading the pair tables: 2 x 65 VALU + 2 x 12 LDS reads per step pair
// became 18 + 2 x 20 VALU and 4 + 2 x 4 LDS; profiles/march_summed_table_ab.txt). (The staged-factor variant of this kernel was
// LDS bandwidth-bound: 72 ds_read_b128 per wave step = 576 clk of the CU's 128 B/clk LDS pipe x 12 resident waves.)
// Against k_march's pass B (16 samples x 4 lanes per step, 18 scattered 64-B gathers per sample; PMC: texture addresser 71 %
// busy, VALU ~70 %) this removes ~15x of the addresser work and the 4x-redundant per-sample coordinate math. The
// transmittance is a per-lane running product in sample order — exactly the reference's cumprod order
// (models/tensorBase.py:23) — so no wave scan is needed; acc/depth accumulate in registers.
//
// Outputs per ray: acc, depth, (slot0, n_app, n_valid, first | Lw << 11) and the ray's contiguous, sample-ordered slice of
// the appearance list (in-kernel compaction, see TileArgs); with weights requested (DENSE) also the weights of the wave's sampled
// window (k_dense_fill writes the z_vals rows and the zeros of the weights rows beforehand).
// EVERY sample reads its density feature from S. A step pair whose taps do not fit one 4 x 4 x 4 table (incoherent rays, huge field of
// view) is served by a wave-uniform loop over boxes: the box at the low taps of the first sample not yet served is built, every
// unserved sample whose cell lies in it reads it, until none is left (a sparse frame can give every lane a box of its own:
// profiles/march_table_every_pair_ab.txt). An entry of S is a function of its texel alone, so a sample gets the same bits whichever
// box serves it.
// S is a function of the density factors alone: a field rendered more than once keeps S of its WHOLE grid in a per-field buffer
// (k_density_sum_table, density_cache_prepare) and the CACHED instantiations read a cell's eight entries there — the same bits,
// without the per-step-pair loads, MFMAs, LDS table and fences (C2 frame: 0.51 -> 0.38 ms; profiles/march_density_cache_ab.txt), and
// with nothing to decide per step pair: no tap bit set, no reduction over the wave, no branch.
// Replaces the same reference lines as k_march (see t2n_march.hip).
#include <type_traits>
#include "t2n_device.h"
#include "t2n_app_rows.h"

namespace t2n {

// Table geometry: a plane rectangle of up to 2^LOG2W x 2^LOG2W texels lives in fixed slots (slot = row << LOG2W | col, so no
// division by the rectangle width), the line segment in up to 2^LOG2W rows. LOG2W = 2 (16 slots = ONE 16x16x4 MFMA row
// block per plane) covers nearly every step of a pinhole frame; LOG2W = 3 (64 slots, four row blocks) takes the rest.
constexpr int kMaxLog2W = 2;
constexpr int kDStrideMax = (1 << (2 * kMaxLog2W)) + 4;   // floats per line row of the transposed table D^T[line row][slot]
constexpr int kPairFloats = 3 * 16 * kDStrideMax;        // per wave: the three pair tables D_k^T
// the summed table S[z][y][x] (4 x 4 x 4, one entry per lane); a lane reads up to 21 floats past its low corner, so the region is
// padded to 64 + 32 floats (zeroed once per wave): a read past the last entry stays inside the wave's own region. S sits IN FRONT
// of the pair tables: the eight entries of a sample are then four ds_read2_b32 off ONE address register (the instruction's two
// offsets are 8-bit dword counts; behind the 960 floats of the pair tables every read pair needs an address of its own).
constexpr int kSumFloats = 96;
constexpr int kStageFloats = kPairFloats + kSumFloats;   // per wave
static_assert(63 + 21 < kSumFloats && kStageFloats % 4 == 0, "summed table: the farthest read stays in the wave's region; 16-B aligned regions");
typedef float f32x4_t __attribute__((ext_vector_type(4)));

struct TileArgs {
    FieldDev F;
    const float* rays; long long n_rays; int ray_stride; int n_samples; int img_w, img_h;
    float* acc; float* depth; int4* ray_app;
    // in-kernel compaction: every lane stages its ray's appearance entries (<= cap) in `scratch`; at the end the wave reserves
    // ONE contiguous region of the appearance list for its 64 rays and copies the entries there, ray by ray in sample order.
    // A ray whose slice is full writes its further weights to its row of `wbuf` (the caller's weights tensor when one was
    // requested, else a scratch matrix) and goes to `ovf_list`; k_compact_list finishes those rays.
    float* wbuf;        // [n_rays, n_samples] spill rows
    float4* scratch; int cap; unsigned* ovf_count; int* ovf_list;
    float4* app_pos; int* app_ray; unsigned* counters; unsigned list_cap; unsigned long long* stats;
    // DENSE: the caller's [n_rays, n_samples] weights tensor. k_dense_fill has written zeros (and the z_vals rows) before this kernel;
    // the marcher writes the weights of the 16-step blocks its wave's window touches, through a per-wave LDS transpose: 16 steps x
    // 64 rays, then 64-B row segments per store
    float* dense_w;
    // ROWS: the feature rows of a fused frame, one [32]-float row per LIST SLOT (row of slot s at feat + 32 s); the volume they are
    // fetched from is F.avol / F.av_row / F.av_slice
    float* feat;
#ifdef MT_PROF
    unsigned long long* prof;   // [waves][8] per-region cycle sums (instrumented build, tools/r5_march_accounting.sh)
#endif
};

__device__ __forceinline__ void lds_fence_w() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Wave-wide min / max with short dependency chains: DPP row_shr scans inside each 16-lane row (lane 15 of a row ends up with
// the row result), then four v_readlane + scalar min/max. (A __shfl_xor butterfly is six dependent ds_bpermute round trips,
// ~2 us per step for the six reductions of a marching step.)
template <int CTRL>
__device__ __forceinline__ int dpp_shr(int v, int identity) {
    return __builtin_amdgcn_update_dpp(identity, v, CTRL, 0xf, 0xf, false);
}
__device__ __forceinline__ int wave_min_i(int v) {
    const int big = 0x7fffffff;
    v = min(v, dpp_shr<0x111>(v, big));
    v = min(v, dpp_shr<0x112>(v, big));
    v = min(v, dpp_shr<0x114>(v, big));
    v = min(v, dpp_shr<0x118>(v, big));
    const int a = __builtin_amdgcn_readlane(v, 15), b = __builtin_amdgcn_readlane(v, 31);
    const int c = __builtin_amdgcn_readlane(v, 47), d = __builtin_amdgcn_readlane(v, 63);
    return min(min(a, b), min(c, d));
}
__device__ __forceinline__ int wave_max_i(int v) {
    const int small = -0x7fffffff;
    v = max(v, dpp_shr<0x111>(v, small));
    v = max(v, dpp_shr<0x112>(v, small));
    v = max(v, dpp_shr<0x114>(v, small));
    v = max(v, dpp_shr<0x118>(v, small));
    const int a = __builtin_amdgcn_readlane(v, 15), b = __builtin_amdgcn_readlane(v, 31);
    const int c = __builtin_amdgcn_readlane(v, 47), d = __builtin_amdgcn_readlane(v, 63);
    return max(max(a, b), max(c, d));
}

__device__ __forceinline__ unsigned wave_or_u(unsigned v) {
    v |= (unsigned)dpp_shr<0x111>((int)v, 0);
    v |= (unsigned)dpp_shr<0x112>((int)v, 0);
    v |= (unsigned)dpp_shr<0x114>((int)v, 0);
    v |= (unsigned)dpp_shr<0x118>((int)v, 0);
    const unsigned a = (unsigned)__builtin_amdgcn_readlane((int)v, 15), b = (unsigned)__builtin_amdgcn_readlane((int)v, 31);
    const unsigned c = (unsigned)__builtin_amdgcn_readlane((int)v, 47), d = (unsigned)__builtin_amdgcn_readlane((int)v, 63);
    return (a | b) | (c | d);
}

// The tap box of a step pair: the low-tap indices of its live samples (ok[q]) over the wave, per axis, as ONE or-reduced bit set —
// 10 bits per axis around the first live lane's index (bit 5); an index outside [-5, +4] of it raises bit 30. amn[a] = the lowest
// low tap of axis a. True when the pair fits ONE 4 x 4 x 4 table: at most three low taps per axis (the high tap is at most one above
// the highest low tap, and inside the grid). okm = the ballot of the lanes with a live sample, not zero.
__device__ __forceinline__ bool pair_box(const Axes3 (&A)[2], const bool (&ok)[2], unsigned long long okm, int (&amn)[3]) {
    int sel0 = 0, sel1 = 0, sel2 = 0;
#pragma unroll
    for (int q = 1; q >= 0; --q)
        if (ok[q]) { sel0 = A[q].a[0].i0; sel1 = A[q].a[1].i0; sel2 = A[q].a[2].i0; }
    const int lead = (int)__builtin_ctzll(okm);
    const int ref0 = __builtin_amdgcn_readlane(sel0, lead), ref1 = __builtin_amdgcn_readlane(sel1, lead),
              ref2 = __builtin_amdgcn_readlane(sel2, lead);
    unsigned bits = 0u;
#pragma unroll
    for (int q = 0; q < 2; ++q)
        if (ok[q]) {
            const unsigned d0 = (unsigned)(A[q].a[0].i0 - ref0 + 5), d1 = (unsigned)(A[q].a[1].i0 - ref1 + 5),
                           d2 = (unsigned)(A[q].a[2].i0 - ref2 + 5);
            bits |= (d0 < 10u ? 1u << d0 : 0x40000000u) | (d1 < 10u ? 1u << (10u + d1) : 0x40000000u) |
                    (d2 < 10u ? 1u << (20u + d2) : 0x40000000u);
        }
    bits = wave_or_u(bits);
    const unsigned f0 = bits & 1023u, f1 = (bits >> 10) & 1023u, f2 = (bits >> 20) & 1023u;
    amn[0] = ref0 - 5 + __builtin_ctz(f0); amn[1] = ref1 - 5 + __builtin_ctz(f1); amn[2] = ref2 - 5 + __builtin_ctz(f2);
    const int span = max(max(32 - __builtin_clz(f0) - __builtin_ctz(f0), 32 - __builtin_clz(f1) - __builtin_ctz(f1)),
                         32 - __builtin_clz(f2) - __builtin_ctz(f2)) + 1;
    return !(bits & 0x40000000u) && span <= 4;
}

// The dot-product tables of one wave step (see the file header). amn[a] = lowest tap index of axis a over the wave; every axis
// spans at most 2^LOG2W taps. table_build computes D_k^T[line row][slot] for the three pairs into the wave's LDS area, table_sum
// adds them into S, table_read3 returns a lane's density feature from its 8 entries of S. Several samples per lane may share
// one build.
template <int LOG2W>
__device__ __forceinline__ void table_build(const FactorSet& S, const int (&amn)[3], float* __restrict__ stD, int l15, int lq) {
    constexpr int WS = 1 << LOG2W, SL = WS * WS, NB = SL / 16, ST = SL + 4;
    const int gs[3] = {S.W[0], S.H[0], S.H[1]};
    // phase 1: every operand load of the step in flight together; slots beyond the rectangle read clamped (valid, unused) texels
    float4 av[3][NB], bv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int m0 = mat0(k), m1 = mat1(k), vv = vecm(k);
        const float4* __restrict__ P = reinterpret_cast<const float4*>(S.plane[k]);
        const float4* __restrict__ Ln = reinterpret_cast<const float4*>(S.line[k]);
        const unsigned jr = (unsigned)min(amn[vv] + (l15 & (WS - 1)), gs[vv] - 1);
        bv[k] = Ln[jr * 4u + (unsigned)lq];
#pragma unroll
        for (int mb = 0; mb < NB; ++mb) {
            const int t = mb * 16 + l15;
            const unsigned yy = (unsigned)min(amn[m1] + (t >> LOG2W), gs[m1] - 1), xx = (unsigned)min(amn[m0] + (t & (WS - 1)), gs[m0] - 1);
            av[k][mb] = P[(__umul24(yy, (unsigned)gs[m0]) + xx) * 4u + (unsigned)lq];   // (24-bit multiply: full rate)
        }
    }
    // phase 2: D_k^T[line row][slot] = sum_c L_k[row][c] P_k[slot][c]; the lane holds slots 4 lq..+3 of line row l15
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float* __restrict__ Dk = stD + kSumFloats + k * 16 * ST + l15 * ST + lq * 4;
#pragma unroll
        for (int mb = 0; mb < NB; ++mb) {
            f32x4_t d = {0.f, 0.f, 0.f, 0.f};
            d = __builtin_amdgcn_mfma_f32_16x16x4f32(av[k][mb].x, bv[k].x, d, 0, 0, 0);
            d = __builtin_amdgcn_mfma_f32_16x16x4f32(av[k][mb].y, bv[k].y, d, 0, 0, 0);
            d = __builtin_amdgcn_mfma_f32_16x16x4f32(av[k][mb].z, bv[k].z, d, 0, 0, 0);
            d = __builtin_amdgcn_mfma_f32_16x16x4f32(av[k][mb].w, bv[k].w, d, 0, 0, 0);
            *reinterpret_cast<float4*>(Dk + mb * 16) = make_float4(d[0], d[1], d[2], d[3]);
        }
    }
}
// The three pair tables summed into ONE 4 x 4 x 4 table, once per build: the 24 entries a lane read from them are the terms of the 8
// corner values of its cell in
//     S[z][y][x] = D_0^T[z][y << 2 | x] + D_1^T[y][z << 2 | x] + D_2^T[x][z << 2 | y]
// (pair 0 = plane (x, y) x line z, pair 1 = plane (x, z) x line y, pair 2 = plane (y, z) x line x), so a sample's density feature is
// the trilinear interpolation of S over that cell. Lane e = z << 4 | y << 2 | x adds its three terms in a fixed order and stores
// S[e]; the caller fences before and after. `lane` arrives behind an opaque copy (see the call site): the three offsets are lane
// constants the compiler would otherwise keep in registers across the whole step loop.
template <int LOG2W>
__device__ __forceinline__ void table_sum(float* __restrict__ stD, int lane) {
    static_assert(LOG2W == 2, "the summed table is one entry per lane: 4 taps per axis");
    constexpr int ST = (1 << (2 * LOG2W)) + 4;
    const unsigned x = (unsigned)lane & 3u, y = ((unsigned)lane >> 2) & 3u, z = (unsigned)lane >> 4;
    const float* __restrict__ D = stD + kSumFloats;
    // (24-bit multiplies: full rate)
    const float d0 = D[__umul24(z, (unsigned)ST) + ((unsigned)lane & 15u)];
    const float d1 = D[16 * ST + __umul24(y, (unsigned)ST) + (z << 2 | x)];
    const float d2 = D[32 * ST + __umul24(x, (unsigned)ST) + (z << 2 | y)];
    stD[lane] = (d0 + d1) + d2;
}
// A lane's density feature from the summed table: ONE offset (the low corner of its cell); the other seven entries sit at fixed
// distances from it, because a high tap is the low tap + 1 wherever its weight is not zero (axis_taps: the clamp at the grid's last
// texel comes with weight 0). There the entry one step further is read instead of the clamped one - a finite value (every entry of S
// is written by each build from slots table_build fills with clamped texels, the padding behind S is zeroed once per wave) times a
// zero weight: the sum is the same. The order of the additions is fixed (it does not depend on the box origin).
// `org` = (amn[2] << 4) + (amn[1] << 2) + amn[0]: the box origin's part of the offset, wave-uniform.
__device__ __forceinline__ float table_read3(const Axes3& A, int org, const float* __restrict__ stS) {
    const Axis& ax = A.a[0];
    const Axis& ay = A.a[1];
    const Axis& az = A.a[2];
    const float* __restrict__ D = stS + (((az.i0 << 4) + ((ay.i0 << 2) + ax.i0)) - org);
    const float wnw = ay.w0 * ax.w0, wne = ay.w0 * ax.w1, wsw = ay.w1 * ax.w0, wse = ay.w1 * ax.w1;
    float v0 = D[0] * wnw, v1 = D[16] * wnw;
    v0 = fmaf(D[1], wne, v0); v1 = fmaf(D[17], wne, v1);
    v0 = fmaf(D[4], wsw, v0); v1 = fmaf(D[20], wsw, v1);
    v0 = fmaf(D[5], wse, v0); v1 = fmaf(D[21], wse, v1);
    return fmaf(v1, az.w1, v0 * az.w0);
}

// The same feature from the CACHED table of the whole grid (FieldDev::dsum, k_density_sum_table): the eight entries of a cell are four
// 8-byte loads (x and x + 1 are adjacent; rows are only 4-B aligned) off one scalar base and a 32-bit byte offset per lane; the
// weight products and multiply-adds are table_read3's, in its order, on entries that are the same bits (tests/test_density_cache.py).
struct __attribute__((aligned(4))) F2U { float a, b; };
struct CellTaps { F2U d00, d01, d10, d11; };   // (z, y), (z, y + 1), (z + 1, y), (z + 1, y + 1); .a = x, .b = x + 1
__device__ __forceinline__ unsigned cached_offset(const FieldDev& F, const Axes3& A) {
    // (24-bit multiplies: full rate; density_cache_prepare refuses grids whose row count or row bytes leave 24 bits)
    return umad24(umad24((unsigned)A.a[2].i0, (unsigned)F.den.H[0] + 1u, (unsigned)A.a[1].i0), F.ds_row, (unsigned)A.a[0].i0 << 2);
}
__device__ __forceinline__ CellTaps cached_load(const FieldDev& F, unsigned off) {
    const char* __restrict__ B = reinterpret_cast<const char*>(F.dsum);
    CellTaps t;
    t.d00 = *reinterpret_cast<const F2U*>(B + off);
    t.d01 = *reinterpret_cast<const F2U*>(B + (off + F.ds_row));
    t.d10 = *reinterpret_cast<const F2U*>(B + (off + F.ds_slice));
    t.d11 = *reinterpret_cast<const F2U*>(B + (off + F.ds_slice + F.ds_row));
    return t;
}
__device__ __forceinline__ float cached_read3(const Axes3& A, const CellTaps& t) {
    const Axis& ax = A.a[0];
    const Axis& ay = A.a[1];
    const Axis& az = A.a[2];
    const float wnw = ay.w0 * ax.w0, wne = ay.w0 * ax.w1, wsw = ay.w1 * ax.w0, wse = ay.w1 * ax.w1;
    float v0 = t.d00.a * wnw, v1 = t.d10.a * wnw;
    v0 = fmaf(t.d00.b, wne, v0); v1 = fmaf(t.d10.b, wne, v1);
    v0 = fmaf(t.d01.a, wsw, v0); v1 = fmaf(t.d11.a, wsw, v1);
    v0 = fmaf(t.d01.b, wse, v0); v1 = fmaf(t.d11.b, wse, v1);
    return fmaf(v1, az.w1, v0 * az.w0);
}

// A reservation that did not fit leaves its sub-list counter raised over entries nobody writes (the readers clamp the counter to
// list_cap, so the part of the region inside the list IS walked by the shading kernels): those entries get a defined content — the
// volume centre, weight 0, ray 0 — whatever the scratch held before (the SH head reads the entry's ray for its view direction).
__device__ __forceinline__ void void_entries(float4* __restrict__ app_pos, int* __restrict__ app_ray, unsigned list, unsigned list_cap,
                                             unsigned lo, unsigned hi, int lane) {
    if (hi > list_cap) hi = list_cap;
    for (unsigned e = lo + (unsigned)lane; e < hi; e += 64u) {
        app_pos[(size_t)list * list_cap + e] = make_float4(0.f, 0.f, 0.f, 0.f);
        app_ray[(size_t)list * list_cap + e] = 0;
    }
}

// The feature rows of `count` slots from `slot` on, whose entries this wave has just written or voided (ROWS frames: whoever writes or
// voids app_pos[slot] also writes feat[slot], with what k_app_features_vol computes from that entry). slot / count wave-uniform.
__device__ __forceinline__ void slot_rows(const FieldDev& F, const float4* __restrict__ app_pos, float* __restrict__ feat, size_t slot,
                                          unsigned count, int lane) {
    if (!count) return;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the entries have reached L2: av_slot_rows reads them back there
    const AvVolume vol{F.avol, F.av_row, F.av_slice, (unsigned)F.app.H[0] + 1u};
    av_slot_rows(F.app, vol, app_pos + slot, feat + slot * 32u, count, lane);
}

// ---- STAGE: the tail's rows from corner boxes staged in LDS ---------------------------------------------------------------------------
// The 64 rays of a tile are less than a voxel apart, so all entries a step pair emits lie in the pair's tap box (<= 4 x 4 x 4 corners,
// the box whose summed-table entries the pair read). The step loop logs every emitting pair (box origin, the ballots of the lanes that
// emitted at step 0 / step 1) in a wave-private LDS log; the tail then walks its entries in EMISSION order instead of list order: per
// logged pair it copies the box's corners from the volume to LDS once (8 coalesced wave loads instead of 8 x 128 B per entry) and
// every row pass reads its eight corners there — no pass holds a dependent global load. Slots, entries and rows are what the direct
// tail writes, bit for bit. A wave whose log overflowed, or that emitted on a pair that does not fit one box, runs the direct tail.
// Per wave: the box | count, direct flag | the log.
constexpr int kRsLogMax = 32;
constexpr unsigned kRsBoxBytes = 64u * kAvBoxCornerBytes;
constexpr unsigned kRsHdrBytes = 16u;
constexpr unsigned kRsRecWords = 6u;                  // origin (10 bits per axis), spare, ballot of step 0 (lo, hi), ballot of step 1 (lo, hi)
constexpr unsigned kRsWaveBytes = kRsBoxBytes + kRsHdrBytes + (unsigned)kRsLogMax * kRsRecWords * 4u;
static_assert(4u * kRsWaveBytes <= 32768u && kRsWaveBytes % 16u == 0u, "five blocks per CU: at most 32 KB of LDS per block; 16-B aligned regions");

// the corners of the box at (ox, oy, oz) -> registers: load j covers corners 8 j .. 8 j + 7, lane = corner 8 j + lane / 8, quad lane % 8
// (one wave instruction = eight whole corners; quad 7 is not needed). Corners past the padded volume's last index read that index.
struct RsBoxRegs { float4 p0, p1, p2, p3, p4, p5, p6, p7; };   // (named members: an array indexed in an unrolled loop stays in scratch)
template <int J>
__device__ __forceinline__ float4 rs_corner_load(const FieldDev& F, unsigned xq, int oy, int oz, int lane) {
    const unsigned cy = (unsigned)min(oy + ((J & 1) * 2 + (lane >> 5)), F.app.H[0]), cz = (unsigned)min(oz + (J >> 1), F.app.H[1]);
    const unsigned off = umad24(umad24(cz, (unsigned)F.app.H[0] + 1u, cy), F.av_row, xq);
    return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(F.avol) + off);
}
__device__ __forceinline__ RsBoxRegs rs_box_load(const FieldDev& F, int ox, int oy, int oz, int lane) {
    // (the eighth lane of a corner repeats quad 6: nothing of it is kept)
    const unsigned xq = (unsigned)min(ox + ((lane >> 3) & 3), F.app.W[0]) * kAvCornerBytes + (unsigned)min(lane & 7, 6) * 16u;
    RsBoxRegs b;
    b.p0 = rs_corner_load<0>(F, xq, oy, oz, lane); b.p1 = rs_corner_load<1>(F, xq, oy, oz, lane);
    b.p2 = rs_corner_load<2>(F, xq, oy, oz, lane); b.p3 = rs_corner_load<3>(F, xq, oy, oz, lane);
    b.p4 = rs_corner_load<4>(F, xq, oy, oz, lane); b.p5 = rs_corner_load<5>(F, xq, oy, oz, lane);
    b.p6 = rs_corner_load<6>(F, xq, oy, oz, lane); b.p7 = rs_corner_load<7>(F, xq, oy, oz, lane);
    return b;
}
// one dword of each of the box's 64 corners (lane = corner): their lines are on the way to the CU's L1; the caller hands the value to
// rs_touch_done behind the work the fetch runs beside (an unused load would be dropped, a volatile one waited for at once)
__device__ __forceinline__ unsigned rs_box_touch(const FieldDev& F, int ox, int oy, int oz, int lane) {
    const unsigned cx = (unsigned)min(ox + (lane & 3), F.app.W[0]), cy = (unsigned)min(oy + ((lane >> 2) & 3), F.app.H[0]);
    const unsigned cz = (unsigned)min(oz + (lane >> 4), F.app.H[1]);
    const unsigned off = umad24(umad24(cz, (unsigned)F.app.H[0] + 1u, cy), F.av_row, cx * kAvCornerBytes);
    return *reinterpret_cast<const unsigned*>(reinterpret_cast<const char*>(F.avol) + off);
}
__device__ __forceinline__ void rs_touch_done(unsigned v) { asm volatile("" ::"v"(v)); }
__device__ __forceinline__ void rs_box_store(char* __restrict__ box, int lane, const RsBoxRegs& b) {
    if ((lane & 7) < 7) {
        constexpr int S = 8 * (int)kAvBoxCornerBytes;
        char* __restrict__ d = box + (unsigned)(lane >> 3) * kAvBoxCornerBytes + (unsigned)(lane & 7) * 16u;
        *reinterpret_cast<float4*>(d) = b.p0;         *reinterpret_cast<float4*>(d + S) = b.p1;
        *reinterpret_cast<float4*>(d + 2 * S) = b.p2; *reinterpret_cast<float4*>(d + 3 * S) = b.p3;
        *reinterpret_cast<float4*>(d + 4 * S) = b.p4; *reinterpret_cast<float4*>(d + 5 * S) = b.p5;
        *reinterpret_cast<float4*>(d + 6 * S) = b.p6; *reinterpret_cast<float4*>(d + 7 * S) = b.p7;
    }
}
__device__ __forceinline__ int rs_permute(int dest, int v) { return __builtin_amdgcn_ds_permute(dest << 2, v); }
// The rows of the entries one step of a logged pair emitted: `mask` = the lanes that hold one (`ent`, list slot `slot`). The entries are
// compacted across lanes (rank by mbcnt, forward permute; the other lanes fill the positions behind them), then eight entries per pass,
// eight lanes per entry, as in av_slot_rows.
__device__ __forceinline__ void rs_rows(const FieldDev& F, const AvVolume& vol, const AvBox& box, unsigned long long mask, const float4 ent,
                                        unsigned slot, float* __restrict__ feat, int lane) {
    const int cnt = __popcll(mask);
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
    const bool bit = (mask >> lane) & 1ull;
    const int dest = bit ? rank : cnt + (lane - rank);
    const int px = rs_permute(dest, __float_as_int(ent.x)), py = rs_permute(dest, __float_as_int(ent.y)), pz = rs_permute(dest, __float_as_int(ent.z));
    const int pw = rs_permute(dest, __float_as_int(ent.w)), ps = rs_permute(dest, (int)slot);
    const int e = lane >> 3, q = lane & 7;
#pragma unroll 1
    for (int s0 = 0; s0 < cnt; s0 += 8) {
        const int src = s0 + e;
        const float4 mine = make_float4(__int_as_float(__shfl(px, src)), __int_as_float(__shfl(py, src)), __int_as_float(__shfl(pz, src)),
                                        __int_as_float(__shfl(pw, src)));
        const unsigned sl = (unsigned)__shfl(ps, src);
        const bool live = src < cnt;
        av_feature_row<8>(F.app, vol, mine, live, q, feat + (size_t)(live ? sl : 0u) * 32u + 4u * (unsigned)q, live, box);
    }
}

constexpr int kDenseLd = 20;                          // floats per ray row of the transpose tile (16 steps + pad, 16-B aligned)
constexpr int kDenseFloats = 64 * kDenseLd;           // per wave: the weights tile
struct __attribute__((aligned(4))) F4U { float x, y, z, w; };   // row segments of an [n_rays, N] tensor are only 4-B aligned for odd N

// Waves per SIMD the register allocation targets. The step loop is a load -> MFMA -> LDS -> read chain that only other waves
// hide: 3 waves 0.95 ms, 4 waves (109 VGPRs) 0.78, 5 waves (96 VGPRs; ten loop-invariant dwords go to scratch and come back
// only where an appearance entry is stored) 0.74, 6 waves (80 VGPRs, 104 B of scratch in the loop) 0.86. The weights-writing
// variant (121 VGPRs) spills inside its loop at 5 (1.46 ms against 1.37 for fill + march) and stays at 4.
#ifndef T2N_MT_WAVES
#define T2N_MT_WAVES 5
#endif
#ifndef T2N_MTD_WAVES
#define T2N_MTD_WAVES 4
#endif
// the instantiations that read the cached table (CACHED): no operand loads, no MFMA results and no LDS table are live in the step loop.
// C2 frame, the marcher's own time: 5 waves (91 VGPRs, no scratch, no LDS) 0.376 / 0.377 / 0.380 ms, 6 waves (80 VGPRs, 48 B of scratch
// per lane) 0.381 / 0.384 / 0.387, 4 waves (104 VGPRs) the same frame time as 5; the weights-writing variant (112 VGPRs, the 20-KB
// transpose tile its only LDS) stays at 4 (profiles/march_density_cache_ab.txt).
#ifndef T2N_MTC_WAVES
#define T2N_MTC_WAVES 5
#endif
#ifndef T2N_MTCD_WAVES
#define T2N_MTCD_WAVES 4
#endif
// -DMT_PROF (timing-only build): s_memtime at the region boundaries of a step pair, summed per wave. With five waves per SIMD a
// region's cycles include what the SIMD gave to the other four meanwhile: the sums say where a wave's time goes, not what the
// instructions cost alone.
#ifdef MT_PROF
#define MT_T(var) do { const unsigned long long tn = __builtin_readcyclecounter(); var += tn - p_t; p_t = tn; } while (0)
#else
#define MT_T(var) do {} while (0)
#endif
// ALPHA: the field carries an AlphaGridMask; RELU: fea2denseAct = relu. Compile-time, like the absent NDC depth table (the host never
// sends NDC renders here): the step loop of the driver's configuration (no mask, softplus) carries neither the mask's eight-tap
// gather with its 64-bit address arithmetic nor a run-time test per sample and option.
// CACHED: the field carries the summed table of its whole grid (FieldDev::dsum): a step pair inside the table's reach reads its entries
// there instead of building its 4 x 4 x 4 piece (same bits, see cached_read3). The uncached kernel serves every sample from a table as
// well (one build for a pair that fits a box, the loop over boxes for one that does not), so the cached one decides nothing: the tap
// bit set, its reduction and the branch go with the operand loads, the MFMAs, the LDS table, its sum pass and the three fences. Only an
// EMITTING pair of a STAGE frame still works out its tap box (pair_box, for the log).
constexpr int mt_waves(bool dense, bool cached) { return cached ? (dense ? T2N_MTCD_WAVES : T2N_MTC_WAVES) : (dense ? T2N_MTD_WAVES : T2N_MT_WAVES); }
// ROWS (CACHED && !DENSE frames that hold the current feature volume and a row per list slot, launch_march_tiles): the wave's tail
// also produces the feature rows of the slots it filled or voided — eight corner fetches and 64 multiply-adds per entry, work bound by
// the texture addresser that runs beside the other waves' marching (bound by VALU issue) instead of in a kernel of its own behind
// this one. Everything the step loop kept in registers is dead by then: the step loop's allocation is what it was.
// STAGE (ROWS only): the tail's rows from corner boxes staged in LDS, see kRsLogMax above.
template <bool DENSE, bool ALPHA = false, bool RELU = false, bool CACHED = false, bool ROWS = false, bool STAGE = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(mt_waves(DENSE, CACHED), mt_waves(DENSE, CACHED)))) void k_march_tiles(const TileArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    float* __restrict__ stD = smem + (size_t)wid * kStageFloats;   // (CACHED: no table area)
    if constexpr (!CACHED) {
        for (int i = lane; i < kStageFloats; i += 64) stD[i] = 0.f;   // the padding behind S stays zero (table_read3 may touch it with weight 0)
        lds_fence_w();
    }
    float* __restrict__ wt = smem + (CACHED ? 0 : 4 * kStageFloats) + (size_t)wid * kDenseFloats;   // DENSE only
    const FieldDev& F = a.F;
    static_assert(!STAGE || ROWS, "staged rows: a tail that writes rows");
    // STAGE only: box | header | log (the wave's offset as a scalar: a lane value would sit in a register pair across the step loop)
    char* __restrict__ rs_box = reinterpret_cast<char*>(smem) + (unsigned)__builtin_amdgcn_readfirstlane(wid) * kRsWaveBytes;
    unsigned* __restrict__ rs_hdr = reinterpret_cast<unsigned*>(rs_box + kRsBoxBytes);
    if constexpr (STAGE) {
        if (lane == 0) { rs_hdr[0] = 0u; rs_hdr[1] = 0u; }   // logged pairs, direct flag (written and read in the loop by lane 0 alone)
    }
    const int tiles_x = (a.img_w + 7) >> 3;
    const long long tile = (long long)blockIdx.x * 4 + wid;
    const int ty = (int)(tile / tiles_x), tx = (int)(tile - (long long)ty * tiles_x);
    const int px = tx * 8 + (lane & 7), py = ty * 8 + (lane >> 3);
    if (ty * 8 >= a.img_h) return;
    const bool have = px < a.img_w && py < a.img_h;
    // (STAGE: the ray index in one register — a launch's rays fit an int, as its list slots do — the staged tail leaves no room for two)
    typedef typename std::conditional<STAGE, int, long long>::type ray_t;
    const ray_t r = have ? (ray_t)((long long)py * a.img_w + px) : 0;
    const int N = a.n_samples;
    Ray ray;
    if (have) ray = load_ray(F, a.rays + (long long)r * a.ray_stride, a.ray_stride);
    else { ray.ox = ray.oy = ray.oz = 1e30f; ray.dx = ray.dy = ray.dz = 0.f; ray.tmin = 0.f; ray.last = 0.f; }
    int lo = N, hi = -1;
    if (have) ray_interval<false>(F, ray, N, lo, hi);
    const int wlo = wave_min_i(lo), whi = wave_max_i(hi);

    float T = 1.f, acc = 0.f, dep = 0.f;
    int first = -1, last = -1;
    unsigned napp = 0;
    int nev = 0;         // evaluated samples (the window [first, last] is the box window: it has gaps under an alpha mask)
    int ovf_from = 0;    // first sample whose weight went to wbuf instead of the (full) staging slice

    // row segments of the transpose flush: lane -> (ray rho = lane / 4 + 16 j, columns 4 (lane & 3) .. + 3), j = 0..3
    long long frow[4];
    if constexpr (DENSE) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int rho = (lane >> 2) + 16 * j;
            const int fx = tx * 8 + (rho & 7), fy = ty * 8 + (rho >> 3);
            frow[j] = (fx < a.img_w && fy < a.img_h) ? ((long long)fy * a.img_w + fx) * N : -1;
        }
    }
    // kSteps consecutive samples per ray share ONE table build: the tap ranges of neighbouring steps overlap (the union of two
    // steps spans 3-4 taps per axis on every pair of a pinhole frame), so the reduction, the six operand loads, the twelve
    // MFMAs and the load -> MFMA -> LDS latency chain are paid once per pair.
    constexpr int kSteps = 2;
    // DENSE: whole 16-step blocks of the weights rows (a wave without samples runs no step: wlo = N, whi = -1)
    const int i_begin = DENSE ? (wlo & ~15) : wlo, i_end = DENSE ? min(N - 1, whi | 15) : whi;
    // early termination (t2n_field_set_early_termination; never with weights rows): a ray below term_eps evaluates nothing further,
    // the wave leaves the loop when none of its rays has anything left to evaluate
    const float eps = DENSE ? 0.f : F.term_eps;
    bool dead = false;   // this ray is below term_eps (as of the last look)
#ifdef MT_PROF
    unsigned long long p_coord = 0, p_axes = 0, p_build = 0, p_read = 0, p_act = 0, p_pairs = 0;
    const unsigned long long p_start = __builtin_readcyclecounter();
    unsigned long long p_t = p_start;
#endif
    for (int i = i_begin; i <= i_end; i += kSteps) {
        // looked at every eighth step pair, and the rays' own gate is refreshed only there: a test of the CURRENT transmittance in front of
        // every step pair chains each iteration to the one before (the step pair's gathers cannot start before the previous pair's
        // compositing is done) — 3 % of a frame on a scene where nothing terminates
        if (eps > 0.f && (((i - i_begin) & 15) == 0)) {
            dead = T < eps;
            if (!__any(have && i <= hi && !dead)) break;
        }
        float xn[kSteps], yn[kSteps], zn[kSteps], z[kSteps], w_out[kSteps];
        bool ok[kSteps];
        Axes3 A[kSteps];
        bool any_ok = false;
#pragma unroll
        for (int q = 0; q < kSteps; ++q) {
            const int idx = i + q;
            xn[q] = yn[q] = zn[q] = z[q] = w_out[q] = 0.f;
            ok[q] = false;
            if (have && idx >= lo && idx <= hi && idx <= i_end && !dead) {
                z[q] = sample_z<false, true>(F, ray, idx, 0.f);
                ok[q] = sample_point<false>(F, ray, z[q], xn[q], yn[q], zn[q]);
                if constexpr (ALPHA) {
                    // the record's window is the box window (box test and z gate), as k_march's: the mask leaves gaps inside it
                    if (ok[q]) {
                        if (first < 0) first = idx;
                        last = idx;
                        ok[q] = alpha_pass(F, ray, z[q]);      // models/tensorBase.py:451-456
                    }
                }
            }
            any_ok |= ok[q];
        }
        const unsigned long long okm = __ballot(any_ok);
        MT_T(p_coord);
        // (a lane whose staging slice is full keeps its spill row gap-free: masked-out samples inside its window get zeros)
        if (!DENSE && !okm && !__any(have && napp >= (unsigned)a.cap)) continue;
        float part[kSteps];
#pragma unroll
        for (int q = 0; q < kSteps; ++q) part[q] = 0.f;
        unsigned emv = 0u;           // STAGE: bit q = the lane stored an entry at step q (one register: masks kept per step cost four scalars)
        if (okm) {
#pragma unroll
            for (int q = 0; q < kSteps; ++q) A[q] = sample_axes_inbox(F.den, xn[q], yn[q], zn[q]);   // used by samples inside the box only (ok[q])
            if constexpr (CACHED) {
                MT_T(p_axes);
                // every sample reads its cell in the table of the whole grid: nothing to decide. Both samples' eight loads in flight
                // together; a lane without a sample reads the table's first cell
                unsigned off[kSteps];
                CellTaps ct[kSteps];
#pragma unroll
                for (int q = 0; q < kSteps; ++q) off[q] = ok[q] ? cached_offset(F, A[q]) : 0u;
#pragma unroll
                for (int q = 0; q < kSteps; ++q) ct[q] = cached_load(F, off[q]);
                MT_T(p_build);
#pragma unroll
                for (int q = 0; q < kSteps; ++q)
                    if (ok[q]) part[q] = cached_read3(A[q], ct[q]);
                MT_T(p_read);
            } else {
                // the table of the box at amn[] -> the wave's LDS area; returns the origin's part of a sample's offset
                auto build_at = [&](const int (&amn)[3]) {
                    table_build<2>(F.den, amn, stD, l15, lq);
                    lds_fence_w();
                    {
                        // (the lane index behind an opaque copy, per build: visible, the sum pass's three lane offsets are hoisted out of
                        // the step loop and spilled)
                        int ln = lane;
                        asm volatile("" : "+v"(ln));
                        table_sum<2>(stD, ln);
                    }
                    lds_fence_w();
                    // (the origin's offset as ONE scalar the compiler cannot take apart again: left visible it subtracts the three
                    // amn[] from the three tap indices of every sample, one vector instruction each)
                    int org = (amn[2] << 4) + (amn[1] << 2) + amn[0];
                    asm volatile("" : "+s"(org));
                    return org;
                };
                int amn[3];
                const bool fits = pair_box(A, ok, okm, amn);
                MT_T(p_axes);
                if (fits) {
                    const int org = build_at(amn);
                    MT_T(p_build);
#pragma unroll
                    for (int q = 0; q < kSteps; ++q)
                        if (ok[q]) part[q] = table_read3(A[q], org, stD);
                    lds_fence_w();
                    MT_T(p_read);
                } else {
                    // a pair wider than one table: a wave-uniform loop over boxes. The box at the low taps of the first sample not yet
                    // served is built as above; every unserved sample whose cell lies in it (low taps origin .. origin + 2 per axis)
                    // reads its feature there. An entry of S is a function of its texel alone, so the samples get the bits of the
                    // one-build form and of the whole-grid table, whichever box serves them. The lead lane's sample is served by
                    // its own box: every trip serves at least one sample.
                    // (the taps are computed again from the coordinates on both sides of a build, behind opaque copies: the eighteen
                    // values of A[] kept across the builds and the loop's back edge push loop-carried values of the step loop to
                    // scratch; a trip's 70 VALU more are nothing beside its build)
                    unsigned todo = (ok[0] ? 1u : 0u) | (ok[1] ? 2u : 0u);
                    unsigned long long tm = okm;
#pragma unroll 1
                    do {
                        const int lead = (int)__builtin_ctzll(tm);
                        int bx[3];
                        {
                            const bool s1 = !(todo & 1u);   // the lane's first unserved sample
                            float x = s1 ? xn[1] : xn[0], y = s1 ? yn[1] : yn[0], zz = s1 ? zn[1] : zn[0];
                            asm volatile("" : "+v"(x), "+v"(y), "+v"(zz));
                            const Axes3 B = sample_axes_inbox(F.den, x, y, zz);
                            // (opaque again: the compiler moves a readlane in front of the arithmetic that feeds it, and the taps of
                            // the lead lane's coordinates come out of vector instructions, not in scalars)
                            int b0 = B.a[0].i0, b1 = B.a[1].i0, b2 = B.a[2].i0;
                            asm volatile("" : "+v"(b0), "+v"(b1), "+v"(b2));
                            bx[0] = __builtin_amdgcn_readlane(b0, lead); bx[1] = __builtin_amdgcn_readlane(b1, lead);
                            bx[2] = __builtin_amdgcn_readlane(b2, lead);
                        }
                        const int org = build_at(bx);
#pragma unroll   // (a rolled loop would index the per-sample arrays dynamically and push them to scratch)
                        for (int q = 0; q < kSteps; ++q) {
                            float x = xn[q], y = yn[q], zz = zn[q];
                            asm volatile("" : "+v"(x), "+v"(y), "+v"(zz));
                            const Axes3 B = sample_axes_inbox(F.den, x, y, zz);
                            const bool in = (unsigned)(B.a[0].i0 - bx[0]) <= 2u && (unsigned)(B.a[1].i0 - bx[1]) <= 2u &&
                                            (unsigned)(B.a[2].i0 - bx[2]) <= 2u;
                            if (((todo >> q) & 1u) && in) {
                                part[q] = table_read3(B, org, stD);
                                todo &= ~(1u << q);
                            }
                        }
                        lds_fence_w();   // the reads of this box are done before the next build overwrites it
                        tm = __ballot(todo != 0u);
                    } while (tm);
                    MT_T(p_read);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < kSteps; ++q) {
            const int idx = i + q;
            const bool spill = have && idx <= i_end && napp >= (unsigned)a.cap && !DENSE;
            if (ok[q]) {
                const float sg = feature2density<RELU ? T2N_ACT_RELU : T2N_ACT_SOFTPLUS>(F, part[q]);
                const float dist = idx < N - 1 ? sample_z<false, true>(F, ray, idx + 1, 0.f) - z[q] : 0.f;     // :448
                const float alpha = 1.f - exp_finite((-sg) * (dist * F.dscale));                      // raw2alpha :19-26 (argument <= 0)
                const float w = alpha * T;
                T = T * ((1.f - alpha) + 1e-10f);
                acc += w;
                dep = fmaf(w, z[q], dep);
                // in-kernel compaction: (x, y, z, w) of the samples above the threshold go to the ray's staging slice
                if (w > F.thres) {
                    if (napp < (unsigned)a.cap) {
                        a.scratch[(size_t)r * a.cap + napp] = make_float4(xn[q], yn[q], zn[q], w);
                        if constexpr (STAGE) emv |= 1u << q;
                    }
                    ++napp;
                    if (napp == (unsigned)a.cap) ovf_from = idx + 1;
                }
                if constexpr (!ALPHA) {
                    if (first < 0) first = idx;
                    last = idx;
                }
                ++nev;
                w_out[q] = w;
            }
            if (spill) a.wbuf[(long long)r * N + idx] = w_out[q];
            if constexpr (DENSE) {
                if (idx < N) {
                    const int c16 = idx & 15;
                    wt[lane * kDenseLd + c16] = w_out[q];
                }
                if ((idx < N && (idx & 15) == 15) || idx == N - 1) {
                    lds_fence_w();
                    const int col = (idx & ~15) + 4 * (lane & 3);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (frow[j] < 0 || col >= N) continue;
                        const int rho = (lane >> 2) + 16 * j;
                        const float4 vw = *reinterpret_cast<const float4*>(wt + rho * kDenseLd + 4 * (lane & 3));
                        if (col + 3 < N) {
                            *reinterpret_cast<F4U*>(a.dense_w + frow[j] + col) = F4U{vw.x, vw.y, vw.z, vw.w};
                        } else {
                            const float ew[4] = {vw.x, vw.y, vw.z, vw.w};
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (col + e < N) a.dense_w[frow[j] + col + e] = ew[e];
                        }
                    }
                    lds_fence_w();
                }
            }
        }
        if constexpr (STAGE) {
            // an emitting pair: one record (lane 0), or the wave's tail turns direct (pair wider than one box, log full)
            if (__any(emv != 0u)) {
                // the pair's tap box, needed here alone (a few pairs per wave emit): over ALL live samples of the pair, emitting or
                // not, by the uncached kernel's rule. The taps are computed again from the coordinates, behind opaque copies: kept
                // from the step's own computation they would stay in registers across the compositing.
                unsigned bo = 0u;    // the pair fits one 4 x 4 x 4 box (bit 30) and the box origin, 10 bits per axis, in ONE scalar
                {
                    Axes3 B[kSteps];
#pragma unroll
                    for (int q = 0; q < kSteps; ++q) {
                        float x = xn[q], y = yn[q], zz = zn[q];
                        asm volatile("" : "+v"(x), "+v"(y), "+v"(zz));
                        B[q] = sample_axes_inbox(F.den, x, y, zz);
                    }
                    int amn[3];
                    if (pair_box(B, ok, okm, amn)) bo = 0x40000000u | (unsigned)amn[0] | (unsigned)amn[1] << 10 | (unsigned)amn[2] << 20;
                }
                const unsigned long long b0 = __ballot((emv & 1u) != 0u), b1 = __ballot((emv & 2u) != 0u);
                if (lane == 0) {
                    const unsigned c = rs_hdr[0];
                    if (!bo || c >= (unsigned)kRsLogMax) rs_hdr[1] = 1u;
                    else {
                        unsigned* __restrict__ rec = rs_hdr + 4 + c * kRsRecWords;
                        rec[0] = bo; rec[1] = 0u;
                        rec[2] = (unsigned)b0; rec[3] = (unsigned)(b0 >> 32); rec[4] = (unsigned)b1; rec[5] = (unsigned)(b1 >> 32);
                        rs_hdr[0] = c + 1u;
                    }
                }
            }
        }
#ifdef MT_PROF
        MT_T(p_act); ++p_pairs;
#endif
    }
#ifdef MT_PROF
    if (lane == 0 && a.prof) {
        unsigned long long* o = a.prof + (size_t)(blockIdx.x * 4 + wid) * 8;
        o[0] = p_coord; o[1] = p_axes; o[2] = p_build; o[3] = p_read; o[4] = p_act; o[5] = p_pairs; o[6] = __builtin_readcyclecounter() - p_start;
    }
#endif
    const int Lw = last >= first && first >= 0 ? last - first + 1 : 0;
    if (have) {
        a.acc[r] = acc;
        a.depth[r] = dep + (1.f - acc) * ray.last;                                         // :504-505
    }
    // ---- in-kernel compaction: one list reservation per wave -------------------------------------------------------------
    const bool over = have && napp > (unsigned)a.cap;
    const unsigned n = (have && !over) ? napp : 0u;
    unsigned incl = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    const unsigned total = __shfl(incl, 63);
    const unsigned list = blockIdx.x & 7u;   // the block's XCD: the reservation atomic stays in that XCD's L2
    unsigned base = 0;
    if (lane == 0 && total) base = atomicAdd(&a.counters[list * kCounterStride], total);
    base = __shfl(base, 0);
    // a region that does not fit its sub-list (small or ragged frames put many tiles on one list): the wave's rays take the
    // per-ray route below, which tries every sub-list; the inflated counter is clamped to list_cap by its readers
    const bool fits = base + total <= a.list_cap;
    if (!fits && total) void_entries(a.app_pos, a.app_ray, list, a.list_cap, base, base + total, lane);
    const unsigned slot0 = list * a.list_cap + base + (incl - n);
    // STAGE: the wave's tail runs staged when its region fits and every emitting pair is in the log
    unsigned rs_n = 0u;
    bool staged = false;
    if constexpr (STAGE) {
        lds_fence_w();
        rs_n = (unsigned)__builtin_amdgcn_readfirstlane((int)rs_hdr[0]);
        const unsigned flag = (unsigned)__builtin_amdgcn_readfirstlane((int)rs_hdr[1]);
        staged = __builtin_amdgcn_readfirstlane((int)(fits && total)) && !flag;
#ifdef T2N_MT_NO_TAIL_ROWS
        staged = false;   // (timing-only build: the copy loop still fills the list)
#endif
    }
    if (have) {
        if (over || !fits) {
            const unsigned k = atomicAdd(a.ovf_count, 1u);
            a.ovf_list[k] = (int)r;
            a.ray_app[r] = make_int4(ovf_from, (int)napp, nev, Lw > 0 ? (first | (Lw << 11)) : 0);   // k_compact_list finishes this ray
        } else {
            a.ray_app[r] = make_int4((int)slot0, fits ? (int)n : 0, nev, Lw > 0 ? (first | (Lw << 11)) : 0);
            if (fits && !staged) {
                // four entries in flight per trip (a wave's tail lasts as long as its longest slice; one dependent round trip
                // per entry otherwise)
                const float4* __restrict__ src = a.scratch + (size_t)r * a.cap;
                for (unsigned k = 0; k < n; k += 4) {
                    const float4 e0 = src[k], e1 = src[k + 1 < n ? k + 1 : n - 1], e2 = src[k + 2 < n ? k + 2 : n - 1],
                                 e3 = src[k + 3 < n ? k + 3 : n - 1];
                    a.app_pos[slot0 + k] = e0; a.app_ray[slot0 + k] = (int)r;
                    if (k + 1 < n) { a.app_pos[slot0 + k + 1] = e1; a.app_ray[slot0 + k + 1] = (int)r; }
                    if (k + 2 < n) { a.app_pos[slot0 + k + 2] = e2; a.app_ray[slot0 + k + 2] = (int)r; }
                    if (k + 3 < n) { a.app_pos[slot0 + k + 3] = e3; a.app_ray[slot0 + k + 3] = (int)r; }
                }
            }
        }
    }
    if constexpr (ROWS) {
        static_assert(CACHED && !DENSE, "rows in the tail: cached, weight-free frames only");
#ifndef T2N_MT_NO_TAIL_ROWS   // (timing-only build without the tails' rows: the frame's colours are invalid)
        // the wave's region of the list: its rays' entries (fits), or what void_entries defined below list_cap
        const unsigned ubase = (unsigned)__builtin_amdgcn_readfirstlane((int)base), utotal = (unsigned)__builtin_amdgcn_readfirstlane((int)total);
        unsigned cnt = utotal;
        if (ubase + utotal > a.list_cap) cnt = ubase < a.list_cap ? a.list_cap - ubase : 0u;
        if constexpr (STAGE) {
            // proof of path: one fire-and-forget atomic per wave with rows, on the XCD's counter line
            if (lane == 0 && cnt) atomicAdd(&a.counters[list * kCounterStride + (staged ? kRowsStagedWord : kRowsDirectWord)], 1u);
#ifdef T2N_RS_STATS   // (instrumented build: logged pairs and entries of the staged waves, words 52 / 53 of the XCD's counter line)
            if (lane == 0 && staged) { atomicAdd(&a.counters[list * kCounterStride + 52], rs_n); atomicAdd(&a.counters[list * kCounterStride + 53], utotal); }
#endif
            if (staged) {
                const AvVolume vol{F.avol, F.av_row, F.av_slice, (unsigned)F.app.H[0] + 1u};
                const unsigned long long mine_m = __ballot(have && !over);   // (a ray handed to k_compact_list contributes nothing here)
                // (the ray's staging slice from its index at every use: the address would sit in a register pair across the passes)
                auto entry_at = [&](unsigned k) {
                    int rr = (int)r;
                    asm volatile("" : "+v"(rr));
                    return a.scratch[(size_t)rr * a.cap + k];
                };
                const unsigned* __restrict__ log = rs_hdr + 4;
                const unsigned last_k = (unsigned)a.cap - 1u;
                // per record: the box to LDS, then the passes of its entries. While record m's passes run, the entries of record m + 1 are
                // on their way to registers and the 64 lines of box m + 1 to this CU's L1 (rs_box_touch: the five-wave allocation has no
                // room for a box in registers beside a pass), so the box load in front of a record's passes is a short round trip.
                float4 ne0, ne1;
                unsigned long long nm0, nm1;
                unsigned kc = 0u;    // entries of this lane's ray walked so far
                nm0 = ((unsigned long long)log[3] << 32 | log[2]) & mine_m; nm1 = ((unsigned long long)log[5] << 32 | log[4]) & mine_m;
                nm0 = (unsigned long long)__builtin_amdgcn_readfirstlane((int)(nm0 >> 32)) << 32 | (unsigned)__builtin_amdgcn_readfirstlane((int)nm0);
                nm1 = (unsigned long long)__builtin_amdgcn_readfirstlane((int)(nm1 >> 32)) << 32 | (unsigned)__builtin_amdgcn_readfirstlane((int)nm1);
                unsigned nbo = (unsigned)__builtin_amdgcn_readfirstlane((int)log[0]);
                ne0 = entry_at(min(kc, last_k));
                ne1 = entry_at(min(kc + (unsigned)((nm0 >> lane) & 1ull), last_k));
#pragma unroll 1
                for (unsigned m = 0; m < rs_n; ++m) {
                    // (a record whose emitting rays were all handed to k_compact_list later has nothing left: no box, no passes)
                    const bool work = (nm0 | nm1) != 0ull;
                    const AvBox box{rs_box, (int)(nbo & 1023u), (int)((nbo >> 10) & 1023u), (int)((nbo >> 20) & 1023u)};
                    if (work) rs_box_store(rs_box, lane, rs_box_load(F, box.ox, box.oy, box.oz, lane));
                    const float4 e0 = ne0, e1 = ne1;
                    const unsigned long long m0 = nm0, m1 = nm1;
                    const bool bit0 = (m0 >> lane) & 1ull, bit1 = (m1 >> lane) & 1ull;
                    const unsigned k0 = kc, k1 = kc + (bit0 ? 1u : 0u);
                    kc = k1 + (bit1 ? 1u : 0u);
                    lds_fence_w();
                    unsigned touched = 0u;
                    if (m + 1 < rs_n) {
                        const unsigned* __restrict__ rec = log + (m + 1) * kRsRecWords;
                        nm0 = ((unsigned long long)rec[3] << 32 | rec[2]) & mine_m; nm1 = ((unsigned long long)rec[5] << 32 | rec[4]) & mine_m;
                        nm0 = (unsigned long long)__builtin_amdgcn_readfirstlane((int)(nm0 >> 32)) << 32 | (unsigned)__builtin_amdgcn_readfirstlane((int)nm0);
                        nm1 = (unsigned long long)__builtin_amdgcn_readfirstlane((int)(nm1 >> 32)) << 32 | (unsigned)__builtin_amdgcn_readfirstlane((int)nm1);
                        nbo = (unsigned)__builtin_amdgcn_readfirstlane((int)rec[0]);
                        if (nm0 | nm1) {
                            touched = rs_box_touch(F, (int)(nbo & 1023u), (int)((nbo >> 10) & 1023u), (int)((nbo >> 20) & 1023u), lane);
                            ne0 = entry_at(min(kc, last_k));
                            ne1 = entry_at(min(kc + (unsigned)((nm0 >> lane) & 1ull), last_k));
                        }
                    }
                    if (work) {
                        // the entries to their slots (the values and slots of the direct tail's copy loop), then their rows
                        if (bit0) { a.app_pos[slot0 + k0] = e0; a.app_ray[slot0 + k0] = (int)r; }
                        if (bit1) { a.app_pos[slot0 + k1] = e1; a.app_ray[slot0 + k1] = (int)r; }
#pragma unroll 1   // (one copy of the passes: two inlined copies push the tail past the five-wave allocation)
                        for (int q = 0; q < kSteps; ++q)
                            rs_rows(F, vol, box, q ? m1 : m0, q ? e1 : e0, slot0 + (q ? k1 : k0), a.feat, lane);
                    }
                    rs_touch_done(touched);
                    lds_fence_w();   // the passes' reads of box m are done before box m + 1 overwrites it
                }
            } else slot_rows(F, a.app_pos, a.feat, (size_t)list * a.list_cap + ubase, cnt, lane);
        } else slot_rows(F, a.app_pos, a.feat, (size_t)list * a.list_cap + ubase, cnt, lane);
#endif
    }
}

// The rays the tile marcher handed over: one wave per ray finishes their appearance slices.
struct CompactArgs {
    FieldDev F;
    const float* rays; long long n_rays; int ray_stride; int n_samples;
    const float* wbuf;                // spill rows (see TileArgs)
    int4* ray_app; float4* app_pos; int* app_ray; unsigned* counters; unsigned list_cap;
    unsigned long long* stats;
    const float4* scratch; int cap;   // the marcher's per-ray staging slices
    int finisher;                     // a ray that fits no sub-list is left to k_finish_rays (t2n_shade.hip) instead of losing its samples
    float* feat;                      // fused frames (TileArgs::feat): the rows of the slots this kernel fills or voids; else NULL
};
// lane 0 reserves `napp` slots on the first sub-list with room; returns (slot0, napp or 0 when nothing fits) to all lanes
// A ray that fits nowhere (budgeted lists, t2n_render_forward): with a finisher behind this kernel the ray keeps its hand-over record
// in ray_app — x = -(first spilled sample) - 1 < 0 tells k_composite that the ray owns no list entries, y stays its appearance
// count (k_ray_stats) — its slot of the overflow list is tagged (sign bit) and its entries are added to word kFailEntriesWord (the
// next frame's budget); k_finish_rays shades and composites such rays from their staging slice and spill row, no list needed.
__device__ __forceinline__ void reserve_slots(const CompactArgs& a, long long r, unsigned list, int lane, const int4 ra, unsigned& slot0,
                                              unsigned& napp, int* ovf_slot) {
    slot0 = 0;
    napp = (unsigned)__builtin_amdgcn_readfirstlane((int)napp);   // (every lane holds the ray's record)
    bool fits = napp == 0;
    for (unsigned att = 0; att < (unsigned)kLists && !fits; ++att) {     // first sub-list with room (a failed try leaves the
        const unsigned l = (list + att) & (unsigned)(kLists - 1);          // counter above list_cap: readers clamp it)
        unsigned s0 = 0xffffffffu;                                         // (no try: the list is full already)
        if (lane == 0 && a.counters[l * kCounterStride] + napp <= a.list_cap) s0 = atomicAdd(&a.counters[l * kCounterStride], napp);
        s0 = (unsigned)__builtin_amdgcn_readfirstlane((int)s0);
        if (s0 == 0xffffffffu) continue;
        if (s0 + napp <= a.list_cap) { slot0 = l * a.list_cap + s0; fits = true; }
        else if (s0 < a.list_cap) {                                        // lost a race for the list's tail: its part of the
            void_entries(a.app_pos, a.app_ray, l, a.list_cap, s0, a.list_cap, lane);   // list gets defined entries (and rows)
            if (a.feat) slot_rows(a.F, a.app_pos, a.feat, (size_t)l * a.list_cap + s0, a.list_cap - s0, lane);
        }
    }
    if (lane == 0) {
        if (fits || !a.finisher) a.ray_app[r] = make_int4((int)slot0, fits ? (int)napp : 0, ra.z, ra.w);
        else {
            a.ray_app[r] = make_int4(-ra.x - 1, (int)napp, ra.z, ra.w);
            *ovf_slot = (int)((unsigned)r | 0x80000000u);
            atomicAdd(&a.counters[kFailEntriesWord], napp);
        }
        if (!fits && !a.finisher && a.stats) a.stats[T2N_STAT_OVERFLOW] = 1ull;
        if (!fits) a.counters[kOverflowWord] = 1u;   // budgeted lists: read back by the host (the next frames' budget, list_retries)
    }
    if (!fits) napp = 0;
}
// append the entries of wbuf[r][from, end) above the threshold at slot0 + run.. (sample order)
__device__ __forceinline__ void compact_span(const CompactArgs& a, long long r, const Ray& ray, int from, int end, unsigned slot0, unsigned run,
                                             int lane) {
    const FieldDev& F = a.F;
    const int N = a.n_samples;
    for (int base = from; base < end; base += 64) {
        const int i = base + lane;
        const float w = i < end ? a.wbuf[r * N + i] : 0.f;
        const bool m = (i < end) & (w > F.thres);
        const unsigned long long bal = __ballot(m);
        if (m) {
            const unsigned pre = (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
            const float z = sample_z<false>(F, ray, i, 0.f);
            float xn, yn, zn;
            sample_point<false>(F, ray, z, xn, yn, zn);
            const unsigned s = slot0 + run + pre;
            a.app_pos[s] = make_float4(xn, yn, zn, w);
            a.app_ray[s] = (int)r;
        }
        run += (unsigned)__popcll(bal);
    }
}
// a ray the tile marcher handed over (staging slice full, or its wave's region did not fit the sub-list): the first
// min(napp, cap) entries sit in the staging slice, the rest in wbuf[r][from..]
__device__ __forceinline__ void compact_ray_staged(const CompactArgs& a, long long r, unsigned list, int lane, int* ovf_slot) {
    const int4 ra = a.ray_app[r];
    const int first = ra.w & 2047, Lw = ra.w >> 11, from = ra.x;
    unsigned napp = (unsigned)ra.y, slot0;
    reserve_slots(a, r, list, lane, ra, slot0, napp, ovf_slot);
    const unsigned staged = napp < (unsigned)a.cap ? napp : (unsigned)a.cap;
    for (unsigned k = (unsigned)lane; k < staged; k += 64u) {
        a.app_pos[slot0 + k] = a.scratch[(size_t)r * a.cap + k];
        a.app_ray[slot0 + k] = (int)r;
    }
    if (napp > staged) {
        const Ray ray = load_ray(a.F, a.rays + r * a.ray_stride, a.ray_stride);
        compact_span(a, r, ray, from, first + Lw, slot0, staged, lane);
    }
    if (a.feat) slot_rows(a.F, a.app_pos, a.feat, (size_t)slot0, napp, lane);
}
// the rays the tile marcher could not stage (more than cap appearance samples): a small persistent grid walks the list
__global__ __launch_bounds__(256) void k_compact_list(const CompactArgs a, const unsigned* ovf_count, int* ovf_list) {
    const int lane = threadIdx.x & 63;
    const unsigned n = *ovf_count;
    for (unsigned k = blockIdx.x * 4u + (threadIdx.x >> 6); k < n; k += gridDim.x * 4u)
        compact_ray_staged(a, ovf_list[k], blockIdx.x & 7u, lane, ovf_list + k);
}

// z_vals rows (z_i of every sample index, models/tensorBase.py:313-318) and zeroed weights rows of a launch's rays: one wave per
// ray, 256-B coalesced stores (2 x 1.33 GB per C2 frame at the HBM write rate). The tile marcher then writes the weights of the
// sampled windows only.
__global__ __launch_bounds__(256) void k_dense_fill(const FieldDev F, const float* __restrict__ rays, long long n_rays, int ray_stride, int N,
                                                    float* __restrict__ w, float* __restrict__ z) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rays) return;
    Ray ray;
    if (z) ray = load_ray(F, rays + r * ray_stride, ray_stride);
    for (int i = lane; i < N; i += 64) {
        if (z) z[r * N + i] = sample_z<false>(F, ray, i, 0.f);
        if (w) w[r * N + i] = 0.f;
    }
}

// ---- the cached summed table of a whole grid ------------------------------------------------------------------------------------
// S[z][y][x] for 0 <= x <= grid[0], 0 <= y <= grid[1], 0 <= z <= grid[2] (one entry past the last texel per axis: the clamped texel
// again, what table_build puts into a slot beyond the grid — a cell at the grid's last texel reads it with weight 0), each entry by
// the marcher's own table_build<2> + table_sum<2> on a synthetic box origin: one wave per 4 x 4 x 4 box anchored at 4 b - shift per
// axis (cut at 0). An entry is three 16-term dot products on v_mfma_f32_16x16x4_f32 — every output element of the instruction runs the
// same four k-steps over the same operand values wherever it sits in the 16 x 16 block — and a fixed-order sum: its bits do not depend
// on the box it was computed in (tests/test_density_cache.py builds with every shift and compares).
struct SumTableArgs { FactorSet den; float* out; int n[3]; int nb[3]; int shift[3]; long long boxes; };
__global__ __launch_bounds__(256) void k_density_sum_table(const SumTableArgs a) {
    __shared__ __attribute__((aligned(16))) float smem[4 * kStageFloats];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long long box = (long long)blockIdx.x * 4 + wid;
    if (box >= a.boxes) return;
    float* __restrict__ stD = smem + (size_t)wid * kStageFloats;
    const int bx = (int)(box % a.nb[0]), by = (int)((box / a.nb[0]) % a.nb[1]), bz = (int)(box / ((long long)a.nb[0] * a.nb[1]));
    const int o[3] = {4 * bx - a.shift[0], 4 * by - a.shift[1], 4 * bz - a.shift[2]};
    const int amn[3] = {max(o[0], 0), max(o[1], 0), max(o[2], 0)};
    table_build<2>(a.den, amn, stD, lane & 15, lane >> 4);
    lds_fence_w();
    table_sum<2>(stD, lane);
    lds_fence_w();
    const int x = amn[0] + (lane & 3), y = amn[1] + ((lane >> 2) & 3), z = amn[2] + (lane >> 4);
    // the box's own cells (a box cut at 0 holds further cells of its neighbour: left to that one), inside the padded grid
    if (x < o[0] + 4 && y < o[1] + 4 && z < o[2] + 4 && x <= a.n[0] && y <= a.n[1] && z <= a.n[2])
        a.out[((size_t)z * (a.n[1] + 1) + y) * (a.n[0] + 1) + x] = stD[lane];
}

size_t density_cache_bytes(const t2n_field* f) {
    const int* g = f->desc.grid;
    return (size_t)(g[0] + 1) * (g[1] + 1) * (g[2] + 1) * sizeof(float);
}

int launch_density_sum_table(const t2n_field* f, float* out, const int shift[3], hipStream_t s) {
    SumTableArgs a;
    a.den = f->dev.den; a.out = out;
    a.boxes = 1;
    for (int k = 0; k < 3; ++k) {
        if (shift[k] < 0 || shift[k] > 3) { set_error("density sum table: shift[%d]=%d outside [0, 3]", k, shift[k]); return T2N_ERR_INVALID; }
        a.n[k] = f->desc.grid[k]; a.shift[k] = shift[k];
        a.nb[k] = (a.n[k] + shift[k]) / 4 + 1;    // boxes b with 4 b - shift <= n
        a.boxes *= a.nb[k];
    }
    hipLaunchKernelGGL(k_density_sum_table, dim3((unsigned)((a.boxes + 3) / 4)), dim3(256), 0, s, a);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

void density_cache_release(t2n_field* f) {
    if (f->dcache) { (void)hipDeviceSynchronize(); (void)hipFree(f->dcache); }
    f->dcache = nullptr; f->dcache_bytes = 0; f->dcache_version = 0; f->dcache_seen = 0; f->dcache_alloc_failed = false;
    f->dev.dsum = nullptr;
}

// Once per tile-marcher frame (t2n_render_forward), before its launches: f->dev.dsum = the cached table when it is current, else NULL.
// The table is built by the SECOND consecutive frame that finds the density factors unchanged (a loop that alternates optimiser steps
// and single frames never builds), on that frame's stream in front of its marcher; frames on other streams wait for the event behind
// the build. A rebuild overwrites the buffer in place: every frame that read the old table was queued before the factors changed, and
// whatever changed them was ordered behind those frames by the caller, as for the factor copies themselves.
int density_cache_prepare(t2n_field* f, hipStream_t s) {
    f->dev.dsum = nullptr;
    const bool second = f->dcache_seen == f->den_version;   // an earlier tile-marcher frame saw these factors (cached or not)
    f->dcache_seen = f->den_version;
    if (!f->dcache_on) return T2N_OK;
    const int* g = f->desc.grid;
    const size_t bytes = density_cache_bytes(f);
    size_t cap = f->dcache_cap;
    if (!cap) {
        static size_t dev_total = 0;
        if (!dev_total) { size_t fr = 0, tot = 0; if (hipMemGetInfo(&fr, &tot) == hipSuccess) dev_total = tot; else (void)hipGetLastError(); }
        cap = dev_total / 64;
    }
    // (cached_offset: 24-bit row counts and row bytes, 32-bit byte offsets)
    const bool addressable = (size_t)(g[1] + 1) * (g[2] + 1) < (1u << 24) && bytes < (1ull << 32);
    if ((size_t)g[0] * g[1] * g[2] * sizeof(float) > cap || !addressable) return T2N_OK;
    if (f->dcache && f->dcache_version == f->den_version) {
        if (f->dcache_stream != (void*)s) T2N_HIP(hipStreamWaitEvent(s, (hipEvent_t)f->dcache_ev, 0));
    } else {
        if (!second) return T2N_OK;   // first frame of this version
        if (!f->dcache) {
            if (f->dcache_alloc_failed) return T2N_OK;
            if (hipMalloc((void**)&f->dcache, bytes + 16) != hipSuccess) {   // no room: the frames stay uncached
                (void)hipGetLastError();
                f->dcache = nullptr; f->dcache_alloc_failed = true;
                return T2N_OK;
            }
            f->dcache_bytes = bytes + 16;
        }
        if (!f->dcache_ev) T2N_HIP(hipEventCreateWithFlags((hipEvent_t*)&f->dcache_ev, hipEventDisableTiming));
        const int shift[3] = {0, 0, 0};
        const int rc = launch_density_sum_table(f, f->dcache, shift, s);
        if (rc) return rc;
        T2N_HIP(hipEventRecord((hipEvent_t)f->dcache_ev, s));
        f->dcache_stream = (void*)s;
        f->dcache_version = f->den_version;
        ++f->dcache_counts[2];
    }
    f->dev.dsum = f->dcache;
    f->dev.ds_row = (unsigned)(g[0] + 1) * 4u;
    f->dev.ds_slice = f->dev.ds_row * (unsigned)(g[1] + 1);
    return T2N_OK;
}

int launch_march_tiles(t2n_field* f, const RenderLaunch& L, int img_w, int img_h, float* spill, float4* scratch, hipStream_t s) {
    const int cap = L.n_samples / 4 > 0 ? L.n_samples / 4 : 1;
    unsigned* ovf_count = (unsigned*)((char*)scratch + (size_t)L.n_rays * cap * 16);
    int* ovf_list = (int*)((char*)ovf_count + 256);
    const bool dense = L.weights != nullptr;
    TileArgs a;
    a.F = f->dev;
    a.rays = L.rays; a.n_rays = L.n_rays; a.ray_stride = L.ray_stride; a.n_samples = L.n_samples; a.img_w = img_w; a.img_h = img_h;
    a.acc = L.acc; a.depth = L.depth; a.ray_app = L.ray_app;
    a.wbuf = L.weights ? L.weights : spill;
    a.scratch = scratch; a.cap = cap; a.ovf_count = ovf_count; a.ovf_list = ovf_list;
    a.app_pos = L.app_pos; a.app_ray = L.app_ray; a.counters = L.counters; a.list_cap = L.list_cap; a.stats = (unsigned long long*)L.stats;
    a.dense_w = L.weights;
    // fused frame (t2n_render_forward decided: cached table, current feature volume, a row per list slot): rows in the marcher's tail
    // (not with an alpha mask: the masked instantiations already spill at five waves, and the tail adds to it)
    const bool rows = L.slot_rows && f->dev.dsum != nullptr && f->dev.avol != nullptr && !dense && !f->dev.alpha;
    if (L.slot_rows && !rows) { set_error("launch_march_tiles: a fused frame needs the cached table, the feature volume, no mask and no weights rows"); return T2N_ERR_STATE; }
    a.feat = rows ? L.feat : nullptr;
    ++f->fusion_counts[rows ? 0 : 1];
    // staged rows (t2n_field_set_row_staging): the box of a step pair is the box of its DENSITY taps, so it holds the entries' appearance
    // cells only where both factor sets have the same tap indices
    const FactorSet& fd = f->dev.den; const FactorSet& fa = f->dev.app;
    const bool stage = rows && f->row_staging_on && fd.W[0] == fa.W[0] && fd.H[0] == fa.H[0] && fd.H[1] == fa.H[1] &&
                       fa.W[0] < 1024 && fa.H[0] < 1024 && fa.H[1] < 1024 &&   // (the log packs the box origin into 10 bits per axis)
                       L.n_rays <= 0x7fffffffll;                               // (the staged kernel holds the ray index in an int)
    f->rows_counters = rows ? L.counters : nullptr; f->rows_stream = (void*)s;
    a.F.term_eps = (!L.weights && !L.z_vals && !L.sigma_ctx) ? f->term_eps : 0.f;   // (eval only: this marcher has no train form)
#ifdef MT_PROF
    static unsigned long long* prof = nullptr;
    static int prof_calls = 0;
    const long long prof_waves = ((long long)((img_w + 7) / 8) * ((img_h + 7) / 8) + 3) / 4 * 4;
    if (!prof) T2N_HIP(hipMalloc((void**)&prof, (size_t)65536 * 8 * 8));
    T2N_HIP(hipMemsetAsync(prof, 0, (size_t)65536 * 8 * 8, s));
    a.prof = prof_waves <= 65536 ? prof : nullptr;
#endif
    // (*ovf_count was zeroed by the launch's setup kernel, t2n_render_forward)
    const long long tiles = (long long)((img_w + 7) / 8) * ((img_h + 7) / 8);
    const dim3 grid((unsigned)((tiles + 3) / 4));
    timing_begin(f, T2N_K_MARCH, s);
    if (L.weights || L.z_vals)
        hipLaunchKernelGGL(k_dense_fill, dim3((unsigned)((L.n_rays + 3) / 4)), dim3(256), 0, s, f->dev, L.rays, (long long)L.n_rays, L.ray_stride,
                           L.n_samples, L.weights, L.z_vals);
    const bool cached = f->dev.dsum != nullptr;
    const size_t lds = stage ? (size_t)4 * kRsWaveBytes : (size_t)4 * ((cached ? 0 : kStageFloats) + (dense ? kDenseFloats : 0)) * sizeof(float);
    const bool mask = f->dev.alpha != nullptr, relu = f->dev.act == T2N_ACT_RELU;
    ++f->dcache_counts[cached ? 0 : 1];
#define T2N_MT_LAUNCH(D, A, R) do { if (stage) hipLaunchKernelGGL((k_march_tiles<D, A, R, true, !D && !A, !D && !A>), grid, dim3(256), lds, s, a); \
                                    else if (rows) hipLaunchKernelGGL((k_march_tiles<D, A, R, true, !D && !A>), grid, dim3(256), lds, s, a); \
                                    else if (cached) hipLaunchKernelGGL((k_march_tiles<D, A, R, true>), grid, dim3(256), lds, s, a); \
                                    else hipLaunchKernelGGL((k_march_tiles<D, A, R, false>), grid, dim3(256), lds, s, a); } while (0)
    if (dense) { if (mask) { if (relu) T2N_MT_LAUNCH(true, true, true); else T2N_MT_LAUNCH(true, true, false); }
                 else { if (relu) T2N_MT_LAUNCH(true, false, true); else T2N_MT_LAUNCH(true, false, false); } }
    else { if (mask) { if (relu) T2N_MT_LAUNCH(false, true, true); else T2N_MT_LAUNCH(false, true, false); }
           else { if (relu) T2N_MT_LAUNCH(false, false, true); else T2N_MT_LAUNCH(false, false, false); } }
#undef T2N_MT_LAUNCH
    T2N_HIP(hipGetLastError());
#ifdef MT_PROF
    if (a.prof && ++prof_calls == 20) {   // one report per process: per-wave cycle sums, averaged over the waves that ran steps
        static unsigned long long h[65536 * 8];
        T2N_HIP(hipStreamSynchronize(s));
        T2N_HIP(hipMemcpy(h, prof, sizeof(h), hipMemcpyDeviceToHost));
        double sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        long long n = 0;
        for (long long i = 0; i < prof_waves; ++i) if (h[i * 8 + 5]) { ++n; for (int k = 0; k < 8; ++k) sum[k] += (double)h[i * 8 + k]; }
        if (n) fprintf(stderr, "[mt prof] %lld waves, per wave: step pairs %.1f, cycles in the step loop %.0f = coordinates + validity %.0f, axis taps + union bit set %.0f, "
                               "table build (loads -> MFMA -> LDS) %.0f, table reads %.0f, activation + compositing + staging %.0f; per step pair %.0f\n",
                       n, sum[5] / n, (sum[0] + sum[1] + sum[2] + sum[3] + sum[4]) / n, sum[0] / n, sum[1] / n, sum[2] / n, sum[3] / n, sum[4] / n,
                       (sum[0] + sum[1] + sum[2] + sum[3] + sum[4]) / (sum[5] > 0 ? sum[5] : 1));
    }
#endif
    CompactArgs c;
    c.F = f->dev;
    c.rays = L.rays; c.n_rays = L.n_rays; c.ray_stride = L.ray_stride; c.n_samples = L.n_samples;
    c.wbuf = a.wbuf;
    c.ray_app = L.ray_app; c.app_pos = L.app_pos; c.app_ray = L.app_ray; c.counters = L.counters; c.list_cap = L.list_cap;
    c.stats = (unsigned long long*)L.stats;
    c.scratch = scratch; c.cap = cap;
    c.finisher = finish_supported(f) ? 1 : 0;
    c.feat = a.feat;
    hipLaunchKernelGGL(k_compact_list, dim3(64), dim3(256), 0, s, c, (const unsigned*)ovf_count, ovf_list);
    timing_end(f, T2N_K_MARCH, s);
    T2N_HIP(hipGetLastError());
    return launch_ray_stats(L, s);
}

}  // namespace t2n

