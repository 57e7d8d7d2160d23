// What the render backward (t2n_backward.hip: kernels, one launcher per stage, t2n_render_backward) shares with the fused training step
// (t2n_train.hip), which enqueues the same stages in another order: the workspace carve, the bin geometries, the device-side plan and
// the stage launchers. Everything more than these two files use lives in t2n_internal.h.
#pragma once
#include "t2n_internal.h"

namespace t2n {

struct GradSet { float* plane[3]; float* line[3]; };
// The same in device memory, for a backward that never reads the counters on the host (T2N_FLAG_DEVICE_ROWS): tile prefix and row
// count from the forward's counters (k_bwd_plan), clipped to the row CAPACITY the caller's buffers hold; overflow = the count
// exceeded it (the rows beyond take no part in this backward: the caller learns it from the forward's posted counters)
struct BwdPlan { TilePrefix tp; unsigned rows; unsigned overflow; };

// One wave: the forward's sub-list counters (clipped to list_cap) -> the tile prefix of `plan` (32 rows per tile), its row count clipped
// to rows_cap and its overflow flag (!stated: the caller's own precondition failed: no rows, overflow says so). Returns the rows the
// counters NEED; ovf is the flag, in every lane.
__device__ __forceinline__ unsigned plan_prefix(const unsigned* __restrict__ counters, unsigned list_cap, unsigned rows_cap, bool stated,
                                                BwdPlan* __restrict__ plan, unsigned& ovf) {
    const int lane = threadIdx.x;
    unsigned cnt, incl;
    const unsigned total = list_tiles(counters, list_cap, kLists, lane, cnt, incl);
    if (lane < kLists) plan->tp.t[lane] = incl - (cnt + 31u) / 32u;
    const unsigned rows = total * 32u;
    ovf = (!stated || rows > rows_cap) ? 1u : 0u;
    if (lane == 0) {
        plan->tp.t[kLists] = total;
        plan->overflow = ovf;
        plan->rows = !stated ? 0u : (rows < rows_cap ? rows : rows_cap);
    }
    return rows;
}

// ---- bins of the binned scatters (t2n_backward.hip): appearance = 16x16-texel plane tiles, density = 15^3-cell blocks -----------------
constexpr int kBinTile = 16;      // texels per tile edge (footprints reach one texel further: 17 staged)
constexpr int kBinCopies = 32;    // privatised histogram / cursor copies (every ray starts in the camera's tile)
constexpr int kBinSegApp = 512;   // smallest segment (sizes the segment list); the scan picks the actual size per call
constexpr int kBlk = 15;          // cells per block edge: taps reach one further, 16 per axis = the MFMA tile edge
constexpr unsigned kDenSeg = 16384;   // density records per segment (see k_bwd_den_block)
struct BinGeom { int tw[3], before[3], total; };
inline BinGeom bin_geom(const FactorSet& S) {
    BinGeom g;
    int t = 0;
    for (int k = 0; k < 3; ++k) {
        g.tw[k] = (S.W[k] + kBinTile) / kBinTile;              // cell + 1 in [0, W]
        g.before[k] = t;
        t += g.tw[k] * ((S.H[k] + kBinTile) / kBinTile);
    }
    g.total = t;
    return g;
}
// Density: 3-D blocks of kBlk^3 cells (k_bwd_den_block). The three density pairs share their axes (plane k spans two of them, line k the
// third), so ONE key per sample serves all six gradients. cell + 1 lies in [0, size]: (size + kBlk) / kBlk blocks per axis.
struct BlockGeom { int nb[3]; int size[3]; int total; int copies; };
inline BlockGeom block_geom(const FactorSet& S) {
    BlockGeom g;
    g.size[0] = S.W[0]; g.size[1] = S.H[0]; g.size[2] = S.H[1];
    for (int a = 0; a < 3; ++a) g.nb[a] = (g.size[a] + kBlk) / kBlk;
    g.total = g.nb[0] * g.nb[1] * g.nb[2];
    g.copies = kBinCopies;   // privatised histogram copies (every ray starts in the camera's block)
    return g;
}
// the density pairs really share their axes (TensorVMSplit: plane k = grid[mat1] x grid[mat0], line k = grid[vec])
inline bool block_geom_ok(const FactorSet& S) {
    return S.C == 16 && S.W[1] == S.W[0] && S.L[2] == S.W[0] && S.W[2] == S.H[0] && S.L[1] == S.H[0] && S.H[2] == S.H[1] && S.L[0] == S.H[1];
}

// Activation / gradient rows of the backward pass. Buffers whose lifetimes do not overlap (or that are rewritten
// element-in-place by the same thread) share storage: g1 over h1, g0 over h0, gx over xpe, gf over feat32, gX over x144.
struct BwdCarve { size_t x144, feat32, h0, h1, go, xpe, part, gpack, hist, bin_total, tile_start, nseg, segs, recs, a_hist, a_bin_total, a_tile_start, a_nseg, a_segs, a_recs, plan, total; unsigned seg_cap, a_seg_cap; };
inline size_t al256(size_t x) { return (x + 255) / 256 * 256; }
inline BwdCarve bwd_carve(int64_t rows, int64_t n_rays, int n_samples, int n_tiles, int n_blocks, int k0 = 351, bool rows_kept = false) {   // k0: inputs of MLP layer 0; n_blocks: density bins x copies; rows_kept: the activation rows live in the forward's workspace (fused step): none here
    BwdCarve c;
    size_t o = 0;
    const size_t R = (size_t)rows;
    const size_t RA = rows_kept ? 0 : R;
    c.x144 = o; o = al256(o + RA * 144 * 4);
    c.feat32 = o; o = al256(o + RA * 32 * 4);
    c.h0 = o; o = al256(o + RA * 128 * 4);
    c.h1 = o; o = al256(o + RA * 128 * 4);
    c.go = o; o = al256(o + R * 16);
    // (fused step: the encoding is never materialised — the rows hold G0 [128] | GF [32] | GX [144] only)
    c.xpe = o; o = al256(o + R * (size_t)(rows_kept ? 304 : ((k0 + 3) & ~3)) * 4);
    c.part = o; o = al256(o + tn_part_bytes(rows, k0));
    c.gpack = o; o = al256(o + (gemm_h_pack_bytes(k0) > mlp_bwd_ss_pack_bytes() ? gemm_h_pack_bytes(k0) : mlp_bwd_ss_pack_bytes()));   // packed W^T operands of the input-gradient GEMMs (t2n_gemm_h.hip / t2n_mlp_bwd_ss.hip)
    // block-binned density scatter: worst case one record per sample
    const size_t cap = (size_t)n_rays * (size_t)n_samples;
    c.seg_cap = (unsigned)(cap / kDenSeg + (size_t)n_blocks + 1);
    c.hist = o; o = al256(o + (size_t)n_blocks * 4);
    c.bin_total = o; o = al256(o + (size_t)n_blocks * 4);
    c.tile_start = o; o = al256(o + ((size_t)n_blocks + 1) * 4);
    c.nseg = o; o = al256(o + 4);
    c.segs = o; o = al256(o + (size_t)c.seg_cap * 16);
    c.recs = o; o = al256(o + cap * 16);
    // the same for the appearance samples (one record per activation row and plane)
    c.a_seg_cap = (unsigned)(3 * R / kBinSegApp + (size_t)n_tiles + 1);
    c.a_hist = o; o = al256(o + (size_t)n_tiles * kBinCopies * 4);
    c.a_bin_total = o; o = al256(o + (size_t)n_tiles * 4);
    c.a_tile_start = o; o = al256(o + ((size_t)n_tiles + 1) * 4);
    c.a_nseg = o; o = al256(o + 4);
    c.a_segs = o; o = al256(o + (size_t)c.a_seg_cap * 16);
    c.a_recs = o; o = al256(o + 3 * R * 16);
    c.plan = o; o = al256(o + sizeof(BwdPlan));
    c.total = o;
    return c;
}

// ---- the stages of a backward, one launcher each --------------------------------------------------------------------------------------
// What a driver knows about its call; filled once, every kernel argument struct is derived from it. The launchers enqueue on the stream
// they are given and never fork or join streams themselves.
struct BwdCall {
    t2n_field* f;
    const float* rays; int64_t n_rays; int ray_stride; int n_samples; const float* jitter; uint32_t flags;
    char* fw; Carve c;        // the forward's (KEEP_CTX) workspace
    char* bw; BwdCarve b;     // the backward's
    TilePrefix tp; const BwdPlan* plan;   // tile prefix from the host's read of the counters, or (plan != NULL) tile prefix and rows in device memory
    int64_t rows;             // appearance rows (with a plan: the capacity)
};
// the fused step's loss, evaluated by the per-ray pass instead of upstream gradients (BwdMarchArgs)
struct BwdLoss { const float* rgb; const float* depth; const float* rgb_t; const float* depth_t; float w_depth, w_trans, delta; float* part; };

// The binned scatters serve this call: grid lines within the LDS budget of the tile accumulate, density pairs on shared axes, record
// indices below 2^31, and T2N_BWD_ATOMIC_SCATTER (read once per process) not set.
bool binned_scatter_ok(const t2n_field* f, int64_t n_rays, int n_samples);
// Per-ray pass, k_bwd_march<TRAIN, bin, loss != NULL, count>. bin = false: the density gradients leave by global atomics; count = false
// (with a loss only): the block histogram was counted from the forward's windows (launch_app_count).
int launch_bwd_march(const BwdCall& k, bool bin, const float* d_rgb, const float* d_depth, const float* d_w, hipStream_t s,
                     const BwdLoss* loss = nullptr, bool count = true);
// Density scatter: the scan of the block histogram; then records + accumulate (all: a record per in-box sample, the early count's predicate)
int launch_den_scan(const BwdCall& k, hipStream_t s);
int launch_den_scatter(const BwdCall& k, bool all, hipStream_t s);
// Appearance binning: the count (with_density: the density block histogram in the same launch); then scan + records
int launch_app_count(const BwdCall& k, bool with_density, hipStream_t s);
int launch_app_records(const BwdCall& k, bool scan_one_launch, hipStream_t s);
// Appearance accumulate of gx [rows][144]. half_groups: 8 channels x 256 threads per workgroup (two workgroups per CU) where the LDS of
// that form fits 80 KiB, else as without: 16 channels x 512 threads
int launch_app_accum(const BwdCall& k, const float* gx, bool half_groups, hipStream_t s);

// The field's two side streams (the process-wide pair; streams = false: none needed) and ALL of its events: ev_fork / ev_join,
// ev_fork2 / ev_join2, ev_pack, ev_den, train_ev[]. Lazy: called by the drivers, a field that never runs a backward creates nothing.
int ensure_side_streams(t2n_field* f, bool streams = true);
// `to` goes on behind what `from` holds now
inline int fork_stream(hipStream_t from, hipStream_t to, void* ev) {
    T2N_HIP(hipEventRecord((hipEvent_t)ev, from));
    T2N_HIP(hipStreamWaitEvent(to, (hipEvent_t)ev, 0));
    return T2N_OK;
}

}  // namespace t2n
