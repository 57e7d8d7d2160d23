/*
 * t2n.h — C-ABI of libt2n_hip.so: the MI355X (gfx950) TensoRF VM-split ray-marching renderer that replaces the
 * PyTorch op sequence behind Text2NeRF's  OctreeRender_trilinear_fast(rays, tensorf, ...)  /  TensorVMSplit.forward.
 *
 * The reference has no native code on this path (it is ~30 eager ATen ops per chunk), so there is no foreign-function
 * interface to mirror; each entry point below cites the reference Python it replaces (paths relative to the reference
 * repository). INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - plain C: pointers + sizes only; every pointer is a DEVICE pointer owned by the caller unless marked "host".
 *   - every call returns 0 on success or a negative T2N_ERR_* code; t2n_last_error() gives a thread-local message.
 *     Nothing throws across the boundary. Unsupported configurations are rejected loudly (T2N_ERR_UNSUPPORTED): there is
 *     no CPU fallback in this library.
 *   - work is enqueued on the caller's HIP stream (pass torch.cuda.current_stream().cuda_stream); calls do not
 *     synchronise unless documented. The library allocates device memory only inside t2n_field_create/_upload (the
 *     channel-last copy of the factor tensors) and, once, in the first t2n_train_step of a field (its training state: a few hundred
 *     KB); per-call scratch comes from the caller's workspace.
 *   - a handle may be used from one host thread at a time. This includes the `const t2n_field*` queries t2n_render_workspace_bytes_hint
 *     and t2n_field_list_retries: they consume the counters that budgeted launches posted (and the latter waits for those still in
 *     flight), i.e. they update the field's hint state.
 */
#ifndef T2N_H_
#define T2N_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct t2n_field t2n_field;      /* opaque */
typedef void* t2n_stream;                /* hipStream_t */

enum {
    T2N_OK = 0,
    T2N_ERR_INVALID = -1,      /* bad argument */
    T2N_ERR_UNSUPPORTED = -2,  /* configuration the HIP path does not implement */
    T2N_ERR_HIP = -3,          /* a HIP runtime call failed */
    T2N_ERR_WORKSPACE = -4,    /* caller workspace too small */
    T2N_ERR_STATE = -5         /* e.g. render before upload, backward without a kept context */
};

/* shading heads: models/tensorBase.py:200-216 */
enum { T2N_SHADE_MLP_FEA_NOVIEW = 0, T2N_SHADE_SH = 1, T2N_SHADE_RGB = 2,
       /* view-dependent heads (models/tensorBase.py:62-86,111-159): general unfused path, csrc/t2n_heads.hip */
       T2N_SHADE_MLP_FEA = 3, T2N_SHADE_MLP_PE = 4, T2N_SHADE_MLP = 5 };
/* fea2denseAct: models/tensorBase.py:406-410 */
enum { T2N_ACT_SOFTPLUS = 0, T2N_ACT_RELU = 1 };

/* render flags */
enum {
    T2N_FLAG_TRAIN = 1u,      /* is_train: per-ray jitter, no z gate (models/tensorBase.py:314-316,459) */
    T2N_FLAG_ADD_BG = 2u,     /* rgb_map += 1-acc  (white_bg, or the train-time coin; models/tensorBase.py:497-498) */
    T2N_FLAG_KEEP_CTX = 4u,   /* keep the per-call context in the workspace for t2n_render_backward */
    T2N_FLAG_NDC = 16u,       /* ndc_ray=True (models/tensorBase.py:293-302,441-446): the sample depths are a table shared by all
                               * rays — pass it through the `jitter` argument: [n_samples] floats = torch.linspace(near, far, N)
                               * (+ the shared train-time jitter, already added); dists are scaled by |d| and the SH head sees
                               * normalised view directions. Not used by the Text2NeRF driver (ndc_ray=0). */
    T2N_FLAG_DEVICE_ROWS = 32u, /* t2n_render_backward only: read NO count on the host. The appearance row capacity is what the two
                               * workspaces hold (the forward's kept activation rows; the backward's row buffers); the actual row count
                               * and tile prefix are derived on the device and every row kernel clips to them. Rows past the capacity
                               * lose their appearance gradient (t2n_field_device_rows_record tells the caller afterwards). ONE backward per
                               * forward in this mode: the kept rows are consumed in place, a second call on the same context finds the
                               * forward's statement cleared and computes no appearance gradients. Needs the fused
                               * MLP_Fea_noview head (27/6/128, 48 comps), the binned scatters and all head gradient tensors. */
    T2N_FLAG_PIPELINE = 64u,  /* t2n_train_step only: the pipelined form is allowed (the caller has not touched the field since its previous
                               * t2n_train_step) */
    T2N_FLAG_GATHER_BATCH = 128u, /* t2n_train_step only: the batch is gathered from the field's training source by row index
                               * (t2n_field_set_train_source): rays / rgb_target / depth_target of the call are DESTINATIONS */
    T2N_FLAG_REG_L1 = 256u,    /* t2n_train_step only: hyper[21] / hyper[22] hold this step's L1 weights (density planes / density lines) */
    T2N_FLAG_REG_ORTHO = 512u, /* t2n_train_step only: hyper[23] / hyper[24] hold this step's ortho weights (density / appearance lines); the
                               * call then issues the two ortho launches behind its seed */
    T2N_FLAG_COHERENT = 8u    /* hint (eval): rays are a row-major image whose width was given by t2n_field_set_frame_width:
                                 march 8x8-pixel tiles whose rays share one texel x line-row dot-product table per step
                                 (f32 matrix cores). Same samples; the density feature is summed in table order and the
                                 transmittance is a sequential product instead of a wave scan (weights agree to ~2e-6) */
};

/* Scalars of TensorBase.__init__/update_stepSize (models/tensorBase.py:163-231), computed by the host mirror. */
typedef struct t2n_field_desc {
    float aabb_min[3], aabb_max[3];
    float inv_aabb_size[3];        /* 2/(aabb_max-aabb_min), fp32 as the reference computes it (:224) */
    int32_t grid[3];               /* gridSize (x,y,z) */
    int32_t density_n_comp;        /* per plane; the three planes must agree */
    int32_t app_n_comp;
    int32_t app_dim;               /* 27 (MLP/SH heads) or 3 (RGB head) */
    int32_t shading;               /* T2N_SHADE_* */
    int32_t fea_pe;                /* 6 */
    int32_t feature_c;             /* 128 */
    int32_t act;                   /* T2N_ACT_* */
    float density_shift;           /* -10 */
    float distance_scale;          /* 25 */
    float weight_thres;            /* rayMarch_weight_thres 1e-4 */
    float step_size;               /* stepSize */
    float near, far;               /* near_far */
    float z_gate;                  /* 2.0: the eval-only world-z gate (models/tensorBase.py:459-462) */
    int32_t view_pe, pos_pe;       /* octaves of the view-direction / position encodings of the MLP_Fea, MLP_PE, MLP heads */
} t2n_field_desc;

/* Reference-layout parameter pointers (device, fp32), i.e. the tensors of TensorVMSplit.state_dict()
 * (models/tensoRF.py:144-160): plane k is [1,C,grid[matMode[k][1]],grid[matMode[k][0]]], line k is [1,C,grid[vecMode[k]],1],
 * basis_mat.weight [app_dim, 3*app_n_comp], renderModule.mlp.{0,2,4}.{weight,bias} (NULL for SH / RGB heads). */
typedef struct t2n_field_params {
    const float* density_plane[3];
    const float* density_line[3];
    const float* app_plane[3];
    const float* app_line[3];
    const float* basis_weight;
    const float* mlp_w0; const float* mlp_b0;
    const float* mlp_w1; const float* mlp_b1;
    const float* mlp_w2; const float* mlp_b2;
} t2n_field_params;

/* Gradient buffers in the SAME reference layouts (device, fp32, caller-zeroed or accumulated into). */
typedef struct t2n_field_grads {
    float* density_plane[3];
    float* density_line[3];
    float* app_plane[3];
    float* app_line[3];
    float* basis_weight;
    float* mlp_w0; float* mlp_b0;
    float* mlp_w1; float* mlp_b1;
    float* mlp_w2; float* mlp_b2;
} t2n_field_grads;

/* Per-call counters written by the render kernels (device memory, 8 x uint64): the units of the roofline model. */
enum { T2N_STAT_EVALUATED = 0,   /* V: in-box (and z-gated) samples that read the density factors */
       T2N_STAT_APPEARANCE = 1,  /* A: samples with weight > weight_thres that read the appearance factors */
       T2N_STAT_RAYS = 2,
       T2N_STAT_OVERFLOW = 3,    /* must stay 0 */
       T2N_STAT_F16_REDO = 4,    /* sub-launches whose split-f16 appearance stage met a value outside the f16 range and were
                                    redone on the exact fp32 path (results are the exact path's) */
       T2N_STAT_LIST_RETRY = 5,  /* 1: some rays of the call found no room in its budgeted appearance lists and were shaded and
                                    composited by the per-ray finisher (k_finish_rays: exact-fp32 head, no list memory). (The general
                                    view-dependent heads always render with worst-case lists.) */
       T2N_STAT_COUNT = 8 };

const char* t2n_last_error(void);
int t2n_version(void);

/* ---- field lifetime: replaces TensorVMSplit.__init__ containers + the implicit "weights are where ATen reads them" */
int t2n_field_create(const t2n_field_desc* desc, t2n_field** out);
int t2n_field_destroy(t2n_field* f);
/* Re-read the reference-layout parameters into the internal channel-last / MFMA-packed device copy. Call after
 * construction, after load_state_dict, and after every optimiser step. Asynchronous on `stream`. */
int t2n_field_upload(t2n_field* f, const t2n_field_params* p, t2n_stream stream);
/* Update scalars only (step size, near/far, ...): TensorBase.update_stepSize (models/tensorBase.py:220-231). */
int t2n_field_set_desc(t2n_field* f, const t2n_field_desc* desc);
/* Factor storage for the forward render: 0 = fp32 (default), 1 = bf16 (BASELINE.json configs[4]). In bf16 mode
 * t2n_field_upload rounds the 12 plane / line tensors to bf16 (nearest-even) and keeps two device copies: 2-byte texels for
 * the march / shade gathers (half the bytes through L1) and the rounded values as fp32 for every other entry point, so a
 * render equals the fp32 render of the bf16-rounded tensors BIT FOR BIT; gradients are taken at the rounded values and
 * returned in fp32 for the caller's fp32 master copy. basis_mat / MLP stay fp32. Call before t2n_field_upload. */
int t2n_field_set_factor_storage(t2n_field* f, int bf16);

/* Arithmetic of the basis/MLP contractions (nn.Linear in the reference, models/tensoRF.py:239, tensorBase.py:94-106):
 * exact_fp32 = 0 (default): every fp32 product as three f16 MFMA products of hi/lo splits (22-bit mantissa), fp32
 * accumulation; exact_fp32 = 1: v_mfma_f32_32x32x2_f32, bit-exact fp32 FMA chains (5x the matrix-core time). The backward
 * pass always recomputes activations with the exact path. */
int t2n_field_set_mlp_precision(t2n_field* f, int exact_fp32);
/* a-7 (optional): AlphaGridMask (models/tensorBase.py:41-59). volume = device fp32 [D(z),H(y),W(x)] occupancy (copied);
 * aabb_min / inv_size (= 1/aabbSize*2, fp32 as the reference computes it) are HOST float[3]. Samples whose trilinear
 * mask value is not > 0 are dropped from ray_valid (:451-456). volume = NULL removes the mask. The tile marcher is
 * bypassed while a mask is set. t2n_alpha_at = AlphaGridMask.sample_alpha at world points. */
int t2n_field_set_alpha_mask(t2n_field* f, const float* volume, int D, int H, int W, const float* aabb_min_host,
                             const float* inv_size_host, t2n_stream stream);
int t2n_alpha_at(const t2n_field* f, const float* xyz_world, int64_t n, float* alpha, t2n_stream stream);
/* Early ray termination for EVAL launches that materialise neither weights nor z_vals (and keep no backward context): once a ray's
 * transmittance T fell below eps it evaluates no further sample — per 8x8-pixel tile in the tile marcher (the wave leaves its step
 * loop when all 64 rays are done), per 64-sample block in the per-ray marcher. The reference has no such mode: it evaluates every
 * in-box sample whatever T is (models/tensorBase.py:19-26 raw2alpha, :494-505 compositing), so this is a bounded deviation, not
 * parity: what the skipped samples could add is < eps to acc, < eps to each colour channel, < eps * (z_max - d_z) to depth; the
 * evaluated-sample count (T2N_STAT_EVALUATED) becomes a lower bound of the reference's. eps in [0, weight_thres]; 0 (default of a new
 * handle) = off = the reference's arithmetic sample for sample. Train launches, launches with weights / z_vals outputs and
 * T2N_FLAG_KEEP_CTX launches ignore it. */
int t2n_field_set_early_termination(t2n_field* f, float eps);
/* Feature stage of the default render path (k_app_features_p, fp32 factor storage): on = 1 (default of a new handle): per 32-entry
 * tile and plane / line pair the wave copies the bounding box of the entries' taps into LDS and reads the taps there, where the box
 * fits (texels of the plane box + taps of the line span <= 64 slots); a pair that does not fit is gathered tap by tap. on = 0:
 * every pair is gathered; bf16 factor storage is always gathered. The feature rows are the same bit for bit either way.
 * t2n_field_feature_staging_counts: the (tile, pair) units that ran staged (out[0]) and gathered (out[1]) since the field was
 * created. A diagnostic: it waits for the whole device (hipDeviceSynchronize), so it must not be called inside a stream capture. */
int t2n_field_set_feature_staging(t2n_field* f, int on);
int t2n_field_feature_staging_counts(const t2n_field* f, uint64_t out[2]);
/* Cached summed density table of the tile marcher (T2N_FLAG_COHERENT eval frames). The marcher's per-step-pair table
 * S[z][y][x] = (D0 + D1) + D2, D_k = P_k L_k^T, is a function of the density factors alone; with the cache on (default of a new
 * handle) the second consecutive tile-marcher frame that finds the factors unchanged builds S for the whole grid once
 * ((grid + 1)^3 floats in a buffer the field owns, built on that frame's stream), and frames read their entries there until the
 * factors change (t2n_field_upload, the field Adam steps, t2n_train_step, a t2n_field_factor_buffer view). Frames are the same bit
 * for bit with and without it. Not cached: grids whose cells x 4 B exceed the cap (t2n_field_set_density_cache_cap; 0 = the default,
 * 1/64 of the device's memory), a failed allocation, cache switched off.
 * t2n_field_release_density_cache frees the buffer (waits for the device); the next two frames build it again.
 * t2n_field_density_cache_counts: out[0] / out[1] = tile-marcher launches served from the cache / without it, out[2] = builds,
 * out[3] = bytes the buffer holds now (host-side counters: no device wait).
 * DIAGNOSTIC t2n_field_density_sum_table: the builder alone — S of the whole grid into `out` ((grid[0] + 1) (grid[1] + 1) (grid[2] + 1)
 * floats, x fastest), computed in 4 x 4 x 4 boxes anchored at 4 b - shift[axis] (shift in [0, 3]): every shift gives the same bits. */
int t2n_field_set_density_cache(t2n_field* f, int on);
int t2n_field_set_density_cache_cap(t2n_field* f, uint64_t bytes);
int t2n_field_release_density_cache(t2n_field* f);
int t2n_field_density_cache_counts(const t2n_field* f, uint64_t out[4]);
int t2n_field_density_sum_table(const t2n_field* f, const int* shift, float* out, t2n_stream stream);
/* Cached appearance feature volume of the tile-marcher frames (T2N_FLAG_COHERENT eval frames, fused MLP_Fea_noview head on split
 * products). The 27 appearance features of a sample are the trilinear interpolation of a per-corner volume
 * F_j(corner) = sum_k sum_c basis_mat[j, 48 k + c] P_k[corner][c] L_k[corner][c], a function of the appearance factors and basis_mat
 * alone. With the volume on (default of a new handle) the min_frames-th CONSECUTIVE tile-marcher frame that finds those tensors
 * unchanged builds F for the whole grid ((grid + 1)^3 corners x 32 floats in a buffer the field owns, on that frame's stream), and the
 * feature stage of the frames after it reads eight corners per sample there until the tensors change (t2n_field_upload[_head], the field
 * Adam steps, t2n_train_step and its graph replay, a t2n_field_factor_buffer view of an appearance tensor). Frames of one version before
 * and after the build differ by rounding only (the interpolation's eight extra multiply-adds per feature); depth, acc, lists and counters
 * are the same bits. The training forward, explicit points and per-ray-marcher launches always run the direct form, as do tiles past
 * the feature-row capacity; the rays the budgeted lists leave to the finisher read the volume like the rest of their frame.
 * Where a frame can hold rows of both forms (they differ by rounding, ~1e-7 in rgb): (a) a volume frame with more appearance tiles than
 * its feature rows hold (32 rows per ray + 1024 with worst-case lists; budgeted lists hold a row per list slot and have none) — the
 * surplus tiles take the one-kernel direct path, so a budgeted and a worst-case volume frame of such a scene need not be equal bit for
 * bit; (b) an image that the caller splits over several t2n_render_forward calls: every call counts as a frame, and the min_frames-th
 * call may fall inside the image. Callers that need bit-stable frames switch the volume off or set min_frames = 1.
 * Footprint: the buffer (3.49 GB at 300^3) is a device allocation of the field outside any caller's allocator; it stays allocated,
 * unread, while the tensors change (training steps between evaluations) and is rebuilt in place by the next run of min_frames frames;
 * t2n_field_release_appearance_volume gives it back.
 * min_frames = 0 restores the default
 * (T2N_APP_VOLUME_MIN_FRAMES = build time / per-frame saving, measured at C2); a loop that alternates optimiser steps and single frames
 * never builds. Not built: grids whose cells x 128 B exceed the cap (t2n_field_set_appearance_volume_cap; 0 = the default, 1/64 of the
 * device's memory) or leave 32-bit byte offsets, a failed allocation, volume switched off, other heads.
 * t2n_field_release_appearance_volume frees the buffer (waits for the device).
 * t2n_field_appearance_volume_counts: out[0] = bytes the buffer holds now, out[1] = builds, out[2] / out[3] = tile-marcher frames that
 * read the volume / ran the direct form (host-side counters: no device wait). */
#define T2N_APP_VOLUME_MIN_FRAMES 33   /* 4.9 ms build / 0.149 ms saved per C2 frame (profiles/appearance_volume_ab.txt) */
int t2n_field_set_appearance_volume(t2n_field* f, int on, int min_frames);
int t2n_field_set_appearance_volume_cap(t2n_field* f, uint64_t bytes);
int t2n_field_release_appearance_volume(t2n_field* f);
int t2n_field_appearance_volume_counts(const t2n_field* f, uint64_t out[4]);
/* Feature rows in the tile marcher's tail. A tile-marcher launch that reads the cached density table, holds the current feature volume
 * and whose workspace carve holds ONE FEATURE ROW PER LIST SLOT writes the rows in the marcher itself — every wave produces the rows of the
 * list slots it fills or voids, k_compact_list those of the rays handed to it — and runs no feature kernel; the head reads the rows by
 * slot. The rows are the bits the feature kernel computes from the same entries, so a fused frame equals the unfused frame of the same
 * field and volume bit for bit. A row per slot: budgeted lists always (the feature rows of a budgeted carve are sized that way: at the
 * ~14 entries per ray a C2 frame settles on 1.15 GB of rows instead of the 0.6 GB of half a row per slot), worst-case lists only where
 * 8 x list_cap <= 32 rows per ray + 1024 (small launches); a C2 frame's worst-case lists (42 GB of rows) stay unfused, as do launches
 * that materialise weights, uncached frames, frames without a current volume and fields with an alpha mask (the masked marcher spills
 * in its step loop once the tail is added). Default of a new handle: on.
 * t2n_field_feature_fusion_counts: out[0] / out[1] = tile-marcher launches (sub-launches of a split call count one each) with the rows
 * in the marcher's tail / with the feature stage (host-side counters: no device wait).
 * t2n_render_list_shape: the carve of one launch of n_rays x n_samples with `entries_per_ray` budgeted lists (0 = worst case): out[0] =
 * list_cap (slots per sub-list), out[1] = feature rows, out[2] = 1 when the rows hold a row per slot (the launch can be fused), out[3] /
 * out[4] / out[5] = byte offsets of the entry list, the feature rows and the counter block in the workspace (tests read a launch's
 * lists and rows there). */
int t2n_field_set_feature_fusion(t2n_field* f, int on);
int t2n_field_feature_fusion_counts(const t2n_field* f, uint64_t out[2]);
int t2n_render_list_shape(int64_t n_rays, int n_samples, int entries_per_ray, uint64_t out[6]);
/* Staged rows of a fused launch. The 64 rays of a tile are less than a voxel apart, so the entries a step pair emits lie in the <= 4 x 4 x 4
 * corner box whose density taps the pair read. With staging on, a wave logs its emitting step pairs (box origin, who emitted) in LDS while
 * it marches; its tail then walks the entries in emission order, copies each logged pair's corner box from the feature volume to LDS once
 * and reads every row's eight corners there instead of fetching 8 x 128 B per entry. Slots, entries and rows are the direct tail's, bit for
 * bit. A wave runs the direct tail when it emitted on a step pair whose taps do not fit one box, logged more than 32 pairs or its list region did
 * not fit; rays handed to k_compact_list and voided regions keep the direct rows. A launch is staged only when the appearance and density
 * factor sets have the same grid (the box is the box of the density taps) of fewer than 1024 texels per axis. Default of a new handle: on.
 * t2n_field_row_staging_counts: out[0] / out[1] = waves of the handle's LAST fused tile-marcher launch whose tail wrote its rows from LDS
 * boxes / in the direct form (both 0 when that launch was not staged: off, unequal grids, unfused). The waves count themselves on the device
 * in words 50 / 51 of each sub-list's line of the launch's counter block; the call waits for that launch's stream and reads the block, so
 * the workspace of that launch must still be allocated. */
int t2n_field_set_row_staging(t2n_field* f, int on);
int t2n_field_row_staging_counts(const t2n_field* f, uint64_t out[2]);
/* DIAGNOSTIC, for tests of the feature stage: the stage alone on caller-made appearance lists. app_pos: device [8][list_cap] entries
 * (x, y, z normalised to [-1, 1], compositing weight); counters: device block of 8 x 64 words, word 64 l = entries of sub-list l (word 32
 * is the stage's f16-range flag: zero it); feat: device [feat_rows][32] rows, row 32 t + s = entry s of tile t, tiles numbered through
 * the sub-lists in order (a sub-list's last tile is padded with zero-weight rows); feat_rows a multiple of 32 that covers the tiles.
 * volume = 0: the direct form; 1: the rows from the cached feature volume, built here if it is not current. */
int t2n_field_feature_rows(t2n_field* f, const float* app_pos, const uint32_t* counters, uint32_t list_cap, int volume, float* feat,
                           uint32_t feat_rows, t2n_stream stream);
/* DIAGNOSTIC, for tests of the appearance head: the sample-stationary head (k_mlp_ss3) alone on caller-made feature rows — no feature
 * stage, no one-kernel tail, no exact redo. feat: device [feat_rows][32] fp32 rows, columns 0..26 the features, column 27 the entry's
 * compositing weight, the rest unused. counters: device block of 8 x 64 words, word 64 l = entries of sub-list l (clamped to list_cap);
 * word 32 is the head's f16-range flag: the caller zeroes it and reads it back. slot_rows = 0: row 32 t + s = entry s of tile t, tiles
 * numbered through the sub-lists in order (feat_rows must cover min(tiles, tile_hi) x 32 rows: a partial tile's dead rows are read);
 * slot_rows = 1: row = list slot l * list_cap + entry (feat_rows >= 8 list_cap; dead slots are never read). Tiles from tile_hi on are
 * left alone. app_rgb: device [8 list_cap] float4 by list slot (r, g, b, the row's weight); slots without a live entry are not written.
 * variant_out (host): the word the weight packer wrote, 1 = the untracked instantiation ran, 0 = the tracked one. Waits for the stream.
 * Other heads and the exact-fp32 mode: T2N_ERR_UNSUPPORTED; sizes that do not cover the launch: T2N_ERR_INVALID. */
int t2n_field_head_rows(t2n_field* f, const float* feat, uint32_t feat_rows, uint32_t* counters, uint32_t list_cap, uint32_t tile_hi,
                        int slot_rows, float* app_rgb, uint32_t* variant_out, t2n_stream stream);
/* DIAGNOSTIC, for tests of the feature stage's tile queue only (like the staging counters above, not part of the rendering API): the
 * shape of the feature stage's launch. At most `workgroups` workgroups of eight waves (0 = the default, 512), and `defer_cap` tiles
 * (1 .. 64; 0 = the default, 16) that a wave sets aside for its gathered loop before it drains them. Small values make one wave see
 * many tiles and drain a full queue on a small frame. Neither value changes a feature row; no caller needs them to render. */
int t2n_field_set_feature_stage_shape(t2n_field* f, int workgroups, int defer_cap);
/* Image width of the row-major frames passed with T2N_FLAG_COHERENT (0 = unknown: the flag is ignored). */
int t2n_field_set_frame_width(t2n_field* f, int width);

/* ---- a-1/a-2: get_ray_directions (dataLoader/ray_utils.py:24-42), normalisation (dataLoader/scene_gen.py:45),
 *      get_rays (dataLoader/ray_utils.py:66-87) */
int t2n_ray_directions(int H, int W, float fx, float fy, float cx, float cy, int normalize, float* dirs /*[H*W,3]*/,
                       t2n_stream stream);
int t2n_get_rays(const float* dirs /*[n,3]*/, int64_t n, const float* c2w_host /*[3 rows x 4] row-major, host*/,
                 float* rays_o /*[n,3] or NULL*/, float* rays_d /*[n,3] or NULL*/, float* rays6 /*[n,6] or NULL*/,
                 t2n_stream stream);
/* fused: pixel -> [H*W,6] ray rows (ox,oy,oz,dx,dy,dz), SceneGen recipe (scene_gen.py:44-45,92-94) */
int t2n_generate_rays(int H, int W, float fx, float fy, float cx, float cy, const float* c2w_host, float* rays6,
                      t2n_stream stream);

/* ---- a-5 as a stage of its own: TensorBase.sample_ray (models/tensorBase.py:304-323; ndc = 0) and sample_ray_ndc (:293-302; ndc = 1).
 * rays_o / rays_d [n,3] -> pts [n,N,3] = o + d z, valid [n,N] = 1 inside the box (the complement of mask_outbbox; no z gate: forward
 * applies that one itself, :459-462). ndc = 0: z_i = t_min + step (i [+ jitter[ray]]) goes to z_vals [n,N]; jitter = the per-ray
 * U[0,1) draws of train mode or NULL. ndc = 1: `jitter` is the caller's table of the N depths shared by all rays (linspace(near, far, N)
 * [+ its jitter row]); z_vals is not written (the reference returns the [1,N] table itself). */
int t2n_sample_ray(const t2n_field* f, const float* rays_o, const float* rays_d, int64_t n, int n_samples, const float* jitter, int ndc,
                   float* pts /*[n,N,3]*/, float* z_vals /*[n,N] or NULL*/, uint8_t* valid /*[n,N]*/, t2n_stream stream);

/* ---- a-16: TensorBase.filtering_rays(bbox_only=True) slab test (models/tensorBase.py:385-391) */
int t2n_filter_rays_bbox(const t2n_field* f, const float* rays, int64_t n_rays, int ray_stride, uint8_t* mask,
                         t2n_stream stream);

/* ---- stage entry points (mirrors of TensorVMSplit methods, used by the Python mirror and the stage parity tests)
 * a-9 + a-10: compute_densityfeature (models/tensoRF.py:205-220) [+ feature2density (tensorBase.py:406-410)].
 *   xyz_norm [n,3] normalised to [-1,1]; feat/sigma [n] (either may be NULL). */
int t2n_density_at(const t2n_field* f, const float* xyz_norm, int64_t n, float* feat, float* sigma, t2n_stream stream);
/* a-12 + a-13: compute_appfeature (models/tensoRF.py:223-239) and renderModule (models/tensorBase.py:29-33,88-109).
 *   viewdirs [n,3] (SH head only, else NULL); app_feat [n,app_dim] and rgb [n,3] (either may be NULL).
 *   workspace: t2n_shade_workspace_bytes(n) bytes of device memory (holds the launch's f16-range flag; T2N_ERR_INVALID when
 *   missing on a field whose head runs as split-f16 products). */
size_t t2n_shade_workspace_bytes(int64_t n);
int t2n_shade_at(const t2n_field* f, const float* xyz_norm, const float* viewdirs, int64_t n, float* app_feat, float* rgb,
                 void* workspace, size_t workspace_bytes, t2n_stream stream);
/* a-11: raw2alpha (models/tensorBase.py:19-26): sigma,dist [R,N] -> alpha, weights [R,N], bg [R] (any output NULL). */
int t2n_raw2alpha(const float* sigma, const float* dist, int64_t n_rays, int n_samples, float* alpha, float* weights,
                  float* bg, t2n_stream stream);

/* ---- geometry outputs of a view (csrc/t2n_geometry.hip; not in the reference, which returns the expected depth only).
 * Density-feature gradient: f(p) = compute_densityfeature at world point p; grad f is its exact gradient under the kernels' own
 *   trilinear arithmetic: on axis a the difference of the two taps axis_taps selects (clamped indices, so 0 on the exact upper face;
 *   the cell is the one the float32 coordinate falls into: floor, one-sided at a cell face) times inv_aabb_size[a] (grid[a] - 1) / 2.
 *   softplus' > 0 and relu' >= 0, so -grad f / |grad f| is the direction of steepest density decrease: no activation derivative is
 *   needed for a unit normal. xyz_norm [n,3] normalised like t2n_density_at's; feat [n] is that call's feature bit for bit;
 *   grad_world [n,3] is in world units. Either output may be NULL.
 * Per ray, for EVAL sampling: the z values, box mask, world-z gate, AlphaGridMask test and last-interval-0 rule of the render call
 *   without T2N_FLAG_TRAIN; early termination is ignored (a ray is always marched to its end). With w_i, z_i as in raw2alpha
 *   (models/tensorBase.py:19-26,448,475):
 *     acc          = sum_i w_i, and depth = the render call's depth_map, with its (1 - acc) rays[..., -1] term
 *     depth_var    = sum_i w_i (z_i - depth)^2: compute_depth_loss's pred_var (utils.py:306-320) without its + 1e-8; float64 moments
 *                    about the first valid sample's depth, rounded once
 *     depth_median = z_k + dist_k (quantile - C_{k-1}) / w_k, with C_i = sum_{j <= i} w_j, k the first sample with C_k >= quantile
 *                    and dist_k the UNSCALED interval z_{k+1} - z_k: w_k is taken as spread over the interval that produced it, so
 *                    the value is continuous and monotone in the quantile. Rays whose cumulative weight never reaches the quantile
 *                    get miss_depth.
 *     normal       = sum_i w_i n_i, n_i = -grad f(p_i) / max(|grad f(p_i)|, FLT_MIN): world space, NOT normalised (length <= acc;
 *                    exactly 0 for a ray without weight)
 *   Every output [n_rays] (normal [n_rays,3]) may be NULL. No workspace, no atomics, no host read; two calls give the same bits and a
 *   ray's outputs depend neither on n_rays nor on its place in the batch. bf16 factor storage and alpha masks are supported.
 *   quantile outside (0,1): T2N_ERR_INVALID. NDC sampling is a flag of one render call (T2N_FLAG_NDC), not a property of the field,
 *   and this entry point takes no flags: it has no NDC form (a normal in NDC space means nothing); the Python mirror refuses
 *   ndc_ray=True, and general-shape fields, which have no native handle. */
int t2n_density_grad_at(const t2n_field* f, const float* xyz_norm, int64_t n, float* feat, float* grad_world /*[n,3]*/,
                        t2n_stream stream);
int t2n_render_geometry(const t2n_field* f, const float* rays, int64_t n_rays, int ray_stride, int n_samples, float quantile,
                        float miss_depth, float* acc, float* depth, float* depth_median, float* depth_var,
                        float* normal /*[n_rays,3]*/, t2n_stream stream);

/* ---- a-3/a-4: the render call. Replaces the chunk loop of OctreeRender_trilinear_fast (renderer.py:28-42) and
 * TensorBase.forward (models/tensorBase.py:436-507) for ndc_ray=False, alphaMask=None.
 *   rays      [n_rays, ray_stride] fp32 rows, first 6 = (o, d); the LAST channel feeds depth's background term (:505)
 *   jitter    [n_rays] U[0,1) draws (required iff T2N_FLAG_TRAIN; the reference draws them on the CPU generator, :313-316)
 *   rgb [n_rays,3], depth [n_rays]   required
 *   weights, z_vals [n_rays, n_samples]   optional (NULL = not materialised; the reference always returns them)
 *   stats     optional device uint64[T2N_STAT_COUNT], zeroed by the call
 *   workspace caller scratch; the call splits n_rays into sub-launches that fit (see t2n_render_workspace_bytes).
 *             t2n_render_workspace_bytes sizes the appearance lists for the worst case (every sample of every ray an appearance
 *             sample: 16 GiB for an 800x800 x 518 frame that uses ~0.2 GB of it). An image-ordered eval frame (T2N_FLAG_COHERENT
 *             with t2n_field_set_frame_width) of >= 65536 rays given LESS than that runs as ONE launch with lists budgeted to
 *             what the workspace holds. The call never waits for the device: rays whose entries find no room are finished on the
 *             device (stats[T2N_STAT_LIST_RETRY] = 1; their colours come from the exact-fp32 head, within ~1e-6 of the split-f16
 *             one; depth and every other ray are unaffected); the sub-list counters travel to pinned host memory behind an event
 *             and a LATER call (or t2n_render_workspace_bytes_hint / t2n_field_list_retries) turns them into the next budget.
 *             t2n_render_workspace_bytes_hint returns a workspace size for that mode: lists for 32 entries per ray while nothing is
 *             known, then one and a half times what the field's last completed budgeted launch needed + 12 (5.0 GB for the frame above:
 *             a budgeted carve holds a feature row per list slot, 164 B per entry, see t2n_field_set_feature_fusion).
 */
size_t t2n_render_workspace_bytes(int64_t rays_per_launch, int n_samples);
/* The general view-dependent heads (T2N_SHADE_MLP_FEA / _MLP_PE / _MLP; models/tensorBase.py:62-86,111-159) evaluate their unfused MLP
 * through activation scratch behind the sizes above: add this many bytes (0 for the other heads) and one pass covers 32 appearance rows
 * per ray; rows beyond that are taken in further passes over the same scratch. The call reads no count on the host and allocates
 * nothing: tile prefix and row count are derived on the device, every kernel clips to them, and the host issues the passes the worst
 * case needs (a pass past the count costs its empty launches). */
size_t t2n_render_head_scratch_bytes(const t2n_field* f, int64_t n_rays);
/* rows per ray that sizing reserves (default 32; the driver's scenes need ~7): fewer rows = less memory per ray, more passes */
int t2n_field_set_head_scratch_rows(t2n_field* f, int rows_per_ray);
size_t t2n_render_workspace_bytes_hint(const t2n_field* f, int64_t n_rays, int n_samples);
size_t t2n_render_workspace_bytes_budget(int64_t n_rays, int n_samples, int entries_per_ray);   /* one launch, lists for this many entries per ray */
uint64_t t2n_field_list_retries(const t2n_field* f);   /* budgeted calls that overflowed their lists since the field was created (waits for counters still in flight) */
int t2n_render_forward(t2n_field* f, const float* rays, int64_t n_rays, int ray_stride, int n_samples, uint32_t flags,
                       const float* jitter, float* rgb, float* depth, float* weights, float* z_vals, uint64_t* stats,
                       void* workspace, size_t workspace_bytes, t2n_stream stream);

/* ---- general-shape path (csrc/t2n_generic.hip): field / head shapes beyond the tuned kernels' — more than 16 density or 48 appearance
 * components per plane (different counts per plane allowed), app_dim up to 64, any fea_pe / view_pe up to 16, featureC up to 256 — the
 * shapes the reference accepts through n_lamb_sigma / n_lamb_sh / data_dim_color / fea_pe / featureC (models/tensoRF.py:144-160,
 * models/tensorBase.py:62-159, e_opt.py:83-107). No field handle: the parameters are read in place in the reference's layouts and the
 * gradients are ACCUMULATED (atomics) into tensors of the same layouts. One thread per ray / per appearance sample, no MFMA: a slow
 * path. Heads: MLP_Fea_noview, MLP_Fea, MLP, SH, RGB. NDC sampling (T2N_FLAG_NDC: `jitter` is then the [n_samples] depth table, as in
 * t2n_render_forward) and the AlphaGridMask (the descriptor's alpha_volume: masked samples are neither evaluated nor differentiated,
 * models/tensorBase.py:451-456) in forward and backward. `weights` / `z_vals` may be NULL in the forward (kept in the workspace then);
 * the backward takes the forward's workspace (and the same weights / z_vals pointers) unchanged.
 * alpha_volume: NULL (no mask: a zeroed tail behaves as before it existed) or the AlphaGridMask occupancy volume on the device,
 * [alpha_dims[0] = D (z)][alpha_dims[1] = H (y)][alpha_dims[2] = W (x)] fp32, over the box alpha_aabb_min / alpha_aabb_max
 * (models/tensorBase.py:41-59). */
typedef struct t2n_generic_desc {
    float aabb_min[3], aabb_max[3], inv_aabb_size[3];
    int32_t grid[3];
    int32_t density_n_comp[3], app_n_comp[3];
    int32_t app_dim, shading, fea_pe, view_pe, feature_c, act;
    float density_shift, distance_scale, weight_thres, step_size, near, far, z_gate;
    const float* alpha_volume;
    int32_t alpha_dims[3];
    float alpha_aabb_min[3], alpha_aabb_max[3];
} t2n_generic_desc;
size_t t2n_generic_workspace_bytes(int64_t n_rays, int n_samples);
/* the same + room for channel-last staging copies of the factor tensors and the appearance-sample list: with this much workspace the
 * FORWARD runs as cooperative kernels (thread per sample for the density, a workgroup per 64 appearance samples for features + head)
 * instead of the plain form — 1 500 x per sample apart on a wide 128^3 field. Same outputs and context; the backward's kernel form
 * (t2n_generic_backward_staged) reuses the staged copies and the list. */
size_t t2n_generic_workspace_bytes_desc(const t2n_generic_desc* desc, int64_t n_rays, int n_samples);
int t2n_generic_forward(const t2n_generic_desc* desc, const t2n_field_params* params, const float* rays, int64_t n_rays, int ray_stride,
                        int n_samples, uint32_t flags, const float* jitter, float* rgb, float* depth, float* weights, float* z_vals,
                        uint64_t* stats, void* workspace, size_t workspace_bytes, t2n_stream stream);
int t2n_generic_backward(const t2n_generic_desc* desc, const t2n_field_params* params, const float* rays, int64_t n_rays, int ray_stride,
                         int n_samples, uint32_t flags, const float* jitter, const float* weights, const float* z_vals,
                         const float* d_rgb, const float* d_depth, const float* d_weights, const t2n_field_grads* grads,
                         void* workspace, size_t workspace_bytes, t2n_stream stream);
/* The same backward as kernels (csrc/t2n_generic_bwd.hip; what autograd derives for models/tensorBase.py:436-507, :19-26, :406-410, the heads
 * :11-17 + :29-39 + :62-159 and models/tensoRF.py:205-239): a wave per ray for the reverse scan, the factor gradients scattered into
 * channel-last copies (lanes along the components of a tap row) and transposed into `grads` at the end, the MLP's weight, bias and basis
 * gradients as exact-fp32 MFMA GEMMs over row chunks with partial slabs and a reduce (no atomics on them: deterministic; the factor
 * gradients carry float-atomic arrival order), in passes of `pass_rows` appearance-list entries issued for the worst case and clipped to
 * the forward's device-side count. `workspace` is the forward's, as t2n_generic_backward receives it: its staged factor copies, list,
 * count and context are reused. t2n_generic_backward_plan (host only, touches no device) says whether the kernel form applies —
 * kernel_form 1: the forward ran its kernel form (head LDS <= 160 KB, T2N_GENERIC_PLAIN unset), the head is SH, RGB or an MLP with <= 512
 * inputs, and T2N_GENERIC_PLAIN_BWD is unset — and how much scratch it needs; where it does not apply, t2n_generic_backward_staged
 * returns T2N_ERR_UNSUPPORTED before it queues anything and the caller takes t2n_generic_backward. pass_rows: 0 = 262144; rounded up to a
 * multiple of 64 and clipped to the call's n_rays * n_samples (rounded likewise). No host read, no allocation, no synchronisation. */
typedef struct t2n_generic_bwd_plan {
    int kernel_form;          /* 1: the kernels, 0: the plain form (t2n_generic_backward) */
    uint32_t pass_rows;       /* list entries per head pass (a multiple of 64) */
    uint32_t max_passes;      /* ceil(n_rays * n_samples / pass_rows) */
    size_t workspace_bytes;   /* of bwd_workspace (0 when kernel_form is 0) */
} t2n_generic_bwd_plan;
int t2n_generic_backward_plan(const t2n_generic_desc* desc, int64_t n_rays, int n_samples, uint32_t pass_rows, t2n_generic_bwd_plan* out);
int t2n_generic_backward_staged(const t2n_generic_desc* desc, const t2n_field_params* params, const float* rays, int64_t n_rays,
                                int ray_stride, int n_samples, uint32_t flags, const float* jitter, const float* weights,
                                const float* z_vals, const float* d_rgb, const float* d_depth, const float* d_weights,
                                const t2n_field_grads* grads, void* workspace, size_t workspace_bytes, void* bwd_workspace,
                                size_t bwd_bytes, uint32_t pass_rows, t2n_stream stream);
/* getDenseAlpha on the general-shape path (models/tensorBase.py:328-344, compute_alpha :412-434): alpha = 1 - exp(-sigma * length) at
 * the nodes aabb_min*(1-s) + aabb_max*s of a dense grid, s = (lin_x[i], lin_y[j], lin_z[k]) (device arrays holding torch.linspace(0,1,g));
 * sigma = 0 where the descriptor's alpha_volume (if any) samples <= 0. alpha is [gx][gy][gz]. Only the density factors and the
 * descriptor are read. Threshold, dilation and bounding box (updateAlphaMask, :346-370) are t2n_alpha_volume's. */
int t2n_generic_dense_alpha(const t2n_generic_desc* desc, const t2n_field_params* params, const float* lin_x, const float* lin_y,
                            const float* lin_z, int gx, int gy, int gz, float length, float* alpha, t2n_stream stream);
/* The pre-activation density feature (compute_densityfeature, models/tensoRF.py:205-220) at exactly the nodes of
 * t2n_generic_dense_alpha, by the same node arithmetic and feature chain: feat [gx][gy][gz], -INFINITY where the descriptor's
 * alpha_volume (if any) samples <= 0 (outside at every finite level: the counterpart of dense alpha's 0 there). The activation is
 * monotone, so feat > f* classifies a node as alpha > alpha(f*) does; marching cubes on feat puts its vertices on the level set. */
int t2n_generic_dense_feature(const t2n_generic_desc* desc, const t2n_field_params* params, const float* lin_x, const float* lin_y,
                              const float* lin_z, int gx, int gy, int gz, float* feat, t2n_stream stream);
/* filtering_rays on the general-shape path (models/tensorBase.py:372-404): bbox_only != 0 — the slab test t_max > t_min against
 * aabb_min / aabb_max (:385-391); bbox_only == 0 — any of the ray's first n_samples eval samples (t_min + i * step, no box test) reads
 * the descriptor's alpha_volume > 0 (:393-395; needs a mask). mask[r] = 0 / 1. No parameters are read. */
int t2n_generic_filter_rays(const t2n_generic_desc* desc, const float* rays, int64_t n_rays, int ray_stride, int n_samples, int bbox_only,
                            uint8_t* mask, t2n_stream stream);

/* ndc_rays_blender (blender = 1) / ndc_rays (0) (dataLoader/ray_utils.py:88-124): [n,3] origins + directions -> NDC. */
int t2n_ndc_rays(int H, int W, float focal, float near, int blender, const float* rays_o, const float* rays_d, int64_t n,
                 float* o_out, float* d_out, t2n_stream stream);

/* eval_sh_bases (models/sh.py:87-133): (deg+1)^2 real SH basis values per unit direction, deg 0..4. dirs [n,3] -> out [n,(deg+1)^2]. */
int t2n_eval_sh_bases(int deg, const float* dirs, int64_t n, float* out, t2n_stream stream);

/* dda + ray_marcher (dataLoader/ray_utils.py:174-228): the AABB-clipped linspace sampler (no call sites in this driver; the
 * live sampler is inside t2n_render_forward). bbox_host = {min xyz, max xyz} or NULL (then near/far = ray columns 6, 7);
 * steps [n_samples] = torch.linspace(0, 1, n_samples) on the device; perturb [n, n_samples] = perturb * U[0,1) draws or NULL.
 * Outputs (any may be NULL): xyz [n, n_samples, 3], z_vals [n, n_samples], near_far [n, 2] (dda's t_min, t_max). */
int t2n_ray_marcher(const float* rays, int64_t n, int ray_stride, int n_samples, int lindisp, const float* bbox_host,
                    const float* steps, const float* perturb, float* xyz, float* z_vals, float* near_far, t2n_stream stream);

/* ---- f-2: frame post-processing of `evaluation` / `evaluation_path` (renderer.py:91-113,168-176; utils.py:241-257) on the
 * device: rgb8 [n,3] = uint8(255 * clamp(rgb,0,1)) (truncation); depth8 [n,3] = OpenCV COLORMAP_JET (B,G,R) of
 * uint8(255 * max((nan_to_num(d) - mi) / (ma - mi + 1e-8), 0)) with d = max((depth - depth_sub) + depth_add, 0) when
 * shift_clamp (the `evaluation` form: push_depth, 0.8) else d = depth (`evaluation_path`); when gt_rgb is given, *sq_err_sum += sum((clamp(rgb) - gt)^2) (double; PSNR = -10 log10(sum / (3 n))). Any output may be NULL. */
int t2n_frame_postprocess(const float* rgb /*[n,3]*/, const float* depth /*[n]*/, int64_t n, float depth_sub, float depth_add,
                          int shift_clamp, float mi, float ma, uint8_t* rgb8, uint8_t* depth8, const float* gt_rgb, double* sq_err_sum,
                          t2n_stream stream);

/* t2n_ssim_views = rgb_ssim (utils.py:436-482; called per view by `evaluation`, renderer.py:103-109, and by the offline scorer
 * extra/compute_metrics.py:34-80,151-162) for a STACK of V image pairs in one tile kernel plus one short reduction, instead of 30
 * scipy.signal.convolve2d calls per view on the host: per channel the five "valid" Gaussian-windowed moments (mu0, mu1, E[a a],
 * E[b b], E[a b]), the clamped variances / covariance, the SSIM map and its mean. Device inputs: img0, img1 [V,H,W,3] of `dtype`
 * (0: float32, 1: float64). The products a*a, b*b, a*b are formed in the input dtype (as `img0**2` is in the reference) and every
 * window sum and all later arithmetic is float64 (scipy widens the image to the float64 filter's dtype), so the map agrees with the
 * reference to ~1e-13 (summation order only). Host input: filter_host [filter_size] = the normalised 1-D taps, copied into the
 * launch by value; 1 <= filter_size <= 33 (compile-time cap of the kernel's LDS stage). c1 = (k1 max_val)^2, c2 = (k2 max_val)^2.
 * clamp01_img0 != 0: img0 is clamped to [0,1] as it is loaded (renderer.py:92), so a raw render can be scored. Device outputs:
 * ssim [V] = mean of each view's map; ssim_map [V,H-fs+1,W-fs+1,3] or NULL; sq_err [V] or NULL = sum((img0 - img1)^2) per view,
 * difference and square in the input dtype, summed in float64 (PSNR = -10 log10(sq_err / (3 H W)), renderer.py:98). No atomics:
 * results are bit-repeatable and a view of a stack is bit-equal to the same view alone. Nothing is allocated or synchronised.
 * Workspace: t2n_ssim_views_workspace_bytes(V, H, W, filter_size) bytes of device memory (0 = bad argument). T2N_ERR_INVALID,
 * before anything is launched: NULL img0 / img1 / filter_host / ssim / workspace, dtype not 0 / 1, filter_size outside 1..33,
 * H or W < filter_size (scipy raises there too), V < 1 (or > 65535), H or W > 32768, workspace too small. */
size_t t2n_ssim_views_workspace_bytes(int V, int H, int W, int filter_size);
int t2n_ssim_views(const void* img0, const void* img1, int dtype /*0: float32, 1: float64*/, int V, int H, int W,
                   const double* filter_host /*[filter_size], host*/, int filter_size, double c1, double c2, int clamp01_img0,
                   double* ssim /*[V]*/, double* ssim_map /*[V,H-fs+1,W-fs+1,3] or NULL*/, double* sq_err /*[V] or NULL*/,
                   void* workspace, size_t workspace_bytes, t2n_stream stream);

/* ---- f-3: the image-space steps either side of the renderer in render_warping_inapinting (text2nerf_main.py:102-141).
 * t2n_sparse_bilateral_filtering = dataLoader/bilateral_filtering.py:5-35 with mask=None, HR=False: per pass the depth
 * discontinuity map (:64-136; 4-neighbour disparity jumps > depth_threshold, or original depth == 0) and the median of the
 * window's non-discontinuity pixels (:138-196) on depth and the three colour channels. Outputs what the driver keeps
 * (:119-120): photo_out [H,W,3] after ALL num_iter passes and depth_out [num_iter,H,W] = the depth BEFORE each pass, i.e.
 * save_depths; its last entry has seen num_iter - 1 passes (reference quirk: the image list aliases one in-place array,
 * the depth list does not). filter_sizes_host: num_iter odd windows <= 7. Bit-exact. */
size_t t2n_image_filter_workspace_bytes(int H, int W);
int t2n_sparse_bilateral_filtering(const float* depth /*[H,W]*/, const float* image /*[H,W,3]*/, int H, int W,
                                   const int* filter_sizes_host, int num_iter, float depth_threshold, float* photo_out,
                                   float* depth_out, void* workspace, size_t workspace_bytes, t2n_stream stream);
/* DIBR: one source view of bilinear_splat_warping_multiview (utils.py:83-119) = Warper.forward_warp (scripts/Warper.py:21-186:
 * per-pixel reprojection in fp64, inverse-bilinear splat with depth-softmax weights into an (H+2, W+2) canvas with fp64
 * atomics) merged into the running target (filled [H,W] u8, image_u8 [H,W,3], depth_out [H,W] f64; caller-zeroed before
 * the first view; earlier views win). Ki9 = inv(K1), T12 = first three rows of T2 inv(T1), K9 = K2 (row-major doubles,
 * host). t2n_warp_finish: white where nothing landed, image / 255 -> fp32, int64 mask. */
size_t t2n_warp_workspace_bytes(int H, int W);
int t2n_warp_view(const float* rgb /*[H,W,3] in [0,1]*/, const float* depth /*[H,W]*/, const uint8_t* mask1 /*[H,W] or NULL*/, int H,
                  int W, const double* Ki9_host, const double* T12_host, const double* K9_host, uint8_t* filled, uint8_t* image_u8,
                  double* depth_out, void* workspace, size_t workspace_bytes, t2n_stream stream);
int t2n_warp_finish(const uint8_t* filled, const uint8_t* image_u8, int H, int W, float* image_out /*[H,W,3]*/,
                    int64_t* mask_out /*[H,W] or NULL*/, t2n_stream stream);

/* dibr_filter_mask2 (utils.py:393-409): raster-order in-place hole filling of the merged warp — unknown pixels whose 5x5
 * neighbourhood is known to more than `threshold` (0.65) take the mean of their known 3x3 neighbours and count as known for
 * the rest of the scan. Runs as skewed wavefronts (t = col + 3 row) in one workgroup. image [H,W,3] fp32, known [H,W]
 * int32 (0 / non-zero), depth [H,W] fp64 or NULL; all updated in place. */
int t2n_dibr_filter_mask2(float* image, int32_t* known, double* depth, int H, int W, float threshold, t2n_stream stream);
/* dibr_filter_mask (utils.py:345-392; the reference's driver does not call it): the scan above with threshold 0.6 and no depth, then a
 * 3x3 fill scan (unknown pixels whose 3x3 neighbourhood is known to more than 0.5), the four border lines (copy the inner neighbour
 * where it is known) and a 3x3 erase scan (known pixels whose neighbourhood is known to less than 0.45 become 255 / unknown), all in
 * place and in raster order (fronts t = col + 2 row). image [H,W,3] fp32, known [H,W] int32. */
int t2n_dibr_filter_mask(float* image, int32_t* known, int H, int W, t2n_stream stream);

/* ---- the support-set builder: from one inpainted RGB-D view to training rays (text2nerf_main.py:380-392,
 * dataLoader/scene_gen.py:305-316), csrc/t2n_support.hip.
 * t2n_warp_views = the bilinear_splat branch of gt_warping (utils.py:122-163): ONE source view forward-warped
 * (Warper.forward_warp, scripts/Warper.py:21-180, fp64) to V target poses, every target an independent output, then the
 * white background and / 255. Device inputs: rgb [H,W,3] fp32 in [0,1] (truncated to uint8 levels like the reference),
 * depth [H,W] fp32, mask1 [H,W] u8 or NULL (the reference's mask_gt, 0 / non-zero: scales every weight), mask_aux [H,W] u8 or
 * NULL (extra output only: aux_out = the mask a second call with mask1 = mask_aux would return, from the same geometry pass).
 * Host inputs (row-major doubles): Ki9 = inv(K), T12 [V][12] = first three rows of inv(pose_tar[v]) inv(inv(pose_gt)), K9 = K.
 * Device outputs: image_out [V,H,W,3] fp32; mask_out [V,H,W] int64 or NULL; depth_out [V,H,W] fp64 or NULL (0 where nothing
 * landed); depth32_out [V,H,W] fp32 or NULL (depth_out rounded, what produce_formatted_data makes of it); aux_out [V,H,W]
 * int64 or NULL (needs mask_aux). Masks are exact; image and depth sum fp64 atomics in an order that varies between runs (image
 * within one uint8 level of numpy's add.at on round-half ties, depth ~1e-15 relative). Views are processed 8 per launch set
 * (three kernels + one memset); workspace: t2n_warp_views_workspace_bytes(H, W, V) bytes of device memory (0 = bad argument).
 * T2N_ERR_INVALID: NULL / non-positive argument, aux_out without mask_aux; T2N_ERR_WORKSPACE: workspace too small. */
size_t t2n_warp_views_workspace_bytes(int H, int W, int V);
int t2n_warp_views(const float* rgb, const float* depth, const uint8_t* mask1, const uint8_t* mask_aux, int H, int W, int V,
                   const double* Ki9_host, const double* T12_host, const double* K9_host, float* image_out, int64_t* mask_out,
                   double* depth_out, float* depth32_out, int64_t* aux_out, void* workspace, size_t workspace_bytes,
                   t2n_stream stream);

/* t2n_format_views = produce_formatted_data (dataLoader/scene_gen.py:31-98): rays of N poses (the arithmetic of
 * t2n_generate_rays: rays_split[i] is bit-equal to it) and the rows whose mask is > 0.5, in the reference's order (view-major,
 * raster order inside a view). Device inputs: images [N,H,W,3] fp32, depths [N,H,W] fp32, masks [N,H,W] of dtype mask_dtype
 * (T2N_MASK_*); masks == NULL is mode 'test': only rays_split is written and images / depths / row buffers / record / workspace
 * may be NULL. Host input: c2w_host [N][12] = first three rows of each camera-to-world matrix (fp32). Device outputs: rays_split
 * [N,H*W,6] or NULL; all_rays [K,6], all_rgbs [K,3], all_depths [K] in buffers of capacity_rows >= N*H*W rows; record [1+N]
 * int64 = {K, kept rows of view 0, ..., of view N-1} (K is data dependent: the caller reads the record once to slice).
 * Deterministic (count, one-workgroup exclusive scan, scatter; no atomics). Workspace: t2n_format_views_workspace_bytes(H, W, N).
 * T2N_ERR_INVALID: NULL / non-positive argument, unknown mask dtype, capacity_rows < N*H*W; T2N_ERR_WORKSPACE: workspace too
 * small. */
enum { T2N_MASK_U8 = 0, T2N_MASK_I32 = 1, T2N_MASK_I64 = 2, T2N_MASK_F32 = 3, T2N_MASK_F64 = 4 };
size_t t2n_format_views_workspace_bytes(int H, int W, int N);
int t2n_format_views(const float* images, const float* depths, const void* masks, int mask_dtype, int N, int H, int W,
                     const float* c2w_host, float fx, float fy, float cx, float cy, float* rays_split, float* all_rays,
                     float* all_rgbs, float* all_depths, int64_t capacity_rows, int64_t* record, void* workspace,
                     size_t workspace_bytes, t2n_stream stream);

/* ---- the inpaint-view builder: everything render_warping_inapinting does before the inpainter (text2nerf_main.py:99-184) without a
 * host hop. The renders are t2n_render_forward and the hole filling t2n_dibr_filter_mask2; the three calls below are the rest.
 * t2n_sparse_bilateral_filtering_views = the per-view filter call of the render loop (text2nerf_main.py:115-119) for a STACK of V
 * views with one schedule: depth [V,H,W], image [V,H,W,3] -> photo_out [V,H,W,3] (vis_photos[-1]) and depth_out [V,H,W]
 * (vis_depths[-1], the depth before the last pass). The view is a grid axis of the kernels of t2n_sparse_bilateral_filtering: a pass
 * is one launch set for all views, and every view is bit-equal to a single-image call. Workspace:
 * t2n_image_filter_views_workspace_bytes(H, W, V) (0 = bad argument). Limits of the stack call, which the single-image call does
 * not have: V <= 4096 (four channels per view on one grid axis) and H * W <= 2^26 pixels per view; beyond either the call returns
 * T2N_ERR_INVALID. */
size_t t2n_image_filter_views_workspace_bytes(int H, int W, int V);
int t2n_sparse_bilateral_filtering_views(const float* depth, const float* image, int V, int H, int W, const int* filter_sizes_host,
                                         int num_iter, float depth_threshold, float* photo_out, float* depth_out, void* workspace,
                                         size_t workspace_bytes, t2n_stream stream);
/* t2n_warp_sources = bilinear_splat_warping_multiview (utils.py:83-119 over Warper.forward_warp, scripts/Warper.py:21-186): V source
 * views forward-warped into ONE target, the earliest source that lands on a pixel wins, then white where nothing landed and / 255 —
 * the work of V t2n_warp_view calls and t2n_warp_finish as one launch set (memset, log-depth maxima, splat, resolve) per chunk of up
 * to 8 sources, each source on its own planar canvas (the arithmetic of t2n_warp_views per source). Device inputs: rgb [V,H,W,3] fp32
 * in [0,1] (truncated to uint8 levels like the reference), depth [V,H,W] fp32, mask1 [V,H,W] u8 or NULL (0 / non-zero: scales the
 * weights of its source). Host inputs (row-major doubles): Ki9 = inv(K), T12 [V][12] = first three rows of inv(pose_tar)
 * inv(inv(pose[v])), K9 = K. Device outputs: image_out [H,W,3] fp32, mask_out [H,W] int64, depth_out [H,W] fp64 (0 where nothing
 * landed). Masks are exact; image and depth sum fp64 atomics in arrival order, as t2n_warp_view does. Workspace:
 * t2n_warp_sources_workspace_bytes(H, W, V), which grows with V up to the 8-source chunk and not beyond (0 = bad argument).
 * T2N_ERR_INVALID: NULL / non-positive argument; T2N_ERR_WORKSPACE: workspace too small. */
size_t t2n_warp_sources_workspace_bytes(int H, int W, int V);
int t2n_warp_sources(const float* rgb, const float* depth, const uint8_t* mask1, int H, int W, int V, const double* Ki9_host,
                     const double* T12_host, const double* K9_host, float* image_out, int64_t* mask_out, double* depth_out,
                     void* workspace, size_t workspace_bytes, t2n_stream stream);
/* t2n_inpaint_pack = the arrays the driver builds around the inpainter (text2nerf_main.py:138-184, update_known_views=False) in one
 * elementwise launch, from the (hole-filled) warp warp_image [H,W,3] fp32, its known map `known` [H,W] int32 (0 / non-zero), the
 * target render rgb_render [H,W,3] fp32 (clamped to [0,1] here) and depth_render [H,W] fp32:
 *   warp_u8 [H,W,3]        uint8(warp_image * 255) * mask  (:138,156-157; a float32 product, truncated)
 *   map_filt [H,W] int64   the mask as 0 / 1;  mask_image, mask_inv [H,W] u8 = mask * 255, (1 - mask) * 255  (:158-159)
 *   mask_ex [H,W,3] int64  the mask on three channels  (:154)
 *   rgb_u8 [H,W,3]         uint8(clamp(rgb_render, 0, 1) * 255)  (:169-170);  rgb_masked_u8 = rgb_u8 * mask + 255 (1 - mask)  (:174-177)
 *   depth_masked [H,W] fp64 = depth_render * mask  (:171)
 * Exact. T2N_ERR_INVALID: NULL / non-positive argument. */
int t2n_inpaint_pack(const float* warp_image, const int32_t* known, const float* rgb_render, const float* depth_render, int H, int W,
                     uint8_t* warp_u8, int64_t* map_filt, uint8_t* mask_image, uint8_t* mask_inv, int64_t* mask_ex, uint8_t* rgb_u8,
                     uint8_t* rgb_masked_u8, double* depth_masked, t2n_stream stream);

/* ---- a-15: backward of the render call w.r.t. all field parameters (what autograd derives in the reference,
 * text2nerf_main.py:589; coordinates are detached there, models/tensoRF.py:208-210,226-228, so no ray gradients exist).
 * Protocol: (1) forward with T2N_FLAG_KEEP_CTX as ONE launch (workspace >= t2n_render_workspace_bytes_ctx), weights and
 * z_vals materialised; (2) t2n_render_ctx_rows returns the padded activation row count: the forward posted the
 * appearance-sample counts to pinned host memory behind its march kernel, so this waits for THAT copy's event (the stream keeps
 * running; a forward whose slot was evicted falls back to a stream-draining read); (3) t2n_render_backward with a second workspace of
 * t2n_backward_workspace_bytes(field, rows, n_rays, n_samples). Differentiable heads: MLP_Fea_noview (fused chain), MLP_Fea and
 * MLP (general path), SH, RGB — tests/test_hip_parity.py::test_g8_*, tests/test_heads.py, tests/test_shapes.py.
 * d_weights may be NULL. Gradients are ACCUMULATED into `g` (reference layouts; NULL members are skipped: the channel-last
 * plane / line gradients then stay in the field for t2n_field_tv_adam_step).
 * Optional: a forward workspace LARGER than t2n_render_workspace_bytes_ctx by 256 + rows * 1728 bytes lets the forward keep
 * the MLP activations of up to `rows` appearance samples (a guess, e.g. 1.25 x the previous call's row count); when the
 * actual count fits — and the same byte count is passed to t2n_render_backward — the backward skips its re-run of the
 * appearance forward. Too small a guess only costs that re-run.
 * Streams: all work is ordered on `stream` as seen by the caller. Internally the density scatter of a call runs on a library-owned
 * side stream that forks from `stream` behind the per-ray backward kernel and is joined into `stream` before the call's gradient
 * writes end (so both workspaces must stay alive until `stream` has passed the call, as for any asynchronous call). */
size_t t2n_render_workspace_bytes_ctx(int64_t n_rays, int n_samples);
int t2n_render_ctx_rows(const void* fwd_workspace, int64_t n_rays, int n_samples, t2n_stream stream, int64_t* rows);
/* What the T2N_FLAG_DEVICE_ROWS backwards of this field recorded, read from pinned host memory (never waits, never touches a
 * stream): out[0..7] = appearance rows the last eight such calls NEEDED (before clipping to their capacity; slot = sequence & 7),
 * out[8] = how many calls overflowed their capacity so far, out[9] = records written. A caller sizes its next capacity from it. */
int t2n_field_device_rows_record(const t2n_field* f, uint32_t out[10]);
size_t t2n_backward_workspace_bytes(const t2n_field* f, int64_t rows, int64_t n_rays, int n_samples);
int t2n_render_backward(t2n_field* f, const float* rays, int64_t n_rays, int ray_stride, int n_samples, uint32_t flags,
                        const float* jitter, const float* d_rgb, const float* d_depth, const float* d_weights,
                        const t2n_field_grads* g, void* fwd_workspace, size_t fwd_workspace_bytes, void* bwd_workspace,
                        size_t bwd_workspace_bytes, t2n_stream stream);

/* The channel-last gradients of the 12 factor tensors live in ONE buffer of t2n_field_grad_buffer_bytes (order: density planes,
 * density lines, appearance planes, appearance lines; 256-B aligned slices). By default the library owns it and every
 * t2n_render_backward zeroes it first (it then holds the gradients of that call). A caller that hands in its own device buffer
 * (t2n_field_set_grad_buffer; NULL returns to the library-owned one) owns the zeroing: backward calls ACCUMULATE into it (a batch
 * split into chunks, gradient accumulation), a data-parallel all-reduce can run on it in place, and t2n_field_tv_adam_step reads
 * it. Replaces the autograd accumulation of text2nerf_main.py:588-590 for those tensors. */
size_t t2n_field_grad_buffer_bytes(const t2n_field* f);
int t2n_field_set_grad_buffer(t2n_field* f, void* buf, size_t bytes);
/* Layout of that buffer: [density planes 0..2 | density lines 0..2 | appearance planes 0..2 | appearance lines 0..2], every tensor
 * channel-last and 256-B aligned. The density part (the first t2n_field_grad_buffer_density_bytes bytes) is final when the backward's
 * density scatter is done — about half a millisecond of a C3 step before the appearance scatter: t2n_field_wait_density_grads makes
 * `waiter` wait for that point of the LAST t2n_render_backward call (no-op before the first one), so that a data-parallel caller
 * can start all-reducing the density bucket on `waiter` while the rest of the backward still runs on its own stream
 * (text2nerf_amd/parallel.py; the reference trains on one GPU: text2nerf_main.py:547-601). */
size_t t2n_field_grad_buffer_density_bytes(const t2n_field* f);
int t2n_field_wait_density_grads(const t2n_field* f, t2n_stream waiter);

/* The driver's loss of one training batch (text2nerf_main.py:559-575; TransMittanceLoss_mask, utils.py:67-80) in one pass over the
 * render outputs: loss = mean((rgb - rgb_t)^2) + w_depth * mean((depth - depth_t)^2) + w_trans * mean_r(m_r^2) with
 * m_r = mean_n(weights[r,n] * [z_vals[r,n] - depth_t[r] + delta < 0]); NaN depths count as 0 and get no gradient (:559-560).
 * Writes the upstream gradients t2n_render_backward takes (d_rgb [R,3], d_depth [R], d_weights [R,N]) and
 * losses[4] = {mse, depth loss, transmittance loss, total} (device floats, deterministic sums). The driver's values:
 * w_depth 0.005, w_trans 1e3, delta 0.1. workspace: t2n_train_loss_workspace_bytes(n_rays). */
size_t t2n_train_loss_workspace_bytes(int64_t n_rays);
int t2n_train_loss(const float* rgb, const float* depth, const float* weights, const float* z_vals, const float* rgb_t,
                   const float* depth_t, int64_t n_rays, int n_samples, float w_depth, float w_trans, float delta, float* d_rgb,
                   float* d_depth, float* d_weights, float* losses, void* workspace, size_t workspace_bytes, t2n_stream stream);

/* The reference's other depth losses (utils.py:301-342, selected upstream by --type_depth_loss, e_opt.py:20) as the depth term of the
 * driver's loss. depth_kind:
 *   0 "mse"     mean((depth - depth_t)^2): t2n_train_loss itself, bit-equal outputs (text2nerf_main.py:563-575);
 *   1 "gnll"    compute_depth_loss + is_not_in_expected_distribution (utils.py:301-320): |mean over the K applying rays of
 *               1/2 (log v + (mu - y)^2 / v)|, var = sum_n (z - mu)^2 w + 1e-8, v = max(var, 1e-3), a ray applies when
 *               |mu - y| - target_std > 0 or target_std^2 < var; K = 0: loss 0, gradients exactly 0;
 *   2 "si_log"  compute_depth_loss_scale_invariant (utils.py:324-331): mean |d + alpha|, d = log mu - log y, alpha = -mean d
 *               (non-positive depths give IEEE's NaN / inf, as upstream);
 *   3 "ssi"     scale_shift_invariant_loss (utils.py:333-342): y ~ s z + t by weighted least squares over all R x N samples
 *               (float64 moments; rank-deficient systems follow the pseudo-inverse), then mean(w (s z + t - y)^2) with s, t
 *               rounded to float32 as upstream's multiplication does; gradient to the weights only.
 * t2n_train_loss_ex: t2n_train_loss with that depth term: losses[4] = {mse, depth term, transmittance loss, mse + w_depth * term +
 * w_trans * transmittance}, d_depth and d_weights carry w_depth times the term's gradients (d_weights: plus the transmittance
 * term's, written once, exact zeros where neither contributes); NaN depths count as 0 and get no d_depth (text2nerf_main.py:559-560).
 * aux (device, 4 doubles): gnll {K, signed mean NLL}, si_log {alpha}, ssi {s, t}, the rest 0. Every scalar that couples the rays
 * stays on the device; sums in a fixed order (two calls give the same bits). workspace: t2n_train_loss_ex_workspace_bytes(n_rays),
 * 8-byte aligned.
 * t2n_depth_loss: the depth term alone (kind 1..3) with its gradients for upstream gradient 1: loss (1 float), d_depth [R] and
 * d_weights [R,N] (either may be NULL); weights / z_vals may be NULL for si_log, depth for ssi; no NaN rule. workspace:
 * t2n_depth_loss_workspace_bytes(n_rays), 8-byte aligned. Python: losses.compute_depth_loss, compute_depth_loss_scale_invariant,
 * scale_shift_invariant_loss.
 * T2N_ERR_INVALID (before any launch): NULL / non-positive argument, unknown kind, target_std <= 0 for gnll, misaligned workspace;
 * T2N_ERR_WORKSPACE: workspace too small. */
size_t t2n_train_loss_ex_workspace_bytes(int64_t n_rays);
int t2n_train_loss_ex(const float* rgb, const float* depth, const float* weights, const float* z_vals, const float* rgb_t,
                      const float* depth_t, int64_t n_rays, int n_samples, float w_depth, float w_trans, float delta, int depth_kind,
                      float target_std, float* d_rgb, float* d_depth, float* d_weights, float* losses, double* aux, void* workspace,
                      size_t workspace_bytes, t2n_stream stream);
size_t t2n_depth_loss_workspace_bytes(int64_t n_rays);
int t2n_depth_loss(int kind, const float* depth, const float* weights, const float* z_vals, const float* depth_t, int64_t n_rays,
                   int n_samples, float target_std, float* loss, double* aux, float* d_depth, float* d_weights, void* workspace,
                   size_t workspace_bytes, t2n_stream stream);

/* The distortion regulariser of mip-NeRF 360 (eq. 15) on the weights along a ray (the reference has no such term). For one ray with
 * ascending sample depths z_0 <= ... <= z_{N-1} (the renderer's z_vals), weights w_n and rho = inv_range = 1 / z_range:
 *   intervals   delta_n = (z_{n+1} - z_n) rho for n < N-1, delta_{N-1} = 0 (the renderer's dists, the last one 0);
 *   midpoints   m_n = ((z_n - z_0) + (z_{n+1} - z_n) / 2) rho, m_{N-1} = (z_{N-1} - z_0) rho (the term is translation-invariant);
 *   loss        L_r = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i;
 *   gradient    dL_r/dw_i = 2 sum_j w_j |m_i - m_j| + (2/3) w_i delta_i;
 *   batch term  D = mean_r L_r; the gradient goes to the weights only (z_vals carry none).
 * Evaluated in O(N) per ray by prefix sums of (w, w m) in sample order (which is why z_vals must ascend). float32 inputs, float64 from
 * the first operation, sums in a fixed order without atomics (two calls give the same bits); the stored gradient and the reported
 * loss are rounded to float32 once.
 * t2n_distortion_loss: the term alone: loss[0] = D (device float) and, unless NULL, d_weights [R,N] = (1/R) dL_r/dw (upstream
 * gradient 1; exact zeros on a ray without weight). workspace: t2n_distortion_loss_workspace_bytes(n_rays), 8-byte aligned. Python:
 * losses.distortion_loss.
 * t2n_train_loss_dist: t2n_train_loss_ex (every depth_kind 0..3) with w_dist D added: losses[4] keeps its layout, total additionally
 * contains w_dist D; dist[0] = D, unweighted (device double); d_weights is still written once: float32(t2n_train_loss_ex's value +
 * (w_dist / R) dL_r/dw); everything else is t2n_train_loss_ex's, bit for bit. With w_dist == 0 every output of t2n_train_loss_ex is
 * bit-equal to that call's (dist[0] is still D). workspace: t2n_train_loss_dist_workspace_bytes(n_rays), 8-byte aligned.
 * T2N_ERR_INVALID (before any launch): NULL / non-positive argument, inv_range not finite or <= 0, w_dist negative or not finite,
 * t2n_train_loss_ex's own cases, misaligned workspace; T2N_ERR_WORKSPACE: workspace too small. */
size_t t2n_distortion_loss_workspace_bytes(int64_t n_rays);
int t2n_distortion_loss(const float* weights, const float* z_vals, int64_t n_rays, int n_samples, float inv_range, float* loss,
                        float* d_weights, void* workspace, size_t workspace_bytes, t2n_stream stream);
size_t t2n_train_loss_dist_workspace_bytes(int64_t n_rays);
int t2n_train_loss_dist(const float* rgb, const float* depth, const float* weights, const float* z_vals, const float* rgb_t,
                        const float* depth_t, int64_t n_rays, int n_samples, float w_depth, float w_trans, float delta, int depth_kind,
                        float target_std, float w_dist, float inv_range, float* d_rgb, float* d_depth, float* d_weights, float* losses,
                        double* aux, double* dist, void* workspace, size_t workspace_bytes, t2n_stream stream);

/* ---- SURVEY.md 8(f-1), optional: the dense tail of the training step as streaming kernels.
 * t2n_tv_grad_add: grad += d/dparam [ weight * TVLoss(param) ] for one reference-layout plane [1,C,H,W]
 *   (utils.py:488-504; the driver's term is TV_loss_*(tvreg) * TV_weight with TV_loss_* = sum_planes 1e-2 * TVLoss,
 *   models/tensoRF.py:193-203 — pass weight = 1e-2 * TV_weight).
 * t2n_adam_step: torch.optim.Adam's update (betas, eps; no weight decay, no amsgrad) on one tensor, `step` = 1-based
 *   step count of that tensor (text2nerf_main.py:453-454,590). */
int t2n_tv_grad_add(const float* param, float* grad, int C, int H, int W, float weight, t2n_stream stream);
/* the same gradient WRITTEN (not added) to `grad`, times the device scalar *upstream when that is non-NULL: the backward of an
 * autograd node whose upstream gradient lives on the device (no host read, no zero fill, no extra scaling pass). */
int t2n_tv_grad_set(const float* param, float* grad, int C, int H, int W, float weight, const float* upstream, t2n_stream stream);
/* TVLoss's two sums of one plane (utils.py:497-498), spread over T2N_TV_SLOTS slot pairs the caller zeroes and adds up (device
 * doubles): sum_s sums[2 s] = sum of squared differences along H, sum_s sums[2 s + 1] = along W;
 * TVLoss(param) = weight * 2 * (h_tv / (C (H-1) W) + w_tv / (C H (W-1))) / batch. */
#define T2N_TV_SLOTS 32
int t2n_tv_value(const float* param, int C, int H, int W, double* sums, t2n_stream stream);
int t2n_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                  float beta2, float eps, int64_t step, t2n_stream stream);
/* the same update for `count` tensors in one launch (host arrays of device pointers / sizes / learning rates / step numbers) */
int t2n_adam_step_multi(int count, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                        const int64_t* sizes, const float* lrs, float beta1, float beta2, float eps, const int64_t* steps,
                        t2n_stream stream);

/* The same step where the data already is: on the field's channel-last device copies, with the channel-last gradients the last
 * t2n_render_backward left in the field (call that with NULL plane / line pointers in t2n_field_grads: the layout pass back
 * to [1,C,H,W] and the caller's zero-filled gradient tensors are then skipped). For each of the 12 factor tensors (order:
 * density_plane[0..2], density_line[0..2], app_plane[0..2], app_line[0..2]): TV gradient (planes; weights as for
 * t2n_tv_grad_add, 0 = none), Adam update with lrs[i] / steps[i], new values written to the device copy AND to the
 * reference-layout tensor params-> (so the caller's nn.Parameters stay current and no t2n_field_upload of the factors is
 * needed — follow with t2n_field_upload_head when the head's tensors changed). exp_avg / exp_avg_sq: caller-owned
 * CHANNEL-LAST state buffers [pos][C] of the tensors' sizes. Per-element arithmetic identical to t2n_tv_grad_add +
 * t2n_adam_step. Not available with bf16 factor storage (T2N_ERR_UNSUPPORTED). */
int t2n_field_tv_adam_step(t2n_field* f, const t2n_field_params* params, float* const* exp_avg, float* const* exp_avg_sq,
                           const float* lrs, const int64_t* steps, float beta1, float beta2, float eps,
                           float tv_weight_density, float tv_weight_app, t2n_stream stream);
/* The TV terms the other way round: the factor gradient buffer (t2n_field_set_grad_buffer, or the library's own) is INITIALISED to the
 * TV gradient of the current device copies — zero for the lines and for a zero weight — before the backward accumulates into it
 * (replaces a zero fill + the TV pass of t2n_field_tv_adam_step, which is then called with both weights 0). One write-only pass that
 * depends on nothing but the parameters: it may run on another stream beside the forward; the backward must be ordered behind it.
 * Replaces (reference): the autograd of TV_loss_density / TV_loss_app (models/tensoRF.py:193-203, text2nerf_main.py:577-586). */
int t2n_field_tv_seed(t2n_field* f, float tv_weight_density, float tv_weight_app, t2n_stream stream);

/* ---- TensoRF's other two parameter regularisers (models/tensoRF.py:173-191; csrc/t2n_reg.hip).
 * L1 (density_L1 = sum_k mean|density_plane[k]| + mean|density_line[k]|), one contiguous tensor of n floats at a time:
 *   t2n_l1_value     sums[0 .. T2N_REG_SLOTS) = partial sums of |param| / n (float64, WRITTEN; the caller adds them: that is mean|param|)
 *   t2n_l1_grad_add  grad += float32(weight / n) * sign(param), sign(+-0) = 0
 *   t2n_l1_grad_set  grad  = float32(weight / n) [* *upstream, a device scalar, when non-NULL] * sign(param)
 * Ortho (vector_comp_diffs), one reference-layout line tensor [1,C,n,1] read as M [C,n], C >= 2 (T2N_ERR_INVALID below):
 *   D = M M^T in float64 in a fixed order (kept in `workspace`: t2n_ortho_workspace_bytes(C) = C * C * 8 bytes, 8-byte aligned)
 *   t2n_ortho_value     *value = sum_{i != j} |D_ij| / (C (C - 1))  (one device double, written)
 *   t2n_ortho_grad_add  grad += weight * 2 / (C (C - 1)) * S M, S_ij = sign(D_ij) off the diagonal, 0 on it (float32 sum over j in order)
 *   t2n_ortho_grad_set  the same WRITTEN, times *upstream when non-NULL
 * No atomics anywhere: two calls on the same input give the same bits. */
#define T2N_REG_SLOTS 64
int t2n_l1_value(const float* param, int64_t n, double* sums, t2n_stream stream);
int t2n_l1_grad_add(const float* param, float* grad, int64_t n, float weight, t2n_stream stream);
int t2n_l1_grad_set(const float* param, float* grad, int64_t n, float weight, const float* upstream, t2n_stream stream);
size_t t2n_ortho_workspace_bytes(int C);
int t2n_ortho_value(const float* param, int C, int64_t n, double* value, void* workspace, size_t workspace_bytes, t2n_stream stream);
int t2n_ortho_grad_add(const float* param, float* grad, int C, int64_t n, float weight, void* workspace, size_t workspace_bytes,
                       t2n_stream stream);
int t2n_ortho_grad_set(const float* param, float* grad, int C, int64_t n, float weight, const float* upstream, void* workspace,
                       size_t workspace_bytes, t2n_stream stream);
/* t2n_field_tv_seed / t2n_field_tv_adam_step with the two terms on the field's channel-last copies: L1 on the density planes
 * (l1_weight_plane) and density lines (l1_weight_line) inside the seed / TV launch — the planes are read and written once, the lines
 * are written with their L1 gradient instead of zero; ortho on the three density lines and the three appearance lines as two more
 * launches for all six (Gram, gradient) behind it on the same stream. Per element the arithmetic of the reference-layout calls above, in
 * the order TV, L1, ortho (bit-identical). With the four new weights 0 these ARE the tv calls. */
int t2n_field_reg_seed(t2n_field* f, float tv_weight_density, float tv_weight_app, float l1_weight_plane, float l1_weight_line,
                       float ortho_weight_density, float ortho_weight_app, t2n_stream stream);
int t2n_field_reg_adam_step(t2n_field* f, const t2n_field_params* params, float* const* exp_avg, float* const* exp_avg_sq,
                            const float* lrs, const int64_t* steps, float beta1, float beta2, float eps,
                            float tv_weight_density, float tv_weight_app, float l1_weight_plane, float l1_weight_line,
                            float ortho_weight_density, float ortho_weight_app, t2n_stream stream);
/* re-pack basis_mat / renderModule only (the factor copies of an uploaded field are left as they are) */
int t2n_field_upload_head(t2n_field* f, const t2n_field_params* p, t2n_stream stream);

/* ---- coarse-to-fine / occupancy-mask maintenance between training stages.
 * t2n_compute_alpha: models/tensorBase.py:412-434 — alpha = 1 - exp(-sigma * length) at world-space points [n,3]; sigma = 0
 *   where the field's AlphaGridMask (if one is set) samples <= 0.
 * t2n_dense_alpha: models/tensorBase.py:328-344 (getDenseAlpha) — the same at the nodes aabb0*(1-s) + aabb1*s of a dense
 *   grid, s = (lin_x[i], lin_y[j], lin_z[k]) (device arrays holding torch.linspace(0,1,g)); alpha is [gx][gy][gz].
 * t2n_dense_feature: the pre-activation density feature (compute_densityfeature, models/tensoRF.py:205-220) at exactly those nodes,
 *   by the same node arithmetic, taps and sum (fp32 or bf16 factor storage alike); feat is [gx][gy][gz], -INFINITY where the
 *   AlphaGridMask samples <= 0 (outside at every finite level: the counterpart of dense alpha's 0 there).
 * t2n_alpha_volume: models/tensorBase.py:349-363 (updateAlphaMask) — clamp, transpose to [gz][gy][gx], 3x3x3 max pool,
 *   binarise at `thres`; bbox_idx (device int[6]) receives the index box of the kept voxels (min x,y,z, max x,y,z;
 *   INT_MAX / -1 when nothing is kept).
 * t2n_upsample_bilinear: models/tensoRF.py:258-272 (up_sampling_VM) — F.interpolate(mode='bilinear', align_corners=True)
 *   of one [C,Hin,Win] factor to [C,Hout,Wout] (lines are [C,L,1]). */
int t2n_compute_alpha(const t2n_field* f, const float* xyz_world, int64_t n, float length, float* alpha, t2n_stream stream);
int t2n_dense_alpha(const t2n_field* f, const float* lin_x, const float* lin_y, const float* lin_z, int gx, int gy, int gz,
                    float length, float* alpha, t2n_stream stream);
int t2n_dense_feature(const t2n_field* f, const float* lin_x, const float* lin_y, const float* lin_z, int gx, int gy, int gz,
                      float* feat, t2n_stream stream);
int t2n_alpha_volume(const float* dense_alpha, int gx, int gy, int gz, float thres, float* volume, int* bbox_idx,
                     t2n_stream stream);
int t2n_upsample_bilinear(const float* src, int C, int Hin, int Win, float* dst, int Hout, int Wout, t2n_stream stream);
/* filtering_rays(bbox_only=False), models/tensorBase.py:393-395: mask[r] = any of the ray's first n_samples eval samples
 * reads the field's AlphaGridMask > 0 (needs a mask set with t2n_field_set_alpha_mask). */
int t2n_filter_rays_alpha(const t2n_field* f, const float* rays, int64_t n_rays, int ray_stride, int n_samples, uint8_t* mask,
                          t2n_stream stream);

/* Global depth alignment of the inpainting loop, text2nerf_main.py:241-270: scale of the monocular estimate from the ratios of depth
 * differences between consecutive pixels of the caller's sample list ([n_samples][2] int32 (row, col): random.sample of the filled
 * pixels, :234-240), kept when finite, >= 0 and within 5 |thresh - 1| of 1, thresh = (max rendered - push_depth) / (max estimate -
 * push_depth), fallback thresh; then the mean shift against the rendered depth over the samples within 2 |max scaled - max rendered|,
 * fallback that difference. depth_shift [H,W] = scale * depth_est - shift; scale_shift: device double[4] = {scale, shift, pairs kept,
 * samples kept}. Double precision, deterministic. */
int t2n_depth_align_global(const float* depth_rendered, const float* depth_est, int H, int W, const int32_t* pixel_sample_yx,
                           int n_samples, double push_depth, float* depth_shift, double* scale_shift, t2n_stream stream);
/* The same over an EMPTY sample list, which t2n_depth_align_global rejects (n_samples < 1): no pixel of the warped view is filled,
 * :233-240 give pixel_sample = [], and the reference falls through to scale = thresh (:251-252) and shift = max scaled - max
 * rendered (:265-266). Same outputs; pairs kept = samples kept = 0. */
int t2n_depth_align_fallback(const float* depth_rendered, const float* depth_est, int H, int W, double push_depth, float* depth_shift,
                             double* scale_shift, t2n_stream stream);

/* ---- The depth stage of a new view: what text2nerf_main.py does between the inpainter and the support set (:230-299) and the
 * update_known_views=True mask expansion (:147-162), apart from the networks. All exact and deterministic (no atomics); H * W < 2^31.
 *
 * Filled pixels, :233-239: `pixel_filled` lists the pixels with myMap_filt > 0 column by column (column ascending, inside a column row
 * ascending; the reference's loop bounds assume H == W, the order is defined here for any H, W) as (row, col), and
 * random.sample(pixel_filled, k) is [pixel_filled[r] for r in random.sample(range(n), k)] with the generator left in the same state.
 * So the draw stays on the host and the image on the device:
 *   t2n_filled_pixels_count   per-column counts of known > 0 (known [H,W] int32), their exclusive scan into the workspace (W + 1 int32
 *                             offsets; t2n_filled_pixels_workspace_bytes(H, W), 0 = bad argument), n to count_out (device int64)
 *   t2n_filled_pixels_select  ranks [K] int32 (device; each in [0, n)) -> pixel_yx [K][2] int32 (row, col), the layout
 *                             t2n_depth_align_global reads; the workspace as the count call left it for the same map. K = 0 is a
 *                             no-op; a rank outside [0, n) gives (-1, -1).
 * T2N_ERR_INVALID: NULL / non-positive argument. */
size_t t2n_filled_pixels_workspace_bytes(int H, int W);
int t2n_filled_pixels_count(const int32_t* known, int H, int W, void* workspace, int64_t* count_out, t2n_stream stream);
int t2n_filled_pixels_select(const int32_t* known, int H, int W, const void* workspace, const int32_t* ranks, int K, int32_t* pixel_yx,
                             t2n_stream stream);
/* t2n_depth_merge_inputs = the merge network's inputs, :275-276, in one elementwise launch, from depth_rendered [H,W] fp64 (the
 * rendered depth times the mask, t2n_inpaint_pack's depth_masked), the map `known` [H,W] int32 (0 / non-zero) and depth_shift [H,W]
 * fp32 (t2n_depth_align_global's output), with numpy's dtype rules for these inputs:
 *   depth_ref [H,W] fp32 = float32(((depth_rendered - push) * 12000 / 32768. - 1.) * mask)   fp64 arithmetic, rounded once  (:275)
 *   depth_src [H,W] fp32 = (depth_shift - push) * 12000 / 32768. - 1.                        fp32 operation by operation    (:276)
 *   mask [H,W] fp32      = the map as 0 / 1: run_finetune_numpy's mask_ref                                                  (:277)
 * T2N_ERR_INVALID: NULL / non-positive argument. */
int t2n_depth_merge_inputs(const double* depth_rendered, const int32_t* known, const float* depth_shift, int H, int W, double push_depth,
                           float* depth_ref, float* depth_src, float* mask, t2n_stream stream);
/* t2n_view_finish = the arrays rebuilt after the merge network, in one elementwise launch, from depth_merged [H,W] fp32 (the
 * network's output in [-1,1]), the chosen inpainted image img_u8 [H,W,3] uint8 and the map `known` [H,W] int32:
 *   depth_new [H,W] fp32            = ((depth_merged + 1.) * 32768.) / 12000 + push   fp32 operation by operation  (:278, :282)
 *   img_new [H,W,3] fp32            = float32(double(img_u8) / 255.)                                               (:285)
 *   mask_inpainted [H,W] int64      = 1 - mask                                                                     (:296)
 * T2N_ERR_INVALID: NULL / non-positive argument. */
int t2n_view_finish(const float* depth_merged, const uint8_t* img_u8, const int32_t* known, int H, int W, double push_depth,
                    float* depth_new, float* img_new, int64_t* mask_inpainted, t2n_stream stream);
/* t2n_mask_expand = the update_known_views=True mask expansion, :147-152: (cv2.blur(myMap_filt as float32, (5,5)) > 0.99) * 1 with
 * OpenCV's default border (BORDER_REFLECT_101). 25 set taps average to >= 0.9999 and 24 to 0.96 in float32 whatever the summation
 * order, so the test is the AND of the 25 taps. known [H,W] int32 (0 / non-zero) -> eroded [H,W] int32 (0 / 1; not in place) and
 * mask_ex [H,W,3] int64 = the removed ring (mask - eroded) on three channels (:150-151). T2N_ERR_INVALID: NULL argument, H or W < 3. */
int t2n_mask_expand(const int32_t* known, int H, int W, int32_t* eroded, int64_t* mask_ex, t2n_stream stream);

/* ---- Mesh export: marching cubes over a dense volume on the device, in the place of skimage.measure.marching_cubes on a host copy
 * in convert_sdf_samples_to_ply (utils.py:512-572; upstream's export_mesh hands it getDenseAlpha's volume). volume [n0][n1][n2] fp32,
 * contiguous, last index fastest. A node is inside iff v > level (strict: NaN is outside). A crossed grid edge carries one vertex,
 * owned by the edge's lower node; cases and triangles come from a generated table (csrc/t2n_mc_table.h, tools/gen_mc_table.py) whose
 * meshes are closed oriented 2-manifolds with right-hand normals towards LOWER values. No atomics: vertices come in node-linear order
 * (inside a node axis 0, 1, 2), triangles in cell-linear order (inside a cell table order), both functions of the input alone.
 *   t2n_mc_count   classifies every node and cell, scans the counts into the workspace (t2n_mc_workspace_bytes(n0, n1, n2) bytes of
 *                  device memory, 0 = bad argument) and writes the totals to counts_out (device int64 [2]: vertices, triangles).
 *                  Totals of 2^31 and more are the caller's to refuse (the workspace then holds wrapped offsets).
 *   t2n_mc_emit    takes the workspace as the count call left it for the same volume and level (it fills in the per-node vertex bases,
 *                  the one region the count call leaves unwritten) and writes verts [V][3] fp32, normals [V][3] fp32 (or NULL: not
 *                  computed) and faces [T][3] int32; flip != 0 swaps the last two indices of every triple. With zero vertices nothing
 *                  is written.
 * Vertex on the edge from node v0 along axis a to v1, fp32, one IEEE operation per step: t = (level - v0) / (v1 - v0), clamped to [0,1]
 * (fmaxf, then fminf: a NaN becomes 0, so +-inf and NaN neighbours give finite vertices), p_a = (float)index_a + t, world = origin + p *
 * spacing per component (origin3, spacing3: host float [3]). Normal: node gradients by central differences / (2 spacing), one-sided /
 * spacing at a border; g = g0 + t * (g1 - g0); -g / |g|, zero where |g| is zero or not finite.
 * T2N_ERR_INVALID (before any HIP call): NULL pointer, a dimension < 2, n0 * n1 * n2 >= 2^31, a spacing that is not finite and
 * positive. */
size_t t2n_mc_workspace_bytes(int n0, int n1, int n2);
int t2n_mc_count(const float* volume, int n0, int n1, int n2, float level, void* workspace, int64_t* counts_out, t2n_stream stream);
int t2n_mc_emit(const float* volume, int n0, int n1, int n2, float level, const void* workspace, const float* origin3,
                const float* spacing3, int flip, float* verts, float* normals_or_null, int32_t* faces, t2n_stream stream);

/* ---- Mesh export: connected components of a triangle list and removal of the unwanted ones ("floaters") on the device, the stage
 * behind marching cubes that users of upstream's --export_mesh run on the host (MeshLab, trimesh). All integer: every output is a
 * function of the input alone, two calls give bit-equal arrays. faces [F][3] int32 into n_verts vertices.
 *   connectivity   two vertices are connected when a face contains both; a vertex that no face references is a component of its own
 *                  with 0 faces. A face with an index outside [0, n_verts) violates the precondition (the Python layer checks it):
 *                  every kernel skips such a face and never touches memory through it.
 *   labels         dense, 0 .. K-1, numbered in the order of each component's SMALLEST vertex index (vertex 0 is in component 0).
 *   t2n_mesh_components       fills labels [V] int32 and K (n_components_out: device int64 [1]). Lock-free union-find: parent[v] = v,
 *                  one thread per face unites (f0,f1) and (f1,f2): find both roots, atomicMin(&parent[hi], lo); a returned value other
 *                  than hi means hi was no longer a root and the thread goes on uniting (returned value, lo). parent[x] <= x only ever
 *                  decreases, so a component's final root is its smallest vertex whatever order the threads ran in. Then flatten,
 *                  exclusive scan of the root flags (per-256 sums, one workgroup with a running carry), labels = rank of the root.
 *   t2n_mesh_component_sizes  vert_counts [K] and face_counts [K] int32 (a face counts for the component of its first vertex); integer
 *                  atomics, equal labels combined inside a wave first.
 *   t2n_mesh_filter_count     keep [K] uint8: per-vertex flags keep[labels[v]], per-face flags through the face's first vertex, two
 *                  exclusive scans into the workspace, the totals to totals_out (device int64 [2]: vertices, faces).
 *   t2n_mesh_filter_emit      takes the workspace as the count call left it for the same arguments and writes the kept vertex rows
 *                  (verts [V'][3] fp32, normals [V'][3] fp32 or NULL, colors [V'][3] uint8 or NULL: in and out NULL together) and the
 *                  kept faces re-indexed, both in their input order. No atomics. With zero kept vertices nothing is written.
 * One workspace serves all four: t2n_mesh_components_workspace_bytes(n_verts, n_faces) bytes of device memory (0 = bad argument).
 * T2N_ERR_INVALID (before any HIP call): NULL required pointer, a negative count, n_verts >= 2^31, 3 * n_faces >= 2^31, n_components
 * outside [0, n_verts], workspace_bytes smaller than required. */
size_t t2n_mesh_components_workspace_bytes(int64_t n_verts, int64_t n_faces);
int t2n_mesh_components(const int32_t* faces, int64_t n_faces, int64_t n_verts, int32_t* labels, int64_t* n_components_out, void* workspace,
                        size_t workspace_bytes, t2n_stream stream);
int t2n_mesh_component_sizes(const int32_t* faces, int64_t n_faces, const int32_t* labels, int64_t n_verts, int64_t n_components,
                             int32_t* vert_counts, int32_t* face_counts, t2n_stream stream);
int t2n_mesh_filter_count(const int32_t* faces, int64_t n_faces, const int32_t* labels, int64_t n_verts, const uint8_t* keep,
                          int64_t n_components, void* workspace, size_t workspace_bytes, int64_t* totals_out, t2n_stream stream);
int t2n_mesh_filter_emit(const int32_t* faces, int64_t n_faces, const int32_t* labels, int64_t n_verts, const uint8_t* keep,
                         int64_t n_components, const float* verts, const float* normals_or_null, const uint8_t* colors_or_null,
                         void* workspace, size_t workspace_bytes, float* verts_out, float* normals_out_or_null,
                         uint8_t* colors_out_or_null, int32_t* faces_out, t2n_stream stream);

/* ---- Mesh export: selection by per-face flags, the generic form of the filter above. keep [F] uint8: face t stays iff keep[t] != 0 (a
 * face with an index outside [0, n_verts) never stays); a vertex stays iff a kept face references it. Kept faces and kept vertices keep
 * their input order, the verts / normals / colors rows move together, faces are re-indexed. The vertices' "used" flags are idempotent
 * byte stores of 1; everything else is scans and one pass: all integer, no float operation, two calls give bit-equal arrays.
 *   t2n_mesh_select_faces_count   marks the used vertices, scans both flag arrays into the workspace
 *                  (t2n_mesh_select_faces_workspace_bytes(n_verts, n_faces) bytes of device memory, 0 = bad argument) and writes the
 *                  totals to totals_out (device int64 [2]: vertices, faces).
 *   t2n_mesh_select_faces_emit    takes the workspace as the count call left it for the same arguments and writes the kept rows and the
 *                  kept faces (normals / colors: in and out NULL together). With zero kept vertices nothing is written.
 * T2N_ERR_INVALID (before any HIP call): NULL required pointer, a negative count, n_verts >= 2^31, 3 * n_faces >= 2^31, workspace_bytes
 * smaller than required. */
size_t t2n_mesh_select_faces_workspace_bytes(int64_t n_verts, int64_t n_faces);
int t2n_mesh_select_faces_count(const int32_t* faces, int64_t n_faces, int64_t n_verts, const uint8_t* keep, void* workspace,
                                size_t workspace_bytes, int64_t* totals_out, t2n_stream stream);
int t2n_mesh_select_faces_emit(const int32_t* faces, int64_t n_faces, int64_t n_verts, const uint8_t* keep, const float* verts,
                               const float* normals_or_null, const uint8_t* colors_or_null, void* workspace, size_t workspace_bytes,
                               float* verts_out, float* normals_out_or_null, uint8_t* colors_out_or_null, int32_t* faces_out,
                               t2n_stream stream);

/* ---- Mesh export: TSDF fusion of depth views (csrc/t2n_tsdf.hip). The volume is a frame of nodes, node (a,b,c) at x_k = (double)o_k +
 * (double)idx_k * (double)s_k (origin3, spacing3: host float [3], the values t2n_mc_emit takes), and its state is float32: tsdf
 * [n0][n1][n2], weight [n0][n1][n2], optionally color [n0][n1][n2][3]; untouched = tsdf 1, weight 0, colour 0. All arithmetic is double,
 * one IEEE operation per written operation in the written order; the state is rounded to float32 AFTER EVERY VIEW, so V calls of one
 * view equal one call of V views bit for bit. No atomics: a node is owned by one thread.
 *   t2n_tsdf_integrate   depth [V][H][W] fp32, rgb [V][H][W][3] fp32 or NULL (rgb and color: NULL together), pixel_weight [V][H][W] fp32
 *     or NULL, w2c [V][12] double in DEVICE memory: the rows of the 3x4 world-to-camera matrices M. kind 0: depth is the distance along
 *     the ray, kind 1: the camera-space z. For every node, views v = 0 .. V-1 in order:
 *       1. p_k = ((M_k0 x_0 + M_k1 x_1) + M_k2 x_2) + M_k3; skip unless p_2 > near
 *       2. u = (fx p_0) / p_2 + cx, v = (fy p_1) / p_2 + cy; skip unless 0 <= u < W and 0 <= v < H; i = floor(u), j = floor(v): the
 *          nearest pixel (pixel i spans [i, i+1), centre i + 0.5: t2n_generate_rays' convention)
 *       3. d = depth[v][j][i], skip unless finite and > 0; w = 1 or pixel_weight[v][j][i], skip unless finite and > 0
 *       4. r = sqrt((p_0 p_0 + p_1 p_1) + p_2 p_2) (kind 0) or p_2 (kind 1); sdf = d - r; skip if sdf < -trunc; s = min(1, sdf / trunc)
 *       5. Wn = (double)W + w; T <- (float)(((double)W (double)T + w s) / Wn), every colour channel the same with rgb in s's place;
 *          W <- (float)min(Wn, max_weight) (max_weight = +inf: no cap)
 *     n_views == 0 launches nothing.
 *   t2n_tsdf_face_flags  the observed-cells rule, keep [F] uint8 for t2n_mesh_select_faces: c_k = (((double)x_a,k + x_b,k) + x_c,k) / 3.0,
 *     g_k = (c_k - (double)o_k) / (double)s_k, cell_k = clamp(floor(g_k), 0, n_k - 2) (a NaN: 0), keep = 1 iff all eight corners of that
 *     cell have (double)weight > min_weight. A face with an index outside [0, n_verts): 0.
 *   t2n_tsdf_sample_colors  colors_out [V][3] uint8: g_k = ((double)x_k - o_k) / s_k, cell_k as above, f_k = clamp(g_k - cell_k, 0, 1);
 *     the eight corners in the order (0,0,0), (0,0,1), (0,1,0), ... (axis 2 fastest), trilinear weight ((a_0 a_1) a_2) with a_k = f_k or
 *     1 - f_k; only corners with weight > min_weight enter sum w and sum w c (both from 0.0 in that order); colour = sum wc / sum w (0
 *     unless sum w > 0), clamped to [0,1], times 255, rounded half to even.
 * T2N_ERR_INVALID (before any HIP call): NULL required pointer, a dimension < 1 (integrate) or < 2 (the other two), a negative count,
 * n_verts >= 2^31, 3 * n_faces >= 2^31, a spacing or trunc that is not finite and positive, an origin or intrinsic that is not finite,
 * fx or fy zero, max_weight not > 0, a NaN min_weight, an unknown kind. T2N_ERR_UNSUPPORTED: n0 * n1 * n2 >= 2^31. */
int t2n_tsdf_integrate(float* tsdf, float* weight, float* color_or_null, int n0, int n1, int n2, const float* depth,
                       const float* rgb_or_null, const float* pixel_weight_or_null, const double* w2c, int n_views, int H, int W, double fx,
                       double fy, double cx, double cy, const float* origin3, const float* spacing3, double trunc, double near,
                       double max_weight, int kind, t2n_stream stream);
int t2n_tsdf_face_flags(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* weight, int n0, int n1,
                        int n2, const float* origin3, const float* spacing3, double min_weight, uint8_t* keep, t2n_stream stream);
int t2n_tsdf_sample_colors(const float* verts, int64_t n_verts, const float* weight, const float* color, int n0, int n1, int n2,
                           const float* origin3, const float* spacing3, double min_weight, uint8_t* colors_out, t2n_stream stream);

/* ---- Mesh export: Taubin (lambda | mu) smoothing and vertex normals on the device, the stage users of TensoRF-family exports run
 * afterwards in MeshLab. Every output is a function of the face SET and the positions alone (not of face order, corner order or thread
 * order): no float atomics, two calls give bit-equal arrays. faces [F][3] int32 into n_verts vertices, 6 * n_faces < 2^31.
 *   rows           Both row structures are CSR arrays (offsets [V+1] int64, values [E] int32) built from 64-bit keys row << 32 | value:
 *                  t2n_mesh_edge_keys writes keys [6 F] (face (a,b,c): a->b, b->a, b->c, c->b, c->a, a->c; an edge whose ends are the
 *                  same index, and every edge of a face with an index outside [0, n_verts), is INT64_MAX), t2n_mesh_face_keys keys [3 F]
 *                  ((vertex, face index) per corner). The caller sorts the keys ascending (any 64-bit sort), and t2n_mesh_csr keeps each
 *                  key that differs from its predecessor and whose row is inside [0, n_rows): values [count] int32 = the keys' low
 *                  words in sorted order (room for n_keys), offsets[v] = the number of kept keys below v << 32, count_out (device int64
 *                  [1]) = offsets[n_rows]. So every row is ascending and unique: N(v) of the adjacency is the set of u != v sharing
 *                  a face edge with v, duplicate faces add nothing, and a vertex twice in a face owns that face once.
 *                  Workspace: t2n_mesh_csr_workspace_bytes(n_keys) bytes of device memory (0 = bad argument).
 *   t2n_mesh_smooth_pass   pos_out[v] = x_v + s * (mean_{u in N(v)} x_u - x_v) on float64 positions [V][3], one thread per vertex: the
 *                  sum starts at 0.0 and runs over the row in its ascending order, then / (double)degree, - x_v, * s, + x_v, every
 *                  operation rounded on its own (no contraction). A vertex with an empty row, or with fixed_or_null[v] != 0, keeps its
 *                  position. One Taubin iteration = a pass with s = lambda, then one with s = mu < 0, between two buffers of the
 *                  caller (pos_out must not be pos_in). n_entries = the length of `neighbours`; rows are clipped to it and a neighbour
 *                  outside [0, n_verts) is skipped, so no memory is touched through a bad array.
 *   t2n_mesh_vertex_normals   n_v = sum over the faces of row v (vf_offsets / vf_faces: the CSR of t2n_mesh_face_keys), in ascending
 *                  face index, of (x_b - x_a) x (x_c - x_a), in float64 from the fp32 positions; h = n / max |component|; normals[v] =
 *                  (float)(h / sqrt(h0 h0 + h1 h1 + h2 h2)): right-hand orientation, which is marching cubes' (out of the dense
 *                  region). Exactly 0 for a vertex of no face, of degenerate faces only, or with a sum that is not finite.
 * T2N_ERR_INVALID (before any HIP call): NULL required pointer, a negative count, n_verts / n_rows / n_keys >= 2^31, 6 * n_faces >=
 * 2^31, workspace_bytes smaller than required, pos_out == pos_in, s not finite. Empty inputs launch nothing they do not need. */
size_t t2n_mesh_csr_workspace_bytes(int64_t n_keys);
int t2n_mesh_edge_keys(const int32_t* faces, int64_t n_faces, int64_t n_verts, int64_t* keys, t2n_stream stream);
int t2n_mesh_face_keys(const int32_t* faces, int64_t n_faces, int64_t n_verts, int64_t* keys, t2n_stream stream);
int t2n_mesh_csr(const int64_t* sorted_keys, int64_t n_keys, int64_t n_rows, int64_t* offsets, int32_t* values, int64_t* count_out,
                 void* workspace, size_t workspace_bytes, t2n_stream stream);
int t2n_mesh_smooth_pass(const double* pos_in, double* pos_out, const int64_t* offsets, const int32_t* neighbours, int64_t n_entries,
                         const uint8_t* fixed_or_null, int64_t n_verts, double s, t2n_stream stream);
int t2n_mesh_vertex_normals(const float* verts, const int32_t* faces, int64_t n_faces, const int64_t* vf_offsets, const int32_t* vf_faces,
                            int64_t n_entries, int64_t n_verts, float* normals, t2n_stream stream);

/* ---- Mesh export: simplification by vertex clustering on a uniform grid with quadric-optimal representatives (Lindstrom's out-of-core
 * simplification), the decimation that users of TensoRF-family exports run last in MeshLab. No priority queue: keys -> sort -> rows -> one
 * thread per row, like the stage above. Every output is a function of the input alone: integer keys, float64 sums in a fixed order, no
 * float atomics, two calls give bit-equal arrays. Clustering does NOT preserve manifoldness. origin3, cell3 (float64) and dims3 (int32)
 * are host arrays of three. Every float64 operation below is a single IEEE operation (no contraction), in the order written.
 *   grid           vertex v lies in cell c_k = floor(((double)x_k - o_k) / h_k), k = 0, 1, 2; the cell's id is (c0 n1 + c1) n2 + c2 with
 *                  n = dims3, n0 n1 n2 < 2^31. t2n_mesh_cluster_keys writes keys [V] = id << 32 | v; a vertex that is not finite or
 *                  whose cell is outside [0, n) gets the high word 2^31 - 1, behind every cell. The caller sorts the keys ascending.
 *   t2n_mesh_cluster_rows   over the SORTED keys: clusters are the occupied cells, numbered 0 .. K-1 in ascending id (a flag where the high
 *                  word changes, per-256 sums, one workgroup's scan with a running carry). vertex_map [V] int32 (-1 for a vertex outside
 *                  the grid), offsets int64 (room for V + 1, K + 1 written), members [V] int32 (row k = members[offsets[k] :
 *                  offsets[k+1]], ascending vertex index), cells int32 (room for [V][3], [K][3] written: c0, c1, c2), K to
 *                  n_clusters_out (device int64 [1]). Workspace: t2n_mesh_cluster_rows_workspace_bytes(n_verts) (0 = bad argument).
 *   t2n_mesh_cluster_face_keys   keys [3 F] = vertex_map[corner] << 32 | face per corner (INT64_MAX for a face with an index outside
 *                  [0, n_verts) or a map outside [0, n_clusters)); sorted and given to t2n_mesh_csr with n_rows = K they are the
 *                  cluster -> face rows: every face with at least one corner in the cluster, once, ascending.
 *   t2n_mesh_cluster_place   out [K][3] fp32, one thread per cluster. mean_k = (the members' (double)x_k summed from 0.0 in ascending
 *                  vertex index) / (double)count. quadric = 0: out = (float)mean. quadric = 1: over the cluster's face row in its
 *                  order, (a, b, c) = the face's corners rotated so that its smallest vertex index (the first of equal ones) comes
 *                  first; u = x_b - x_a, w = x_c - x_a in float64 from the fp32 positions; n = (u1 w2 - u2 w1, u2 w0 - u0 w2,
 *                  u0 w1 - u1 w0), unnormalised: faces weigh by squared area and there is no square root; a face whose n is all zero or
 *                  not finite is skipped; d = x_a - mean; r = (n0 d0 + n1 d1) + n2 d2; A00 += n0 n0, A01 += n0 n1, A02 += n0 n2,
 *                  A11 += n1 n1, A12 += n1 n2, A22 += n2 n2, b_k += n_k r (product, then sum). t = (A00 + A11) + A22; if t is not > 0 or
 *                  not finite the result is the mean. Else e = regularisation * t, M_kk = A_kk + e, and (A + e I) x = b by cofactors:
 *                      C00 = M11 M22 - A12 A12    C01 = A02 A12 - A01 M22    C02 = A01 A12 - A02 M11
 *                      C11 = M00 M22 - A02 A02    C12 = A01 A02 - M00 A12    C22 = M00 M11 - A01 A01
 *                      det = (M00 C00 + A01 C01) + A02 C02
 *                      x_0 = ((C00 b0 + C01 b1) + C02 b2) / det, x_1 with (C01, C11, C12), x_2 with (C02, C12, C22)
 *                  p = mean + x; lo_k = o_k + (double)c_k h_k, hi_k = o_k + (double)(c_k + 1) h_k with c = cells[cluster]; p is the
 *                  result iff lo_k <= p_k <= hi_k on every axis (a p that is not finite fails), else the mean. Rounded to fp32 once. The
 *                  Tikhonov term e pulls flat and creased clusters towards the mean and keeps the system positive definite: no SVD, no
 *                  threshold. n_members / n_entries = the lengths of members / face_rows; rows are clipped to them, and a member, face
 *                  or corner outside its range is skipped. With quadric = 0 faces, cells, face_offsets and face_rows may be NULL.
 *   t2n_mesh_cluster_colors   out [K][3] uint8 = (sum of the members' channel + count / 2) / count in integers.
 *   t2n_mesh_simplify_face_map   rotated [F][3] int32: every index through vertex_map, the triple rotated so that the smallest index
 *                  comes first (cyclic order kept); (-1, -1, -1) for a face with two equal mapped indices (dropped) or a bad index.
 *                  key_hi [F] = the first index (n_clusters for a dropped face), key_lo [F] = second << 32 | third (INT64_MAX for a
 *                  dropped face). The caller sorts STABLY by key_lo, then stably by key_hi: `order` [F] int64, the faces by rotated
 *                  triple, equal triples in ascending face index.
 *   t2n_mesh_simplify_faces   keeps, of the faces with the same rotated triple, the one with the lowest face index (an oppositely
 *                  oriented twin (a, c, b) is another triple and stays), and writes the kept rotated triples in ascending face index to
 *                  faces_out (room for [F][3]) and their number to count_out (device int64 [1]). Flags, scan and compaction as above.
 *                  Workspace: t2n_mesh_simplify_faces_workspace_bytes(n_faces) (0 = bad argument).
 * T2N_ERR_INVALID (before any HIP call): NULL required pointer, a negative count, n_verts >= 2^31, 3 * n_faces >= 2^31, n_clusters outside
 * [0, n_verts], a cell that is not finite and positive, an origin that is not finite, a dimension < 1, 2^31 cells and more, a
 * regularisation that is negative or not finite, quadric outside {0, 1}, workspace_bytes smaller than required. Empty inputs launch no
 * kernel. */
int t2n_mesh_cluster_keys(const float* verts, int64_t n_verts, const double* origin3, const double* cell3, const int32_t* dims3, int64_t* keys,
                          t2n_stream stream);
size_t t2n_mesh_cluster_rows_workspace_bytes(int64_t n_verts);
int t2n_mesh_cluster_rows(const int64_t* sorted_keys, int64_t n_verts, const int32_t* dims3, int32_t* vertex_map, int64_t* offsets,
                          int32_t* members, int32_t* cells, int64_t* n_clusters_out, void* workspace, size_t workspace_bytes, t2n_stream stream);
int t2n_mesh_cluster_face_keys(const int32_t* faces, int64_t n_faces, int64_t n_verts, const int32_t* vertex_map, int64_t n_clusters,
                               int64_t* keys, t2n_stream stream);
int t2n_mesh_cluster_place(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const int64_t* offsets,
                           const int32_t* members, int64_t n_members, const int32_t* cells, int64_t n_clusters, const int64_t* face_offsets,
                           const int32_t* face_rows, int64_t n_entries, const double* origin3, const double* cell3, double regularisation,
                           int quadric, float* out, t2n_stream stream);
int t2n_mesh_cluster_colors(const uint8_t* colors, int64_t n_verts, const int64_t* offsets, const int32_t* members, int64_t n_members,
                            int64_t n_clusters, uint8_t* out, t2n_stream stream);
int t2n_mesh_simplify_face_map(const int32_t* faces, int64_t n_faces, int64_t n_verts, const int32_t* vertex_map, int64_t n_clusters,
                               int32_t* rotated, int64_t* key_hi, int64_t* key_lo, t2n_stream stream);
size_t t2n_mesh_simplify_faces_workspace_bytes(int64_t n_faces);
int t2n_mesh_simplify_faces(const int32_t* rotated, const int64_t* order, int64_t n_faces, int32_t* faces_out, int64_t* count_out,
                            void* workspace, size_t workspace_bytes, t2n_stream stream);

/* ---- Floaters in the field: connected components of a dense volume on the device and removal of the unwanted ones, the stage users of
 * TensoRF-family code run on the host (alpha volume to the CPU, scipy.ndimage.label, a mask built by hand). All integer: every output is
 * a function of the input alone, two calls give bit-equal arrays. No float atomics, no host read inside the calls.
 *   volume         [n0][n1][n2] fp32, C order, n2 fastest (t2n_alpha_volume's layout). A voxel is foreground iff volume > level (strict:
 *                  NaN is background, +inf foreground).
 *   connectivity   6, 18 or 26: two foreground voxels are neighbours when their indices differ by at most one on every axis and on at
 *                  most 1, 2 or 3 axes (faces; plus edges; plus corners): scipy's generate_binary_structure(3, 1 | 2 | 3).
 *   labels         [n0][n1][n2] int32: -1 on background; on foreground dense, 0 .. K-1, numbered in the order of each component's
 *                  SMALLEST linear voxel index. `labels` is one fixed array for an input, not merely a partition.
 *   t2n_volume_components        fills labels and K (n_components_out: device int64 [1]). Block-based union-find: a workgroup owns a tile
 *                  (t2n_volume_components_tile: 4 x 8 x 64, the n2 extent one wave of 256 contiguous bytes), finds the runs along n2
 *                  with one ballot per row, unites the runs of neighbouring rows in an LDS parent array (atomicMin, larger root under
 *                  smaller) and writes every voxel's parent as the global linear index of its tile-local root. One thread per voxel on a
 *                  tile face then unites it with its foreground neighbours in other tiles (also those that share only an edge or a
 *                  corner) on the global parents, with the find / atomicMin discipline of t2n_mesh_components: parent[x] <= x only ever
 *                  decreases, so a component's final root is its smallest voxel whatever order the threads ran in. Then flatten,
 *                  exclusive scan of the root flags (per-256 sums, one workgroup with a running carry), labels = rank of the root.
 *                  With K = 0 only labels (all -1) and K are written.
 *   t2n_volume_component_stats   voxel_counts [K] int32 and, unless NULL, boxes [K][6] int32 (min0, min1, min2, max0, max1, max2:
 *                  inclusive index box); integer atomics, equal labels combined inside a wave first. K = 0 writes nothing.
 *   t2n_volume_filter            keep [K] uint8: volume_out = keep[label] ? volume : fill on foreground (label in [0, K)), volume_out =
 *                  volume elsewhere, bits preserved. volume_out may alias volume.
 * Workspace of t2n_volume_components: t2n_volume_components_workspace_bytes(n0, n1, n2) bytes of device memory (0 = bad argument).
 * T2N_ERR_INVALID (before any HIP call): NULL required pointer, a dimension < 1, n0 * n1 * n2 >= 2^31, a connectivity other than 6, 18
 * or 26, a level that is not finite, workspace_bytes smaller than required, n_components outside [0, n0 * n1 * n2]. */
size_t t2n_volume_components_workspace_bytes(int n0, int n1, int n2);
int t2n_volume_components_tile(int tile3[3]);
int t2n_volume_components(const float* volume, int n0, int n1, int n2, float level, int connectivity, int32_t* labels,
                          int64_t* n_components_out, void* workspace, size_t workspace_bytes, t2n_stream stream);
int t2n_volume_component_stats(const int32_t* labels, int n0, int n1, int n2, int64_t n_components, int32_t* voxel_counts,
                               int32_t* boxes_or_null, t2n_stream stream);
int t2n_volume_filter(const float* volume, const int32_t* labels, int n0, int n1, int n2, const uint8_t* keep, int64_t n_components,
                      float fill, float* volume_out, t2n_stream stream);

/* ---- One optimisation step of the reference's loop (text2nerf_main.py:547-601) as ONE submission: TV gradient -> train-mode render
 * (KEEP_CTX) -> t2n_train_loss -> t2n_render_backward (device-side row plan, as T2N_FLAG_DEVICE_ROWS) -> Adam on all 19 tensors ->
 * re-packed head operands, on the caller's stream and three library-owned side streams (forked from / joined into `stream` by events, so
 * the whole call can be captured into a hipGraph: t2n_train_graph_*). Nothing in it is read on the host and no kernel argument changes
 * from step to step: the batch comes through the caller's fixed device buffers, the per-step scalars (learning rates, TV weights) through
 * `hyper` in device memory, Adam's step count lives in the field (device memory; bias corrections are derived from it on the device).
 * Fused MLP_Fea_noview head (27 / 6 / 128), 16 + 48 components, fp32 factor storage, split-f16 head arithmetic, no NDC, no alpha mask:
 * anything else is T2N_ERR_UNSUPPORTED (use the separate calls).
 *   hyper          device float[T2N_TRAIN_HYPER_FLOATS]: [0..18] learning rates of the 19 tensors in t2n_field_params order, [19] / [20]
 *                  TV weights of the density / appearance planes (already x 1e-2: models/tensoRF.py:193-203), rest reserved
 *   params         the caller's reference-layout tensors: updated in place (like t2n_field_tv_adam_step / t2n_adam_step_multi)
 *   exp_avg(_sq)   Adam moments: [0..11] CHANNEL-LAST buffers of the factor tensors, [12..18] reference layout
 *   head_grads     device float[T2N_TRAIN_HEAD_GRAD_FLOATS]: the gradients of basis_mat and the six MLP tensors, contiguous, in
 *                  parameter order, followed by ONE vote word (a data-parallel caller all-reduces the whole buffer with the gradients;
 *                  the factor gradients are in the field's gradient buffer: t2n_field_set_grad_buffer)
 *   rows_capacity  appearance rows (multiple of 32) the workspace is sized for. A step that needs MORE applies NO update at all (every
 *                  optimiser kernel reads the verdict from device memory and returns; Adam's step count does not advance): the caller
 *                  learns it from t2n_field_train_record — without waiting — and submits the same batch again with a capacity >= the
 *                  recorded need.
 *   shard_world    > 1 selects the SHARDED OPTIMISER of a data-parallel group: of every plane's n / 64 whole 64-position
 *                  blocks, rank r owns blocks [r c, (r + 1) c), c = (n / 64) / world (the "body", world c blocks); the blocks behind the
 *                  body and the six lines are replicated (t2n_field_shard_layout gives the offsets). phases = 1 then seeds the gradient
 *                  buffer with world x the TV gradient on the blocks this rank owns, zero on the rest of the body and the plain TV
 *                  gradient on the replicated part: AVERAGING the ranks' buffers — a reduce-scatter of each body, one small all-reduce of
 *                  the replicated parts and head_grads — leaves every owner the full-batch gradient of its slice. phases = 2 steps the
 *                  owned and the replicated blocks only (1 / world of the TV + Adam traffic); the caller then all-gathers each body of
 *                  the channel-last parameter copies (t2n_field_factor_buffer) and a phases = 4 call writes the gathered blocks into its
 *                  reference-layout tensors. Moments of blocks a rank does not own are never touched.
 *   phases         1: render + loss + backward only (gradients left in the field's buffer and head_grads), 2: optimiser only (after a
 *                  data-parallel all-reduce of both; a non-zero vote word withholds the update on every rank), 3: both.
 *   losses         device float[4] = {mse, depth loss, transmittance loss, total} of the batch
 * host_batch: the call itself copies host_batch_bytes from pinned host memory to batch_buffer (asynchronously, ahead of everything that
 * reads the batch, with an engine copy). Pipelined form — an eager call with T2N_FLAG_PIPELINE, phases = 3, host_batch set and a workspace of TWICE
 * t2n_train_step_workspace_bytes: the copy and the step's early part (zero fills, the march — it reads the density factors only —, the
 * plan, the appearance binning) are enqueued on the library's side stream right behind the PREVIOUS step's density Adam instead of
 * behind `stream`, i.e. they run beside the previous step's appearance scatter / weight-gradient GEMMs / Adam. The two halves of the
 * workspace and two slots of per-step scalars alternate. The caller must not have touched the field (uploads, other optimiser steps)
 * between the two calls and must not reuse host_batch / batch_buffer before the call after next has been submitted; everything else
 * about the call (ordering of its results on `stream`, the record) is unchanged. head_grads is left ZEROED by the optimiser phase (and
 * must be zero when a phases = 1 | 3 call starts). The whole call uses three side streams (early part + TV seed + density scatter; layer
 * 2 + weight-gradient GEMMs + head step; none for the rest): with the caller's, one per hardware queue.
 * Replaces (reference): text2nerf_main.py:553-590 (renderer call, losses, TV terms, zero_grad / backward / step). */
#define T2N_TRAIN_HYPER_FLOATS 32
#define T2N_TRAIN_HEAD_GRAD_FLOATS (27 * 144 + 128 * 351 + 128 + 128 * 128 + 128 + 3 * 128 + 3 + 1)
typedef struct t2n_train_step_args {
    const float* rays; int64_t n_rays; int32_t ray_stride; int32_t n_samples;
    uint32_t flags;            /* T2N_FLAG_ADD_BG, T2N_FLAG_PIPELINE, T2N_FLAG_GATHER_BATCH or 0 (T2N_FLAG_TRAIN is implied) */
    uint32_t phases;           /* 1 | 2, or 4 alone (sharded optimiser: see shard_world) */
    const float* jitter; const float* rgb_target; const float* depth_target;
    float w_depth, w_trans, delta;
    float beta1, beta2, eps;
    const float* hyper;
    t2n_field_params params;
    float* exp_avg[19]; float* exp_avg_sq[19];
    float* head_grads;
    int64_t rows_capacity;
    void* workspace; size_t workspace_bytes;
    float* losses;
    const void* host_batch;    /* optional: the batch in PINNED host memory (NULL: the device buffers are already filled), see below */
    size_t host_batch_bytes;
    void* batch_buffer;        /* device destination of host_batch: the start of the ONE allocation rays / jitter / targets / hyper point into */
    int32_t shard_world, shard_rank;   /* sharded optimiser (data-parallel): ranks and this rank; 0 / 1 = every rank steps every factor */
} t2n_train_step_args;
size_t t2n_train_step_workspace_bytes(const t2n_field* f, int64_t n_rays, int n_samples, int64_t rows_capacity);
int t2n_train_step(t2n_field* f, const t2n_train_step_args* a, t2n_stream stream);
/* A training set that lives on the device, and a step that takes ROW INDICES (T2N_FLAG_GATHER_BATCH): the field remembers where the set
 * is (by value; NULL clears; host-only: no stream work, nothing is read here), and a flagged phases & 1 call fills its own batch —
 * a->rays (ray_stride must be 6), a->rgb_target, a->depth_target, destinations inside batch_buffer — from the rows ids[0..n_rays) as its
 * first device work: further rows of the step's zero-fill launch (no extra launch; a captured step keeps its DAG), on the stream the
 * early part runs on, behind the engine copy of host_batch,
 * which then covers ids | jitter | hyper only (2 n_rays + 32 words where the plain form sends 11 n_rays + 32). An id outside [0, n_rows) is clamped into range by the kernel: a caller error, never an
 * out-of-bounds read. The flag without a source: T2N_ERR_STATE; n_rows < 1 or ray_stride < 6: T2N_ERR_INVALID (both before anything is
 * enqueued). phases = 2 and phases = 4 calls ignore the flag. The source's rows must have been written on `stream` (or be complete) when
 * the step is submitted: the first gathering step after a source whose pointers or n_rows differ from the previous one orders its early
 * part behind `stream` even in the pipelined form; the caller keeps the source's memory alive until the step has run. A captured graph
 * freezes the source's pointers like every other: re-capture after a change. */
typedef struct t2n_train_source {
    const float* rays;  int32_t ray_stride;   /* [n_rows, ray_stride], ray_stride >= 6 (origin, direction first) */
    const float* rgb;                         /* [n_rows, 3] */
    const float* depth;                       /* [n_rows] */
    int64_t n_rows;
    const int32_t* ids;                       /* device, n_rays entries: normally inside batch_buffer, filled by the host_batch copy */
} t2n_train_source;
int t2n_field_set_train_source(t2n_field* f, const t2n_train_source* src);
/* The sharded optimiser's partition for `world` ranks: out[3 t + 0] = offset of factor tensor t in the field's gradient buffer (floats),
 * out[3 t + 1] = floats of ONE rank's slice of its body (0 for the lines), out[3 t + 2] = its floats in all; t = 0..11 in the order density
 * planes, density lines, appearance planes, appearance lines (channel-last: position-major, C = 16 / 48 floats per position). */
int t2n_field_shard_layout(const t2n_field* f, int world, int64_t out[36]);
/* Device pointer of the channel-last fp32 master copy of factor tensor t (the array the kernels read and the fused step's Adam updates). */
int t2n_field_factor_buffer(const t2n_field* f, int t, void** ptr);
/* Adam's step count of the field's fused steps (device memory): set when an optimiser state is loaded / reset. Asynchronous on `stream`. */
int t2n_field_train_set_step(t2n_field* f, uint32_t step, t2n_stream stream);
/* What the fused steps recorded, from pinned host memory (never waits, never touches a stream): out[0] = newest sequence number + 1 in
 * the ring (steps of the field are numbered from 0), out[1] = Adam steps applied, out[2] = steps withheld (both informational: written
 * without ordering); out[4 + 2 k], out[5 + 2 k], k = 0..15: the record of the step with (sequence number & 15) == k — the appearance rows
 * it NEEDED and its tag = (sequence number + 1) << 1 | withheld. A record is ONE 8-byte store: a slot whose tag carries another sequence
 * number has not been written for this step yet. */
int t2n_field_train_record(const t2n_field* f, uint32_t out[36]);
/* The same call captured ONCE into a hipGraph (stream capture of t2n_train_step on `stream`, the side streams included) and replayed:
 * every pointer and size in `a` is frozen — the caller refills the buffers behind them (batch, hyper) before each launch and
 * re-captures when a size (n_rays, n_samples, rows_capacity, workspace) or a pointer changes. t2n_train_step must have run eagerly once
 * with the same field (lazy stream / event / buffer creation cannot be captured). */
typedef struct t2n_train_graph t2n_train_graph;
int t2n_train_graph_capture(t2n_field* f, const t2n_train_step_args* a, t2n_stream stream, t2n_train_graph** out);
int t2n_train_graph_launch(t2n_train_graph* g, t2n_stream stream);
int t2n_train_graph_nodes(const t2n_train_graph* g);   /* kernel nodes of the captured step */
int t2n_train_graph_destroy(t2n_train_graph* g);

/* ---- measurement hooks (bench.py): when enabled, each kernel launch of the render call is bracketed by HIP events on
 * the launch stream. t2n_timing_read synchronises those events and returns accumulated milliseconds and launch counts
 * per kernel since the last reset (up to 1024 launches per kernel are timed between two reads; launches beyond that are counted and
 * priced at the timed average). Kernel ids: */
enum { T2N_K_MARCH = 0, T2N_K_SHADE = 1, T2N_K_COMPOSITE = 2, T2N_K_UPLOAD = 3, T2N_K_BWD_MARCH = 4, T2N_K_BWD_MLP = 5,
       T2N_K_BWD_SCATTER = 6, T2N_K_DENSITY = 7, T2N_K_APPFEAT = 8 /* appearance gather + basis_mat */,
       /* t2n_train_step only (its groups run side by side on four streams: each figure is the group's own start-to-end time under that
        * concurrency): weight-gradient GEMMs + their reduce; density binning + scatter; TV seed; Adam on the factors; head Adam + re-packs */
       T2N_K_BWD_WGRAD = 9, T2N_K_BWD_DENSITY = 10, T2N_K_TV_SEED = 11, T2N_K_ADAM = 12, T2N_K_HEAD_STEP = 13, T2N_K_COUNT = 14 };
int t2n_timing_enable(t2n_field* f, int on);   /* on: 0 off, 1 every kernel, else a mask: bit (k + 1) brackets kernel id k only */
int t2n_timing_read(t2n_field* f, double* ms /*[T2N_K_COUNT]*/, int64_t* launches /*[T2N_K_COUNT]*/, int reset);

#ifdef __cplusplus
}
#endif
#endif /* T2N_H_ */
