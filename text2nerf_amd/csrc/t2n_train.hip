// t2n_train_step: one optimisation step of text2nerf_main.py:547-601 as ONE submission (include/t2n.h). The kernels are those of
// t2n_render_forward (KEEP_CTX, train), t2n_train_loss, t2n_render_backward (T2N_FLAG_DEVICE_ROWS: the stage launchers of t2n_backward.h) and the
// optimiser entry points; what is new is the ORDER: every launch that does not lie on the step's dependency chain runs on a side stream
// beside it, and nothing about a step is decided on the host. Two side streams, the process-wide pair (ensure_side_streams):
//   s  (caller)  [setup -> march] -> shade (kept rows) -> composite -> bwd_march (with the loss) -> mlp_bwd_ss -> tile_accum -> Adam (appearance factors)
//   sa (side)    plan (rows, tile prefix, verdict, Adam scalars, host record) -> appearance binning (needs the forward's lists only) -> TV seed of the
//                gradient buffer (behind the march; + the L1 term, + the lines' ortho launches in a step that carries them) -> density scatter (behind bwd_march) -> Adam (density factors)
//   sg (gemm)    [early form: density scan] -> layer-2 gradients (behind bwd_march) -> weight-gradient GEMMs (behind mlp_bwd_ss) -> reduce + losses
//                -> Adam (head) -> operand re-packs
// [setup -> march]: on sa in the pipelined form (beside the previous step's tail), behind the engine copy of the host batch.
#include <stdlib.h>

#include "t2n_backward.h"

namespace t2n {

// zero fills of one step as ONE launch: region r = blockIdx.y (a uniform index into the kernel arguments)
constexpr int kZeroRegions = 12;
// T2N_FLAG_GATHER_BATCH: the batch rows of a device-resident training set, by index (one more grid row of the zero-fill launch)
struct GatherOps { const float* rays; const float* rgb; const float* depth; const int* ids; float* d_rays; float* d_rgb; float* d_depth;
    long long n_rows; unsigned n; int stride; int vec; };
struct ZeroOps { unsigned* ptr[kZeroRegions]; unsigned long long words[kZeroRegions]; int n = 0;
    int g_row = -1; GatherOps g = {};   // optional gather (grid row g_row = n, behind the zero fills)
    bool add(void* p, size_t bytes) { if (!p || !bytes) return true; if (n >= kZeroRegions) return false; ptr[n] = (unsigned*)p; words[n] = (bytes + 3) / 4; ++n; return true; } };
__global__ __launch_bounds__(256) void k_zero_regions(const ZeroOps o) {
    const int r = blockIdx.y;
    if (r == o.g_row) {   // one thread per batch row: rays[id] (24 B, three 8-byte loads when source and destination allow), rgbs[id], depths[id]
        const GatherOps& g = o.g;
        for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < g.n; i += gridDim.x * 256u) {
            long long id = g.ids[i];
            id = id < 0 ? 0 : (id >= g.n_rows ? g.n_rows - 1 : id);     // (memory safety does not depend on the caller)
            const float* __restrict__ sr = g.rays + id * g.stride;
            float* __restrict__ dr = g.d_rays + (size_t)i * 6;
            if (g.vec) {
                const float2 a = reinterpret_cast<const float2*>(sr)[0], b = reinterpret_cast<const float2*>(sr)[1], c = reinterpret_cast<const float2*>(sr)[2];
                reinterpret_cast<float2*>(dr)[0] = a; reinterpret_cast<float2*>(dr)[1] = b; reinterpret_cast<float2*>(dr)[2] = c;
            } else {
                const float a0 = sr[0], a1 = sr[1], a2 = sr[2], a3 = sr[3], a4 = sr[4], a5 = sr[5];
                dr[0] = a0; dr[1] = a1; dr[2] = a2; dr[3] = a3; dr[4] = a4; dr[5] = a5;
            }
            const float* __restrict__ sc = g.rgb + id * 3;
            const float c0 = sc[0], c1 = sc[1], c2 = sc[2];
            float* __restrict__ dc = g.d_rgb + (size_t)i * 3;
            dc[0] = c0; dc[1] = c1; dc[2] = c2;
            g.d_depth[i] = g.depth[id];
        }
        return;
    }
    unsigned* __restrict__ p = o.ptr[r];
    const unsigned long long n = o.words[r];
    if ((((uintptr_t)p) & 15u) == 0) {
        uint4* __restrict__ p4 = reinterpret_cast<uint4*>(p);
        const unsigned long long n4 = n / 4;
        for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (unsigned long long)gridDim.x * 256) p4[i] = make_uint4(0u, 0u, 0u, 0u);
        for (unsigned long long i = n4 * 4 + (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) p[i] = 0u;
    } else {
        for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) p[i] = 0u;
    }
}

// The plan of a fused step (one wave, right behind the forward's march): k_bwd_plan's tile prefix / row count / overflow from the
// sub-list counters (plan_prefix), and with them the step's VERDICT — a step whose rows exceed the capacity applies no update — Adam's step count and
// this step's bias-corrected scalars (torch.optim.Adam: step_size = lr / (1 - beta1^t), denom = sqrt(v) / sqrt(1 - beta2^t) + eps, in
// double like the host entry points), the vote word behind the head gradients and the record in pinned host memory.
__global__ __launch_bounds__(64) void k_train_plan(const unsigned* __restrict__ counters, unsigned list_cap, unsigned rows_cap, BwdPlan* __restrict__ plan,
                                                   TrainState* __restrict__ st, const float* __restrict__ hyper, float beta1, float beta2, float* vote,
                                                   unsigned* host_rec, unsigned slot) {
    TrainScalars* __restrict__ sc = &st->sc[slot];
    const int lane = threadIdx.x;
    unsigned ovf;
    const unsigned rows = plan_prefix(counters, list_cap, rows_cap, true, plan, ovf);
    const unsigned step = st->step + (ovf ? 0u : 1u);     // (every lane reads the old value; lane 0 writes below)
    if (lane < 19 && !ovf) {
        const double bc1 = 1.0 - pow((double)beta1, (double)step);
        sc->lr_over_bc1[lane] = (float)((double)hyper[lane] / bc1);
        if (lane == 0) sc->inv_bc2_sqrt = (float)(1.0 / sqrt(1.0 - pow((double)beta2, (double)step)));
    }
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
        const unsigned seq = st->seq;
        st->seq = seq + 1u;
        sc->skip = ovf;
        st->step = step;
        if (ovf) st->skipped = st->skipped + 1u;
        if (vote) *vote = ovf ? 1.f : 0.f;
        if (host_rec) {
            // ONE 8-byte store per record into fine-grained pinned memory: {rows needed, (sequence + 1) << 1 | withheld}. No fence: a
            // system-scope release writes the L2 back (60 us behind the march's 50 MB of output), and the host needs no ordering between
            // records — an entry whose sequence number is not the one it waits for has simply not arrived yet
            volatile unsigned long long* h = reinterpret_cast<volatile unsigned long long*>(host_rec);
            h[2 + (seq & 15u)] = ((unsigned long long)(((seq + 1u) << 1) | ovf) << 32) | rows;
            host_rec[1] = step; host_rec[2] = st->skipped;
        }
    }
}
// Data-parallel steps (phases 1 | all-reduce | 2): the vote word came back from the all-reduce of the head gradients. A rank whose own
// rows fitted but whose peers' did not withholds its update too: the optimistic count of k_train_plan is taken back.
__global__ __launch_bounds__(64) void k_train_commit(TrainState* __restrict__ st, const float* __restrict__ vote, unsigned* host_rec, unsigned slot) {
    if (threadIdx.x != 0) return;
    if (*vote != 0.f && !st->sc[slot].skip) {
        st->sc[slot].skip = 1u; st->step = st->step - 1u; st->skipped = st->skipped + 1u;
        if (host_rec) {
            volatile unsigned long long* h = reinterpret_cast<volatile unsigned long long*>(host_rec);
            const unsigned seq = st->seq - 1u;
            h[2 + (seq & 15u)] = h[2 + (seq & 15u)] | (1ull << 32);
            host_rec[1] = st->step; host_rec[2] = st->skipped;
        }
    }
}
__global__ __launch_bounds__(64) void k_train_set_step(TrainState* st, unsigned step, unsigned* host_rec) {
    if (threadIdx.x == 0) { st->step = step; if (host_rec) ((volatile unsigned*)host_rec)[1] = step; }
}

struct TrainCarve { size_t fwd, fwd_bytes, bwd, bwd_bytes, g1, rgb, depth, part, total; };
static TrainCarve train_carve(const t2n_field* f, int64_t R, int N, int64_t rows) {
    TrainCarve t;
    const BinGeom geom = bin_geom(f->dev.den);
    const BlockGeom bg = block_geom(f->dev.den);
    size_t o = 0;
    const Carve c = carve_workspace(R, N, true, false);
    t.fwd = o; t.fwd_bytes = al256(c.total) + (size_t)rows * (144 + 32 + 128 + 128) * 4; o = al256(o + t.fwd_bytes);
    t.bwd = o; t.bwd_bytes = bwd_carve(rows, R, N, geom.total, bg.total * bg.copies, 351, true).total; o = al256(o + t.bwd_bytes);
    t.g1 = o; o = al256(o + (size_t)rows * 128 * 4);
    t.rgb = o; o = al256(o + (size_t)R * 12);
    t.depth = o; o = al256(o + (size_t)R * 4);
    t.part = o; o = al256(o + (size_t)((R + 3) / 4) * 12);
    t.total = o;
    return t;
}
static size_t train_dev_bytes() { return 256 + al256(mlp_bwd_ss_pack_bytes()); }
static bool train_supported(const t2n_field* f) {
    return f->desc.shading == T2N_SHADE_MLP_FEA_NOVIEW && f->desc.app_dim == 27 && f->dev.app.C == 48 && f->dev.den.C == 16 && f->mlp_split &&
           !f->factor_bf16 && !f->dev.alpha && block_geom_ok(f->dev.den);
}
static int train_ensure(t2n_field* f, hipStream_t s) {
    if (!f->train_dev) {
        T2N_HIP(hipMalloc(&f->train_dev, train_dev_bytes()));
        T2N_HIP(hipMemsetAsync(f->train_dev, 0, 256, s));
        T2N_HIP(hipHostMalloc((void**)&f->train_host, 64 * sizeof(unsigned), hipHostMallocDefault));
        for (int i = 0; i < 64; ++i) f->train_host[i] = 0u;
        f->train_packed = false;
    }
    return ensure_side_streams(f);
}
// the backward chain's transposed split-f16 operands + the forward's packed head operands from the CURRENT head weights
// (the forward pack reads every weight anyway: it leaves the four matrices' largest magnitudes in the chain pack's absmax words — zeroed
// by the head Adam launch in front of it — so the chain pack is one short launch; a pack kernel that scanned the matrices itself took
// 60-105 us at the end of the step's longest chain)
static int train_repack(t2n_field* f, const t2n_field_params* p, hipStream_t s) {
    int rc;
    void* gpack = (char*)f->train_dev + 256;
    if ((rc = launch_pack_mlp(f, p, s, (unsigned*)mlp_bwd_ss_absmax_words(gpack)))) return rc;
    if ((rc = mlp_bwd_ss_pack(f, gpack, s, true, false, true))) return rc;
    f->train_packed = true;
    return T2N_OK;
}

}  // namespace t2n

using namespace t2n;

extern "C" size_t t2n_train_step_workspace_bytes(const t2n_field* f, int64_t n_rays, int n_samples, int64_t rows_capacity) {
    if (!f || n_rays <= 0 || n_samples <= 0 || rows_capacity < 32) return 0;
    return train_carve(f, n_rays, n_samples, rows_capacity / 32 * 32).total;
}

extern "C" int t2n_field_train_set_step(t2n_field* f, uint32_t step, t2n_stream stream) {
    if (!f) { set_error("t2n_field_train_set_step: NULL field"); return T2N_ERR_INVALID; }
    int rc;
    if ((rc = train_ensure(f, (hipStream_t)stream))) return rc;
    hipLaunchKernelGGL(k_train_set_step, dim3(1), dim3(64), 0, (hipStream_t)stream, (TrainState*)f->train_dev, (unsigned)step, f->train_host);
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

extern "C" int t2n_field_set_train_source(t2n_field* f, const t2n_train_source* src) {
    if (!f) { set_error("t2n_field_set_train_source: NULL field"); return T2N_ERR_INVALID; }
    if (!src) { f->train_src = t2n_train_source{}; f->train_src_set = false; f->train_src_fresh = false; return T2N_OK; }
    if (src->n_rows < 1 || src->ray_stride < 6 || !src->rays || !src->rgb || !src->depth || !src->ids) {
        set_error("t2n_field_set_train_source: n_rows %lld (>= 1), ray_stride %d (>= 6) or a NULL pointer", (long long)src->n_rows, src->ray_stride);
        return T2N_ERR_INVALID;
    }
    const t2n_train_source& o = f->train_src;
    if (!f->train_src_set || o.rays != src->rays || o.rgb != src->rgb || o.depth != src->depth || o.n_rows != src->n_rows || o.ray_stride != src->ray_stride)
        f->train_src_fresh = true;
    f->train_src = *src; f->train_src_set = true;
    return T2N_OK;
}

extern "C" int t2n_field_train_record(const t2n_field* f, uint32_t out[36]) {
    if (!f || !out) { set_error("t2n_field_train_record: NULL argument"); return T2N_ERR_INVALID; }
    if (!f->train_host) { for (int i = 0; i < 36; ++i) out[i] = 0u; return T2N_OK; }
    // pinned layout: words 1, 2 = steps applied / withheld (informational: written without ordering), then 16 eight-byte records
    // {rows needed, (sequence + 1) << 1 | withheld} at sequence & 15. out[0] = number of consecutive records present from the field's
    // first step on, i.e. records of sequence numbers < out[0] have all landed (the host keeps its own count of what it consumed).
    const volatile unsigned long long* h = reinterpret_cast<const volatile unsigned long long*>(f->train_host);
    out[1] = f->train_host[1]; out[2] = f->train_host[2]; out[3] = 0u;
    unsigned newest = 0u;
    for (int k = 0; k < 16; ++k) {
        const unsigned long long e = h[2 + k];
        const unsigned tag = (unsigned)(e >> 32);
        out[4 + 2 * k] = (unsigned)e;           // rows needed
        out[5 + 2 * k] = tag;                   // (sequence + 1) << 1 | withheld; 0 = never written
        if ((tag >> 1) > newest) newest = tag >> 1;
    }
    out[0] = newest;   // newest sequence number + 1 seen in the ring (records arrive in order: one plan kernel after the other)
    return T2N_OK;
}

extern "C" int t2n_train_step(t2n_field* f, const t2n_train_step_args* A, t2n_stream stream) {
    if (!f || !A || !A->rays || !A->jitter || !A->rgb_target || !A->depth_target || !A->hyper || !A->head_grads || !A->workspace || !A->losses ||
        A->n_rays <= 0 || A->ray_stride < 6 || A->n_samples <= 0 || !(A->phases & 7u) || ((A->phases & 4u) && A->phases != 4u)) {
        set_error("t2n_train_step: bad argument");
        return T2N_ERR_INVALID;
    }
    const int sworld = A->shard_world > 1 ? A->shard_world : 1, srank = A->shard_world > 1 ? A->shard_rank : 0;
    if (srank < 0 || srank >= sworld || (sworld > 1 && (A->phases & 3u) == 3u)) {
        set_error("t2n_train_step: shard_rank %d of %d, or a sharded step as one call (the gradient exchange lies between phases 1 and 2)", A->shard_rank, A->shard_world);
        return T2N_ERR_INVALID;
    }
    // the L1 / ortho regularisers (hyper[21..24]; the flags say which the caller set): single rank only — the sharded seed scales the TV term
    // per owner and knows nothing of these; refused rather than dropped
    const bool reg_l1 = (A->flags & T2N_FLAG_REG_L1) != 0, reg_ortho = (A->flags & T2N_FLAG_REG_ORTHO) != 0;
    if (sworld > 1 && (reg_l1 || reg_ortho)) {
        set_error("t2n_train_step: the L1 / ortho regularisers (T2N_FLAG_REG_L1 / T2N_FLAG_REG_ORTHO) are not implemented for the sharded optimiser (shard_world %d)", sworld);
        return T2N_ERR_UNSUPPORTED;
    }
    if (A->phases == 4u) {   // sharded optimiser: the gathered body blocks of the other ranks -> the caller's reference-layout tensors
        if (!f->uploaded || !train_supported(f)) { set_error("t2n_train_step: phases = 4 needs an uploaded field of the fused step's shape"); return T2N_ERR_STATE; }
        if (sworld < 2) return T2N_OK;
        return launch_factor_adam_dev(f, &A->params, nullptr, nullptr, 0.f, 0.f, 0.f, nullptr, 0, 12, (hipStream_t)stream, sworld, srank, true);
    }
    if (!f->uploaded) { set_error("t2n_train_step: field has no uploaded parameters"); return T2N_ERR_STATE; }
    if (!train_supported(f)) {
        set_error("t2n_train_step: needs the fused MLP_Fea_noview head (27 / 6 / 128) in split-f16 mode, 16 + 48 components, fp32 factor storage, no alpha mask");
        return T2N_ERR_UNSUPPORTED;
    }
    const int64_t R = A->n_rays;
    const int N = A->n_samples;
    const int64_t rows = A->rows_capacity / 32 * 32;
    if (N > 1024 || rows < 32 || (uint64_t)R * N * 3 >= 0x7fffffffull || (uint64_t)list_capacity(R, N) * kLists > 0x7fffffffull) {
        set_error("t2n_train_step: n_samples %d (<= 1024), rows_capacity %lld (>= 32) or n_rays x n_samples out of range", N, (long long)A->rows_capacity);
        return T2N_ERR_UNSUPPORTED;
    }
    if (!binned_scatter_ok(f, R, N)) { set_error("t2n_train_step: needs the binned scatters (grid lines within their LDS budget, T2N_BWD_ATOMIC_SCATTER not set)"); return T2N_ERR_UNSUPPORTED; }
    const TrainCarve T = train_carve(f, R, N, rows);
    if (T.total > A->workspace_bytes) { set_error("t2n_train_step: workspace %zu B < %zu B", A->workspace_bytes, T.total); return T2N_ERR_WORKSPACE; }
    if (!f->gbuf_all) { set_error("t2n_train_step: the field has no gradient buffer (t2n_field_set_grad_buffer)"); return T2N_ERR_STATE; }
    // T2N_FLAG_GATHER_BATCH: refused before anything is enqueued
    const bool gather = (A->flags & T2N_FLAG_GATHER_BATCH) && (A->phases & 1u);
    if (gather) {
        if (!f->train_src_set) { set_error("t2n_train_step: T2N_FLAG_GATHER_BATCH without a training source (t2n_field_set_train_source)"); return T2N_ERR_STATE; }
        const t2n_train_source& S = f->train_src;
        if (S.n_rows < 1 || S.ray_stride < 6 || !S.rays || !S.rgb || !S.depth || !S.ids) { set_error("t2n_train_step: training source with n_rows %lld, ray_stride %d or a NULL pointer", (long long)S.n_rows, S.ray_stride); return T2N_ERR_INVALID; }
        if (A->ray_stride != 6) { set_error("t2n_train_step: T2N_FLAG_GATHER_BATCH fills a batch of ray_stride 6 (got %d)", A->ray_stride); return T2N_ERR_INVALID; }
    }
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = train_ensure(f, s))) return rc;
    // two streams beside the caller's (one per hardware queue): sa = early part + plan + binning + TV seed + density scatter / Adam, sg =
    // layer 2 + weight-gradient GEMMs + head step. (With separate streams for the plan / binning, the early part and the caller's batch
    // copy, seven streams shared four queues: whichever chain landed behind the GEMM chain's queue waited for it — 0.86 or 0.99 ms per
    // step depending on the order the streams had been created in.)
    hipStream_t sa = (hipStream_t)f->side_stream, sg = (hipStream_t)f->gemm_stream;
    hipEvent_t* ev = (hipEvent_t*)f->train_ev;   // 0 begin, 1 seed, 2 march, 3 plan, 4 appbin, 5 bwd_march, 6 chain, 7 gemm-stream join, 9 density Adam, 10 early bins, 11 density scan
    TrainState* st = (TrainState*)f->train_dev;
    void* gpack = (char*)f->train_dev + 256;
    float* vote = A->head_grads + (T2N_TRAIN_HEAD_GRAD_FLOATS - 1);
    const bool do_grad = (A->phases & 1u) != 0, do_opt = (A->phases & 2u) != 0;
    // pipelined form: the early part of this step on `se`, beside the previous step's tail (see include/t2n.h)
    // density bins counted from the forward's windows, beside the shade kernel, instead of behind the backward march (as t2n_render_backward
    // does): takes ~110 us of small kernels off the chain backward march -> density scatter -> density Adam -> next march, at the price of
    // records for zero-gradient samples and a second evaluation of the sample positions. Small batches are bound by that chain (2 048 rays:
    // 0.404 -> 0.392 ms; 8 192 rays: 0.575 -> 0.564), large ones by the machine's throughput (16 384 rays: 0.851 -> 0.857, later 0.829 / 0.845 ->
    // 0.838 / 0.826: nothing either way): taken up to 4 096 rays (the configuration every record of the round ran)
    // (T2N_DEN_EARLY=0 / 1 forces it; profiles/round6_train_ab.txt)
    static const int den_env = getenv("T2N_DEN_EARLY") ? atoi(getenv("T2N_DEN_EARLY")) : -1;
    bool den_early = den_env >= 0 ? den_env != 0 : A->n_rays <= 4096;
    hipStreamCaptureStatus cap_status = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(s, &cap_status);
    if (cap_status != hipStreamCaptureStatusNone && (reg_l1 || reg_ortho)) {
        set_error("t2n_train_step: the L1 / ortho regularisers (T2N_FLAG_REG_L1 / T2N_FLAG_REG_ORTHO) are not part of the captured step");
        return T2N_ERR_UNSUPPORTED;
    }
    if (cap_status != hipStreamCaptureStatusNone) den_early = false;   // (the captured step keeps the one DAG its replay was tested with: the early form's extra fork crashed hipStreamEndCapture on ROCm 7.2)
    const bool pipe = (A->flags & T2N_FLAG_PIPELINE) && A->host_batch && do_grad && do_opt && A->workspace_bytes >= 2 * T.total && cap_status == hipStreamCaptureStatusNone;
    const bool chain_prev = f->train_chain;               // the previous call was a full step of this form and left its density-Adam event
    f->train_chain = false;
    const unsigned par = f->train_calls & 1u;            // scalar slot (always alternates) and, pipelined, workspace half
    if (do_grad) f->train_calls++;
    const unsigned slot = do_grad ? par : ((f->train_calls - 1u) & 1u);   // an optimiser-only call takes the slot its gradient call wrote
    TrainScalars* sc = &st->sc[slot];
    hipStream_t se = pipe ? sa : s;     // (on sa the early part is ordered behind the previous step's density Adam by the stream itself)
    // the caller's tensors are the parameters from here on (the optimiser writes them; the packs read them)
    const t2n_field_params* P = &A->params;
    if (do_opt && (!P->basis_weight || !P->mlp_w0 || !P->mlp_b0 || !P->mlp_w1 || !P->mlp_b1 || !P->mlp_w2 || !P->mlp_b2)) { set_error("t2n_train_step: NULL head tensor"); return T2N_ERR_INVALID; }

    char* ws = (char*)A->workspace + (pipe ? (size_t)par * T.total : 0);
    char* fw = ws + T.fwd;
    char* bw = ws + T.bwd;
    const Carve c = carve_workspace(R, N, true, false);
    const KeptRows kr = kept_rows(c.total, T.fwd_bytes);
    if ((int64_t)kr.rows < rows) { set_error("t2n_train_step: internal carve mismatch (%u kept rows < %lld)", kr.rows, (long long)rows); return T2N_ERR_WORKSPACE; }
    const BinGeom ageom = bin_geom(f->dev.app);
    const BlockGeom bgeom = block_geom(f->dev.den);
    const BwdCarve b = bwd_carve(rows, R, N, bin_geom(f->dev.den).total, bgeom.total * bgeom.copies, 351, true);
    float* rgb = (float*)(ws + T.rgb); float* depth = (float*)(ws + T.depth);
    const uint32_t flags = (A->flags & T2N_FLAG_ADD_BG) | T2N_FLAG_TRAIN | T2N_FLAG_KEEP_CTX;

    if (do_grad) {
        if (!f->train_packed) {   // first step / after an upload: the operands an optimiser phase leaves packed behind every later step
            if ((rc = mlp_bwd_ss_pack(f, gpack, s, false, true))) return rc;
            f->train_packed = true;
        }
        T2N_HIP(hipEventRecord(ev[0], s));
        // (the previous call left no density-Adam event on sa: behind `stream`; so is the first gather from a training source that changed —
        // its rows were written on the caller's stream)
        if (pipe && (!chain_prev || (gather && f->train_src_fresh))) T2N_HIP(hipStreamWaitEvent(se, ev[0], 0));
        if (gather) f->train_src_fresh = false;
        if (A->host_batch) {   // the batch goes through the copy engine (a gathering step's gather row reads the ids this copy writes)
            if (!A->batch_buffer || !A->host_batch_bytes) { set_error("t2n_train_step: host_batch without batch_buffer / host_batch_bytes"); return T2N_ERR_INVALID; }
            T2N_HIP(hipMemcpyAsync(A->batch_buffer, A->host_batch, A->host_batch_bytes, hipMemcpyHostToDevice, se));
        }
        // ---- every zero fill of the step in one launch
        RenderLaunch L;
        L.rays = A->rays; L.n_rays = R; L.ray_stride = A->ray_stride; L.n_samples = N; L.flags = flags; L.jitter = A->jitter;
        L.rgb = rgb; L.depth = depth; L.weights = nullptr; L.z_vals = nullptr; L.stats = nullptr;   // (weights / sample depths: recomputed where they are needed)
        L.counters = (unsigned*)(fw + c.counters); L.acc = (float*)(fw + c.acc); L.ray_app = (int4*)(fw + c.ray_app);
        L.app_pos = (float4*)(fw + c.app_pos); L.app_rgb = (float4*)(fw + c.app_rgb); L.app_ray = (int*)(fw + c.app_ray);
        L.list_cap = c.list_cap; L.feat = nullptr; L.feat_rows = 0;
        L.sigma_ctx = (float*)(fw + c.sigma); L.rgb_raw = (float4*)(fw + c.rgb_raw);
        float4* go = (float4*)(bw + b.go);
        {
            ZeroOps zo;
            bool ok = zo.add(L.counters, (size_t)kLists * kCounterStride * 4);
            ok = ok && zo.add(go, (size_t)rows * 16);
            ok = ok && zo.add(bw + b.hist, (size_t)bgeom.total * bgeom.copies * 4);
            ok = ok && zo.add(bw + b.a_hist, (size_t)ageom.total * kBinCopies * 4);
            // (head_grads: left zeroed by the previous optimiser phase — its Adam kernel clears what it consumed; a pipelined early part
            // must not clear a buffer the previous step's head Adam has yet to read)
            if (!ok) { set_error("t2n_train_step: zero-fill table overflow"); return T2N_ERR_INVALID; }
            unsigned long long mx = 1;
            for (int r = 0; r < zo.n; ++r) mx = zo.words[r] > mx ? zo.words[r] : mx;
            if (gather) {   // behind the copy of ids | jitter | hyper on the same stream; device memory only
                const t2n_train_source& S = f->train_src;
                zo.g_row = zo.n;
                zo.g = GatherOps{S.rays, S.rgb, S.depth, (const int*)S.ids, const_cast<float*>(A->rays), const_cast<float*>(A->rgb_target), const_cast<float*>(A->depth_target),
                                 (long long)S.n_rows, (unsigned)R, (int)S.ray_stride,
                                 (((uintptr_t)S.rays | (uintptr_t)A->rays) & 7u) == 0 && (S.ray_stride & 1) == 0 ? 1 : 0};
                mx = (unsigned long long)R * 16 > mx ? (unsigned long long)R * 16 : mx;   // (one thread per batch row up to 256 workgroups)
            }
            unsigned bx = (unsigned)((mx + 4095) / 4096);
            bx = bx > 256 ? 256 : (bx < 1 ? 1 : bx);
            hipLaunchKernelGGL(k_zero_regions, dim3(bx, (unsigned)zo.n + (gather ? 1u : 0u)), dim3(256), 0, se, zo);
        }
        // ---- forward: march
        if ((rc = launch_march(f, L, se))) return rc;
        T2N_HIP(hipEventRecord(ev[2], se));
        if (pipe) T2N_HIP(hipStreamWaitEvent(s, ev[2], 0));
        // ---- forward: shade with the activation rows kept, composite; the driver's loss
        {
            ShadeCtx ctx{(float*)(fw + kr.x144), (float*)(fw + kr.feat32), (float*)(fw + kr.h0), (float*)(fw + kr.h1)};
            if ((rc = launch_shade_list(f, L.app_pos, L.app_ray, L.rays, A->ray_stride, L.counters, L.list_cap, L.app_rgb, &ctx, s, false, kr.rows))) return rc;
        }
        if ((rc = launch_composite(f, L, s))) return rc;
        // (the driver's loss is evaluated by k_bwd_march<.., LOSS>; its partial sums are added up by the step's one reduce launch)
        // ---- sa: plan, then the appearance binning (needs the forward's lists and the plan, not a single gradient)
        T2N_HIP(hipStreamWaitEvent(sa, ev[2], 0));
        BwdPlan* plan = (BwdPlan*)(bw + b.plan);
        hipLaunchKernelGGL(k_train_plan, dim3(1), dim3(64), 0, sa, (const unsigned*)L.counters, c.list_cap, (unsigned)rows, plan, st, A->hyper,
                           A->beta1, A->beta2, vote, f->train_host, slot);
        T2N_HIP(hipEventRecord(ev[3], sa));
        // (the tile prefix and the row count of every stage come from the plan: the host's prefix stays zero)
        const BwdCall call{f, A->rays, R, A->ray_stride, N, A->jitter, flags, fw, c, bw, b, TilePrefix{}, plan, rows};
        float* GX = (float*)(bw + b.xpe) + (size_t)rows * 160;
        if ((rc = launch_app_count(call, den_early, sa))) return rc;
        if (den_early) {
            // + the density scatter's block histogram from the forward's windows (positions only, no gradient needed); its reduce + scan
            // run on sg while the shade kernel runs: behind the backward march only the record pass and the accumulate pass are left
            // on the density chain (k_bin_reduce + k_bin_scan took ~110 us there under the concurrency of the input-gradient chain)
            if ((rc = fork_stream(sa, sg, ev[10])) || (rc = launch_den_scan(call, sg))) return rc;
            T2N_HIP(hipEventRecord(ev[11], sg));
        }
        if ((rc = launch_app_records(call, true, sa))) return rc;
        T2N_HIP(hipEventRecord(ev[4], sa));
        // ---- sa: the gradient buffer starts as the TV gradient of the current factors (zero where no weight is set): 140 MB of streaming
        // beside the shade kernel (matrix cores + LDS) rather than beside the march (gathers: the two slow each other by a third)
        T2N_HIP(hipStreamWaitEvent(sa, ev[0], 0));     // (behind the previous step's Adam: it read this buffer and wrote the factors)
        T2N_HIP(hipStreamWaitEvent(sa, ev[2], 0));
        timing_begin(f, T2N_K_TV_SEED, sa);
        if ((rc = launch_tv_seed_dev(f, A->hyper + 19, sa, sworld, srank, reg_l1))) return rc;
        timing_end(f, T2N_K_TV_SEED, sa);
        // the ortho term of the six lines, added directly behind the seed (Gram, gradient: two launches, only in a step that carries the term)
        if (reg_ortho && (rc = launch_ortho_lines(f, 0.f, 0.f, A->hyper + 23, sa))) return rc;
        T2N_HIP(hipEventRecord(ev[1], sa));
        // ---- backward: per-ray pass
        float* x144 = (float*)(fw + kr.x144); float* feat32 = (float*)(fw + kr.feat32); float* h0 = (float*)(fw + kr.h0); float* h1 = (float*)(fw + kr.h1);
        float* part = (float*)(bw + b.part);
        float* xpe = (float*)(bw + b.xpe);
        float* G0 = xpe; float* GF = xpe + (size_t)rows * 128;
        float* G1 = (float*)(ws + T.g1);
        const unsigned* rows_dev = &plan->rows;
        T2N_HIP(hipStreamWaitEvent(s, ev[3], 0));
        {
            const BwdLoss loss{rgb, depth, A->rgb_target, A->depth_target, A->w_depth, A->w_trans, A->delta, (float*)(ws + T.part)};
            timing_begin(f, T2N_K_BWD_MARCH, s);
            if ((rc = launch_bwd_march(call, true, nullptr, nullptr, nullptr, s, &loss, !den_early))) return rc;
            timing_end(f, T2N_K_BWD_MARCH, s);
            T2N_HIP(hipEventRecord(ev[5], s));
        }
        float* hg = A->head_grads;   // basis | w0 | b0 | w1 | b1 | w2 | b2
        float* g_basis = hg; float* g_w0 = g_basis + 27 * 144; float* g_b0 = g_w0 + 128 * 351; float* g_w1 = g_b0 + 128; float* g_b1 = g_w1 + 128 * 128;
        float* g_w2 = g_b1 + 128; float* g_b2 = g_w2 + 3 * 128;
        // ---- the input-gradient chain
        timing_begin(f, T2N_K_BWD_MLP, s);
        if ((rc = launch_mlp_bwd_ss(f, gpack, (const float4*)go, h1, h0, feat32, G0, GF, GX, rows, s, true, rows_dev, G1))) return rc;
        timing_end(f, T2N_K_BWD_MLP, s);
        T2N_HIP(hipEventRecord(ev[6], s));
        // ---- sa: density scatter (behind the TV seed on the same stream)
        T2N_HIP(hipStreamWaitEvent(sa, ev[5], 0));
        timing_begin(f, T2N_K_BWD_DENSITY, sa);
        if (den_early) T2N_HIP(hipStreamWaitEvent(sa, ev[11], 0));     // counted, reduced and scanned on sg beside the shade kernel
        else if ((rc = launch_den_scan(call, sa))) return rc;
        if ((rc = launch_den_scatter(call, den_early, sa))) return rc;
        timing_end(f, T2N_K_BWD_DENSITY, sa);
        T2N_HIP(hipEventRecord((hipEvent_t)f->ev_den, sa));
        // ---- sg: layer 2's weight gradient needs go and the kept h1 only (the chain writes g1 elsewhere in this form)
        T2N_HIP(hipStreamWaitEvent(sg, ev[5], 0));
        const WgradRegions WR = wgrad_regions(rows, 351);
        launch_bwd_l2((const float4*)go, (const float*)h1, rows, f->params_ref.mlp_w2, nullptr, nullptr, nullptr, (float*)((char*)part + WR.l2), sg, rows_dev);
        T2N_HIP(hipStreamWaitEvent(sg, ev[6], 0));
        timing_begin(f, T2N_K_BWD_WGRAD, sg);
        launch_gemm_tn(4, false, G1, 128, h0, 128, rows, 128, 128, g_w1, 128, (float*)((char*)part + WR.tn[0]), sg, nullptr, g_b1, rows_dev, false);
        launch_gemm_tn(4, false, G0, 128, xpe, 352, rows, 128, 351, g_w0, 351, (float*)((char*)part + WR.tn[1]), sg, feat32, g_b0, rows_dev, false);
        launch_gemm_tn(1, false, GF, 32, x144, 144, rows, 27, 144, g_basis, 144, (float*)((char*)part + WR.tn[2]), sg, nullptr, nullptr, rows_dev, false);
        launch_wgrad_reduce((const char*)part, rows, g_w2, g_b2, g_w1, g_w0, g_basis, sg, (const float*)(ws + T.part), R, A->w_depth, A->w_trans, A->losses);
        timing_end(f, T2N_K_BWD_WGRAD, sg);
        // ---- appearance scatter: records binned and gradient buffer seeded on sa
        T2N_HIP(hipStreamWaitEvent(s, ev[4], 0));
        T2N_HIP(hipStreamWaitEvent(s, ev[1], 0));
        timing_begin(f, T2N_K_BWD_SCATTER, s);
        if ((rc = launch_app_accum(call, GX, true, s))) return rc;
        timing_end(f, T2N_K_BWD_SCATTER, s);
        T2N_HIP(hipGetLastError());
        if (!do_opt) {   // gradients final on `s`: join both side chains
            T2N_HIP(hipEventRecord(ev[7], sg));
            T2N_HIP(hipStreamWaitEvent(s, ev[7], 0));
            T2N_HIP(hipStreamWaitEvent(s, (hipEvent_t)f->ev_den, 0));
            return T2N_OK;
        }
    } else {
        // optimiser-only phase (data-parallel): the vote word has been all-reduced with the head gradients
        hipLaunchKernelGGL(k_train_commit, dim3(1), dim3(64), 0, s, st, (const float*)vote, f->train_host, slot);
        if ((rc = fork_stream(s, sg, ev[6]))) return rc;
    }
    // ---- optimiser. sg: Adam on the seven head tensors, then every packed form of the new head weights (the forward's fp32 and
    // split-f16 operands, the backward chain's transposed ones) beside the factor tensors' Adam on `s`
    timing_begin(f, T2N_K_HEAD_STEP, sg);
    if ((rc = launch_head_adam_dev(P, A->head_grads, A->exp_avg + 12, A->exp_avg_sq + 12, A->beta1, A->beta2, A->eps, sc, sg, true, (unsigned*)mlp_bwd_ss_absmax_words(gpack)))) return rc;
    f->params_ref.basis_weight = P->basis_weight;
    f->params_ref.mlp_w0 = P->mlp_w0; f->params_ref.mlp_b0 = P->mlp_b0; f->params_ref.mlp_w1 = P->mlp_w1; f->params_ref.mlp_b1 = P->mlp_b1;
    f->params_ref.mlp_w2 = P->mlp_w2; f->params_ref.mlp_b2 = P->mlp_b2;
    for (int k = 0; k < 3; ++k) {
        f->params_ref.density_plane[k] = P->density_plane[k]; f->params_ref.density_line[k] = P->density_line[k];
        f->params_ref.app_plane[k] = P->app_plane[k]; f->params_ref.app_line[k] = P->app_line[k];
    }
    if ((rc = train_repack(f, P, sg))) return rc;
    f->ss_dirty = true;
    timing_end(f, T2N_K_HEAD_STEP, sg);
    T2N_HIP(hipEventRecord(ev[7], sg));
    if (do_grad) {
        // the density factors (a quarter of the bytes) step on sa right behind their scatter, beside the appearance scatter on `s`
        if ((rc = launch_factor_adam_dev(f, P, A->exp_avg, A->exp_avg_sq, A->beta1, A->beta2, A->eps, sc, 0, 6, sa, sworld, srank))) return rc;
        T2N_HIP(hipEventRecord(ev[9], sa));
        f->train_chain = true;      // (the next call's early part may start behind this event)
        timing_begin(f, T2N_K_ADAM, s);
        if ((rc = launch_factor_adam_dev(f, P, A->exp_avg, A->exp_avg_sq, A->beta1, A->beta2, A->eps, sc, 6, 6, s, sworld, srank))) return rc;
        timing_end(f, T2N_K_ADAM, s);
        T2N_HIP(hipStreamWaitEvent(s, ev[9], 0));
    } else if ((rc = launch_factor_adam_dev(f, P, A->exp_avg, A->exp_avg_sq, A->beta1, A->beta2, A->eps, sc, 0, 12, s, sworld, srank))) return rc;
    T2N_HIP(hipStreamWaitEvent(s, ev[7], 0));
    T2N_HIP(hipGetLastError());
    return T2N_OK;
}

// ---- the step as a hipGraph: stream capture of the call above (relaxed mode: the library's side streams join the capture through
// their event waits), instantiated once, replayed per step
struct t2n_train_graph { hipGraph_t graph; hipGraphExec_t exec; int nodes; t2n_field* f; };

extern "C" int t2n_train_graph_capture(t2n_field* f, const t2n_train_step_args* a, t2n_stream stream, t2n_train_graph** out) {
    if (!f || !a || !out) { set_error("t2n_train_graph_capture: NULL argument"); return T2N_ERR_INVALID; }
    if (!f->train_dev || !f->train_packed) { set_error("t2n_train_graph_capture: run t2n_train_step eagerly once first (lazy state cannot be captured)"); return T2N_ERR_STATE; }
    if (a->flags & (T2N_FLAG_REG_L1 | T2N_FLAG_REG_ORTHO)) {
        set_error("t2n_train_graph_capture: the L1 / ortho regularisers (T2N_FLAG_REG_L1 / T2N_FLAG_REG_ORTHO) are not part of the captured step: run it eagerly");
        return T2N_ERR_UNSUPPORTED;
    }
    // captured on a stream of its own: the caller's may be the legacy default stream, which cannot capture (hipErrorStreamCaptureUnsupported);
    // the instantiated graph is launched on whatever stream the caller passes to t2n_train_graph_launch
    (void)stream;
    hipStream_t s = nullptr;
    T2N_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    const hipError_t e0 = hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed);
    if (e0 != hipSuccess) { (void)hipStreamDestroy(s); return hip_fail(e0, "hipStreamBeginCapture"); }
    const int rc = t2n_train_step(f, a, (t2n_stream)s);
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(s, &g);
    (void)hipStreamDestroy(s);
    if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
    if (e != hipSuccess || !g) return hip_fail(e, "hipStreamEndCapture");
    hipGraphExec_t ex = nullptr;
    const hipError_t e2 = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    if (e2 != hipSuccess) { (void)hipGraphDestroy(g); return hip_fail(e2, "hipGraphInstantiate"); }
    size_t n = 0;
    (void)hipGraphGetNodes(g, nullptr, &n);
    t2n_train_graph* tg = new t2n_train_graph{g, ex, (int)n, f};
    *out = tg;
    return T2N_OK;
}
extern "C" int t2n_train_graph_launch(t2n_train_graph* g, t2n_stream stream) {
    if (!g) { set_error("t2n_train_graph_launch: NULL graph"); return T2N_ERR_INVALID; }
    t2n_field* f = g->f;
    if (!f->train_packed) {   // the head was uploaded since the last step (load_state_dict, a step of another optimiser): the captured step
        // expects the backward chain's operands of the CURRENT weights, which an optimiser phase leaves behind and an upload does not
        const int rc = mlp_bwd_ss_pack(f, (char*)f->train_dev + 256, (hipStream_t)stream, false, true);
        if (rc) return rc;
        f->train_packed = true;
    }
    ++f->den_version;   // the replayed step's Adam kernels rewrite the density factors (no launcher runs): the cached summed density table is stale
    ++f->app_version;   // ... and the appearance factors and basis_mat: the cached feature volume too
    T2N_HIP(hipGraphLaunch(g->exec, (hipStream_t)stream));
    return T2N_OK;
}
extern "C" int t2n_train_graph_nodes(const t2n_train_graph* g) { return g ? g->nodes : 0; }
extern "C" int t2n_train_graph_destroy(t2n_train_graph* g) {
    if (!g) return T2N_OK;
    (void)hipGraphExecDestroy(g->exec);
    (void)hipGraphDestroy(g->graph);
    delete g;
    return T2N_OK;
}
