// train.hip -- the train step as native calls (sgr_trainer_*, include/sugar_raster.h).
//
// Restates the order of gaussian_splatting/train.py:86-128 (render -> loss -> backward -> optimizer.step) on the caller's
// stream with the library's own kernels: sync-free rasterizer forward in raw-parameter mode, fused L1 + D-SSIM loss and its
// backward, blend backward, backward preprocess (gradients land in the flat gradient buffer), SH-Adam from the per-view
// colour gradients and flat Adam over the other 11 floats per Gaussian.  Host side only: ~25 launches per step and nothing
// else -- no allocation, no host wait, no interpreter between the kernels (the Python loop this replaces finished 27 us
// ahead of the GPU at 1.29 ms per step).
#include "../../include/sugar_raster.h"
#include "sgr_common.h"
#include "tile_order.h"

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <string>

namespace {

struct FixedBuf { char* p; size_t bytes; size_t asked; };
char* fixed_alloc(void* user, size_t bytes)
{
    FixedBuf* b = static_cast<FixedBuf*>(user);
    b->asked = bytes;
    return bytes <= b->bytes ? b->p : nullptr;
}

// ---- RCCL, bound at run time (no link-time dependency: a process that never exchanges gradients never loads it, and a process that
// already has torch's copy loaded shares it).  Only what the view-sharded step needs: rccl.h:40-43,187,220,260,339,448,466,611,678.
struct RcclUniqueId { char internal[128]; };
typedef void* RcclComm;
struct Rccl {
    void* handle = nullptr;
    int (*GetUniqueId)(RcclUniqueId*) = nullptr;
    int (*CommInitRank)(RcclComm*, int, RcclUniqueId, int) = nullptr;
    int (*CommDestroy)(RcclComm) = nullptr;
    int (*CommAbort)(RcclComm) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, RcclComm, hipStream_t) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, RcclComm, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool ok() const { return GetUniqueId && CommInitRank && CommDestroy && AllGather && AllReduce; }
};
const int RCCL_FLOAT = 7, RCCL_SUM = 0;
Rccl& rccl()
{
    static Rccl r;
    if (r.handle) return r;
    for (const char* name : {"librccl.so.1", "librccl.so"}) {
        r.handle = dlopen(name, RTLD_NOW | RTLD_NOLOAD);  // torch's copy, if it is already in the process
        if (r.handle) break;
    }
    if (!r.handle)
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            r.handle = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (r.handle) break;
        }
    if (!r.handle) return r;
    r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(dlsym(r.handle, "ncclGetUniqueId"));
    r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(dlsym(r.handle, "ncclCommInitRank"));
    r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(r.handle, "ncclCommDestroy"));
    r.CommAbort = reinterpret_cast<decltype(r.CommAbort)>(dlsym(r.handle, "ncclCommAbort"));
    r.AllGather = reinterpret_cast<decltype(r.AllGather)>(dlsym(r.handle, "ncclAllGather"));
    r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(dlsym(r.handle, "ncclAllReduce"));
    r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(r.handle, "ncclGetErrorString"));
    return r;
}

// ---- the process-wide switches of sgr_trainer_step, their only reader
// SH-Adam of unreached Gaussians inside the blend backward's launch (include/sugar_raster.h: sgr_set_adam_overlap); SGR_ADAM_OVERLAP
// in the environment sets the default, SGR_ADAM_OVERLAP_WAVES the persistent Adam workgroups in front of the blend's (a multiple of 8)
#define SGR_ADAM_OVERLAP_DEFAULT 1
#define SGR_ADAM_OVERLAP_WAVES_DEFAULT 512
int g_adam_overlap = -1;
int sgr_adam_overlap()
{
    if (g_adam_overlap < 0) { const char* e = getenv("SGR_ADAM_OVERLAP"); g_adam_overlap = e ? (e[0] == '2' ? 2 : (e[0] != '0' ? 1 : 0)) : SGR_ADAM_OVERLAP_DEFAULT; }
    return g_adam_overlap;
}
int sgr_adam_overlap_waves()  // SgrShAdamJob.n_adam
{
    const char* e = getenv("SGR_ADAM_OVERLAP_WAVES");  // (read per step: one getenv, and a test or an A/B run can change it in-process)
    const int n = e ? atoi(e) : SGR_ADAM_OVERLAP_WAVES_DEFAULT;
    return (n < 8 || (n & 7) || n > 65536) ? SGR_ADAM_OVERLAP_WAVES_DEFAULT : n;
}
// Backward preprocess of the train step by reach flag (include/sugar_raster.h: sgr_set_rows_by_reach); SGR_ROWS_BY_REACH=0 / 1 in the
// environment sets the default (on)
int g_rows_by_reach = -1;
int sgr_rows_by_reach()
{
    if (g_rows_by_reach < 0) { const char* e = getenv("SGR_ROWS_BY_REACH"); g_rows_by_reach = (e && e[0] == '0') ? 0 : 1; }
    return g_rows_by_reach;
}

}  // namespace

struct sgr_trainer {
    sgr_train_config c;
    // gradient exchange inside the library (sgr_trainer_comm_init)
    RcclComm comm = nullptr;
    int world = 1, rank = 0;
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_colors = nullptr, ev_small = nullptr;
    int chunks = 1;                                   // pieces of the colour all-gather / the small all-reduce (sgr_trainer_set_exchange_chunks)
    hipEvent_t ev_gathered[16] = {}, ev_reduced[16] = {};  // piece k has landed
    float* recv = nullptr;        // caller's buffer: world x (P + 1) x 3 floats
    float* campos_all = nullptr;  // world x 3 floats (owned)
    double last_wait_ms = 0.0;    // what the last sgr_trainer_step_exchange spent waiting for the forward's header
    hipEvent_t hdr_event = nullptr;
    bool have_forward = false;
    bool acc_dirty = true;      // the geometry scratch's accumulator table may hold non-zero records: the next backward resets it
    bool rows_unknown = true;   // the step's output rows (flat gradient, masked colours) may not match the geometry scratch's row-dirty
                                // table: the next backward by reach flag treats every row as dirty (SGR_BWD_ROWS_UNKNOWN)
    bool defer_post = false;    // the post-blend bookkeeping rides in the loss forward kernel (needs a device-mapped header_host)
    int64_t R = 0;              // what the last forward returned (= the capacity)
    long long seg_begin[4], seg_end[4];
    float seg_lr[4];
    int seg_one[4];
    std::string err;
};

extern "C" {

static thread_local std::string g_train_err;
static int tfail(int code, const std::string& m) { g_train_err = m; return code; }
const char* sgr_trainer_last_error(void) { return g_train_err.c_str(); }

void sgr_set_rows_by_reach(int on) { g_rows_by_reach = on ? 1 : 0; }
int sgr_get_rows_by_reach(void) { return sgr_rows_by_reach(); }
void sgr_set_adam_overlap(int on) { g_adam_overlap = on == 2 ? 2 : (on ? 1 : 0); }
int sgr_get_adam_overlap(void) { return sgr_adam_overlap(); }

sgr_trainer* sgr_trainer_create(const sgr_train_config* cfg)
{
    if (!cfg) { g_train_err = "null config"; return nullptr; }
    const sgr_train_config& c = *cfg;
    const bool ok = c.P > 0 && c.width > 0 && c.height > 0 && c.M >= (c.D + 1) * (c.D + 1) && c.M <= 16 && c.D >= 0 && c.D <= 3 &&
                    c.flat && c.flat_grad && c.exp_avg && c.exp_avg_sq && c.background && c.geom && c.img && c.binning &&
                    c.loss_scratch && c.image && c.grad_image && c.loss_out && c.colors && c.header_host &&
                    c.binning_capacity > 0 && c.n_small > 0 && (c.n_small & 3) == 0 && (c.off_features & 3) == 0;
    if (!ok) { g_train_err = "sgr_trainer_create: bad configuration (null pointer, size or alignment)"; return nullptr; }
    if (c.geom_bytes < sgr_geom_bytes(c.P) || c.img_bytes < sgr_img_bytes(c.width, c.height) + sgr_bin2_bytes(c.P, c.width, c.height) ||
        c.binning_bytes < sgr_binning_bytes(c.binning_capacity, c.width, c.height)) {
        g_train_err = "sgr_trainer_create: a scratch buffer is smaller than sgr_geom_bytes / sgr_img_bytes + sgr_bin2_bytes / sgr_binning_bytes";
        return nullptr;
    }
    sgr_trainer* t = new sgr_trainer;
    t->c = c;
    if (hipEventCreateWithFlags(&t->hdr_event, hipEventDisableTiming) != hipSuccess) { delete t; g_train_err = "hipEventCreate failed"; return nullptr; }
    const long long P = c.P;
    const long long b[4] = {c.off_xyz, c.off_opacity, c.off_scaling, c.off_rotation};
    const long long n[4] = {3 * P, P, 3 * P, 4 * P};
    const float lr[4] = {c.lr_xyz, c.lr_opacity, c.lr_scaling, c.lr_rotation};
    for (int k = 0; k < 4; k++) { t->seg_begin[k] = b[k]; t->seg_end[k] = b[k] + n[k]; t->seg_lr[k] = lr[k]; t->seg_one[k] = 1; }
    std::memset(c.header_host, 0, 64);
    // the reach flags start from zero (a stale 1 is safe, a stale 0 is not: sh_adam_update.h); a new topology is a new trainer.  The
    // row-dirty table behind them is cleared in the same stroke (rows_unknown holds until the first step by reach flag anyway)
    if (hipMemset(c.geom + sgr_geom_reach_offset(c.P), 0, sgr_geom_rowdirty_offset(c.P) + (size_t)c.P - sgr_geom_reach_offset(c.P)) != hipSuccess) {
        (void)hipEventDestroy(t->hdr_event); delete t; g_train_err = "sgr_trainer_create: clearing the reach flags failed"; return nullptr;
    }
    {
        // (pinned memory that is not mapped into the device's address space: the forward copies the header with copy commands and
        // does its own bookkeeping; SGR_TRAINER_NO_DEFER forces that path for a test)
        void* mapped = nullptr;
        t->defer_post = hipHostGetDevicePointer(&mapped, c.header_host, 0) == hipSuccess && mapped && !getenv("SGR_TRAINER_NO_DEFER");
        if (!t->defer_post) (void)hipGetLastError();
    }
    return t;
}

void sgr_trainer_destroy(sgr_trainer* t)
{
    if (!t) return;
    (void)sgr_trainer_comm_destroy(t);
    if (t->hdr_event) (void)hipEventDestroy(t->hdr_event);
    delete t;
}

int sgr_trainer_set_binning(sgr_trainer* t, char* binning, size_t bytes, int64_t capacity)
{
    if (!t || !binning || capacity <= 0 || bytes < sgr_binning_bytes(capacity, t->c.width, t->c.height))
        return tfail(SGR_E_INVALID, "sgr_trainer_set_binning: bad buffer");
    t->c.binning = binning; t->c.binning_bytes = bytes; t->c.binning_capacity = capacity;
    return 0;
}

int sgr_trainer_acc_dirty(sgr_trainer* t) { return (t && !t->acc_dirty) ? 0 : 1; }
void sgr_trainer_invalidate_rows(sgr_trainer* t) { if (t) t->rows_unknown = true; }

int sgr_trainer_forward_valid(sgr_trainer* t, uint32_t* header_out)
{
    if (!t || !t->have_forward) return tfail(SGR_E_INVALID, "sgr_trainer_forward_valid: no forward yet");
    if (hipEventSynchronize(t->hdr_event) != hipSuccess) return tfail(SGR_E_HIP, "hipEventSynchronize failed");
    const uint32_t* h = t->c.header_host;
    if (header_out) std::memcpy(header_out, h, 64);
    const bool bad = (int64_t)h[SGR_HDR_R] > t->R || h[8 + SGR_HDR_HINT_MISS] != 0u || h[SGR_HDR_L1_OVERFLOW] != 0u;
    return bad ? 0 : 1;
}

int sgr_trainer_step(sgr_trainer* t, const sgr_train_view* v, int phases, const sgr_train_exchange* ex, void* stream)
{
    if (!t || !v) return tfail(SGR_E_INVALID, "sgr_trainer_step: null argument");
    const sgr_train_config& c = t->c;
    hipStream_t s = (hipStream_t)stream;
    const int P = c.P, W = c.width, H = c.height;
    float* flat = c.flat;
    float* grad = c.flat_grad;
    const float* means3D = flat + c.off_xyz;
    const float* shs = flat + c.off_features;
    const float* opac = flat + c.off_opacity;
    const float* scal = flat + c.off_scaling;
    const float* rot = flat + c.off_rotation;
    const uint32_t* header = reinterpret_cast<const uint32_t*>(c.img + sgr_img_header_offset(W, H));
    const uint32_t cap = (uint32_t)(c.binning_capacity > 0xFFFFFFFFll ? 0xFFFFFFFFll : c.binning_capacity);
    // SGR_BWD_DENSE in the environment: the verification switch of the backward preprocess (every rendered row read) for the whole step
    const char* dense_env = getenv("SGR_BWD_DENSE");
    const bool bwd_dense = dense_env && dense_env[0] && dense_env[0] != '0';
    // SH-Adam split by reach flag (sh_adam_update.h): only for a whole step on this rank's one view -- a Gaussian unreached here may be
    // reached in another rank's view --, M == 16, a preprocess that takes its zero-row exit, and a view that does not ask for the
    // eight-wave blend kernel (which does not flag).  overlap == 2: the forward flags, the
    // dense kernel runs and nothing clears them (verification of the flags).
    const int overlap = sgr_adam_overlap();
    const bool reach_ok = overlap != 0 && phases == 15 && !(v->flags & SGR_VIEW_DEEP_LISTS) && ex && ex->n_views == 1 && !ex->all_colors && !ex->all_campos &&
                          !(ex->g_end > ex->g_begin) && c.M == 16 && !bwd_dense &&
                          ((((uintptr_t)(flat + c.off_features) | (uintptr_t)(c.exp_avg + c.off_features) |
                             (uintptr_t)(c.exp_avg_sq + c.off_features)) & 15) == 0);
    const bool split = reach_ok && overlap == 1;
    // ... and the backward preprocess by the same flags: an unflagged Gaussian costs it two flag bytes (sgr_set_rows_by_reach)
    const bool by_reach = split && sgr_rows_by_reach() != 0;
    uint8_t* reach = reinterpret_cast<uint8_t*>(c.geom + sgr_geom_reach_offset(P));
    // the SH-Adam step of ex->step, described once for both of its halves (a split step has phases == 15)
    SgrShAdamHyper sh_hyper = {};
    if ((phases & 12) && ex && ex->step >= 1)
        sh_hyper = sgr_sh_adam_hyper(c.lr_features_dc, c.lr_features_rest, c.beta1, c.beta2, c.eps, ex->step, ex->grad_scale, header, cap);
    if (phases & 1) {
        if (!v->viewmatrix || !v->projmatrix || !v->campos || !v->gt_image) return tfail(SGR_E_INVALID, "sgr_trainer_step: null view");
        FixedBuf g = {c.geom, c.geom_bytes, 0}, b = {c.binning, c.binning_bytes, 0}, i = {c.img, c.img_bytes, 0};
        sgr_forward_opts fo;
        std::memset(&fo, 0, sizeof(fo));
        fo.binning_capacity = c.binning_capacity;
        fo.flags = SGR_FLAG_RAW_PARAMS | ((v->flags & SGR_VIEW_DEEP_LISTS) ? 0 : SGR_FLAG_NO_DEEP) | (reach_ok ? SGR_FLAG_REACH : 0);
        fo.header_host = c.header_host;
        // the post-blend bookkeeping (launch order, walk hint, second header copy) rides in the loss forward kernel, which is what
        // follows the blend here; the event for the host is recorded behind it
        if (t->defer_post) fo.flags |= SGR_FLAG_DEFER_POST;
        fo.header_event = t->defer_post ? nullptr : t->hdr_event;
        fo.tile_need = v->tile_need;
        fo.tile_need_out = v->tile_need_out;
        fo.hint_margin = v->hint_margin;
        fo.chunk_grid = v->chunk_grid;
        fo.tile_order = v->tile_order;
        fo.tile_order_out = v->tile_order_out;
        const int64_t R = sgr_forward_ex(fixed_alloc, &g, fixed_alloc, &b, fixed_alloc, &i, P, c.D, c.M, c.background, W, H, means3D, shs,
                                         nullptr, opac, scal, 1.0f, rot, nullptr, v->viewmatrix, v->projmatrix, v->campos,
                                         v->tan_fovx, v->tan_fovy, 0, c.image, c.radii, 0, stream, &fo);
        if (R < 0) return tfail((int)R, std::string("forward: ") + sgr_last_error());
        t->R = R;
        t->have_forward = true;
        SgrTileOrderJob job = {};
        int rc = t->defer_post ? sgr_forward_post_job(W, H, c.img, R, &fo, &job) : 0;
        if (rc < 0) return tfail(rc, "sgr_forward_post_job failed");
        // (the loss value comes out of a spare workgroup of the backward kernel)
        { SgrStageTimer tm(s, SGR_STAGE_LOSS_FWD); rc = sgr_l1_ssim_forward_job(3, W, H, c.image, v->gt_image, c.lambda_dssim, c.loss_scratch, nullptr, t->defer_post ? &job : nullptr, stream); }
        if (rc < 0) return tfail(rc, "l1_ssim_forward failed");
        if (t->defer_post && hipEventRecord(t->hdr_event, s) != hipSuccess) return tfail(SGR_E_HIP, "hipEventRecord failed");
        { SgrStageTimer tm(s, SGR_STAGE_LOSS_BWD); rc = sgr_l1_ssim_backward_ex(3, W, H, c.image, v->gt_image, c.lambda_dssim, c.loss_scratch, nullptr, c.grad_image, c.loss_out, stream); }
        if (rc < 0) return tfail(rc, "l1_ssim_backward failed");
    }
    if (phases & 3) {
        if (!t->have_forward) return tfail(SGR_E_INVALID, "sgr_trainer_step: backward before any forward");
        // (camera centre: the row behind the colours; the launch order: sorted by the job that rode in the loss kernel, or by the
        // forward itself when the view keeps the order)
        // (SGR_BWD_ACC_CLEAN: the accumulator table is zero between steps -- the preprocess kernel puts the few records the blend
        // backward dirtied back -- so no step resets its 64 B per Gaussian; see acc_dirty below)
        sgr_backward_opts bo = {c.max_radii2D, c.grad_accum, c.denom, c.colors + 3 * (size_t)P,
                                ((t->defer_post || v->tile_order_out) ? SGR_BWD_TILE_ORDER_READY : 0) | SGR_BWD_ACC_CLEAN |
                                    (bwd_dense ? SGR_BWD_DENSE : 0) |
                                    (by_reach ? (SGR_BWD_ROWS_BY_REACH | (t->rows_unknown ? SGR_BWD_ROWS_UNKNOWN : 0)) : 0)};
        // every backward that writes the rows densely leaves them out of step with the row-dirty table, and so does one that returns
        // an error half-way: the table counts again once a backward by reach flag has been enqueued
        t->rows_unknown = true;
        // the zero-gradient half of SH-Adam rides in the blend backward's launch (the bias corrections of ex->step are known here)
        SgrShAdamJob job = {};
        if (split) {
            if (ex->step < 1) return tfail(SGR_E_INVALID, "sgr_trainer_step: exchange description missing");
            job = sgr_sh_adam_job(sh_hyper, P, sgr_adam_overlap_waves(), flat + c.off_features, c.exp_avg + c.off_features,
                                  c.exp_avg_sq + c.off_features, reach);
        }
        // compact SH mode (dL_dsh == NULL), raw-parameter gradients straight into the flat gradient buffer.  Both halves asked
        // for at once (no collective to start in between): ONE pass, the preprocess kernel writes the masked colour gradients
        // itself (the split costs a 23 us kernel of its own)
        const int first = (phases & 3) == 3 ? 0 : ((phases & 1) ? 1 : 2);
        const int last = (phases & 3) == 3 ? 0 : ((phases & 2) ? 2 : 1);
        for (int ph = first; ph <= last; ph++) {
            if (ph != 2) {
                // the table is dirty from here until the preprocess half has been enqueued: a step that returns an error in between
                // costs the next one a reset, not wrong gradients
                if (t->acc_dirty && sgr_acc_reset(c.geom, P, s) != hipSuccess)
                    return tfail(SGR_E_HIP, "sgr_trainer_step: accumulator reset failed");
                t->acc_dirty = true;
            }
            const int rc = sgr_backward_job(ph | SGR_MODE_RAW_PARAMS, P, c.D, c.M, t->R, c.background, W, H, means3D, shs, scal, rot,
                                            v->viewmatrix, v->projmatrix, v->campos, v->tan_fovx, v->tan_fovy, c.geom, c.binning, c.img,
                                            c.grad_image, c.dL_dmean2D, grad + c.off_opacity, c.colors, grad + c.off_xyz,
                                            grad + c.off_scaling, grad + c.off_rotation, stream, &bo, split ? &job : nullptr);
            if (rc < 0) return tfail(rc, std::string("backward: ") + sgr_last_error());
            if (ph != 1) t->acc_dirty = false;
            if (by_reach) t->rows_unknown = false;
        }
    }
    if (phases & 12) {
        if (!ex || ex->step < 1 || ex->n_views < 1) return tfail(SGR_E_INVALID, "sgr_trainer_step: exchange description missing");
        if (phases & 4) {
            const float* cols = ex->all_colors ? ex->all_colors : c.colors;
            const float* cams = ex->all_campos ? ex->all_campos : (ex->all_colors ? nullptr : c.colors + 3 * (size_t)P);
            if (!cams) return tfail(SGR_E_INVALID, "sgr_trainer_step: all_campos missing");
            const size_t stride = (size_t)(ex->view_stride ? ex->view_stride : (ex->all_colors ? P : P + 1));
            // a chunk of the Gaussians (the exchange in pieces): the colour block starts at the chunk's first Gaussian
            const bool part = ex->g_end > ex->g_begin;
            const long long g0 = part ? ex->g_begin : 0, g1 = part ? ex->g_end : P;
            if (g0 < 0 || g1 > P || (g0 & 63)) return tfail(SGR_E_INVALID, "sgr_trainer_step: bad Gaussian range (g_begin must be a multiple of 64)");
            if (part && !ex->all_colors) cols += 3 * (size_t)g0;
            const size_t fo = (size_t)g0 * 3 * (size_t)c.M;
            SgrStageTimer tm(s, SGR_STAGE_SH_ADAM);
            sgr_launch_sh_adam_from_views((int)(g1 - g0), ex->n_views, c.D, c.M, stride, means3D + 3 * (size_t)g0, cams, cols,
                                          flat + c.off_features + fo, c.exp_avg + c.off_features + fo, c.exp_avg_sq + c.off_features + fo,
                                          sh_hyper, nullptr, split ? reach : nullptr, s);  // (split: the flagged rows only; clears the flags)
            tm.stop();
            if (hipGetLastError() != hipSuccess) return tfail(SGR_E_HIP, "sh_adam launch failed");
        }
        if (phases & 8) {
            const bool part = ex->f_end > ex->f_begin;
            const long long f0 = part ? ex->f_begin : 0, f1 = part ? ex->f_end : c.n_small;
            if (f0 < 0 || f1 > c.n_small || (f0 & 3)) return tfail(SGR_E_INVALID, "sgr_trainer_step: bad float range (f_begin must be a multiple of 4)");
            long long sb[4], se[4];
            for (int k = 0; k < 4; k++) { sb[k] = t->seg_begin[k] - f0; se[k] = t->seg_end[k] - f0; }  // (the launch indexes from its own base)
            SgrStageTimer tm(s, SGR_STAGE_ADAM);
            const int rc = sgr_adam_launch(f1 - f0, flat + f0, grad + f0, c.exp_avg + f0, c.exp_avg_sq + f0, 4, sb, se, t->seg_lr, t->seg_lr,
                                           t->seg_one, t->seg_one, c.beta1, c.beta2, c.eps, ex->step, ex->grad_scale, nullptr, 0, header,
                                           cap, s);
            tm.stop();
            if (rc < 0) return tfail(rc, "adam launch failed");
        }
    }
    return 0;
}


// ---- the gradient exchange of the view-sharded step inside the library: RCCL on a stream of its own, no interpreter between
// the four phases (include/sugar_raster.h)
int sgr_rccl_unique_id(char* out128)
{
    Rccl& r = rccl();
    if (!r.ok()) return tfail(SGR_E_INVALID, "RCCL could not be loaded (librccl.so)");
    RcclUniqueId id;
    const int rc = r.GetUniqueId(&id);
    if (rc != 0) return tfail(SGR_E_HIP, std::string("ncclGetUniqueId: ") + (r.GetErrorString ? r.GetErrorString(rc) : "failed"));
    std::memcpy(out128, id.internal, 128);
    return 0;
}

int sgr_trainer_comm_init(sgr_trainer* t, const char* id128, int world, int rank, float* recv, size_t recv_bytes)
{
    if (!t || !id128 || world < 1 || rank < 0 || rank >= world || !recv) return tfail(SGR_E_INVALID, "sgr_trainer_comm_init: bad argument");
    if (recv_bytes < (size_t)world * ((size_t)t->c.P + 1) * 3 * sizeof(float))
        return tfail(SGR_E_INVALID, "sgr_trainer_comm_init: receive buffer smaller than world x (P + 1) x 3 floats");
    if (t->comm) return tfail(SGR_E_INVALID, "sgr_trainer_comm_init: already initialised");
    Rccl& r = rccl();
    if (!r.ok()) return tfail(SGR_E_INVALID, "RCCL could not be loaded (librccl.so)");
    RcclUniqueId id;
    std::memcpy(id.internal, id128, 128);
    int rc = r.CommInitRank(&t->comm, world, id, rank);
    if (rc != 0) { t->comm = nullptr; return tfail(SGR_E_HIP, std::string("ncclCommInitRank: ") + (r.GetErrorString ? r.GetErrorString(rc) : "failed")); }
    t->world = world; t->rank = rank; t->recv = recv;
    bool ok = hipStreamCreateWithFlags(&t->comm_stream, hipStreamNonBlocking) == hipSuccess;
    for (hipEvent_t* e : {&t->ev_colors, &t->ev_small})
        ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    for (int k = 0; k < 16; k++)
        ok = ok && hipEventCreateWithFlags(&t->ev_gathered[k], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&t->ev_reduced[k], hipEventDisableTiming) == hipSuccess;
    ok = ok && hipMalloc(reinterpret_cast<void**>(&t->campos_all), (size_t)world * 3 * sizeof(float)) == hipSuccess;
    if (!ok) { (void)sgr_trainer_comm_destroy(t); return tfail(SGR_E_HIP, "sgr_trainer_comm_init: stream / event / buffer creation failed"); }
    return 0;
}

// A rank that cannot go on (an error no repeat of the step repairs) tears its communicator down instead of leaving the others
// blocked in the collective it will never join: their pending RCCL calls then fail with an error instead of waiting for ever.
int sgr_trainer_comm_abort(sgr_trainer* t)
{
    if (!t || !t->comm) return 0;
    Rccl& r = rccl();
    if (r.CommAbort) (void)r.CommAbort(t->comm); else (void)r.CommDestroy(t->comm);
    t->comm = nullptr;
    return sgr_trainer_comm_destroy(t);
}

double sgr_trainer_last_exchange_wait_ms(sgr_trainer* t) { return t ? t->last_wait_ms : 0.0; }

int sgr_trainer_set_exchange_chunks(sgr_trainer* t, int n)
{
    if (!t || n < 1 || n > 16) return tfail(SGR_E_INVALID, "sgr_trainer_set_exchange_chunks: 1 <= n <= 16");
    t->chunks = n;
    return 0;
}

int sgr_trainer_comm_destroy(sgr_trainer* t)
{
    if (!t) return 0;
    if (t->comm_stream) (void)hipStreamSynchronize(t->comm_stream);
    if (t->comm) { (void)rccl().CommDestroy(t->comm); t->comm = nullptr; }
    for (hipEvent_t* e : {&t->ev_colors, &t->ev_small})
        if (*e) { (void)hipEventDestroy(*e); *e = nullptr; }
    for (int k = 0; k < 16; k++)
        for (hipEvent_t* e : {&t->ev_gathered[k], &t->ev_reduced[k]})
            if (*e) { (void)hipEventDestroy(*e); *e = nullptr; }
    if (t->comm_stream) { (void)hipStreamDestroy(t->comm_stream); t->comm_stream = nullptr; }
    if (t->campos_all) { (void)hipFree(t->campos_all); t->campos_all = nullptr; }
    t->world = 1; t->rank = 0; t->recv = nullptr;
    return 0;
}

// One view-sharded step with the exchange inside: forward + loss + blend half of the backward; the forward's header is waited for
// and checked HERE, before anything is sent (a rank whose list outgrew its capacity or missed its walk hint returns 1 with nothing
// sent and nothing changed: the caller enlarges the capacity / drops the hint and calls again, while the other ranks wait in the
// all-gather); then all-gather of the masked colour gradients (+ camera centre row) on the communication stream beside the
// preprocess half, all-reduce of the 11 small floats per Gaussian beside the SH half of Adam, and the two Adam kernels behind their
// events.  Same kernels and the same places for the collectives as the torch.distributed path of sugar_amd.train_step.NativeTrainer.
int sgr_trainer_step_exchange(sgr_trainer* t, const sgr_train_view* v, int step, void* stream)
{
    if (!t || !v || step < 1) return tfail(SGR_E_INVALID, "sgr_trainer_step_exchange: bad argument");
    if (!t->comm) return tfail(SGR_E_INVALID, "sgr_trainer_step_exchange: sgr_trainer_comm_init first");
    Rccl& r = rccl();
    hipStream_t s = (hipStream_t)stream;
    const sgr_train_config& c = t->c;
    const size_t P = (size_t)c.P;
    int rc = sgr_trainer_step(t, v, 1, nullptr, stream);
    if (rc < 0) return rc;
    uint32_t hdr[16];
    const auto w0 = std::chrono::steady_clock::now();
    rc = sgr_trainer_forward_valid(t, hdr);
    t->last_wait_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
    if (rc < 0) return rc;
    if (rc == 0) return 1;  // invalid forward: nothing was sent
#define EX_TRY(expr, what)                                                                     \
    do {                                                                                       \
        if ((expr) != hipSuccess) return tfail(SGR_E_HIP, std::string(what) + ": HIP call failed"); \
    } while (0)
    // The exchange in `chunks` pieces (round 6).  Communication stream, in order: the camera centres (3 floats per rank), the colour
    // gradients of Gaussian chunk 0 .. C-1 (each rank's piece lands in the chunk's own [world][len][3] block of `recv`), then -- once
    // the preprocess half has produced them -- the 11 small floats per Gaussian as C slices of the flat gradient buffer (in place).
    // Compute stream: preprocess half, then SH-Adam of chunk k behind ITS gather, then flat Adam of slice j behind ITS reduction.
    // Only the first piece of each collective and whatever the wire cannot hide is exposed (DESIGN.md section 6 has the model).
    const int C = t->chunks;
    auto g_at = [&](int k) { return k >= C ? P : (k <= 0 ? (size_t)0 : (P * (size_t)k / (size_t)C) & ~(size_t)255); };
    const size_t NS = (size_t)c.n_small;
    auto f_at = [&](int k) { return k >= C ? NS : (k <= 0 ? (size_t)0 : (NS * (size_t)k / (size_t)C) & ~(size_t)1023); };
#define NCCL_TRY(expr, what)                                                                                            \
    do {                                                                                                                \
        const int nrc_ = (expr);                                                                                        \
        if (nrc_ != 0) return tfail(SGR_E_HIP, std::string(what) + ": " + (r.GetErrorString ? r.GetErrorString(nrc_) : "failed")); \
    } while (0)
    EX_TRY(hipEventRecord(t->ev_colors, s), "record colours");
    EX_TRY(hipStreamWaitEvent(t->comm_stream, t->ev_colors, 0), "wait colours");
    NCCL_TRY(r.AllGather(c.colors + 3 * P, t->campos_all, 3, RCCL_FLOAT, t->comm, t->comm_stream), "ncclAllGather (camera centres)");
    for (int k = 0; k < C; k++) {
        const size_t g0 = g_at(k), g1 = g_at(k + 1);
        if (g1 > g0)
            NCCL_TRY(r.AllGather(c.colors + 3 * g0, t->recv + 3 * (size_t)t->world * g0, 3 * (g1 - g0), RCCL_FLOAT, t->comm, t->comm_stream),
                     "ncclAllGather (colour gradients)");
        EX_TRY(hipEventRecord(t->ev_gathered[k], t->comm_stream), "record gathered");
    }
    rc = sgr_trainer_step(t, v, 2, nullptr, stream);
    if (rc < 0) return rc;
    EX_TRY(hipEventRecord(t->ev_small, s), "record small gradients");
    EX_TRY(hipStreamWaitEvent(t->comm_stream, t->ev_small, 0), "wait small gradients");
    for (int k = 0; k < C; k++) {
        const size_t f0 = f_at(k), f1 = f_at(k + 1);
        if (f1 > f0)
            NCCL_TRY(r.AllReduce(c.flat_grad + f0, c.flat_grad + f0, f1 - f0, RCCL_FLOAT, RCCL_SUM, t->comm, t->comm_stream), "ncclAllReduce");
        EX_TRY(hipEventRecord(t->ev_reduced[k], t->comm_stream), "record reduced");
    }
    sgr_train_exchange ex;
    std::memset(&ex, 0, sizeof(ex));
    ex.n_views = t->world; ex.all_campos = t->campos_all; ex.grad_scale = 1.0f / (float)t->world; ex.step = step;
    for (int k = 0; k < C; k++) {
        const size_t g0 = g_at(k), g1 = g_at(k + 1);
        EX_TRY(hipStreamWaitEvent(s, t->ev_gathered[k], 0), "wait gathered");
        if (g1 <= g0) continue;
        ex.all_colors = t->recv + 3 * (size_t)t->world * g0; ex.view_stride = (int64_t)(g1 - g0);
        ex.g_begin = (int64_t)g0; ex.g_end = (int64_t)g1;
        rc = sgr_trainer_step(t, v, 4, &ex, stream);
        if (rc < 0) return rc;
    }
    for (int k = 0; k < C; k++) {
        const size_t f0 = f_at(k), f1 = f_at(k + 1);
        EX_TRY(hipStreamWaitEvent(s, t->ev_reduced[k], 0), "wait reduced");
        if (f1 <= f0) continue;
        ex.f_begin = (int64_t)f0; ex.f_end = (int64_t)f1;
        rc = sgr_trainer_step(t, v, 8, &ex, stream);
        if (rc < 0) return rc;
    }
#undef NCCL_TRY
#undef EX_TRY
    return 0;
}

}  // extern "C"
