// extern "C" surface of libvdx.so: argument validation + dispatch to the kernel launchers.
#include <stdio.h>
#include <string.h>
#include <math.h>
#include "vdx_internal.h"
#include "model.h"
#include "comm.h"

// Everything a sampling step can bake into its captured graph: what the fifteen vdx_*_sample_loop* entry points (the eleven over a
// network with out_dim == channels, the three super-resolution ones, vdx_*_sample_loop_sr, and the mixed-noise ancestral one,
// vdx_p_sample_loop_mixed) fill in and sample_loop() runs.  A field the entry does not have stays zero.
// (CHAIN_VLB tags the graph key of vdx_vlb_loop only: it never goes through sample_loop, whose slot arithmetic 3 * variant + chain takes 0..2)
// (CHAIN_LV / CHAIN_VLB_LV: the learned-variance loops, vdx_p_sample_loop_lv / vdx_vlb_loop_lv, likewise outside sample_loop)
enum { CHAIN_ANCESTRAL = 0, CHAIN_DDIM = 1, CHAIN_DPM = 2, CHAIN_VLB = 3, CHAIN_LV = 4, CHAIN_VLB_LV = 5 };
struct LoopArgs {
    int chain, masked, guided;                          // CHAIN_*; the masked (inpainting) step; classifier-free guidance over 2 * batch rows
    const float* params; const void* packed;
    float* img; float* eps_buf; float* hist; int* t_dev; uint64_t* step_dev;
    float* xin;                                         // the super-resolution loops alone: the network's input [batch, 2C, F, S, S]
    const float* tables; int timesteps;                 // [5][T]: the ancestral step and the dynamic threshold; T is also mask_tables' row length
    const float* alphas_cumprod; const int* seq; int seq_len;     // the two sequence chains
    const float* cond; uint64_t seed; int clip_denoised, order;
    float percentile; float* thres_buf;                 // dynamic threshold: percentile > 0 && clip_denoised
    const float* known; const unsigned char* mask; const float* mask_tables; int resample_steps;
    float cond_scale, rescale; double* cfg_scratch;
    float mix_a, mix_b;                                 // vdx_p_sample_loop_mixed alone: the step is p_sample_mixed_kernel; (0, 0) everywhere else
    float post_scale, post_shift;                       // the learned-variance sampling loop (vdx_p_sample_loop_lv) alone
    const float* vlb_x; const double* vlb_tables; double* vlb_partial; double* vlb_out;     // the evaluation loop (vdx_vlb_loop) alone
    void* workspace; size_t workspace_bytes; int batch;
};

struct vdx_handle {
    vdx::Model model;
    // the key of a captured sampling step: the LoopArgs of the call with every field its step does not read set to zero (sample_loop()),
    // the stream and the activation storage.  Full pointers: two workspaces / streams never alias one key.  Compared with memcmp, so it
    // is zero-filled before the fields are assigned.  pred / pred_sa / pred_s1: the prediction the step converts (vdx_set_prediction);
    // sc / sc_T / sc_tab: the self-condition state (vdx_set_self_condition), whose tables the sequence chains' steps read as well
    struct GraphKey { LoopArgs a; const void* stream; int act16; int pred; const float* pred_sa; const float* pred_s1; int sc; int sc_T; const float* sc_tab; };
    // one cached graph per (chain, variant): slot = 3 * variant + chain with variant 0 = plain, 1 = masked, 2 = guided and chain 0 = the
    // ancestral loop, 1 = DDIM, 2 = DPM-Solver++; slot 9 = the evaluation loop (vdx_vlb_loop), 10 / 11 = the learned-variance sampling and
    // evaluation loops, 12 + chain = the super-resolution loops (vdx_*_sample_loop_sr), 15 / 16 = the plain and the guided mixed-noise
    // ancestral loop (vdx_p_sample_loop_mixed) -- no loop ever evicts another one's graph
    // `last` = the stream the exec was last launched on: replays may still be running when the graph has to go
    struct GraphSlot {
        hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; GraphKey key; hipStream_t last = nullptr;
        void drop() {
            if (exec && last) (void)hipStreamSynchronize(last);       // earlier hipGraphLaunch calls of this exec have finished
            if (exec) { (void)hipGraphExecDestroy(exec); exec = nullptr; }
            if (graph) { (void)hipGraphDestroy(graph); graph = nullptr; }
            last = nullptr;
        }
    } gs[17];
    void drop_graphs() { for (GraphSlot& g : gs) g.drop(); }
    // what the network predicts (vdx_set_prediction): 0 = eps, 1 = v with the caller's device tables sqrt(ac) | sqrt(1 - ac) [pred_T]
    int pred = 0; const float* pred_sa = nullptr; const float* pred_s1 = nullptr; int pred_T = 0;
    // self-conditioning (vdx_set_self_condition): 1 = the step of an xin loop writes x0~ into planes [C, 2C) of xin, with rows 0, 1 of the
    // caller's [5][sc_T] device step tables
    int sc = 0; const float* sc_tab = nullptr; int sc_T = 0;
    void key_prediction(GraphKey& k) const { k.pred = pred; k.pred_sa = pred_sa; k.pred_s1 = pred_s1; k.sc = sc; k.sc_T = sc_T; k.sc_tab = sc_tab; }
    vdx::BwdState bwd;
    vdx::Comm comm;
};

namespace vdx {
vdx_launch_hook g_launch_hook = nullptr;
void* g_launch_hook_user = nullptr;
}

static thread_local char g_err[512] = "";

int vdx_set_error(int code, const char* msg, const char* file, int line) {
    snprintf(g_err, sizeof(g_err), "%s (%s:%d)", msg ? msg : "error", file ? file : "?", line);
    return code;
}
#define VDX_FAIL(code, msg) return vdx_set_error((code), (msg), __FILE__, __LINE__)
#define VDX_HIP(expr)                                                                   \
    do { hipError_t _e = (expr); if (_e != hipSuccess) return vdx_set_error(VDX_ERR_HIP, hipGetErrorString(_e), __FILE__, __LINE__); } while (0)
// a refused call of a family's builder: "<entry>: <rule>", so that the rule's text exists once for all the entries of the family
#define VDX_REFUSE(who, rule) do { char msg_[256]; snprintf(msg_, sizeof(msg_), "%s: %s", (who), (rule)); VDX_FAIL(VDX_ERR_INVALID, msg_); } while (0)

static bool mode_ok(int mode) { return mode == VDX_MODE_F32 || mode == VDX_MODE_BF16 || mode == VDX_MODE_F16; }

// runs `step` nsteps times on `st`: eagerly, or (use_graph) captured once into the handle's graph slot `which` and replayed
template <class Step>
static int run_steps(vdx_handle* h, int which, const vdx_handle::GraphKey& key, int nsteps, int use_graph, hipStream_t st, Step step) {
    if (!use_graph) {
        for (int i = 0; i < nsteps; ++i) { int rc = step(); if (rc != VDX_OK) return rc; }
        return VDX_OK;
    }
    vdx_handle::GraphSlot& g = h->gs[which];
    int done = 0;
    if (!g.exec || memcmp(&key, &g.key, sizeof(key)) != 0) {
        if (nsteps == 0) return VDX_OK;
        int rc = step();                                    // eager first step (also sets kernel attributes before capture)
        if (rc != VDX_OK) return rc;
        done = 1;
        g.drop();
        VDX_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        rc = step();
        hipError_t ce = hipStreamEndCapture(st, &g.graph);
        if (rc != VDX_OK || ce != hipSuccess) {             // a failed capture leaves no half-built graph behind
            if (g.graph) { (void)hipGraphDestroy(g.graph); g.graph = nullptr; }
            if (rc != VDX_OK) return rc;
            return vdx_set_error(VDX_ERR_HIP, hipGetErrorString(ce), __FILE__, __LINE__);
        }
        hipError_t ie = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0);
        if (ie != hipSuccess) { g.exec = nullptr; g.drop(); return vdx_set_error(VDX_ERR_HIP, hipGetErrorString(ie), __FILE__, __LINE__); }
        g.key = key;
    }
    g.last = st;
    for (int i = done; i < nsteps; ++i) VDX_HIP(hipGraphLaunch(g.exec, st));
    return VDX_OK;
}

extern "C" {

static void free_pos_bias(vdx::Model& m);

const char* vdx_last_error(void) { return g_err; }
int vdx_version(void) { return 1; }

size_t vdx_packed_conv_bytes(int mode, int taps, int cin, int cout) { return vdx::conv_packed_bytes(mode, taps, cin, cout); }

int vdx_pack_conv_weights(int mode, const float* kernel, void* packed, int taps, int cin, int cout, void* stream) {
    if (!kernel || !packed || taps <= 0 || cin <= 0 || cout <= 0) VDX_FAIL(VDX_ERR_INVALID, "pack_conv_weights: bad argument");
    if (!mode_ok(mode)) VDX_FAIL(VDX_ERR_INVALID, "bad mode");
    VDX_HIP(vdx::launch_pack_weights(mode, kernel, packed, taps, cin, cout, (hipStream_t)stream));
    return VDX_OK;
}

void vdx_set_launch_hook(vdx_launch_hook hook, void* user) { vdx::g_launch_hook = hook; vdx::g_launch_hook_user = user; }

size_t vdx_gn_stats_bytes(int batch, int groups) { return (size_t)batch * 32 /*GN_SLOTS*/ * groups * 2 * sizeof(double); }

static int conv_forward_rows(int mode, const vdx_conv_desc* d, int w_rows, int w_row0, void* stream) {
    if (!d || !d->x0 || !d->packed_w || !d->y) VDX_FAIL(VDX_ERR_INVALID, "conv: null tensor");
    if (!mode_ok(mode)) VDX_FAIL(VDX_ERR_INVALID, "bad mode");
    if (d->c0 % 4 || d->c1 % 4 || d->cout % 4) VDX_FAIL(VDX_ERR_INVALID, "conv: channel counts must be multiples of 4");
    if (d->c1 && !d->x1) VDX_FAIL(VDX_ERR_INVALID, "conv: x1 missing");
    if (d->batch <= 0 || d->frames <= 0 || d->h <= 0 || d->w <= 0) VDX_FAIL(VDX_ERR_INVALID, "conv: bad geometry");
    vdx::ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.x0 = d->x0; a.x1 = d->x1; a.C0 = d->c0; a.C1 = d->c1;
    a.wp = d->packed_w; a.bias = d->bias; a.y = d->y; a.Cout = d->cout;
    a.NF = d->batch * d->frames; a.F = d->frames; a.H = d->h; a.W = d->w;
    a.kind = d->kind;
    if (d->kind == 0) {
        if (d->kh != d->kw || d->kh < 1 || d->kh > 4 || (d->stride != 1 && d->stride != 2)) VDX_FAIL(VDX_ERR_INVALID, "conv: unsupported kernel/stride");
        if (d->stride == 2 && (d->h % 2 || d->w % 2)) VDX_FAIL(VDX_ERR_INVALID, "conv: stride 2 needs even H, W");
        a.kh = d->kh; a.kw = d->kw; a.stride = d->stride;
        // Flax SAME: total = max((ceil(n/s)-1)*s + k - n, 0), low = total/2 (n even for s=2)
        const int total = d->stride == 1 ? d->kh - 1 : d->kh - 2;
        a.pad = total / 2;
        if (d->stride == 1 && (d->kh % 2) == 0) VDX_FAIL(VDX_ERR_INVALID, "conv: even kernel needs stride 2");
    } else if (d->kind == 1) {
        a.kh = a.kw = 4; a.stride = 1; a.pad = 0;
    } else VDX_FAIL(VDX_ERR_INVALID, "conv: bad kind");
    if (d->in_stats) {
        if (d->c1) VDX_FAIL(VDX_ERR_INVALID, "conv: prologue with concat input is not supported");
        if (!d->gamma || !d->beta || d->groups <= 0 || d->groups > 32 || d->c0 % d->groups) VDX_FAIL(VDX_ERR_INVALID, "conv: bad prologue");
        a.pro = 1; a.in_stats = d->in_stats; a.gamma = d->gamma; a.beta = d->beta; a.groups = d->groups;
        a.ss = d->scale_shift; a.ss_stride = d->scale_shift_stride;
    }
    if (d->out_stats) {
        if (d->out_groups <= 0 || d->cout % d->out_groups) VDX_FAIL(VDX_ERR_INVALID, "conv: bad out_groups");
        a.out_stats = d->out_stats; a.out_groups = d->out_groups;
    }
    if ((d->x_bf16 || d->y_bf16) && mode != VDX_MODE_BF16) VDX_FAIL(VDX_ERR_INVALID, "conv: bf16 tensors need VDX_MODE_BF16");
    if (d->x_bf16 && (d->c0 % 8 || d->c1 % 8)) VDX_FAIL(VDX_ERR_INVALID, "conv: bf16 inputs need channel counts that are multiples of 8");
    a.x0_bf16 = a.x1_bf16 = d->x_bf16 ? 1 : 0; a.y_bf16 = d->y_bf16 ? 1 : 0;
    if (d->res) {
        if (d->out_stats || d->kind != 0 || d->stride != 1) VDX_FAIL(VDX_ERR_INVALID, "conv: res needs a stride-1 conv without statistics");
        if (d->res_bf16 && mode != VDX_MODE_BF16) VDX_FAIL(VDX_ERR_INVALID, "conv: bf16 tensors need VDX_MODE_BF16");
        a.res = (const float*)d->res; a.res_bf16 = d->res_bf16 ? 1 : 0;
    }
    a.wrows = w_rows; a.wrow0 = w_row0;                    // (0, 0 = cout rows from 0)
    VDX_HIP(vdx::launch_conv(mode, a, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_conv_forward(int mode, const vdx_conv_desc* d, void* stream) { return conv_forward_rows(mode, d, 0, 0, stream); }

int vdx_conv_forward_rows(int mode, const vdx_conv_desc* d, int w_rows, int w_row0, void* stream) {
    if (!d) VDX_FAIL(VDX_ERR_INVALID, "conv: null tensor");
    if (w_rows < 1 || w_row0 < 0 || w_row0 + d->cout > w_rows) VDX_FAIL(VDX_ERR_INVALID, "conv_forward_rows: rows [w_row0, w_row0 + cout) must lie inside the w_rows packed rows");
    if (w_rows % 4 || w_row0 % 4) VDX_FAIL(VDX_ERR_INVALID, "conv_forward_rows: w_rows and w_row0 must be multiples of 4");
    return conv_forward_rows(mode, d, w_rows, w_row0, stream);
}

// ---- the ResnetBlock tail.  What its four entries share: the GroupNorm / LayerNorm operands and the shape rules of the tail kernels
static int tail_args(vdx::TailArgs& a, const char* who, const void* y2, int y2_bf16, const double* stats, const float* gn_gamma, const float* gn_beta,
                     int groups, const float* ln_gamma, const float* ln_beta, int c, int batch, long pix_per_sample) {
    if (!y2 || !stats || !gn_gamma || !gn_beta || !ln_gamma || !ln_beta) VDX_REFUSE(who, "null tensor");
    if (c < 1 || batch < 1 || pix_per_sample < 1 || groups < 1 || groups > 32 || c % groups)
        VDX_REFUSE(who, "c, batch and pix_per_sample must be >= 1 and groups (1..32) divide c");
    memset(&a, 0, sizeof(a));
    a.y2 = (const float*)y2; a.y2_bf16 = y2_bf16 ? 1 : 0; a.stats = stats; a.gn_gamma = gn_gamma; a.gn_beta = gn_beta; a.groups = groups;
    a.ln_gamma = ln_gamma; a.ln_beta = ln_beta; a.C = c; a.batch = batch; a.pix_per_sample = pix_per_sample;
    return VDX_OK;
}
// the two rc entries: the fused 1x1 res_conv over concat(x0, x1) stands in for `r`; every tensor is bf16
static int tail_rc_args(vdx::TailArgs& a, const char* who, const void* x0, const void* x1, int c0, int c1, const void* rc_w_packed, const float* rc_bias) {
    if (!x0 || !rc_w_packed || !rc_bias || (c1 && !x1)) VDX_REFUSE(who, "null tensor");
    if (c1 < 0 || !vdx::tail_rc16_supported(c0 + c1, c0, a.C, a.pix_per_sample)) VDX_REFUSE(who, "shape not served");
    a.y2_bf16 = a.r_bf16 = a.out_bf16 = 1;
    a.x0 = (const float*)x0; a.x1 = (const float*)x1; a.C0 = c0; a.C1 = c1; a.rc_w = rc_w_packed; a.rc_b = rc_bias;
    return VDX_OK;
}
// vdx_resblock_tail and _ex: `r` is a tensor
static int tail_r(const char* who, const void* y2, int y2_bf16, const void* r, int r_bf16, void* out, int out_bf16, const double* stats,
                  const float* gn_gamma, const float* gn_beta, int groups, const float* ln_gamma, const float* ln_beta, int c, int batch,
                  long pix_per_sample, void* stream) {
    vdx::TailArgs a;
    if (int rc = tail_args(a, who, y2, y2_bf16, stats, gn_gamma, gn_beta, groups, ln_gamma, ln_beta, c, batch, pix_per_sample)) return rc;
    if (!r || !out) VDX_REFUSE(who, "null tensor");
    if (c % 4 || c > 1024) VDX_REFUSE(who, "c must be a multiple of 4 up to 1024");
    if ((y2_bf16 || r_bf16 || out_bf16) && c % 8) VDX_REFUSE(who, "bf16 tensors need c % 8 == 0");
    a.r = (const float*)r; a.r_bf16 = r_bf16 ? 1 : 0; a.out = (float*)out; a.out_bf16 = out_bf16 ? 1 : 0;
    VDX_HIP(vdx::launch_resblock_tail(a, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_resblock_tail(const float* y2, const float* r, float* out, const double* stats, const float* gn_gamma,
                      const float* gn_beta, int groups, const float* ln_gamma, const float* ln_beta, int c, int batch,
                      long pix_per_sample, void* stream) {
    return tail_r("resblock_tail", y2, 0, r, 0, out, 0, stats, gn_gamma, gn_beta, groups, ln_gamma, ln_beta, c, batch, pix_per_sample, stream);
}

int vdx_resblock_tail_rc_bf16(const void* y2, const void* x0, const void* x1, int c0, int c1, const void* rc_w_packed,
                              const float* rc_bias, void* out, const double* stats, const float* gn_gamma, const float* gn_beta,
                              int groups, const float* ln_gamma, const float* ln_beta, int c, int batch, long pix_per_sample,
                              void* stream) {
    const char* who = "resblock_tail_rc_bf16";
    vdx::TailArgs a;
    if (int rc = tail_args(a, who, y2, 1, stats, gn_gamma, gn_beta, groups, ln_gamma, ln_beta, c, batch, pix_per_sample)) return rc;
    if (!out) VDX_REFUSE(who, "null tensor");
    if (int rc = tail_rc_args(a, who, x0, x1, c0, c1, rc_w_packed, rc_bias)) return rc;
    a.out = (float*)out;
    VDX_HIP(vdx::launch_resblock_tail(a, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_gn_silu_apply_bf16(void* y, const double* stats, const float* gn_gamma, const float* gn_beta, const float* scale_shift,
                           int ss_stride, int groups, int c, int batch, long pix_per_sample, void* stream) {
    if (!y || !stats || !gn_gamma || !gn_beta) VDX_FAIL(VDX_ERR_INVALID, "gn_silu_apply: null tensor");
    if (batch < 1 || pix_per_sample < 1 || c < 8 || c % 8 || c > 1024 || groups <= 0 || groups > 32 || c % groups || (scale_shift && ss_stride < 2 * c))
        VDX_FAIL(VDX_ERR_INVALID, "gn_silu_apply: shape not served");
    VDX_HIP(vdx::launch_gn_silu_apply16((float*)y, stats, gn_gamma, gn_beta, scale_shift, ss_stride, groups, c, batch, pix_per_sample, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_init_conv(const float* x, const float* kernel, const float* bias, float* y, int batch, int cin, int frames,
                  int h, int w, int cout, int k, void* stream) {
    if (!x || !kernel || !bias || !y) VDX_FAIL(VDX_ERR_INVALID, "init_conv: null tensor");
    if (k < 1 || k > 15 || !(k & 1) || cin < 1 || cin > 8) VDX_FAIL(VDX_ERR_INVALID, "init_conv: bad kernel size / channels");
    VDX_HIP(vdx::launch_init_conv(x, kernel, bias, y, batch, cin, frames, h, w, cout, k, 0, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_final_conv(const float* x, const float* kernel, const float* bias, float* y, long npix, int d, int cout, void* stream) {
    if (!x || !kernel || !bias || !y || d % 4) VDX_FAIL(VDX_ERR_INVALID, "final_conv: bad argument");
    VDX_HIP(vdx::launch_final_conv(x, kernel, bias, y, npix, d, cout, 0, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_time_mlp(const int* time, const float* w1, const float* b1, const float* w2, const float* b2, int dim,
                 const float* cond, const float* null_cond_emb, const unsigned char* cond_mask, int null_all, int cond_dim,
                 float* temb, int batch, void* stream) {
    if (!time || !w1 || !b1 || !w2 || !b2 || !temb || dim < 4 || (dim % 4)) VDX_FAIL(VDX_ERR_INVALID, "time_mlp: bad argument (dim must be a multiple of 4; Unet3D itself needs dim % 8 == 0)");
    if (cond_dim && (!cond || !null_cond_emb)) VDX_FAIL(VDX_ERR_INVALID, "time_mlp: cond missing");
    vdx::TimeMlpArgs a;
    memset(&a, 0, sizeof(a));
    a.time = time; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.dim = dim; a.time_dim = 4 * dim;
    a.cond = cond; a.null_cond_emb = null_cond_emb; a.cond_mask = cond_mask; a.null_all = null_all; a.cond_dim = cond_dim;
    a.temb = temb; a.temb_dim = 4 * dim + cond_dim;
    VDX_HIP(vdx::launch_time_mlp(a, batch, (hipStream_t)stream));
    return VDX_OK;
}

// ---- the attention block forward.  What its eight entries share: the rules of the block's kernels and the arguments every route reads,
// the token geometry as the network builds it (attn_token_geometry).  fused_only: the entries of the fused kernels (<= 64 tokens); else the
// route decides (attention_block_forward)
static int attn_args(vdx::AttnArgs& a, const char* who, int mode, const void* x, void* y, int io_bf16, const void* wqkv_packed, const float* bqkv,
                     const void* wo_packed, const float* bo, int batch, int frames, int h, int w, int c, int heads, int temporal, bool fused_only) {
    if (!x || !y || !wqkv_packed || !bqkv || !wo_packed || !bo) VDX_REFUSE(who, "null tensor");
    if (!mode_ok(mode)) VDX_REFUSE(who, "bad mode");
    if (io_bf16 && mode != VDX_MODE_BF16) VDX_REFUSE(who, "bf16 tensors need VDX_MODE_BF16");
    if (batch < 1 || frames < 1 || h < 1 || w < 1 || heads < 1 || c < 4 || c % (io_bf16 ? 8 : 4) || c > 1024)
        VDX_REFUSE(who, "batch, frames, h, w and heads must be >= 1 and C a multiple of 4 (8 for bf16 tensors) up to 1024");
    memset(&a, 0, sizeof(a));
    a.x = reinterpret_cast<const float*>(x); a.y = reinterpret_cast<float*>(y); a.io_bf16 = io_bf16 ? 1 : 0;
    a.wqkv = wqkv_packed; a.bqkv = bqkv; a.wo = wo_packed; a.bo = bo; a.C = c; a.heads = heads;
    a.scale = 1.0f / sqrtf(32.0f);
    vdx::attn_token_geometry(a, batch, frames, h, w, c, temporal != 0);
    if (fused_only && a.L > 64) VDX_REFUSE(who, "more than 64 tokens per sequence is not supported");
    return VDX_OK;
}

// vdx_attention_forward, _ex and _bf16: the fused kernels, on fp32 or bf16 tensors, with or without the fp8 core
static int attn_fused(const char* who, int mode, const void* x, void* y, int io_bf16, const void* wqkv_packed, const float* bqkv, const void* wo_packed,
                      const float* bo, int batch, int frames, int h, int w, int c, int heads, int temporal, int fp8_core, void* stream) {
    if (fp8_core && mode != VDX_MODE_BF16) VDX_REFUSE(who, "the fp8 core needs VDX_MODE_BF16");
    vdx::AttnArgs a;
    if (int rc = attn_args(a, who, mode, x, y, io_bf16, wqkv_packed, bqkv, wo_packed, bo, batch, frames, h, w, c, heads, temporal, true)) return rc;
    a.fp8_core = fp8_core ? 1 : 0;
    VDX_HIP(vdx::launch_attention(mode, a, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_attention_forward(int mode, const float* x, float* y, const void* wqkv_packed, const float* bqkv,
                          const void* wo_packed, const float* bo, int batch, int frames, int h, int w, int c, int heads,
                          int temporal, void* stream) {
    return attn_fused("attention_forward", mode, x, y, 0, wqkv_packed, bqkv, wo_packed, bo, batch, frames, h, w, c, heads, temporal, 0, stream);
}

int vdx_attention_forward_ex(int mode, const float* x, float* y, const void* wqkv_packed, const float* bqkv,
                             const void* wo_packed, const float* bo, int batch, int frames, int h, int w, int c, int heads,
                             int temporal, int fp8_core, void* stream) {
    return attn_fused("attention_forward_ex", mode, x, y, 0, wqkv_packed, bqkv, wo_packed, bo, batch, frames, h, w, c, heads, temporal, fp8_core, stream);
}

int vdx_attention_forward_bf16(const void* x_bf16, void* y_bf16, const void* wqkv_packed, const float* bqkv,
                               const void* wo_packed, const float* bo, int batch, int frames, int h, int w, int c, int heads,
                               int temporal, int fp8_core, void* stream) {
    return attn_fused("attention_forward_bf16", VDX_MODE_BF16, x_bf16, y_bf16, 1, wqkv_packed, bqkv, wo_packed, bo, batch, frames, h, w, c, heads, temporal,
                      fp8_core, stream);
}

int vdx_attention_forward_bias(int mode, const void* x, void* y, int io_bf16, const void* wqkv_packed, const float* bqkv,
                               const void* wo_packed, const float* bo, const float* bias, int batch, int frames, int h, int w, int c,
                               int heads, int temporal, void* stream) {
    const char* who = "attention_forward_bias";
    vdx::AttnArgs a;
    if (int rc = attn_args(a, who, mode, x, y, io_bf16, wqkv_packed, bqkv, wo_packed, bo, batch, frames, h, w, c, heads, temporal, true)) return rc;
    if (!bias) VDX_REFUSE(who, "null tensor");
    a.pos_bias = bias;
    // the route of the network's temporal blocks with the switch on (model.hip: attention_block_forward)
    VDX_HIP(vdx::attention_block_forward(mode, a, temporal != 0, batch * frames, frames, h, w, nullptr, 0, vdx::ATTN_ANY, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_attention_forward_focus(int mode, const void* x, void* y, int io_bf16, const void* wqkv_packed, const float* bqkv,
                                const void* wo_packed, const float* bo, const float* bias_or_null, const unsigned char* focus_dev, int focus_n,
                                int batch, int frames, int h, int w, int c, int heads, int temporal, void* stream) {
    const char* who = "attention_forward_focus";
    vdx::AttnArgs a;
    if (int rc = attn_args(a, who, mode, x, y, io_bf16, wqkv_packed, bqkv, wo_packed, bo, batch, frames, h, w, c, heads, temporal, true)) return rc;
    if (!focus_dev || focus_n < 1) VDX_REFUSE(who, "null or empty mask");
    a.pos_bias = bias_or_null; a.focus = focus_dev; a.focus_n = focus_n;
    // the route of the network's masked temporal blocks under vdx_set_focus_present(mode 2) (model.hip: attention_block_forward)
    VDX_HIP(vdx::attention_block_forward(mode, a, temporal != 0, batch * frames, frames, h, w, nullptr, 0, vdx::ATTN_ANY, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_attention_present_forward(int mode, const void* x, void* y, int io_bf16, const void* wqkv_packed, const float* bqkv,
                                  const void* wo_packed, const float* bo, int batch, int frames, int h, int w, int c, int heads, int temporal,
                                  void* stream) {
    vdx::AttnArgs a;
    if (int rc = attn_args(a, "attention_present_forward", mode, x, y, io_bf16, wqkv_packed, bqkv, wo_packed, bo, batch, frames, h, w, c, heads, temporal, false)) return rc;
    a.present = 1;
    // the route of the network's temporal blocks under vdx_set_focus_present(mode 1)
    VDX_HIP(vdx::attention_block_forward(mode, a, temporal != 0, batch * frames, frames, h, w, nullptr, 0, vdx::ATTN_ANY, (hipStream_t)stream));
    return VDX_OK;
}

// ---- forward forms of the network (vdx.h: "Forward forms of the network"): the compositions and flags model.hip sets ----------------

size_t vdx_attention_heads_scratch_bytes(int batch, int frames, int h, int w) { return (size_t)batch * frames * h * w * 8 * 32 * 2; }
size_t vdx_attention_long_scratch_bytes(int batch, int frames, int h, int w, int heads) {
    return (size_t)batch * frames * h * w * heads * 32 * 4 * sizeof(float);
}

int vdx_attention_heads_forward(const void* x, void* y, int io_bf16, const void* wqkv_packed, const float* bqkv, const void* wo_packed,
                                const float* bo, void* o_scratch, size_t o_scratch_bytes, int batch, int frames, int h, int w, int c,
                                int temporal, int fp8_core, void* stream) {
    const char* who = "attention_heads_forward";
    vdx::AttnArgs a;
    if (int rc = attn_args(a, who, VDX_MODE_BF16, x, y, io_bf16, wqkv_packed, bqkv, wo_packed, bo, batch, frames, h, w, c, 8, temporal, false)) return rc;
    if (!o_scratch) VDX_REFUSE(who, "null tensor");
    if (c % 8) VDX_REFUSE(who, "C must be a multiple of 8");
    a.fp8_core = fp8_core ? 1 : 0;
    const hipError_t e = vdx::attention_block_forward(VDX_MODE_BF16, a, temporal != 0, batch * frames, frames, h, w, o_scratch, o_scratch_bytes,
                                                      vdx::ATTN_HEADS, (hipStream_t)stream);
    if (e == hipErrorInvalidValue) VDX_REFUSE(who, "the network does not run this shape on the per-head kernel");
    VDX_HIP(e);
    return VDX_OK;
}

int vdx_attention_long_forward(int mode, const void* x, void* y, int io_bf16, const void* wqkv_packed, const float* bqkv,
                               const void* wo_packed, const float* bo, void* scratch, size_t scratch_bytes, int batch, int frames, int h,
                               int w, int c, int heads, void* stream) {
    const char* who = "attention_long_forward";
    vdx::AttnArgs a;
    if (int rc = attn_args(a, who, mode, x, y, io_bf16, wqkv_packed, bqkv, wo_packed, bo, batch, frames, h, w, c, heads, 0, false)) return rc;
    if (!scratch) VDX_REFUSE(who, "null tensor");
    const hipError_t e = vdx::attention_block_forward(mode, a, false, batch * frames, frames, h, w, scratch, scratch_bytes, vdx::ATTN_LONG, (hipStream_t)stream);
    if (e == hipErrorInvalidValue) VDX_REFUSE(who, "needs more than 64 tokens per frame and vdx_attention_long_scratch_bytes of scratch");
    VDX_HIP(e);
    return VDX_OK;
}

// ---- the SpatialLinearAttention block forward.  What its three entries share: 8 heads x 32 and the rules of the SLA kernels
size_t vdx_sla_workspace_bytes(int mode, int nframes, int npix, int heads) { return vdx::sla_workspace_bytes(mode, nframes, npix, heads); }

static int sla_args(vdx::SlaArgs& a, const char* who, int mode, const void* x, void* y, int io_bf16, const void* wq_packed, const void* wk_packed,
                    const void* wv_packed, const void* wo_packed, int batch, int frames, int h, int w, int c, int heads) {
    if (!x || !y || !wq_packed || !wk_packed || !wv_packed || !wo_packed) VDX_REFUSE(who, "null tensor");
    if (!mode_ok(mode)) VDX_REFUSE(who, "bad mode");
    if (batch < 1 || frames < 1 || h < 1 || w < 1 || heads != 8 || c < 4 || c % (io_bf16 ? 8 : 4) || c > 1024)
        VDX_REFUSE(who, "batch, frames, h and w must be >= 1, heads 8 and C a multiple of 4 (8 for bf16 tensors) up to 1024");
    memset(&a, 0, sizeof(a));
    a.x = reinterpret_cast<const float*>(x); a.y = reinterpret_cast<float*>(y); a.io_bf16 = io_bf16 ? 1 : 0;
    a.wq = wq_packed; a.wk = wk_packed; a.wv = wv_packed; a.wo = wo_packed;
    a.C = c; a.heads = heads; a.NF = batch * frames; a.N = h * w;
    return VDX_OK;
}

// vdx_sla_forward and _bf16: the generic kernels on fp32 or bf16 tensors
static int sla_generic(const char* who, int mode, const void* x, void* y, int io_bf16, const void* wq_packed, const void* wk_packed, const void* wv_packed,
                       const void* wo_packed, void* workspace, int batch, int frames, int h, int w, int c, int heads, void* stream) {
    vdx::SlaArgs a;
    if (int rc = sla_args(a, who, mode, x, y, io_bf16, wq_packed, wk_packed, wv_packed, wo_packed, batch, frames, h, w, c, heads)) return rc;
    if (!workspace) VDX_REFUSE(who, "null tensor");
    a.workspace = workspace;
    VDX_HIP(vdx::launch_sla(mode, a, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_sla_forward(int mode, const float* x, float* y, const void* wq_packed, const void* wk_packed, const void* wv_packed,
                    const void* wo_packed, void* workspace, int batch, int frames, int h, int w, int c, int heads, void* stream) {
    return sla_generic("sla_forward", mode, x, y, 0, wq_packed, wk_packed, wv_packed, wo_packed, workspace, batch, frames, h, w, c, heads, stream);
}

int vdx_sla_forward_bf16(const void* x_bf16, void* y_bf16, const void* wq_packed, const void* wk_packed, const void* wv_packed,
                         const void* wo_packed, void* workspace, int batch, int frames, int h, int w, int c, int heads, void* stream) {
    return sla_generic("sla_forward_bf16", VDX_MODE_BF16, x_bf16, y_bf16, 1, wq_packed, wk_packed, wv_packed, wo_packed, workspace, batch, frames, h, w, c, heads, stream);
}

int vdx_sla_heads_forward(const void* x, void* y, int io_bf16, const void* wq_packed, const void* wk_packed, const void* wv_packed,
                          const void* wo_packed, void* o_scratch, size_t o_scratch_bytes, int batch, int frames, int h, int w, int c,
                          void* stream) {
    const char* who = "sla_heads_forward";
    vdx::SlaArgs a;
    if (int rc = sla_args(a, who, VDX_MODE_BF16, x, y, io_bf16, wq_packed, wk_packed, wv_packed, wo_packed, batch, frames, h, w, c, 8)) return rc;
    if (!o_scratch) VDX_REFUSE(who, "null tensor");
    if (c % 8) VDX_REFUSE(who, "C must be a multiple of 8");
    const hipError_t e = vdx::sla_block_forward(VDX_MODE_BF16, a, frames, h, w, o_scratch, o_scratch_bytes, vdx::ATTN_HEADS, (hipStream_t)stream);
    if (e == hipErrorInvalidValue) VDX_REFUSE(who, "the network does not run this shape on the per-head kernel");
    VDX_HIP(e);
    return VDX_OK;
}

int vdx_resblock_tail_ex(const void* y2, int y2_bf16, const void* r, int r_bf16, void* out, int out_bf16, const double* stats,
                         const float* gn_gamma, const float* gn_beta, int groups, const float* ln_gamma, const float* ln_beta, int c,
                         int batch, long pix_per_sample, void* stream) {
    return tail_r("resblock_tail_ex", y2, y2_bf16, r, r_bf16, out, out_bf16, stats, gn_gamma, gn_beta, groups, ln_gamma, ln_beta, c, batch, pix_per_sample, stream);
}

int vdx_resblock_tail_rc_head_bf16(const void* y2, const void* x0, const void* x1, int c0, int c1, const void* rc_w_packed,
                                   const float* rc_bias, const double* stats, const float* gn_gamma, const float* gn_beta, int groups,
                                   const float* ln_gamma, const float* ln_beta, int c, const float* fin_w, const float* fin_b,
                                   float* fin_out, int batch, long pix_per_sample, void* stream) {
    const char* who = "resblock_tail_rc_head_bf16";
    vdx::TailArgs a;
    if (int rc = tail_args(a, who, y2, 1, stats, gn_gamma, gn_beta, groups, ln_gamma, ln_beta, c, batch, pix_per_sample)) return rc;
    if (!x1 || !fin_w || !fin_b || !fin_out) VDX_REFUSE(who, "null tensor");
    if (c1 != c0 || !((c0 + c1 == 128 && c == 64) || (c0 + c1 == 64 && c == 32))) VDX_REFUSE(who, "shape not served");
    if (int rc = tail_rc_args(a, who, x0, x1, c0, c1, rc_w_packed, rc_bias)) return rc;
    a.fin_w = fin_w; a.fin_b = fin_b; a.fin_out = fin_out;
    VDX_HIP(vdx::launch_resblock_tail(a, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_final_conv_ex(const void* x, int x_bf16, const float* kernel, const float* bias, float* y, long npix, int d, int cout,
                      void* stream) {
    if (!x || !kernel || !bias || !y || npix < 1 || cout < 1 || d % (x_bf16 ? 8 : 4)) VDX_FAIL(VDX_ERR_INVALID, "final_conv: bad argument");
    VDX_HIP(vdx::launch_final_conv((const float*)x, kernel, bias, y, npix, d, cout, x_bf16 ? 1 : 0, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_init_conv_ex(int mode, const float* x, const float* kernel, const float* bias, void* y, int y_bf16, int batch, int cin,
                     int frames, int h, int w, int cout, int k, void* stream) {
    if (!x || !kernel || !bias || !y) VDX_FAIL(VDX_ERR_INVALID, "init_conv: null tensor");
    if (mode != VDX_MODE_F32 && mode != VDX_MODE_BF16) VDX_FAIL(VDX_ERR_INVALID, "init_conv: bad mode");
    if (k < 1 || k > 15 || !(k & 1) || cin < 1 || cin > 8 || cout % 4) VDX_FAIL(VDX_ERR_INVALID, "init_conv: bad kernel size / channels");
    if (y_bf16 && mode != VDX_MODE_BF16) VDX_FAIL(VDX_ERR_INVALID, "init_conv: a bf16 output needs VDX_MODE_BF16");
    VDX_HIP(vdx::launch_init_conv_mode(mode, x, kernel, bias, (float*)y, batch, cin, frames, h, w, cout, k, y_bf16 ? 1 : 0, (hipStream_t)stream));
    return VDX_OK;
}

static_assert(sizeof(vdx_ss_layer) == sizeof(vdx::SsLayer) && offsetof(vdx_ss_layer, n) == offsetof(vdx::SsLayer, n) &&
              offsetof(vdx_ss_layer, out_off) == offsetof(vdx::SsLayer, out_off), "vdx_ss_layer mirrors SsLayer");

int vdx_resblock_scale_shift(const float* params, const float* temb, const vdx_ss_layer* layers_dev, int nlayers, float* ss, float* lin,
                             int temb_dim, int batch, int max_n, void* stream) {
    if (!params || !temb || !layers_dev || !ss || !lin) VDX_FAIL(VDX_ERR_INVALID, "scale_shift: null tensor");
    if (nlayers < 1 || temb_dim < 1 || batch < 1 || max_n < 1 || max_n > 2048 || (size_t)temb_dim * 8 * 4 + 8192 > 64 * 1024)      // (the Linear's LDS: 8 samples of temb + the partial sums)
        VDX_FAIL(VDX_ERR_INVALID, "scale_shift: bad geometry");
    VDX_HIP(vdx::launch_resblock_ss(params, temb, reinterpret_cast<const vdx::SsLayer*>(layers_dev), nlayers, ss, lin, temb_dim, batch, max_n,
                                    (hipStream_t)stream));
    return VDX_OK;
}

int vdx_create(const vdx_config* cfg, vdx_handle** out) {
    if (!cfg || !out) VDX_FAIL(VDX_ERR_INVALID, "create: null argument");
    if (!mode_ok(cfg->mode)) VDX_FAIL(VDX_ERR_INVALID, "bad mode");
    vdx_handle* h = new vdx_handle();
    h->model.cfg = *cfg;
    int rc = vdx::model_build(&h->model);
    if (rc != VDX_OK) { delete h; return rc; }
    // the only device memory the handle owns: the small ResnetBlock time-MLP table
    const size_t tb = h->model.ss_layers.size() * sizeof(vdx::SsLayer);
    if (tb) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
            hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->model.d_ss_layers), tb);
            if (e == hipSuccess) e = hipMemcpy(h->model.d_ss_layers, h->model.ss_layers.data(), tb, hipMemcpyHostToDevice);
            if (e != hipSuccess) { delete h; return vdx_set_error(VDX_ERR_HIP, hipGetErrorString(e), __FILE__, __LINE__); }
            vdx::model_build_pack_tables(&h->model);
            for (int k = 0; k < 2 && e == hipSuccess; ++k) {
                const std::vector<vdx::PackJob>& v = k ? h->model.pack_t_jobs : h->model.pack_jobs;
                vdx::PackJob** d = k ? &h->model.d_pack_t_jobs : &h->model.d_pack_jobs;
                e = hipMalloc(reinterpret_cast<void**>(d), v.size() * sizeof(vdx::PackJob));
                if (e == hipSuccess) e = hipMemcpy(*d, v.data(), v.size() * sizeof(vdx::PackJob), hipMemcpyHostToDevice);
            }
            if (e != hipSuccess) { vdx_destroy(h); return vdx_set_error(VDX_ERR_HIP, hipGetErrorString(e), __FILE__, __LINE__); }
        }   // without a device the handle still serves the layout queries (CPU-side tests)
    }
    *out = h;
    return VDX_OK;
}

void vdx_destroy(vdx_handle* h) {
    if (!h) return;
    h->drop_graphs();
    vdx::comm_destroy(&h->comm);
    vdx::bwd_state_free(&h->bwd);
    free_pos_bias(h->model);
    if (h->model.d_focus_ones) (void)hipFree(h->model.d_focus_ones);
    if (h->model.d_ss_layers) (void)hipFree(h->model.d_ss_layers);
    if (h->model.d_pack_jobs) (void)hipFree(h->model.d_pack_jobs);
    if (h->model.d_pack_t_jobs) (void)hipFree(h->model.d_pack_t_jobs);
    delete h;
}

int vdx_set_activation_storage(vdx_handle* h, int bf16) {
    if (!h) VDX_FAIL(VDX_ERR_INVALID, "set_activation_storage: null handle");
    if (bf16 && h->model.mode != VDX_MODE_BF16) VDX_FAIL(VDX_ERR_INVALID, "bf16 activation storage needs a VDX_MODE_BF16 handle");
    if (bf16 < 0 || bf16 > 2) VDX_FAIL(VDX_ERR_INVALID, "set_activation_storage: 0 (fp32), 1 (bf16, inference) or 2 (bf16, training forward)");
    const int v = bf16;
    if (v != h->model.act16) {                       // a cached sampling graph was captured with the other storage
        h->drop_graphs();
        h->model.act16 = v;
    }
    return VDX_OK;
}
int vdx_get_activation_storage(const vdx_handle* h) { return h ? h->model.act16 : 0; }

int vdx_set_attention_fp8(vdx_handle* h, int on) {
    if (!h) VDX_FAIL(VDX_ERR_INVALID, "set_attention_fp8: null handle");
    if (on && h->model.mode != VDX_MODE_BF16) VDX_FAIL(VDX_ERR_INVALID, "fp8 attention needs a VDX_MODE_BF16 handle");
    if (on && h->model.pos_bias) VDX_FAIL(VDX_ERR_STATE, "set_attention_fp8: fp8 attention and the temporal position bias exclude each other (the fp8 cores have no bias form)");
    if (on && h->model.focus) VDX_FAIL(VDX_ERR_STATE, "set_attention_fp8: fp8 attention and focus-present exclude each other (the fp8 cores have no mask form)");
    const int v = on ? 1 : 0;
    if (v != h->model.attn_fp8) { h->drop_graphs(); h->model.attn_fp8 = v; }
    return VDX_OK;
}
int vdx_get_attention_fp8(const vdx_handle* h) { return h ? h->model.attn_fp8 : 0; }

static void free_pos_bias(vdx::Model& m) {
    if (m.d_pos_buckets) { (void)hipFree(m.d_pos_buckets); m.d_pos_buckets = nullptr; }
    if (m.d_pos_table) { (void)hipFree(m.d_pos_table); m.d_pos_table = nullptr; }
    if (m.d_pos_dbias) { (void)hipFree(m.d_pos_dbias); m.d_pos_dbias = nullptr; }
}

int vdx_set_temporal_pos_bias(vdx_handle* h, int on, const int* buckets) {
    if (!h) VDX_FAIL(VDX_ERR_INVALID, "set_temporal_pos_bias: null handle");
    vdx::Model& m = h->model;
    if (!on) {
        if (m.pos_bias) { h->drop_graphs(); m.pos_bias = 0; }
        return VDX_OK;
    }
    if (m.attn_fp8) VDX_FAIL(VDX_ERR_STATE, "set_temporal_pos_bias: the temporal position bias and fp8 attention exclude each other (the fp8 cores have no bias form)");
    const int F = m.cfg.num_frames;
    if (F < 1 || F > 64) VDX_FAIL(VDX_ERR_INVALID, "set_temporal_pos_bias: 1..64 frames");
    if (!buckets) VDX_FAIL(VDX_ERR_INVALID, "set_temporal_pos_bias: null bucket map");
    for (int i = 0; i < F * F; ++i) if (buckets[i] < 0 || buckets[i] >= 32) VDX_FAIL(VDX_ERR_INVALID, "set_temporal_pos_bias: bucket outside [0, 32)");
    if (!m.d_ss_layers) VDX_FAIL(VDX_ERR_STATE, "set_temporal_pos_bias: handle was created without a GPU");
    h->drop_graphs();                                // (also: no replay of this handle is in flight while the map is rewritten)
    m.pos_bias = 0;
    const size_t nb = (size_t)F * F * sizeof(int), nt = (size_t)m.cfg.attn_heads * F * F * sizeof(float);
    hipError_t e = hipSuccess;
    if (!m.d_pos_buckets) e = hipMalloc(reinterpret_cast<void**>(&m.d_pos_buckets), nb);
    if (e == hipSuccess && !m.d_pos_table) e = hipMalloc(reinterpret_cast<void**>(&m.d_pos_table), nt);
    if (e == hipSuccess && !m.d_pos_dbias) e = hipMalloc(reinterpret_cast<void**>(&m.d_pos_dbias), nt);
    if (e == hipSuccess) e = hipMemcpy(m.d_pos_buckets, buckets, nb, hipMemcpyHostToDevice);
    if (e != hipSuccess) { free_pos_bias(m); return vdx_set_error(VDX_ERR_HIP, hipGetErrorString(e), __FILE__, __LINE__); }
    m.pos_bias = 1;
    return VDX_OK;
}
int vdx_get_temporal_pos_bias(const vdx_handle* h) { return h ? h->model.pos_bias : 0; }

int vdx_set_focus_present(vdx_handle* h, int mode, const unsigned char* mask_dev, int n) {
    if (!h) VDX_FAIL(VDX_ERR_INVALID, "set_focus_present: null handle");
    vdx::Model& m = h->model;
    if (mode < 0 || mode > 2) VDX_FAIL(VDX_ERR_INVALID, "set_focus_present: mode 0 (off), 1 (every sample) or 2 (per-sample mask)");
    if (mode == 0) {
        if (m.focus) { h->drop_graphs(); m.focus = 0; m.focus_mask = nullptr; m.focus_n = 0; }
        return VDX_OK;
    }
    if (m.attn_fp8) VDX_FAIL(VDX_ERR_STATE, "set_focus_present: focus-present and fp8 attention exclude each other (the fp8 cores have no mask form)");
    if (m.cfg.num_frames < 1 || m.cfg.num_frames > 64) VDX_FAIL(VDX_ERR_INVALID, "set_focus_present: 1..64 frames");
    if (mode == 2 && (!mask_dev || n < 1)) VDX_FAIL(VDX_ERR_INVALID, "set_focus_present: mode 2 needs a device mask of n >= 1 bytes");
    if (!m.d_ss_layers) VDX_FAIL(VDX_ERR_STATE, "set_focus_present: handle was created without a GPU");
    if (mode == 1) { mask_dev = nullptr; n = 0; }
    if (mode == m.focus && mask_dev == m.focus_mask && n == m.focus_n) return VDX_OK;
    if (!m.d_focus_ones) {                           // the one-byte all-ones mask of the backward of an all-present batch (read as focus[r % 1])
        const unsigned char one = 1;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&m.d_focus_ones), 16);
        if (e == hipSuccess) e = hipMemcpy(m.d_focus_ones, &one, 1, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (m.d_focus_ones) { (void)hipFree(m.d_focus_ones); m.d_focus_ones = nullptr; }
            return vdx_set_error(VDX_ERR_HIP, hipGetErrorString(e), __FILE__, __LINE__);
        }
    }
    h->drop_graphs();                                // a cached sampling graph holds the other route's kernels / the other pointer
    m.focus = mode; m.focus_mask = mask_dev; m.focus_n = n;
    return VDX_OK;
}
int vdx_get_focus_present(const vdx_handle* h) { return h ? h->model.focus : 0; }

int vdx_set_prediction(vdx_handle* h, int kind, const float* sqrt_ac, const float* sqrt_1mac, int timesteps) {
    if (!h) VDX_FAIL(VDX_ERR_INVALID, "set_prediction: null handle");
    if (kind != 0 && kind != 1) VDX_FAIL(VDX_ERR_INVALID, "set_prediction: kind 0 (eps) or 1 (v)");
    if (kind == 1 && (!sqrt_ac || !sqrt_1mac || timesteps < 1)) VDX_FAIL(VDX_ERR_INVALID, "set_prediction: kind 1 needs both tables and timesteps >= 1");
    // (no graph is dropped: kind and the two pointers are part of every loop's graph key, so a change re-captures)
    h->pred = kind; h->pred_sa = kind ? sqrt_ac : nullptr; h->pred_s1 = kind ? sqrt_1mac : nullptr; h->pred_T = kind ? timesteps : 0;
    return VDX_OK;
}
int vdx_get_prediction(const vdx_handle* h) { return h ? h->pred : 0; }

int vdx_set_self_condition(vdx_handle* h, int on, const float* tables, int timesteps) {
    if (!h) VDX_FAIL(VDX_ERR_INVALID, "set_self_condition: null handle");
    if (on != 0 && on != 1) VDX_FAIL(VDX_ERR_INVALID, "set_self_condition: on is 0 or 1");
    if (on && (!tables || timesteps < 1)) VDX_FAIL(VDX_ERR_INVALID, "set_self_condition: on = 1 needs the step tables and timesteps >= 1");
    // (no graph is dropped: the state is part of every loop's graph key, so a step captured under another state is not replayed)
    h->sc = on; h->sc_tab = on ? tables : nullptr; h->sc_T = on ? timesteps : 0;
    return VDX_OK;
}

int vdx_get_self_condition(const vdx_handle* h) { return h ? h->sc : 0; }

int vdx_param_count(const vdx_handle* h) { return h ? (int)h->model.params.size() : 0; }
long vdx_param_total(const vdx_handle* h) { return h ? h->model.param_total : 0; }

int vdx_param_info(const vdx_handle* h, int index, char* name, int name_cap, int* ndim, long shape[6], long* offset) {
    if (!h || index < 0 || index >= (int)h->model.params.size()) VDX_FAIL(VDX_ERR_INVALID, "param_info: bad index");
    const vdx::ParamInfo& p = h->model.params[index];
    if (name && name_cap > 0) snprintf(name, name_cap, "%s", p.name.c_str());
    if (ndim) *ndim = p.ndim;
    if (shape) for (int i = 0; i < 6; ++i) shape[i] = i < p.ndim ? p.shape[i] : 1;
    if (offset) *offset = p.offset;
    return VDX_OK;
}

size_t vdx_packed_bytes(const vdx_handle* h) { return h ? h->model.packed_bytes : 0; }

int vdx_pack_params(const vdx_handle* h, const float* params, void* packed, void* stream) {
    if (!h || !params || !packed) VDX_FAIL(VDX_ERR_INVALID, "pack_params: null argument");
    VDX_HIP(vdx::model_pack(&h->model, params, packed, (hipStream_t)stream));
    return VDX_OK;
}

size_t vdx_workspace_bytes(const vdx_handle* h, int batch) { return h ? vdx::model_workspace_bytes(&h->model, batch) : 0; }
int vdx_slot_count(const vdx_handle* h) { return h ? (int)h->model.slots.size() : 0; }

int vdx_slot_info(const vdx_handle* h, int index, char* name, int name_cap, long* floats_per_sample, long* float_offset_per_sample) {
    if (!h || index < 0 || index >= (int)h->model.slots.size()) VDX_FAIL(VDX_ERR_INVALID, "slot_info: bad index");
    const vdx::Slot& s = h->model.slots[index];
    if (name && name_cap > 0) snprintf(name, name_cap, "%s", s.name.c_str());
    if (floats_per_sample) *floats_per_sample = s.floats_per_sample;
    if (float_offset_per_sample) *float_offset_per_sample = s.offset_per_sample;
    return VDX_OK;
}

int vdx_unet_forward(const vdx_handle* h, const float* params, const void* packed, const float* x, const int* time,
                     const float* cond, const unsigned char* cond_mask, int null_all, float* out, void* workspace,
                     size_t workspace_bytes, int batch, void* stream) {
    if (!h || !params || !packed || !x || !time || !out || !workspace) VDX_FAIL(VDX_ERR_INVALID, "unet_forward: null argument");
    if (!h->model.d_ss_layers) VDX_FAIL(VDX_ERR_STATE, "unet_forward: handle was created without a GPU");
    return vdx::model_forward(&h->model, params, packed, x, time, cond, cond_mask, null_all, out, workspace, workspace_bytes, batch,
                              (hipStream_t)stream);
}

int vdx_randn(float* out, long n, uint64_t seed, uint64_t offset, const uint64_t* dev_offset, void* stream) {
    if (n == 0) return VDX_OK;
    if (!out || n < 0) VDX_FAIL(VDX_ERR_INVALID, "randn: bad argument");
    VDX_HIP(vdx::launch_randn(out, n, seed, offset, reinterpret_cast<const unsigned long long*>(dev_offset), (hipStream_t)stream));
    return VDX_OK;
}

int vdx_q_sample(const float* x_start, const int* t, const float* noise, float* out, const float* sqrt_ac,
                 const float* sqrt_one_minus_ac, int batch, long per_sample, float pre_scale, float pre_shift, void* stream) {
    if (!x_start || !t || !noise || !out || !sqrt_ac || !sqrt_one_minus_ac || batch < 1 || per_sample < 1) VDX_FAIL(VDX_ERR_INVALID, "q_sample: bad argument");
    if (per_sample % 4) VDX_FAIL(VDX_ERR_INVALID, "q_sample: per_sample must be a multiple of 4");
    VDX_HIP(vdx::launch_q_sample(x_start, t, noise, out, sqrt_ac, sqrt_one_minus_ac, batch, per_sample, pre_scale, pre_shift, (hipStream_t)stream));
    return VDX_OK;
}

static vdx::PSampleArgs psample_args(const float* x, const float* eps_hat, float* out, const int* t, const float* tables, int timesteps,
                                     const float* noise, uint64_t seed, uint64_t offset, const uint64_t* dev_offset, const float* thres,
                                     int clip, int channels, long per_sample) {
    vdx::PSampleArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.eps = eps_hat; a.out = out; a.t = t; a.tables = tables; a.T = timesteps; a.noise = noise;
    a.seed = seed; a.offset = offset; a.dev_offset = reinterpret_cast<const unsigned long long*>(dev_offset);
    a.thres = thres; a.clip = clip; a.C = channels; a.per_sample = per_sample; a.post_scale = 1.f; a.post_shift = 0.f;
    return a;
}

int vdx_p_sample_step(const float* x, const float* eps_hat, float* out, const int* t, const float* tables, int timesteps,
                      const float* noise, uint64_t seed, uint64_t offset, const uint64_t* dev_offset, const float* thres,
                      int clip_denoised, int batch, int channels, long per_sample, void* stream) {
    if (!x || !eps_hat || !out || !t || !tables || timesteps < 1 || batch < 1 || channels < 1) VDX_FAIL(VDX_ERR_INVALID, "p_sample: bad argument");
    if (per_sample % channels) VDX_FAIL(VDX_ERR_INVALID, "p_sample: per_sample must be a multiple of channels");
    if (!noise && per_sample % 4) VDX_FAIL(VDX_ERR_INVALID, "p_sample: generated noise needs per_sample % 4 == 0");
    const vdx::PSampleArgs a = psample_args(x, eps_hat, out, t, tables, timesteps, noise, seed, offset, dev_offset, thres, clip_denoised, channels, per_sample);
    VDX_HIP(vdx::launch_p_sample(a, batch, (hipStream_t)stream));
    return VDX_OK;
}

// a >= 0, b >= 0, both finite, a^2 + b^2 = 1 within 1e-5, by the bits of the floats (the library is built with -fno-honor-nans, under
// which a comparison may let a NaN through): the weights of the mixed noise
static bool mix_weights_ok(float a, float b) {
    unsigned ua, ub;
    memcpy(&ua, &a, sizeof(ua));
    memcpy(&ub, &b, sizeof(ub));
    if ((ua >= 0x7F800000u && ua != 0x80000000u) || (ub >= 0x7F800000u && ub != 0x80000000u)) return false;      // negative, inf or NaN
    const double d = (double)a * (double)a + (double)b * (double)b - 1.0;
    return d >= -1e-5 && d <= 1e-5;
}
#define VDX_MIX_WEIGHTS_RULE "a and b must be finite, >= 0 and a^2 + b^2 = 1 (within 1e-5)"

int vdx_randn_mixed(float* out, int batch, int channels, int frames, long hw, float a, float b, uint64_t seed, uint64_t draw,
                    const uint64_t* dev_draw, void* stream) {
    if (!out) VDX_FAIL(VDX_ERR_INVALID, "randn_mixed: null out");
    if (batch < 1 || channels < 1 || frames < 1 || hw < 1) VDX_FAIL(VDX_ERR_INVALID, "randn_mixed: batch, channels, frames and hw must be >= 1");
    if (!mix_weights_ok(a, b)) VDX_FAIL(VDX_ERR_INVALID, "randn_mixed: " VDX_MIX_WEIGHTS_RULE);
    if (draw >= VDX_DRAW_SHARED) VDX_FAIL(VDX_ERR_INVALID, "randn_mixed: draw must be below 2^60 (VDX_DRAW_SHARED)");
    if ((uintptr_t)out % 16) VDX_FAIL(VDX_ERR_INVALID, "randn_mixed: out must be 16-byte aligned");
    const vdx::MixArgs m = {frames, hw, a, b};
    VDX_HIP(vdx::launch_randn_mixed(out, batch, channels, m, seed, draw, reinterpret_cast<const unsigned long long*>(dev_draw), (hipStream_t)stream));
    return VDX_OK;
}

int vdx_p_sample_step_mixed(const float* x, const float* eps_hat, float* out, const int* t, const float* tables, int timesteps,
                            int frames, float a, float b, uint64_t seed, uint64_t offset, const uint64_t* dev_offset, const float* thres,
                            int clip_denoised, int batch, int channels, long per_sample, void* stream) {
    if (!x || !eps_hat || !out || !t || !tables || timesteps < 1 || batch < 1 || channels < 1 || frames < 1 || per_sample < 1)
        VDX_FAIL(VDX_ERR_INVALID, "p_sample_mixed: bad argument");
    if (per_sample % ((long)channels * frames)) VDX_FAIL(VDX_ERR_INVALID, "p_sample_mixed: per_sample must be a multiple of channels * frames");
    if (per_sample % 4) VDX_FAIL(VDX_ERR_INVALID, "p_sample_mixed: generated noise needs per_sample % 4 == 0");
    if (!mix_weights_ok(a, b)) VDX_FAIL(VDX_ERR_INVALID, "p_sample_mixed: " VDX_MIX_WEIGHTS_RULE);
    if (offset >= VDX_DRAW_SHARED) VDX_FAIL(VDX_ERR_INVALID, "p_sample_mixed: offset must be below 2^60 (VDX_DRAW_SHARED)");
    if ((uintptr_t)x % 16 || (uintptr_t)out % 16) VDX_FAIL(VDX_ERR_INVALID, "p_sample_mixed: x / out must be 16-byte aligned");
    const vdx::PSampleArgs pa = psample_args(x, eps_hat, out, t, tables, timesteps, nullptr, seed, offset, dev_offset, thres, clip_denoised, channels, per_sample);
    const vdx::MixArgs m = {frames, per_sample / ((long)channels * frames), a, b};
    VDX_HIP(vdx::launch_p_sample_mixed(pa, m, batch, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_loss_sum(const float* eps_hat, const float* noise, double* acc, int batch, int channels, long fhw, int l2, void* stream) {
    if (!eps_hat || !noise || !acc) VDX_FAIL(VDX_ERR_INVALID, "loss: null tensor");
    VDX_HIP(vdx::launch_loss(eps_hat, noise, acc, batch, channels, fhw, l2, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_affine(const float* x, float* y, long n, float a, float b, void* stream) {
    if (!x || !y || n < 0) VDX_FAIL(VDX_ERR_INVALID, "affine: bad argument");
    if (n) VDX_HIP(vdx::launch_affine(x, y, n, a, b, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_dynamic_threshold(const float* x, const float* eps_hat, const int* t, const float* tables, int timesteps, float percentile,
                          float* thres_out, int batch, int channels, long per_sample, void* stream) {
    if (!x || !eps_hat || !t || !tables || !thres_out || batch < 1 || channels < 1 || per_sample < 1) VDX_FAIL(VDX_ERR_INVALID, "dynamic_threshold: bad argument");
    if (!(percentile > 0.f && percentile <= 1.f) || per_sample % channels) VDX_FAIL(VDX_ERR_INVALID, "dynamic_threshold: percentile must be in (0, 1]");
    VDX_HIP(vdx::launch_dyn_thres(x, eps_hat, t, tables, timesteps, percentile, thres_out, batch, channels, per_sample, (hipStream_t)stream));
    return VDX_OK;
}

// the masked kernels move 16-byte float4 and 4-byte uchar4 vectors
static bool masked_aligned(const void* x, const void* known, const void* out, const void* mask) {
    return !((uintptr_t)x % 16 || (uintptr_t)known % 16 || (uintptr_t)out % 16 || (uintptr_t)mask % 4);
}

int vdx_inpaint_init(float* x, const float* known, const unsigned char* mask, const float* mask_tables, int timesteps, int t0,
                     long n, void* stream) {
    if (!x || !known || !mask || !mask_tables || timesteps < 1 || t0 < 0 || t0 >= timesteps || n < 0) VDX_FAIL(VDX_ERR_INVALID, "inpaint_init: bad argument");
    if (n % 4) VDX_FAIL(VDX_ERR_INVALID, "inpaint_init: n must be a multiple of 4");
    if (!masked_aligned(x, known, x, mask)) VDX_FAIL(VDX_ERR_INVALID, "inpaint_init: x / known must be 16-byte and mask 4-byte aligned");
    if (n) VDX_HIP(vdx::launch_inpaint_init(x, known, mask, mask_tables, timesteps, t0, n, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_p_sample_step_masked(const float* x, const float* eps_hat, float* out, const int* t, const float* tables, int timesteps,
                             const float* known, const unsigned char* mask, const float* mask_tables, int resample_steps,
                             uint64_t seed, uint64_t step, const uint64_t* step_dev, const float* thres, int clip_denoised,
                             int batch, int channels, long per_sample, void* stream) {
    if (!x || !eps_hat || !out || !t || !tables || !known || !mask || !mask_tables || timesteps < 1 || batch < 1 || channels < 1 || per_sample < 1)
        VDX_FAIL(VDX_ERR_INVALID, "p_sample_masked: bad argument");
    if (resample_steps < 1) VDX_FAIL(VDX_ERR_INVALID, "p_sample_masked: resample_steps must be >= 1");
    if (per_sample % channels || per_sample % 4) VDX_FAIL(VDX_ERR_INVALID, "p_sample_masked: per_sample must be a multiple of channels and of 4");
    if (!masked_aligned(x, known, out, mask)) VDX_FAIL(VDX_ERR_INVALID, "p_sample_masked: x / known / out must be 16-byte and mask 4-byte aligned");
    const vdx::PSampleArgs a = psample_args(x, eps_hat, out, t, tables, timesteps, nullptr, seed, 0, nullptr, thres, clip_denoised, channels, per_sample);
    const vdx::MaskArgs m = {known, mask, mask_tables, resample_steps, step, reinterpret_cast<const unsigned long long*>(step_dev)};
    VDX_HIP(vdx::launch_p_sample_masked(a, m, batch, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_ddim_step(const float* x, const float* eps_hat, float* out, const float* alphas_cumprod, const int* seq,
                  const uint64_t* step_dev, const float* thres, int clip_denoised, int batch, int channels, long per_sample, void* stream) {
    if (!x || !eps_hat || !out || !alphas_cumprod || !seq || batch < 1 || channels < 1 || per_sample < 1 || per_sample % channels)
        VDX_FAIL(VDX_ERR_INVALID, "ddim_step: bad argument");
    VDX_HIP(vdx::launch_ddim_step(x, eps_hat, out, alphas_cumprod, seq, reinterpret_cast<const unsigned long long*>(step_dev), thres,
                                  clip_denoised, batch, channels, per_sample, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_ddim_step_masked(const float* x, const float* eps_hat, float* out, const float* alphas_cumprod, const int* seq,
                         const uint64_t* step_dev, const float* thres, int clip_denoised, const float* known, const unsigned char* mask,
                         const float* mask_tables, int timesteps, uint64_t seed, int batch, int channels, long per_sample, void* stream) {
    if (!x || !eps_hat || !out || !alphas_cumprod || !seq || !known || !mask || !mask_tables || timesteps < 1 || batch < 1 || channels < 1 ||
        per_sample < 1 || per_sample % channels)
        VDX_FAIL(VDX_ERR_INVALID, "ddim_step_masked: bad argument");
    if (per_sample % 4) VDX_FAIL(VDX_ERR_INVALID, "ddim_step_masked: per_sample must be a multiple of 4");
    if (!masked_aligned(x, known, out, mask)) VDX_FAIL(VDX_ERR_INVALID, "ddim_step_masked: x / known / out must be 16-byte and mask 4-byte aligned");
    const vdx::MaskArgs m = {known, mask, mask_tables, 1, 0ull, nullptr};
    VDX_HIP(vdx::launch_ddim_step_masked(x, eps_hat, out, alphas_cumprod, seq, reinterpret_cast<const unsigned long long*>(step_dev), thres,
                                         clip_denoised, batch, channels, per_sample, m, timesteps, seed, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_dpm_step(const float* x, const float* eps_hat, float* out, float* hist, const float* alphas_cumprod, const int* seq,
                 const uint64_t* step_dev, const float* thres, int clip_denoised, int order, int batch, int channels, long per_sample,
                 void* stream) {
    if (!x || !eps_hat || !out || !alphas_cumprod || !seq || batch < 1 || channels < 1 || per_sample < 1 || per_sample % channels)
        VDX_FAIL(VDX_ERR_INVALID, "dpm_step: bad argument");
    if (order != 1 && order != 2) VDX_FAIL(VDX_ERR_INVALID, "dpm_step: order must be 1 or 2");
    if (order == 2 && !hist) VDX_FAIL(VDX_ERR_INVALID, "dpm_step: order 2 needs hist");
    if (per_sample % 4) VDX_FAIL(VDX_ERR_INVALID, "dpm_step: per_sample must be a multiple of 4");
    if ((uintptr_t)x % 16 || (uintptr_t)out % 16 || (uintptr_t)hist % 16) VDX_FAIL(VDX_ERR_INVALID, "dpm_step: x / out / hist must be 16-byte aligned");
    VDX_HIP(vdx::launch_dpm_step(x, eps_hat, out, hist, alphas_cumprod, seq, reinterpret_cast<const unsigned long long*>(step_dev), thres,
                                 clip_denoised, order, batch, channels, per_sample, nullptr, 0, 0ull, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_dpm_step_masked(const float* x, const float* eps_hat, float* out, float* hist, const float* alphas_cumprod, const int* seq,
                        const uint64_t* step_dev, const float* thres, int clip_denoised, int order, const float* known,
                        const unsigned char* mask, const float* mask_tables, int timesteps, uint64_t seed, int batch, int channels,
                        long per_sample, void* stream) {
    if (!x || !eps_hat || !out || !alphas_cumprod || !seq || !known || !mask || !mask_tables || timesteps < 1 || batch < 1 || channels < 1 ||
        per_sample < 1 || per_sample % channels)
        VDX_FAIL(VDX_ERR_INVALID, "dpm_step_masked: bad argument");
    if (order != 1 && order != 2) VDX_FAIL(VDX_ERR_INVALID, "dpm_step_masked: order must be 1 or 2");
    if (order == 2 && !hist) VDX_FAIL(VDX_ERR_INVALID, "dpm_step_masked: order 2 needs hist");
    if (per_sample % 4) VDX_FAIL(VDX_ERR_INVALID, "dpm_step_masked: per_sample must be a multiple of 4");
    if (!masked_aligned(x, known, out, mask) || (uintptr_t)hist % 16)
        VDX_FAIL(VDX_ERR_INVALID, "dpm_step_masked: x / known / out / hist must be 16-byte and mask 4-byte aligned");
    const vdx::MaskArgs m = {known, mask, mask_tables, 1, 0ull, nullptr};
    VDX_HIP(vdx::launch_dpm_step(x, eps_hat, out, hist, alphas_cumprod, seq, reinterpret_cast<const unsigned long long*>(step_dev), thres,
                                 clip_denoised, order, batch, channels, per_sample, &m, timesteps, seed, (hipStream_t)stream));
    return VDX_OK;
}

size_t vdx_cfg_scratch_doubles(int batch) { return batch > 0 ? vdx::cfg_scratch_doubles(batch) : 0; }

int vdx_cfg_combine(const float* eps2, float* out, float cond_scale, float rescale, double* scratch, int batch, long per_sample, void* stream) {
    if (!eps2 || !out || batch < 1 || per_sample < 1) VDX_FAIL(VDX_ERR_INVALID, "cfg_combine: bad argument");
    if (per_sample % 4) VDX_FAIL(VDX_ERR_INVALID, "cfg_combine: per_sample must be a multiple of 4");
    if ((uintptr_t)eps2 % 16 || (uintptr_t)out % 16) VDX_FAIL(VDX_ERR_INVALID, "cfg_combine: eps2 / out must be 16-byte aligned");
    if (!(rescale >= 0.f && rescale <= 1.f)) VDX_FAIL(VDX_ERR_INVALID, "cfg_combine: rescale must be in [0, 1]");
    if (rescale > 0.f && (!scratch || (uintptr_t)scratch % 8)) VDX_FAIL(VDX_ERR_INVALID, "cfg_combine: rescale needs an 8-byte aligned scratch");
    VDX_HIP(vdx::launch_cfg_combine(eps2, out, cond_scale, rescale, scratch, batch, per_sample, (hipStream_t)stream));
    return VDX_OK;
}

// ---- the sampling loops: one step builder, fifteen positional entry points ----

// 0 <= x <= 1 by the bits of x (non-negative floats order like unsigned integers): the library is built with -fno-honor-nans, under
// which a comparison may let a NaN through, and a NaN rescale has to be refused
static bool in_unit_interval(float x) {
    unsigned u;
    memcpy(&u, &x, sizeof(u));
    return u <= 0x3F800000u || u == 0x80000000u;       // [+0, 1] or -0
}

// The step of every loop, launch for launch: (guided: copy img[:B] -> img[B:]) -> (super-resolution, a.xin: lowres_pack img -> the
// first half of xin, the forward then reads xin) -> model_forward over B samples (guided: 2B, the second half with the null embedding) ->
// (v-prediction, vdx_set_prediction kind 1: v_to_eps over the forward's rows, in place on eps_buf, x = img) -> (guided: cfg_combine) -> (dynamic threshold) ->
// (self-conditioning, vdx_set_self_condition, an xin loop: selfcond_x0 of img and eps_buf at t_dev -> planes [C, 2C) of xin, what the next
// step's forward reads) -> the chain's step kernel on B samples -> the chain's advance (guided: over 2B).  Mixed noise (a.mix_a / a.mix_b, the ancestral chain only): p_sample_mixed_kernel is that step kernel.
// Validates, derives the graph key from `a` and runs nsteps steps eagerly or as replays of one captured step.
// Guided loops (classifier-free guidance; EXTENSION, parity unpinned: the reference's p_sample_loop drops cond): img / t_dev / eps_buf /
// workspace hold 2 * batch samples; the step kernels, the threshold and the result use the first `batch`.
static int sample_loop(const char* who, vdx_handle* h, const LoopArgs& a, int nsteps, int use_graph, void* stream) {
    char msg[160];
#define LOOP_FAIL(code, text) do { snprintf(msg, sizeof(msg), "%s: %s", who, text); VDX_FAIL(code, msg); } while (0)
    const bool anc = a.chain == CHAIN_ANCESTRAL, dpm = a.chain == CHAIN_DPM, masked = a.masked != 0, guided = a.guided != 0;
    const bool mixed = a.mix_a != 0.f || a.mix_b != 0.f;                  // (the entry has checked the pair: a^2 + b^2 = 1)
    if (!h || !a.params || !a.packed || !a.img || !a.eps_buf || !a.t_dev || !a.step_dev || !a.workspace) LOOP_FAIL(VDX_ERR_INVALID, "null argument");
    if (anc ? !a.tables : (!a.alphas_cumprod || !a.seq)) LOOP_FAIL(VDX_ERR_INVALID, "null argument");
    if (masked && (!a.known || !a.mask || !a.mask_tables)) LOOP_FAIL(VDX_ERR_INVALID, "null argument");
    if (guided && (!a.cond || !a.cfg_scratch)) LOOP_FAIL(VDX_ERR_INVALID, "null argument");
    // super-resolution (a.xin; vdx.h: "Cascaded super-resolution"): the network reads xin [batch, 2C, F, S, S], everything else is over
    // C = out_dim channels.  Plain variants only: there is no masked or guided entry that sets xin
    const bool sr = a.xin != nullptr;
    if (h->sc && !sr) LOOP_FAIL(VDX_ERR_STATE, "self-conditioning (vdx_set_self_condition) needs a loop over xin (vdx_*_sample_loop_sr)");
    if (sr && h->model.cfg.channels != 2 * h->model.out_dim) LOOP_FAIL(VDX_ERR_INVALID, "channels must equal 2 * out_dim");
    if (!h->model.d_ss_layers) LOOP_FAIL(VDX_ERR_STATE, "handle was created without a GPU");
    // the rules of the variants, keyed on chain / masked / guided (all VDX_ERR_INVALID)
    const vdx::Model& m = h->model;
    const long per_sample = (long)(sr ? m.out_dim : m.cfg.channels) * m.cfg.num_frames * m.cfg.image_size * m.cfg.image_size;
    const bool dyn = a.percentile > 0.f && a.clip_denoised;
    if (guided && !m.cfg.cond_dim) LOOP_FAIL(VDX_ERR_INVALID, "the network has no condition (cond_dim == 0)");
    if (guided && a.batch < 1) LOOP_FAIL(VDX_ERR_INVALID, "batch must be >= 1");
    if (guided && !in_unit_interval(a.rescale)) LOOP_FAIL(VDX_ERR_INVALID, "rescale must be in [0, 1]");
    if (dpm && a.order != 1 && a.order != 2) LOOP_FAIL(VDX_ERR_INVALID, "order must be 1 or 2");
    if (dpm && a.order == 2 && !a.hist) LOOP_FAIL(VDX_ERR_INVALID, "order 2 needs hist");
    if (anc && masked && a.resample_steps < 1) LOOP_FAIL(VDX_ERR_INVALID, "resample_steps must be >= 1");
    if ((masked || (anc && guided)) && a.timesteps < 1) LOOP_FAIL(VDX_ERR_INVALID, "timesteps (the row length of the tables) must be >= 1");
    const long chain_len = !anc ? a.seq_len : masked ? (long)a.timesteps * a.resample_steps : a.timesteps;
    if ((!anc && a.seq_len < 1) || nsteps < 0 || nsteps > chain_len) LOOP_FAIL(VDX_ERR_INVALID, "nsteps out of range");
    if (dyn && (!a.thres_buf || a.percentile > 1.f)) LOOP_FAIL(VDX_ERR_INVALID, "dynamic threshold needs thres_buf and a percentile in (0, 1]");
    if (dyn && !anc && (!a.tables || a.timesteps < 1)) LOOP_FAIL(VDX_ERR_INVALID, "dynamic threshold needs tables and timesteps >= 1");
    // (ddim_step_kernel alone has a scalar form; every other step kernel, and cfg_combine, move four elements per thread)
    if (per_sample % 4 && (a.chain != CHAIN_DDIM || masked || guided)) LOOP_FAIL(VDX_ERR_INVALID, "C*F*H*W must be a multiple of 4");
    if (!sr && m.out_dim != m.cfg.channels) LOOP_FAIL(VDX_ERR_INVALID, "out_dim must equal channels");
    if (sr && ((uintptr_t)a.img % 16 || (uintptr_t)a.xin % 16)) LOOP_FAIL(VDX_ERR_INVALID, "img / xin must be 16-byte aligned");
    if (masked && !masked_aligned(a.img, a.known, a.img, a.mask)) LOOP_FAIL(VDX_ERR_INVALID, "img / known must be 16-byte and mask 4-byte aligned");
    if (mixed && (uintptr_t)a.img % 16) LOOP_FAIL(VDX_ERR_INVALID, "img must be 16-byte aligned");
    if (dpm && ((uintptr_t)a.img % 16 || (uintptr_t)a.hist % 16)) LOOP_FAIL(VDX_ERR_INVALID, "img / hist must be 16-byte aligned");
    if (guided && ((uintptr_t)a.img % 16 || (uintptr_t)a.eps_buf % 16 || (uintptr_t)a.hist % 16 || (uintptr_t)a.cfg_scratch % 8))
        LOOP_FAIL(VDX_ERR_INVALID, "img / eps_buf / hist must be 16-byte and the cfg scratch 8-byte aligned");
#undef LOOP_FAIL
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* sd = reinterpret_cast<unsigned long long*>(a.step_dev);
    const int B = a.batch, rows = guided ? 2 * B : B, C = sr ? m.out_dim : m.cfg.channels;      // rows: what the forward and the advance cover
    const float* th = dyn ? a.thres_buf : nullptr;
    const unsigned char* cond_mask = guided ? vdx::cfg_scratch_mask(a.cfg_scratch, B) : nullptr;
    // (ancestral: one Philox draw per step through step_dev, resampling or not; the sequence chains draw for the known region only)
    const vdx::MaskArgs ma = {a.known, a.mask, a.mask_tables, anc ? a.resample_steps : 1, 0ull, anc ? sd : nullptr};
    const vdx::MixArgs mx = {m.cfg.num_frames, (long)m.cfg.image_size * m.cfg.image_size, a.mix_a, a.mix_b};
    if (guided) VDX_HIP(vdx::launch_cfg_mask(a.cfg_scratch, B, st));
    auto step = [&]() -> int {
        hipError_t e = hipSuccess;
        // guided: both halves of the batched forward see the same x_t; the null rows never read cond (time_mlp), so cond stays [batch, cond_dim]
        if (guided) e = hipMemcpyAsync(a.img + (size_t)B * per_sample, a.img, (size_t)B * per_sample * sizeof(float), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return vdx_set_error(VDX_ERR_HIP, hipGetErrorString(e), __FILE__, __LINE__);
        // reference p_sample_loop never forwards cond (Q10); when a cond tensor is supplied to an unguided loop it is used un-masked
        if (sr) e = vdx::launch_lowres_pack(a.img, a.xin, B, per_sample, st);
        if (e != hipSuccess) return vdx_set_error(VDX_ERR_HIP, hipGetErrorString(e), __FILE__, __LINE__);
        int rc = vdx::model_forward(&m, a.params, a.packed, sr ? a.xin : a.img, a.t_dev, a.cond, cond_mask, 0, a.eps_buf, a.workspace, a.workspace_bytes, rows, st);
        if (rc != VDX_OK) return rc;
        // v-prediction: the output becomes eps_hat before anything reads it (both halves of a guided batch: guidance acts on eps_hat)
        if (h->pred) e = vdx::launch_v_to_eps(a.eps_buf, a.img, a.t_dev, h->pred_sa, h->pred_s1, h->pred_T, rows, C, per_sample, st);
        if (e == hipSuccess && guided) e = vdx::launch_cfg_combine(a.eps_buf, a.eps_buf, a.cond_scale, a.rescale, a.cfg_scratch, B, per_sample, st);
        if (e == hipSuccess && dyn) e = vdx::launch_dyn_thres(a.img, a.eps_buf, a.t_dev, a.tables, a.timesteps, a.percentile, a.thres_buf, B, C, per_sample, st);
        // self-conditioning: x0~ of this step (the level is t_dev's for all three chains) is the second half of the next step's input
        if (e == hipSuccess && h->sc) {
            const vdx::SelfcondArgs sa = {a.img, per_sample, a.eps_buf, a.t_dev, h->sc_tab, h->sc_T, th, a.clip_denoised, a.xin, C, per_sample};
            e = vdx::launch_selfcond_x0(sa, B, st);
        }
        if (anc) {
            const vdx::PSampleArgs pa = psample_args(a.img, a.eps_buf, a.img, a.t_dev, a.tables, a.timesteps, nullptr, a.seed, masked ? 0 : 1,
                                                     masked ? nullptr : a.step_dev, th, a.clip_denoised, C, per_sample);
            if (e == hipSuccess)
                e = masked ? vdx::launch_p_sample_masked(pa, ma, B, st) : mixed ? vdx::launch_p_sample_mixed(pa, mx, B, st) : vdx::launch_p_sample(pa, B, st);
            if (e == hipSuccess) e = masked ? vdx::launch_resample_advance(a.t_dev, B, sd, a.resample_steps, st) : vdx::launch_advance(a.t_dev, rows, sd, st);
        } else {
            if (e == hipSuccess && dpm)
                e = vdx::launch_dpm_step(a.img, a.eps_buf, a.img, a.hist, a.alphas_cumprod, a.seq, sd, th, a.clip_denoised, a.order, B, C, per_sample,
                                         masked ? &ma : nullptr, a.timesteps, a.seed, st);
            else if (e == hipSuccess && masked)
                e = vdx::launch_ddim_step_masked(a.img, a.eps_buf, a.img, a.alphas_cumprod, a.seq, sd, th, a.clip_denoised, B, C, per_sample, ma, a.timesteps, a.seed, st);
            else if (e == hipSuccess)
                e = vdx::launch_ddim_step(a.img, a.eps_buf, a.img, a.alphas_cumprod, a.seq, sd, th, a.clip_denoised, B, C, per_sample, st);
            if (e == hipSuccess) e = vdx::launch_ddim_advance(a.t_dev, rows, a.seq, sd, st);
        }
        if (e != hipSuccess) return vdx_set_error(VDX_ERR_HIP, hipGetErrorString(e), __FILE__, __LINE__);
        return VDX_OK;
    };
    // the key: `a` itself (zero-filled, then assigned field by field: loop_args) with what this step does not read set to zero
    vdx_handle::GraphKey key;
    memset(&key, 0, sizeof(key));
    memcpy(&key.a, &a, sizeof(a));
    key.stream = stream; key.act16 = m.act16; h->key_prediction(key);
    LoopArgs& k = key.a;
    if (!dyn) { k.percentile = 0.f; k.thres_buf = nullptr; }
    if (anc) { k.alphas_cumprod = nullptr; k.seq = nullptr; k.seq_len = 0; }
    if (!anc && !dyn) { k.tables = nullptr; if (!masked) k.timesteps = 0; }
    if (!anc && !masked) k.seed = 0;
    if (!dpm) { k.hist = nullptr; k.order = 0; }
    if (!masked) { k.known = nullptr; k.mask = nullptr; k.mask_tables = nullptr; }
    if (!masked || !anc) k.resample_steps = 0;
    if (!guided) { k.cond_scale = 0.f; k.rescale = 0.f; k.cfg_scratch = nullptr; }
    const int slot = mixed ? 15 + (guided ? 1 : 0) : sr ? 12 + a.chain : 3 * (guided ? 2 : masked ? 1 : 0) + a.chain;
    return run_steps(h, slot, key, nsteps, use_graph, st, step);
}

// what all fifteen entries share; the rest of `a` is zero (and so is its padding: the bytes of a LoopArgs are a graph key)
static void loop_args(LoopArgs& a, int chain, const float* params, const void* packed, float* img, float* eps_buf, int* t_dev, uint64_t* step_dev,
                      const float* cond, int clip_denoised, float percentile, float* thres_buf, void* workspace, size_t workspace_bytes, int batch) {
    memset(&a, 0, sizeof(a));
    a.chain = chain; a.params = params; a.packed = packed; a.img = img; a.eps_buf = eps_buf; a.t_dev = t_dev; a.step_dev = step_dev;
    a.cond = cond; a.clip_denoised = clip_denoised; a.percentile = percentile; a.thres_buf = thres_buf;
    a.workspace = workspace; a.workspace_bytes = workspace_bytes; a.batch = batch;
}
static void set_sequence(LoopArgs& a, const float* alphas_cumprod, const int* seq, int seq_len, const float* tables, int timesteps) {
    a.alphas_cumprod = alphas_cumprod; a.seq = seq; a.seq_len = seq_len; a.tables = tables; a.timesteps = timesteps;
}
static void set_masked(LoopArgs& a, const float* known, const unsigned char* mask, const float* mask_tables, uint64_t seed) {
    a.masked = 1; a.known = known; a.mask = mask; a.mask_tables = mask_tables; a.seed = seed;
}
static void set_guided(LoopArgs& a, float cond_scale, float rescale, double* cfg_scratch) {
    a.guided = 1; a.cond_scale = cond_scale; a.rescale = rescale; a.cfg_scratch = cfg_scratch;
}

int vdx_p_sample_loop_dyn(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, int* t_dev,
                          uint64_t* step_dev, const float* tables, int timesteps, int nsteps, const float* cond, uint64_t seed,
                          int clip_denoised, float percentile, float* thres_buf, void* workspace, size_t workspace_bytes, int batch,
                          int use_graph, void* stream) {
    LoopArgs a;
    loop_args(a, CHAIN_ANCESTRAL, params, packed, img, eps_buf, t_dev, step_dev, cond, clip_denoised, percentile, thres_buf, workspace, workspace_bytes, batch);
    a.tables = tables; a.timesteps = timesteps; a.seed = seed;
    return sample_loop("p_sample_loop", h, a, nsteps, use_graph, stream);
}

int vdx_p_sample_loop(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, int* t_dev,
                      uint64_t* step_dev, const float* tables, int timesteps, int nsteps, const float* cond, uint64_t seed,
                      int clip_denoised, void* workspace, size_t workspace_bytes, int batch, int use_graph, void* stream) {
    return vdx_p_sample_loop_dyn(h, params, packed, img, eps_buf, t_dev, step_dev, tables, timesteps, nsteps, cond, seed, clip_denoised,
                                 0.f, nullptr, workspace, workspace_bytes, batch, use_graph, stream);
}

int vdx_p_sample_loop_masked(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, int* t_dev,
                             uint64_t* step_dev, const float* tables, int timesteps, int nsteps, const float* cond, uint64_t seed,
                             int clip_denoised, float percentile, float* thres_buf, const float* known, const unsigned char* mask,
                             const float* mask_tables, int resample_steps, void* workspace, size_t workspace_bytes, int batch,
                             int use_graph, void* stream) {
    LoopArgs a;
    loop_args(a, CHAIN_ANCESTRAL, params, packed, img, eps_buf, t_dev, step_dev, cond, clip_denoised, percentile, thres_buf, workspace, workspace_bytes, batch);
    a.tables = tables; a.timesteps = timesteps; a.resample_steps = resample_steps;
    set_masked(a, known, mask, mask_tables, seed);
    return sample_loop("p_sample_loop_masked", h, a, nsteps, use_graph, stream);
}

int vdx_p_sample_loop_guided(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, int* t_dev,
                             uint64_t* step_dev, const float* tables, int timesteps, int nsteps, const float* cond, uint64_t seed,
                             int clip_denoised, float percentile, float* thres_buf, float cond_scale, float rescale, double* cfg_scratch,
                             void* workspace, size_t workspace_bytes, int batch, int use_graph, void* stream) {
    LoopArgs a;
    loop_args(a, CHAIN_ANCESTRAL, params, packed, img, eps_buf, t_dev, step_dev, cond, clip_denoised, percentile, thres_buf, workspace, workspace_bytes, batch);
    a.tables = tables; a.timesteps = timesteps; a.seed = seed;
    set_guided(a, cond_scale, rescale, cfg_scratch);
    return sample_loop("p_sample_loop_guided", h, a, nsteps, use_graph, stream);
}

int vdx_p_sample_loop_mixed(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, int* t_dev,
                            uint64_t* step_dev, const float* tables, int timesteps, int nsteps, const float* cond, uint64_t seed,
                            int clip_denoised, float percentile, float* thres_buf, float cond_scale, float rescale, double* cfg_scratch,
                            float a, float b, void* workspace, size_t workspace_bytes, int batch, int use_graph, void* stream) {
    if (!mix_weights_ok(a, b)) VDX_FAIL(VDX_ERR_INVALID, "p_sample_loop_mixed: " VDX_MIX_WEIGHTS_RULE);
    LoopArgs la;
    loop_args(la, CHAIN_ANCESTRAL, params, packed, img, eps_buf, t_dev, step_dev, cond, clip_denoised, percentile, thres_buf, workspace, workspace_bytes, batch);
    la.tables = tables; la.timesteps = timesteps; la.seed = seed;
    la.mix_a = a; la.mix_b = b;
    if (cond_scale != 1.f && cfg_scratch) set_guided(la, cond_scale, rescale, cfg_scratch);
    return sample_loop("p_sample_loop_mixed", h, la, nsteps, use_graph, stream);
}

int vdx_ddim_sample_loop_dyn(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, int* t_dev,
                             uint64_t* step_dev, const float* alphas_cumprod, const int* seq, int seq_len, int nsteps, const float* cond,
                             int clip_denoised, const float* tables, int timesteps, float percentile, float* thres_buf, void* workspace,
                             size_t workspace_bytes, int batch, int use_graph, void* stream) {
    LoopArgs a;
    loop_args(a, CHAIN_DDIM, params, packed, img, eps_buf, t_dev, step_dev, cond, clip_denoised, percentile, thres_buf, workspace, workspace_bytes, batch);
    set_sequence(a, alphas_cumprod, seq, seq_len, tables, timesteps);
    return sample_loop("ddim_sample_loop", h, a, nsteps, use_graph, stream);
}

int vdx_ddim_sample_loop(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, int* t_dev,
                         uint64_t* step_dev, const float* alphas_cumprod, const int* seq, int seq_len, int nsteps, const float* cond,
                         int clip_denoised, void* workspace, size_t workspace_bytes, int batch, int use_graph, void* stream) {
    return vdx_ddim_sample_loop_dyn(h, params, packed, img, eps_buf, t_dev, step_dev, alphas_cumprod, seq, seq_len, nsteps, cond, clip_denoised,
                                    nullptr, 0, 0.f, nullptr, workspace, workspace_bytes, batch, use_graph, stream);
}

int vdx_ddim_sample_loop_masked(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, int* t_dev,
                                uint64_t* step_dev, const float* alphas_cumprod, const int* seq, int seq_len, int nsteps, const float* cond,
                                int clip_denoised, const float* tables, int timesteps, float percentile, float* thres_buf,
                                const float* known, const unsigned char* mask, const float* mask_tables, uint64_t seed,
                                void* workspace, size_t workspace_bytes, int batch, int use_graph, void* stream) {
    LoopArgs a;
    loop_args(a, CHAIN_DDIM, params, packed, img, eps_buf, t_dev, step_dev, cond, clip_denoised, percentile, thres_buf, workspace, workspace_bytes, batch);
    set_sequence(a, alphas_cumprod, seq, seq_len, tables, timesteps);
    set_masked(a, known, mask, mask_tables, seed);
    return sample_loop("ddim_sample_loop_masked", h, a, nsteps, use_graph, stream);
}

int vdx_ddim_sample_loop_guided(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, int* t_dev,
                                uint64_t* step_dev, const float* alphas_cumprod, const int* seq, int seq_len, int nsteps, const float* cond,
                                int clip_denoised, const float* tables, int timesteps, float percentile, float* thres_buf, float cond_scale,
                                float rescale, double* cfg_scratch, void* workspace, size_t workspace_bytes, int batch, int use_graph,
                                void* stream) {
    LoopArgs a;
    loop_args(a, CHAIN_DDIM, params, packed, img, eps_buf, t_dev, step_dev, cond, clip_denoised, percentile, thres_buf, workspace, workspace_bytes, batch);
    set_sequence(a, alphas_cumprod, seq, seq_len, tables, timesteps);
    set_guided(a, cond_scale, rescale, cfg_scratch);
    return sample_loop("ddim_sample_loop_guided", h, a, nsteps, use_graph, stream);
}

int vdx_dpm_sample_loop(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, float* hist, int* t_dev,
                        uint64_t* step_dev, const float* alphas_cumprod, const int* seq, int seq_len, int nsteps, const float* cond,
                        int clip_denoised, int order, const float* tables, int timesteps, float percentile, float* thres_buf,
                        void* workspace, size_t workspace_bytes, int batch, int use_graph, void* stream) {
    LoopArgs a;
    loop_args(a, CHAIN_DPM, params, packed, img, eps_buf, t_dev, step_dev, cond, clip_denoised, percentile, thres_buf, workspace, workspace_bytes, batch);
    set_sequence(a, alphas_cumprod, seq, seq_len, tables, timesteps);
    a.hist = hist; a.order = order;
    return sample_loop("dpm_sample_loop", h, a, nsteps, use_graph, stream);
}

int vdx_dpm_sample_loop_masked(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, float* hist, int* t_dev,
                               uint64_t* step_dev, const float* alphas_cumprod, const int* seq, int seq_len, int nsteps, const float* cond,
                               int clip_denoised, int order, const float* tables, int timesteps, float percentile, float* thres_buf,
                               const float* known, const unsigned char* mask, const float* mask_tables, uint64_t seed,
                               void* workspace, size_t workspace_bytes, int batch, int use_graph, void* stream) {
    LoopArgs a;
    loop_args(a, CHAIN_DPM, params, packed, img, eps_buf, t_dev, step_dev, cond, clip_denoised, percentile, thres_buf, workspace, workspace_bytes, batch);
    set_sequence(a, alphas_cumprod, seq, seq_len, tables, timesteps);
    set_masked(a, known, mask, mask_tables, seed);
    a.hist = hist; a.order = order;
    return sample_loop("dpm_sample_loop_masked", h, a, nsteps, use_graph, stream);
}

int vdx_dpm_sample_loop_guided(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, float* hist, int* t_dev,
                               uint64_t* step_dev, const float* alphas_cumprod, const int* seq, int seq_len, int nsteps, const float* cond,
                               int clip_denoised, int order, const float* tables, int timesteps, float percentile, float* thres_buf,
                               float cond_scale, float rescale, double* cfg_scratch, void* workspace, size_t workspace_bytes, int batch,
                               int use_graph, void* stream) {
    LoopArgs a;
    loop_args(a, CHAIN_DPM, params, packed, img, eps_buf, t_dev, step_dev, cond, clip_denoised, percentile, thres_buf, workspace, workspace_bytes, batch);
    set_sequence(a, alphas_cumprod, seq, seq_len, tables, timesteps);
    set_guided(a, cond_scale, rescale, cfg_scratch);
    a.hist = hist; a.order = order;
    return sample_loop("dpm_sample_loop_guided", h, a, nsteps, use_graph, stream);
}

// ---- cascaded super-resolution (vdx.h: "Cascaded super-resolution"): the three loops over xin = [ x_t | u ] and the kernels around them ----

int vdx_p_sample_loop_sr(vdx_handle* h, const float* params, const void* packed, float* img, float* xin, float* eps_buf, int* t_dev,
                         uint64_t* step_dev, const float* tables, int timesteps, int nsteps, const float* cond, uint64_t seed,
                         int clip_denoised, float percentile, float* thres_buf, void* workspace, size_t workspace_bytes, int batch,
                         int use_graph, void* stream) {
    const char* who = "p_sample_loop_sr";
    if (!xin) VDX_REFUSE(who, "null argument");
    LoopArgs a;
    loop_args(a, CHAIN_ANCESTRAL, params, packed, img, eps_buf, t_dev, step_dev, cond, clip_denoised, percentile, thres_buf, workspace, workspace_bytes, batch);
    a.tables = tables; a.timesteps = timesteps; a.seed = seed; a.xin = xin;
    return sample_loop(who, h, a, nsteps, use_graph, stream);
}

int vdx_ddim_sample_loop_sr(vdx_handle* h, const float* params, const void* packed, float* img, float* xin, float* eps_buf, int* t_dev,
                            uint64_t* step_dev, const float* alphas_cumprod, const int* seq, int seq_len, int nsteps, const float* cond,
                            int clip_denoised, const float* tables, int timesteps, float percentile, float* thres_buf, void* workspace,
                            size_t workspace_bytes, int batch, int use_graph, void* stream) {
    const char* who = "ddim_sample_loop_sr";
    if (!xin) VDX_REFUSE(who, "null argument");
    LoopArgs a;
    loop_args(a, CHAIN_DDIM, params, packed, img, eps_buf, t_dev, step_dev, cond, clip_denoised, percentile, thres_buf, workspace, workspace_bytes, batch);
    set_sequence(a, alphas_cumprod, seq, seq_len, tables, timesteps);
    a.xin = xin;
    return sample_loop(who, h, a, nsteps, use_graph, stream);
}

int vdx_dpm_sample_loop_sr(vdx_handle* h, const float* params, const void* packed, float* img, float* xin, float* eps_buf, float* hist,
                           int* t_dev, uint64_t* step_dev, const float* alphas_cumprod, const int* seq, int seq_len, int nsteps,
                           const float* cond, int clip_denoised, int order, const float* tables, int timesteps, float percentile,
                           float* thres_buf, void* workspace, size_t workspace_bytes, int batch, int use_graph, void* stream) {
    const char* who = "dpm_sample_loop_sr";
    if (!xin) VDX_REFUSE(who, "null argument");
    LoopArgs a;
    loop_args(a, CHAIN_DPM, params, packed, img, eps_buf, t_dev, step_dev, cond, clip_denoised, percentile, thres_buf, workspace, workspace_bytes, batch);
    set_sequence(a, alphas_cumprod, seq, seq_len, tables, timesteps);
    a.hist = hist; a.order = order; a.xin = xin;
    return sample_loop(who, h, a, nsteps, use_graph, stream);
}

// the geometry rules the lowres kernels share (who-prefixed, VDX_ERR_INVALID)
static int lowres_rules(const char* who, int batch, int channels, int frames, int size, int ft, int fs) {
    if (batch < 1 || channels < 1 || frames < 1 || size < 1) VDX_REFUSE(who, "batch, channels, frames and size must be >= 1");
    if (ft < 1 || fs < 1) VDX_REFUSE(who, "the factors ft and fs must be >= 1");
    if (frames % ft || size % fs) VDX_REFUSE(who, "ft must divide frames and fs must divide size");
    return VDX_OK;
}

int vdx_lowres_down(const float* x, float* lo, int batch, int channels, int frames, int size, int ft, int fs, void* stream) {
    const char* who = "lowres_down";
    if (!x || !lo) VDX_REFUSE(who, "null tensor");
    if (int rc = lowres_rules(who, batch, channels, frames, size, ft, fs)) return rc;
    VDX_HIP(vdx::launch_lowres_down(x, lo, batch, channels, frames, size, ft, fs, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_lowres_input(const float* x0, const int* t, const float* noise, const float* lo, const int* aug_level, float* xin, const float* sqrt_ac,
                     const float* sqrt_one_minus_ac, int timesteps, uint64_t seed, uint64_t draw, float pre_scale, float pre_shift, int batch,
                     int channels, int frames, int size, int ft, int fs, void* stream) {
    const char* who = "lowres_input";
    if (!lo || !xin) VDX_REFUSE(who, "null tensor");
    if (x0 && (!t || !noise)) VDX_REFUSE(who, "x0 needs t and noise");
    if ((x0 || aug_level) && (!sqrt_ac || !sqrt_one_minus_ac || timesteps < 1)) VDX_REFUSE(who, "x0 / aug_level need the tables and timesteps >= 1");
    if (int rc = lowres_rules(who, batch, channels, frames, size, ft, fs)) return rc;
    if ((uintptr_t)x0 % 4 || (uintptr_t)noise % 4 || (uintptr_t)lo % 4 || (uintptr_t)xin % 4) VDX_REFUSE(who, "x0 / noise / lo / xin must be 4-byte aligned");
    vdx::LowresArgs a;
    memset(&a, 0, sizeof(a));
    a.x0 = x0; a.t = t; a.noise = noise; a.lo = lo; a.aug = aug_level; a.xin = xin; a.sqrt_ac = sqrt_ac; a.sqrt_1mac = sqrt_one_minus_ac;
    a.T = timesteps; a.seed = seed; a.draw = draw; a.pre_scale = pre_scale; a.pre_shift = pre_shift;
    a.C = channels; a.F = frames; a.S = size; a.ft = ft; a.fs = fs;
    VDX_HIP(vdx::launch_lowres_input(a, batch, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_lowres_pack(const float* img, float* xin, int batch, long per_sample, void* stream) {
    const char* who = "lowres_pack";
    if (!img || !xin) VDX_REFUSE(who, "null tensor");
    if (batch < 1 || per_sample < 1) VDX_REFUSE(who, "batch and per_sample must be >= 1");
    if ((uintptr_t)img % 4 || (uintptr_t)xin % 4) VDX_REFUSE(who, "img / xin must be 4-byte aligned");
    VDX_HIP(vdx::launch_lowres_pack(img, xin, batch, per_sample, (hipStream_t)stream));
    return VDX_OK;
}

// ---- held-out evaluation (vdx.h: "Held-out evaluation"): the three single-step entries and the loop ----

size_t vdx_vlb_scratch_doubles(int batch) { return batch > 0 ? (size_t)batch * vdx::vlb_blocks() * 3 : 0; }

// what the entries share: the rules of the vlb kernels (who-prefixed, all VDX_ERR_INVALID)
static int vlb_rules(const char* who, const void* x, const void* xt, const void* noise, const char* names16, const void* tables, const void* partial,
                     const void* out, int timesteps, int batch, int channels, long per_sample) {
    if (batch < 1 || channels < 1 || per_sample < 1) VDX_REFUSE(who, "batch, channels and per_sample must be >= 1");
    if (timesteps < 2) VDX_REFUSE(who, "timesteps must be >= 2");
    if (per_sample % 4 || per_sample % channels) VDX_REFUSE(who, "per_sample must be a multiple of 4 and of channels");
    if ((uintptr_t)x % 16 || (uintptr_t)xt % 16 || (uintptr_t)noise % 16) { char r_[96]; snprintf(r_, sizeof(r_), "%s must be 16-byte aligned", names16); VDX_REFUSE(who, r_); }
    if ((uintptr_t)tables % 8 || (uintptr_t)partial % 8 || (uintptr_t)out % 8) VDX_REFUSE(who, "vlb_tables / partial / out must be 8-byte aligned");
    return VDX_OK;
}

static vdx::VlbArgs vlb_args(const float* x, const float* eps_hat, float* xt, const float* noise, const int* t, const double* tables, int timesteps,
                             uint64_t seed, uint64_t draw, const uint64_t* step_dev, int clip, int channels, long per_sample, double* partial) {
    vdx::VlbArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.eps = eps_hat; a.xt = xt; a.noise = noise; a.t = t; a.tab = tables; a.T = timesteps;
    a.seed = seed; a.draw = draw; a.step_dev = reinterpret_cast<const unsigned long long*>(step_dev);
    a.clip = clip ? 1 : 0; a.C = channels; a.per_sample = per_sample; a.partial = partial;
    return a;
}

int vdx_vlb_noise(const float* x, float* xt, const int* t, const double* vlb_tables, int timesteps, const float* noise, uint64_t seed,
                  uint64_t draw, const uint64_t* step_dev, int batch, long per_sample, void* stream) {
    const char* who = "vlb_noise";
    if (!x || !xt || !t || !vlb_tables) VDX_REFUSE(who, "null tensor");
    if (int rc = vlb_rules(who, x, xt, noise, "x / xt / noise", vlb_tables, nullptr, nullptr, timesteps, batch, 1, per_sample)) return rc;
    const vdx::VlbArgs a = vlb_args(x, nullptr, xt, noise, t, vlb_tables, timesteps, seed, draw, step_dev, 0, 1, per_sample, nullptr);
    VDX_HIP(vdx::launch_vlb_noise(a, batch, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_vlb_terms(const float* x, const float* eps_hat, const int* t, const double* vlb_tables, int timesteps, const float* noise,
                  uint64_t seed, uint64_t draw, const uint64_t* step_dev, int clip_denoised, double* partial, double* out, int batch,
                  int channels, long per_sample, void* stream) {
    const char* who = "vlb_terms";
    if (!x || !eps_hat || !t || !vlb_tables || !partial || !out) VDX_REFUSE(who, "null tensor");
    if (int rc = vlb_rules(who, x, nullptr, noise, "x / noise", vlb_tables, partial, out, timesteps, batch, channels, per_sample)) return rc;
    const vdx::VlbArgs a = vlb_args(x, eps_hat, nullptr, noise, t, vlb_tables, timesteps, seed, draw, step_dev, clip_denoised, channels, per_sample, partial);
    VDX_HIP(vdx::launch_vlb_terms(a, batch, (hipStream_t)stream));
    VDX_HIP(vdx::launch_vlb_advance(partial, out, 3, batch, per_sample, nullptr, nullptr, 0, nullptr, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_vlb_prior(const float* x, const double* vlb_tables, int timesteps, double* partial, double* out, int batch, long per_sample,
                  void* stream) {
    const char* who = "vlb_prior";
    if (!x || !vlb_tables || !partial || !out) VDX_REFUSE(who, "null tensor");
    if (int rc = vlb_rules(who, x, nullptr, nullptr, "x", vlb_tables, partial, out, timesteps, batch, 1, per_sample)) return rc;
    VDX_HIP(vdx::launch_vlb_prior(x, vlb_tables, timesteps, partial, batch, per_sample, (hipStream_t)stream));
    VDX_HIP(vdx::launch_vlb_advance(partial, out, 1, batch, per_sample, nullptr, nullptr, 0, nullptr, (hipStream_t)stream));
    return VDX_OK;
}

// the two evaluation loops: lv = the learned-variance one (out_dim = 2 * channels, vlb_term_lv_kernel, graph slot 11)
static int vlb_loop(const char* who, bool lv, vdx_handle* h, const float* params, const void* packed, const float* x, float* xt_buf, float* eps_buf, int* t_dev,
                    uint64_t* step_dev, const double* vlb_tables, int timesteps, const int* seq, int seq_len, int nsteps, const float* cond,
                    uint64_t seed, int clip_denoised, double* partial, double* out, void* workspace, size_t workspace_bytes, int batch,
                    int use_graph, void* stream) {
    if (!h || !params || !packed || !x || !xt_buf || !eps_buf || !t_dev || !step_dev || !vlb_tables || !seq || !partial || !out || !workspace)
        VDX_REFUSE(who, "null argument");
    if (lv && h->pred) { char msg_[128]; snprintf(msg_, sizeof(msg_), "%s: v-prediction (vdx_set_prediction) has no learned-variance form", who); VDX_FAIL(VDX_ERR_STATE, msg_); }
    if (h->sc) { char msg_[128]; snprintf(msg_, sizeof(msg_), "%s: self-conditioning (vdx_set_self_condition) has no bits/dim form", who); VDX_FAIL(VDX_ERR_STATE, msg_); }
    if (!h->model.d_ss_layers) { char msg_[96]; snprintf(msg_, sizeof(msg_), "%s: handle was created without a GPU", who); VDX_FAIL(VDX_ERR_STATE, msg_); }
    const vdx::Model& m = h->model;
    const int C = m.cfg.channels;
    const long per_sample = (long)C * m.cfg.num_frames * m.cfg.image_size * m.cfg.image_size;
    if (int rc = vlb_rules(who, x, xt_buf, eps_buf, "x / xt_buf / eps_buf", vlb_tables, partial, out, timesteps, batch, C, per_sample)) return rc;
    if (!lv && m.out_dim != C) VDX_REFUSE(who, "out_dim must equal channels");
    if (lv && m.out_dim != 2 * C) VDX_REFUSE(who, "out_dim must equal 2 * channels");
    if (seq_len < 1) VDX_REFUSE(who, "seq_len must be >= 1");
    if (nsteps < 0 || nsteps > seq_len) VDX_REFUSE(who, "nsteps out of range");
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* sd = reinterpret_cast<unsigned long long*>(step_dev);
    const vdx::VlbArgs na = vlb_args(x, nullptr, xt_buf, nullptr, t_dev, vlb_tables, timesteps, seed, 1, step_dev, 0, C, per_sample, nullptr);
    const vdx::VlbArgs ta = vlb_args(x, eps_buf, nullptr, nullptr, t_dev, vlb_tables, timesteps, seed, 1, step_dev, clip_denoised, C, per_sample, partial);
    auto step = [&]() -> int {
        hipError_t e = vdx::launch_vlb_noise(na, batch, st);
        if (e != hipSuccess) return vdx_set_error(VDX_ERR_HIP, hipGetErrorString(e), __FILE__, __LINE__);
        // cond is used un-masked, as in the unguided sampling loops
        int rc = vdx::model_forward(&m, params, packed, xt_buf, t_dev, cond, nullptr, 0, eps_buf, workspace, workspace_bytes, batch, st);
        if (rc != VDX_OK) return rc;
        if (h->pred) e = vdx::launch_v_to_eps(eps_buf, xt_buf, t_dev, h->pred_sa, h->pred_s1, h->pred_T, batch, C, per_sample, st);      // (never with lv)
        if (e == hipSuccess) e = lv ? vdx::launch_vlb_terms_lv(ta, batch, st) : vdx::launch_vlb_terms(ta, batch, st);
        if (e == hipSuccess) e = vdx::launch_vlb_advance(partial, out, 3, batch, per_sample, t_dev, seq, seq_len, sd, st);
        if (e != hipSuccess) return vdx_set_error(VDX_ERR_HIP, hipGetErrorString(e), __FILE__, __LINE__);
        return VDX_OK;
    };
    // the key, built like the sampling loops': a zero-filled LoopArgs with every field this step reads
    vdx_handle::GraphKey key;
    memset(&key, 0, sizeof(key));
    LoopArgs& k = key.a;
    k.chain = lv ? CHAIN_VLB_LV : CHAIN_VLB; k.params = params; k.packed = packed; k.img = xt_buf; k.eps_buf = eps_buf; k.t_dev = t_dev; k.step_dev = step_dev;
    k.timesteps = timesteps; k.seq = seq; k.seq_len = seq_len; k.cond = cond; k.seed = seed; k.clip_denoised = clip_denoised ? 1 : 0;
    k.vlb_x = x; k.vlb_tables = vlb_tables; k.vlb_partial = partial; k.vlb_out = out;
    k.workspace = workspace; k.workspace_bytes = workspace_bytes; k.batch = batch;
    key.stream = stream; key.act16 = m.act16; h->key_prediction(key);
    return run_steps(h, lv ? 11 : 9, key, nsteps, use_graph, st, step);
}

int vdx_vlb_loop(vdx_handle* h, const float* params, const void* packed, const float* x, float* xt_buf, float* eps_buf, int* t_dev,
                 uint64_t* step_dev, const double* vlb_tables, int timesteps, const int* seq, int seq_len, int nsteps, const float* cond,
                 uint64_t seed, int clip_denoised, double* partial, double* out, void* workspace, size_t workspace_bytes, int batch,
                 int use_graph, void* stream) {
    return vlb_loop("vlb_loop", false, h, params, packed, x, xt_buf, eps_buf, t_dev, step_dev, vlb_tables, timesteps, seq, seq_len, nsteps, cond, seed,
                    clip_denoised, partial, out, workspace, workspace_bytes, batch, use_graph, stream);
}

// ---- learned variances (vdx.h: "Learned variances"): the step, the sampling loop, the hybrid loss, the bound ----

static vdx::LvStepArgs lv_step_args(const float* x, const float* out2, float* out, const int* level_dev, const float* lv_tables, int S, uint64_t step,
                                    const uint64_t* step_dev, const float* noise, uint64_t seed, uint64_t offset, const uint64_t* dev_offset, int clip,
                                    float post_scale, float post_shift, int channels, long per_sample) {
    vdx::LvStepArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.out2 = out2; a.out = out; a.tables = lv_tables; a.S = S; a.idx = level_dev; a.step = step;
    a.step_dev = reinterpret_cast<const unsigned long long*>(step_dev); a.noise = noise; a.seed = seed; a.offset = offset;
    a.dev_offset = reinterpret_cast<const unsigned long long*>(dev_offset); a.clip = clip ? 1 : 0; a.C = channels; a.per_sample = per_sample;
    a.post_scale = post_scale; a.post_shift = post_shift;
    return a;
}

// the rules the learned-variance entries share (who-prefixed, VDX_ERR_INVALID)
static int lv_rules(const char* who, int S, int timesteps, int batch, int channels, long per_sample) {
    if (batch < 1 || channels < 1 || per_sample < 1) VDX_REFUSE(who, "batch, channels and per_sample must be >= 1");
    if (per_sample % channels) VDX_REFUSE(who, "per_sample must be a multiple of channels");
    if (S < 1 || S > timesteps) VDX_REFUSE(who, "S must be in [1, timesteps]");
    return VDX_OK;
}

int vdx_p_sample_step_lv(const float* x, const float* out2, float* out, const int* level_dev, const float* lv_tables, int S, uint64_t step,
                         const uint64_t* step_dev, const float* noise, uint64_t seed, uint64_t offset, const uint64_t* dev_offset,
                         int clip_denoised, float post_scale, float post_shift, int batch, int channels, long per_sample, void* stream) {
    const char* who = "p_sample_step_lv";
    if (!x || !out2 || !out || !lv_tables) VDX_REFUSE(who, "null tensor");
    if (int rc = lv_rules(who, S, S, batch, channels, per_sample)) return rc;
    if (!level_dev && !step_dev && step >= (uint64_t)S) VDX_REFUSE(who, "step must be below S");
    if (!noise && per_sample % 4) VDX_REFUSE(who, "generated noise needs per_sample % 4 == 0");
    const vdx::LvStepArgs a = lv_step_args(x, out2, out, level_dev, lv_tables, S, step, step_dev, noise, seed, offset, dev_offset, clip_denoised,
                                           post_scale, post_shift, channels, per_sample);
    VDX_HIP(vdx::launch_p_sample_lv(a, batch, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_p_sample_loop_lv(vdx_handle* h, const float* params, const void* packed, float* img, float* out2_buf, int* t_dev, uint64_t* step_dev,
                         const float* lv_tables, const int* seq, int S, int timesteps, int nsteps, const float* cond, uint64_t seed,
                         int clip_denoised, float post_scale, float post_shift, void* workspace, size_t workspace_bytes, int batch,
                         int use_graph, void* stream) {
    const char* who = "p_sample_loop_lv";
    if (!h || !params || !packed || !img || !out2_buf || !t_dev || !step_dev || !lv_tables || !seq || !workspace) VDX_REFUSE(who, "null argument");
    if (h->pred) VDX_FAIL(VDX_ERR_STATE, "p_sample_loop_lv: v-prediction (vdx_set_prediction) has no learned-variance form");
    if (h->sc) VDX_FAIL(VDX_ERR_STATE, "p_sample_loop_lv: self-conditioning (vdx_set_self_condition) has no learned-variance form");
    const vdx::Model& m = h->model;
    const int C = m.cfg.channels;
    const long per_sample = (long)C * m.cfg.num_frames * m.cfg.image_size * m.cfg.image_size;
    if (m.out_dim != 2 * C) VDX_REFUSE(who, "out_dim must equal 2 * channels");
    if (int rc = lv_rules(who, S, timesteps, batch, C, per_sample)) return rc;
    if (per_sample % 4) VDX_REFUSE(who, "C*F*H*W must be a multiple of 4");
    if (nsteps < 0 || nsteps > S) VDX_REFUSE(who, "nsteps out of range");
    if (!m.d_ss_layers) { char msg_[96]; snprintf(msg_, sizeof(msg_), "%s: handle was created without a GPU", who); VDX_FAIL(VDX_ERR_STATE, msg_); }
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* sd = reinterpret_cast<unsigned long long*>(step_dev);
    const vdx::LvStepArgs sa = lv_step_args(img, out2_buf, img, nullptr, lv_tables, S, 0, step_dev, nullptr, seed, 1, step_dev, clip_denoised, post_scale,
                                            post_shift, C, per_sample);
    auto step = [&]() -> int {
        // cond is used un-masked, as in the unguided sampling loops
        int rc = vdx::model_forward(&m, params, packed, img, t_dev, cond, nullptr, 0, out2_buf, workspace, workspace_bytes, batch, st);
        if (rc != VDX_OK) return rc;
        hipError_t e = vdx::launch_p_sample_lv(sa, batch, st);
        if (e == hipSuccess) e = vdx::launch_ddim_advance(t_dev, batch, seq, sd, st);
        if (e != hipSuccess) return vdx_set_error(VDX_ERR_HIP, hipGetErrorString(e), __FILE__, __LINE__);
        return VDX_OK;
    };
    vdx_handle::GraphKey key;
    memset(&key, 0, sizeof(key));
    LoopArgs& k = key.a;
    k.chain = CHAIN_LV; k.params = params; k.packed = packed; k.img = img; k.eps_buf = out2_buf; k.t_dev = t_dev; k.step_dev = step_dev;
    k.tables = lv_tables; k.timesteps = timesteps; k.seq = seq; k.seq_len = S; k.cond = cond; k.seed = seed; k.clip_denoised = clip_denoised ? 1 : 0;
    k.post_scale = post_scale; k.post_shift = post_shift;
    k.workspace = workspace; k.workspace_bytes = workspace_bytes; k.batch = batch;
    key.stream = stream; key.act16 = m.act16;
    return run_steps(h, 10, key, nsteps, use_graph, st, step);
}

size_t vdx_hybrid_scratch_doubles(int batch) { return batch > 0 ? vdx::hybrid_scratch_doubles(batch) : 0; }

static int hybrid_loss_call(const char* who, const float* x, const float* noise, const float* out2, const int* t, const double* lv_tables64,
                            int timesteps, float pre_scale, float pre_shift, int l2, double vlb_weight, int want_grad, float* d_out,
                            double* scratch, double* out, const double* iw, int batch, int channels, long per_sample, void* stream) {
    if (!x || !noise || !out2 || !t || !lv_tables64 || !scratch || !out) VDX_REFUSE(who, "null tensor");
    if (want_grad && !d_out) VDX_REFUSE(who, "want_grad needs d_out");
    if (int rc = lv_rules(who, 1, 1, batch, channels, per_sample)) return rc;
    if (timesteps < 2) VDX_REFUSE(who, "timesteps must be >= 2");
    if ((uintptr_t)x % 16 || (uintptr_t)noise % 16) VDX_REFUSE(who, "x / noise must be 16-byte aligned");
    if ((uintptr_t)lv_tables64 % 8 || (uintptr_t)scratch % 8 || (uintptr_t)out % 8) VDX_REFUSE(who, "lv_tables64 / scratch / out must be 8-byte aligned");
    const double n = (double)batch * (double)per_sample;
    vdx::HybridArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.noise = noise; a.out2 = out2; a.d_out = want_grad ? d_out : nullptr; a.t = t; a.tab = lv_tables64; a.T = timesteps;
    a.l2 = l2 ? 1 : 0; a.C = channels; a.per_sample = per_sample; a.pre_scale = pre_scale; a.pre_shift = pre_shift;
    a.inv_count = 1.0f / (float)((long)batch * per_sample); a.vscale = vlb_weight / (n * 0.69314718055994530942); a.partial = scratch;
    a.iw = iw; a.inv_count64 = 1.0 / n;
    VDX_HIP(vdx::launch_hybrid_loss(a, out, vlb_weight, batch, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_hybrid_loss(const float* x, const float* noise, const float* out2, const int* t, const double* lv_tables64, int timesteps,
                    float pre_scale, float pre_shift, int l2, double vlb_weight, int want_grad, float* d_out, double* scratch, double* out,
                    int batch, int channels, long per_sample, void* stream) {
    return hybrid_loss_call("hybrid_loss", x, noise, out2, t, lv_tables64, timesteps, pre_scale, pre_shift, l2, vlb_weight, want_grad, d_out, scratch,
                            out, nullptr, batch, channels, per_sample, stream);
}

int vdx_hybrid_loss_w(const float* x, const float* noise, const float* out2, const int* t, const double* lv_tables64, int timesteps,
                      float pre_scale, float pre_shift, int l2, double vlb_weight, int want_grad, float* d_out, double* scratch, double* out,
                      int batch, int channels, long per_sample, const double* iw, void* stream) {
    if ((uintptr_t)iw % 8) VDX_REFUSE("hybrid_loss_w", "iw must be 8-byte aligned");
    return hybrid_loss_call("hybrid_loss_w", x, noise, out2, t, lv_tables64, timesteps, pre_scale, pre_shift, l2, vlb_weight, want_grad, d_out,
                            scratch, out, iw, batch, channels, per_sample, stream);
}

// ---- loss-aware timestep sampling (vdx.h: "Loss-aware timestep sampling") ----

int vdx_tsampler_draw(const double* hist, const int* count, int timesteps, int history, double uniform_prob, const int* t_given, uint64_t seed,
                      uint64_t draw, int* t_out, double* iw_out, double* p_out, int batch, void* stream) {
    const char* who = "tsampler_draw";
    if (timesteps < 1 || timesteps > 4096) VDX_REFUSE(who, "timesteps must be in [1, 4096]");
    if (history < 1 || history > 32) VDX_REFUSE(who, "history must be in [1, 32]");
    if (!(uniform_prob > 0.0 && uniform_prob <= 1.0)) VDX_REFUSE(who, "uniform_prob must be in (0, 1]");
    if (batch < 1) VDX_REFUSE(who, "batch must be >= 1");
    if (!hist || !count || !t_out || !iw_out) VDX_REFUSE(who, "null tensor");
    if ((uintptr_t)hist % 8 || (uintptr_t)iw_out % 8 || (uintptr_t)p_out % 8) VDX_REFUSE(who, "hist / iw_out / p_out must be 8-byte aligned");
    VDX_HIP(vdx::launch_tsampler_draw(hist, count, timesteps, history, uniform_prob, t_given, seed, draw, t_out, iw_out, p_out, batch,
                                      (hipStream_t)stream));
    return VDX_OK;
}

int vdx_tsampler_update(double* hist, int* count, int timesteps, int history, const double* entries, int n, void* stream) {
    const char* who = "tsampler_update";
    if (timesteps < 1 || timesteps > 4096) VDX_REFUSE(who, "timesteps must be in [1, 4096]");
    if (history < 1 || history > 32) VDX_REFUSE(who, "history must be in [1, 32]");
    if (n < 0) VDX_REFUSE(who, "n must be >= 0");
    if (!hist || !count || (n > 0 && !entries)) VDX_REFUSE(who, "null tensor");
    if ((uintptr_t)hist % 8 || (uintptr_t)entries % 8) VDX_REFUSE(who, "hist / entries must be 8-byte aligned");
    if (n == 0) return VDX_OK;
    VDX_HIP(vdx::launch_tsampler_update(hist, count, timesteps, history, entries, n, (hipStream_t)stream));
    return VDX_OK;
}

size_t vdx_loss_weighted_scratch_doubles(int batch) { return batch > 0 ? vdx::loss_weighted_scratch_doubles(batch) : 0; }

int vdx_loss_weighted(const float* eps_hat, const float* noise, const double* iw, float* d_eps_hat, double* scratch, double* out, int batch,
                      int channels, long fhw, int l2, void* stream) {
    const char* who = "loss_weighted";
    if (!eps_hat || !noise || !scratch || !out) VDX_REFUSE(who, "null tensor");
    if (batch < 1 || channels < 1 || fhw < 1) VDX_REFUSE(who, "batch, channels and fhw must be >= 1");
    if ((uintptr_t)iw % 8 || (uintptr_t)scratch % 8 || (uintptr_t)out % 8) VDX_REFUSE(who, "iw / scratch / out must be 8-byte aligned");
    VDX_HIP(vdx::launch_loss_weighted(eps_hat, noise, iw, d_eps_hat, scratch, out, batch, channels, fhw, l2 ? 1 : 0, (hipStream_t)stream));
    return VDX_OK;
}

// ---- v-prediction (vdx.h: "v-prediction") ----

int vdx_v_to_eps(float* out, const float* x, const int* t, const float* sqrt_ac, const float* sqrt_1mac, int timesteps, int rows, int channels,
                 long per_sample, void* stream) {
    const char* who = "v_to_eps";
    if (!out || !x || !t || !sqrt_ac || !sqrt_1mac) VDX_REFUSE(who, "null tensor");
    if (rows < 1 || channels < 1 || timesteps < 1 || per_sample < 1) VDX_REFUSE(who, "rows, channels, timesteps and per_sample must be >= 1");
    if (per_sample % channels) VDX_REFUSE(who, "per_sample must be a multiple of channels");
    VDX_HIP(vdx::launch_v_to_eps(out, x, t, sqrt_ac, sqrt_1mac, timesteps, rows, channels, per_sample, (hipStream_t)stream));
    return VDX_OK;
}

// ---- self-conditioning (vdx.h: "Self-conditioning") ----

int vdx_selfcond_x0(const float* x, long x_pitch, const float* eps_hat, const int* t, const float* tables, int timesteps, const float* thres,
                    int clip_denoised, float* xin, int batch, int channels, long per_sample, void* stream) {
    const char* who = "selfcond_x0";
    if (!x || !eps_hat || !t || !tables || !xin) VDX_REFUSE(who, "null tensor");
    if (batch < 1 || channels < 1 || timesteps < 1 || per_sample < 1) VDX_REFUSE(who, "batch, channels, timesteps and per_sample must be >= 1");
    if (per_sample % channels) VDX_REFUSE(who, "per_sample must be a multiple of channels");
    if (x_pitch < per_sample) VDX_REFUSE(who, "x_pitch must be >= per_sample");
    if ((uintptr_t)x % 4 || (uintptr_t)eps_hat % 4 || (uintptr_t)xin % 4) VDX_REFUSE(who, "x / eps_hat / xin must be 4-byte aligned");
    const vdx::SelfcondArgs a = {x, x_pitch, eps_hat, t, tables, timesteps, thres, clip_denoised ? 1 : 0, xin, channels, per_sample};
    VDX_HIP(vdx::launch_selfcond_x0(a, batch, (hipStream_t)stream));
    return VDX_OK;
}

size_t vdx_v_loss_scratch_doubles(int batch) { return batch > 0 ? vdx::v_loss_scratch_doubles(batch) : 0; }

int vdx_v_loss(const float* out, const float* x0, const float* noise, const int* t, const float* sqrt_ac, const float* sqrt_1mac,
               const double* wtab, const double* iw, int timesteps, int kind, float pre_scale, float pre_shift, int l2, float* d_out,
               double* scratch, double* result, int batch, int channels, long fhw, void* stream) {
    const char* who = "v_loss";
    if (kind != 0 && kind != 1) VDX_REFUSE(who, "kind 0 (target noise) or 1 (target v)");
    if (!out || !noise || !scratch || !result) VDX_REFUSE(who, "null tensor");
    if (kind == 1 && (!x0 || !sqrt_ac || !sqrt_1mac)) VDX_REFUSE(who, "kind 1 needs x0 and both tables");
    if ((kind == 1 || wtab) && (!t || timesteps < 1)) VDX_REFUSE(who, "levels: t and timesteps >= 1");
    if (batch < 1 || channels < 1 || fhw < 1) VDX_REFUSE(who, "batch, channels and fhw must be >= 1");
    if ((uintptr_t)wtab % 8 || (uintptr_t)iw % 8 || (uintptr_t)scratch % 8 || (uintptr_t)result % 8)
        VDX_REFUSE(who, "wtab / iw / scratch / result must be 8-byte aligned");
    vdx::VLossArgs a;
    memset(&a, 0, sizeof(a));
    a.out = out; a.x0 = kind ? x0 : nullptr; a.noise = noise; a.d_out = d_out; a.t = t; a.sqrt_ac = sqrt_ac; a.sqrt_1mac = sqrt_1mac; a.T = timesteps;
    a.wtab = wtab; a.iw = iw; a.kind = kind; a.l2 = l2 ? 1 : 0; a.C = channels; a.fhw = fhw; a.pre_scale = pre_scale; a.pre_shift = pre_shift;
    VDX_HIP(vdx::launch_v_loss(a, scratch, result, batch, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_vlb_terms_lv(const float* x, const float* out2, const int* t, const double* lv_tables64, int timesteps, const float* noise,
                     uint64_t seed, uint64_t draw, const uint64_t* step_dev, int clip_denoised, double* partial, double* out, int batch,
                     int channels, long per_sample, void* stream) {
    const char* who = "vlb_terms_lv";
    if (!x || !out2 || !t || !lv_tables64 || !partial || !out) VDX_REFUSE(who, "null tensor");
    if (int rc = vlb_rules(who, x, nullptr, noise, "x / noise", lv_tables64, partial, out, timesteps, batch, channels, per_sample)) return rc;
    const vdx::VlbArgs a = vlb_args(x, out2, nullptr, noise, t, lv_tables64, timesteps, seed, draw, step_dev, clip_denoised, channels, per_sample, partial);
    VDX_HIP(vdx::launch_vlb_terms_lv(a, batch, (hipStream_t)stream));
    VDX_HIP(vdx::launch_vlb_advance(partial, out, 3, batch, per_sample, nullptr, nullptr, 0, nullptr, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_vlb_loop_lv(vdx_handle* h, const float* params, const void* packed, const float* x, float* xt_buf, float* out2_buf, int* t_dev,
                    uint64_t* step_dev, const double* lv_tables64, int timesteps, const int* seq, int seq_len, int nsteps, const float* cond,
                    uint64_t seed, int clip_denoised, double* partial, double* out, void* workspace, size_t workspace_bytes, int batch,
                    int use_graph, void* stream) {
    return vlb_loop("vlb_loop_lv", true, h, params, packed, x, xt_buf, out2_buf, t_dev, step_dev, lv_tables64, timesteps, seq, seq_len, nsteps, cond, seed,
                    clip_denoised, partial, out, workspace, workspace_bytes, batch, use_graph, stream);
}

int vdx_pack_conv_weights_t(int mode, const float* kernel, void* packed, int taps, int cin, int cout, void* stream) {
    if (!kernel || !packed || taps <= 0 || cin <= 0 || cout <= 0) VDX_FAIL(VDX_ERR_INVALID, "pack_conv_weights_t: bad argument");
    if (!mode_ok(mode)) VDX_FAIL(VDX_ERR_INVALID, "bad mode");
    VDX_HIP(vdx::launch_pack_weights_t(mode, kernel, packed, taps, cin, cout, (hipStream_t)stream));
    return VDX_OK;
}

}  // extern "C" (a template needs C++ linkage)

// ---- the conv weight gradient.  What vdx_wgrad_desc and vdx_wgrad_ex_desc share, under the same field names: the rules of the wgrad
// kernels and the arguments of the plain form
template <class Desc>
static int wgrad_args(vdx::WgradArgs& a, const char* who, const Desc* d) {
    if (!d || !d->x0 || !d->dy || !d->dw) VDX_REFUSE(who, "null tensor");
    if (d->c0 < 4 || d->c0 % 4 || d->c1 < 0 || d->c1 % 4 || d->cout < 4 || d->cout % 4 || (d->c1 && !d->x1)) VDX_REFUSE(who, "bad channels");
    if (d->batch < 1 || d->frames < 1 || d->h < 1 || d->w < 1) VDX_REFUSE(who, "bad geometry");
    if (d->kind == 0 && (d->kh != d->kw || d->kh < 1 || d->kh > 4 || (d->stride != 1 && d->stride != 2))) VDX_REFUSE(who, "unsupported kernel/stride");
    memset(&a, 0, sizeof(a));
    a.x0 = (const float*)d->x0; a.x1 = (const float*)d->x1; a.C0 = d->c0; a.C1 = d->c1; a.dy = (const float*)d->dy; a.Cout = d->cout; a.dW = d->dw;
    a.NF = d->batch * d->frames; a.F = d->frames; a.H = d->h; a.W = d->w;
    a.kind = d->kind; a.kh = d->kind ? 4 : d->kh; a.kw = d->kind ? 4 : d->kw; a.stride = d->kind ? 1 : d->stride;
    if (d->in_stats) {
        if (d->c1 || !d->gamma || !d->beta || d->groups <= 0 || d->groups > 32 || d->c0 % d->groups) VDX_REFUSE(who, "bad prologue");
        if (d->scale_shift && d->scale_shift_stride < 2 * d->c0) VDX_REFUSE(who, "scale_shift rows hold scale[c0] | shift[c0]");
        a.pro = 1; a.in_stats = d->in_stats; a.gamma = d->gamma; a.beta = d->beta; a.groups = d->groups; a.ss = d->scale_shift; a.ss_stride = d->scale_shift_stride;
    }
    a.bf16_mma = d->bf16_operands ? 1 : 0;
    return VDX_OK;
}

extern "C" {

int vdx_conv_backward_weights(const vdx_wgrad_desc* d, void* stream) {
    vdx::WgradArgs a;
    if (int rc = wgrad_args(a, "conv_backward_weights", d)) return rc;
    VDX_HIP(vdx::launch_conv_wgrad(a, (hipStream_t)stream));
    return VDX_OK;
}

// ---- the norm + activation backward: vdx_norm_act_backward is the _ex form on fp32 tensors without the deterministic rows
static int norm_act_bwd(const char* who, const float* dact, const void* y, int y_bf16, void* dy, int dy_bf16, const double* stats, const float* gamma,
                        const float* beta, int groups, const float* scale_shift, int scale_shift_stride, float* d_gamma, float* d_beta, float* dss,
                        const void* r, int r_bf16, const float* ln_gamma, float* dr, float* d_ln_gamma, float* d_ln_beta, float* scratch, float* dgp, int c,
                        int batch, long pix_per_sample, void* stream) {
    if (!dact || !y || !dy || !stats || !gamma || !beta || !d_gamma || !d_beta || !scratch) VDX_REFUSE(who, "null tensor");
    if (r && (!ln_gamma || !dr || !d_ln_gamma || !d_ln_beta)) VDX_REFUSE(who, "incomplete LayerNorm branch");
    if (r_bf16 && !r) VDX_REFUSE(who, "r_bf16 without r");
    if (c < 4 || c % 4 || c > 1024 || groups < 1 || groups > 32 || c % groups || batch < 1 || pix_per_sample < 1) VDX_REFUSE(who, "bad channels/groups/shape");
    if (scale_shift && scale_shift_stride < 2 * c) VDX_REFUSE(who, "scale_shift rows hold scale[c] | shift[c]");
    vdx::NormBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.dact = dact; a.y = (const float*)y; a.y_bf16 = y_bf16 ? 1 : 0; a.dy = (float*)dy; a.dy_bf16 = dy_bf16 ? 1 : 0;
    a.stats = stats; a.gamma = gamma; a.beta = beta; a.groups = groups;
    a.ss = scale_shift; a.ss_stride = scale_shift_stride; a.d_gamma = d_gamma; a.d_beta = d_beta; a.dss = dss;
    a.r = (const float*)r; a.r_bf16 = r_bf16 ? 1 : 0; a.ln_gamma = ln_gamma; a.dr = dr; a.d_ln_gamma = d_ln_gamma; a.d_ln_beta = d_ln_beta;
    a.R = scratch; a.G = scratch + (vdx::norm_bwd_scratch_floats(c, batch, pix_per_sample) - (size_t)batch * 64);
    a.dgp = dgp; a.C = c; a.batch = batch; a.pix_per_sample = pix_per_sample;
    VDX_HIP(vdx::launch_norm_bwd(a, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_norm_act_backward(const float* dact, const float* y, float* dy, const double* stats, const float* gamma, const float* beta,
                          int groups, const float* scale_shift, int scale_shift_stride, float* d_gamma, float* d_beta, float* dss,
                          const float* r, const float* ln_gamma, float* dr, float* d_ln_gamma, float* d_ln_beta, float* scratch,
                          int c, int batch, long pix_per_sample, void* stream) {
    return norm_act_bwd("norm_act_backward", dact, y, 0, dy, 0, stats, gamma, beta, groups, scale_shift, scale_shift_stride, d_gamma, d_beta, dss, r, 0, ln_gamma,
                        dr, d_ln_gamma, d_ln_beta, scratch, nullptr, c, batch, pix_per_sample, stream);
}

size_t vdx_norm_act_backward_scratch_floats(int c, int batch, long pix_per_sample) {
    if (c < 4 || c % 4 || c > 1024 || batch < 1 || pix_per_sample < 1) return 0;
    return vdx::norm_bwd_scratch_floats(c, batch, pix_per_sample);
}

// ---- the attention core backward.  What its five entries share: the pixel geometry as the network builds it (attn_pixel_geometry), the
// lengths the cores serve and the outputs' layout.  dk == dv == null: one [rows][dq | dk | dv] buffer at dq with row stride dstride
// (split_dqkv); else three tensors of row stride heads * 32
static int attn_bwd_args(vdx::AttnBwdArgs& a, const char* who, const void* qkv, const void* d_o, void* o, void* dq, void* dk, void* dv, int dstride,
                         int io_bf16, int batch, int frames, int h, int w, int heads, int temporal, int bf16_operands) {
    const bool interleaved = !dk && !dv;
    if (!qkv || !d_o || !o || !dq || (!dk != !dv) || heads < 1 || batch < 1 || frames < 1 || h < 1 || w < 1) VDX_REFUSE(who, "bad argument");
    const int HD = heads * 32;
    if (interleaved && (dstride < 3 * HD || dstride % 8)) VDX_REFUSE(who, "dstride must be a multiple of 8, at least 3 * heads * 32 (one [rows][dq|dk|dv] buffer)");
    memset(&a, 0, sizeof(a));
    vdx::attn_pixel_geometry(a, batch, frames, h, w, temporal != 0);
    if (a.L > 64 && temporal) VDX_REFUSE(who, "temporal sequences of more than 64 frames are not served");
    if (a.L > 64 && !vdx::attn_bwd_long_served(a.L)) VDX_REFUSE(who, "above 64 tokens per sequence only multiples of 64 up to 640 are served");
    // bf16 tensors exist for the bf16 MFMA kernel only (vdx_internal.h AttnBwdArgs::io_bf16): never hand bf16 pointers to the fp32 kernel
    if (io_bf16 && (!bf16_operands || a.L > 16)) VDX_REFUSE(who, "bf16 tensors need bf16_operands and at most 16 tokens per sequence");
    a.qkv = (const float*)qkv; a.dO = (const float*)d_o; a.O = (float*)o; a.heads = heads; a.scale = 1.0f / sqrtf(32.0f);
    a.dq = (float*)dq; a.dk = (float*)dk; a.dv = (float*)dv;
    if (interleaved) vdx::split_dqkv(a.dq, HD, io_bf16, a.dk, a.dv);
    a.dstride = interleaved ? dstride : HD; a.io_bf16 = io_bf16 ? 1 : 0; a.bf16_mma = bf16_operands ? 1 : 0;
    return VDX_OK;
}

int vdx_attention_core_backward(const float* qkv, const float* d_o, float* o, float* dq, float* dk, float* dv, int batch, int frames,
                                int h, int w, int heads, int temporal, void* stream) {
    return vdx_attention_core_backward_ex(qkv, d_o, o, dq, dk, dv, batch, frames, h, w, heads, temporal, 0, stream);
}

int vdx_attention_core_backward_ex(const float* qkv, const float* d_o, float* o, float* dq, float* dk, float* dv, int batch, int frames,
                                   int h, int w, int heads, int temporal, int bf16_operands, void* stream) {
    const char* who = "attention_core_backward";
    if (!dk || !dv) VDX_REFUSE(who, "bad argument");
    vdx::AttnBwdArgs a;
    if (int rc = attn_bwd_args(a, who, qkv, d_o, o, dq, dk, dv, 0, 0, batch, frames, h, w, heads, temporal, bf16_operands)) return rc;
    VDX_HIP(vdx::launch_attn_core_bwd(a, (hipStream_t)stream));
    return VDX_OK;
}

// vdx_attention_core_backward_bias and _focus: the interleaved form on the fixed grid of <= 64 tokens.  focus_form: the mask is required
// and bias / dbias / scratch are optional (null together); else the bias is required and there is no mask
static int attn_core_bwd_fixed_grid(const char* who, bool focus_form, const void* qkv, const void* d_o, void* o, void* dqkv, int dstride, int io_bf16,
                                    const float* bias, float* dbias, float* scratch, size_t scratch_floats, const unsigned char* focus_dev, int focus_n,
                                    int batch, int frames, int h, int w, int heads, int temporal, int bf16_operands, void* stream) {
    // (before the null checks: a caller that sizes the scratch by vdx_attention_bias_backward_scratch_floats has none above 64 tokens)
    if ((temporal ? (long)frames : (long)h * w) > 64) VDX_REFUSE(who, "this form serves at most 64 tokens per sequence (the plain core alone goes beyond)");
    if (focus_form ? (!focus_dev || focus_n < 1) : (!bias || !dbias || !scratch)) VDX_REFUSE(who, "bad argument");
    if ((bias != nullptr) != (dbias != nullptr)) VDX_REFUSE(who, "bias and dbias come together");
    vdx::AttnBwdArgs a;
    if (int rc = attn_bwd_args(a, who, qkv, d_o, o, dqkv, nullptr, nullptr, dstride, io_bf16, batch, frames, h, w, heads, temporal, bf16_operands)) return rc;
    if (bias && (!scratch || scratch_floats < vdx::attn_bwd_bias_scratch_floats(heads, a.L))) VDX_REFUSE(who, "scratch too small (vdx_attention_bias_backward_scratch_floats)");
    if (bias) { a.bias = bias; a.dbias = dbias; a.part = scratch; a.part_cap = scratch_floats; }
    if (focus_form) { a.focus = focus_dev; a.focus_n = focus_n; }
    VDX_HIP(vdx::launch_attn_core_bwd(a, (hipStream_t)stream));
    return VDX_OK;
}

// ---- the fused temporal attention backward: the plain entry is the _ex form on an fp32 x
static int attn_bwd_fused(const char* who, const void* x, int x_bf16, const float* dy, const void* packed_wqkv, const float* bqkv, const void* packed_wo_t,
                          void* o_bf16, void* dqkv_bf16, float* dx, int batch, int frames, int h, int w, void* stream) {
    if (!x || !dy || !packed_wqkv || !bqkv || !packed_wo_t || !o_bf16 || !dqkv_bf16 || !dx) VDX_REFUSE(who, "null argument");
    if (batch < 1 || frames < 1 || frames > 16 || h < 1 || w < 1) VDX_REFUSE(who, "1..16 frames");
    vdx::AttnBwdXArgs a;
    memset(&a, 0, sizeof(a));
    a.x = (const float*)x; a.x_bf16 = x_bf16 ? 1 : 0; a.g = dy; a.wqkv = packed_wqkv; a.bqkv = bqkv; a.woT = packed_wo_t; a.O = o_bf16; a.dqkv = dqkv_bf16; a.dx = dx;
    vdx::attn_pixel_geometry(a, batch, frames, h, w, true);
    a.scale = 1.0f / sqrtf(32.0f);
    VDX_HIP(vdx::launch_attn_bwd_fused(a, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_temporal_attention_backward_fused(const float* x, const float* dy, const void* packed_wqkv, const float* bqkv, const void* packed_wo_t,
                                          void* o_bf16, void* dqkv_bf16, float* dx, int batch, int frames, int h, int w, void* stream) {
    return attn_bwd_fused("temporal_attention_backward_fused", x, 0, dy, packed_wqkv, bqkv, packed_wo_t, o_bf16, dqkv_bf16, dx, batch, frames, h, w, stream);
}

size_t vdx_sla_backward_scratch_floats(int nframes, int heads) { return vdx::sla_bwd_scratch_floats(nframes, heads); }

// ---- the SLA core backward.  What its three entries share; the outputs' layout as in attn_bwd_args (256 columns per tensor)
static int sla_core_bwd(const char* who, const void* q, const void* k, const void* v, const void* d_out, void* o, void* dq, void* dk, void* dv, int dstride,
                        int io_bf16, float* scratch, int nframes, int npix, int heads, int bf16_operands, void* stream) {
    const bool interleaved = !dk && !dv;
    if (!q || !k || !v || !d_out || !o || !dq || (!dk != !dv) || !scratch || heads != 8 || nframes < 1 || npix < 1) VDX_REFUSE(who, "bad argument");
    if (interleaved && (dstride < 768 || dstride % 8)) VDX_REFUSE(who, "dstride must be a multiple of 8, at least 768 (one [rows][dq|dk|dv] buffer)");
    if (io_bf16 && !bf16_operands) VDX_REFUSE(who, "bf16 tensors need bf16_operands");
    vdx::SlaBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.q = (const float*)q; a.k = (const float*)k; a.v = (const float*)v; a.dOut = (const float*)d_out; a.O = (float*)o;
    a.dq = (float*)dq; a.dk = (float*)dk; a.dv = (float*)dv;
    if (interleaved) vdx::split_dqkv(a.dq, 256, io_bf16, a.dk, a.dv);
    a.A = scratch; a.NF = nframes; a.N = npix; a.heads = heads;
    a.dstride = interleaved ? dstride : 256; a.io_bf16 = io_bf16 ? 1 : 0; a.bf16_mma = bf16_operands ? 1 : 0;
    VDX_HIP(vdx::launch_sla_bwd(a, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_sla_core_backward(const float* q, const float* k, const float* v, const float* d_out, float* o, float* dq, float* dk, float* dv,
                          float* scratch, int nframes, int npix, int heads, void* stream) {
    return vdx_sla_core_backward_ex(q, k, v, d_out, o, dq, dk, dv, scratch, nframes, npix, heads, 0, stream);
}

int vdx_sla_core_backward_ex(const float* q, const float* k, const float* v, const float* d_out, float* o, float* dq, float* dk, float* dv,
                             float* scratch, int nframes, int npix, int heads, int bf16_operands, void* stream) {
    if (!dk || !dv) VDX_REFUSE("sla_core_backward", "bad argument");
    return sla_core_bwd("sla_core_backward", q, k, v, d_out, o, dq, dk, dv, 0, 0, scratch, nframes, npix, heads, bf16_operands, stream);
}

int vdx_colsum(const float* x, float* out, long rows, int c, void* stream) {
    if (!x || !out || rows < 0 || c < 1 || c % 4) VDX_FAIL(VDX_ERR_INVALID, "colsum: bad argument");
    if (rows) VDX_HIP(vdx::launch_colsum(x, out, rows, c, (hipStream_t)stream));
    return VDX_OK;
}

// ---- test-facing entry points for the forms only vdx_unet_backward sets on the launchers (vdx.h: "Backward forms of the network") ----

int vdx_conv_backward_weights_ex(const vdx_wgrad_ex_desc* d, void* stream) {
    const char* who = "conv_backward_weights_ex";
    vdx::WgradArgs a;
    if (int rc = wgrad_args(a, who, d)) return rc;
    if (d->kind != 0 && d->kind != 1) VDX_REFUSE(who, "bad kind");
    // only the forms model_bwd.hip launches: 1x1 and 3x3 at stride 1, Downsample 4x4 at stride 2, Upsample (kind 1)
    if (d->kind == 0) {
        const bool s1 = d->stride == 1 && d->kh == d->kw && (d->kh == 1 || d->kh == 3);
        const bool s2 = d->stride == 2 && d->kh == 4 && d->kw == 4;
        if (!s1 && !s2) VDX_REFUSE(who, "kernel/stride must be 1x1 or 3x3 at stride 1, or 4x4 at stride 2");
        if (s2 && (d->h % 2 || d->w % 2)) VDX_REFUSE(who, "stride 2 needs even H, W");
    }
    if (d->in_stats && (d->kind != 0 || d->kh != 3 || d->stride != 1 || d->split)) VDX_REFUSE(who, "the prologue form is the 3x3 stride-1 conv without split");
    if (d->split && (d->kind != 0 || d->kh != 1)) VDX_REFUSE(who, "split is the 1x1 (q|k|v projection) form");
    if ((d->x_bf16 || d->dy_bf16) && !d->bf16_operands) VDX_REFUSE(who, "bf16 tensors need bf16_operands (the exact-f32 kernel reads fp32 tensors only)");
    if (d->x_bf16 && (d->c0 % 8 || d->c1 % 8)) VDX_REFUSE(who, "bf16 inputs need channel counts that are multiples of 8");
    if (d->dy_bf16 && d->cout % 8) VDX_REFUSE(who, "a bf16 dy needs cout a multiple of 8");
    if (d->split) {
        // a 64-wide output tile never straddles two tensors (wgrad.hip); at most three targets
        if (d->split < 0 || d->split % 64 || d->cout % d->split || d->cout / d->split > 3) VDX_REFUSE(who, "split must be a multiple of 64 that divides cout into at most 3 blocks");
        const int nb = d->cout / d->split;
        if ((nb >= 2 && !d->dw1) || (nb >= 3 && !d->dw2)) VDX_REFUSE(who, "split needs dw1 / dw2");
        if (d->db && ((nb >= 2 && !d->db1) || (nb >= 3 && !d->db2))) VDX_REFUSE(who, "split with db needs db1 / db2");
    } else if (d->dw1 || d->dw2 || d->db1 || d->db2) VDX_REFUSE(who, "dw1 / dw2 / db1 / db2 need split");
    if (!d->db && (d->db1 || d->db2)) VDX_REFUSE(who, "db1 / db2 need db");
    if ((d->scratch == nullptr) != (d->scratch_floats == 0)) VDX_REFUSE(who, "scratch and scratch_floats go together");
    a.dW1 = d->dw1; a.dW2 = d->dw2; a.db = d->db; a.db1 = d->db1; a.db2 = d->db2; a.split = d->split;
    a.x0_bf16 = d->x_bf16 ? 1 : 0; a.dy_bf16 = d->dy_bf16 ? 1 : 0;
    a.part = d->scratch; a.part_cap = d->scratch_floats;
    VDX_HIP(vdx::launch_conv_wgrad(a, (hipStream_t)stream));
    return VDX_OK;
}

size_t vdx_wgrad_scratch_floats(void) { return vdx::WG_PART_FLOATS; }

int vdx_slot_sum(const float* part, int nslots, size_t slot_stride, long e, int cout, int split, float* d0, float* d1, float* d2, void* stream) {
    if (!part || !d0 || nslots < 1 || e < 1 || slot_stride < (size_t)e) VDX_FAIL(VDX_ERR_INVALID, "slot_sum: bad argument");
    if (split) {
        if (split < 0 || cout < 1 || cout % split || cout / split > 3 || e % cout) VDX_FAIL(VDX_ERR_INVALID, "slot_sum: split must divide cout into at most 3 blocks, cout must divide e");
        const int nb = cout / split;
        if ((nb >= 2 && !d1) || (nb >= 3 && !d2)) VDX_FAIL(VDX_ERR_INVALID, "slot_sum: split needs d1 / d2");
    }
    VDX_HIP(vdx::launch_slot_sum(part, nslots, slot_stride, e, cout, split, d0, d1, d2, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_norm_act_backward_ex(const float* dact, const void* y, int y_bf16, void* dy, int dy_bf16, const double* stats, const float* gamma,
                             const float* beta, int groups, const float* scale_shift, int scale_shift_stride, float* d_gamma, float* d_beta,
                             float* dss, const void* r, int r_bf16, const float* ln_gamma, float* dr, float* d_ln_gamma, float* d_ln_beta,
                             float* scratch, float* dgp, int c, int batch, long pix_per_sample, void* stream) {
    return norm_act_bwd("norm_act_backward_ex", dact, y, y_bf16, dy, dy_bf16, stats, gamma, beta, groups, scale_shift, scale_shift_stride, d_gamma, d_beta, dss, r,
                        r_bf16, ln_gamma, dr, d_ln_gamma, d_ln_beta, scratch, dgp, c, batch, pix_per_sample, stream);
}

int vdx_attention_core_backward_io(const void* qkv, const void* d_o, void* o, void* dqkv, int dstride, int io_bf16, int batch, int frames,
                                   int h, int w, int heads, int temporal, int bf16_operands, void* stream) {
    vdx::AttnBwdArgs a;
    if (int rc = attn_bwd_args(a, "attention_core_backward_io", qkv, d_o, o, dqkv, nullptr, nullptr, dstride, io_bf16, batch, frames, h, w, heads, temporal, bf16_operands)) return rc;
    VDX_HIP(vdx::launch_attn_core_bwd(a, (hipStream_t)stream));
    return VDX_OK;
}

size_t vdx_attention_bias_backward_scratch_floats(int heads, int tokens) {
    return (heads < 1 || tokens < 1 || tokens > 64) ? 0 : vdx::attn_bwd_bias_scratch_floats(heads, tokens);
}

int vdx_attention_core_backward_bias(const void* qkv, const void* d_o, void* o, void* dqkv, int dstride, int io_bf16, const float* bias,
                                     float* dbias, float* scratch, size_t scratch_floats, int batch, int frames, int h, int w, int heads,
                                     int temporal, int bf16_operands, void* stream) {
    return attn_core_bwd_fixed_grid("attention_core_backward_bias", false, qkv, d_o, o, dqkv, dstride, io_bf16, bias, dbias, scratch, scratch_floats, nullptr, 0,
                                    batch, frames, h, w, heads, temporal, bf16_operands, stream);
}

int vdx_attention_core_backward_focus(const void* qkv, const void* d_o, void* o, void* dqkv, int dstride, int io_bf16, const float* bias_or_null,
                                      float* dbias_or_null, float* scratch, size_t scratch_floats, const unsigned char* focus_dev, int focus_n,
                                      int batch, int frames, int h, int w, int heads, int temporal, int bf16_operands, void* stream) {
    return attn_core_bwd_fixed_grid("attention_core_backward_focus", true, qkv, d_o, o, dqkv, dstride, io_bf16, bias_or_null, dbias_or_null, scratch, scratch_floats,
                                    focus_dev, focus_n, batch, frames, h, w, heads, temporal, bf16_operands, stream);
}

int vdx_temporal_attention_backward_fused_ex(const void* x, int x_bf16, const float* dy, const void* packed_wqkv, const float* bqkv,
                                             const void* packed_wo_t, void* o_bf16, void* dqkv_bf16, float* dx, int batch, int frames, int h,
                                             int w, void* stream) {
    return attn_bwd_fused("temporal_attention_backward_fused_ex", x, x_bf16, dy, packed_wqkv, bqkv, packed_wo_t, o_bf16, dqkv_bf16, dx, batch, frames, h, w, stream);
}

int vdx_sla_core_backward_io(const void* q, const void* k, const void* v, const void* d_out, void* o, void* dqkv, int dstride, int io_bf16,
                             float* scratch, int nframes, int npix, int heads, int bf16_operands, void* stream) {
    return sla_core_bwd("sla_core_backward_io", q, k, v, d_out, o, dqkv, nullptr, nullptr, dstride, io_bf16, scratch, nframes, npix, heads, bf16_operands, stream);
}

int vdx_final_conv_backward(const void* x, int x_bf16, const float* d_out, const float* kernel, float* dx, float* dw, float* db, long npix, int d,
                            int cout, float* scratch, size_t scratch_floats, void* stream) {
    if (!x || !d_out || !kernel || !dx || !dw || !db || npix < 1) VDX_FAIL(VDX_ERR_INVALID, "final_conv_backward: bad argument");
    if (d < 4 || d % 4 || d > 256 || cout < 1 || cout > 4) VDX_FAIL(VDX_ERR_INVALID, "final_conv_backward: d a multiple of 4 up to 256, cout 1..4");
    if ((scratch == nullptr) != (scratch_floats == 0)) VDX_FAIL(VDX_ERR_INVALID, "final_conv_backward: scratch and scratch_floats go together");
    VDX_HIP(vdx::launch_final_conv_bwd((const float*)x, d_out, kernel, dx, dw, db, npix, d, cout, x_bf16 ? 1 : 0, (hipStream_t)stream, scratch, scratch_floats));
    return VDX_OK;
}

int vdx_final_conv_backward_wide(const void* x, int x_bf16, const float* d_out, const float* kernel, float* dx, float* dw, float* db, long npix,
                                 int d, int cout, float* scratch, size_t scratch_floats, void* stream) {
    if (!x || !d_out || !kernel || !dx || !dw || !db || npix < 1) VDX_FAIL(VDX_ERR_INVALID, "final_conv_backward_wide: bad argument");
    if (d < 4 || d % 4 || d > 256 || cout < 1 || cout > 6) VDX_FAIL(VDX_ERR_INVALID, "final_conv_backward_wide: d a multiple of 4 up to 256, cout 1..6");
    if ((scratch == nullptr) != (scratch_floats == 0)) VDX_FAIL(VDX_ERR_INVALID, "final_conv_backward_wide: scratch and scratch_floats go together");
    VDX_HIP(vdx::launch_final_conv_bwd((const float*)x, d_out, kernel, dx, dw, db, npix, d, cout, x_bf16 ? 1 : 0, (hipStream_t)stream, scratch, scratch_floats));
    return VDX_OK;
}

int vdx_init_conv_backward_weights(const float* x, const float* dy, float* dw, float* db, int batch, int cin, int frames, int h, int w, int cout,
                                   int k, float* scratch, size_t scratch_floats, void* stream) {
    if (!x || !dy || !dw || !db || batch < 1 || cin < 1 || frames < 1 || h < 1 || w < 1 || cout < 1) VDX_FAIL(VDX_ERR_INVALID, "init_conv_backward_weights: bad argument");
    if (k < 1 || k % 2 == 0) VDX_FAIL(VDX_ERR_INVALID, "init_conv_backward_weights: odd kernel size");
    // the staged input tile [cin][16 + k - 1]^2 + the dy tile must fit the default 64 KB of dynamic LDS
    if (((size_t)cin * (16 + k - 1) * (16 + k - 1) + 256 * 17) * 4 > 64 * 1024) VDX_FAIL(VDX_ERR_INVALID, "init_conv_backward_weights: cin * (k + 15)^2 too large for one LDS tile");
    if ((long)batch * frames > 65535 || (cout + 15) / 16 > 65535) VDX_FAIL(VDX_ERR_INVALID, "init_conv_backward_weights: batch * frames exceeds the grid");
    if ((scratch == nullptr) != (scratch_floats == 0)) VDX_FAIL(VDX_ERR_INVALID, "init_conv_backward_weights: scratch and scratch_floats go together");
    VDX_HIP(vdx::launch_init_conv_wgrad(x, dy, dw, db, batch, cin, frames, h, w, cout, k, (hipStream_t)stream, scratch, scratch_floats));
    return VDX_OK;
}

int vdx_time_mlp_backward(const int* time, const float* w1, const float* b1, const float* w2, const float* b2, int dim, const unsigned char* cond_mask,
                          int null_all, int cond_dim, const float* dtemb, float* dw1, float* db1, float* dw2, float* db2, float* dnull, int batch,
                          void* stream) {
    if (!time || !w1 || !b1 || !w2 || !b2 || !dtemb || !dw1 || !db1 || !dw2 || !db2 || batch < 1) VDX_FAIL(VDX_ERR_INVALID, "time_mlp_backward: null argument");
    if (dim < 4 || dim % 4 || cond_dim < 0) VDX_FAIL(VDX_ERR_INVALID, "time_mlp_backward: dim must be a multiple of 4");
    if (cond_dim && !dnull) VDX_FAIL(VDX_ERR_INVALID, "time_mlp_backward: cond_dim needs dnull");
    vdx::TimeMlpArgs a;
    memset(&a, 0, sizeof(a));
    a.time = time; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.dim = dim; a.time_dim = 4 * dim;
    a.cond_mask = cond_mask; a.null_all = null_all; a.cond_dim = cond_dim; a.temb_dim = a.time_dim + cond_dim;
    if ((size_t)batch * (a.dim + 2 * a.time_dim + 64) * 4 > 150 * 1024) VDX_FAIL(VDX_ERR_INVALID, "time_mlp_backward: batch too large for the LDS-resident recompute");
    VDX_HIP(vdx::launch_time_mlp_bwd(a, dtemb, dw1, db1, dw2, db2, cond_dim ? dnull : nullptr, batch, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_resblock_scale_shift_backward(const float* params, float* grads, const float* temb, const vdx_ss_layer* layers_dev, int nlayers,
                                      const float* lin, float* dss, float* dtemb, int temb_dim, int batch, float* slots, size_t slots_cap,
                                      void* stream) {
    if (!params || !grads || !temb || !layers_dev || !lin || !dss || !dtemb) VDX_FAIL(VDX_ERR_INVALID, "scale_shift_backward: null tensor");
    if (nlayers < 1 || temb_dim < 1 || batch < 1) VDX_FAIL(VDX_ERR_INVALID, "scale_shift_backward: bad geometry");
    if (temb_dim > 65535) VDX_FAIL(VDX_ERR_INVALID, "scale_shift_backward: temb_dim exceeds the grid (one row of the Linear per workgroup)");
    if ((slots == nullptr) != (slots_cap == 0)) VDX_FAIL(VDX_ERR_INVALID, "scale_shift_backward: slots and slots_cap go together");
    VDX_HIP(vdx::launch_resblock_ss_bwd(params, grads, temb, reinterpret_cast<const vdx::SsLayer*>(layers_dev), nlayers, lin, dss, dtemb, temb_dim,
                                        batch, (hipStream_t)stream, slots, slots_cap));
    return VDX_OK;
}

int vdx_num_stages(const vdx_handle* h) { return h ? 2 * h->model.cfg.n_mults + 3 : 0; }
size_t vdx_packed_bwd_bytes(const vdx_handle* h) { return h ? h->model.packed_t_bytes : 0; }
size_t vdx_bwd_workspace_bytes(const vdx_handle* h, int batch) { return h ? vdx::model_bwd_workspace_bytes(&h->model, batch) : 0; }

int vdx_pack_params_bwd(const vdx_handle* h, const float* params, void* packed_t, void* stream) {
    if (!h || !params || !packed_t) VDX_FAIL(VDX_ERR_INVALID, "pack_params_bwd: null argument");
    VDX_HIP(vdx::model_pack_t(&h->model, params, packed_t, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_unet_backward(vdx_handle* h, const float* params, const void* packed, const void* packed_t, const float* x, const int* time,
                      const float* cond, const unsigned char* cond_mask, int null_all, const float* d_out, void* fwd_workspace,
                      void* bwd_workspace, size_t bwd_workspace_bytes, float* grads, int stage_hi, int stage_lo, int batch, void* stream) {
    if (!h || !params || !packed || !packed_t || !x || !time || !d_out || !fwd_workspace || !bwd_workspace || !grads) VDX_FAIL(VDX_ERR_INVALID, "unet_backward: null argument");
    if (!h->model.d_ss_layers) VDX_FAIL(VDX_ERR_STATE, "unet_backward: handle was created without a GPU");
    if (h->model.act16 == 1) VDX_FAIL(VDX_ERR_STATE, "unet_backward: the forward ran with the INFERENCE form of bf16 activation storage (res_conv folded into the block tail); use vdx_set_activation_storage(h, 2) for a forward that feeds the backward");
    if (h->model.attn_fp8) VDX_FAIL(VDX_ERR_STATE, "unet_backward: fp8 attention is a forward (sampling) option; the backward differentiates the bf16 cores");
    // the fused q|k|v weight gradient (wgrad.hip, split = heads * 32) owns whole 64-wide output tiles per tensor
    if ((h->model.cfg.attn_heads * 32) % 64) VDX_FAIL(VDX_ERR_INVALID, "unet_backward: attn_heads must be even (heads * 32 a multiple of 64); odd head counts are forward / sampling only");
    return vdx::model_backward(&h->model, &h->bwd, params, packed, packed_t, x, time, cond, cond_mask, null_all, d_out, fwd_workspace,
                               bwd_workspace, bwd_workspace_bytes, grads, stage_hi, stage_lo, batch, (hipStream_t)stream);
}

int vdx_loss_grad(const float* eps_hat, const float* noise, float* d_eps_hat, int batch, int channels, long fhw, int l2, void* stream) {
    if (!eps_hat || !noise || !d_eps_hat || batch < 1 || channels < 1 || fhw < 1) VDX_FAIL(VDX_ERR_INVALID, "loss_grad: bad argument");
    VDX_HIP(vdx::launch_loss_grad(eps_hat, noise, d_eps_hat, batch, channels, fhw, l2, (hipStream_t)stream));
    return VDX_OK;
}

// ---- frame-conditioned training: the masked ends of the train step (float4 / uchar4 moves, as the masked sampling steps) ----

int vdx_q_sample_masked(const float* x_start, const int* t, const float* noise, const unsigned char* mask, float* out, const float* sqrt_ac,
                        const float* sqrt_one_minus_ac, int batch, long per_sample, float pre_scale, float pre_shift, void* stream) {
    if (!x_start || !t || !noise || !mask || !out || !sqrt_ac || !sqrt_one_minus_ac || batch < 1 || per_sample < 1)
        VDX_FAIL(VDX_ERR_INVALID, "q_sample_masked: bad argument");
    if (per_sample % 4) VDX_FAIL(VDX_ERR_INVALID, "q_sample_masked: per_sample must be a multiple of 4");
    if ((uintptr_t)x_start % 16 || (uintptr_t)noise % 16 || (uintptr_t)out % 16 || (uintptr_t)mask % 4)
        VDX_FAIL(VDX_ERR_INVALID, "q_sample_masked: x_start / noise / out must be 16-byte and mask 4-byte aligned");
    VDX_HIP(vdx::launch_q_sample_masked(x_start, t, noise, mask, out, sqrt_ac, sqrt_one_minus_ac, batch, per_sample, pre_scale, pre_shift,
                                        (hipStream_t)stream));
    return VDX_OK;
}

size_t vdx_loss_masked_scratch_doubles(void) { return vdx::loss_masked_scratch_doubles(); }

int vdx_loss_sum_masked(const float* eps_hat, const float* noise, const unsigned char* mask, double* scratch, double* out, int batch,
                        int channels, long fhw, int l2, void* stream) {
    if (!eps_hat || !noise || !mask || !scratch || !out || batch < 1 || channels < 1 || fhw < 1) VDX_FAIL(VDX_ERR_INVALID, "loss_sum_masked: bad argument");
    if (((long)channels * fhw) % 4) VDX_FAIL(VDX_ERR_INVALID, "loss_sum_masked: channels * fhw must be a multiple of 4");
    if ((uintptr_t)noise % 16 || (uintptr_t)mask % 4 || (uintptr_t)eps_hat % 4 || (uintptr_t)scratch % 8 || (uintptr_t)out % 8)
        VDX_FAIL(VDX_ERR_INVALID, "loss_sum_masked: noise must be 16-byte and mask 4-byte aligned");
    VDX_HIP(vdx::launch_loss_masked(eps_hat, noise, mask, scratch, out, batch, channels, fhw, l2, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_loss_grad_masked(const float* eps_hat, const float* noise, const unsigned char* mask, const double* count_dev, float* d_eps_hat,
                         int batch, int channels, long fhw, int l2, void* stream) {
    if (!eps_hat || !noise || !mask || !count_dev || !d_eps_hat || batch < 1 || channels < 1 || fhw < 1)
        VDX_FAIL(VDX_ERR_INVALID, "loss_grad_masked: bad argument");
    if (((long)channels * fhw) % 4) VDX_FAIL(VDX_ERR_INVALID, "loss_grad_masked: channels * fhw must be a multiple of 4");
    if ((uintptr_t)noise % 16 || (uintptr_t)mask % 4 || (uintptr_t)eps_hat % 4 || (uintptr_t)d_eps_hat % 4 || (uintptr_t)count_dev % 8)
        VDX_FAIL(VDX_ERR_INVALID, "loss_grad_masked: noise must be 16-byte and mask 4-byte aligned");
    VDX_HIP(vdx::launch_loss_grad_masked(eps_hat, noise, mask, count_dev, d_eps_hat, batch, channels, fhw, l2, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_adam_ema_step(float* params, const float* grads, float* m, float* v, float* ema, long n, float lr, float b1, float b2,
                      float eps, long step_count, float grad_scale, int do_ema, float ema_decay, void* stream) {
    if (!params || !grads || !m || !v || (do_ema && !ema) || n < 1 || step_count < 0) VDX_FAIL(VDX_ERR_INVALID, "adam_ema_step: bad argument");
    VDX_HIP(vdx::launch_adam_ema(params, grads, m, v, ema, n, lr, b1, b2, eps, step_count, grad_scale, do_ema, ema_decay, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_grad_accumulate(float* acc, const float* g, long n, void* stream) {
    if (!acc || !g || n < 1 || ((uintptr_t)acc & 3) || ((uintptr_t)g & 3)) VDX_FAIL(VDX_ERR_INVALID, "grad_accumulate: bad argument");
    VDX_HIP(vdx::launch_grad_accumulate(acc, g, n, (hipStream_t)stream));
    return VDX_OK;
}

size_t vdx_grad_sqnorm_scratch_doubles(void) { return vdx::grad_sqnorm_scratch_doubles(); }

int vdx_grad_sqnorm(const float* g, long n, double* scratch, double* out, void* stream) {
    if (!g || !scratch || !out || n < 1 || ((uintptr_t)g & 3)) VDX_FAIL(VDX_ERR_INVALID, "grad_sqnorm: bad argument");
    VDX_HIP(vdx::launch_grad_sqnorm(g, n, scratch, out, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_adam_ema_step_clip(float* params, const float* grads, float* m, float* v, float* ema, long n, float lr, float b1, float b2,
                           float eps, long step_count, float grad_scale, int do_ema, float ema_decay, const double* sqnorm,
                           float max_grad_norm, float* norm_out, void* stream) {
    if (!params || !grads || !m || !v || (do_ema && !ema) || !sqnorm || n < 1 || step_count < 0 || !(max_grad_norm > 0.f))
        VDX_FAIL(VDX_ERR_INVALID, "adam_ema_step_clip: bad argument");
    VDX_HIP(vdx::launch_adam_ema_clip(params, grads, m, v, ema, n, lr, b1, b2, eps, step_count, grad_scale, do_ema, ema_decay, sqnorm,
                                      max_grad_norm, norm_out, (hipStream_t)stream));
    return VDX_OK;
}

int vdx_comm_unique_id(void* unique_id_out) {
    if (!unique_id_out) VDX_FAIL(VDX_ERR_INVALID, "comm_unique_id: null argument");
    return vdx::comm_unique_id(unique_id_out);
}

int vdx_comm_init(vdx_handle* h, int rank, int world, const void* unique_id) {
    if (!h || !unique_id || world < 1 || rank < 0 || rank >= world) VDX_FAIL(VDX_ERR_INVALID, "comm_init: bad argument");
    return vdx::comm_init(&h->comm, rank, world, unique_id);
}

int vdx_allreduce_bucket(vdx_handle* h, float* ptr, size_t count, void* stream) {
    if (!h || !ptr) VDX_FAIL(VDX_ERR_INVALID, "allreduce_bucket: null argument");
    if (count == 0) return VDX_OK;
    return vdx::comm_allreduce(&h->comm, ptr, count, (hipStream_t)stream);
}

int vdx_comm_world(const vdx_handle* h) { return h ? h->comm.world : 1; }

int vdx_comm_destroy(vdx_handle* h) {
    if (!h) VDX_FAIL(VDX_ERR_INVALID, "comm_destroy: null handle");
    vdx::comm_destroy(&h->comm);
    return VDX_OK;
}

}  // extern "C"
