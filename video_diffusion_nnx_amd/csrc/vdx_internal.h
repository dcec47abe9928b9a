// Internal (non-ABI) declarations shared by the kernel translation units and the host runtime.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <algorithm>
#include <type_traits>
#include "../../include/vdx.h"

int vdx_set_error(int code, const char* msg, const char* file, int line);

namespace vdx {

// A kernel launched with more than the default 64 KB of dynamic LDS has to opt in first; at or below it nothing is set.
template <typename K>
inline hipError_t lds_opt_in(K kfn, size_t lds) {
    if (lds <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// Instrumentation hook (vdx.h: vdx_set_launch_hook).  A LaunchScope brackets ONE kernel launch: its constructor calls the hook with
// phase 0, its destructor with phase 1.  Costs one load + branch when no hook is installed (nothing is formatted then).
// Every instrumented launch is one expression, LaunchScope(st, kernel, flops, bytes, label...).launch(kfn, grid, block, lds, args...):
// hook, LDS opt-in, launch, hipGetLastError() in that order everywhere, so the hook has seen the route of a call before its first
// runtime call can fail (tests/test_host_routes.py reads the routes on a machine without a device).
extern vdx_launch_hook g_launch_hook;
extern void* g_launch_hook_user;
struct LaunchScope {
    vdx_launch_info info; char desc[192]; hipStream_t st; bool on;
    LaunchScope(hipStream_t s, const char* kernel, double flops, double bytes, const char* fmt, ...) __attribute__((format(printf, 6, 7))) : st(s), on(g_launch_hook != nullptr) {
        if (!on) return;
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(desc, sizeof(desc), fmt, ap);
        va_end(ap);
        info.kernel = kernel; info.shape = desc; info.flops = flops; info.bytes = bytes;
        g_launch_hook(g_launch_hook_user, 0, &info, st);
    }
    ~LaunchScope() { if (on && g_launch_hook) g_launch_hook(g_launch_hook_user, 1, &info, st); }
    template <typename K, typename... A>
    hipError_t launch(K kfn, dim3 grid, dim3 block, size_t lds, const A&... args) {
        if (hipError_t e = lds_opt_in(kfn, lds); e != hipSuccess) return e;
        hipLaunchKernelGGL(kfn, grid, block, lds, st, args...);
        return hipGetLastError();
    }
    LaunchScope(const LaunchScope&) = delete;
    LaunchScope& operator=(const LaunchScope&) = delete;
};

// Compute units of the current device (256 when the query fails): the width of the persistent launches.
inline int device_cus() {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v; }
    return cus;
}

// Persistent split of `total` (>= 1) work items over at most `slots` workers (workgroups or waves): each worker walks `per` consecutive
// items; `workers` of them get work.
struct PersistentSplit { long per, workers; };
inline PersistentSplit persistent_split(long total, long slots) {
    const long n = std::min(total, slots);
    const long per = (total + n - 1) / n;
    return {per, (total + per - 1) / per};
}

// Arguments of conv_igemm_kernel (POD, passed by value).  Caller fills the first block; launch_conv
// completes the geometry.
struct ConvArgs {
    // tensors (channel-last fp32): input = concat(x0[.., C0], x1[.., C1]) on the channel axis
    const float* x0; const float* x1; int C0, C1;
    const void* wp;                 // packed weights [taps][Cout][CinPad] (fp32 or bf16 per mode)
    const float* bias;              // [Cout] or null
    float* y; int Cout;
    int NF, F;                      // frames total (B*F), frames per sample
    int H, W;                       // input spatial size
    int kind;                       // 0: conv (kh, kw, stride, pad)   1: ConvTranspose 4x4 / stride 2 (4 phases)
    int kh, kw, stride, pad;
    // prologue on the input: 0 none, 1 GroupNorm-apply (+scale/shift) + SiLU
    int pro;
    const double* in_stats; const float* gamma; const float* beta; int groups;
    const float* ss; int ss_stride; // per-sample [scale(Cin) | shift(Cin)] rows, or null
    // epilogue: GroupNorm partial statistics of the output (or null)
    double* out_stats; int out_groups;
    int x0_bf16, y_bf16;            // x0 / y are stored as bf16 (the intra-ResnetBlock tensors in bf16 mode); y_bf16 excludes res
    int x1_bf16;                    // x1 stored as bf16 (bf16 activation storage)
    const float* res;               // optional residual added to the output: y = conv + bias + res  ([.., Cout] like y)
    int res_bf16;                   // res stored as bf16
    int wrows, wrow0;               // packed weight rows per tap / first row (0,0 = Cout rows from 0): slices a wider packing
    // completed by launch_conv
    int Ho, Wo, Hy, Wy, CinPad, PH, PW, NP, tiles_y, tiles_x;
    unsigned x0_bytes, x1_bytes, w_bytes;          // buffer-descriptor extents
    unsigned m_ihiw, m_iw, m_phpw, m_pw;           // floor(2^32 / d) + 1 for d = IH*IW, IW, PH*PW, PW (div_magic)
};

// out = SiLU(GroupNorm(y2; stats, gn_gamma, gn_beta)) + LayerNorm_C(r; ln_gamma, ln_beta), channel-last [B][pix][C]
struct TailArgs {
    const float* y2; const float* r; float* out;
    int y2_bf16;                    // y2 stored as bf16
    int r_bf16, out_bf16;           // r / out stored as bf16 (bf16 activation storage)
    const double* stats; const float* gn_gamma; const float* gn_beta; int groups;
    const float* ln_gamma; const float* ln_beta;
    int C; int batch; long pix_per_sample;
    int lpp;                        // completed by the launcher
    // fused 1x1 res_conv (bf16 tensors, bf16 mode): r = concat(x0[.., C0], x1[.., C1]) . rc_w + rc_b is computed on the MFMA inside
    // the tail instead of being read from `r` (resblock_tail_rc16_kernel; `r` is ignored when rc_w is set)
    const float* x0; const float* x1; int C0, C1;
    const void* rc_w;               // packed [C rows][C0 + C1] bf16 (conv_packed_bytes(MODE_BF16, 1, C0 + C1, C)), or null
    const float* rc_b;              // [C]
    // fused head (sampling forward, the network's last block): fin_out[pix][0] = out[pix][:] . fin_w[:][0] + fin_b[0] is written INSTEAD of
    // `out` (final_conv of unet3d.py:251 with one output channel; `out` may be null then)
    const float* fin_w; const float* fin_b; float* fin_out;
};
// shapes resblock_tail_rc16_kernel is instantiated for
bool tail_rc16_supported(int cin, int c0, int cout, long pix_per_sample);

struct TimeMlpArgs {
    const int* time; int t_is_device_scalar;     // time[b] (or time[0] for every sample)
    const float* w1; const float* b1; const float* w2; const float* b2;   // Flax [in][out]
    int dim, time_dim;
    const float* cond; const float* null_cond_emb; const unsigned char* cond_mask; int null_all; int cond_dim;
    float* temb; int temb_dim;      // temb_dim = time_dim + cond_dim
};

// one ResnetBlock time-MLP: offsets (in floats) into the flat parameter buffer / the scale-shift workspace
struct SsLayer { long w_off, b_off, g_off, be_off, out_off; int n; int pad_; };

hipError_t launch_resblock_tail(TailArgs a, hipStream_t st);
hipError_t launch_init_conv(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int F, int H, int W,
                            int Cout, int K, int y_bf16, hipStream_t st);
hipError_t launch_init_conv_mode(int mode, const float* x, const float* w, const float* bias, float* y, int B, int Cin, int F, int H, int W,
                                 int Cout, int K, int y_bf16, hipStream_t st);     // bf16 mode: MFMA im2col kernel when Cin == 1
hipError_t launch_final_conv(const float* x, const float* w, const float* bias, float* y, long npix, int D, int Cout, int x_bf16, hipStream_t st);
hipError_t launch_time_mlp(const TimeMlpArgs& a, int B, hipStream_t st);
hipError_t launch_resblock_ss(const float* params, const float* temb, const SsLayer* layers, int nlayers, float* ss_base,
                              float* lin_base, int temb_dim, int B, int max_n, hipStream_t st);   // max_n = widest layer (2 * cout)

// y = MHA(x) + x over sequences of L tokens; token address = (s / inner) * outer_stride + (s % inner) * inner_stride + tok * tok_stride
struct AttnArgs {
    const float* x; float* y;
    const void* wqkv; const float* bqkv;      // packed [3*heads*32][CPad]; bias [3][heads][32]
    const void* wo; const float* bo;          // packed [C][HDPad]; bias [C]
    int C, heads, L;
    long nseq, inner, inner_stride, outer_stride, tok_stride;
    float scale;
    int io_bf16;                              // x and y stored as bf16 (bf16 activation storage); strides stay in elements
    int fp8_core;                             // bf16 mode, <= 16 tokens: QK^T and PV on fp8 (e4m3) MFMA operands (vdx_set_attention_fp8)
    void* oscratch;                           // [rows][heads*32] bf16: per-head attention output of launch_attention_heads
    int CPad, HDPad;                          // completed by the launcher
    const float* pos_bias;                    // [heads][L][L] fp32 added to the scaled scores before the softmax (vdx_set_temporal_pos_bias), or null:
                                              // the generic kernels only (attention_reg_kernel / attention_kernel, BIAS instantiations)
    // focus-present mask (vdx_set_focus_present): sequence s belongs to sample s / inner, whose flag is focus[(s / inner) % focus_n]; a set
    // flag masks every score with key != query to -1e30 (after the bias, with the key mask): each token attends to itself only.  Device
    // bytes, or null.  The generic kernels only (FOCUS instantiations; pos_bias may be null there)
    const unsigned char* focus; int focus_n;
    int present;                              // every sample is focus-present: attention_block_forward runs launch_attention_present instead
};
hipError_t launch_attention(int mode, AttnArgs a, hipStream_t st);
// the block when every token attends to itself only: y = x + bo + Wo . rd(Wv . x + bv) in one launch (attention_present_kernel), rd = the
// operand rounding of the mode; reads the v rows of the packed wqkv only.  C % 4 == 0 (8 for bf16 tensors), C <= 1024
hipError_t launch_attention_present(int mode, AttnArgs a, hipStream_t st);
// table[h][i][j] = emb[buckets[i * n + j]][h]: the [heads][n][n] bias of the temporal attention blocks from the [32][heads] embedding
hipError_t launch_pos_bias_table(const float* emb, const int* buckets, float* table, int heads, int n, hipStream_t st);
// bf16 mode, <= 16 tokens, 8 heads: q/k/v projection + attention core per head (one workgroup per head: its weights resident in LDS,
// every wave streams its own sequences, no barriers) -> a.oscratch; the out-projection + residual is a 1x1 conv_igemm by the caller
hipError_t launch_attention_heads(AttnArgs a, hipStream_t st);
// sequences of more than 64 tokens (token-major rows): softmax(q k^T / sqrt(d)) v per (sequence, head) from a materialised
// qkv [rows][3 * heads * 32] fp32 into o [rows][heads * 32] fp32; the projections are 1x1 convs by the caller
hipError_t launch_attention_long_core(const float* qkv, float* o, long nseq, int L, int heads, float scale, hipStream_t st);

// the attention / SLA block as the network composes it (model.hip; route decided there and only there): require = ATTN_ANY, or the
// route a test-facing entry point is about (hipErrorInvalidValue when the network would take another)
enum { ATTN_ANY = -1, ATTN_HEADS = 1, ATTN_LONG = 2 };
hipError_t attention_block_forward(int mode, AttnArgs a, bool temporal, int NF, int Fr, int H, int W, void* scratch, size_t scratch_bytes,
                                   int require, hipStream_t st);

// y = SpatialLinearAttention(x) + x, x/y channel-last [NF][N][C]; 8 heads x 32
struct SlaArgs {
    const float* x; float* y;
    const void* wq; const void* wk; const void* wv;   // packed [256][CPad] each
    const void* wo;                                    // packed [C][256]
    void* workspace;                                   // sla_workspace_bytes()
    int C, heads, NF, N;
    int io_bf16;                                       // x and y stored as bf16 (bf16 activation storage)
    // completed by the launcher
    int CPad, nsub, nchunk; float* part; void* ctxT;
};
size_t sla_workspace_bytes(int mode, int NF, int N, int heads);
hipError_t launch_sla(int mode, SlaArgs a, hipStream_t st);
// bf16 mode, 8 heads, N % 16 == 0: per-head kernel (weights resident in LDS, one wave per frame) -> O [NF * N rows][heads * 32] bf16;
// to_out + residual is a 1x1 conv_igemm by the caller
hipError_t launch_sla_heads(SlaArgs a, void* O, hipStream_t st);

hipError_t sla_block_forward(int mode, SlaArgs a, int Fr, int H, int W, void* scratch, size_t scratch_bytes, int require, hipStream_t st);

// grid of the elementwise kernels of diffusion.hip / mixnoise.hip: one 256-thread workgroup per 256 work items, at most 2048 (the
// kernels stride over the rest)
inline int ew_blocks(long work_items) { return (int)std::max<long>(1, std::min<long>((work_items + 255) / 256, 2048)); }

struct PSampleArgs {
    const float* x; const float* eps; float* out;       // x/out [B,C,F,H,W] (may alias); eps channel-last [B,F,H,W,C]
    const int* t; const float* tables; int T;           // device t[B]; tables [5][T]
    const float* noise;                                 // explicit z [B,C,F,H,W], or null -> Philox(seed, offset + *dev_offset)
    unsigned long long seed, offset; const unsigned long long* dev_offset;
    const float* thres;                                 // per-sample dynamic threshold s[B] or null (s = 1)
    int clip; int C; long per_sample;
    float post_scale, post_shift;
};
hipError_t launch_randn(float* out, long n, unsigned long long seed, unsigned long long offset, const unsigned long long* dev_offset, hipStream_t st);
hipError_t launch_q_sample(const float* x0, const int* t, const float* noise, float* out, const float* sqrt_ac, const float* sqrt_1mac,
                           int B, long per_sample, float pre_scale, float pre_shift, hipStream_t st);
hipError_t launch_p_sample(const PSampleArgs& a, int B, hipStream_t st);
hipError_t launch_advance(int* t, int B, unsigned long long* dev_offset, hipStream_t st);
// Temporally correlated noise (vdx.h: "Mixed noise"; mixnoise.hip): z = a s + b e over [B,C,F,H,W], s shared by the F frames of a (b, c)
struct MixArgs { int F; long hw; float a, b; };         // frames, H * W, the two weights
hipError_t launch_randn_mixed(float* out, int B, int C, const MixArgs& m, unsigned long long seed, unsigned long long draw,
                              const unsigned long long* dev_draw, hipStream_t st);
// launch_p_sample with z generated in the kernel: P.noise is not read, the draw is P.offset + *P.dev_offset; per_sample % 4 == 0
hipError_t launch_p_sample_mixed(const PSampleArgs& a, const MixArgs& m, int B, hipStream_t st);
struct MaskArgs {                                        // the known region of a masked (inpainting) reverse step
    const float* known; const unsigned char* mask;       // k = 2 video - 1 and the element mask (1 = known), both [B,C,F,H,W]
    const float* mtab;                                   // [4][T] = sqrt_ac | sqrt_1mac | sqrt(alpha) | sqrt(beta)
    int U;                                               // resample steps per noise level
    unsigned long long step; const unsigned long long* step_dev;   // global step counter s = step + *step_dev
};
// P.noise / P.offset / P.dev_offset are not read: the draws are 1 + s, VDX_DRAW_KNOWN + s, VDX_DRAW_RENOISE + s
hipError_t launch_p_sample_masked(const PSampleArgs& a, const MaskArgs& m, int B, hipStream_t st);
hipError_t launch_resample_advance(int* t, int B, unsigned long long* step_dev, int U, hipStream_t st);
hipError_t launch_ddim_step_masked(const float* x, const float* eps, float* out, const float* ac, const int* seq, const unsigned long long* step_dev,
                                   const float* thres, int clip, int B, int C, long per_sample, const MaskArgs& m, int T, unsigned long long seed,
                                   hipStream_t st);
hipError_t launch_inpaint_init(float* x, const float* known, const unsigned char* mask, const float* mtab, int T, int t0, long n, hipStream_t st);
hipError_t launch_ddim_step(const float* x, const float* eps, float* out, const float* ac, const int* seq, const unsigned long long* step_dev,
                            const float* thres, int clip, int B, int C, long per_sample, hipStream_t st);
hipError_t launch_ddim_advance(int* t, int B, const int* seq, unsigned long long* step_dev, hipStream_t st);
// DPM-Solver++(2M) step; m != nullptr: the masked form (m->mtab rows of length T, draw VDX_DRAW_KNOWN + k of `seed`).  per_sample % 4 == 0
hipError_t launch_dpm_step(const float* x, const float* eps, float* out, float* hist, const float* ac, const int* seq,
                           const unsigned long long* step_dev, const float* thres, int clip, int order, int B, int C, long per_sample,
                           const MaskArgs* m, int T, unsigned long long seed, hipStream_t st);
hipError_t launch_dyn_thres(const float* x, const float* eps, const int* t, const float* tables, int T, float q, float* out, int B, int C,
                            long per_sample, hipStream_t st);
hipError_t launch_loss(const float* eps_hat, const float* noise, double* acc, int B, int Cc, long fhw, int l2, hipStream_t st);
hipError_t launch_affine(const float* x, float* y, long n, float a, float b, hipStream_t st);
// classifier-free guidance: out [B][per] = n + (c - n) s from eps2 [2B][per] (rows [0, B) = c, [B, 2B) = n; out may be eps2), times the
// per-sample rescale factor when rescale > 0 (scratch: cfg_scratch_doubles(B), whose tail holds the guided loops' 2B-byte cond_mask)
size_t cfg_scratch_doubles(int B);
unsigned char* cfg_scratch_mask(double* scratch, int B);
hipError_t launch_cfg_mask(double* scratch, int B, hipStream_t st);
hipError_t launch_cfg_combine(const float* eps2, float* out, float cond_scale, float rescale, double* scratch, int B, long per_sample,
                              hipStream_t st);
// Held-out evaluation (variational bound in bits/dim; vdx.h: "Held-out evaluation").  x [B,C,F,H,W] in [0, 1]; tab [VDX_VLB_ROWS][T]
// doubles; draw index = draw + *step_dev.  launch_vlb_noise writes xt (the double x_t rounded to fp32 once); launch_vlb_terms forms the same double again and leaves one
// (vb, mse, xstart_mse) triple per workgroup in partial [B][vlb_blocks()][3]; launch_vlb_prior leaves (prior, 0, 0) there;
// launch_vlb_advance adds the partials in index order into out[(k * B + b) * nout ..] (k = *step_dev, or 0) and, with seq, sets
// t[:] = max(seq[k + 1], 0) and k += 1 (nothing is written once k >= seq_len).
struct VlbArgs {
    const float* x; const float* eps; float* xt;        // eps channel-last [B,F,H,W,C] (terms); xt [B,C,F,H,W] (noise)
    const float* noise;                                 // explicit eps [B,C,F,H,W], or null -> Philox(seed, draw + *step_dev)
    const int* t; const double* tab; int T;
    unsigned long long seed, draw; const unsigned long long* step_dev;
    int clip; int C; long per_sample;
    double* partial;
};
int vlb_blocks();
hipError_t launch_vlb_noise(const VlbArgs& a, int B, hipStream_t st);
hipError_t launch_vlb_terms(const VlbArgs& a, int B, hipStream_t st);
hipError_t launch_vlb_prior(const float* x, const double* tab, int T, double* partial, int B, long per_sample, hipStream_t st);
hipError_t launch_vlb_advance(const double* partial, double* out, int nout, int B, long per_sample, int* t, const int* seq, int seq_len,
                              unsigned long long* step_dev, hipStream_t st);
// Learned reverse-process variances (vdx.h: "Learned variances").  out2 = the network's channel-last output [B,F,H,W,2C], eps_hat | v.
struct LvStepArgs {
    const float* x; const float* out2; float* out;      // x/out [B,C,F,H,W] (may alias)
    const float* tables; int S;                         // [6][S] of the (respaced) chain, level-indexed
    const int* idx;                                     // device level per sample [B], or null -> S - 1 - (step + *step_dev)
    unsigned long long step; const unsigned long long* step_dev;
    const float* noise;                                 // explicit z [B,C,F,H,W], or null -> Philox(seed, offset + *dev_offset)
    unsigned long long seed, offset; const unsigned long long* dev_offset;
    int clip; int C; long per_sample;
    float post_scale, post_shift;                       // applied on level 0 only
};
hipError_t launch_p_sample_lv(const LvStepArgs& a, int B, hipStream_t st);
struct HybridArgs {
    const float* x; const float* noise; const float* out2; float* d_out;   // d_out [B,F,H,W,2C] or null (no gradient)
    const int* t; const double* tab; int T;             // tab [VDX_LV_ROWS][T] doubles
    int l2; int C; long per_sample;
    float pre_scale, pre_shift;                         // x0 = x pre_scale + pre_shift (normalize_img)
    float inv_count; double vscale;                     // 1 / N as launch_loss_grad forms it; w / (N ln 2)
    double* partial;                                    // hybrid_scratch_doubles(B)
    const double* iw; double inv_count64;               // importance weights [B] or null (vdx_hybrid_loss_w); 1 / N in double
};
size_t hybrid_scratch_doubles(int B);
// out [2 B + 3] doubles: per-sample means (mse, vb), then the batch's (mse, vb, mse + w vb)
hipError_t launch_hybrid_loss(const HybridArgs& a, double* out, double w, int B, hipStream_t st);
// launch_vlb_terms with the model's variance: a.eps = out2, a.tab = the [VDX_LV_ROWS][T] table
hipError_t launch_vlb_terms_lv(const VlbArgs& a, int B, hipStream_t st);
// Cascaded super-resolution (vdx.h: "Cascaded super-resolution"; lowres.hip).  xin [B,2C,F,S,S] = [ x_t | aug(up(2 lo - 1)) ].
struct LowresArgs {
    const float* x0; const int* t; const float* noise;  // x0 [B,C,F,S,S] (null: the second half alone; t / noise are not read then)
    const float* lo; const int* aug;                    // lo [B,C,F/ft,S/fs,S/fs]; device levels [B] (< 0 = none) or null (none)
    float* xin;
    const float* sqrt_ac; const float* sqrt_1mac; int T;
    unsigned long long seed, draw;                      // the augmentation noise: Philox(seed, draw) over the index of [B,C,F,S,S]
    float pre_scale, pre_shift;                         // x0 pre_scale + pre_shift (normalize_img), as launch_q_sample
    int C, F, S, ft, fs;
};
hipError_t launch_lowres_down(const float* x, float* lo, int B, int C, int F, int S, int ft, int fs, hipStream_t st);
hipError_t launch_lowres_input(const LowresArgs& a, int B, hipStream_t st);
hipError_t launch_lowres_pack(const float* img, float* xin, int B, long per_sample, hipStream_t st);
// frame-conditioned training (mask [B,C,F,H,W] bytes, nonzero = clean context): masked q_sample, the deterministic (sum, count) of the
// loss over the mask-0 elements (scratch: loss_masked_scratch_doubles()), and its gradient with the count read from the device
hipError_t launch_q_sample_masked(const float* x0, const int* t, const float* noise, const unsigned char* mask, float* out, const float* sqrt_ac,
                                  const float* sqrt_1mac, int B, long per_sample, float pre_scale, float pre_shift, hipStream_t st);
size_t loss_masked_scratch_doubles();
hipError_t launch_loss_masked(const float* eps_hat, const float* noise, const unsigned char* mask, double* scratch, double* out, int B, int Cc,
                              long fhw, int l2, hipStream_t st);
hipError_t launch_loss_grad_masked(const float* eps_hat, const float* noise, const unsigned char* mask, const double* count_dev, float* d_eps,
                                   int B, int Cc, long fhw, int l2, hipStream_t st);

hipError_t launch_loss_grad(const float* eps_hat, const float* noise, float* d_eps, int B, int Cc, long fhw, int l2, hipStream_t st);
// Loss-aware timestep sampling (vdx.h: "Loss-aware timestep sampling"; tsampler.hip).  hist double [T][H], count int [T]; one workgroup each.
size_t tsampler_draw_lds_bytes(int T);
hipError_t launch_tsampler_draw(const double* hist, const int* count, int T, int H, double eps, const int* t_given, unsigned long long seed,
                                unsigned long long draw, int* t_out, double* iw_out, double* p_out, int batch, hipStream_t st);
hipError_t launch_tsampler_update(double* hist, int* count, int T, int H, const double* entries, int n, hipStream_t st);
size_t loss_weighted_scratch_doubles(int B);
// out [B + 1] doubles: the per-sample means, then (1 / B) sum_b iw_b l_b; d_eps (may be null) channel-last like eps_hat
hipError_t launch_loss_weighted(const float* eps_hat, const float* noise, const double* iw, float* d_eps, double* scratch, double* out, int B,
                                int Cc, long fhw, int l2, hipStream_t st);
// v-prediction (vdx.h: "v-prediction"; vpred.hip).  launch_v_to_eps: out [rows][F,H,W,C] (the network's v_hat) <- eps_hat in place, x
// [rows][C,F,H,W] = x_t.  launch_v_loss: result [B + 1] doubles, the per-sample weighted means, then (1 / B) sum_b iw_b result[b].
hipError_t launch_v_to_eps(float* out, const float* x, const int* t, const float* sqrt_ac, const float* sqrt_1mac, int T, int rows, int Cc,
                           long per_sample, hipStream_t st);
struct VLossArgs {
    const float* out; const float* x0; const float* noise; float* d_out;   // out / d_out channel-last [B,F,H,W,C]; d_out or null (no gradient)
    const int* t; const float* sqrt_ac; const float* sqrt_1mac; int T;     // t may be null with kind 0 and no wtab
    const double* wtab; const double* iw;                                  // per-level weights [T] / importance weights [B], or null (all 1)
    int kind, l2, C; long fhw;                                             // kind 1: target v; kind 0: target noise
    float pre_scale, pre_shift;                                            // x0n = x0 pre_scale + pre_shift (normalize_img), as launch_q_sample
    // completed by the launcher
    float inv_count; int vec; double* partial;
};
size_t v_loss_scratch_doubles(int B);
hipError_t launch_v_loss(VLossArgs a, double* scratch, double* result, int B, hipStream_t st);
// Self-conditioning (vdx.h: "Self-conditioning"; selfcond.hip): x0~ of (x, eps_hat) at levels t into planes [C, 2C) of xin [B,2C,F,H,W]
struct SelfcondArgs {
    const float* x; long x_pitch;                       // x_t [B][C,F,H,W], sample b at x + b * x_pitch (floats; >= per_sample)
    const float* eps; const int* t;                     // eps_hat channel-last [B,F,H,W,C]; levels [B], clamped to [0, T - 1]
    const float* tables; int T;                         // rows 0, 1 of the [5][T] step tables: sqrt(1 / ac) | sqrt(1 / ac - 1)
    const float* thres; int clip;                       // the dynamic threshold s [B] or null (s = 1); clip: min(max(x0, -s), s) / s
    float* xin; int C; long per_sample;                 // per_sample = C * F * H * W
};
hipError_t launch_selfcond_x0(const SelfcondArgs& a, int B, hipStream_t st);
hipError_t launch_adam_ema(float* p, const float* g, float* m, float* v, float* ema, long n, float lr, float b1, float b2, float eps,
                           long step_count, float grad_scale, int do_ema, float decay, hipStream_t st);
hipError_t launch_adam_ema_clip(float* p, const float* g, float* m, float* v, float* ema, long n, float lr, float b1, float b2, float eps,
                                long step_count, float grad_scale, int do_ema, float decay, const double* sqnorm, float max_grad_norm,
                                float* norm_out, hipStream_t st);
hipError_t launch_grad_accumulate(float* acc, const float* g, long n, hipStream_t st);
size_t grad_sqnorm_scratch_doubles();
hipError_t launch_grad_sqnorm(const float* g, long n, double* scratch, double* out, hipStream_t st);

// Weight gradient of a conv (kind 0: (kh,kw)/stride SAME; kind 1: ConvTranspose 4x4/2): dW += Xhat^T (*) dY
struct WgradArgs {
    const float* x0; const float* x1; int C0, C1;          // conv input (channel-last), optional concat
    const float* dy; int Cout;                             // output gradient [NF, Hy, Wy, Cout]
    float* dW;                                             // Flax layout [taps][Cin][Cout], accumulated with atomics
    float* db;                                             // optional: db[co] += sum_pixels dY (bias gradient), or null
    int NF, F, H, W;                                       // input geometry
    int kind, kh, kw, stride;
    int pro; const double* in_stats; const float* gamma; const float* beta; int groups; const float* ss; int ss_stride;
    int x0_bf16;                                           // x0 (and x1) stored as bf16
    int dy_bf16;                                           // dy stored as bf16 (backward intermediates of bf16 mode)
    int split; float* dW1; float* dW2; float* db1; float* db2;   // split > 0: dY column block co / split goes to (dW, dW1, dW2)[co / split], each [taps][Cin][split]
    int bf16_mma;                                          // bf16 MFMA operands (bf16 mode) instead of exact f32
    // deterministic accumulation (round 3): when `part` is set and large enough, every workgroup STORES its partial tile into its own slot
    // part[slot][taps][Cin][Cout] (bias sums: behind them, [slot][Cout]) and a finalize pass adds the slots in a fixed order -- no atomics,
    // so two runs give bit-identical gradients.  Without scratch (the block-level entry points) the kernels add with float atomics.
    float* part; size_t part_cap;                          // scratch and its capacity in floats, or null / 0
    float* part_b; long part_E;                            // completed by the launcher: bias slots, floats per dW slot
    // completed by the launcher
    int taps, sa, sb, ext, halo, Hm, Wm, Hy, Wy, PH, PW, co_tiles;
    unsigned m_iw, m_bw;                                   // magic multipliers (div_magic) of the staged window widths
    int pwl;                                               // log2(PW) (bf16 form)
};
hipError_t launch_conv_wgrad(WgradArgs a, hipStream_t st);
struct PackJob;
hipError_t launch_pack_jobs(int mode, const float* params, void* dst_base, const PackJob* d_jobs, int njobs, hipStream_t st);
hipError_t launch_colsum(const float* x, float* out, long rows, int C, hipStream_t st, float* part = nullptr, size_t part_cap = 0);
// dst[e] (+= the split targets: column block co / split of a [rows][Cout] layout goes to d0 / d1 / d2) += sum over slots k < nslots, in
// order, of part[k * slot_stride + e], e < E: the second half of every deterministic accumulation of the backward
hipError_t launch_slot_sum(const float* part, int nslots, size_t slot_stride, long E, int Cout, int split, float* d0, float* d1, float* d2, hipStream_t st);
// what follows a launch that stored `nslots` slots of E weight-gradient floats and, behind them, `nslots` rows of Cout bias sums: dW
// (+ its split targets) += the slots, then db += the rows (db[0] null: no bias gradient)
hipError_t launch_slot_sum_dw_db(const float* part, int nslots, long E, int Cout, int split, float* const (&dW)[3], float* const (&db)[3], hipStream_t st);
// the slot scratch of a deterministic accumulation if the launch's slots fit it, else null: the kernel then adds with float atomics and
// two runs no longer give the same bits (the label of every such launch says which: `det 1|0`)
inline float* slots_if_fit(float* part, size_t need, size_t cap) { return part && need <= cap ? part : nullptr; }
constexpr size_t WG_PART_FLOATS = (size_t)12 << 20;        // scratch per stream for the slots (48 MB; a launch that needs more falls back to atomics)
hipError_t launch_add_inplace(float* y, const float* x, long n, hipStream_t st);

// Backward of  act = SiLU((gamma*GN(y)+beta)*(1+s)+sh)  [+ LayerNorm_C(r) branch of the block tail]; channel-last [B][pix][C]
struct NormBwdArgs {
    const float* dact; const float* y; float* dy;                 // dL/dact (or dL/dout), saved pre-norm tensor, result dL/dy
    int y_bf16;                                                   // y stored as bf16
    int dy_bf16;                                                  // dy written as bf16 (its consumers, the conv data / weight gradients, round it to bf16 anyway)
    int r_bf16;                                                   // r stored as bf16 (bf16 activation storage of the training forward)
    const double* stats; const float* gamma; const float* beta; int groups;
    const float* ss; int ss_stride;                               // forward scale/shift rows or null
    float* d_gamma; float* d_beta;                                // accumulated (atomics)
    float* dss;                                                   // [B][2C] (ds | dsh) written, or null
    const float* r; const float* ln_gamma; float* dr; float* d_ln_gamma; float* d_ln_beta;   // LN branch (tail) or nulls
    float* R; float* G;                                           // scratch: per-workgroup partial sums [B][nwg][4][C] (written, never accumulated), [B][groups][2]
    int nwg;                                                      // workgroups per sample of the reduce pass (completed by the launcher)
    float* dgp;                                                   // deterministic mode: scratch [batch][4][C] for the per-sample parameter-gradient rows (or null: float atomics)
    int C, batch; long pix_per_sample;
    int lpp;
};
hipError_t launch_norm_bwd(NormBwdArgs a, hipStream_t st);
size_t norm_bwd_scratch_floats(int C, int batch, long pix_per_sample);     // floats behind NormBwdArgs::R + G (G = R + that - 64 * batch)

// attention core backward: qkv [npix][3*heads*32] (biased, q unscaled), dO [npix][heads*32] -> O, dq, dk, dv [npix][heads*32]
struct AttnBwdArgs {
    const float* qkv; const float* dO; float* O; float* dq; float* dk; float* dv;
    int heads, L; long nseq, inner, outer_p, tok_p; float scale;
    int dstride;                                                     // row stride (elements) of dq / dk / dv: heads*32, or 3*heads*32 for one [rows][dq|dk|dv] buffer
    int io_bf16;                                                     // qkv, dO, O, dq, dk, dv are bf16 tensors (bf16 MFMA form only)
    int bf16_mma;                                                    // bf16 MFMA form (bf16 mode, L <= 16) instead of the exact fp32 VALU form
    // pre-softmax bias (vdx_set_temporal_pos_bias): logits = scale q.k + bias[h][i][j].  The bias forms run on a fixed grid, every workgroup
    // STORES the sum of dS over its sequences into its own slot of `part`, and a second pass adds the slots in order into dbias (+=)
    const float* bias; float* dbias;                                 // [heads][L][L] each, or null / null
    float* part; size_t part_cap;                                    // scratch for the slots and its capacity in floats (attn_bwd_bias_scratch_floats)
    // focus-present mask as in AttnArgs (sample of sequence s = s / inner, flag focus[sample % focus_n]): the recomputed P of a flagged
    // sample is one-hot, so its dS, dq, dk and its share of dBias are exactly 0 and dv = dO.  The focus forms run on the fixed grid of the
    // bias forms; bias / dbias / part may all be null there (focus without the position bias)
    const unsigned char* focus; int focus_n;
};
size_t attn_bwd_bias_scratch_floats(int heads, int L);
hipError_t launch_attn_core_bwd(const AttnBwdArgs& a, hipStream_t st);
// more than 64 tokens (attn_long_bwd.hip): served for L a multiple of 64 up to 640 (attn_bwd_long_served), fp32 tensors, no bias, no focus;
// three launches (stats -> dkv -> dq) whose per-row softmax scalars travel in the rows' own dq columns, so there is no scratch.
// launch_attn_core_bwd routes every L > 64 here; anything unserved is hipErrorInvalidValue with nothing launched
bool attn_bwd_long_served(int L);
hipError_t launch_attn_core_bwd_long(const AttnBwdArgs& a, hipStream_t st);
// demb[b][h] = sum over (i, j) with buckets[i * n + j] == b, in (i, j) order, of dbias[h][i][j]   (one thread per (b, h): no atomics)
hipError_t launch_pos_bias_scatter(const float* dbias, const int* buckets, float* demb, int heads, int n, hipStream_t st);
// fused attention backward of the widest level (bf16 mode, C == 64, 8 heads x 32, <= 16 tokens): q/k/v recompute, dO = g Wo^T, the
// core and dx = g + dq|dk|dv . Wqkv^T in one kernel; O and dq|dk|dv are written (bf16) for the weight-gradient kernels
struct AttnBwdXArgs {
    const float* x; const float* g;            // block input, dL/d(block output): fp32 [rows][64]
    int x_bf16;                                // x stored as bf16 (bf16 activation storage of the training forward)
    const void* wqkv; const float* bqkv;       // forward packing [3 * 256][64] bf16, biases [3 * 256]
    const void* woT;                           // transposed packing of the out-projection [256][64] bf16
    void* O; void* dqkv;                       // bf16 [rows][256], [rows][768]
    float* dx;                                 // fp32 [rows][64]
    int L; long nseq, inner, outer_p, tok_p; float scale;
};
hipError_t launch_attn_bwd_fused(const AttnBwdXArgs& a, hipStream_t st);
// SLA core backward: q,k,v,dOut [NF*N][256] -> O (forward, pre to_out), dq, dk, dv ; A = scratch (sla_bwd_scratch_floats)
struct SlaBwdArgs {
    const float* q; const float* k; const float* v; const float* dOut; float* O; float* dq; float* dk; float* dv; float* A;
    int NF, N, heads;
    int dstride;                                  // row stride (elements) of dq / dk / dv: 256, or 768 for one interleaved buffer
    int io_bf16;                                  // q, k, v, dOut, O, dq, dk, dv are bf16 tensors (bf16 MFMA forms only)
    int bf16_mma;                                 // pass A on bf16 MFMA (bf16 mode) instead of the exact fp32 VALU form
};
size_t sla_bwd_scratch_floats(int NF, int heads);
hipError_t launch_sla_bwd(const SlaBwdArgs& a, hipStream_t st);

// ---- geometry and layout of the attention blocks over a channel-last [batch][frames][h][w][C] tensor, defined once for the network
// (model.hip, model_bwd.hip) and for the block-level entry points that stand for it in the tests (vdx_api.cpp).  temporal: sequences
// over the frames of one pixel, else over the pixels of one frame
inline void attn_token_geometry(AttnArgs& a, long batch, long frames, long h, long w, long C, bool temporal) {
    const long hw = h * w;
    if (temporal) { a.L = (int)frames; a.nseq = batch * hw; a.inner = hw; a.inner_stride = C; a.outer_stride = frames * hw * C; a.tok_stride = hw * C; }
    else { a.L = (int)hw; a.nseq = batch * frames; a.inner = 1; a.inner_stride = 0; a.outer_stride = hw * C; a.tok_stride = C; }
}
// the same in pixels (rows of the backward's token-major tensors): AttnBwdArgs and AttnBwdXArgs
template <class Args>
inline void attn_pixel_geometry(Args& a, long batch, long frames, long h, long w, bool temporal) {
    const long hw = h * w;
    if (temporal) { a.L = (int)frames; a.nseq = batch * hw; a.inner = hw; a.outer_p = frames * hw; a.tok_p = hw; }
    else { a.L = (int)hw; a.nseq = batch * frames; a.inner = 1; a.outer_p = hw; a.tok_p = 1; }
}
// dk and dv of one interleaved [rows][dq | dk | dv] buffer of hd = heads * 32 columns each, by the element size of its tensors
inline void split_dqkv(float* dq, int hd, int io_bf16, float*& dk, float*& dv) {
    const size_t es = io_bf16 ? 2 : 4;
    dk = reinterpret_cast<float*>(reinterpret_cast<char*>(dq) + (size_t)hd * es);
    dv = reinterpret_cast<float*>(reinterpret_cast<char*>(dq) + (size_t)2 * hd * es);
}

hipError_t launch_final_conv_bwd(const float* x, const float* dout, const float* w, float* dx, float* dW, float* db, long npix, int D, int Cout, int x_bf16, hipStream_t st, float* part = nullptr, size_t part_cap = 0);
hipError_t launch_init_conv_wgrad(const float* x, const float* dy, float* dW, float* db, int B, int Cin, int F, int H, int W, int Cout, int K, hipStream_t st, float* part = nullptr, size_t part_cap = 0);
hipError_t launch_resblock_ss_bwd(const float* params, float* grads, const float* temb, const SsLayer* layers, int nlayers, const float* lin_base,
                                  float* dss_base, float* dtemb, int temb_dim, int B, hipStream_t st, float* part = nullptr, size_t part_cap = 0);
hipError_t launch_time_mlp_bwd(const TimeMlpArgs& a, const float* dtemb, float* dw1, float* db1, float* dw2, float* db2, float* dnull, int B, hipStream_t st);

size_t conv_packed_bytes(int mode, int taps, int Cin, int Cout);
int conv_cin_pad(int mode, int Cin);
hipError_t launch_pack_weights(int mode, const float* src, void* dst, int taps, int Cin, int Cout, hipStream_t st);
hipError_t launch_conv(int mode, ConvArgs a, hipStream_t st);
// ---- routing of launch_conv: geometry completion, conv_route(), launch.  A kernel form is ONE ConvRoute record.  `plan` is its only gate;
// it makes no runtime call and hands what it computed on the way (tile geometry, channel tiles, tile count) to `launch`, which picks the
// template instantiation, composes the hook's label from the values it instantiates with, and launches through LaunchScope::launch.
struct ConvPlan {
    int geo, nct, total;                                               // tile geometry (conv1x1_pw: weight rows), output-channel tiles, tiles of the launch
    int BC, TN, inf, PH, PW, NP; size_t lds;                           // conv_igemm_kernel: channel tile, wave tile, input format, pixel patch, LDS bytes
};
struct ConvWork { double flops, bytes; char shape[128]; };             // what the hook is told about the call (conv_igemm.hip: conv_work)
struct ConvRoute {
    bool (*plan)(int mode, const ConvArgs& a, ConvPlan& p);            // `a` geometry-completed by launch_conv
    hipError_t (*launch)(int mode, const ConvArgs& a, const ConvPlan& p, const ConvWork& w, hipStream_t st);
};
// the records whose kernels live outside conv_igemm.hip (conv_ws.hip, conv_rs.hip, conv_pw.hip); the list itself is conv_igemm.hip's conv_routes
#define VDX_CONV_ROUTE_DECL(NAME_)                                                                                  \
    bool NAME_##_plan(int mode, const ConvArgs& a, ConvPlan& p);                                                    \
    hipError_t NAME_##_launch(int mode, const ConvArgs& a, const ConvPlan& p, const ConvWork& w, hipStream_t st)
VDX_CONV_ROUTE_DECL(conv3x3_ws);
VDX_CONV_ROUTE_DECL(conv4x4_ws);
VDX_CONV_ROUTE_DECL(resample32);
VDX_CONV_ROUTE_DECL(conv1x1_pw);
#undef VDX_CONV_ROUTE_DECL
// a run-time flag / size as a template argument: f(std::true_type{}) or f(std::false_type{}); Int<V>{} for the sizes
template <int V> using Int = std::integral_constant<int, V>;
template <typename F> inline auto with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
// f(Int<T>{}) with T = 1, 2, 4, 8, 16: the 64-channel tiles that cover C <= 1024 channels, the output tiling of the attention and SLA kernels
template <typename F> inline hipError_t with_channel_tiles(int C, F&& f) {
    if (C <= 64) return f(Int<1>{});
    if (C <= 128) return f(Int<2>{});
    if (C <= 256) return f(Int<4>{});
    if (C <= 512) return f(Int<8>{});
    if (C <= 1024) return f(Int<16>{});
    return hipErrorInvalidValue;
}
// y <- SiLU(GroupNorm(y) * (scale + 1) + shift) in place on a bf16 tensor [batch][pix][C] (the Block prologue as its own pass; elementwise.hip)
hipError_t launch_gn_silu_apply16(float* y_bf16, const double* stats, const float* gamma, const float* beta, const float* ss, int ss_stride, int groups,
                                  int C, int batch, long pix_per_sample, hipStream_t st);
hipError_t launch_pack_weights_t(int mode, const float* src, void* dst, int taps, int Cin, int Cout, hipStream_t st);

}  // namespace vdx
