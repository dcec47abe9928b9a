/* vdx.h -- C ABI of the MI355X-native video-diffusion hot path (libvdx.so).
 *
 * The reference (maxsonate/video-diffusion-nnx) has NO FFI: its device boundary is the XLA runtime
 * under jax/flax.  This header is therefore the boundary the new path defines underneath the
 * reference's Python surface (Unet3D / GaussianDiffusion / Trainer); each entry cites the reference
 * function whose device work it replaces.  The reference-side binding is the ctypes layer in
 * video_diffusion_nnx_amd/_lib.py.
 *
 * Conventions
 *   - every function returns int: 0 = VDX_OK, negative = vdx_status; vdx_last_error() gives the text
 *     (thread-local);
 *   - ALL tensor memory is caller-owned device memory (the PyTorch allocator in the Python host);
 *     the library owns only the handle and never frees or allocates caller tensors;
 *   - pointers are device pointers on the current HIP device, contiguous, 16-byte aligned, fp32 unless
 *     stated; layouts are documented per call;
 *   - no hidden synchronisation: work is enqueued on the caller's stream (a hipStream_t passed as
 *     void*), the calls are graph-capturable (no malloc/free/sync inside);
 *   - a handle is not thread-safe: one host thread per rank / GPU.
 *
 * Tensor layouts: external video tensors are [B, C, F, H, W] (as the reference's public API);
 * internal activations are channel-last [B, F, H, W, C] (as the reference after unet3d.py:280).
 */
#ifndef VDX_H_
#define VDX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    VDX_OK = 0,
    VDX_ERR_INVALID = -1,     /* bad argument / unsupported shape */
    VDX_ERR_HIP = -2,         /* a HIP runtime call failed */
    VDX_ERR_NOMEM = -3,       /* workspace too small */
    VDX_ERR_STATE = -4        /* call sequence error (e.g. backward without forward) */
} vdx_status;

/* Arithmetic of the MFMA contractions (activations and master weights are fp32 in HBM either way):
 *   VDX_MODE_F32  exact fp32 products (v_mfma_f32_16x16x4_f32)  -- the parity mode
 *   VDX_MODE_BF16 operands rounded to bf16 at LDS staging, fp32 accumulate (v_mfma_f32_16x16x32_bf16)
 *   VDX_MODE_F16  operands rounded to IEEE fp16 at LDS staging, fp32 accumulate (v_mfma_f32_16x16x32_f16): the "fp16" of
 *                 BASELINE.json configs[3]; generic kernels only (every tensor stays fp32 in HBM, no bf16 activation storage) */
typedef enum { VDX_MODE_F32 = 0, VDX_MODE_BF16 = 1, VDX_MODE_F16 = 2 } vdx_mode;

const char* vdx_last_error(void);
int vdx_version(void);

/* ------------------------------------------------------------------------------------------------
 * Operator-level entry points (used by the per-block parity tests; the network entry points below
 * are built from the same launchers).
 * ---------------------------------------------------------------------------------------------- */

/* Packs a Flax kernel [taps][Cin][Cout] (fp32) into the MFMA staging layout [taps][Cout][CinPad]
 * (fp32 or bf16 per mode, zero padded).  vdx_packed_conv_bytes gives the destination size. */
size_t vdx_packed_conv_bytes(int mode, int taps, int cin, int cout);
int vdx_pack_conv_weights(int mode, const float* kernel, void* packed, int taps, int cin, int cout, void* stream);

/* Size in bytes of one GroupNorm statistics slab for `batch` samples and `groups` groups. */
size_t vdx_gn_stats_bytes(int batch, int groups);

typedef struct {
    /* input = concat(x0 [B*F,H,W,c0], x1 [B*F,H,W,c1]) on channels (x1 may be NULL with c1 = 0) */
    const float* x0; const float* x1; int c0, c1;
    const void* packed_w;           /* from vdx_pack_conv_weights */
    const float* bias;              /* [cout] or NULL */
    float* y;                       /* [B*F, Ho, Wo, cout] */
    int cout;
    int batch, frames, h, w;
    int kind;                       /* 0: Conv(1,kh,kw) SAME, stride (1,s,s); 1: ConvTranspose(1,4,4)/(1,2,2) SAME */
    int kh, kw, stride;
    /* optional prologue on x0 (c1 must be 0): SiLU(GroupNorm(x0; in_stats, gamma, beta) * (scale+1) + shift) */
    const double* in_stats; const float* gamma; const float* beta; int groups;
    const float* scale_shift; int scale_shift_stride;   /* rows [scale(c0) | shift(c0)] per sample, or NULL */
    /* optional epilogue: accumulate GroupNorm partial statistics of y into out_stats (pre-zeroed) */
    double* out_stats; int out_groups;
    /* storage of the activation tensors (VDX_MODE_BF16 only): nonzero = the tensor holds bf16 elements instead of fp32 */
    int x_bf16;                     /* x0 and x1 */
    int y_bf16;
    /* optional residual added to the output, y = conv + bias + res ([.., cout] like y; the attention / SLA `to_out` projections of
     * the wide levels run as 1x1 convs with the block input as res: modules.py:312-326, unet3d.py:86-96 Residual) */
    const void* res; int res_bf16;
} vdx_conv_desc;

/* nnx.Conv / nnx.ConvTranspose on channel-last video (reference: modules.py:162-179 Block.proj + norm
 * + scale/shift + SiLU; utils.py:103-125 Up/Downsample; modules.py:219-222 res_conv). */
int vdx_conv_forward(int mode, const vdx_conv_desc* d, void* stream);

/* Instrumentation (bench.py's roofline leg): a process-global hook the library calls immediately before (phase 0) and after
 * (phase 1) EVERY kernel launch of the forward / sampling path -- inside vdx_unet_forward / vdx_p_sample_loop too -- so that a caller
 * can bracket each launch with its own events on `stream` while the real step runs.  `kernel` = the __global__ function's name
 * without template arguments (a substring of the name rocprofv3 prints); `shape` = its template arguments + the operand shape as
 * text (the key bench.py groups launches by: one symbol serves several levels of the network); flops / bytes = the ALGORITHMIC work
 * of this launch (SURVEY 8d op-level definition: 2*M*N*K per contraction; input + output tensors in their storage type + weights).
 * The strings are only valid during the call.  NULL disables.  Not for use while a stream is being captured into a graph (run the
 * loop with use_graph = 0). */
typedef struct {
    const char* kernel;
    const char* shape;
    double flops, bytes;
} vdx_launch_info;
typedef void (*vdx_launch_hook)(void* user, int phase, const vdx_launch_info* info, void* stream);
void vdx_set_launch_hook(vdx_launch_hook hook, void* user);

/* ResnetBlock tail: out = SiLU(GroupNorm(y2; stats, gn_gamma, gn_beta)) + LayerNorm_C(r; ln_gamma, ln_beta)
 * (reference: modules.py:173-179 for Block 2 and :240-243 `h + norm_2(res_conv(x))`).  r is res_conv(x), or x itself
 * when the block has no res_conv.  All tensors channel-last [batch, pix_per_sample, c]. */
int vdx_resblock_tail(const float* y2, const float* r, float* out, const double* stats, const float* gn_gamma,
                      const float* gn_beta, int groups, const float* ln_gamma, const float* ln_beta, int c, int batch,
                      long pix_per_sample, void* stream);

/* ResnetBlock tail with the block's 1x1 res_conv inside (reference: modules.py:219-222 `res_conv` + :240-243
 * `h + norm_2(res_conv(x))`), bf16 tensors (bf16 activation storage of a bf16-mode network):
 * out = SiLU(GroupNorm(y2)) + LayerNorm_C(concat(x0[..,c0], x1[..,c1]) . W + rc_bias).  y2, x0, x1, out: bf16 channel-last;
 * rc_w_packed: bf16 [c][c0 + c1] (row = output channel, K-contiguous: the packing vdx_pack_params produces for this conv);
 * x1 may be NULL with c1 = 0.  Shapes served: (c0 + c1, c) in {(128,64), (64,128), (256,64), (128,256)}, c1 = 0 or c1 = c0,
 * pix_per_sample a multiple of 16; anything else returns VDX_ERR_INVALID. */
int vdx_resblock_tail_rc_bf16(const void* y2, const void* x0, const void* x1, int c0, int c1, const void* rc_w_packed,
                              const float* rc_bias, void* out, const double* stats, const float* gn_gamma, const float* gn_beta,
                              int groups, const float* ln_gamma, const float* ln_beta, int c, int batch, long pix_per_sample,
                              void* stream);

/* Block prologue as its own pass, in place on a bf16 tensor (reference: modules.py:171-179, Block.__call__: GroupNorm, the
 * time-embedding `x * (scale + 1) + shift`, SiLU): y <- SiLU(GroupNorm(y) * (scale + 1) + shift).  y bf16 channel-last
 * [batch, pix_per_sample, c]; stats as the producing conv's epilogue leaves them (vdx_resblock_tail); scale_shift NULL (Block 2) or
 * fp32 [batch][ss_stride] rows holding scale[c] | shift[c].  c a multiple of 8, c <= 1024.  The sampling forward runs it in front of
 * the wide (c >= 256) second convs of bf16-storage networks. */
int vdx_gn_silu_apply_bf16(void* y, const double* stats, const float* gn_gamma, const float* gn_beta, const float* scale_shift,
                           int ss_stride, int groups, int c, int batch, long pix_per_sample, void* stream);

/* init_conv (reference: unet3d.py:110-115,282): x EXTERNAL layout [B,Cin,F,H,W], Flax kernel (1,k,k,Cin,Cout) fp32,
 * y channel-last [B,F,H,W,Cout]. */
int vdx_init_conv(const float* x, const float* kernel, const float* bias, float* y, int batch, int cin, int frames,
                  int h, int w, int cout, int k, void* stream);

/* final 1x1 conv (reference: unet3d.py:251): x [npix, d] channel-last, Flax kernel (1, d, cout), y [npix, cout]. */
int vdx_final_conv(const float* x, const float* kernel, const float* bias, float* y, long npix, int d, int cout, void* stream);

/* time_mlp (reference: modules.py:30-45 SinusoidalPosEmb; unet3d.py:128-133,288 Linear-GELU-Linear; :291-298 cond mix).
 * temb [batch, time_dim + cond_dim].  cond/null_cond_emb/cond_mask may be NULL when cond_dim == 0;
 * cond_mask (bytes, 1 = use null_cond_emb) overrides null_all. */
int vdx_time_mlp(const int* time, const float* w1, const float* b1, const float* w2, const float* b2, int dim,
                 const float* cond, const float* null_cond_emb, const unsigned char* cond_mask, int null_all, int cond_dim,
                 float* temb, int batch, void* stream);

/* Multi-head self-attention + residual (reference: modules.py:247-326 inside Residual(PreNorm(EinopsToAndFrom(..)))
 * where PreNorm is a no-op, unet3d.py:86-96 temporal / :196-208 bottleneck spatial).  x, y channel-last [B,F,H,W,C].
 * temporal != 0: sequences over F per (b,h,w); else sequences over (h w) per (b,f).  dim_head must be 32.
 * wqkv_packed: vdx_pack_conv_weights of the [C, 3*heads*32] matrix (q|k|v column blocks); bqkv [3*heads*32];
 * wo_packed: packed [heads*32, C] matrix; bo [C]. */
int vdx_attention_forward(int mode, const float* x, float* y, const void* wqkv_packed, const float* bqkv,
                          const void* wo_packed, const float* bo, int batch, int frames, int h, int w, int c, int heads,
                          int temporal, void* stream);
/* Same; fp8_core != 0 (VDX_MODE_BF16 only): QK^T and PV of sequences of <= 16 tokens on e4m3 operands (see vdx_set_attention_fp8;
 * longer sequences ignore the flag). */
int vdx_attention_forward_ex(int mode, const float* x, float* y, const void* wqkv_packed, const float* bqkv,
                             const void* wo_packed, const float* bo, int batch, int frames, int h, int w, int c, int heads,
                             int temporal, int fp8_core, void* stream);

/* Same block on bf16 TENSORS (the form the network runs under bf16 activation storage, vdx_set_activation_storage): x and y are
 * channel-last bf16 [batch, frames, h, w, c]; VDX_MODE_BF16 operands.  The level-0 shape of the N config (c = 64, 8 heads, temporal,
 * 16 frames) runs attention_w_kernel (one wave per group of 4 sequences), other shapes the kernels of vdx_attention_forward. */
int vdx_attention_forward_bf16(const void* x_bf16, void* y_bf16, const void* wqkv_packed, const float* bqkv,
                               const void* wo_packed, const float* bo, int batch, int frames, int h, int w, int c, int heads,
                               int temporal, int fp8_core, void* stream);

/* The attention block with a pre-softmax bias, as the network runs its temporal blocks under vdx_set_temporal_pos_bias: bias is device fp32
 * [heads][L][L] (L = frames when temporal, else h * w; at most 64), added to q_i . k_j / sqrt(d) before the key mask and the softmax.
 * io_bf16: x and y hold bf16 (VDX_MODE_BF16 only).  Always the generic fused kernels (BIAS instantiations). */
int vdx_attention_forward_bias(int mode, const void* x, void* y, int io_bf16, const void* wqkv_packed, const float* bqkv,
                               const void* wo_packed, const float* bo, const float* bias, int batch, int frames, int h, int w, int c,
                               int heads, int temporal, void* stream);

/* The attention block with the per-sample focus-present mask, as the network runs the temporal blocks of downs / mid / ups under
 * vdx_set_focus_present(mode 2): focus_dev is device memory, focus_n bytes; sequence s belongs to sample s / (h * w) when temporal (s itself
 * otherwise) and reads focus_dev[sample % focus_n].  A set byte masks every score of the sample with key != query to -1e30 -- after the bias,
 * in the place of the key mask -- so each of its tokens attends to itself only: the softmax row is exactly one-hot and the block's output
 * for that sample is x + bo + Wo . rd(Wv x + bv) (rd: the mode's operand rounding).  bias_or_null: as in vdx_attention_forward_bias, or null
 * for no bias.  Unmasked samples are bit-equal to vdx_attention_forward_bias on the same inputs.  Always the generic fused kernels. */
int vdx_attention_forward_focus(int mode, const void* x, void* y, int io_bf16, const void* wqkv_packed, const float* bqkv,
                                const void* wo_packed, const float* bo, const float* bias_or_null, const unsigned char* focus_dev, int focus_n,
                                int batch, int frames, int h, int w, int c, int heads, int temporal, void* stream);

/* The block of a batch in which EVERY sample is focus-present (vdx_set_focus_present(mode 1)): y = x + bo + Wo . rd(Wv x + bv) in one launch
 * of attention_present_kernel -- pointwise over the token rows, reads only the v rows of wqkv_packed; no q, no k, no scores.
 * C % 4 == 0 (8 for bf16 tensors), C <= 1024; any number of tokens. */
int vdx_attention_present_forward(int mode, const void* x, void* y, int io_bf16, const void* wqkv_packed, const float* bqkv,
                                  const void* wo_packed, const float* bo, int batch, int frames, int h, int w, int c, int heads, int temporal,
                                  void* stream);

/* SpatialLinearAttention + residual (reference: modules.py:64-129 inside Residual(PreNorm(..)), unet3d.py:170-178).
 * heads must be 8, head dim 32.  wq/wk/wv_packed: packed [C,256]; wo_packed: packed [256,C].
 * workspace: vdx_sla_workspace_bytes(mode, batch*frames, h*w, heads). */
size_t vdx_sla_workspace_bytes(int mode, int nframes, int npix, int heads);
int vdx_sla_forward(int mode, const float* x, float* y, const void* wq_packed, const void* wk_packed, const void* wv_packed,
                    const void* wo_packed, void* workspace, int batch, int frames, int h, int w, int c, int heads, void* stream);

/* The same block on bf16 channel-last tensors (bf16 activation storage; VDX_MODE_BF16 operands).  c = 64 with >= 128 frames runs the
 * second half on sla_out_w_kernel (one wave per 64 pixels), other shapes the kernels of vdx_sla_forward.  workspace:
 * vdx_sla_workspace_bytes(VDX_MODE_BF16, batch*frames, h*w, heads). */
int vdx_sla_forward_bf16(const void* x_bf16, void* y_bf16, const void* wq_packed, const void* wk_packed, const void* wv_packed,
                         const void* wo_packed, void* workspace, int batch, int frames, int h, int w, int c, int heads, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Forward forms of the network (test-facing).  vdx_unet_forward composes launches and sets flags on the launchers that the
 * operator-level entry points above never do: the per-head attention / SLA kernels of the wide levels followed by the 1x1
 * out-projection with residual, the long attention core between two 1x1 convs, bf16 TENSORS on the tail, the final conv and the init
 * conv, the final conv inside the last tail, the MFMA init conv, the scale/shift pass.  The functions below call the same
 * compositions (model.hip: attention_block_forward, sla_block_forward) and the same launchers, so that each of those kernel forms can be
 * compared with a reference on its own (tests/test_gpu_forward_forms.py).  No kernel is specific to them.
 * ---------------------------------------------------------------------------------------------- */

/* Scratch the two attention compositions need for a block of `batch` samples: the per-head output [rows][heads*32] bf16 of the heads
 * path, or qkv + o [rows][4*heads*32] fp32 of the long path (h*w > 64, spatial). */
size_t vdx_attention_heads_scratch_bytes(int batch, int frames, int h, int w);
size_t vdx_attention_long_scratch_bytes(int batch, int frames, int h, int w, int heads);

/* Attention block as run_attn launches it at the wide levels of a VDX_MODE_BF16 network: attention_head_kernel (q|k|v projection +
 * core per head) -> o_scratch [rows][256] bf16 (caller-owned, so the core can be checked apart from the projection), then the 1x1
 * out-projection + bias + residual -> y.  x, y fp32 or (io_bf16) bf16 channel-last [batch, frames, h, w, c]; 8 heads x 32; weights as
 * vdx_attention_forward (VDX_MODE_BF16 packing).  VDX_ERR_INVALID exactly where run_attn would not take this path (c < 256, c % 128,
 * more than 16 temporal / 64 spatial tokens, a scratch that is too small). */
int vdx_attention_heads_forward(const void* x, void* y, int io_bf16, const void* wqkv_packed, const float* bqkv, const void* wo_packed,
                                const float* bo, void* o_scratch, size_t o_scratch_bytes, int batch, int frames, int h, int w, int c,
                                int temporal, int fp8_core, void* stream);

/* Spatial attention over more than 64 tokens as run_attn launches it: 1x1 q|k|v conv -> fp32 core (attention_long_core_kernel) -> 1x1
 * out-projection + bias + residual.  scratch: vdx_attention_long_scratch_bytes, holds qkv [rows][3*heads*32] then o [rows][heads*32],
 * fp32.  io_bf16 needs VDX_MODE_BF16.  h*w <= 64 is VDX_ERR_INVALID.  The forward serves every h*w up to 640; the backward of this block
 * (vdx_unet_backward, vdx_attention_core_backward*) serves the multiples of 64 among them. */
int vdx_attention_long_forward(int mode, const void* x, void* y, int io_bf16, const void* wqkv_packed, const float* bqkv,
                               const void* wo_packed, const float* bo, void* scratch, size_t scratch_bytes, int batch, int frames, int h,
                               int w, int c, int heads, void* stream);

/* SpatialLinearAttention block as run_sla launches it at the wide levels: sla_head_kernel -> o_scratch [rows][256] bf16
 * (caller-owned), then the 1x1 to_out + residual -> y.  VDX_ERR_INVALID where run_sla would not take this path (c < 256, c % 128,
 * h*w % 16). */
int vdx_sla_heads_forward(const void* x, void* y, int io_bf16, const void* wq_packed, const void* wk_packed, const void* wv_packed,
                          const void* wo_packed, void* o_scratch, size_t o_scratch_bytes, int batch, int frames, int h, int w, int c,
                          void* stream);

/* vdx_resblock_tail with a storage type per tensor (run_res: y2 bf16 in bf16 mode, r / out bf16 under bf16 activation storage).
 * All three bf16 with c % 8 == 0 runs resblock_tail16_kernel, anything else resblock_tail_kernel. */
int vdx_resblock_tail_ex(const void* y2, int y2_bf16, const void* r, int r_bf16, void* out, int out_bf16, const double* stats,
                         const float* gn_gamma, const float* gn_beta, int groups, const float* ln_gamma, const float* ln_beta, int c,
                         int batch, long pix_per_sample, void* stream);

/* vdx_resblock_tail_rc_bf16 with the network's one-channel head inside (the FIN form of resblock_tail_rc16_kernel, model.hip run_res
 * for the last block): fin_out [batch * pix_per_sample] fp32 = out . fin_w[c] + fin_b[0] is written INSTEAD of out (the dot product
 * takes the fp32 values of out, nothing is rounded to bf16).  Served: (c0 + c1, c) in {(128, 64), (64, 32)} with c1 == c0. */
int vdx_resblock_tail_rc_head_bf16(const void* y2, const void* x0, const void* x1, int c0, int c1, const void* rc_w_packed,
                                   const float* rc_bias, const double* stats, const float* gn_gamma, const float* gn_beta, int groups,
                                   const float* ln_gamma, const float* ln_beta, int c, const float* fin_w, const float* fin_b,
                                   float* fin_out, int batch, long pix_per_sample, void* stream);

/* vdx_final_conv with x_bf16: x holds bf16 (d % 8 == 0; final_conv16_kernel for d in {8, 16, 32, 64, 128} and cout <= 4, else
 * final_conv_kernel). */
int vdx_final_conv_ex(const void* x, int x_bf16, const float* kernel, const float* bias, float* y, long npix, int d, int cout,
                      void* stream);

/* vdx_init_conv as the network launches it: mode VDX_MODE_BF16 with cin == 1 runs init_conv_mfma_kernel (x and the kernel rounded to
 * bf16, fp32 accumulate); y_bf16: y is WRITTEN as bf16 (VDX_MODE_BF16 only). */
int vdx_init_conv_ex(int mode, const float* x, const float* kernel, const float* bias, void* y, int y_bf16, int batch, int cin,
                     int frames, int h, int w, int cout, int k, void* stream);

/* Every ResnetBlock's (scale, shift) in one launch pair (resblock_ss_lin_kernel, resblock_ss_norm_kernel; reference modules.py:202-208,
 * 233-238): for layer l and sample b, lin[out_off * batch + b * n ..] = SiLU(temb[b]) . W + bias and ss[same] = LayerNorm_n(lin).
 * Offsets are in floats: w_off ([temb_dim][n] Flax kernel), b_off, g_off, be_off into params; out_off (per sample) into ss / lin.
 * layers_dev: device array of nlayers entries; max_n = the widest layer (n <= 2048). */
typedef struct { long w_off, b_off, g_off, be_off, out_off; int n; int pad_; } vdx_ss_layer;
int vdx_resblock_scale_shift(const float* params, const float* temb, const vdx_ss_layer* layers_dev, int nlayers, float* ss, float* lin,
                             int temb_dim, int batch, int max_n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Network-level entry points.
 * ---------------------------------------------------------------------------------------------- */

/* Mirror of the reference constructors' arguments that shape the device work:
 * Unet3D(dim, rngs, dim_mults, cond_dim, out_dim, channels, attn_heads, attn_dim_head, use_bert_text_cond,
 *        init_dim, init_kernel_size, use_sparse_linear_attn, block_type, resnet_groups)   unet3d.py:58-75
 * GaussianDiffusion(image_size, num_frames, ...)                                          gaussian_diffusion.py:53-65
 * (use_bert_text_cond is resolved by the host to cond_dim = 768; 0 means "no conditioning"). */
typedef struct {
    int dim;
    int n_mults; int dim_mults[8];
    int channels;
    int out_dim;                 /* 0 = channels */
    int cond_dim;                /* 0 = none */
    int attn_heads, attn_dim_head;
    int init_dim;                /* 0 = dim */
    int init_kernel_size;
    int use_sparse_linear_attn;
    int resnet_groups;
    int image_size, num_frames;
    int mode;                    /* vdx_mode */
} vdx_config;

typedef struct vdx_handle vdx_handle;

int vdx_create(const vdx_config* cfg, vdx_handle** out);
void vdx_destroy(vdx_handle* h);

/* Activation storage of vdx_unet_forward / vdx_p_sample_loop.  0 (default): every inter-kernel activation is fp32 in the
 * workspace (required by vdx_unet_backward, and what vdx_slot_info describes).  1 (VDX_MODE_BF16 handles only): they are
 * stored as bf16 -- half the HBM traffic of the bandwidth-bound levels; arithmetic stays fp32-accumulate.  The reference
 * has no such knob (XLA picks its own buffer types); this is the "bf16" of BASELINE.json's sampling configuration. */
int vdx_set_activation_storage(vdx_handle* h, int bf16);
int vdx_get_activation_storage(const vdx_handle* h);

/* fp8 attention (BASELINE.json configs[4]: "fp8 attention QK^T / PV on CDNA4"; no reference counterpart -- XLA picks its own types).
 * VDX_MODE_BF16 handles only, forward / sampling only.  1: the QK^T and PV products of every attention block over <= 16 tokens (all
 * temporal attention blocks of the configured shapes) round their operands (q, k, v, softmax probabilities) to OCP e4m3 and run on
 * v_mfma_f32_16x16x32_fp8_fp8, fp32 accumulate and fp32 softmax; projections stay bf16.  Longer sequences (the 64-token spatial block
 * of the bottleneck) keep bf16 operands.  Tolerance: tests/test_gpu_blocks.py (attention block 4e-2 of the attention branch). */
int vdx_set_attention_fp8(vdx_handle* h, int on);
int vdx_get_attention_fp8(const vdx_handle* h);

/* Temporal relative position bias (reference: RelativePositionBias, modules.py:350-390, built by unet3d.py and handed to every temporal
 * attention block -- where PreNorm drops it; DESIGN.md 9: an extension, parity unpinned).  Off (default): the network is the
 * reference's, equivariant under permutations of its frames, bit for bit and launch for launch what it was.  On: the ten temporal
 * attention blocks (init, downs, mid temporal, ups) compute softmax_j(q_i . k_j / sqrt(d) + bias[h][i][j]) v_j with
 * bias[h][i][j] = embedding[buckets[i * F + j]][h] -- BEFORE the softmax (the T5 / Video Diffusion Models form; the reference's dead code
 * would add it after).  The mid spatial attention gets none.  `buckets`: HOST int [F * F], values in [0, 32), F = the handle's
 * num_frames (the map of modules.py:350-390 with its defaults of 32 buckets / max distance 128; the Python package computes it); it is
 * uploaded here, once, never during a capture; ignored (may be null) when on == 0.  Every cached sampling graph of the handle is dropped.
 * The embedding is the parameter "time_rel_pos_bias.relative_attention_bias.embedding" of the flat buffer: no new parameter.  With the
 * switch on the temporal blocks run the generic fused kernels (attention_reg_kernel / attention_kernel, BIAS instantiations) and
 * vdx_unet_backward the generic attention route, whose cores emit dBias deterministically (fixed grid of slots + ordered sum; the stem
 * stage scatters it to the embedding's gradient).  VDX_ERR_STATE together with fp8 attention, VDX_ERR_INVALID for more than 64 frames. */
int vdx_set_temporal_pos_bias(vdx_handle* h, int on, const int* buckets);
int vdx_get_temporal_pos_bias(const vdx_handle* h);

/* Focus-present mask: joint image-video training and "image mode" sampling (Video Diffusion Models, Ho et al. 2022, section 3.1; reference:
 * the focus_present_mask keyword that PreNorm drops; DESIGN.md 9: an extension, parity unpinned).  A focus-present sample is
 * treated as a bag of images: in the nine temporal attention blocks of downs, mid and ups every frame attends to itself only.  The mask
 * is applied BEFORE the softmax (scores with key != query become -1e30, after the position bias when that is on), so the softmax row is
 * exactly one-hot; the reference's dead code would mask after it.  init_temporal_attn and the mid spatial attention are never masked.
 * GroupNorm statistics span the frames, so the frames of a masked sample are still not independent of each other.
 *   mode 0: off (default): bit for bit and launch for launch what the handle did before.
 *   mode 1: every sample.  The forward runs attention_present_kernel (one launch per block); the backward the masked generic cores.
 *   mode 2: per sample.  mask_dev is the CALLER's device pointer to n bytes; it is stored, not copied, and read when the kernels run: its
 *           contents may change between calls (and between replays of a captured sampling graph) without a new call.  Row r of a forward,
 *           backward or sampling loop reads mask_dev[r % n] (a guided 2B-row forward works with a [B] mask); a batch that is no multiple
 *           of n fails with VDX_ERR_INVALID.  The temporal blocks run the generic fused kernels (FOCUS instantiations) and the generic
 *           backward route, as under vdx_set_temporal_pos_bias, with which it combines.
 * Any change of mode, pointer or n drops the handle's cached sampling graphs.  VDX_ERR_STATE together with fp8 attention, VDX_ERR_INVALID
 * for more than 64 frames. */
int vdx_set_focus_present(vdx_handle* h, int mode, const unsigned char* mask_dev, int n);
int vdx_get_focus_present(const vdx_handle* h);

/* Flat fp32 parameter buffer layout (names = nnx state-tree paths, shapes = Flax shapes). */
int vdx_param_count(const vdx_handle* h);
long vdx_param_total(const vdx_handle* h);                       /* floats in the flat buffer */
int vdx_param_info(const vdx_handle* h, int index, char* name, int name_cap, int* ndim, long shape[6], long* offset);

/* Derived (packed) weights in the MFMA staging layout; re-run after every parameter update. */
size_t vdx_packed_bytes(const vdx_handle* h);
int vdx_pack_params(const vdx_handle* h, const float* params, void* packed, void* stream);

/* Activation workspace for a batch; every intermediate keeps its own slot (inspectable for parity tests). */
size_t vdx_workspace_bytes(const vdx_handle* h, int batch);
int vdx_slot_count(const vdx_handle* h);
int vdx_slot_info(const vdx_handle* h, int index, char* name, int name_cap, long* floats_per_sample, long* float_offset_per_sample);

/* Unet3D.__call__ (reference: unet3d.py:262-387).  x [B,C,F,H,W]; time [B] int32 (device); cond [B,cond_dim] or NULL;
 * cond_mask [B] bytes (1 = replace by null_cond_emb) or NULL, in which case null_all selects all/none
 * (null_cond_prob 1 / 0); out channel-LAST [B,F,H,W,out_dim] (unet3d.py:387). */
int vdx_unet_forward(const vdx_handle* h, const float* params, const void* packed, const float* x, const int* time,
                     const float* cond, const unsigned char* cond_mask, int null_all, float* out, void* workspace,
                     size_t workspace_bytes, int batch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GaussianDiffusion device work.  External tensors [B,C,F,H,W]; eps_hat is the UNet output, channel-last.
 * ---------------------------------------------------------------------------------------------- */

/* N(0,1) stream replacing jax.random.normal (gaussian_diffusion.py:254,309,416,445): Philox4x32-10 keyed by `seed`,
 * draw number = offset (+ *dev_offset when given, a device counter advanced by the sampling loop). */
int vdx_randn(float* out, long n, uint64_t seed, uint64_t offset, const uint64_t* dev_offset, void* stream);

/* q_sample (gaussian_diffusion.py:401-420) with normalize_img folded in: x_t = sqrt_ac[t] (x0*pre_scale+pre_shift)
 * + sqrt_1m_ac[t] noise.  t device int32 [B]; tables are device fp32 [T]. */
int vdx_q_sample(const float* x_start, const int* t, const float* noise, float* out, const float* sqrt_ac,
                 const float* sqrt_one_minus_ac, int batch, long per_sample, float pre_scale, float pre_shift, void* stream);

/* p_sample (gaussian_diffusion.py:231-261 incl. predict_start_from_noise :120-136, clip :203-220, q_posterior :139-159).
 * tables: device fp32 [5][T] = sqrt_recip_ac | sqrt_recipm1_ac | posterior_mean_coef1 | posterior_mean_coef2 |
 * posterior_log_variance_clipped.  noise NULL -> Philox(seed, offset + *dev_offset) (per_sample % 4 == 0 required).
 * thres: per-sample dynamic-threshold s [B] or NULL.  x and out may alias. */
int vdx_p_sample_step(const float* x, const float* eps_hat, float* out, const int* t, const float* tables, int timesteps,
                      const float* noise, uint64_t seed, uint64_t offset, const uint64_t* dev_offset, const float* thres,
                      int clip_denoised, int batch, int channels, long per_sample, void* stream);

/* sum |eps_hat - noise| (l2 == 0) or (eps_hat - noise)^2 (l2 != 0) accumulated into *acc (device double, pre-zeroed);
 * the mean of gaussian_diffusion.py:463-466 is acc / (batch*channels*fhw). */
int vdx_loss_sum(const float* eps_hat, const float* noise, double* acc, int batch, int channels, long fhw, int l2, void* stream);

/* y = a x + b (normalize_img / unnormalize_img, utils.py:259-280). */
int vdx_affine(const float* x, float* y, long n, float a, float b, void* stream);

/* p_sample_loop (gaussian_diffusion.py:264-320): img holds x_T on entry and x_0 (still in [-1,1]) on return.
 * t_dev [B] int32 must hold T-1, *step_dev (device uint64) must be 0 on entry; eps_buf [B,F,H,W,out_dim] scratch.
 * One step = Unet3D forward + p_sample + (t -= 1); with use_graph != 0 the step is captured once into a hipGraph on
 * `stream` (which must not be the legacy default stream) and replayed, so the loop issues no per-step host work.
 * Draw k of the noise stream is Philox(seed, 1 + k); the caller draws x_T itself (e.g. vdx_randn with offset 0).
 * nsteps (<= timesteps) steps are enqueued, continuing from the state in t_dev / step_dev, so a loop may be issued in
 * pieces.  The instantiated graph is cached in the handle and reused while every argument but nsteps is unchanged. */
int vdx_p_sample_loop(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, int* t_dev,
                      uint64_t* step_dev, const float* tables, int timesteps, int nsteps, const float* cond, uint64_t seed,
                      int clip_denoised, void* workspace, size_t workspace_bytes, int batch, int use_graph, void* stream);

/* Dynamic thresholding of p_mean_variance (gaussian_diffusion.py:205-217): s[b] = max(quantile(|x0_hat_b|, percentile), 1) with
 * x0_hat = predict_start_from_noise(x, t, eps_hat) and the linearly interpolated quantile (jnp.quantile default).  tables as in
 * vdx_p_sample_step (rows 0 and 1 are used).  thres_out [B]. */
int vdx_dynamic_threshold(const float* x, const float* eps_hat, const int* t, const float* tables, int timesteps, float percentile,
                          float* thres_out, int batch, int channels, long per_sample, void* stream);

/* vdx_p_sample_loop with use_dynamic_thres (gaussian_diffusion.py:205-217) inside the captured step: thres_buf [B] floats scratch,
 * percentile in (0, 1].  percentile <= 0 is exactly vdx_p_sample_loop. */
int vdx_p_sample_loop_dyn(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, int* t_dev,
                          uint64_t* step_dev, const float* tables, int timesteps, int nsteps, const float* cond, uint64_t seed,
                          int clip_denoised, float percentile, float* thres_buf, void* workspace, size_t workspace_bytes, int batch,
                          int use_graph, void* stream);

/* DDIM sampling, eta = 0 (EXTENSION: the reference has ancestral DDPM sampling only; BASELINE.json configs[3] names "DDIM-100").
 * One step: x0 = (x - sqrt(1-ac_t) eps) / sqrt(ac_t), clipped like p_sample; eps' re-derived from the clipped x0;
 * out = sqrt(ac_next) x0 + sqrt(1-ac_next) eps'.  seq: device int32 [n + 1] = the time sequence t_0 > t_1 > ... > t_{n-1}, -1
 * (-1 = the data, alpha_bar 1); step k uses (seq[k], seq[k+1]) with k = *step_dev (device uint64) or 0 when step_dev is NULL.
 * alphas_cumprod: device fp32 [T].  x and out may alias. */
int vdx_ddim_step(const float* x, const float* eps_hat, float* out, const float* alphas_cumprod, const int* seq,
                  const uint64_t* step_dev, const float* thres, int clip_denoised, int batch, int channels, long per_sample, void* stream);

/* The DDIM loop: nsteps x { Unet3D forward at t = seq[k] ; vdx_ddim_step ; t = max(seq[k+1], 0), k += 1 }, captured once in a
 * hipGraph like vdx_p_sample_loop.  t_dev [B] must hold seq[0] and *step_dev 0 on entry; seq_len = n (seq has n + 1 entries). */
int vdx_ddim_sample_loop(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, int* t_dev,
                         uint64_t* step_dev, const float* alphas_cumprod, const int* seq, int seq_len, int nsteps, const float* cond,
                         int clip_denoised, void* workspace, size_t workspace_bytes, int batch, int use_graph, void* stream);

/* vdx_ddim_sample_loop with use_dynamic_thres inside the captured step (the threshold of gaussian_diffusion.py:205-217 applied to DDIM's
 * x0): tables = the [5][T] tables of vdx_p_sample_step (rows 0, 1 are read), thres_buf [B] floats scratch, percentile in (0, 1].
 * percentile <= 0 is exactly vdx_ddim_sample_loop. */
int vdx_ddim_sample_loop_dyn(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, int* t_dev,
                             uint64_t* step_dev, const float* alphas_cumprod, const int* seq, int seq_len, int nsteps, const float* cond,
                             int clip_denoised, const float* tables, int timesteps, float percentile, float* thres_buf, void* workspace,
                             size_t workspace_bytes, int batch, int use_graph, void* stream);

/* Frame-conditioned sampling (EXTENSION: the replacement method of Ho et al. 2022, "Video Diffusion Models" sec. 3.1, with
 * optional RePaint resampling, Lugmayr et al. 2022).  known = 2 video - 1 [B,C,F,H,W]; mask [B,C,F,H,W] bytes, nonzero = known;
 * mask_tables: device fp32 [4][T] = sqrt_ac | sqrt(1 - ac) | sqrt(alpha) | sqrt(beta).  s is the global step counter (0, 1, ...
 * over every reverse step incl. the resampling ones).  Draws: x_T = Philox(seed, 0), step noise 1 + s (as vdx_p_sample_loop), the
 * known region's noise VDX_DRAW_KNOWN + s, the re-noise VDX_DRAW_RENOISE + s.  per_sample % 4 == 0 everywhere, and the kernels move
 * 4 elements at a time: x / img, known and out must be 16-byte aligned, mask 4-byte aligned (checked: VDX_ERR_INVALID).
 *
 * Clean context (for a denoiser trained with vdx_q_sample_masked / vdx_loss_sum_masked below, RaMViD): every kernel here forms the
 * known region as mask_tables[0][.] * known + mask_tables[1][.] * z.  A mask_tables whose row 0 is all 1 and row 1 all 0 (rows 2, 3
 * unchanged) makes that `known` exactly, at vdx_inpaint_init (x = mask ? known : x_T) and at every step of all three loops: the
 * known frames then enter the network clean at every noise level, which is what such a denoiser was trained on.  No other kernel or
 * argument changes; the VDX_DRAW_KNOWN draws are still made and multiplied by 0.  Not with resample_steps > 1: the re-noise of rows
 * 2, 3 touches the whole tensor. */
#define VDX_DRAW_KNOWN (1ull << 62)
#define VDX_DRAW_RENOISE (1ull << 63)

/* First merge, in place: x = mask ? sqrt_ac[t0] known + sqrt(1 - ac[t0]) x : x (the known region noised with x_T's own noise).
 * n = B*C*F*H*W, n % 4 == 0; t0 = T-1 for the ancestral chain. */
int vdx_inpaint_init(float* x, const float* known, const unsigned char* mask, const float* mask_tables, int timesteps, int t0,
                     long n, void* stream);

/* One masked ancestral step at t = t[b], s = step + (*step_dev if step_dev): x' = vdx_p_sample_step(x, Philox(seed, 1 + s));
 * kn = t == 0 ? known : sqrt_ac[t-1] known + sqrt(1 - ac[t-1]) Philox(seed, VDX_DRAW_KNOWN + s); out = mask ? kn : x';
 * then, when s % resample_steps != resample_steps - 1, out = sqrt(alpha_t) out + sqrt(beta_t) Philox(seed, VDX_DRAW_RENOISE + s)
 * (back to level t).  tables / thres / clip as vdx_p_sample_step.  An all-zero mask with resample_steps 1 is vdx_p_sample_step
 * with offset 1 + s, bit for bit.  x and out may alias. */
int vdx_p_sample_step_masked(const float* x, const float* eps_hat, float* out, const int* t, const float* tables, int timesteps,
                             const float* known, const unsigned char* mask, const float* mask_tables, int resample_steps,
                             uint64_t seed, uint64_t step, const uint64_t* step_dev, const float* thres, int clip_denoised,
                             int batch, int channels, long per_sample, void* stream);

/* vdx_p_sample_loop_dyn with the masked step: one step = Unet3D forward + (dynamic threshold) + vdx_p_sample_step_masked with
 * s = *step_dev + { t -= 1 when s % resample_steps == resample_steps - 1 ; s += 1 }, so one captured step serves every (t, u).
 * img holds vdx_inpaint_init's output on entry; t_dev = T-1, *step_dev = 0.  nsteps <= timesteps * resample_steps.  Own graph
 * slot: does not evict the graphs of the unconditional loops. */
int vdx_p_sample_loop_masked(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, int* t_dev,
                             uint64_t* step_dev, const float* tables, int timesteps, int nsteps, const float* cond, uint64_t seed,
                             int clip_denoised, float percentile, float* thres_buf, const float* known, const unsigned char* mask,
                             const float* mask_tables, int resample_steps, void* workspace, size_t workspace_bytes, int batch,
                             int use_graph, void* stream);

/* One masked DDIM step (eta = 0; no resampling): x' = vdx_ddim_step(x) from seq[j] to seq[j+1], j = *step_dev (or 0);
 * kn = seq[j+1] < 0 ? known : sqrt_ac[tn] known + sqrt(1 - ac[tn]) Philox(seed, VDX_DRAW_KNOWN + j); out = mask ? kn : x'.
 * mask_tables has rows of length `timesteps`.  The DDIM chain starts from vdx_inpaint_init with t0 = seq[0].  An all-zero mask is
 * vdx_ddim_step bit for bit.  x and out may alias. */
int vdx_ddim_step_masked(const float* x, const float* eps_hat, float* out, const float* alphas_cumprod, const int* seq,
                         const uint64_t* step_dev, const float* thres, int clip_denoised, const float* known, const unsigned char* mask,
                         const float* mask_tables, int timesteps, uint64_t seed, int batch, int channels, long per_sample, void* stream);

/* vdx_ddim_sample_loop_dyn with vdx_ddim_step_masked as the step (draw of step j: VDX_DRAW_KNOWN + j).  timesteps is required
 * (mask_tables' row length) even without the dynamic threshold.  Own graph slot, as vdx_p_sample_loop_masked. */
int vdx_ddim_sample_loop_masked(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, int* t_dev,
                                uint64_t* step_dev, const float* alphas_cumprod, const int* seq, int seq_len, int nsteps, const float* cond,
                                int clip_denoised, const float* tables, int timesteps, float percentile, float* thres_buf,
                                const float* known, const unsigned char* mask, const float* mask_tables, uint64_t seed,
                                void* workspace, size_t workspace_bytes, int batch, int use_graph, void* stream);

/* DPM-Solver++(2M) sampling (EXTENSION, parity unpinned: no reference code.  Lu et al. 2022, "DPM-Solver++", the data-prediction
 * multistep form): the same one network evaluation per step as DDIM, second order through one history tensor the size of the image.
 * With a_t = alphas_cumprod[t]: alpha_t = sqrt(a_t), sigma_t = sqrt(1 - a_t), lambda_t = 0.5 ln(a_t / (1 - a_t)).  seq as in
 * vdx_ddim_step (n + 1 entries, the last -1 = the data).  Step k = *step_dev (or 0 when step_dev is NULL) goes from s = seq[k] to
 * n = seq[k+1]:
 *   x0 = (x - sigma_s eps) / alpha_s                  clipped exactly as vdx_ddim_step does (+-1, or +-thres[b] then / thres[b])
 *   n < 0:  out = x0                                  (the step into the data is first order; in [-1, 1] when clipping)
 *   else    h = lambda_n - lambda_s
 *           D = x0                                    if k == 0 or order == 1
 *           D = (1 + c) x0 - c hist,  c = h / (2 (lambda_s - lambda_{seq[k-1]}))       otherwise
 *           out = (sigma_n / sigma_s) x - alpha_n expm1(-h) D
 *   hist = x0                                         (written on every step when hist is given)
 * Whether a step is first or second order is decided from *step_dev on the device, so one captured step serves every k.  order is 1
 * or 2; order 1 is algebraically vdx_ddim_step (including its re-derivation of eps from the clipped x0) and may pass hist = NULL.
 * hist [B,C,F,H,W] floats: read (k >= 1, order 2) before it is written, by the same thread.  The kernels move 4 elements at a time:
 * per_sample % 4 == 0, x / out / hist 16-byte aligned (checked: VDX_ERR_INVALID).  x and out may alias; hist may alias neither. */
int vdx_dpm_step(const float* x, const float* eps_hat, float* out, float* hist, const float* alphas_cumprod, const int* seq,
                 const uint64_t* step_dev, const float* thres, int clip_denoised, int order, int batch, int channels, long per_sample,
                 void* stream);

/* vdx_dpm_step with the known region merged as vdx_ddim_step_masked does: kn = seq[k+1] < 0 ? known : sqrt_ac[n] known +
 * sqrt(1 - ac[n]) Philox(seed, VDX_DRAW_KNOWN + k); out = mask ? kn : x'.  hist holds the network's x0 everywhere.  An all-zero mask
 * is vdx_dpm_step bit for bit. */
int vdx_dpm_step_masked(const float* x, const float* eps_hat, float* out, float* hist, const float* alphas_cumprod, const int* seq,
                        const uint64_t* step_dev, const float* thres, int clip_denoised, int order, const float* known,
                        const unsigned char* mask, const float* mask_tables, int timesteps, uint64_t seed, int batch, int channels,
                        long per_sample, void* stream);

/* The DPM-Solver++ loop: nsteps x { Unet3D forward at t = seq[k] ; (dynamic threshold) ; vdx_dpm_step ; t = max(seq[k+1], 0), k += 1 },
 * captured once in a hipGraph like vdx_ddim_sample_loop_dyn, whose arguments it takes plus hist and order.  t_dev [B] must hold seq[0]
 * and *step_dev 0 on entry; a loop issued in pieces continues from t_dev / step_dev / hist.  percentile <= 0: static clip.  Own graph
 * slot: does not evict the graphs of the other loops. */
int vdx_dpm_sample_loop(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, float* hist, int* t_dev,
                        uint64_t* step_dev, const float* alphas_cumprod, const int* seq, int seq_len, int nsteps, const float* cond,
                        int clip_denoised, int order, const float* tables, int timesteps, float percentile, float* thres_buf,
                        void* workspace, size_t workspace_bytes, int batch, int use_graph, void* stream);

/* vdx_dpm_sample_loop with vdx_dpm_step_masked as the step; img holds vdx_inpaint_init's output (t0 = seq[0]) on entry.  timesteps is
 * required (mask_tables' row length) even without the dynamic threshold.  Own graph slot. */
int vdx_dpm_sample_loop_masked(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, float* hist, int* t_dev,
                               uint64_t* step_dev, const float* alphas_cumprod, const int* seq, int seq_len, int nsteps, const float* cond,
                               int clip_denoised, int order, const float* tables, int timesteps, float percentile, float* thres_buf,
                               const float* known, const unsigned char* mask, const float* mask_tables, uint64_t seed,
                               void* workspace, size_t workspace_bytes, int batch, int use_graph, void* stream);

/* Classifier-free guidance (EXTENSION, parity unpinned: no reference code -- the reference's p_sample_loop drops cond; Ho & Salimans
 * 2022, with the guidance rescale of Lin et al. 2023, sec. 3.4).  eps2 [2 * batch][per_sample] is the output of ONE forward over 2 * batch
 * samples: rows [0, batch) conditioned (c), rows [batch, 2 * batch) on the null embedding (n).  out [batch][per_sample]:
 *   g   = n + (c - n) * cond_scale          three separately rounded fp32 operations, no contraction: bit for bit what
 *                                           Unet3D.forward_with_cond_scale forms with torch
 *   out = g                                 rescale == 0 (one kernel)
 *   out = g * (float)(rescale * std(c) / std(g) + 1 - rescale)          rescale in (0, 1], the standard deviations per sample
 * For the rescale a statistics pass forms g again with the same three operations and adds sum c, sum c^2, sum g, sum g^2 per sample in
 * double: a fixed grid whatever per_sample or the device, a fixed quad-to-thread map, a fixed-order tree per workgroup, one partial per
 * workgroup in scratch, a second kernel that adds the partials in index order (the scheme of vdx_grad_sqnorm: no atomics, the bits of
 * out depend on the values only).  std^2 = (sum x^2 - (sum x)^2 / per_sample) / (per_sample - 1), the n - 1 cancels in the ratio; where
 * that of g is <= 0 or anything is not finite the factor is 1.  scratch: vdx_cfg_scratch_doubles(batch) doubles, 8-byte aligned (may be
 * NULL with rescale == 0); its tail is the cond_mask of the guided loops below.  out may be eps2 itself (the first half is then
 * overwritten in place) or disjoint from it.  The kernels move float4: per_sample % 4 == 0, eps2 / out 16-byte aligned, rescale in
 * [0, 1] (checked: VDX_ERR_INVALID). */
size_t vdx_cfg_scratch_doubles(int batch);
int vdx_cfg_combine(const float* eps2, float* out, float cond_scale, float rescale, double* scratch, int batch, long per_sample, void* stream);

/* The unmasked loops with classifier-free guidance inside the captured step: vdx_p_sample_loop_dyn, vdx_ddim_sample_loop_dyn and
 * vdx_dpm_sample_loop with cond [batch, cond_dim] required, plus cond_scale, rescale and cfg_scratch (vdx_cfg_scratch_doubles(batch)
 * doubles).  `batch` = B counts the videos; img [2B,C,F,H,W], t_dev [2B], eps_buf [2B,F,H,W,out_dim] and the workspace
 * (vdx_workspace_bytes(h, 2B)) hold 2B samples, hist and thres_buf B.  On entry img[:B] = x_T, t_dev[0..2B) = T-1 or seq[0],
 * *step_dev = 0; on return img[:B] = x_0.  One step, all of it on `stream` (a chain without parallel branches):
 *   img[B:] = img[:B]  (device-to-device copy) ; one forward over 2B samples with cond_mask = 0 for rows [0, B), 1 for rows [B, 2B) (the
 *   null rows never read cond) ; vdx_cfg_combine(eps_buf -> eps_buf[:B]) ; (dynamic threshold) ; the unguided loop's step kernel on the
 *   first B samples, with its draws ; the unguided loop's advance over all 2B entries of t_dev.
 * So the result is the bits of the step-by-step loop over Unet3D.forward_with_cond_scale and vdx_p_sample_step / vdx_ddim_step /
 * vdx_dpm_step when rescale == 0.  Own graph slots; the key holds the bits of cond_scale and rescale, cond and cfg_scratch.  DDIM too
 * needs C*F*H*W % 4 == 0 here. */
int vdx_p_sample_loop_guided(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, int* t_dev,
                             uint64_t* step_dev, const float* tables, int timesteps, int nsteps, const float* cond, uint64_t seed,
                             int clip_denoised, float percentile, float* thres_buf, float cond_scale, float rescale, double* cfg_scratch,
                             void* workspace, size_t workspace_bytes, int batch, int use_graph, void* stream);
int vdx_ddim_sample_loop_guided(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, int* t_dev,
                                uint64_t* step_dev, const float* alphas_cumprod, const int* seq, int seq_len, int nsteps, const float* cond,
                                int clip_denoised, const float* tables, int timesteps, float percentile, float* thres_buf, float cond_scale,
                                float rescale, double* cfg_scratch, void* workspace, size_t workspace_bytes, int batch, int use_graph,
                                void* stream);
int vdx_dpm_sample_loop_guided(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, float* hist, int* t_dev,
                               uint64_t* step_dev, const float* alphas_cumprod, const int* seq, int seq_len, int nsteps, const float* cond,
                               int clip_denoised, int order, const float* tables, int timesteps, float percentile, float* thres_buf,
                               float cond_scale, float rescale, double* cfg_scratch, void* workspace, size_t workspace_bytes, int batch,
                               int use_graph, void* stream);

/* Held-out evaluation (EXTENSION, no reference code: Ho et al. 2020, eq. 5; Nichol & Dhariwal 2021, calc_bpd_loop): the terms of the
 * variational bound of a video x [batch,C,F,H,W] in [0, 1], in bits per dimension (means over the C*F*H*W elements of a sample, nats /
 * ln 2).  x0 = 2 x - 1 is formed in the kernels.  vlb_tables [VDX_VLB_ROWS][timesteps] DOUBLES (device; make_vlb_tables of the Python
 * host): rows 0-5 = sqrt_ac | sqrt(1 - ac) | sqrt_recip_ac | sqrt_recipm1_ac | posterior_mean_coef1 | coef2, the fp32 schedule values
 * the sampling kernels use, widened; row 6 = w_t = coef1_t^2 / (2 post_var_t ln 2) formed in double; row 7 = the decoder's
 * log-variance, log post_var_max(t,1); row 8 = alphas_cumprod.  With t = t[b] per sample and eps = `noise` [batch,C,F,H,W] or, when
 * noise is NULL, Philox(seed, draw + *step_dev) indexed by the element index of the whole tensor (vdx_p_sample_step's stream):
 *   x_t   = sqrt_ac[t] x0 + sqrt(1 - ac[t]) eps                              (formed in double, exact products and one fused multiply-add;
 *                                                                            vdx_vlb_noise rounds it to fp32 once for the network, vdx_vlb_terms
 *                                                                            uses the double itself: the two differ by one correct rounding)
 *   x0^   = sqrt_recip_ac[t] x_t - sqrt_recipm1_ac[t] eps_hat, clamped to [-1, 1] when clip_denoised (no dynamic threshold); in double, as are
 *           the differences below
 *   mse = mean (eps_hat - eps)^2      xstart_mse = mean (x0^ - x0)^2
 *   t >= 1:  vb = mean w_t (x0 - x0^)^2         -- KL(q(x_{t-1} | x_t, x0) || p(x_{t-1} | x_t)) with both variances post_var_t
 *   t == 0:  vb = -mean log2 P(x0)              -- discretized Gaussian on the 8-bit grid (bin half-width 1/255), mean coef1_0 x0^ +
 *            coef2_0 x_t, log-variance row 7; P = max(Phi(z+), 1e-12) for x0 < -0.999, max(1 - Phi(z-), 1e-12) for x0 > 0.999,
 *            max(Phi(z+) - Phi(z-), 1e-12) otherwise, z+- = (x0 - mean +- 1/255) / sigma, evaluated in double
 * eps_hat is channel-last [batch,F,H,W,C].  vdx_vlb_terms: out [batch][3] = (vb, mse, xstart_mse); vdx_vlb_prior: out [batch] =
 * mean 0.5 (-1 - log(1 - ac_{T-1}) + (1 - ac_{T-1}) + ac_{T-1} x0^2) / ln 2.  The sums are taken in double by a fixed grid with a fixed
 * quad-to-thread map, a fixed-order tree per workgroup and an in-order sum of the workgroups' partials: no atomics, the bits of out
 * depend on the inputs only.  partial: vdx_vlb_scratch_doubles(batch) doubles.  per_sample % 4 == 0 and % channels == 0; x / xt /
 * noise 16-byte, partial / out / vlb_tables 8-byte aligned; timesteps >= 2 (all VDX_ERR_INVALID). */
#define VDX_VLB_ROWS 9
size_t vdx_vlb_scratch_doubles(int batch);
int vdx_vlb_noise(const float* x, float* xt, const int* t, const double* vlb_tables, int timesteps, const float* noise, uint64_t seed,
                  uint64_t draw, const uint64_t* step_dev, int batch, long per_sample, void* stream);
int vdx_vlb_terms(const float* x, const float* eps_hat, const int* t, const double* vlb_tables, int timesteps, const float* noise,
                  uint64_t seed, uint64_t draw, const uint64_t* step_dev, int clip_denoised, double* partial, double* out, int batch,
                  int channels, long per_sample, void* stream);
int vdx_vlb_prior(const float* x, const double* vlb_tables, int timesteps, double* partial, double* out, int batch, long per_sample,
                  void* stream);
/* nsteps repetitions of  vdx_vlb_noise(x -> xt_buf, draw 1 + k) ; the forward (xt_buf, t_dev, cond un-masked -> eps_buf) ; the terms ;
 * an advance that writes out[k][batch][3], sets t_dev[:] = max(seq[k + 1], 0) and k = *step_dev += 1 -- eagerly or (use_graph) as
 * replays of one captured step in a graph slot of its own (no sampling loop's graph is evicted).  seq: seq_len + 1 descending levels
 * ending in -1 (the DDIM loops' sequence).  On entry t_dev[0..batch) = seq[0] and *step_dev = 0, or where an earlier call over the
 * same buffers left them: the loop may be issued in pieces.  out [seq_len][batch][3]. */
int vdx_vlb_loop(vdx_handle* h, const float* params, const void* packed, const float* x, float* xt_buf, float* eps_buf, int* t_dev,
                 uint64_t* step_dev, const double* vlb_tables, int timesteps, const int* seq, int seq_len, int nsteps, const float* cond,
                 uint64_t seed, int clip_denoised, double* partial, double* out, void* workspace, size_t workspace_bytes, int batch,
                 int use_graph, void* stream);

/* Learned variances (EXTENSION, parity unpinned: no reference code.  Nichol & Dhariwal 2021, "Improved DDPM": learned reverse-process
 * variances, the hybrid loss, respaced ancestral sampling).  Off unless these entries are called: every entry above keeps refusing a
 * network with out_dim != channels.  The network has out_dim = 2 C (C = channels); its channel-last output out2 [batch,F,H,W,2C] holds
 * eps_hat in channels [0, C) and v in [C, 2C).  With f = (v + 1) / 2 (v is NOT clamped, it may extrapolate):
 *   log sigma^2 = f max_log + (1 - f) min_log,   max_log = log beta_t,   min_log = log beta~_t  (min_log[0] = log beta~_1)
 * Tables (make_lv_tables of the Python host, fp64; a respaced chain over S of the T levels has alpha_bar'_i = alpha_bar_{seq_i},
 * beta'_i = 1 - alpha_bar'_i / alpha_bar'_{i-1} and everything else derived from them; the network is still called with t = seq_i):
 *   lv_tables       float  [6][S]            sqrt_recip_ac | sqrt_recipm1_ac | coef1 | coef2 | max_log | min_log     (the step)
 *   lv_tables64     double [VDX_LV_ROWS][T]  sqrt_ac | sqrt(1 - ac) | sqrt_recip_ac | sqrt_recipm1_ac | coef1 | coef2 | max_log | min_log | ac
 *                                            (the loss and the bound; rows 0, 1 and 8 sit where vdx_vlb_noise / vdx_vlb_prior read them)
 *
 * vdx_p_sample_step_lv: x0^ = sqrt_recip_ac x - sqrt_recipm1_ac eps_hat, clamped to [-1, 1] when clip_denoised; mean = coef1 x0^ + coef2 x;
 *   out = mean + 1[i != 0] exp(0.5 log sigma^2) z, at level i = level_dev[b] or, when level_dev is NULL, S - 1 - (step + *step_dev).
 *   z = noise, or Philox(seed, offset + *dev_offset) indexed as vdx_p_sample_step does (per_sample % 4 == 0 then).  On level 0 the result
 *   is out * post_scale + post_shift (unnormalize_img folded into the last step; 1, 0 = none).  The arithmetic is vdx_p_sample_step's: at
 *   v = -1 and min_log = posterior_log_variance_clipped the two write the same bits.  Any per_sample; x and out may alias.
 * vdx_p_sample_loop_lv: nsteps x { forward at t_dev -> out2_buf ; the step at level S - 1 - k, draw 1 + k ; t_dev[:] = max(seq[k + 1], 0),
 *   k = *step_dev += 1 }, captured once in a hipGraph slot of its own like vdx_p_sample_loop (use_graph = 0: eagerly, the same launches).
 *   seq: device int32 [S + 1], the chain's levels descending then -1 (vdx_ddim_sample_loop's sequence; S = T: T-1 .. 0, -1).  On entry
 *   t_dev[:] = seq[0], *step_dev = 0, img = x_T; a loop may be issued in pieces.  post_scale / post_shift as in the step.
 * vdx_hybrid_loss: L = mean |eps_hat - eps|^p + w mean vb over all batch * per_sample elements (p = 2 when l2 else 1), vb in bits per
 *   element with eps_hat DETACHED inside it: with x0 = x pre_scale + pre_shift, x_t = sqrt_ac x0 + sqrt(1 - ac) noise formed in double (as
 *   vdx_vlb_terms does), x0^ unclipped, for t >= 1 vb = KL(N(mu~, beta~_t) || N(mu, sigma^2)) / ln 2 with
 *   KL = 0.5 (expm1(D) - D + (mu~ - mu)^2 e^{-log sigma^2}), D = log beta~_t - log sigma^2, and for t = 0 the discretized-Gaussian decoder
 *   term of vdx_vlb_terms (exact erfc, the same tail rules and 1e-12 floor) with sigma = exp(0.5 log sigma^2).  out [2 batch + 3] doubles:
 *   the per-sample means (mse_b, vb_b), then (mean mse, mean vb, L).  d_out (may be NULL: no gradient) [batch,F,H,W,2C] fp32 = dL/d out2:
 *   the eps_hat half is vdx_loss_grad's value bit for bit, the v half d vb / d log sigma^2 * 0.5 (max_log - min_log) * w / (N ln 2) with
 *   d KL / d log sigma^2 = 0.5 (1 - e^D - (mu~ - mu)^2 e^{-log sigma^2}) and, at t = 0, 0.5 (phi(z+) z+ - phi(z-) z-) / P (without the
 *   absent term on a tail, 0 where P is floored).  Everything in double, sums by the fixed-order scheme of vdx_vlb_terms: no atomics, no
 *   host read.  scratch: vdx_hybrid_scratch_doubles(batch) doubles.  Any per_sample that is a multiple of channels.
 * vdx_vlb_terms_lv / vdx_vlb_loop_lv: vdx_vlb_terms / vdx_vlb_loop (same arguments, rules, output triple and graph contract, a graph slot
 *   of its own) with the model's log sigma^2 in the KL and decoder terms: eps_hat = out2, vlb_tables = lv_tables64.
 * Refused before any launch (VDX_ERR_INVALID): a network whose out_dim is not 2 * channels ("out_dim must equal 2 * channels"), S outside
 * [1, timesteps] ("S must be in [1, timesteps]"). */
#define VDX_LV_ROWS 9
int vdx_p_sample_step_lv(const float* x, const float* out2, float* out, const int* level_dev, const float* lv_tables, int S, uint64_t step,
                         const uint64_t* step_dev, const float* noise, uint64_t seed, uint64_t offset, const uint64_t* dev_offset,
                         int clip_denoised, float post_scale, float post_shift, int batch, int channels, long per_sample, void* stream);
int vdx_p_sample_loop_lv(vdx_handle* h, const float* params, const void* packed, float* img, float* out2_buf, int* t_dev, uint64_t* step_dev,
                         const float* lv_tables, const int* seq, int S, int timesteps, int nsteps, const float* cond, uint64_t seed,
                         int clip_denoised, float post_scale, float post_shift, void* workspace, size_t workspace_bytes, int batch,
                         int use_graph, void* stream);
size_t vdx_hybrid_scratch_doubles(int batch);
int vdx_hybrid_loss(const float* x, const float* noise, const float* out2, const int* t, const double* lv_tables64, int timesteps,
                    float pre_scale, float pre_shift, int l2, double vlb_weight, int want_grad, float* d_out, double* scratch, double* out,
                    int batch, int channels, long per_sample, void* stream);
int vdx_vlb_terms_lv(const float* x, const float* out2, const int* t, const double* lv_tables64, int timesteps, const float* noise,
                     uint64_t seed, uint64_t draw, const uint64_t* step_dev, int clip_denoised, double* partial, double* out, int batch,
                     int channels, long per_sample, void* stream);
int vdx_vlb_loop_lv(vdx_handle* h, const float* params, const void* packed, const float* x, float* xt_buf, float* out2_buf, int* t_dev,
                    uint64_t* step_dev, const double* lv_tables64, int timesteps, const int* seq, int seq_len, int nsteps, const float* cond,
                    uint64_t seed, int clip_denoised, double* partial, double* out, void* workspace, size_t workspace_bytes, int batch,
                    int use_graph, void* stream);

/* Cascaded super-resolution (EXTENSION, parity unpinned: no reference code.  Ho et al. 2021, "Cascaded Diffusion Models"; the second
 * stage of Video Diffusion Models / Imagen Video).  Off unless these entries are called: the eleven loops above keep refusing a network
 * with out_dim != channels and perform the launches they always did.  The denoiser has channels = 2 C and out_dim = C; its input is
 *   xin [batch, 2C, F, S, S]:  planes [0, C) of each sample = x_t,  planes [C, 2C) = u = aug(up(2 lo - 1))
 * with lo [batch, C, F/ft, S/fs, S/fs] in [0, 1] the low-resolution clip (ft, fs >= 1 integers dividing F and S; (1, 1) = plain concat
 * conditioning).  up: separable linear interpolation in frames, rows and columns with half-pixel centres, src = (dst + 0.5) in / out - 0.5,
 * neighbours clamped at both edges (torch's interpolate(mode='trilinear', align_corners=False)); normalise first, then interpolate.
 * aug: noise conditioning augmentation, blind (the network is not told the level): per sample u = sqrt_ac[s_b] up + sqrt(1 - ac[s_b]) z
 * with z = Philox(seed, draw) over the element index of [batch, C, F, S, S] as vdx_randn lays it out; s_b < 0 (or aug_level NULL): u = up
 * exactly, nothing is drawn.  Levels above timesteps - 1 are read as timesteps - 1.
 *
 * vdx_lowres_down: lo = the box mean of x [batch, C, F, S, S] over ft x fs x fs blocks: an fp32 sum in (frame, row, column) order, then one
 *   multiply by 1 / n (ft = fs = 1: the bits of x).
 * vdx_lowres_input: one pass over both halves of xin.  x0 != NULL: planes [0, C) = sqrt_ac[t] (x0 pre_scale + pre_shift) + sqrt_1m_ac[t]
 *   noise, vdx_q_sample's expression and bits; x0 == NULL: only planes [C, 2C) are written (the sampling-time form; t / noise are not
 *   read).  Any S and per_sample, sample bases off 16 bytes included.
 * vdx_lowres_pack: xin[b, 0 : per_sample] = img[b, :] for img [batch, per_sample] and xin rows of pitch 2 per_sample; the second half
 *   of every row is not touched.  float4 where per_sample % 4 == 0 and both bases are 16-byte aligned, scalar otherwise.
 * vdx_p_sample_loop_sr / vdx_ddim_sample_loop_sr / vdx_dpm_sample_loop_sr: vdx_p_sample_loop_dyn / vdx_ddim_sample_loop_dyn /
 *   vdx_dpm_sample_loop (same arguments and contract) with xin after img: img / eps_buf / hist are over C = out_dim channels, the step is
 *   vdx_lowres_pack(img -> xin) -> forward on xin -> (dynamic threshold) -> the unchanged step kernel on img -> advance.  The caller fills
 *   planes [C, 2C) of xin once (vdx_lowres_input with x0 = NULL; draw VDX_DRAW_LOWRES of the chain's seed when augmented).  Graph slots
 *   of their own: no other loop's graph is evicted.
 * Refused before any launch: a NULL pointer, a network whose channels is not 2 * out_dim ("channels must equal 2 * out_dim"), img / xin
 *   off 16 bytes (VDX_ERR_INVALID); a handle created without a GPU (VDX_ERR_STATE). */
#define VDX_DRAW_LOWRES (1ull << 61)
int vdx_lowres_down(const float* x, float* lo, int batch, int channels, int frames, int size, int ft, int fs, void* stream);
int vdx_lowres_input(const float* x0, const int* t, const float* noise, const float* lo, const int* aug_level, float* xin, const float* sqrt_ac,
                     const float* sqrt_one_minus_ac, int timesteps, uint64_t seed, uint64_t draw, float pre_scale, float pre_shift, int batch,
                     int channels, int frames, int size, int ft, int fs, void* stream);
int vdx_lowres_pack(const float* img, float* xin, int batch, long per_sample, void* stream);
int vdx_p_sample_loop_sr(vdx_handle* h, const float* params, const void* packed, float* img, float* xin, float* eps_buf, int* t_dev,
                         uint64_t* step_dev, const float* tables, int timesteps, int nsteps, const float* cond, uint64_t seed,
                         int clip_denoised, float percentile, float* thres_buf, void* workspace, size_t workspace_bytes, int batch,
                         int use_graph, void* stream);
int vdx_ddim_sample_loop_sr(vdx_handle* h, const float* params, const void* packed, float* img, float* xin, float* eps_buf, int* t_dev,
                            uint64_t* step_dev, const float* alphas_cumprod, const int* seq, int seq_len, int nsteps, const float* cond,
                            int clip_denoised, const float* tables, int timesteps, float percentile, float* thres_buf, void* workspace,
                            size_t workspace_bytes, int batch, int use_graph, void* stream);
int vdx_dpm_sample_loop_sr(vdx_handle* h, const float* params, const void* packed, float* img, float* xin, float* eps_buf, float* hist,
                           int* t_dev, uint64_t* step_dev, const float* alphas_cumprod, const int* seq, int seq_len, int nsteps,
                           const float* cond, int clip_denoised, int order, const float* tables, int timesteps, float percentile,
                           float* thres_buf, void* workspace, size_t workspace_bytes, int batch, int use_graph, void* stream);

/* Loss-aware timestep sampling (EXTENSION, parity unpinned: no reference code.  Nichol & Dhariwal 2021, "Improved DDPM", section 3.3;
 * improved-diffusion's LossSecondMomentResampler, restated in fp64 in tests/_tsampler_ref.py).  Off unless these entries are called.
 * State (the caller's device memory): hist double [T][H], the last H = history losses seen at each of the T = timesteps levels (oldest
 * first), and count int32 [T], how many of a row's slots are filled.  Probabilities, with eps = uniform_prob:
 *   cold (any count[t] < H):  p_t = 1 / T
 *   warm:  w_t = sqrt((sum_j hist[t][j]^2) / H),  W = sum_t w_t,  p_t = (w_t / W)(1 - eps) + eps / T;  W zero or not finite: p_t = 1 / T
 * No atomics in any of these kernels and every sum in a fixed order: the bits of every output depend on the inputs only.
 *
 * vdx_tsampler_draw: one workgroup; w, p and the inclusive prefix sum of p in double in LDS (2 T doubles: the cap T <= 4096).  Sample b:
 *   r = Philox4x32-10(counter (b, 0, draw lo, draw hi), key (seed lo, seed hi)),  m = (r0 << 21) | (r1 >> 11),  u = (m + 0.5) 2^-53;
 *   cold: t = min(floor(u T), T - 1), iw = 1.0 exactly;  warm: t = the first index whose prefix sum exceeds u (binary search), at most
 *   T - 1, iw = 1 / (T p_t).  t_given (may be NULL) [batch]: nothing is drawn, t_out = t_given and iw is that of the current p (1.0 when
 *   cold; a level outside [0, T) reads the nearest one).  p_out (may be NULL) [T] receives p.  Any batch >= 1.
 *   Refused before any launch (VDX_ERR_INVALID): timesteps outside [1, 4096], history outside [1, 32], uniform_prob outside (0, 1],
 *   batch < 1.
 * vdx_tsampler_update: entries double [n][2] = (t, loss), applied as if one after the other in index order: an entry whose loss or level
 *   is not finite, or whose level is outside [0, T), is skipped; count[t] == H: the row moves left by one and the loss goes last;
 *   otherwise hist[t][count[t]++] = loss.  (One workgroup; the first entry of each level applies that level's entries in order.)
 * vdx_loss_weighted: the plain loss per sample and its importance-weighted gradient in ONE pass over eps_hat (channel-last [B,F,H,W,C])
 *   and noise ([B,C,F,H,W]): d = eps_hat - noise in fp32 as vdx_loss_sum / vdx_loss_grad form it, |d| (l2 == 0) or d^2 added in double
 *   through a fixed-order tree and an in-order final.  out [batch + 1] doubles: out[b] = l_b, the sample's mean, out[batch] =
 *   (1 / batch) sum_b iw_b l_b.  d_eps_hat (may be NULL) = l2 ? 2.0f d f_b : sign(d) f_b with f_b = (float)iw_b * inv_count, inv_count
 *   the float vdx_loss_grad uses: with iw NULL (all weights 1) or iw_b == 1 the gradient is vdx_loss_grad's bit for bit.  scratch:
 *   vdx_loss_weighted_scratch_doubles(batch) doubles.  Any channels * fhw.
 * vdx_hybrid_loss_w: vdx_hybrid_loss with importance weights iw [batch] (NULL: vdx_hybrid_loss bit for bit): the three totals
 *   out[2 batch ..] are (1 / batch) sum_b iw_b (.)_b and both halves of d_out carry iw_b -- formed in double and rounded to fp32 once
 *   where iw_b != 1, the unweighted expressions and bits where iw_b == 1; the per-sample pairs out[0 .. 2 batch) stay unweighted. */
int vdx_tsampler_draw(const double* hist, const int* count, int timesteps, int history, double uniform_prob, const int* t_given, uint64_t seed,
                      uint64_t draw, int* t_out, double* iw_out, double* p_out, int batch, void* stream);
int vdx_tsampler_update(double* hist, int* count, int timesteps, int history, const double* entries, int n, void* stream);
size_t vdx_loss_weighted_scratch_doubles(int batch);
int vdx_loss_weighted(const float* eps_hat, const float* noise, const double* iw, float* d_eps_hat, double* scratch, double* out, int batch,
                      int channels, long fhw, int l2, void* stream);
int vdx_hybrid_loss_w(const float* x, const float* noise, const float* out2, const int* t, const double* lv_tables64, int timesteps,
                      float pre_scale, float pre_shift, int l2, double vlb_weight, int want_grad, float* d_out, double* scratch, double* out,
                      int batch, int channels, long per_sample, const double* iw, void* stream);

/* Mixed noise (EXTENSION, parity unpinned: no reference code.  Ge et al. 2023, "Preserve Your Own Correlation", section 3.2, the mixed
 * noise model): a temporally correlated noise prior for video.  Off unless these entries are called.  Over a [batch,C,F,H,W] tensor
 *   z[b,c,f,h,w] = a s[b,c,h,w] + b e[b,c,f,h,w],   s, e ~ N(0, 1),   a = alpha / sqrt(1 + alpha^2),  b = 1 / sqrt(1 + alpha^2)
 * so each element is N(0, 1) and two frames of one clip correlate with rho = a^2 at the same pixel.  Draws: e is vdx_randn's element of
 * the [batch,C,F,H,W] tensor at draw d; s is the stream at draw VDX_DRAW_SHARED + d, indexed as vdx_randn would index a [batch,C,H,W]
 * tensor (flat index (b C + c) HW + hw, counter = index / 4, lane = index % 4).  d < 2^60: no draw of any entry above collides (0 .. T,
 * VDX_DRAW_LOWRES, VDX_DRAW_KNOWN + s, VDX_DRAW_RENOISE + s).  The two products and the sum are rounded to fp32 one by one (no fused
 * multiply-add), so z is a * S + b * E formed in fp32 from vdx_randn's two tensors, bit for bit.  Where HW % 4 == 0 one shared counter
 * serves four consecutive elements; elsewhere a quad may straddle frames or channels and takes up to four: the values are the same.
 *
 * vdx_randn_mixed: out [batch,channels,frames,hw] = z at draw `draw` (+ *dev_draw when given).  Any sizes >= 1.
 * vdx_p_sample_step_mixed: vdx_p_sample_step with z generated in the kernel at draw offset (+ *dev_offset): `frames, a, b` stand where
 *   `noise` stands there.  One fused kernel; the bits of vdx_p_sample_step(noise = vdx_randn_mixed(...)).  per_sample % 4 == 0 and
 *   % (channels * frames) == 0; x / out 16-byte aligned (they may alias).
 * vdx_p_sample_loop_mixed: vdx_p_sample_loop_guided's arguments plus a, b: the ancestral loop with vdx_p_sample_step_mixed's kernel as
 *   its step (draw 1 + k at step k; frames and H W are the handle's).  cond_scale == 1 or cfg_scratch NULL: the plain loop
 *   (vdx_p_sample_loop_dyn's buffers: `batch` rows; rescale is not read), otherwise the guided one (2 batch rows, as
 *   vdx_p_sample_loop_guided).  The dynamic threshold, the guidance combine and the advance are those loops'.  Two graph slots of its own
 *   (plain, guided): no other loop's graph is evicted.  There is no masked and no super-resolution form.
 * Refused before any launch (VDX_ERR_INVALID): a NULL tensor, a size < 1, a or b negative or not finite, |a^2 + b^2 - 1| > 1e-5, a draw
 *   (offset) >= 2^60; for the loop also what vdx_p_sample_loop_dyn / _guided refuse. */
#define VDX_DRAW_SHARED (1ull << 60)
int vdx_randn_mixed(float* out, int batch, int channels, int frames, long hw, float a, float b, uint64_t seed, uint64_t draw,
                    const uint64_t* dev_draw, void* stream);
int vdx_p_sample_step_mixed(const float* x, const float* eps_hat, float* out, const int* t, const float* tables, int timesteps,
                            int frames, float a, float b, uint64_t seed, uint64_t offset, const uint64_t* dev_offset, const float* thres,
                            int clip_denoised, int batch, int channels, long per_sample, void* stream);
int vdx_p_sample_loop_mixed(vdx_handle* h, const float* params, const void* packed, float* img, float* eps_buf, int* t_dev,
                            uint64_t* step_dev, const float* tables, int timesteps, int nsteps, const float* cond, uint64_t seed,
                            int clip_denoised, float percentile, float* thres_buf, float cond_scale, float rescale, double* cfg_scratch,
                            float a, float b, void* workspace, size_t workspace_bytes, int batch, int use_graph, void* stream);

/* v-prediction (EXTENSION, parity unpinned: no reference code.  Salimans & Ho 2022, "Progressive Distillation", appendix D; the loss
 * weights: Hang et al. 2023, min-SNR-gamma).  Off unless these entries are called.  The network predicts
 *   v = sqrt(ac_t) eps - sqrt(1 - ac_t) x0,   and exactly   eps = sqrt(ac_t) v + sqrt(1 - ac_t) x_t,   x0 = sqrt(ac_t) x_t - sqrt(1 - ac_t) v.
 * One conversion point: the network output is overwritten with eps_hat by one streaming launch directly behind the forward; every step
 * kernel, the dynamic threshold, vdx_cfg_combine and the bits/dim terms take eps_hat as they always did.  No atomics in these kernels and
 * every sum in a fixed order.
 *
 * vdx_v_to_eps: out [rows][F,H,W,C] (channel-last, the network's v_hat) is overwritten with eps_hat; x [rows][C,F,H,W] = x_t; t [rows]
 *   int32 (a level outside [0, timesteps) reads the nearest one).  Per element eps_hat = fl(fl(sa v) + fl(s1 x)) with sa = sqrt_ac[t_b],
 *   s1 = sqrt_1mac[t_b]: no fused multiply-add, so fp32 `sa * v + s1 * x` restates it bit for bit.  Fixed grid, four elements per thread,
 *   tails guarded: any per_sample that is a multiple of channels, any alignment (the float4 forms only where per_sample % 4 == 0 and
 *   the bases are 16-byte aligned).  Refused before any launch (VDX_ERR_INVALID): a NULL tensor, rows, channels, timesteps or
 *   per_sample < 1, per_sample % channels != 0.
 * vdx_v_loss: the loss of the network output `out` (channel-last [batch,F,H,W,C]) per sample, with a weight per level, and its gradient
 *   in ONE pass (vdx_loss_weighted's shape: per-workgroup partials in double, a fixed-order tree, an in-order final).
 *     kind 1: target = fl(fl(sa noise) - fl(s1 x0n)), x0n = fma(x0, pre_scale, pre_shift) as vdx_q_sample forms it (x0, noise [batch,C,F,H,W])
 *     kind 0: target = noise (x0, the tables and the pre_* are not read): min-SNR weighting of the eps objective
 *   d = out - target in fp32, |d| (l2 == 0) or d^2 added in double.  w_b = wtab[t_b] (double [timesteps]; NULL: 1), g_b = iw[b] w_b
 *   (iw double [batch]; NULL: 1).  result [batch + 1] doubles: result[b] = w_b (mean of sample b), result[batch] = (1 / batch) sum_b
 *   iw_b result[b].  d_out (may be NULL) = l2 ? 2.0f d f_b : sign(d) f_b with f_b = (float)g_b * inv_count, inv_count the float
 *   vdx_loss_grad uses: kind 0 with wtab NULL gives vdx_loss_weighted's result and gradient bit for bit.  t may be NULL with kind 0 and
 *   wtab NULL.  scratch: vdx_v_loss_scratch_doubles(batch) doubles.  Any channels * fhw.  Refused before any launch (VDX_ERR_INVALID):
 *   a kind other than 0 / 1, a NULL out / noise / scratch / result, kind 1 without x0 or a table, levels (kind 1 or wtab) without t or
 *   with timesteps < 1, a size < 1, doubles off 8 bytes.
 * vdx_set_prediction: what the handle's network predicts, for the loops: kind 0 = eps (always accepted; clears the tables), kind 1 = v
 *   with the caller's device tables sqrt_ac | sqrt_1mac [timesteps] floats (they must outlive the setting).  With kind 1 the step of
 *   every vdx_*_sample_loop* entry and of vdx_vlb_loop launches vdx_v_to_eps's kernel over the rows of the forward (2 batch under
 *   guidance, before vdx_cfg_combine: guidance and its rescale act on eps_hat) directly behind it, with x = img (xt_buf) and t = t_dev.
 *   kind and the two pointers are part of every loop's graph key: a change re-captures, no graph is evicted for it.  VDX_ERR_INVALID:
 *   another kind, kind 1 without a table or with timesteps < 1.  vdx_p_sample_loop_lv and vdx_vlb_loop_lv return VDX_ERR_STATE while
 *   kind 1 is set, before any launch.  Like the other handle settings it needs no GPU. */
int vdx_v_to_eps(float* out, const float* x, const int* t, const float* sqrt_ac, const float* sqrt_1mac, int timesteps, int rows, int channels,
                 long per_sample, void* stream);
size_t vdx_v_loss_scratch_doubles(int batch);
int vdx_v_loss(const float* out, const float* x0, const float* noise, const int* t, const float* sqrt_ac, const float* sqrt_1mac,
               const double* wtab, const double* iw, int timesteps, int kind, float pre_scale, float pre_shift, int l2, float* d_out,
               double* scratch, double* result, int batch, int channels, long fhw, void* stream);
int vdx_set_prediction(vdx_handle* h, int kind, const float* sqrt_ac, const float* sqrt_1mac, int timesteps);
int vdx_get_prediction(const vdx_handle* h);

/* Self-conditioning (EXTENSION, parity unpinned: no reference code.  Chen et al. 2022, "Analog Bits", section 2.2; used by Imagen Video
 * and RIN).  Off unless these entries are called.  The denoiser has channels = 2 C and out_dim = C, as a super-resolution one; its input is
 *   xin [batch, 2C, F, H, W]:  planes [0, C) of each sample = x_t,  planes [C, 2C) = x0~, the network's own previous estimate of x0
 * (zero where there is none: the first step of a chain, and the training steps whose coin says so).
 *
 * vdx_selfcond_x0: x0~ = clip(sqrt(1 / ac_t) x - sqrt(1 / ac_t - 1) eps_hat), written into planes [C, 2C) of xin (row pitch 2 per_sample;
 *   planes [0, C) are not touched).  x [batch][C,F,H,W] with sample b at x + b * x_pitch floats (x_pitch >= per_sample: img of a loop with
 *   x_pitch = per_sample, or xin itself with x_pitch = 2 per_sample); eps_hat channel-last [batch,F,H,W,C], dense; t [batch] int32 (a level
 *   outside [0, timesteps) reads the nearest one); tables: the [5][timesteps] step tables of vdx_p_sample_step, rows 0 and 1 are read;
 *   thres (may be NULL) [batch]: the dynamic threshold s of vdx_dynamic_threshold, NULL: s = 1.  Per element
 *     x0 = fl(fl(k_recip x) - fl(k_recipm1 eps_hat)),  and with clip_denoised  x0 = fminf(fmaxf(x0, -s), s) / s
 *   with no fused multiply-add, so fp32 torch restates it bit for bit.  Four consecutive elements per thread, tails guarded: any
 *   per_sample that is a multiple of channels, any channels, sample bases off 16 bytes (the float4 forms only where a whole quad's
 *   address allows them).  Refused before any launch (VDX_ERR_INVALID): a NULL x / eps_hat / t / tables / xin, batch, channels, timesteps
 *   or per_sample < 1, per_sample % channels != 0, x_pitch < per_sample, a tensor off 4 bytes.
 * vdx_set_self_condition: the handle's self-condition state, for the loops: on = 0 (always accepted; clears the table) or 1 with the
 *   caller's device step tables [5][timesteps] (they must outlive the setting).  With on = 1 the step of vdx_p_sample_loop_sr /
 *   vdx_ddim_sample_loop_sr / vdx_dpm_sample_loop_sr gains ONE launch, vdx_selfcond_x0's kernel with x = img, thres = the step's dynamic
 *   threshold (or NULL), clip = clip_denoised and the levels of t_dev, behind vdx_v_to_eps's and the threshold's and in front of the
 *   chain's step kernel: the next step's forward reads it.  The caller zeroes planes [C, 2C) of xin before the first step.  The state
 *   (on, the pointer, timesteps) is part of every loop's graph key: a change re-captures, no graph is evicted for it.  While it is on,
 *   every loop entry without xin, vdx_p_sample_loop_lv, vdx_vlb_loop and vdx_vlb_loop_lv return VDX_ERR_STATE before any launch.
 *   VDX_ERR_INVALID: on other than 0 / 1, on = 1 without tables or with timesteps < 1.  Like the other handle settings it needs no GPU. */
int vdx_selfcond_x0(const float* x, long x_pitch, const float* eps_hat, const int* t, const float* tables, int timesteps, const float* thres,
                    int clip_denoised, float* xin, int batch, int channels, long per_sample, void* stream);
int vdx_set_self_condition(vdx_handle* h, int on, const float* tables, int timesteps);
int vdx_get_self_condition(const vdx_handle* h);

/* ------------------------------------------------------------------------------------------------
 * Backward building blocks (autodiff of the forward operators; reference trainer.py:361 jax.value_and_grad).
 * ---------------------------------------------------------------------------------------------- */

/* Transposed, tap-reversed packing [taps][Cin][CoutPad]: vdx_conv_forward(dy, this packing, cout = Cin) is the data
 * gradient of a stride-1 conv; with kind swapped (Conv 4x4/s2 <-> ConvTranspose) it is the data gradient of
 * Downsample / Upsample.  Size: vdx_packed_conv_bytes(mode, taps, cout, cin). */
int vdx_pack_conv_weights_t(int mode, const float* kernel, void* packed, int taps, int cin, int cout, void* stream);

typedef struct {
    const float* x0; const float* x1; int c0, c1;      /* the conv's input (concat on channels) */
    const float* dy; int cout;                         /* gradient of the conv's output [B*F, Ho, Wo, cout] */
    float* dw;                                         /* Flax layout [taps][c0+c1][cout] fp32, ACCUMULATED (atomics) */
    int batch, frames, h, w;                           /* input geometry */
    int kind, kh, kw, stride;                          /* as vdx_conv_desc */
    const double* in_stats; const float* gamma; const float* beta; int groups;     /* optional fused prologue of the forward */
    const float* scale_shift; int scale_shift_stride;
    int bf16_operands;                                 /* 0: exact-f32 MFMA; 1: operands rounded to bf16, fp32 accumulate (what a
                                                          VDX_MODE_BF16 handle's backward uses) */
} vdx_wgrad_desc;

/* dW += Xhat^T (*) dY on exact-f32 MFMA (both arithmetic modes use it).  This block-level entry point has no workspace and accumulates with
 * float atomics (the result is reproducible to rounding); inside vdx_unet_backward the same kernels store per-workgroup partial tiles
 * into the backward workspace and a second pass adds them in a fixed order (bit-reproducible gradients, round 3). */
int vdx_conv_backward_weights(const vdx_wgrad_desc* d, void* stream);

/* Backward of act = SiLU((gamma*GroupNorm(y)+beta)*(1+s)+sh) and, when r != NULL, of out = act + LayerNorm_C(r)
 * (reference forward: modules.py:171-179,233-243).  dact/y/dy/r/dr channel-last [batch, pix_per_sample, c];
 * stats = the forward's GroupNorm statistics slab; scale_shift rows [s(c)|sh(c)] or NULL; d_gamma/d_beta/d_ln_* are
 * ACCUMULATED; dss [batch][2c] (ds|dsh) written when non-NULL; scratch >= vdx_norm_act_backward_scratch_floats(c, batch,
 * pix_per_sample) floats, uninitialised (per-workgroup partial sums of the reduction pass + the per-group terms). */
size_t vdx_norm_act_backward_scratch_floats(int c, int batch, long pix_per_sample);
int vdx_norm_act_backward(const float* dact, const float* y, float* dy, const double* stats, const float* gamma, const float* beta,
                          int groups, const float* scale_shift, int scale_shift_stride, float* d_gamma, float* d_beta, float* dss,
                          const float* r, const float* ln_gamma, float* dr, float* d_ln_gamma, float* d_ln_beta, float* scratch,
                          int c, int batch, long pix_per_sample, void* stream);

/* Attention core backward (autodiff of modules.py:294-323 per sequence and head).  qkv [npix][3*heads*32] = x Wqkv + b
 * (q unscaled), d_o [npix][heads*32] = dy Wo^T; writes o (attention output before the out projection), dq, dk, dv
 * [npix][heads*32].  temporal != 0: sequences over F per (b,h,w), else over (h w) per (b,f).
 * Lengths: up to 64 tokens per sequence in both directions.  Spatial sequences (temporal == 0) are also served at every multiple of 64
 * up to 640 tokens (the limit of the forward core): a tiled exact-fp32 core on the matrix cores, three launches
 * (attn_long_bwd_stats / dkv / dq_kernel) without scratch -- between them the three softmax scalars of a row travel in the first
 * columns of the row's own dq slot, which the last launch overwrites with dq -- no float atomics, bit-reproducible.  Any other h*w above
 * 64, and temporal != 0 with more than 64 frames, is VDX_ERR_INVALID with nothing launched. */
int vdx_attention_core_backward(const float* qkv, const float* d_o, float* o, float* dq, float* dk, float* dv, int batch, int frames,
                                int h, int w, int heads, int temporal, void* stream);
/* Same with a choice of arithmetic: bf16_operands != 0 = the form a VDX_MODE_BF16 handle's backward uses for sequences of <= 16
 * tokens (q, k, v, d_o rounded to bf16, every product on MFMA, fp32 accumulate); 0 = exact fp32.  Above 16 tokens the flag is accepted
 * and ignored: those cores (17..64 tokens, and the tiled one above 64) compute in fp32 in every mode. */
int vdx_attention_core_backward_ex(const float* qkv, const float* d_o, float* o, float* dq, float* dk, float* dv, int batch, int frames,
                                   int h, int w, int heads, int temporal, int bf16_operands, void* stream);

/* Whole backward of a temporal attention block y = MHA(x) + x (modules.py:271-327 under Residual, unet3d.py:284,308,365) except its
 * weight gradients, in one pass over x and dy: the shape a VDX_MODE_BF16 handle's backward runs at the widest level (C = 64 channels,
 * 8 heads x 32, sequences over <= 16 frames per (b, h, w); bf16 operands, fp32 accumulate).  x, dy, dx: fp32 [B][F][h][w][64];
 * packed_wqkv = vdx_pack_conv_weights(BF16) of the [64][q|k|v = 768] kernel, bqkv [768]; packed_wo_t =
 * vdx_pack_conv_weights_t(BF16) of the [256][64] out kernel.  Writes dx = dy + d(q|k|v) Wqkv^T and, as bf16 tensors for the
 * weight-gradient kernels, o [rows][256] (attention output before the out projection) and dqkv [rows][768]. */
int vdx_temporal_attention_backward_fused(const float* x, const float* dy, const void* packed_wqkv, const float* bqkv, const void* packed_wo_t,
                                          void* o_bf16, void* dqkv_bf16, float* dx, int batch, int frames, int h, int w, void* stream);

/* SpatialLinearAttention core backward (autodiff of modules.py:105-118 per frame and head; heads = 8, D = 32).
 * q, k, v, d_out [B*F*h*w][256]; writes o (pre to_out), dq, dk, dv.  scratch >= vdx_sla_backward_scratch_floats floats. */
size_t vdx_sla_backward_scratch_floats(int nframes, int heads);
int vdx_sla_core_backward(const float* q, const float* k, const float* v, const float* d_out, float* o, float* dq, float* dk, float* dv,
                          float* scratch, int nframes, int npix, int heads, void* stream);
/* Same with a choice of arithmetic for the per-(frame, head) reductions (softmax-over-pixels statistics, ctx, dctx):
 * bf16_operands != 0 = bf16 MFMA with fp32 accumulate (what a VDX_MODE_BF16 handle's backward uses); 0 = exact fp32. */
int vdx_sla_core_backward_ex(const float* q, const float* k, const float* v, const float* d_out, float* o, float* dq, float* dk, float* dv,
                             float* scratch, int nframes, int npix, int heads, int bf16_operands, void* stream);

/* out[c] += sum_rows x[row][c]  (bias gradients). */
int vdx_colsum(const float* x, float* out, long rows, int c, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Backward forms of the network (test-facing).  vdx_unet_backward sets flags on the launchers that the block-level entry points
 * above never set: bf16 TENSORS (not only bf16 operands), the q|k|v split epilogue, fused bias sums, per-workgroup slots with a
 * fixed-order second pass, interleaved [rows][dq|dk|dv] outputs, row slices of a transposed packing.  The functions below fill the
 * launchers' argument structs the way model_bwd.hip does and call the same launchers, so that each of those kernel forms can be
 * compared with a reference on its own (tests/test_gpu_backward_forms.py).  No kernel is specific to them.
 * ---------------------------------------------------------------------------------------------- */

/* Weight gradient as model_bwd.hip's wgrad() (:102-117), wgrad1x1() (:179-190) and wgrad1x1_qkv() (:193-206) launch it.
 * Served forms (anything else is VDX_ERR_INVALID): 1x1 and 3x3 at stride 1, 4x4 at stride 2, kind 1; the prologue only with 3x3 and no
 * split; split only with 1x1.
 *   x_bf16 / dy_bf16: x0 (and x1) / dy hold bf16 elements (bf16_operands only; channel counts multiples of 8).  wgrad() passes
 *     x_bf16 = activation storage (block inputs) or 1 (the prologue form reading y1), dy_bf16 = 1 in bf16 mode;
 *   split > 0 (a multiple of 64 dividing cout into <= 3 blocks): column block co / split of dy goes to (dw, dw1, dw2), each
 *     [taps][c0+c1][split], and to (db, db1, db2) -- the q|k|v launch (split = heads * 32);
 *   db (db1, db2): bias gradient(s) [cout] (or [split]) accumulated in the same pass, or NULL;
 *   scratch / scratch_floats: per-workgroup slots (wgrad(): vdx_wgrad_scratch_floats()).  When the launch's slots fit, every
 *     workgroup stores its partial tile and a second pass adds the slots in a fixed order: two runs are bit-identical.  When they do
 *     not fit (or scratch is NULL) the kernels add with float atomics.  Either way the outputs are ACCUMULATED into. */
typedef struct {
    const void* x0; const void* x1; int c0, c1; int x_bf16;
    const void* dy; int cout; int dy_bf16;
    float* dw; float* dw1; float* dw2; int split;
    float* db; float* db1; float* db2;
    int batch, frames, h, w;
    int kind, kh, kw, stride;
    const double* in_stats; const float* gamma; const float* beta; int groups;
    const float* scale_shift; int scale_shift_stride;
    int bf16_operands;
    float* scratch; size_t scratch_floats;
} vdx_wgrad_ex_desc;
int vdx_conv_backward_weights_ex(const vdx_wgrad_ex_desc* d, void* stream);
/* Floats of slot scratch vdx_unet_backward hands every weight gradient (per stream): tests pass the same size, so that a launch
 * takes the slot or the atomic path exactly where the network's does. */
size_t vdx_wgrad_scratch_floats(void);

/* The fixed-order second pass on its own (launch_slot_sum): d[e'] += sum over k < nslots, in order, of part[k * slot_stride + e],
 * e < e_count.  split == 0: d0[e].  split > 0: e = row * cout + co goes to (d0, d1, d2)[co / split][row * split + co % split].
 * nslots >= 32 runs slot_sum16_kernel (16 lanes per element), fewer slot_sum_kernel. */
int vdx_slot_sum(const float* part, int nslots, size_t slot_stride, long e_count, int cout, int split, float* d0, float* d1, float* d2,
                 void* stream);

/* vdx_norm_act_backward with the tensor types and the deterministic parameter-gradient path of model_bwd.hip's res_bwd() (:128-137
 * tail, :144-151 prologue): y_bf16 / r_bf16 = y / r hold bf16, dy_bf16 = dy is WRITTEN as bf16 (one rounding of the fp32 result);
 * dact, dr stay fp32.  dgp: NULL (parameter gradients by float atomics) or scratch [batch][4][c] floats, uninitialised: the
 * per-sample rows are stored there and added in sample order -- two runs are bit-identical.  scratch as vdx_norm_act_backward:
 * uninitialised in every mode (the reduce pass stores each workgroup's row, nothing accumulates into it; the network keeps it at a
 * fixed offset of its workspace for the same reason). */
int vdx_norm_act_backward_ex(const float* dact, const void* y, int y_bf16, void* dy, int dy_bf16, const double* stats, const float* gamma,
                             const float* beta, int groups, const float* scale_shift, int scale_shift_stride, float* d_gamma, float* d_beta,
                             float* dss, const void* r, int r_bf16, const float* ln_gamma, float* dr, float* d_ln_gamma, float* d_ln_beta,
                             float* scratch, float* dgp, int c, int batch, long pix_per_sample, void* stream);

/* vdx_attention_core_backward_ex as attn_bwd() launches it (model_bwd.hip:234-243): ONE output buffer dqkv [rows][dq|dk|dv] with
 * dstride = 3 * heads * 32 in the network (a wider row, a multiple of 8, leaves the columns behind dq|dk|dv untouched; dk / dv start
 * heads*32 / 2*heads*32 elements into the row, in the buffer's own element size); io_bf16:
 * qkv, d_o, o, dqkv hold bf16.  bf16 tensors exist for the bf16 MFMA kernel only: io_bf16 without bf16_operands, or with more than
 * 16 tokens per sequence, is VDX_ERR_INVALID.  Lengths as vdx_attention_core_backward: above 64 tokens only spatial sequences of a
 * multiple of 64 up to 640 tokens, fp32 tensors. */
int vdx_attention_core_backward_io(const void* qkv, const void* d_o, void* o, void* dqkv, int dstride, int io_bf16, int batch, int frames,
                                   int h, int w, int heads, int temporal, int bf16_operands, void* stream);

/* vdx_attention_core_backward_io with the pre-softmax bias of vdx_attention_forward_bias: logits = q_i . k_j / sqrt(d) + bias[h][i][j]
 * (bias device fp32 [heads][L][L]); besides o and dqkv it ADDS dBias[h][i][j] = sum over the sequences of dS[h][i][j] into dbias
 * (fp32 [heads][L][L]; the caller zeroes it).  Deterministic: a fixed grid of workgroups stores per-workgroup sums into `scratch`
 * (scratch_floats >= vdx_attention_bias_backward_scratch_floats(heads, L)) and a second pass adds them in order -- no float atomics.
 * At most 64 tokens per sequence (this form and the focus form below): more is VDX_ERR_INVALID. */
size_t vdx_attention_bias_backward_scratch_floats(int heads, int tokens);
int vdx_attention_core_backward_bias(const void* qkv, const void* d_o, void* o, void* dqkv, int dstride, int io_bf16, const float* bias,
                                     float* dbias, float* scratch, size_t scratch_floats, int batch, int frames, int h, int w, int heads,
                                     int temporal, int bf16_operands, void* stream);

/* vdx_attention_core_backward_bias with the focus-present mask of vdx_attention_forward_focus on the recomputed probabilities.  For a masked
 * sample, exactly: dq == dk == 0, dv == dO, o == v, and a contribution of 0 to dbias.  bias_or_null / dbias_or_null come together; without
 * them scratch may be null. */
int vdx_attention_core_backward_focus(const void* qkv, const void* d_o, void* o, void* dqkv, int dstride, int io_bf16, const float* bias_or_null,
                                      float* dbias_or_null, float* scratch, size_t scratch_floats, const unsigned char* focus_dev, int focus_n,
                                      int batch, int frames, int h, int w, int heads, int temporal, int bf16_operands, void* stream);

/* vdx_temporal_attention_backward_fused with x_bf16 (model_bwd.hip:219-227 under bf16 activation storage): x holds bf16. */
int vdx_temporal_attention_backward_fused_ex(const void* x, int x_bf16, const float* dy, const void* packed_wqkv, const float* bqkv,
                                             const void* packed_wo_t, void* o_bf16, void* dqkv_bf16, float* dx, int batch, int frames, int h,
                                             int w, void* stream);

/* vdx_sla_core_backward_ex as sla_bwd() launches it (model_bwd.hip:261-268): one dqkv [rows][dq|dk|dv] buffer, dstride = 768 (or wider);
 * io_bf16: q, k, v, d_out, o, dqkv hold bf16 (bf16_operands only). */
int vdx_sla_core_backward_io(const void* q, const void* k, const void* v, const void* d_out, void* o, void* dqkv, int dstride, int io_bf16,
                             float* scratch, int nframes, int npix, int heads, int bf16_operands, void* stream);

/* vdx_conv_forward reading rows [w_row0, w_row0 + cout) of a packing with w_rows rows per tap: the data gradient of one half of a
 * concat input from the transposed packing of the whole kernel (model_bwd.hip dgrad() :89-100, res_bwd() :156-160), usually with
 * d->res.  Multiples of 4. */
int vdx_conv_forward_rows(int mode, const vdx_conv_desc* d, int w_rows, int w_row0, void* stream);

/* Backward of vdx_final_conv (model_bwd.hip:392): dx [npix][d] written; dw [d][cout], db [cout] ACCUMULATED.  x_bf16: x holds bf16.
 * d a multiple of 4, <= 256; cout <= 4.  scratch: optional slots for the fixed-order sums (atomics when NULL or too small). */
int vdx_final_conv_backward(const void* x, int x_bf16, const float* d_out, const float* kernel, float* dx, float* dw, float* db, long npix, int d,
                            int cout, float* scratch, size_t scratch_floats, void* stream);
/* The same launches as the network makes them for the eps | v head of a learned-variance network: cout up to 6 (cout <= 4 writes
 * vdx_final_conv_backward's bits). */
int vdx_final_conv_backward_wide(const void* x, int x_bf16, const float* d_out, const float* kernel, float* dx, float* dw, float* db, long npix,
                                 int d, int cout, float* scratch, size_t scratch_floats, void* stream);

/* Weight and bias gradient of vdx_init_conv (model_bwd.hip:465): x external [B,Cin,F,H,W], dy channel-last [B,F,H,W,Cout];
 * dw Flax (k,k,Cin,Cout), db [Cout] ACCUMULATED.  scratch as above. */
int vdx_init_conv_backward_weights(const float* x, const float* dy, float* dw, float* db, int batch, int cin, int frames, int h, int w, int cout,
                                   int k, float* scratch, size_t scratch_floats, void* stream);

/* Backward of vdx_time_mlp (model_bwd.hip:456-461): dtemb [batch][4*dim + cond_dim]; dw1 [dim][4 dim], db1, dw2 [4 dim][4 dim], db2 and
 * dnull [cond_dim] (rows whose sample used null_cond_emb: cond_mask, else null_all) are ACCUMULATED. */
int vdx_time_mlp_backward(const int* time, const float* w1, const float* b1, const float* w2, const float* b2, int dim, const unsigned char* cond_mask,
                          int null_all, int cond_dim, const float* dtemb, float* dw1, float* db1, float* dw2, float* db2, float* dnull, int batch,
                          void* stream);

/* Backward of vdx_resblock_scale_shift as model_bwd.hip's ss_bwd() launches it (launch_resblock_ss_bwd: the LayerNorm backward per
 * (layer, sample), then the Linear's, then the fixed-order sum of the per-layer d(temb) slots).  The layer table is the forward's;
 * grads is laid out like params, lin and dss like the forward's lin / ss (layer l, sample b at [out_off * batch + b * n, + n); n <= 2048).
 * dss holds d(scale|shift) on entry and d(lin) on return.  dW, db, d gamma, d beta of every listed layer (in grads) and
 * dtemb [batch][temb_dim] are ACCUMULATED: one add per element and call.  slots / slots_cap: scratch of at least
 * nlayers * batch * temb_dim floats, uninitialised, for the per-layer d(temb) contributions (added in table order: two runs are
 * bit-identical); NULL with 0, or a capacity below that, adds them with float atomics instead.  nlayers >= 8 gives a workgroup 8 rows of
 * the Linear, fewer layers 1 (the staged backward passes 2 layers per call). */
int vdx_resblock_scale_shift_backward(const float* params, float* grads, const float* temb, const vdx_ss_layer* layers_dev, int nlayers,
                                      const float* lin, float* dss, float* dtemb, int temb_dim, int batch, float* slots, size_t slots_cap,
                                      void* stream);

/* ------------------------------------------------------------------------------------------------
 * Train step (reference trainer.py:322-392).
 * ---------------------------------------------------------------------------------------------- */

/* Unet3D backward (jax.value_and_grad of unet3d.py:262-387, reference trainer.py:361).  Must follow a vdx_unet_forward of the
 * same inputs on the same fwd_workspace (every intermediate is read back from its slot).  The reverse walk is cut in
 * vdx_num_stages() stages (head = num_stages-1, ups, mid, downs, stem = 0) so that the caller can all-reduce finished
 * gradient buckets while earlier stages still run: call with descending, contiguous [stage_hi .. stage_lo] ranges, starting
 * at the head (which zeroes `grads`).  grads: flat fp32, same layout as params (vdx_param_info).
 * packed_t: vdx_pack_params_bwd (transposed packing for the data gradients).
 * The gradients are bit-reproducible run to run (round 3): no sum of the pass depends on the arrival order of workgroups or of the
 * two streams it runs on (per-workgroup partial slots in bwd_workspace + a fixed-order second pass; vdx_bwd_workspace_bytes includes
 * 2 x 48 MB for them).
 * Sizes: at most 64 frames; the bottleneck (image_size >> (levels - 1), squared, tokens per frame) either has at most 64 tokens or a
 * multiple of 64 up to 640 (sides 16 and 24: e.g. 128 x 128 frames with four levels).  Any other bottleneck above 64 tokens (96 x 96
 * frames -> 144) is VDX_ERR_INVALID before anything is launched.  The tiled core needs no room in bwd_workspace (see
 * vdx_attention_core_backward), so a one-level network whose only level has such a token count is served as well. */
int vdx_num_stages(const vdx_handle* h);
size_t vdx_packed_bwd_bytes(const vdx_handle* h);
int vdx_pack_params_bwd(const vdx_handle* h, const float* params, void* packed_t, void* stream);
size_t vdx_bwd_workspace_bytes(const vdx_handle* h, int batch);
int vdx_unet_backward(vdx_handle* h, const float* params, const void* packed, const void* packed_t, const float* x, const int* time,
                      const float* cond, const unsigned char* cond_mask, int null_all, const float* d_out, void* fwd_workspace,
                      void* bwd_workspace, size_t bwd_workspace_bytes, float* grads, int stage_hi, int stage_lo, int batch, void* stream);

/* d(mean loss)/d(eps_hat) for the l1 / l2 loss of gaussian_diffusion.py:463-466, written channel-last like eps_hat. */
int vdx_loss_grad(const float* eps_hat, const float* noise, float* d_eps_hat, int batch, int channels, long fhw, int l2, void* stream);

/* Frame-conditioned training (EXTENSION: RaMViD, Hoeppe et al. 2022, "Diffusion Models for Video Prediction and Infilling"; the
 * reference trains unconditionally only).  A random subset of frames enters the network clean, the rest noised to level t, and the
 * loss is taken over the noised elements.  mask is inpaint's: [B,C,F,H,W] bytes in the layout of x / noise, nonzero = known (clean
 * context), zero = noised and learned from.  The kernels move 4 elements at a time: channels * fhw (per_sample) % 4 == 0, the
 * [B,C,F,H,W] float tensors 16-byte aligned, mask 4-byte aligned (checked: VDX_ERR_INVALID).
 *
 * vdx_q_sample_masked: out = mask ? x0n : sqrt_ac[t] x0n + sqrt_1m_ac[t] noise, x0n = x_start * pre_scale + pre_shift.  The noised
 * branch is vdx_q_sample's expression: an all-zero mask is vdx_q_sample bit for bit. */
int vdx_q_sample_masked(const float* x_start, const int* t, const float* noise, const unsigned char* mask, float* out, const float* sqrt_ac,
                        const float* sqrt_one_minus_ac, int batch, long per_sample, float pre_scale, float pre_shift, void* stream);

/* out[0] = sum of |eps_hat - noise| (l2 == 0) or (eps_hat - noise)^2 over the elements whose mask is 0, out[1] = their number (device
 * doubles; the loss is out[0] / max(out[1], 1)).  eps_hat channel-last [B,F,H,W,C] as in vdx_loss_sum; noise, mask [B,C,F,H,W].
 * Deterministic: a fixed grid writes one (sum, count) partial per workgroup into scratch[vdx_loss_masked_scratch_doubles()], a second
 * one-workgroup kernel adds them in index order (the scheme of vdx_grad_sqnorm); no atomics, the bits of out depend on the inputs only.
 * out needs no zeroing. */
size_t vdx_loss_masked_scratch_doubles(void);
int vdx_loss_sum_masked(const float* eps_hat, const float* noise, const unsigned char* mask, double* scratch, double* out, int batch,
                        int channels, long fhw, int l2, void* stream);

/* d(out[0] / max(out[1], 1))/d(eps_hat) of vdx_loss_sum_masked, written channel-last like eps_hat: exactly 0.0f where the mask is
 * nonzero.  count_dev = &out[1] on the device: the host reads nothing, the train step stays free of host syncs.  The factor is the
 * correctly rounded 1.0f / (float)count, so with an all-zero mask (count = batch * channels * fhw) the result is vdx_loss_grad's
 * bit for bit. */
int vdx_loss_grad_masked(const float* eps_hat, const float* noise, const unsigned char* mask, const double* count_dev, float* d_eps_hat,
                         int batch, int channels, long fhw, int l2, void* stream);

/* optax.adam + EMA on flat fp32 buffers (trainer.py:367-382): m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
 * p -= lr * (m / (1-b1^t)) / (sqrt(v / (1-b2^t)) + eps), t = step_count + 1; g is read as grad * grad_scale
 * (1/world_size after a sum all-reduce).  If do_ema: ema = decay * ema + (1 - decay) * p_new. */
int vdx_adam_ema_step(float* params, const float* grads, float* m, float* v, float* ema, long n, float lr, float b1, float b2,
                      float eps, long step_count, float grad_scale, int do_ema, float ema_decay, void* stream);

/* Gradient accumulation and global-norm clipping on the flat gradient buffer (the reference documents gradient_accumulate_every and
 * max_grad_norm, trainer.py:65,71, and ships clip_grad_norm, utils.py:127-152, without calling either).  All tensors are the caller's,
 * all work goes on `stream`, nothing synchronises, and no float is added atomically: every result is a function of its inputs only.
 *
 * vdx_grad_accumulate: acc[i] += g[i], i < n.  Called on bucket sub-ranges of the flat buffers, so acc and g may each sit on any
 * 4-byte boundary (also two different ones) and n >= 1 is arbitrary. */
int vdx_grad_accumulate(float* acc, const float* g, long n, void* stream);

/* *out = sum_i (double)g[i]^2 (a float squared is exact in double; no underflow, no float overflow).  A fixed grid writes one
 * partial per workgroup into scratch[vdx_grad_sqnorm_scratch_doubles()], a second one-workgroup kernel adds them in index order: the
 * bits of *out depend on (g's values, n) only -- not on the device, on g's alignment or on the run.  g: any 4-byte boundary. */
size_t vdx_grad_sqnorm_scratch_doubles(void);
int vdx_grad_sqnorm(const float* g, long n, double* scratch, double* out, void* stream);

/* vdx_adam_ema_step behind clip_grad_norm of the averaged gradient grad_scale * g.  From *sqnorm = sum g^2 (device,
 * vdx_grad_sqnorm) every thread derives, in double,
 *     l2 = sqrt(grad_scale^2 * *sqnorm + 1e-6);  clip = min(max_grad_norm / (l2 + 1e-6), 1);  s = (float)(grad_scale * clip)
 * and runs vdx_adam_ema_step's arithmetic with g * s in place of g * grad_scale (clip == 1: bit-identical results).
 * max_grad_norm > 0; FLT_MAX = no clipping, only the norm.  norm_out (device float, may be NULL) receives l2, the pre-clip norm. */
int vdx_adam_ema_step_clip(float* params, const float* grads, float* m, float* v, float* ema, long n, float lr, float b1, float b2,
                           float eps, long step_count, float grad_scale, int do_ema, float ema_decay, const double* sqnorm,
                           float max_grad_norm, float* norm_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Data-parallel communicator (reference trainer.py:161-177, 307-320: the batch is sharded over a 'data' mesh axis and XLA inserts
 * the all-reduce of every gradient behind jax.value_and_grad, trainer.py:361 -- SURVEY section 2, collective C1).  Here: one
 * process per GPU, one RCCL communicator per handle, the flat gradient buffer reduced bucket by bucket as the staged backward
 * finishes them.  RCCL is loaded at run time on the first call (no link-time dependency).
 * ---------------------------------------------------------------------------------------------- */
#define VDX_UNIQUE_ID_BYTES 128

/* rank 0 creates the rendezvous id (ncclGetUniqueId) and hands its 128 bytes to the other ranks through any channel it has (a
 * torch.distributed broadcast, a file, MPI); host memory. */
int vdx_comm_unique_id(void* unique_id_out);
/* joins the communicator of `world` ranks as `rank` on the CURRENT device (collective: every rank calls it). */
int vdx_comm_init(vdx_handle* h, int rank, int world, const void* unique_id);
/* in-place SUM all-reduce of count floats (a bucket of the flat gradient buffer) enqueued on `stream`; the mean's 1/world is folded
 * into vdx_adam_ema_step's grad_scale. */
int vdx_allreduce_bucket(vdx_handle* h, float* ptr, size_t count, void* stream);
int vdx_comm_world(const vdx_handle* h);         /* ranks of the handle's communicator, 1 when none */
int vdx_comm_destroy(vdx_handle* h);             /* also done by vdx_destroy */

#ifdef __cplusplus
}
#endif
#endif /* VDX_H_ */
