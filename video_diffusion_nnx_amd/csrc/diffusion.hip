// GaussianDiffusion device work (gfx950): HBM-bound elementwise kernels + the sampling loop driver.
//
//   randn ............ counter-based N(0,1) stream (Philox4x32-10 + Box-Muller), replaces jax.random.normal
//                      (gaussian_diffusion.py:254,309,416,445); restated for parity in oracle/philox_ref.py
//   q_sample ......... sqrt(ac_t) x0 + sqrt(1-ac_t) eps                         gaussian_diffusion.py:401-420
//   p_sample_step .... eps_hat -> x0_hat -> clip -> posterior mean -> + sigma z   gaussian_diffusion.py:120-159,162-261
//   loss ............. mean |eps_hat - eps| or (eps_hat - eps)^2                 gaussian_diffusion.py:460-468
//   p_sample_loop .... T x { Unet3D forward ; p_sample_step ; t -= 1 } on one stream, the step captured once
//                      in a hipGraph and replayed (no host work per step)      gaussian_diffusion.py:264-320
//   vlb_* ............ held-out evaluation (extension): x_t, then the terms of the variational bound in bits/dim as deterministic
//                      per-sample sums; the loop is vdx_vlb_loop in vdx_api.cpp
// External tensors are [B,C,F,H,W]; the UNet output eps_hat is channel-last [B,F,H,W,C] (unet3d.py:387) and is
// re-indexed on the fly (the reference's rearrange at gaussian_diffusion.py:197,460).
#include "vdx_common.h"
#include "vdx_internal.h"
#include "model.h"
#include "vdx_philox.h"
#include "vdx_pstep.h"

namespace vdx {

__global__ __launch_bounds__(256) void randn_kernel(float* __restrict__ out, long n, unsigned long long seed,
                                                    unsigned long long offset, const unsigned long long* __restrict__ dev_offset) {
    if (dev_offset) offset += *dev_offset;
    const long nq = (n + 3) / 4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += (long)gridDim.x * blockDim.x) {
        const float4 z = randn4((unsigned long long)i, seed, offset);
        if (4 * i + 3 < n) *reinterpret_cast<float4*>(out + 4 * i) = z;
        else { const float v[4] = {z.x, z.y, z.z, z.w}; for (int k = 0; 4 * i + k < n; ++k) out[4 * i + k] = v[k]; }
    }
}

// x_t = a[t_b] * (x0 * pre_scale + pre_shift) + b[t_b] * noise     (pre_* = normalize_img of __call__, :499)
__global__ __launch_bounds__(256) void q_sample_kernel(const float* __restrict__ x0, const int* __restrict__ t,
                                                       const float* __restrict__ noise, float* __restrict__ out,
                                                       const float* __restrict__ sqrt_ac, const float* __restrict__ sqrt_1mac,
                                                       long per_sample, float pre_scale, float pre_shift) {
    const int b = blockIdx.y;
    const float a = sqrt_ac[t[b]], s = sqrt_1mac[t[b]];
    const size_t base = (size_t)b * per_sample;
    for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < per_sample; i += (long)gridDim.x * blockDim.x * 4) {
        if (i + 3 < per_sample) {
            const float4 x = *reinterpret_cast<const float4*>(x0 + base + i);
            const float4 n = *reinterpret_cast<const float4*>(noise + base + i);
            float4 o;
            o.x = a * fmaf(x.x, pre_scale, pre_shift) + s * n.x; o.y = a * fmaf(x.y, pre_scale, pre_shift) + s * n.y;
            o.z = a * fmaf(x.z, pre_scale, pre_shift) + s * n.z; o.w = a * fmaf(x.w, pre_scale, pre_shift) + s * n.w;
            *reinterpret_cast<float4*>(out + base + i) = o;
        } else {
            for (long k = i; k < per_sample; ++k) out[base + k] = a * fmaf(x0[base + k], pre_scale, pre_shift) + s * noise[base + k];
        }
    }
}

// q_sample with clean context frames (frame-conditioned training, RaMViD: Hoeppe et al. 2022): out = m ? x0n : a[t_b] x0n + b[t_b] noise
// with x0n = x0 * pre_scale + pre_shift.  The noised branch is q_sample_kernel's expression, so an all-zero mask gives its values bit
// for bit.  Needs per_sample % 4 == 0 (float4 x0 / noise / out, uchar4 mask).
__global__ __launch_bounds__(256) void q_sample_masked_kernel(const float* __restrict__ x0, const int* __restrict__ t,
                                                              const float* __restrict__ noise, const unsigned char* __restrict__ mask,
                                                              float* __restrict__ out, const float* __restrict__ sqrt_ac,
                                                              const float* __restrict__ sqrt_1mac, long per_sample, float pre_scale,
                                                              float pre_shift) {
    const int b = blockIdx.y;
    const float a = sqrt_ac[t[b]], s = sqrt_1mac[t[b]];
    const size_t base = (size_t)b * per_sample;
    for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < per_sample; i += (long)gridDim.x * blockDim.x * 4) {
        const float4 x = *reinterpret_cast<const float4*>(x0 + base + i);
        const float4 n = *reinterpret_cast<const float4*>(noise + base + i);
        const uchar4 m = *reinterpret_cast<const uchar4*>(mask + base + i);
        float4 o;
        o.x = a * fmaf(x.x, pre_scale, pre_shift) + s * n.x; o.y = a * fmaf(x.y, pre_scale, pre_shift) + s * n.y;
        o.z = a * fmaf(x.z, pre_scale, pre_shift) + s * n.z; o.w = a * fmaf(x.w, pre_scale, pre_shift) + s * n.w;
        if (m.x) o.x = fmaf(x.x, pre_scale, pre_shift);
        if (m.y) o.y = fmaf(x.y, pre_scale, pre_shift);
        if (m.z) o.z = fmaf(x.z, pre_scale, pre_shift);
        if (m.w) o.w = fmaf(x.w, pre_scale, pre_shift);
        *reinterpret_cast<float4*>(out + base + i) = o;
    }
}

// (the per-element arithmetic of one ancestral reverse step, p_step_coef / p_step_elem: vdx_pstep.h)

// one reverse step.  tables: [5][T] = sqrt_recip_ac | sqrt_recipm1_ac | post_mean_coef1 | post_mean_coef2 | post_logvar_clipped
__global__ __launch_bounds__(256) void p_sample_kernel(PSampleArgs P) {
    const int b = blockIdx.y;
    const PStepCoef kc = p_step_coef(P, b, P.t[b]);
    unsigned long long off = P.offset;
    if (P.dev_offset) off += *P.dev_offset;
    const long per = P.per_sample, fhw = P.per_sample / P.C;
    const size_t base = (size_t)b * per;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; 4 * q < per; q += (long)gridDim.x * blockDim.x) {
        const long i = 4 * q;
        float xv[4], ev[4], nv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long e = i + k;
            xv[k] = ev[k] = 0.f;
            if (e < per) {
                xv[k] = P.x[base + e];
                const long c = e / fhw, r = e - c * fhw;                 // [C,F,H,W] -> channel-last [F,H,W,C]
                ev[k] = P.eps[base + r * P.C + c];
            }
        }
        if (P.noise) {
#pragma unroll
            for (int k = 0; k < 4; ++k) nv[k] = (i + k < per) ? P.noise[base + i + k] : 0.f;
        } else {
            const float4 z = randn4((unsigned long long)(base / 4 + q), P.seed, off);   // element index of the whole tensor
            nv[0] = z.x; nv[1] = z.y; nv[2] = z.z; nv[3] = z.w;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float o = p_step_elem(kc, xv[k], ev[k], nv[k]);
            if (i + k < per) P.out[base + i + k] = o * P.post_scale + P.post_shift;
        }
    }
}

// Replacement-method conditioning (Ho et al. 2022, sec. 3.1) + RePaint resampling (Lugmayr et al. 2022): one pass that does the
// ancestral step, merges the known region and optionally re-noises back to level t.  s = M.step + *M.step_dev (global step counter):
//   x' = p_step(x, eps, Philox(seed, 1 + s))
//   kn = t == 0 ? k : sqrt_ac[t-1] k + sqrt_1mac[t-1] Philox(seed, VDX_DRAW_KNOWN + s)
//   x  = m ? kn : x'
//   if s % U != U-1:  x = sqrt(alpha_t) x + sqrt(beta_t) Philox(seed, VDX_DRAW_RENOISE + s)
// Needs per_sample % 4 == 0 (float4 x / known / out, uchar4 mask).  x and out may alias.
__global__ __launch_bounds__(256) void p_sample_masked_kernel(PSampleArgs P, MaskArgs M) {
    const int b = blockIdx.y;
    const int tb = P.t[b];
    const PStepCoef kc = p_step_coef(P, b, tb);
    const unsigned long long s = M.step + (M.step_dev ? *M.step_dev : 0ull);
    const bool renoise = (s % (unsigned long long)M.U) != (unsigned long long)(M.U - 1);
    const float ka = tb > 0 ? M.mtab[tb - 1] : 1.f, kb = tb > 0 ? M.mtab[P.T + tb - 1] : 0.f;
    const float ra = M.mtab[2 * P.T + tb], rb = M.mtab[3 * P.T + tb];
    const long per = P.per_sample, fhw = P.per_sample / P.C;
    const size_t base = (size_t)b * per;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; 4 * q < per; q += (long)gridDim.x * blockDim.x) {
        const long i = 4 * q;
        const unsigned long long ctr = (unsigned long long)(base / 4 + q);      // element index of the whole tensor / 4
        const float4 x4 = *reinterpret_cast<const float4*>(P.x + base + i);
        const uchar4 m4 = *reinterpret_cast<const uchar4*>(M.mask + base + i);
        const float xv[4] = {x4.x, x4.y, x4.z, x4.w};
        const bool mk[4] = {m4.x != 0, m4.y != 0, m4.z != 0, m4.w != 0};
        float ev[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long e = i + k, c = e / fhw, r = e - c * fhw;                 // [C,F,H,W] -> channel-last [F,H,W,C]
            ev[k] = P.eps[base + r * P.C + c];
        }
        const float4 z = randn4(ctr, P.seed, 1ull + s);
        const float nv[4] = {z.x, z.y, z.z, z.w};
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = p_step_elem(kc, xv[k], ev[k], nv[k]);
        if (mk[0] | mk[1] | mk[2] | mk[3]) {                                   // the known-region draw only where a lane needs it
            const float4 k4 = *reinterpret_cast<const float4*>(M.known + base + i);
            const float kv[4] = {k4.x, k4.y, k4.z, k4.w};
            float zk[4] = {0.f, 0.f, 0.f, 0.f};
            if (tb > 0) { const float4 w = randn4(ctr, P.seed, VDX_DRAW_KNOWN + s); zk[0] = w.x; zk[1] = w.y; zk[2] = w.z; zk[3] = w.w; }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (mk[k]) o[k] = tb > 0 ? ka * kv[k] + kb * zk[k] : kv[k];
        }
        if (renoise) {
            const float4 w = randn4(ctr, P.seed, VDX_DRAW_RENOISE + s);
            const float zr[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = ra * o[k] + rb * zr[k];
        }
        *reinterpret_cast<float4*>(P.out + base + i) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// after a masked step: t[b] -= 1 (floor 0) when s % U == U-1, then s += 1 -- one captured step serves every (t, u)
__global__ void resample_advance_kernel(int* t, int B, unsigned long long* step_dev, int U) {
    const unsigned long long s = *step_dev;
    if (s % (unsigned long long)U == (unsigned long long)(U - 1))
        for (int i = threadIdx.x; i < B; i += blockDim.x)
            if (t[i] > 0) t[i] -= 1;
    __syncthreads();
    if (threadIdx.x == 0) *step_dev = s + 1;
}

// first merge of the known region: x = m ? sqrt_ac[t0] k + sqrt_1mac[t0] x : x  (x_T's own noise; in place)
__global__ __launch_bounds__(256) void inpaint_init_kernel(float* __restrict__ x, const float* __restrict__ known,
                                                           const unsigned char* __restrict__ mask, const float* __restrict__ mtab,
                                                           int T, int t0, long n) {
    const float a = mtab[t0], bb = mtab[T + t0];
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; 4 * q < n; q += (long)gridDim.x * blockDim.x) {
        const uchar4 m4 = *reinterpret_cast<const uchar4*>(mask + 4 * q);
        if (!(m4.x | m4.y | m4.z | m4.w)) continue;
        float4 x4 = *reinterpret_cast<const float4*>(x + 4 * q);
        const float4 k4 = *reinterpret_cast<const float4*>(known + 4 * q);
        if (m4.x) x4.x = a * k4.x + bb * x4.x;
        if (m4.y) x4.y = a * k4.y + bb * x4.y;
        if (m4.z) x4.z = a * k4.z + bb * x4.z;
        if (m4.w) x4.w = a * k4.w + bb * x4.w;
        *reinterpret_cast<float4*>(x + 4 * q) = x4;
    }
}

// DDIM reverse step, eta = 0 (Song et al. 2020, eq. 12; NO reference code: the reference samples with ancestral DDPM only --
// BASELINE.json configs[3] asks for "DDIM-100").  Time pair (t, t_next) = (seq[k], seq[k+1]) with k = *step_dev
// (or 0); t_next < 0 means "the data itself" (alpha_bar = 1).
//   x0 = (x - sqrt(1 - ac_t) eps) / sqrt(ac_t)        [clip to +-s, / s as p_sample does]
//   eps' = (x - sqrt(ac_t) x0) / sqrt(1 - ac_t)       (re-derived from the CLIPPED x0, as the usual implementations do)
//   out = sqrt(ac_next) x0 + sqrt(1 - ac_next) eps'
// (x and out may alias -- vdx.h -- so neither is __restrict__)
// the per-element arithmetic of one DDIM step, shared by ddim_step_kernel and ddim_step_masked_kernel
struct DdimCoef { float sa, s1, na, n1, s; int clip; };

__device__ __forceinline__ DdimCoef ddim_coef(const float* ac, int tb, int tn, const float* thres, int b, int clip) {
    const float a_t = ac[tb], a_n = tn >= 0 ? ac[tn] : 1.0f;
    DdimCoef k;
    k.sa = sqrtf(a_t); k.s1 = sqrtf(1.0f - a_t); k.na = sqrtf(a_n); k.n1 = sqrtf(1.0f - a_n);
    k.s = thres ? thres[b] : 1.0f;
    k.clip = clip;
    return k;
}

__device__ __forceinline__ float ddim_mix(float a, float x, float b, float y) {
#pragma clang fp contract(off)
    return a * x + b * y;
}

// The contractions are spelled out: the one-element form and the four-element form would otherwise be fused differently by the
// compiler (packed multiplies vs fma), and an all-zero mask must give vdx_ddim_step's values bit for bit.
__device__ __forceinline__ float ddim_elem(const DdimCoef& k, float xv, float ev) {
    float x0 = fmaf(-k.s1, ev, xv) / k.sa;
    if (k.clip) x0 = fminf(fmaxf(x0, -k.s), k.s) / k.s;
    const float e2 = fmaf(-k.sa, x0, xv) / k.s1;                    // eps re-derived from the clipped x0
    return ddim_mix(k.na, x0, k.n1, e2);
}

__global__ __launch_bounds__(256) void ddim_step_kernel(const float* x, const float* __restrict__ eps, float* out,
                                                        const float* __restrict__ ac, const int* __restrict__ seq,
                                                        const unsigned long long* __restrict__ step_dev, const float* __restrict__ thres,
                                                        int clip, int C, long per_sample) {
    const int b = blockIdx.y;
    const int k = step_dev ? (int)*step_dev : 0;
    const DdimCoef kc = ddim_coef(ac, seq[k], seq[k + 1], thres, b, clip);
    const long per = per_sample, fhw = per_sample / C;
    const size_t base = (size_t)b * per;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < per; e += (long)gridDim.x * blockDim.x) {
        const float xv = x[base + e];
        const long c = e / fhw, r = e - c * fhw;                         // [C,F,H,W] -> channel-last [F,H,W,C]
        out[base + e] = ddim_elem(kc, xv, eps[base + r * C + c]);
    }
}

// masked DDIM step (eta = 0), 4 elements per thread: x' = ddim step (seq[j] -> seq[j+1]), j = *step_dev (or 0);
//   kn = seq[j+1] < 0 ? k : sqrt_ac[tn] k + sqrt_1mac[tn] Philox(seed, VDX_DRAW_KNOWN + j);  out = m ? kn : x'
__global__ __launch_bounds__(256) void ddim_step_masked_kernel(const float* x, const float* __restrict__ eps, float* out,
                                                               const float* __restrict__ ac, const int* __restrict__ seq,
                                                               const unsigned long long* __restrict__ step_dev, const float* __restrict__ thres,
                                                               int clip, int C, long per_sample, MaskArgs M, int T, unsigned long long seed) {
    const int b = blockIdx.y;
    const int j = step_dev ? (int)*step_dev : 0;
    const int tn = seq[j + 1];
    const DdimCoef kc = ddim_coef(ac, seq[j], tn, thres, b, clip);
    const float ka = tn >= 0 ? M.mtab[tn] : 1.f, kb = tn >= 0 ? M.mtab[T + tn] : 0.f;
    const long per = per_sample, fhw = per_sample / C;
    const size_t base = (size_t)b * per;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; 4 * q < per; q += (long)gridDim.x * blockDim.x) {
        const long i = 4 * q;
        const float4 x4 = *reinterpret_cast<const float4*>(x + base + i);
        const uchar4 m4 = *reinterpret_cast<const uchar4*>(M.mask + base + i);
        const float xv[4] = {x4.x, x4.y, x4.z, x4.w};
        const bool mk[4] = {m4.x != 0, m4.y != 0, m4.z != 0, m4.w != 0};
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long e = i + k, c = e / fhw, r = e - c * fhw;                 // [C,F,H,W] -> channel-last [F,H,W,C]
            o[k] = ddim_elem(kc, xv[k], eps[base + r * C + c]);
        }
        if (mk[0] | mk[1] | mk[2] | mk[3]) {
            const float4 k4 = *reinterpret_cast<const float4*>(M.known + base + i);
            const float kv[4] = {k4.x, k4.y, k4.z, k4.w};
            float zk[4] = {0.f, 0.f, 0.f, 0.f};
            if (tn >= 0) {
                const float4 w = randn4((unsigned long long)(base / 4 + q), seed, VDX_DRAW_KNOWN + (unsigned long long)j);
                zk[0] = w.x; zk[1] = w.y; zk[2] = w.z; zk[3] = w.w;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (mk[k]) o[k] = tn >= 0 ? ka * kv[k] + kb * zk[k] : kv[k];
        }
        *reinterpret_cast<float4*>(out + base + i) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// DPM-Solver++(2M) step (Lu et al. 2022, data-prediction multistep form; NO reference code: EXTENSION, parity unpinned).  With
// a_t = ac[t]: alpha_t = sqrt(a_t), sigma_t = sqrt(1 - a_t), lambda_t = 0.5 ln(a_t / (1 - a_t)).  Step k = *step_dev (or 0) goes
// from s = seq[k] to n = seq[k+1]:
//   x0 = (x - sigma_s eps) / alpha_s                 [clipped exactly as ddim_elem does]
//   n < 0:  out = x0                                  (the step into the data is first order)
//   else    h = lambda_n - lambda_s
//           D = x0                                    if k == 0 or order == 1
//           D = (1 + c) x0 - c hist,  c = h / (2 (lambda_s - lambda_{seq[k-1]}))   otherwise
//           out = (sigma_n / sigma_s) x - alpha_n expm1(-h) D
//   hist = x0                                         (every step; each thread reads its hist element before it writes it)
// order == 1 is ddim_step_kernel's update written in lambda.  The per-step scalars are evaluated in double by one thread of the
// workgroup (h and expm1(-h) are differences of nearly equal numbers on a fine sequence) and handed on as fp32.
struct DpmCoef { float sa, s1, r, g, c1, c, s; int clip, last, second; };

__device__ DpmCoef dpm_coef(const float* ac, const int* seq, int k, int order, const float* thres, int b, int clip) {
    const int ts = seq[k], tn = seq[k + 1];
    const double a_s = (double)ac[ts];
    const double al_s = sqrt(a_s), sg_s = sqrt(1.0 - a_s);
    DpmCoef K;
    K.sa = (float)al_s; K.s1 = (float)sg_s;
    K.s = thres ? thres[b] : 1.0f;
    K.clip = clip;
    K.last = tn < 0;
    K.second = 0;
    K.r = 0.f; K.g = 1.f; K.c1 = 1.f; K.c = 0.f;
    if (tn >= 0) {
        const double a_n = (double)ac[tn];
        const double lam_s = 0.5 * log(a_s / (1.0 - a_s)), lam_n = 0.5 * log(a_n / (1.0 - a_n));
        const double h = lam_n - lam_s;
        K.r = (float)(sqrt(1.0 - a_n) / sg_s);
        K.g = (float)(-sqrt(a_n) * expm1(-h));
        if (order == 2 && k > 0) {
            const double a_p = (double)ac[seq[k - 1]];
            const double c = h / (2.0 * (lam_s - 0.5 * log(a_p / (1.0 - a_p))));
            K.c1 = (float)(1.0 + c); K.c = (float)c;
            K.second = 1;
        }
    }
    return K;
}

// the contractions are spelled out, as in ddim_elem: an all-zero mask must give the unmasked kernel's values bit for bit
__device__ __forceinline__ float dpm_elem(const DpmCoef& k, float xv, float ev, float hv, float* x0_out) {
#pragma clang fp contract(off)
    float x0 = fmaf(-k.s1, ev, xv) / k.sa;
    if (k.clip) x0 = fminf(fmaxf(x0, -k.s), k.s) / k.s;
    *x0_out = x0;
    if (k.last) return x0;
    const float d = k.second ? fmaf(k.c1, x0, -(k.c * hv)) : x0;
    return fmaf(k.r, xv, k.g * d);
}

// 4 elements per thread (float4 x / hist / known / out, uchar4 mask; per_sample % 4 == 0).  x and out may alias.  MASKED merges the
// known region exactly as ddim_step_masked_kernel does; hist holds the network's x0 in the known region too.
template <bool MASKED>
__global__ __launch_bounds__(256) void dpm_step_kernel(const float* x, const float* __restrict__ eps, float* out, float* hist,
                                                       const float* __restrict__ ac, const int* __restrict__ seq,
                                                       const unsigned long long* __restrict__ step_dev, const float* __restrict__ thres,
                                                       int clip, int order, int C, long per_sample, MaskArgs M, int T, unsigned long long seed) {
    __shared__ DpmCoef coef;
    const int b = blockIdx.y;
    const int j = step_dev ? (int)*step_dev : 0;
    if (threadIdx.x == 0) coef = dpm_coef(ac, seq, j, order, thres, b, clip);
    __syncthreads();
    const DpmCoef kc = coef;
    const int tn = seq[j + 1];
    float ka = 1.f, kb = 0.f;
    if (MASKED && tn >= 0) { ka = M.mtab[tn]; kb = M.mtab[T + tn]; }
    const long per = per_sample, fhw = per_sample / C;
    const size_t base = (size_t)b * per;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; 4 * q < per; q += (long)gridDim.x * blockDim.x) {
        const long i = 4 * q;
        const float4 x4 = *reinterpret_cast<const float4*>(x + base + i);
        float4 h4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (kc.second) h4 = *reinterpret_cast<const float4*>(hist + base + i);
        const float xv[4] = {x4.x, x4.y, x4.z, x4.w};
        const float hv[4] = {h4.x, h4.y, h4.z, h4.w};
        float o[4], p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long e = i + k, c = e / fhw, r = e - c * fhw;                 // [C,F,H,W] -> channel-last [F,H,W,C]
            o[k] = dpm_elem(kc, xv[k], eps[base + r * C + c], hv[k], &p[k]);
        }
        if (hist) *reinterpret_cast<float4*>(hist + base + i) = make_float4(p[0], p[1], p[2], p[3]);
        if (MASKED) {
            const uchar4 m4 = *reinterpret_cast<const uchar4*>(M.mask + base + i);
            const bool mk[4] = {m4.x != 0, m4.y != 0, m4.z != 0, m4.w != 0};
            if (mk[0] | mk[1] | mk[2] | mk[3]) {
                const float4 k4 = *reinterpret_cast<const float4*>(M.known + base + i);
                const float kv[4] = {k4.x, k4.y, k4.z, k4.w};
                float zk[4] = {0.f, 0.f, 0.f, 0.f};
                if (tn >= 0) {
                    const float4 w = randn4((unsigned long long)(base / 4 + q), seed, VDX_DRAW_KNOWN + (unsigned long long)j);
                    zk[0] = w.x; zk[1] = w.y; zk[2] = w.z; zk[3] = w.w;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (mk[k]) o[k] = tn >= 0 ? ka * kv[k] + kb * zk[k] : kv[k];
            }
        }
        *reinterpret_cast<float4*>(out + base + i) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// after a DDIM step: t[b] = max(seq[k + 1], 0) for the next forward, k += 1
__global__ void ddim_advance_kernel(int* t, int B, const int* __restrict__ seq, unsigned long long* step_dev) {
    const int k = (int)*step_dev;
    const int tn = max(seq[k + 1], 0);
    for (int i = threadIdx.x; i < B; i += blockDim.x) t[i] = tn;
    __syncthreads();
    if (threadIdx.x == 0) *step_dev = (unsigned long long)(k + 1);
}

// Dynamic thresholding (Imagen; reference gaussian_diffusion.py:205-217): s_b = max(quantile_q(|x0_hat| over the sample), 1) with
// x0_hat = sqrt_recip_ac[t] x - sqrt_recipm1_ac[t] eps and the linearly interpolated quantile of jnp.quantile / torch.quantile
// (position q (n - 1)).  One workgroup per sample; the two order statistics are found by an exact 4 x 8-bit radix select on the
// bit patterns of the (non-negative) magnitudes, recomputing x0_hat in every pass instead of storing it.
__global__ __launch_bounds__(1024) void dyn_thres_kernel(const float* __restrict__ x, const float* __restrict__ eps, const int* __restrict__ t,
                                                         const float* __restrict__ tables, int T, float q, float* __restrict__ out,
                                                         int C, long per_sample) {
    __shared__ unsigned hist[256];
    __shared__ unsigned sel_prefix, sel_rank;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int tb = t[b];
    const float kr = tables[tb], km = tables[T + tb];
    const long per = per_sample, fhw = per_sample / C;
    const size_t base = (size_t)b * per;
    const double pos = (double)q * (double)(per - 1);
    const long k_lo = (long)floor(pos);
    const long k_hi = min(k_lo + 1, per - 1);
    const float frac = (float)(pos - (double)k_lo);
    float val[2];
    for (int which = 0; which < 2; ++which) {
        unsigned prefix = 0, rank = (unsigned)(which ? k_hi : k_lo);      // rank of the wanted element among those matching `prefix`
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            for (int i = tid; i < 256; i += blockDim.x) hist[i] = 0;
            __syncthreads();
            for (long e = tid; e < per; e += blockDim.x) {
                const long c = e / fhw, r = e - c * fhw;
                const unsigned u = __float_as_uint(fabsf(kr * x[base + e] - km * eps[base + r * C + c]));
                if (pass == 0 || (u >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(u >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned acc = 0, d = 0;
                for (; d < 256; ++d) { if (acc + hist[d] > rank) break; acc += hist[d]; }
                sel_prefix = prefix | (d << shift); sel_rank = rank - acc;
            }
            __syncthreads();
            prefix = sel_prefix; rank = sel_rank;
            __syncthreads();
        }
        val[which] = __uint_as_float(prefix);
    }
    if (tid == 0) out[b] = fmaxf(val[0] + frac * (val[1] - val[0]), 1.0f);
}

__global__ void advance_kernel(int* t, int B, unsigned long long* dev_offset) {
    for (int i = threadIdx.x; i < B; i += blockDim.x)         // one workgroup strides over the batch (any B)
        if (t[i] > 0) t[i] -= 1;
    if (threadIdx.x == 0 && dev_offset) *dev_offset += 1;
}

// sum over all elements of |eps_hat - eps| or (eps_hat - eps)^2 -> acc[0] (double); host divides by the count
__global__ __launch_bounds__(256) void loss_kernel(const float* __restrict__ eps_hat, const float* __restrict__ noise, double* acc,
                                                   int B, int Cc, long fhw, int l2) {
    __shared__ float red[4];
    const long n = (long)B * Cc * fhw;
    float s = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long b = i / (Cc * fhw), r = i - b * Cc * fhw;
        const long c = r / fhw, p = r - c * fhw;
        const float d = eps_hat[(b * fhw + p) * Cc + c] - noise[i];
        s += l2 ? d * d : fabsf(d);
    }
    for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) unsafeAtomicAdd(acc, (double)(red[0] + red[1] + red[2] + red[3]));
}

// Masked loss (frame-conditioned training): the sum of |eps_hat - eps| or (eps_hat - eps)^2 and the number of elements, both over
// the elements whose mask byte is 0 (the noised frames).  Pass 1: quad q of the [B,C,F,H,W] tensor belongs to thread q mod (grid * 256)
// of a fixed grid, every thread adds in double, a fixed-order tree over the workgroup leaves one (sum, count) pair per workgroup in
// partial[2 * blockIdx.x ..].  No atomics: the bits of the result depend on the inputs only (the scheme of grad_sqnorm_partial_kernel).
constexpr int kLossMaskedBlocks = 256;
__global__ __launch_bounds__(256) void loss_masked_partial_kernel(const float* __restrict__ eps_hat, const float* __restrict__ noise,
                                                                  const unsigned char* __restrict__ mask, double* __restrict__ partial,
                                                                  int B, int Cc, long fhw, int l2) {
    __shared__ double red_s[256];
    __shared__ double red_c[256];
    const long n = (long)B * Cc * fhw, quads = n / 4;
    double s = 0.0, cnt = 0.0;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long)gridDim.x * blockDim.x) {
        const long i0 = 4 * q;
        const uchar4 m4 = *reinterpret_cast<const uchar4*>(mask + i0);
        if (m4.x && m4.y && m4.z && m4.w) continue;                       // a quad inside a context frame
        const float4 n4 = *reinterpret_cast<const float4*>(noise + i0);
        const float nv[4] = {n4.x, n4.y, n4.z, n4.w};
        const bool mk[4] = {m4.x != 0, m4.y != 0, m4.z != 0, m4.w != 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (mk[k]) continue;
            const long i = i0 + k;
            const long b = i / (Cc * fhw), r = i - b * Cc * fhw;
            const long c = r / fhw, p = r - c * fhw;                      // [C,F,H,W] -> channel-last [F,H,W,C]
            const float d = eps_hat[(b * fhw + p) * Cc + c] - nv[k];
            s += l2 ? (double)d * (double)d : (double)fabsf(d);
            cnt += 1.0;
        }
    }
    red_s[threadIdx.x] = s; red_c[threadIdx.x] = cnt;
    __syncthreads();
#pragma unroll
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { red_s[threadIdx.x] += red_s[threadIdx.x + w]; red_c[threadIdx.x] += red_c[threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = red_s[0]; partial[2 * blockIdx.x + 1] = red_c[0]; }
}

// pass 2, one workgroup: the partial pairs are staged in LDS and added by one thread in index order; out = (sum, count)
__global__ __launch_bounds__(256) void loss_masked_final_kernel(const double* __restrict__ partial, double* __restrict__ out) {
    __shared__ double part[2 * kLossMaskedBlocks];
    for (int i = threadIdx.x; i < 2 * kLossMaskedBlocks; i += blockDim.x) part[i] = partial[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0, c = 0.0;
        for (int i = 0; i < kLossMaskedBlocks; ++i) { s += part[2 * i]; c += part[2 * i + 1]; }
        out[0] = s; out[1] = c;
    }
}

// Classifier-free guidance (Ho & Salimans 2022; NO reference code: the reference's p_sample_loop drops cond -- EXTENSION, parity
// unpinned).  eps2 [2B][per] = the batched forward's output, rows [0, B) conditioned (c), rows [B, 2B) on the null embedding (n):
//   g = n + (c - n) s          three separately rounded operations: the bits torch forms in Unet3D.forward_with_cond_scale
// With guidance rescale phi (Lin et al. 2023, sec. 3.4) out = g * (float)(phi std(c) / std(g) + 1 - phi), the standard deviations per
// sample.  out may be eps2 itself (every thread reads its c and n before it writes g over c), so neither pointer is __restrict__.
constexpr int kCfgBlocks = 16;                 // workgroups per sample of the statistics pass, whatever per_sample or the device

// (plain operators under contract(off), as ddim_mix: __fmul_rn / __fadd_rn are `x * y` / `x + y` inlined from a header compiled with
// contraction on, and the pair came out as v_pk_fma_f32)
__device__ __forceinline__ float cfg_g(float c, float n, float s) {
#pragma clang fp contract(off)
    const float d = c - n;
    const float p = d * s;
    return n + p;
}

__device__ __forceinline__ float cfg_scale(float g, float f) {
#pragma clang fp contract(off)
    return g * f;
}

__global__ __launch_bounds__(256) void cfg_combine_kernel(const float* eps2, float* out, float s, const double* __restrict__ factor,
                                                          int B, long per_sample) {
    const int b = blockIdx.y;
    const float f = factor ? (float)factor[b] : 1.0f;
    const float* c = eps2 + (size_t)b * per_sample;
    const float* n = eps2 + (size_t)(B + b) * per_sample;
    float* o = out + (size_t)b * per_sample;
    const long quads = per_sample / 4;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long)gridDim.x * blockDim.x) {
        const float4 c4 = *reinterpret_cast<const float4*>(c + 4 * q);
        const float4 n4 = *reinterpret_cast<const float4*>(n + 4 * q);
        float4 g = make_float4(cfg_g(c4.x, n4.x, s), cfg_g(c4.y, n4.y, s), cfg_g(c4.z, n4.z, s), cfg_g(c4.w, n4.w, s));
        if (factor) { g.x = cfg_scale(g.x, f); g.y = cfg_scale(g.y, f); g.z = cfg_scale(g.z, f); g.w = cfg_scale(g.w, f); }
        *reinterpret_cast<float4*>(o + 4 * q) = g;
    }
}

// Statistics of the rescale, pass 1: per sample the sums of c, c^2, g, g^2 in double, g formed again by cfg_g (no stored copy).  Quad q
// of a sample belongs to thread q mod (kCfgBlocks * 256) of the sample's kCfgBlocks workgroups, a fixed-order tree over the workgroup
// leaves four partials per workgroup in partial[(b * kCfgBlocks + blockIdx.x) * 4 ..].  No atomics (the scheme of
// loss_masked_partial_kernel): the bits depend on the values only.
__global__ __launch_bounds__(256) void cfg_stats_partial_kernel(const float* __restrict__ eps2, float s, double* __restrict__ partial,
                                                                int B, long per_sample) {
    __shared__ double red[4][256];
    const int b = blockIdx.y;
    const float* c = eps2 + (size_t)b * per_sample;
    const float* n = eps2 + (size_t)(B + b) * per_sample;
    const long quads = per_sample / 4;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long)gridDim.x * blockDim.x) {
        const float4 c4 = *reinterpret_cast<const float4*>(c + 4 * q);
        const float4 n4 = *reinterpret_cast<const float4*>(n + 4 * q);
        const float cv[4] = {c4.x, c4.y, c4.z, c4.w}, nv[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double cd = (double)cv[k], gd = (double)cfg_g(cv[k], nv[k], s);
            a[0] += cd; a[1] += cd * cd; a[2] += gd; a[3] += gd * gd;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = a[k];
    __syncthreads();
#pragma unroll
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x < 4) partial[((size_t)b * kCfgBlocks + blockIdx.x) * 4 + threadIdx.x] = red[threadIdx.x][0];
}

__device__ __forceinline__ bool cfg_finite(double x) {      // on the bits: the library is built with -fno-honor-nans
    return ((unsigned long long)__double_as_longlong(x) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}

// pass 2, one workgroup, thread b = sample b: the sample's partials added in index order, then factor[b] = phi sqrt(SS_c / SS_g) + 1 - phi
// with SS_x = sum x^2 - (sum x)^2 / per_sample (the n - 1 of the two variances cancels); 1 when SS_g <= 0 or anything is not finite
__global__ __launch_bounds__(256) void cfg_stats_final_kernel(const double* __restrict__ partial, double* __restrict__ factor, float phi,
                                                              int B, long per_sample) {
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = 0; i < kCfgBlocks; ++i)
            for (int k = 0; k < 4; ++k) a[k] += partial[((size_t)b * kCfgBlocks + i) * 4 + k];
        const double cnt = (double)per_sample;
        const double ss_c = a[1] - a[0] * a[0] / cnt, ss_g = a[3] - a[2] * a[2] / cnt;
        double f = 1.0;
        if (cfg_finite(ss_c) && cfg_finite(ss_g) && ss_g > 0.0) {
            const double r = (double)phi * sqrt(fmax(ss_c, 0.0) / ss_g) + (1.0 - (double)phi);
            if (cfg_finite(r)) f = r;
        }
        factor[b] = f;
    }
}

// the constant cond_mask of the guided loops' batched forward: rows [0, B) conditioned (0), rows [B, 2B) on the null embedding (1)
__global__ void cfg_mask_kernel(unsigned char* mask, int B) {
    for (int i = threadIdx.x; i < 2 * B; i += blockDim.x) mask[i] = i >= B ? 1 : 0;
}

// Held-out evaluation: the terms of the variational bound in bits/dim (vdx.h: "Held-out evaluation"; EXTENSION, no reference code).
// tab [VDX_VLB_ROWS][T] doubles.  Both kernels run a fixed grid (kVlbBlocks, B), whatever per_sample or the device: quad q of a sample
// belongs to thread q mod (kVlbBlocks * 256) of the sample's workgroups.
constexpr int kVlbBlocks = 64;                 // one quad per thread at 16 x 64 x 64 x 1

// x0 = 2 x - 1 and x_t = a x0 + s eps of one element in double: the products of two floats are exact there, so x_t carries one double
// rounding.  vlb_noise_kernel rounds it to fp32 once for the network -- the correctly rounded value of the x_t vlb_term_kernel uses.
__device__ __forceinline__ double vlb_x0(float x) { return 2.0 * (double)x - 1.0; }
__device__ __forceinline__ double vlb_xt(float a, float s, float x, float n) { return fma((double)a, vlb_x0(x), (double)s * (double)n); }

__device__ __forceinline__ int vlb_level(const int* t, int b, int T) { return min(max(t[b], 0), T - 1); }

// the noise of quad q of sample b: the explicit tensor, or the Philox draw indexed by the element index of the whole tensor
__device__ __forceinline__ float4 vlb_eps4(const VlbArgs& P, size_t base, long q, unsigned long long draw) {
    if (P.noise) return *reinterpret_cast<const float4*>(P.noise + base + 4 * q);
    return randn4((unsigned long long)(base / 4 + q), P.seed, draw);
}

__global__ __launch_bounds__(256) void vlb_noise_kernel(VlbArgs P) {
    const int b = blockIdx.y;
    const int tb = vlb_level(P.t, b, P.T);
    const float a = (float)P.tab[tb], s = (float)P.tab[P.T + tb];
    const unsigned long long draw = P.draw + (P.step_dev ? *P.step_dev : 0ull);
    const size_t base = (size_t)b * P.per_sample;
    const long quads = P.per_sample / 4;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long)gridDim.x * blockDim.x) {
        const float4 x4 = *reinterpret_cast<const float4*>(P.x + base + 4 * q);
        const float4 n4 = vlb_eps4(P, base, q, draw);
        *reinterpret_cast<float4*>(P.xt + base + 4 * q) =
            make_float4((float)vlb_xt(a, s, x4.x, n4.x), (float)vlb_xt(a, s, x4.y, n4.y), (float)vlb_xt(a, s, x4.z, n4.z), (float)vlb_xt(a, s, x4.w, n4.w));
    }
}

// Phi(z) of the standard normal, in double
__device__ __forceinline__ double vlb_phi(double z) { return 0.5 * erfc(-z * 0.70710678118654752440); }

// -log2 of the discretized Gaussian's mass on the bin of x0 (half-width 1/255); on the upper tail the difference is taken between
// the two small complements
__device__ double vlb_decoder_bits(double x0, double mu, double inv_sigma) {
    const double zp = (x0 - mu + 1.0 / 255.0) * inv_sigma, zm = (x0 - mu - 1.0 / 255.0) * inv_sigma;
    double p;
    if (x0 < -0.999) p = vlb_phi(zp);
    else if (x0 > 0.999) p = vlb_phi(-zm);
    else p = zm > 0.0 ? vlb_phi(-zm) - vlb_phi(-zp) : vlb_phi(zp) - vlb_phi(zm);
    return -log(fmax(p, 1e-12)) * 1.44269504088896340736;
}

// the three doubles of every thread -> one triple per workgroup, by a fixed-order tree in LDS (the scheme of loss_masked_partial_kernel)
__device__ __forceinline__ void vlb_block_reduce(double (&red)[3][256], const double (&a)[3], double* __restrict__ partial, int b) {
#pragma unroll
    for (int k = 0; k < 3; ++k) red[k][threadIdx.x] = a[k];
    __syncthreads();
#pragma unroll
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) partial[((size_t)b * kVlbBlocks + blockIdx.x) * 3 + threadIdx.x] = red[threadIdx.x][0];
}

__global__ __launch_bounds__(256) void vlb_term_kernel(VlbArgs P) {
    __shared__ double red[3][256];
    const int b = blockIdx.y;
    const int tb = vlb_level(P.t, b, P.T);
    const double* tab = P.tab;
    const float a = (float)tab[tb], s = (float)tab[P.T + tb];
    const float kr = (float)tab[2 * P.T + tb], km = (float)tab[3 * P.T + tb];
    const double c1 = tab[4 * P.T + tb], c2 = tab[5 * P.T + tb], w = tab[6 * P.T + tb];
    const double inv_sigma = exp(-0.5 * tab[7 * P.T + tb]);
    const unsigned long long draw = P.draw + (P.step_dev ? *P.step_dev : 0ull);
    const long per = P.per_sample, fhw = P.per_sample / P.C, quads = P.per_sample / 4;
    const size_t base = (size_t)b * per;
    double acc[3] = {0.0, 0.0, 0.0};                                        // vb, mse, xstart_mse
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long)gridDim.x * blockDim.x) {
        const long i = 4 * q;
        const float4 x4 = *reinterpret_cast<const float4*>(P.x + base + i);
        const float4 n4 = vlb_eps4(P, base, q, draw);
        const float xv[4] = {x4.x, x4.y, x4.z, x4.w}, nv[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long e = i + k, c = e / fhw, r = e - c * fhw;                 // [C,F,H,W] -> channel-last [F,H,W,C]
            const float ev = P.eps[base + r * P.C + c];
            // x0, x_t (vlb_noise_kernel's expression: the network read its fp32 rounding) and x0_hat in double; at the low levels, where
            // x0_hat - x0 is a difference of nearly equal numbers, fp32 here would be the whole error of xstart_mse
            const double x0 = vlb_x0(xv[k]);
            const double xt = vlb_xt(a, s, xv[k], nv[k]);
            double xh = (double)kr * xt - (double)km * (double)ev;              // predict_start_from_noise
            if (P.clip) xh = fmin(fmax(xh, -1.0), 1.0);
            const double de = (double)ev - (double)nv[k], dx = xh - x0;
            acc[1] += de * de;
            acc[2] += dx * dx;
            if (tb > 0) acc[0] += w * (dx * dx);
            else acc[0] += vlb_decoder_bits(x0, c1 * xh + c2 * xt, inv_sigma);
        }
    }
    vlb_block_reduce(red, acc, P.partial, b);
}

// the prior term's sum, KL(q(x_{T-1} | x0) || N(0, 1)) in bits, as the first entry of the workgroup's triple
__global__ __launch_bounds__(256) void vlb_prior_kernel(const float* __restrict__ x, const double* __restrict__ tab, int T,
                                                        double* __restrict__ partial, long per_sample) {
    __shared__ double red[3][256];
    const int b = blockIdx.y;
    const double ac = tab[8 * T + T - 1];
    const double k0 = -log1p(-ac) - ac;                                   // -1 - log(1 - ac) + (1 - ac), without the cancellation
    const size_t base = (size_t)b * per_sample;
    const long quads = per_sample / 4;
    double acc[3] = {0.0, 0.0, 0.0};
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long)gridDim.x * blockDim.x) {
        const float4 x4 = *reinterpret_cast<const float4*>(x + base + 4 * q);
        const float xv[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double x0 = vlb_x0(xv[k]);
            acc[0] += 0.5 * (k0 + ac * x0 * x0) * 1.44269504088896340736;
        }
    }
    vlb_block_reduce(red, acc, partial, b);
}

// One workgroup, thread b = sample b: the sample's kVlbBlocks triples added in index order, / per_sample, the first nout of them to
// out[(k * B + b) * nout ..] with k = *step_dev (or 0).  With seq (the loop): t[:] = max(seq[k + 1], 0) for the next forward and k += 1;
// a step past the end of the sequence (k >= seq_len) writes nothing.
__global__ __launch_bounds__(256) void vlb_advance_kernel(const double* __restrict__ partial, double* __restrict__ out, int nout, int B,
                                                          long per_sample, int* t, const int* __restrict__ seq, int seq_len,
                                                          unsigned long long* step_dev) {
    const unsigned long long k = step_dev ? *step_dev : 0ull;
    const bool live = !seq || k < (unsigned long long)seq_len;
    if (live) {
        const int tn = seq ? max(seq[k + 1], 0) : 0;
        for (int b = threadIdx.x; b < B; b += blockDim.x) {
            double a[3] = {0.0, 0.0, 0.0};
            for (int i = 0; i < kVlbBlocks; ++i)
                for (int j = 0; j < 3; ++j) a[j] += partial[((size_t)b * kVlbBlocks + i) * 3 + j];
            for (int j = 0; j < nout; ++j) out[((size_t)k * B + b) * nout + j] = a[j] / (double)per_sample;
            if (seq) t[b] = tn;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && seq && live) *step_dev = k + 1;
}

// Learned reverse-process variances (vdx.h: "Learned variances"; EXTENSION, no reference code: Nichol & Dhariwal 2021).  The network's
// channel-last output [B,F,H,W,2C] holds eps_hat in channels [0, C) and v in [C, 2C); log sigma^2 = f max_log + (1 - f) min_log with
// f = (v + 1) / 2, v not clamped.

// p_step_elem with every rounding spelled out, in the order p_sample_kernel is compiled to (its two products of x0 and of the mean are
// rounded on their own -- packed multiplies -- and only c1 x0 + (c2 x) and the affine are fused): with sigma per element the compiler
// would otherwise pick other contractions, and at v = -1 the step has to be p_sample_kernel's bit for bit (as ddim_elem / cfg_g do it)
__device__ __forceinline__ float lv_step_elem(const PStepCoef& k, float sigma, float x, float eps, float z, float ps, float sh) {
#pragma clang fp contract(off)
    const float t1 = k.k_recip * x;
    const float t2 = k.k_recipm1 * eps;
    float x0 = t1 - t2;
    if (k.clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
    const float m2 = k.c2 * x;
    const float mean = fmaf(k.c1, x0, m2);
    const float sz = sigma * z;
    const float o = sz + mean;
    return fmaf(ps, o, sh);
}

// one reverse step with the model's variance.  tables [6][S] = sqrt_recip_ac | sqrt_recipm1_ac | coef1 | coef2 | max_log | min_log of the
// (respaced) chain; level i = idx[b], or S - 1 - (step + *step_dev).  The element arithmetic is p_sample_kernel's with sigma per element
// (lv_step_elem), so at v = -1 (log sigma^2 = min_log exactly) and min_log = the posterior log-variance the output is its bit for bit.  The
// affine post_scale / post_shift is applied on level 0 only (the last step of a chain).  x and out may alias.
__global__ __launch_bounds__(256) void p_sample_lv_kernel(LvStepArgs P) {
    const int b = blockIdx.y;
    const long k = (long)(P.step + (P.step_dev ? *P.step_dev : 0ull));
    const int lvl = P.idx ? P.idx[b] : (int)((long)P.S - 1 - k);
    const int i_lv = min(max(lvl, 0), P.S - 1);
    PStepCoef kc;
    kc.k_recip = P.tables[i_lv]; kc.k_recipm1 = P.tables[P.S + i_lv];
    kc.c1 = P.tables[2 * P.S + i_lv]; kc.c2 = P.tables[3 * P.S + i_lv];
    kc.sigma = 0.f; kc.s = 1.0f; kc.clip = P.clip;
    const float max_log = P.tables[4 * P.S + i_lv], min_log = P.tables[5 * P.S + i_lv];
    const float ps = i_lv == 0 ? P.post_scale : 1.0f, sh = i_lv == 0 ? P.post_shift : 0.0f;
    unsigned long long off = P.offset;
    if (P.dev_offset) off += *P.dev_offset;
    const long per = P.per_sample, fhw = P.per_sample / P.C;
    const int C2 = 2 * P.C;
    const size_t base = (size_t)b * per, base2 = 2 * base;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; 4 * q < per; q += (long)gridDim.x * blockDim.x) {
        const long i = 4 * q;
        float xv[4], ev[4], vv[4], nv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long e = i + j;
            xv[j] = ev[j] = 0.f; vv[j] = -1.f;
            if (e < per) {
                xv[j] = P.x[base + e];
                const long c = e / fhw, r = e - c * fhw;                 // [C,F,H,W] -> channel-last [F,H,W,2C]
                ev[j] = P.out2[base2 + r * C2 + c];
                vv[j] = P.out2[base2 + r * C2 + P.C + c];
            }
        }
        if (P.noise) {
#pragma unroll
            for (int j = 0; j < 4; ++j) nv[j] = (i + j < per) ? P.noise[base + i + j] : 0.f;
        } else {
            const float4 z = randn4((unsigned long long)(base / 4 + q), P.seed, off);   // element index of the whole tensor
            nv[0] = z.x; nv[1] = z.y; nv[2] = z.z; nv[3] = z.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float f = (vv[j] + 1.0f) * 0.5f;
            const float sigma = (i_lv == 0) ? 0.f : expf(0.5f * (f * max_log + (1.0f - f) * min_log));
            const float o = lv_step_elem(kc, sigma, xv[j], ev[j], nv[j], ps, sh);
            if (i + j < per) P.out[base + i + j] = o;
        }
    }
}

// log sigma^2 of the model in double
__device__ __forceinline__ double lv_logvar(double v, double max_log, double min_log) {
    const double f = 0.5 * (v + 1.0);
    return f * max_log + (1.0 - f) * min_log;
}

// KL(N(mu~, beta~) || N(mu, sigma^2)) in nats with dmu = mu~ - mu, D = log beta~ - log sigma^2: 0.5 (expm1(D) - D + dmu^2 e^{-log sigma^2});
// *dlv = its derivative in log sigma^2, 0.5 (1 - e^D - dmu^2 e^{-log sigma^2})
__device__ __forceinline__ double lv_kl(double dmu, double min_true, double lv, double* dlv) {
    const double delta = min_true - lv, em1 = expm1(delta), qd = dmu * dmu * exp(-lv);
    *dlv = 0.5 * (-em1 - qd);
    return 0.5 * (em1 - delta + qd);
}

// -ln of the discretized Gaussian's mass on the bin of x0 (vlb_decoder_bits' rules: tails, complements, the 1e-12 floor) with
// sigma = exp(0.5 lv); *dlv = its derivative in lv, 0.5 (phi(z+) z+ - phi(z-) z-) / p without the absent term on a tail, 0 where p is floored
__device__ double lv_decoder_nll(double x0, double mu, double lv, double* dlv) {
    const double inv_sigma = exp(-0.5 * lv);
    const double zp = (x0 - mu + 1.0 / 255.0) * inv_sigma, zm = (x0 - mu - 1.0 / 255.0) * inv_sigma;
    const double gp = 0.39894228040143267794 * exp(-0.5 * zp * zp) * zp, gm = 0.39894228040143267794 * exp(-0.5 * zm * zm) * zm;
    double p, g;
    if (x0 < -0.999) { p = vlb_phi(zp); g = gp; }
    else if (x0 > 0.999) { p = vlb_phi(-zm); g = -gm; }
    else { p = zm > 0.0 ? vlb_phi(-zm) - vlb_phi(-zp) : vlb_phi(zp) - vlb_phi(zm); g = gp - gm; }
    const bool floored = !(p > 1e-12);
    *dlv = floored ? 0.0 : 0.5 * g / p;
    return -log(floored ? 1e-12 : p);
}

// what the hybrid loss and the bound read of one level of the [VDX_LV_ROWS][T] double table
struct LvLevel { float a, s; double kr, km, c1, c2, max_log, min_log; };
__device__ __forceinline__ LvLevel lv_level(const double* tab, int T, int tb) {
    LvLevel L;
    L.a = (float)tab[tb]; L.s = (float)tab[T + tb];
    L.kr = tab[2 * T + tb]; L.km = tab[3 * T + tb]; L.c1 = tab[4 * T + tb]; L.c2 = tab[5 * T + tb];
    L.max_log = tab[6 * T + tb]; L.min_log = tab[7 * T + tb];
    return L;
}

// the variational term of one element in bits and its derivative in log sigma^2 (nats): the KL at t >= 1 (min_log[t] = log beta~_t
// there), the decoder at t = 0
__device__ __forceinline__ double lv_vb_elem(const LvLevel& L, int tb, double x0, double xt, double xh, double lv, double* dlv) {
    const double nats = tb > 0 ? lv_kl(L.c1 * (x0 - xh), L.min_log, lv, dlv) : lv_decoder_nll(x0, L.c1 * xh + L.c2 * xt, lv, dlv);
    return nats * 1.44269504088896340736;
}

// Hybrid loss L_simple + w L_vlb (Nichol & Dhariwal 2021, eq. 16) in one pass over x0, the noise and the network output: per-workgroup
// (mse, vb) sums in double into partial [B][kVlbBlocks][3] and, with d_out, the gradient [B,F,H,W,2C] in fp32.  x_t is formed again from
// x0 = x pre_scale + pre_shift and the noise as vlb_xt does.  eps_hat is detached inside vb: the eps_hat half of d_out is
// loss_grad_kernel's expression (the same bits), the v half dvb/dlogvar * 0.5 (max_log - min_log) * vscale with vscale = w / (N ln 2).
// Fixed grid (kVlbBlocks, B), element quads guarded, so any per_sample; no atomics.
__global__ __launch_bounds__(256) void hybrid_loss_kernel(HybridArgs P) {
    __shared__ double red[3][256];
    const int b = blockIdx.y;
    const int tb = vlb_level(P.t, b, P.T);
    const LvLevel L = lv_level(P.tab, P.T, tb);
    const double dv_scale = 0.5 * (L.max_log - L.min_log) * P.vscale;
    // importance weight of the sample (vdx_hybrid_loss_w): none, or exactly 1 -> the unweighted expressions and their bits
    const double iwb = P.iw ? P.iw[b] : 1.0;
    const bool plain = iwb == 1.0;
    const double g_scale = P.inv_count64 * iwb;
    const long per = P.per_sample, fhw = P.per_sample / P.C;
    const int C2 = 2 * P.C;
    const size_t base = (size_t)b * per, base2 = 2 * base;
    const bool vec = (per & 3) == 0;
    double acc[3] = {0.0, 0.0, 0.0};                                        // mse, vb
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; 4 * q < per; q += (long)gridDim.x * blockDim.x) {
        const long i = 4 * q;
        float xv[4], nv[4];
        if (vec) {
            const float4 x4 = *reinterpret_cast<const float4*>(P.x + base + i);
            const float4 n4 = *reinterpret_cast<const float4*>(P.noise + base + i);
            xv[0] = x4.x; xv[1] = x4.y; xv[2] = x4.z; xv[3] = x4.w;
            nv[0] = n4.x; nv[1] = n4.y; nv[2] = n4.z; nv[3] = n4.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool ok = i + k < per;
                xv[k] = ok ? P.x[base + i + k] : 0.f;
                nv[k] = ok ? P.noise[base + i + k] : 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long e = i + k;
            if (e >= per) continue;
            const long c = e / fhw, r = e - c * fhw;                            // [C,F,H,W] -> channel-last [F,H,W,2C]
            const size_t j = base2 + (size_t)r * C2 + c;
            const float ev = P.out2[j], vv = P.out2[j + P.C];
            const double x0 = fma((double)xv[k], (double)P.pre_scale, (double)P.pre_shift);
            const double xt = fma((double)L.a, x0, (double)L.s * (double)nv[k]);
            const double xh = L.kr * xt - L.km * (double)ev;                    // predict_start_from_noise, not clipped in training
            const double de = (double)ev - (double)nv[k];
            double dlv;
            acc[0] += P.l2 ? de * de : fabs(de);
            acc[1] += lv_vb_elem(L, tb, x0, xt, xh, lv_logvar((double)vv, L.max_log, L.min_log), &dlv);
            if (P.d_out) {
                const float d = ev - nv[k];
                if (plain) {
                    P.d_out[j] = P.l2 ? 2.0f * d * P.inv_count : ((d > 0.f) - (d < 0.f)) * P.inv_count;
                    P.d_out[j + P.C] = (float)(dlv * dv_scale);
                } else {                                                        // both halves in double, rounded once
                    P.d_out[j] = (float)((P.l2 ? 2.0 * de : (double)((de > 0.0) - (de < 0.0))) * g_scale);
                    P.d_out[j + P.C] = (float)(dlv * dv_scale * iwb);
                }
            }
        }
    }
    vlb_block_reduce(red, acc, P.partial, b);
}

// One workgroup: thread b adds sample b's partials in index order -> out[2 b ..] = the sample's means (mse, vb); then thread 0 adds the
// samples' sums in index order -> out[2 B ..] = (mean mse, mean vb, mean mse + w mean vb) over the batch
__global__ __launch_bounds__(256) void hybrid_final_kernel(const double* __restrict__ partial, double* __restrict__ out, int B, long per_sample,
                                                           double w, double* __restrict__ sums, const double* __restrict__ iw) {
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        double a[2] = {0.0, 0.0};
        for (int i = 0; i < kVlbBlocks; ++i)
            for (int j = 0; j < 2; ++j) a[j] += partial[((size_t)b * kVlbBlocks + i) * 3 + j];
        sums[2 * b] = a[0]; sums[2 * b + 1] = a[1];
        out[2 * b] = a[0] / (double)per_sample; out[2 * b + 1] = a[1] / (double)per_sample;
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x == 0) {
        double s0 = 0.0, s1 = 0.0;
        if (iw) for (int b = 0; b < B; ++b) { s0 += iw[b] * sums[2 * b]; s1 += iw[b] * sums[2 * b + 1]; }      // the totals carry iw_b
        else for (int b = 0; b < B; ++b) { s0 += sums[2 * b]; s1 += sums[2 * b + 1]; }
        const double n = (double)B * (double)per_sample;
        out[2 * B] = s0 / n; out[2 * B + 1] = s1 / n; out[2 * B + 2] = s0 / n + w * (s1 / n);
    }
}

// vlb_term_kernel with the model's log sigma^2 in the KL and decoder terms: eps = the [B,F,H,W,2C] output, tab [VDX_LV_ROWS][T]
__global__ __launch_bounds__(256) void vlb_term_lv_kernel(VlbArgs P) {
    __shared__ double red[3][256];
    const int b = blockIdx.y;
    const int tb = vlb_level(P.t, b, P.T);
    const LvLevel L = lv_level(P.tab, P.T, tb);
    const unsigned long long draw = P.draw + (P.step_dev ? *P.step_dev : 0ull);
    const long per = P.per_sample, fhw = P.per_sample / P.C, quads = P.per_sample / 4;
    const int C2 = 2 * P.C;
    const size_t base = (size_t)b * per, base2 = 2 * base;
    double acc[3] = {0.0, 0.0, 0.0};                                        // vb, mse, xstart_mse
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long)gridDim.x * blockDim.x) {
        const long i = 4 * q;
        const float4 x4 = *reinterpret_cast<const float4*>(P.x + base + i);
        const float4 n4 = vlb_eps4(P, base, q, draw);
        const float xv[4] = {x4.x, x4.y, x4.z, x4.w}, nv[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long e = i + k, c = e / fhw, r = e - c * fhw;                 // [C,F,H,W] -> channel-last [F,H,W,2C]
            const size_t j = base2 + (size_t)r * C2 + c;
            const float ev = P.eps[j], vv = P.eps[j + P.C];
            const double x0 = vlb_x0(xv[k]);
            const double xt = vlb_xt(L.a, L.s, xv[k], nv[k]);
            double xh = L.kr * xt - L.km * (double)ev;
            if (P.clip) xh = fmin(fmax(xh, -1.0), 1.0);
            const double de = (double)ev - (double)nv[k], dx = xh - x0;
            double dlv;
            acc[0] += lv_vb_elem(L, tb, x0, xt, xh, lv_logvar((double)vv, L.max_log, L.min_log), &dlv);
            acc[1] += de * de;
            acc[2] += dx * dx;
        }
    }
    vlb_block_reduce(red, acc, P.partial, b);
}

__global__ void affine_kernel(const float* __restrict__ x, float* __restrict__ y, long n, float a, float b) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) y[i] = fmaf(x[i], a, b);
}

// ---- launchers ------------------------------------------------------------------------------------------------

hipError_t launch_randn(float* out, long n, unsigned long long seed, unsigned long long offset, const unsigned long long* dev_offset, hipStream_t st) {
    hipLaunchKernelGGL(randn_kernel, dim3(ew_blocks((n + 3) / 4)), dim3(256), 0, st, out, n, seed, offset, dev_offset);
    return hipGetLastError();
}

hipError_t launch_q_sample(const float* x0, const int* t, const float* noise, float* out, const float* sqrt_ac, const float* sqrt_1mac,
                           int B, long per_sample, float pre_scale, float pre_shift, hipStream_t st) {
    hipLaunchKernelGGL(q_sample_kernel, dim3(ew_blocks((per_sample + 3) / 4), B), dim3(256), 0, st, x0, t, noise, out, sqrt_ac, sqrt_1mac,
                       per_sample, pre_scale, pre_shift);
    return hipGetLastError();
}

hipError_t launch_p_sample(const PSampleArgs& a, int B, hipStream_t st) {
    return LaunchScope(st, "p_sample_kernel", 0.0, 12.0 * B * a.per_sample, "B%d px%ld", B, a.per_sample)
        .launch(p_sample_kernel, dim3(ew_blocks((a.per_sample + 3) / 4), B), dim3(256), 0, a);
}

hipError_t launch_p_sample_masked(const PSampleArgs& a, const MaskArgs& m, int B, hipStream_t st) {
    return LaunchScope(st, "p_sample_masked_kernel", 0.0, 17.0 * B * a.per_sample, "B%d px%ld", B, a.per_sample)
        .launch(p_sample_masked_kernel, dim3(ew_blocks(a.per_sample / 4), B), dim3(256), 0, a, m);
}

hipError_t launch_resample_advance(int* t, int B, unsigned long long* step_dev, int U, hipStream_t st) {
    return LaunchScope(st, "resample_advance_kernel", 0.0, 0.0, "B%d", B).launch(resample_advance_kernel, dim3(1), dim3(1024), 0, t, B, step_dev, U);
}

hipError_t launch_inpaint_init(float* x, const float* known, const unsigned char* mask, const float* mtab, int T, int t0, long n, hipStream_t st) {
    return LaunchScope(st, "inpaint_init_kernel", 0.0, 13.0 * n, "n%ld", n).launch(inpaint_init_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, x, known, mask, mtab, T, t0, n);
}

hipError_t launch_advance(int* t, int B, unsigned long long* dev_offset, hipStream_t st) {
    return LaunchScope(st, "advance_kernel", 0.0, 0.0, "B%d", B).launch(advance_kernel, dim3(1), dim3(1024), 0, t, B, dev_offset);
}

hipError_t launch_ddim_step(const float* x, const float* eps, float* out, const float* ac, const int* seq, const unsigned long long* step_dev,
                            const float* thres, int clip, int B, int C, long per_sample, hipStream_t st) {
    return LaunchScope(st, "ddim_step_kernel", 0.0, 12.0 * B * per_sample, "B%d px%ld", B, per_sample)
        .launch(ddim_step_kernel, dim3(ew_blocks(per_sample), B), dim3(256), 0, x, eps, out, ac, seq, step_dev, thres, clip, C, per_sample);
}

hipError_t launch_ddim_step_masked(const float* x, const float* eps, float* out, const float* ac, const int* seq, const unsigned long long* step_dev,
                                   const float* thres, int clip, int B, int C, long per_sample, const MaskArgs& m, int T, unsigned long long seed,
                                   hipStream_t st) {
    return LaunchScope(st, "ddim_step_masked_kernel", 0.0, 17.0 * B * per_sample, "B%d px%ld", B, per_sample)
        .launch(ddim_step_masked_kernel, dim3(ew_blocks(per_sample / 4), B), dim3(256), 0, x, eps, out, ac, seq, step_dev, thres, clip, C, per_sample, m, T, seed);
}

hipError_t launch_dpm_step(const float* x, const float* eps, float* out, float* hist, const float* ac, const int* seq,
                           const unsigned long long* step_dev, const float* thres, int clip, int order, int B, int C, long per_sample,
                           const MaskArgs* m, int T, unsigned long long seed, hipStream_t st) {
    const dim3 grid(ew_blocks(per_sample / 4), B);
    if (m)
        return LaunchScope(st, "dpm_step_masked_kernel", 0.0, 25.0 * B * per_sample, "B%d px%ld o%d", B, per_sample, order)
            .launch(dpm_step_kernel<true>, grid, dim3(256), 0, x, eps, out, hist, ac, seq, step_dev, thres, clip, order, C, per_sample, *m, T, seed);
    return LaunchScope(st, "dpm_step_kernel", 0.0, 20.0 * B * per_sample, "B%d px%ld o%d", B, per_sample, order)
        .launch(dpm_step_kernel<false>, grid, dim3(256), 0, x, eps, out, hist, ac, seq, step_dev, thres, clip, order, C, per_sample, MaskArgs{}, 0, 0ull);
}

hipError_t launch_ddim_advance(int* t, int B, const int* seq, unsigned long long* step_dev, hipStream_t st) {
    return LaunchScope(st, "ddim_advance_kernel", 0.0, 0.0, "B%d", B).launch(ddim_advance_kernel, dim3(1), dim3(256), 0, t, B, seq, step_dev);
}

hipError_t launch_dyn_thres(const float* x, const float* eps, const int* t, const float* tables, int T, float q, float* out, int B, int C,
                            long per_sample, hipStream_t st) {
    return LaunchScope(st, "dyn_thres_kernel", 0.0, 8.0 * B * per_sample, "B%d px%ld", B, per_sample)
        .launch(dyn_thres_kernel, dim3(B), dim3(1024), 0, x, eps, t, tables, T, q, out, C, per_sample);
}

hipError_t launch_loss(const float* eps_hat, const float* noise, double* acc, int B, int Cc, long fhw, int l2, hipStream_t st) {
    hipLaunchKernelGGL(loss_kernel, dim3(ew_blocks((long)B * Cc * fhw)), dim3(256), 0, st, eps_hat, noise, acc, B, Cc, fhw, l2);
    return hipGetLastError();
}

hipError_t launch_q_sample_masked(const float* x0, const int* t, const float* noise, const unsigned char* mask, float* out, const float* sqrt_ac,
                                  const float* sqrt_1mac, int B, long per_sample, float pre_scale, float pre_shift, hipStream_t st) {
    hipLaunchKernelGGL(q_sample_masked_kernel, dim3(ew_blocks(per_sample / 4), B), dim3(256), 0, st, x0, t, noise, mask, out, sqrt_ac, sqrt_1mac,
                       per_sample, pre_scale, pre_shift);
    return hipGetLastError();
}

size_t loss_masked_scratch_doubles() { return 2 * kLossMaskedBlocks; }

hipError_t launch_loss_masked(const float* eps_hat, const float* noise, const unsigned char* mask, double* scratch, double* out, int B, int Cc,
                              long fhw, int l2, hipStream_t st) {
    hipLaunchKernelGGL(loss_masked_partial_kernel, dim3(kLossMaskedBlocks), dim3(256), 0, st, eps_hat, noise, mask, scratch, B, Cc, fhw, l2);
    hipLaunchKernelGGL(loss_masked_final_kernel, dim3(1), dim3(256), 0, st, scratch, out);
    return hipGetLastError();
}

// scratch of the guidance kernels, in doubles: partials [B][kCfgBlocks][4] | factor [B] | the guided loops' cond_mask (2B bytes)
static size_t cfg_factor_offset(int B) { return (size_t)B * kCfgBlocks * 4; }
static size_t cfg_mask_offset(int B) { return cfg_factor_offset(B) + (size_t)B; }
size_t cfg_scratch_doubles(int B) { return cfg_mask_offset(B) + ((size_t)2 * B + 7) / 8; }
unsigned char* cfg_scratch_mask(double* scratch, int B) { return reinterpret_cast<unsigned char*>(scratch + cfg_mask_offset(B)); }

hipError_t launch_cfg_mask(double* scratch, int B, hipStream_t st) {
    hipLaunchKernelGGL(cfg_mask_kernel, dim3(1), dim3(256), 0, st, cfg_scratch_mask(scratch, B), B);
    return hipGetLastError();
}

hipError_t launch_cfg_combine(const float* eps2, float* out, float cond_scale, float rescale, double* scratch, int B, long per_sample,
                              hipStream_t st) {
    double* factor = nullptr;
    if (rescale > 0.f) {
        factor = scratch + cfg_factor_offset(B);
        hipError_t e = LaunchScope(st, "cfg_stats_partial_kernel", 0.0, 8.0 * B * per_sample, "B%d px%ld", B, per_sample)
                           .launch(cfg_stats_partial_kernel, dim3(kCfgBlocks, B), dim3(256), 0, eps2, cond_scale, scratch, B, per_sample);
        if (e != hipSuccess) return e;
        e = LaunchScope(st, "cfg_stats_final_kernel", 0.0, 0.0, "B%d", B).launch(cfg_stats_final_kernel, dim3(1), dim3(256), 0, scratch, factor, rescale, B, per_sample);
        if (e != hipSuccess) return e;
    }
    return LaunchScope(st, "cfg_combine_kernel", 0.0, 12.0 * B * per_sample, "B%d px%ld", B, per_sample)
        .launch(cfg_combine_kernel, dim3(ew_blocks(per_sample / 4), B), dim3(256), 0, eps2, out, cond_scale, factor, B, per_sample);
}

int vlb_blocks() { return kVlbBlocks; }

hipError_t launch_vlb_noise(const VlbArgs& a, int B, hipStream_t st) {
    return LaunchScope(st, "vlb_noise_kernel", 0.0, 8.0 * B * a.per_sample, "B%d px%ld %s", B, a.per_sample, a.noise ? "noise" : "philox")
        .launch(vlb_noise_kernel, dim3(kVlbBlocks, B), dim3(256), 0, a);
}

hipError_t launch_vlb_terms(const VlbArgs& a, int B, hipStream_t st) {
    return LaunchScope(st, "vlb_term_kernel", 0.0, 8.0 * B * a.per_sample, "B%d px%ld C%d %s clip%d", B, a.per_sample, a.C,
                       a.noise ? "noise" : "philox", a.clip)
        .launch(vlb_term_kernel, dim3(kVlbBlocks, B), dim3(256), 0, a);
}

hipError_t launch_vlb_prior(const float* x, const double* tab, int T, double* partial, int B, long per_sample, hipStream_t st) {
    return LaunchScope(st, "vlb_prior_kernel", 0.0, 4.0 * B * per_sample, "B%d px%ld", B, per_sample)
        .launch(vlb_prior_kernel, dim3(kVlbBlocks, B), dim3(256), 0, x, tab, T, partial, per_sample);
}

hipError_t launch_vlb_advance(const double* partial, double* out, int nout, int B, long per_sample, int* t, const int* seq, int seq_len,
                              unsigned long long* step_dev, hipStream_t st) {
    return LaunchScope(st, "vlb_advance_kernel", 0.0, 0.0, "B%d n%d", B, nout)
        .launch(vlb_advance_kernel, dim3(1), dim3(256), 0, partial, out, nout, B, per_sample, t, seq, seq_len, step_dev);
}

hipError_t launch_p_sample_lv(const LvStepArgs& a, int B, hipStream_t st) {
    return LaunchScope(st, "p_sample_lv_kernel", 0.0, 16.0 * B * a.per_sample, "B%d px%ld S%d", B, a.per_sample, a.S)
        .launch(p_sample_lv_kernel, dim3(ew_blocks((a.per_sample + 3) / 4), B), dim3(256), 0, a);
}

size_t hybrid_scratch_doubles(int B) { return (size_t)B * kVlbBlocks * 3 + (size_t)2 * B; }

hipError_t launch_hybrid_loss(const HybridArgs& a, double* out, double w, int B, hipStream_t st) {
    hipError_t e = LaunchScope(st, "hybrid_loss_kernel", 0.0, (a.d_out ? 24.0 : 16.0) * B * a.per_sample, "B%d px%ld C%d l2 %d grad %d", B,
                               a.per_sample, a.C, a.l2, a.d_out ? 1 : 0)
                       .launch(hybrid_loss_kernel, dim3(kVlbBlocks, B), dim3(256), 0, a);
    if (e != hipSuccess) return e;
    return LaunchScope(st, "hybrid_final_kernel", 0.0, 0.0, "B%d", B)
        .launch(hybrid_final_kernel, dim3(1), dim3(256), 0, (const double*)a.partial, out, B, a.per_sample, w, a.partial + (size_t)B * kVlbBlocks * 3,
                a.iw);
}

hipError_t launch_vlb_terms_lv(const VlbArgs& a, int B, hipStream_t st) {
    return LaunchScope(st, "vlb_term_lv_kernel", 0.0, 12.0 * B * a.per_sample, "B%d px%ld C%d %s clip%d", B, a.per_sample, a.C,
                       a.noise ? "noise" : "philox", a.clip)
        .launch(vlb_term_lv_kernel, dim3(kVlbBlocks, B), dim3(256), 0, a);
}

hipError_t launch_affine(const float* x, float* y, long n, float a, float b, hipStream_t st) {
    hipLaunchKernelGGL(affine_kernel, dim3(ew_blocks(n)), dim3(256), 0, st, x, y, n, a, b);
    return hipGetLastError();
}

}  // namespace vdx
