// v-prediction (vdx.h: "v-prediction"; EXTENSION, no reference code: Salimans & Ho 2022, "Progressive Distillation", appendix D;
// min-SNR-gamma loss weights: Hang et al. 2023).  The network predicts v = sqrt(ac_t) eps - sqrt(1 - ac_t) x0.
//   v_to_eps ... the network output, converted in place to eps_hat = sqrt(ac_t) v_hat + sqrt(1 - ac_t) x_t: one streaming launch directly
//                behind the forward, so that every step kernel, the dynamic threshold, cfg_combine and the bits/dim terms stay the
//                eps-model's they are
//   v_loss ..... the loss against the v target (or against the noise: min-SNR weighting of the eps objective) with per-level weights
//                and importance weights, per sample, and its gradient in one pass; loss_weighted_kernel's shape (tsampler.hip)
// No atomics: every sum runs in a fixed order, so the bits of every output depend on the inputs only.
#include "vdx_common.h"
#include "vdx_internal.h"

namespace vdx {

// Grid (vlb_blocks(), rows); a thread takes quads of four consecutive elements of x [C,F,H,W], guarded element by element as
// loss_weighted_kernel guards them: any per_sample.  vec: per % 4 == 0 and x 16-byte aligned (float4 loads of x); vout: that, C == 1
// (channel-last is then x's own order) and out 16-byte aligned (float4 loads and stores of out).  The two products and the sum are
// rounded to fp32 one by one, whichever path an element takes.
__global__ __launch_bounds__(256) void v_to_eps_kernel(float* __restrict__ out, const float* __restrict__ x, const int* __restrict__ t,
                                                       const float* __restrict__ sqrt_ac, const float* __restrict__ sqrt_1mac, int T, int Cc,
                                                       long fhw, int vec, int vout) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int tb = min(max(t[b], 0), T - 1);
    const float sa = sqrt_ac[tb], s1 = sqrt_1mac[tb];
    const long per = (long)Cc * fhw;
    const size_t base = (size_t)b * per;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; 4 * q < per; q += (long)gridDim.x * blockDim.x) {
        const long i = 4 * q;
        float xv[4];
        if (vec) {
            const float4 x4 = *reinterpret_cast<const float4*>(x + base + i);
            xv[0] = x4.x; xv[1] = x4.y; xv[2] = x4.z; xv[3] = x4.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) xv[k] = i + k < per ? x[base + i + k] : 0.f;
        }
        if (vout) {
            float4 v4 = *reinterpret_cast<const float4*>(out + base + i);
            v4.x = sa * v4.x + s1 * xv[0]; v4.y = sa * v4.y + s1 * xv[1]; v4.z = sa * v4.z + s1 * xv[2]; v4.w = sa * v4.w + s1 * xv[3];
            *reinterpret_cast<float4*>(out + base + i) = v4;
            continue;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long e = i + k;
            if (e >= per) continue;
            const long c = e / fhw, r = e - c * fhw;                                // [C,F,H,W] -> channel-last [F,H,W,C]
            const size_t j = base + (size_t)r * Cc + c;
            out[j] = sa * out[j] + s1 * xv[k];
        }
    }
}

// loss_weighted_kernel with a target formed on the fly and a weight per level.  kind 1: target = sa noise - s1 x0n, the two products
// and the difference rounded to fp32 one by one, x0n = fma(x0, pre_scale, pre_shift) as q_sample_kernel forms it; kind 0: target =
// noise.  d = out - target in fp32, |d| or d^2 added in double, one partial per workgroup by a fixed-order tree.  d_out =
// loss_weighted_kernel's expression with f = (float)(iw_b w_b) * inv_count: kind 0 without wtab gives that kernel's bits.
__global__ __launch_bounds__(256) void v_loss_kernel(VLossArgs P) {
#pragma clang fp contract(off)
    __shared__ double red[256];
    const int b = blockIdx.y;
    const int Cc = P.C;
    const long fhw = P.fhw, per = (long)Cc * fhw;
    const size_t base = (size_t)b * per;
    const int tb = P.t ? min(max(P.t[b], 0), P.T - 1) : 0;
    const float sa = P.kind ? P.sqrt_ac[tb] : 0.f, s1 = P.kind ? P.sqrt_1mac[tb] : 0.f;
    const double g = (P.iw ? P.iw[b] : 1.0) * (P.wtab ? P.wtab[tb] : 1.0);
    const float f = (float)g * P.inv_count;
    double acc = 0.0;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; 4 * q < per; q += (long)gridDim.x * blockDim.x) {
        const long i = 4 * q;
        float nv[4], xv[4];
        if (P.vec) {
            const float4 n4 = *reinterpret_cast<const float4*>(P.noise + base + i);
            nv[0] = n4.x; nv[1] = n4.y; nv[2] = n4.z; nv[3] = n4.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) nv[k] = i + k < per ? P.noise[base + i + k] : 0.f;
        }
        if (P.kind && P.vec) {
            const float4 x4 = *reinterpret_cast<const float4*>(P.x0 + base + i);
            xv[0] = x4.x; xv[1] = x4.y; xv[2] = x4.z; xv[3] = x4.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) xv[k] = (P.kind && i + k < per) ? P.x0[base + i + k] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long e = i + k;
            if (e >= per) continue;
            const long c = e / fhw, r = e - c * fhw;                                // [C,F,H,W] -> channel-last [F,H,W,C]
            const size_t j = base + (size_t)r * Cc + c;
            const float target = P.kind ? sa * nv[k] - s1 * fmaf(xv[k], P.pre_scale, P.pre_shift) : nv[k];
            const float d = P.out[j] - target;
            acc += P.l2 ? (double)d * (double)d : (double)fabsf(d);
            if (P.d_out) P.d_out[j] = P.l2 ? 2.0f * d * f : ((d > 0.f) - (d < 0.f)) * f;
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) P.partial[(size_t)b * gridDim.x + blockIdx.x] = red[0];
}

// One workgroup: thread b adds sample b's partials in index order -> result[b] = w_b * (the sample's mean); thread 0 then adds
// iw_b result[b] over the samples in index order -> result[B] = (1 / B) sum_b iw_b result[b].  (loss_weighted_final_kernel with w_b.)
__global__ __launch_bounds__(256) void v_loss_final_kernel(const double* __restrict__ partial, const double* __restrict__ iw,
                                                           const double* __restrict__ wtab, const int* __restrict__ t, int T,
                                                           double* __restrict__ result, int B, int nblk, long per_sample) {
    __shared__ double tot[256];
    double run = 0.0;
    for (int b0 = 0; b0 < B; b0 += 256) {
        const int b = b0 + threadIdx.x;
        double l = 0.0;
        if (b < B) {
            double a = 0.0;
            for (int i = 0; i < nblk; ++i) a += partial[(size_t)b * nblk + i];
            l = a / (double)per_sample;
            if (wtab) l = wtab[min(max(t[b], 0), T - 1)] * l;
            result[b] = l;
            l = iw ? iw[b] * l : l;
        }
        tot[threadIdx.x] = l;
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < min(256, B - b0); ++i) run += tot[i];
        __syncthreads();
    }
    if (threadIdx.x == 0) result[B] = run / (double)B;
}

hipError_t launch_v_to_eps(float* out, const float* x, const int* t, const float* sqrt_ac, const float* sqrt_1mac, int T, int rows, int Cc,
                           long per_sample, hipStream_t st) {
    const int vec = (per_sample % 4 == 0) && ((uintptr_t)x % 16 == 0);
    const int vout = vec && Cc == 1 && ((uintptr_t)out % 16 == 0);
    return LaunchScope(st, "v_to_eps_kernel", 0.0, 12.0 * rows * per_sample, "B%d px%ld C%d %s", rows, per_sample, Cc,
                       vout ? "float4" : vec ? "float4 x" : "scalar")
        .launch(v_to_eps_kernel, dim3(vlb_blocks(), rows), dim3(256), 0, out, x, t, sqrt_ac, sqrt_1mac, T, Cc, per_sample / Cc, vec, vout);
}

size_t v_loss_scratch_doubles(int B) { return (size_t)B * vlb_blocks(); }

hipError_t launch_v_loss(VLossArgs a, double* scratch, double* result, int B, hipStream_t st) {
    const long per = (long)a.C * a.fhw, n = (long)B * per;
    a.vec = (per % 4 == 0) && ((uintptr_t)a.noise % 16 == 0) && (!a.kind || (uintptr_t)a.x0 % 16 == 0);
    a.inv_count = 1.0f / (float)n;
    a.partial = scratch;
    hipError_t e = LaunchScope(st, "v_loss_kernel", 0.0, ((a.d_out ? 12.0 : 8.0) + (a.kind ? 4.0 : 0.0)) * n,
                               "B%d C%d fhw%ld kind %d l2 %d w %d iw %d grad %d", B, a.C, a.fhw, a.kind, a.l2, a.wtab ? 1 : 0, a.iw ? 1 : 0,
                               a.d_out ? 1 : 0)
                       .launch(v_loss_kernel, dim3(vlb_blocks(), B), dim3(256), 0, a);
    if (e != hipSuccess) return e;
    return LaunchScope(st, "v_loss_final_kernel", 0.0, 0.0, "B%d", B)
        .launch(v_loss_final_kernel, dim3(1), dim3(256), 0, (const double*)scratch, a.iw, a.wtab, a.t, a.T, result, B, vlb_blocks(), per);
}

}  // namespace vdx
