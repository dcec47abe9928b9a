// Optimizer-side kernels of the train step (reference trainer.py:361-382): loss gradient, fused Adam + EMA on the
// flat parameter buffer (optax.adam semantics: bias-corrected, eps outside the sqrt, no weight decay).
#include "vdx_common.h"
#include "vdx_internal.h"

namespace vdx {

// d(mean loss)/d(eps_hat) in the UNet's channel-last layout; noise is [B,C,F,H,W]
__global__ __launch_bounds__(256) void loss_grad_kernel(const float* __restrict__ eps_hat, const float* __restrict__ noise,
                                                        float* __restrict__ d_eps, int B, int Cc, long fhw, int l2, float inv_count) {
    const long n = (long)B * Cc * fhw;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long b = i / (Cc * fhw), r = i - b * Cc * fhw;
        const long c = r / fhw, p = r - c * fhw;
        const long j = (b * fhw + p) * Cc + c;
        const float d = eps_hat[j] - noise[i];
        d_eps[j] = l2 ? 2.0f * d * inv_count : ((d > 0.f) - (d < 0.f)) * inv_count;
    }
}

// d(sum over the mask-0 elements / max(count, 1))/d(eps_hat) of the masked loss (frame-conditioned training), channel-last; exactly 0
// where the mask is nonzero.  count is read from the device (loss_masked_final_kernel's out[1]), so the host never sees it.  The
// reciprocal is the correctly rounded 1 / (float)count that launch_loss_grad forms on the host and the element expression is
// loss_grad_kernel's: with an all-zero mask the two kernels write the same bits.  4 elements per thread (float4 noise, uchar4 mask).
__global__ __launch_bounds__(256) void loss_grad_masked_kernel(const float* __restrict__ eps_hat, const float* __restrict__ noise,
                                                               const unsigned char* __restrict__ mask, const double* __restrict__ count_dev,
                                                               float* __restrict__ d_eps, int B, int Cc, long fhw, int l2) {
    const float inv_count = __fdiv_rn(1.0f, (float)fmax(*count_dev, 1.0));
    const long n = (long)B * Cc * fhw, quads = n / 4;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long)gridDim.x * blockDim.x) {
        const long i0 = 4 * q;
        const uchar4 m4 = *reinterpret_cast<const uchar4*>(mask + i0);
        const float4 n4 = *reinterpret_cast<const float4*>(noise + i0);
        const float nv[4] = {n4.x, n4.y, n4.z, n4.w};
        const bool mk[4] = {m4.x != 0, m4.y != 0, m4.z != 0, m4.w != 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long i = i0 + k;
            const long b = i / (Cc * fhw), r = i - b * Cc * fhw;
            const long c = r / fhw, p = r - c * fhw;
            const long j = (b * fhw + p) * Cc + c;
            const float d = eps_hat[j] - nv[k];
            const float g = l2 ? 2.0f * d * inv_count : ((d > 0.f) - (d < 0.f)) * inv_count;
            d_eps[j] = mk[k] ? 0.0f : g;
        }
    }
}

// The fused Adam + EMA update of one thread's elements of the flat buffers, g read as g * GRAD_SCALE: the body of adam_ema_kernel
// (GRAD_SCALE = grad_scale) and of adam_ema_clip_kernel (GRAD_SCALE = grad_scale * clip).  One text for both, so that with clip == 1
// the two kernels run the same arithmetic on the same values; a macro rather than a __device__ function because adam_ema_kernel then
// compiles to the instructions it had before the clipping form existed (the inlined function schedules differently).
#define VDX_ADAM_EMA_BODY(GRAD_SCALE)                                                                                                      \
    for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (long)gridDim.x * blockDim.x * 4) {                       \
        if (i + 3 < n) {                                                                                                                   \
            float4 pv = *reinterpret_cast<float4*>(p + i), gv = *reinterpret_cast<const float4*>(g + i);                                   \
            float4 mv = *reinterpret_cast<float4*>(m + i), vv = *reinterpret_cast<float4*>(v + i);                                         \
            float* pp = &pv.x; float* gg = &gv.x; float* mm = &mv.x; float* v2 = &vv.x;                                                    \
            _Pragma("unroll")                                                                                                              \
            for (int k = 0; k < 4; ++k) {                                                                                                  \
                const float gk = gg[k] * (GRAD_SCALE);                                                                                     \
                mm[k] = b1 * mm[k] + (1.f - b1) * gk;                                                                                      \
                v2[k] = b2 * v2[k] + (1.f - b2) * gk * gk;                                                                                 \
                pp[k] -= lr * (mm[k] / bc1) / (sqrtf(v2[k] / bc2) + eps);                                                                  \
            }                                                                                                                              \
            *reinterpret_cast<float4*>(p + i) = pv; *reinterpret_cast<float4*>(m + i) = mv; *reinterpret_cast<float4*>(v + i) = vv;        \
            if (do_ema) {                                                                                                                  \
                float4 e = *reinterpret_cast<float4*>(ema + i);                                                                            \
                e.x = decay * e.x + (1.f - decay) * pv.x; e.y = decay * e.y + (1.f - decay) * pv.y;                                        \
                e.z = decay * e.z + (1.f - decay) * pv.z; e.w = decay * e.w + (1.f - decay) * pv.w;                                        \
                *reinterpret_cast<float4*>(ema + i) = e;                                                                                   \
            }                                                                                                                              \
        } else {                                                                                                                           \
            for (long k = i; k < n; ++k) {                                                                                                 \
                const float gk = g[k] * (GRAD_SCALE);                                                                                      \
                m[k] = b1 * m[k] + (1.f - b1) * gk;                                                                                        \
                v[k] = b2 * v[k] + (1.f - b2) * gk * gk;                                                                                   \
                p[k] -= lr * (m[k] / bc1) / (sqrtf(v[k] / bc2) + eps);                                                                     \
                if (do_ema) ema[k] = decay * ema[k] + (1.f - decay) * p[k];                                                                \
            }                                                                                                                              \
        }                                                                                                                                  \
    }

// p, m, v, ema: flat fp32 [n]; g: gradient (already averaged over ranks).  grad_scale folds 1/world into the read.
__global__ __launch_bounds__(256) void adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, float* __restrict__ ema, long n, float lr, float b1, float b2,
                                                       float eps, float bc1, float bc2, float grad_scale, int do_ema, float decay) {
    VDX_ADAM_EMA_BODY(grad_scale)
}

// adam_ema_kernel behind global-norm clipping (reference utils.py:127-152 applied to the averaged gradient grad_scale * g):
// every thread derives the clip factor from the device-resident sum of squares, so the host never reads the norm.
__global__ __launch_bounds__(256) void adam_ema_clip_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, float* __restrict__ ema, long n, float lr, float b1,
                                                            float b2, float eps, float bc1, float bc2, float grad_scale, int do_ema,
                                                            float decay, const double* __restrict__ sqnorm, float max_grad_norm,
                                                            float* __restrict__ norm_out) {
    const double gs = (double)grad_scale;
    const double l2 = sqrt(gs * gs * *sqnorm + 1e-6);
    const double clip = fmin((double)max_grad_norm / (l2 + 1e-6), 1.0);
    const float s = (float)(gs * clip);
    if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) *norm_out = (float)l2;
    VDX_ADAM_EMA_BODY(s)
}

// a float4 that may sit on any 4-byte boundary (bucket offsets of the flat gradient buffer are tensor offsets)
struct __attribute__((packed, aligned(4))) float4u { float x, y, z, w; };

// acc[i] += g[i].  The head is peeled up to acc's 16-byte boundary and the tail after the last whole quad, one element per thread;
// the body reads and writes acc as aligned float4 and reads g, which may be misaligned differently, as float4u.
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g, long n, long head, long quads) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long tail0 = head + 4 * quads;
    if (tid < head) acc[tid] += g[tid];
    if (tail0 + tid < n) acc[tail0 + tid] += g[tail0 + tid];
    float* __restrict__ a = acc + head;
    const float* __restrict__ b = g + head;
    for (long q = tid; q < quads; q += (long)gridDim.x * blockDim.x) {
        float4 av = *reinterpret_cast<float4*>(a + 4 * q);
        const float4u gv = *reinterpret_cast<const float4u*>(b + 4 * q);
        av.x += gv.x; av.y += gv.y; av.z += gv.z; av.w += gv.w;
        *reinterpret_cast<float4*>(a + 4 * q) = av;
    }
}

// Sum of squares in double, pass 1: element i belongs to quad i / 4 whatever g's alignment, quad q to thread q mod (grid * 256),
// so the partial of a workgroup -- and the result -- depends on (g, n) only.  Four per-thread accumulators (one per quad lane), a
// fixed-order tree over the workgroup, one partial per workgroup; the < 4 elements after the last quad go to thread 0 of workgroup 0.
constexpr int kSqnormBlocks = 1024;
__global__ __launch_bounds__(256) void grad_sqnorm_partial_kernel(const float* __restrict__ g, long n, double* __restrict__ partial) {
    __shared__ double red[256];
    const long quads = n / 4;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll 4
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long)gridDim.x * blockDim.x) {
        const float4u gv = *reinterpret_cast<const float4u*>(g + 4 * q);
        const double x = (double)gv.x, y = (double)gv.y, z = (double)gv.z, w = (double)gv.w;
        a0 += x * x; a1 += y * y; a2 += z * z; a3 += w * w;
    }
    double acc = (a0 + a1) + (a2 + a3);
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long k = 4 * quads; k < n; ++k) { const double x = (double)g[k]; acc += x * x; }
    red[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// pass 2, one workgroup: the partials are staged in LDS and summed by one thread in index order
__global__ __launch_bounds__(256) void grad_sqnorm_final_kernel(const double* __restrict__ partial, double* __restrict__ out) {
    __shared__ double part[kSqnormBlocks];
    for (int i = threadIdx.x; i < kSqnormBlocks; i += blockDim.x) part[i] = partial[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < kSqnormBlocks; ++i) s += part[i];
        *out = s;
    }
}

hipError_t launch_loss_grad(const float* eps_hat, const float* noise, float* d_eps, int B, int Cc, long fhw, int l2, hipStream_t st) {
    const long n = (long)B * Cc * fhw;
    const int blocks = (int)std::max<long>(1, std::min<long>((n + 255) / 256, 2048));
    return LaunchScope(st, "loss_grad_kernel", 0.0, 0.0, "B%d C%d fhw%ld l2 %d", B, Cc, fhw, l2)
        .launch(loss_grad_kernel, dim3(blocks), dim3(256), 0, eps_hat, noise, d_eps, B, Cc, fhw, l2, 1.0f / (float)n);
}

hipError_t launch_loss_grad_masked(const float* eps_hat, const float* noise, const unsigned char* mask, const double* count_dev, float* d_eps,
                                   int B, int Cc, long fhw, int l2, hipStream_t st) {
    const long quads = (long)B * Cc * fhw / 4;
    const int blocks = (int)std::max<long>(1, std::min<long>((quads + 255) / 256, 2048));
    return LaunchScope(st, "loss_grad_masked_kernel", 0.0, 0.0, "B%d C%d fhw%ld l2 %d", B, Cc, fhw, l2)
        .launch(loss_grad_masked_kernel, dim3(blocks), dim3(256), 0, eps_hat, noise, mask, count_dev, d_eps, B, Cc, fhw, l2);
}

hipError_t launch_adam_ema(float* p, const float* g, float* m, float* v, float* ema, long n, float lr, float b1, float b2, float eps,
                           long step_count, float grad_scale, int do_ema, float decay, hipStream_t st) {
    const double t = (double)step_count + 1.0;                    // optax: bias correction with count + 1
    const float bc1 = (float)(1.0 - pow((double)b1, t)), bc2 = (float)(1.0 - pow((double)b2, t));
    const int blocks = (int)std::max<long>(1, std::min<long>((n / 4 + 255) / 256, 4096));
    return LaunchScope(st, "adam_ema_kernel", 0.0, 0.0, "n%ld ema %d", n, do_ema ? 1 : 0)
        .launch(adam_ema_kernel, dim3(blocks), dim3(256), 0, p, g, m, v, ema, n, lr, b1, b2, eps, bc1, bc2, grad_scale, do_ema, decay);
}

hipError_t launch_adam_ema_clip(float* p, const float* g, float* m, float* v, float* ema, long n, float lr, float b1, float b2, float eps,
                                long step_count, float grad_scale, int do_ema, float decay, const double* sqnorm, float max_grad_norm,
                                float* norm_out, hipStream_t st) {
    const double t = (double)step_count + 1.0;
    const float bc1 = (float)(1.0 - pow((double)b1, t)), bc2 = (float)(1.0 - pow((double)b2, t));
    const int blocks = (int)std::max<long>(1, std::min<long>((n / 4 + 255) / 256, 4096));
    return LaunchScope(st, "adam_ema_clip_kernel", 0.0, 0.0, "n%ld ema %d", n, do_ema ? 1 : 0)
        .launch(adam_ema_clip_kernel, dim3(blocks), dim3(256), 0, p, g, m, v, ema, n, lr, b1, b2, eps, bc1, bc2, grad_scale, do_ema, decay, sqnorm,
                max_grad_norm, norm_out);
}

hipError_t launch_grad_accumulate(float* acc, const float* g, long n, hipStream_t st) {
    const long head = std::min<long>(n, (long)((4 - (((uintptr_t)acc >> 2) & 3)) & 3));
    const long quads = (n - head) / 4;
    const int blocks = (int)std::max<long>(1, std::min<long>((quads + 255) / 256, 2048));
    return LaunchScope(st, "grad_accumulate_kernel", 0.0, 0.0, "n%ld head%ld", n, head)
        .launch(grad_accumulate_kernel, dim3(blocks), dim3(256), 0, acc, g, n, head, quads);
}

size_t grad_sqnorm_scratch_doubles() { return kSqnormBlocks; }

hipError_t launch_grad_sqnorm(const float* g, long n, double* scratch, double* out, hipStream_t st) {
    const hipError_t e = LaunchScope(st, "grad_sqnorm_partial_kernel", 0.0, 0.0, "n%ld blocks%d", n, kSqnormBlocks)
                             .launch(grad_sqnorm_partial_kernel, dim3(kSqnormBlocks), dim3(256), 0, g, n, scratch);
    if (e != hipSuccess) return e;
    return LaunchScope(st, "grad_sqnorm_final_kernel", 0.0, 0.0, "blocks%d", kSqnormBlocks)
        .launch(grad_sqnorm_final_kernel, dim3(1), dim3(256), 0, scratch, out);
}

}  // namespace vdx
