// Loss-aware timestep sampling (vdx.h: "Loss-aware timestep sampling"; EXTENSION, no reference code: Nichol & Dhariwal 2021, section 3.3,
// improved-diffusion's LossSecondMomentResampler restated in tests/_tsampler_ref.py).  The history of per-level losses, the
// probabilities, the draw and the importance weights live on the device: the train step issues launches and reads nothing back.
// No atomics anywhere: every sum runs in a fixed order, so the bits of every output depend on the inputs only.
#include "vdx_common.h"
#include "vdx_internal.h"
#include "vdx_philox.h"

namespace vdx {

constexpr int kTsThreads = 256;

__device__ __forceinline__ bool ts_finite(double x) {      // on the bits: the library is built with -fno-honor-nans
    return ((unsigned long long)__double_as_longlong(x) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}

// One workgroup.  LDS: p [T] | cum [max(T, 256)] doubles (the first 256 of cum double as the reduction scratch before cum is written).
// Thread i owns the contiguous levels [i chunk, (i + 1) chunk): W and the prefix are sums of the threads' chunk sums, the chunks added in
// index order inside a thread, the threads' sums by a fixed tree (W) or by thread 0 in index order (the prefix).
__global__ __launch_bounds__(kTsThreads) void tsampler_draw_kernel(const double* __restrict__ hist, const int* __restrict__ count, int T, int H,
                                                                   double eps, const int* __restrict__ t_given, unsigned long long seed,
                                                                   unsigned long long draw, int* __restrict__ t_out, double* __restrict__ iw_out,
                                                                   double* __restrict__ p_out, int batch) {
    extern __shared__ __attribute__((aligned(16))) char ts_smem[];
    double* p = reinterpret_cast<double*>(ts_smem);
    double* cum = p + T;
    const int tid = threadIdx.x;
    const int chunk = (T + kTsThreads - 1) / kTsThreads;
    const int lo = min(tid * chunk, T), hi = min(lo + chunk, T);
    int cold = 0;
    for (int t = tid; t < T; t += kTsThreads) cold |= count[t] < H;
    cold = __syncthreads_or(cold);
    const double uni = 1.0 / (double)T;
    if (!cold) {
        double part = 0.0;
        for (int t = lo; t < hi; ++t) {
            double s = 0.0;
            for (int j = 0; j < H; ++j) { const double v = hist[(size_t)t * H + j]; s += v * v; }
            const double w = sqrt(s / (double)H);
            p[t] = w; part += w;
        }
        cum[tid] = part;
        __syncthreads();
        for (int w = kTsThreads / 2; w > 0; w >>= 1) {
            if (tid < w) cum[tid] += cum[tid + w];
            __syncthreads();
        }
        const double W = cum[0];
        __syncthreads();
        const bool ok = ts_finite(W) && W > 0.0;
        part = 0.0;
        for (int t = lo; t < hi; ++t) {
            const double pt = ok ? (p[t] / W) * (1.0 - eps) + eps * uni : uni;
            p[t] = pt; part += pt;
        }
        cum[tid] = part;
        __syncthreads();
        if (tid == 0) {
            double run = 0.0;
            for (int i = 0; i < kTsThreads; ++i) { const double v = cum[i]; cum[i] = run; run += v; }
        }
        __syncthreads();
        double run = cum[tid];
        __syncthreads();
        for (int t = lo; t < hi; ++t) { run += p[t]; cum[t] = run; }
        __syncthreads();
    }
    if (p_out)
        for (int t = tid; t < T; t += kTsThreads) p_out[t] = cold ? uni : p[t];
    for (int b = tid; b < batch; b += kTsThreads) {
        int t;
        if (t_given) {
            t = t_given[b];
        } else {
            const Philox r = philox4x32_10((unsigned)b, 0u, (unsigned)draw, (unsigned)(draw >> 32), (unsigned)seed, (unsigned)(seed >> 32));
            const unsigned long long m = ((unsigned long long)r.c[0] << 21) | (unsigned long long)(r.c[1] >> 11);
            const double u = ((double)m + 0.5) * 1.1102230246251565404e-16;                      // 2^-53
            if (cold) {
                t = min((int)floor(u * (double)T), T - 1);
            } else {
                int a = 0, z = T;                                                                // first index whose prefix exceeds u
                while (a < z) { const int mid = (a + z) >> 1; if (cum[mid] > u) z = mid; else a = mid + 1; }
                t = min(a, T - 1);
            }
        }
        t_out[b] = t;
        iw_out[b] = cold ? 1.0 : 1.0 / ((double)T * p[min(max(t, 0), T - 1)]);
    }
}

// the level of entry i, or -1 when the entry is skipped (a loss or a level that is not finite, a level outside [0, T))
__device__ __forceinline__ int ts_entry_level(const double* __restrict__ entries, int i, int T) {
    const double tv = entries[2 * (size_t)i], l = entries[2 * (size_t)i + 1];
    if (!ts_finite(tv) || !ts_finite(l) || tv < 0.0 || tv >= (double)T) return -1;
    return (int)tv;
}

// One workgroup.  The first entry of every level (its leader) applies that level's entries in index order; rows of different levels
// share nothing, so the result is the one of a single walk over the list.
__global__ __launch_bounds__(kTsThreads) void tsampler_update_kernel(double* __restrict__ hist, int* __restrict__ count, int T, int H,
                                                                     const double* __restrict__ entries, int n) {
    for (int i = threadIdx.x; i < n; i += kTsThreads) {
        const int t = ts_entry_level(entries, i, T);
        if (t < 0) continue;
        bool leader = true;
        for (int j = 0; j < i && leader; ++j) leader = ts_entry_level(entries, j, T) != t;
        if (!leader) continue;
        double* row = hist + (size_t)t * H;
        int c = min(max(count[t], 0), H);
        for (int j = i; j < n; ++j) {
            if (ts_entry_level(entries, j, T) != t) continue;
            const double l = entries[2 * (size_t)j + 1];
            if (c == H) {
                for (int k = 0; k + 1 < H; ++k) row[k] = row[k + 1];
                row[H - 1] = l;
            } else {
                row[c++] = l;
            }
        }
        count[t] = c;
    }
}

// The plain loss per sample and its importance-weighted gradient in one pass (grid (vlb_blocks(), B), element quads guarded as in
// hybrid_loss_kernel): d = eps_hat - noise in fp32 as loss_kernel / loss_grad_kernel form it, |d| or d^2 added in double, one partial per
// workgroup by a fixed-order tree.  d_eps = loss_grad_kernel's expression with inv_count replaced by (float)iw_b * inv_count.
__global__ __launch_bounds__(256) void loss_weighted_kernel(const float* __restrict__ eps_hat, const float* __restrict__ noise,
                                                            const double* __restrict__ iw, float* __restrict__ d_eps,
                                                            double* __restrict__ partial, int Cc, long fhw, int l2, float inv_count, int vec) {
    __shared__ double red[256];
    const int b = blockIdx.y;
    const long per = (long)Cc * fhw;
    const size_t base = (size_t)b * per;
    const float f = iw ? (float)iw[b] * inv_count : inv_count;
    double acc = 0.0;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; 4 * q < per; q += (long)gridDim.x * blockDim.x) {
        const long i = 4 * q;
        float nv[4];
        if (vec) {
            const float4 n4 = *reinterpret_cast<const float4*>(noise + base + i);
            nv[0] = n4.x; nv[1] = n4.y; nv[2] = n4.z; nv[3] = n4.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) nv[k] = i + k < per ? noise[base + i + k] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long e = i + k;
            if (e >= per) continue;
            const long c = e / fhw, r = e - c * fhw;                                // [C,F,H,W] -> channel-last [F,H,W,C]
            const size_t j = base + (size_t)r * Cc + c;
            const float d = eps_hat[j] - nv[k];
            acc += l2 ? (double)d * (double)d : (double)fabsf(d);
            if (d_eps) d_eps[j] = l2 ? 2.0f * d * f : ((d > 0.f) - (d < 0.f)) * f;
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = red[0];
}

// One workgroup: thread b adds sample b's partials in index order -> out[b] = the sample's mean; thread 0 then adds iw_b out[b] over the
// samples in index order -> out[B] = (1 / B) sum_b iw_b l_b
__global__ __launch_bounds__(256) void loss_weighted_final_kernel(const double* __restrict__ partial, const double* __restrict__ iw,
                                                                  double* __restrict__ out, int B, int nblk, long per_sample) {
    __shared__ double tot[256];
    double run = 0.0;
    for (int b0 = 0; b0 < B; b0 += 256) {
        const int b = b0 + threadIdx.x;
        double l = 0.0;
        if (b < B) {
            double a = 0.0;
            for (int i = 0; i < nblk; ++i) a += partial[(size_t)b * nblk + i];
            l = a / (double)per_sample;
            out[b] = l;
            l = iw ? iw[b] * l : l;
        }
        tot[threadIdx.x] = l;
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < min(256, B - b0); ++i) run += tot[i];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[B] = run / (double)B;
}

size_t tsampler_draw_lds_bytes(int T) { return ((size_t)T + (size_t)std::max(T, kTsThreads)) * sizeof(double); }

hipError_t launch_tsampler_draw(const double* hist, const int* count, int T, int H, double eps, const int* t_given, unsigned long long seed,
                                unsigned long long draw, int* t_out, double* iw_out, double* p_out, int batch, hipStream_t st) {
    return LaunchScope(st, "tsampler_draw_kernel", 0.0, 8.0 * T * H, "T%d H%d B%d %s", T, H, batch, t_given ? "given" : "philox")
        .launch(tsampler_draw_kernel, dim3(1), dim3(kTsThreads), tsampler_draw_lds_bytes(T), hist, count, T, H, eps, t_given, seed, draw, t_out,
                iw_out, p_out, batch);
}

hipError_t launch_tsampler_update(double* hist, int* count, int T, int H, const double* entries, int n, hipStream_t st) {
    return LaunchScope(st, "tsampler_update_kernel", 0.0, 16.0 * n, "T%d H%d n%d", T, H, n)
        .launch(tsampler_update_kernel, dim3(1), dim3(kTsThreads), 0, hist, count, T, H, entries, n);
}

size_t loss_weighted_scratch_doubles(int B) { return (size_t)B * vlb_blocks(); }

hipError_t launch_loss_weighted(const float* eps_hat, const float* noise, const double* iw, float* d_eps, double* scratch, double* out, int B,
                                int Cc, long fhw, int l2, hipStream_t st) {
    const long per = (long)Cc * fhw, n = (long)B * per;
    const int vec = (per % 4 == 0) && ((uintptr_t)noise % 16 == 0);
    hipError_t e = LaunchScope(st, "loss_weighted_kernel", 0.0, (d_eps ? 12.0 : 8.0) * n, "B%d C%d fhw%ld l2 %d iw %d grad %d", B, Cc, fhw, l2,
                               iw ? 1 : 0, d_eps ? 1 : 0)
                       .launch(loss_weighted_kernel, dim3(vlb_blocks(), B), dim3(256), 0, eps_hat, noise, iw, d_eps, scratch, Cc, fhw, l2,
                               1.0f / (float)n, vec);
    if (e != hipSuccess) return e;
    return LaunchScope(st, "loss_weighted_final_kernel", 0.0, 0.0, "B%d", B)
        .launch(loss_weighted_final_kernel, dim3(1), dim3(256), 0, (const double*)scratch, iw, out, B, vlb_blocks(), per);
}

}  // namespace vdx
