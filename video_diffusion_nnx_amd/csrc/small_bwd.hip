// Small backward kernels (gfx950): final 1x1 conv, init 7x7 conv weight gradient, time-embedding MLPs.
// Autodiff of unet3d.py:110-115,128-133,251,288-298 and modules.py:202-208,233-238 (reference trainer.py:361).
#include "vdx_common.h"
#include "vdx_internal.h"

namespace vdx {

// final conv: dx[pix][c] = sum_co dout[pix][co] W[c][co]
__global__ __launch_bounds__(256) void final_conv_dx_kernel(const float* __restrict__ dout, const float* __restrict__ w, float* __restrict__ dx,
                                                            long npix, int D, int Cout) {
    const long n4 = npix * (D / 4);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const long pix = i / (D / 4);
        const int c = (int)(i % (D / 4)) * 4;
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        for (int co = 0; co < Cout; ++co) {
            const float d = dout[pix * Cout + co];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = fmaf(d, w[(size_t)(c + e) * Cout + co], o[e]);
        }
        *reinterpret_cast<float4*>(dx + pix * D + c) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// final conv: dW[c][co] += sum_pix x[pix][c] dout[pix][co] ; db[co] += sum_pix dout[pix][co]     (D <= 256, Cout <= NCO)
// part (deterministic mode): this workgroup's sums go to part[blockIdx.x][D * Cout] and, behind all of those, [blockIdx.x][Cout]
// NCO = 4 is the text the kernel always had (Cout <= 4: the same bits); NCO = 6 serves the eps | v head of a learned-variance network at C = 3
template <int NCO>
__global__ __launch_bounds__(256) void final_conv_dw_kernel(const float* __restrict__ x, const float* __restrict__ dout, float* __restrict__ dW,
                                                            float* __restrict__ db, long npix, int D, int Cout, int x_bf16, float* __restrict__ part) {
    __shared__ float red[256 * 4];
    const int c = threadIdx.x % D, pl = threadIdx.x / D, PL = 256 / D;
    float acc[NCO] = {}, accb[NCO] = {};
    if (pl < PL) {
        // 8 pixels per pass, every load issued before the first use (one dependent load per pass was a 128-step latency chain: 112 us)
        const long stride = (long)gridDim.x * PL;
        for (long pix0 = (long)blockIdx.x * PL + pl; pix0 < npix; pix0 += stride * 8) {
            float xv[8], dv[8][NCO];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const long pix = pix0 + u * stride;
                const bool ok = pix < npix;
                const long pe = ok ? pix : 0;
                xv[u] = x_bf16 ? __uint_as_float((unsigned)reinterpret_cast<const unsigned short*>(x)[pe * D + c] << 16) : x[pe * D + c];
                if (!ok) xv[u] = 0.f;
                for (int co = 0; co < NCO; ++co) dv[u][co] = (ok && co < Cout) ? dout[pe * Cout + co] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                for (int co = 0; co < NCO; ++co) { acc[co] = fmaf(xv[u], dv[u][co], acc[co]); accb[co] += dv[u][co]; }
        }
    }
    for (int co = 0; co < Cout; ++co) {
        __syncthreads();
        red[threadIdx.x] = (pl < PL) ? acc[co] : 0.f;
        __syncthreads();
        if (pl == 0) {
            float t = 0.f;
            for (int k = 0; k < PL; ++k) t += red[k * D + c];
            if (part) part[(size_t)blockIdx.x * D * Cout + (size_t)c * Cout + co] = t;
            else atomicAdd(dW + (size_t)c * Cout + co, t);
        }
        if (!part) { if (c == 0 && pl < PL) atomicAdd(db + co, accb[co]); }
        else {
            __syncthreads();
            if (c == 0 && pl < PL) red[pl] = accb[co];
            __syncthreads();
            if (threadIdx.x == 0) {
                float t = 0.f;
                for (int k = 0; k < PL; ++k) t += red[k];
                part[(size_t)gridDim.x * D * Cout + (size_t)blockIdx.x * Cout + co] = t;
            }
        }
    }
}

// init conv weight gradient: x external [B,Cin,F,H,W]; dy channel-last [B,F,H,W,Cout]; dW Flax (K,K,Cin,Cout); db [Cout]
// part (deterministic mode): slot = (frame, tile); dW slots [slot][K * K * Cin * Cout], bias slots behind them [slot][Cout]
__global__ __launch_bounds__(256) void init_conv_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dW,
                                                              float* __restrict__ db, int B, int Cin, int F, int H, int W, int Cout, int K, float* __restrict__ part) {
    extern __shared__ float sm[];
    const int pad = K / 2, TW = 16 + K - 1;
    float* xs = sm;                               // [Cin][TW][TW]
    float* ds = sm + Cin * TW * TW;               // [256][17]
    const int tx = blockIdx.x % ((W + 15) / 16), ty = blockIdx.x / ((W + 15) / 16);
    const int f = blockIdx.y % F, b = blockIdx.y / F;
    const int co0 = blockIdx.z * 16;
    for (int i = threadIdx.x; i < Cin * TW * TW; i += 256) {
        const int c = i / (TW * TW), r = i % (TW * TW);
        const int gy = ty * 16 + r / TW - pad, gx = tx * 16 + r % TW - pad;
        xs[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? x[((((size_t)b * Cin + c) * F + f) * H + gy) * W + gx] : 0.f;
    }
    for (int i = threadIdx.x; i < 256 * 16; i += 256) {
        const int p = i >> 4, j = i & 15;
        const int oy = ty * 16 + (p >> 4), ox = tx * 16 + (p & 15);
        ds[p * 17 + j] = (oy < H && ox < W && co0 + j < Cout) ? dy[((((size_t)b * F + f) * H + oy) * W + ox) * Cout + co0 + j] : 0.f;
    }
    __syncthreads();
    const int nout = K * K * Cin * 16;
    for (int o = threadIdx.x; o < nout; o += 256) {
        const int j = o & 15, r = o >> 4;
        const int c = r % Cin, tap = r / Cin;
        const int ky = tap / K, kx = tap % K;
        float acc = 0.f;
        for (int p = 0; p < 256; ++p) acc = fmaf(xs[(c * TW + (p >> 4) + ky) * TW + (p & 15) + kx], ds[p * 17 + j], acc);
        if (co0 + j < Cout) {
            if (part) part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * ((size_t)K * K * Cin * Cout) + ((size_t)tap * Cin + c) * Cout + co0 + j] = acc;
            else atomicAdd(dW + ((size_t)tap * Cin + c) * Cout + co0 + j, acc);
        }
    }
    if (threadIdx.x < 16 && co0 + threadIdx.x < Cout) {
        float t = 0.f;
        for (int p = 0; p < 256; ++p) t += ds[p * 17 + threadIdx.x];
        if (part) part[(size_t)gridDim.y * gridDim.x * ((size_t)K * K * Cin * Cout) + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * Cout + co0 + threadIdx.x] = t;
        else atomicAdd(db + co0 + threadIdx.x, t);
    }
}

__device__ __forceinline__ float dsilu2_f(float z) {
    const float sg = 1.0f / (1.0f + __expf(-z));
    return sg * (1.0f + z * (1.0f - sg));
}

// per-ResnetBlock time MLP backward, first half: the LayerNorm.  grid = nlayers.  dss (in: d(scale|shift), overwritten by d(lin)) laid
// out like ss.  lin = the forward's pre-LayerNorm values.  N <= 2048 (8 columns per thread), as in resblock_ss_norm_kernel.
__global__ __launch_bounds__(256) void resblock_ss_bwd_kernel(const float* __restrict__ params, float* __restrict__ grads, const float* __restrict__ temb,
                                                              const SsLayer* __restrict__ layers, const float* __restrict__ lin_base,
                                                              float* __restrict__ dss_base, float* __restrict__ dtemb, int temb_dim, int B) {
    __shared__ float red[16];
    const int tid = threadIdx.x;
    const SsLayer L = layers[blockIdx.x];
    const int N = L.n;
    const float* g = params + L.g_off;
    float* db = grads + L.b_off; float* dg = grads + L.g_off; float* dbe = grads + L.be_off;
    const float* lin = lin_base + (size_t)L.out_off * B;
    float* dss = dss_base + (size_t)L.out_off * B;
    // this workgroup owns the layer's parameters: their gradients are summed over the samples in registers (sample order, from 0) and
    // added to grads ONCE at the end -- no atomics, and a call on grads that already hold a value adds exactly the sum a call on zeros stores
    float adg[8], adbe[8], adb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) adg[j] = adbe[j] = adb[j] = 0.f;
    // LayerNorm backward per sample (in place: dss <- dlin)
    for (int b = 0; b < B; ++b) {
        float s = 0.f, ss = 0.f;
        for (int n = tid; n < N; n += 256) { const float v = lin[(size_t)b * N + n]; s += v; ss += v * v; }
        for (int o = 1; o < 64; o <<= 1) { s += __shfl_xor(s, o); ss += __shfl_xor(ss, o); }
        __syncthreads();
        if ((tid & 63) == 0) { red[tid >> 6] = s; red[4 + (tid >> 6)] = ss; }
        __syncthreads();
        s = red[0] + red[1] + red[2] + red[3]; ss = red[4] + red[5] + red[6] + red[7];
        const float mean = s / N, rstd = rsqrtf(fmaxf(ss / N - mean * mean, 0.f) + NORM_EPS);
        float m1 = 0.f, m2 = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int n = tid + 256 * j;
            if (n < N) {
                const float xh = (lin[(size_t)b * N + n] - mean) * rstd, d = dss[(size_t)b * N + n], gd = g[n] * d;
                m1 += gd; m2 += gd * xh;
                adg[j] += d * xh; adbe[j] += d;
            }
        }
        for (int o = 1; o < 64; o <<= 1) { m1 += __shfl_xor(m1, o); m2 += __shfl_xor(m2, o); }
        __syncthreads();
        if ((tid & 63) == 0) { red[8 + (tid >> 6)] = m1; red[12 + (tid >> 6)] = m2; }
        __syncthreads();
        m1 = (red[8] + red[9] + red[10] + red[11]) / N; m2 = (red[12] + red[13] + red[14] + red[15]) / N;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int n = tid + 256 * j;
            if (n < N) {
                const float xh = (lin[(size_t)b * N + n] - mean) * rstd;
                const float dl = rstd * (g[n] * dss[(size_t)b * N + n] - m1 - xh * m2);
                dss[(size_t)b * N + n] = dl;
                adb[j] += dl;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int n = tid + 256 * j;
        if (n < N) { dg[n] += adg[j]; dbe[n] += adbe[j]; db[n] += adb[j]; }
    }
}

// second half of the time-MLP backward, parallel over (layer, KB rows of the Linear): with dlin from the kernel above
//   dW[k][n] += sum_b SiLU(temb[b][k]) dlin[b][n]          (coalesced over n)
//   dtemb[b][k] += SiLU'(temb[b][k]) sum_n dlin[b][n] W[k][n]   (workgroup reduction over n, one atomic per (b, k))
// part (deterministic mode): layer l writes its d(temb) contribution to part[l][B][temb_dim]; the launcher adds the layers in order
__global__ __launch_bounds__(256) void resblock_ss_bwd_w_kernel(const float* __restrict__ params, float* __restrict__ grads, const float* __restrict__ temb,
                                                                const SsLayer* __restrict__ layers, const float* __restrict__ dss_base,
                                                                float* __restrict__ dtemb, int temb_dim, int B, int SS_KB, float* __restrict__ part) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const SsLayer L = layers[blockIdx.x];
    const int N = L.n;
    const float* W = params + L.w_off;
    float* dW = grads + L.w_off;
    const float* dlin = dss_base + (size_t)L.out_off * B;
    for (int kk = 0; kk < SS_KB; ++kk) {
        const int k = blockIdx.y * SS_KB + kk;
        if (k >= temb_dim) break;
        for (int n = tid; n < N; n += 256) {
            float acc = 0.f;
            for (int b = 0; b < B; ++b) acc = fmaf(silu_f(temb[(size_t)b * temb_dim + k]), dlin[(size_t)b * N + n], acc);
            dW[(size_t)k * N + n] += acc;                       // this workgroup owns rows k of this layer: no atomics
        }
        for (int b = 0; b < B; ++b) {
            float acc = 0.f;
            for (int n = tid; n < N; n += 256) acc = fmaf(dlin[(size_t)b * N + n], W[(size_t)k * N + n], acc);
            for (int o = 1; o < 64; o <<= 1) acc += __shfl_xor(acc, o);
            __syncthreads();
            if ((tid & 63) == 0) red[tid >> 6] = acc;
            __syncthreads();
            if (tid == 0) {
                const float v = (red[0] + red[1] + red[2] + red[3]) * dsilu2_f(temb[(size_t)b * temb_dim + k]);
                if (part) part[((size_t)blockIdx.x * B + b) * temb_dim + k] = v;
                else atomicAdd(dtemb + (size_t)b * temb_dim + k, v);
            }
        }
    }
}

__device__ __forceinline__ float gelu_tanh_b(float x) {
    return 0.5f * x * (1.0f + tanhf(0.7978845608028654f * (x + 0.044715f * x * x * x)));
}
__device__ __forceinline__ float dgelu_tanh_b(float x) {
    const float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
    const float t = tanhf(u);
    return 0.5f * (1.0f + t) + 0.5f * x * (1.0f - t * t) * 0.7978845608028654f * (1.0f + 3.0f * 0.044715f * x * x);
}

// time MLP backward: workgroup s owns the 64-wide slice [64 s, 64 s + 64) of the hidden dimension (columns of W2 / rows of its
// transpose / columns of W1).  Every workgroup recomputes emb / lin1 / h of all samples into LDS (tiny); the batch reduction
// happens in registers, so each weight gets ONE global "+=".
__global__ __launch_bounds__(256) void time_mlp_bwd_kernel(TimeMlpArgs P, const float* __restrict__ dtemb, float* __restrict__ dw1, float* __restrict__ db1,
                                                           float* __restrict__ dw2, float* __restrict__ db2, float* __restrict__ dnull, int B) {
    extern __shared__ float sm[];                  // emb[B][dim] | lin1[B][td] | h[B][td] | dl1[B][64]
    const int tid = threadIdx.x, half = P.dim / 2, td = P.time_dim, dim = P.dim;
    float* emb = sm; float* lin1 = emb + (size_t)B * dim; float* h = lin1 + (size_t)B * td; float* dl1 = h + (size_t)B * td;
    const int n0 = blockIdx.x * 64;
    for (int i = tid; i < B * half; i += 256) {
        const int b = i / half, j = i - b * half;
        const float fr = expf((float)j * -(logf(10000.0f) / (float)(half - 1)));
        const float arg = (float)P.time[b] * fr;
        emb[b * dim + j] = sinf(arg); emb[b * dim + half + j] = cosf(arg);
    }
    __syncthreads();
    for (int i = tid; i < B * td; i += 256) {
        const int b = i / td, n = i - b * td;
        float acc = P.b1[n];
        // (8 weight loads in flight per pass: one dependent L2 round trip per k made this loop a 64-step latency chain on 4 workgroups)
        for (int k0 = 0; k0 < dim; k0 += 8) {
            float wv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) wv[u] = (k0 + u < dim) ? P.w1[(size_t)(k0 + u) * td + n] : 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) if (k0 + u < dim) acc = fmaf(emb[b * dim + k0 + u], wv[u], acc);
        }
        lin1[i] = acc; h[i] = gelu_tanh_b(acc);
    }
    __syncthreads();
    const int col = tid & 63, part = tid >> 6;      // 4 parts
    {   // dW2[k][n] += sum_b h_b[k] dt_b[n],  db2[n] += sum_b dt_b[n]      for n = n0 + col
        const int n = n0 + col;
        if (n < td) {
            const int kper = (td + 3) / 4;
            const int k1 = min(td, (part + 1) * kper);
            for (int k0 = part * kper; k0 < k1; k0 += 8) {             // 8 read-modify-writes of dW2 in flight
                float old[8], acc[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { old[u] = (k0 + u < k1) ? dw2[(size_t)(k0 + u) * td + n] : 0.f; acc[u] = 0.f; }
                for (int b = 0; b < B; ++b) {
                    const float dt = dtemb[(size_t)b * P.temb_dim + n];
#pragma unroll
                    for (int u = 0; u < 8; ++u) if (k0 + u < k1) acc[u] = fmaf(h[b * td + k0 + u], dt, acc[u]);
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) if (k0 + u < k1) dw2[(size_t)(k0 + u) * td + n] = old[u] + acc[u];
            }
            if (part == 0) { float acc = 0.f; for (int b = 0; b < B; ++b) acc += dtemb[(size_t)b * P.temb_dim + n]; db2[n] += acc; }
        }
    }
    // dl1[b][k] = (sum_n dt_b[n] W2[k][n]) * gelu'(lin1_b[k])      for k = n0 + 0..63: wave `part` takes 16 rows k, a row of W2 is read ONCE
    // by the whole wave (lane = n: coalesced) for all samples, the dot products are reduced with shuffles.  (First form: one thread per k
    // walking its own row -- 256 dependent, uncoalesced loads per thread: 244 us for 0.3 MFLOP on the critical path of the stem stage.)
    {
        const int lane = tid & 63;
        for (int kk = 0; kk < 16; ++kk) {
            const int kc = part * 16 + kk, k = n0 + kc;
            if (k >= td) break;                                       // (wave-uniform)
            for (int b = 0; b < B; ++b) {
                const float* dt = dtemb + (size_t)b * P.temb_dim;
                float acc = 0.f;
                for (int n = lane; n < td; n += 64) acc = fmaf(dt[n], P.w2[(size_t)k * td + n], acc);
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
                if (lane == 0) dl1[b * 64 + kc] = acc * dgelu_tanh_b(lin1[b * td + k]);
            }
        }
        for (int i = tid; i < B * 64; i += 256) if (n0 + (i & 63) >= td) dl1[i] = 0.f;      // columns beyond the hidden width
    }
    __syncthreads();
    {   // db1[k] += sum_b dl1_b[k],  dW1[j][k] += sum_b emb_b[j] dl1_b[k]
        const int k = n0 + col;
        if (k < td) {
            if (part == 0) { float acc = 0.f; for (int b = 0; b < B; ++b) acc += dl1[b * 64 + col]; db1[k] += acc; }
            const int jper = (dim + 3) / 4;
            for (int j = part * jper; j < min(dim, (part + 1) * jper); ++j) {
                float acc = 0.f;
                for (int b = 0; b < B; ++b) acc = fmaf(emb[b * dim + j], dl1[b * 64 + col], acc);
                dw1[(size_t)j * td + k] += acc;
            }
        }
    }
    if (blockIdx.x == 0 && P.cond_dim && dnull)
        for (int n = tid; n < P.cond_dim; n += 256) {
            float acc = 0.f;
            for (int b = 0; b < B; ++b) {
                const bool use_null = P.cond_mask ? (P.cond_mask[b] != 0) : (P.null_all != 0);
                if (use_null) acc += dtemb[(size_t)b * P.temb_dim + td + n];
            }
            dnull[n] += acc;
        }
}

hipError_t launch_final_conv_bwd(const float* x, const float* dout, const float* w, float* dx, float* dW, float* db, long npix, int D, int Cout, int x_bf16, hipStream_t st, float* part, size_t part_cap) {
    if (D > 256 || Cout > 6) return hipErrorInvalidValue;
    const int blocks = (int)std::max<long>(1, std::min<long>((npix * (D / 4) + 255) / 256, 4096));
    hipError_t e = LaunchScope(st, "final_conv_dx_kernel", 0.0, 0.0, "D%d Cout%d npix%ld", D, Cout, npix).launch(final_conv_dx_kernel, dim3(blocks), dim3(256), 0, dout, w, dx, npix, D, Cout);
    if (e != hipSuccess) return e;
    const int PL = 256 / D;
    const int b2 = (int)std::max<long>(1, std::min<long>((npix + PL - 1) / PL, 512));
    part = slots_if_fit(part, (size_t)b2 * (D + 1) * Cout, part_cap);
    e = LaunchScope(st, "final_conv_dw_kernel", 0.0, 0.0, "<x16 %d> D%d Cout%d npix%ld slots%d det %d", x_bf16, D, Cout, npix, b2, part ? 1 : 0)
                       .launch(Cout <= 4 ? final_conv_dw_kernel<4> : final_conv_dw_kernel<6>, dim3(b2), dim3(256), 0, x, dout, dW, db, npix, D, Cout, x_bf16, part);
    if (e != hipSuccess || !part) return e;
    return launch_slot_sum_dw_db(part, b2, (long)D * Cout, Cout, 0, {dW, nullptr, nullptr}, {db, nullptr, nullptr}, st);
}

hipError_t launch_init_conv_wgrad(const float* x, const float* dy, float* dW, float* db, int B, int Cin, int F, int H, int W, int Cout, int K, hipStream_t st, float* part, size_t part_cap) {
    const int TW = 16 + K - 1;
    dim3 grid(((W + 15) / 16) * ((H + 15) / 16), B * F, (Cout + 15) / 16);
    const size_t lds = ((size_t)Cin * TW * TW + 256 * 17) * 4;
    const size_t E = (size_t)K * K * Cin * Cout, nslots = (size_t)grid.x * grid.y;
    part = slots_if_fit(part, nslots * (E + Cout), part_cap);
    hipError_t e = LaunchScope(st, "init_conv_wgrad_kernel", 0.0, 0.0, "conv%dx%d %d->%d %dx%dx%d slots%zu det %d", K, K, Cin, Cout, B * F, H, W, nslots, part ? 1 : 0)
                       .launch(init_conv_wgrad_kernel, grid, dim3(256), lds, x, dy, dW, db, B, Cin, F, H, W, Cout, K, part);
    if (e != hipSuccess || !part) return e;
    return launch_slot_sum_dw_db(part, (int)nslots, (long)E, Cout, 0, {dW, nullptr, nullptr}, {db, nullptr, nullptr}, st);
}

hipError_t launch_resblock_ss_bwd(const float* params, float* grads, const float* temb, const SsLayer* layers, int nlayers, const float* lin_base,
                                  float* dss_base, float* dtemb, int temb_dim, int B, hipStream_t st, float* part, size_t part_cap) {
    hipError_t e = LaunchScope(st, "resblock_ss_bwd_kernel", 0.0, 0.0, "layers%d temb%d B%d", nlayers, temb_dim, B)
                       .launch(resblock_ss_bwd_kernel, dim3(nlayers), dim3(256), 0, params, grads, temb, layers, lin_base, dss_base, dtemb, temb_dim, B);
    if (e != hipSuccess) return e;
    // rows of the Linear per workgroup: the per-stage launches of the staged backward cover 2 layers each (data-parallel bucket
    // readiness, model_bwd.hip ss_bwd), so they take one row per workgroup to still fill the chip
    const int kb = nlayers >= 8 ? 8 : 1;
    part = slots_if_fit(part, (size_t)nlayers * B * temb_dim, part_cap);
    e = LaunchScope(st, "resblock_ss_bwd_w_kernel", 0.0, 0.0, "layers%d temb%d B%d kb%d det %d", nlayers, temb_dim, B, kb, part ? 1 : 0)
            .launch(resblock_ss_bwd_w_kernel, dim3(nlayers, (temb_dim + kb - 1) / kb), dim3(256), 0, params, grads, temb, layers, dss_base, dtemb, temb_dim, B, kb, part);
    if (e != hipSuccess || !part) return e;
    return launch_slot_sum(part, nlayers, (size_t)B * temb_dim, (long)B * temb_dim, temb_dim, 0, dtemb, nullptr, nullptr, st);
}

hipError_t launch_time_mlp_bwd(const TimeMlpArgs& a, const float* dtemb, float* dw1, float* db1, float* dw2, float* db2, float* dnull, int B, hipStream_t st) {
    const size_t lds = (size_t)B * (a.dim + 2 * a.time_dim + 64) * 4;
    if (lds > 150 * 1024) return hipErrorInvalidValue;             // B <= ~60 at the N shape
    return LaunchScope(st, "time_mlp_bwd_kernel", 0.0, 0.0, "dim%d time_dim%d cond%d B%d", a.dim, a.time_dim, a.cond_dim, B)
        .launch(time_mlp_bwd_kernel, dim3((a.time_dim + 63) / 64), dim3(256), lds, a, dtemb, dw1, db1, dw2, db2, dnull, B);
}

}  // namespace vdx
