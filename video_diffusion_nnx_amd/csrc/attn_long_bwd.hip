// Backward core of softmax(q k^T) v for sequences of MORE than 64 tokens (gfx950): the bottleneck spatial attention of frames larger than
// 64 x 64 (16 x 16 = 256 tokens at 128 x 128).  Same contract as attn_core_bwd_kernel (attn_bwd.hip) through AttnBwdArgs; L is a multiple
// of 64, 64 < L <= 640, so every 64-token query / key tile is whole and nothing is masked.
//
// Flash-attention backward with recompute, in three launches; every workgroup (256 threads = 4 waves, wave w owns 16 rows of its tile)
// owns its outputs, so there are no atomics and the output bits depend on the values only:
//   stats (sequence, head, query tile): walk the key tiles with an online softmax -> O, and per query row m = max_j s_j,
//                                       1 / sum_j exp(s_j - m) and delta = sum_d dO . O
//   dkv   (sequence, head, key tile)  : walk the query tiles; P^T = exp(S^T - m) / sum, dP^T = V dO^T, dS^T = P^T o (dP^T - delta);
//                                       dV += P^T dO, dK += dS^T q
//   dq    (sequence, head, query tile): walk the key tiles; the same P, dS in the other orientation; dQ += dS k
// The three row scalars live in the first three columns of the row's own 32-column dq slot of the head until the dq pass, which reads
// the scalars of its own rows before it stores dq there: no scratch, and the columns behind dq|dk|dv stay untouched.
// Arithmetic: fp32 operands on the matrix cores in every mode (v_mfma_f32_16x16x4_f32, exact fp32; lane (lp = lane & 15, q = lane >> 4)
// supplies A[lp][k = q] and B[k = q][lp], and holds D[4q + e][lp]); the operands are scalar LDS reads of padded tiles.
#include "vdx_common.h"
#include "vdx_internal.h"

namespace vdx {

constexpr int AL_LD = 36;            // floats per row of a [64 tokens][32] tile: 16-byte rows, conflict-free (row lp, k q) reads
constexpr int AL_LP = 68;            // floats per row of a [64][64] probability / dS tile
constexpr size_t AL_LDS_STATS = ((size_t)3 * 64 * AL_LD + 64 * AL_LP) * 4;                   // Q | K | V | P
constexpr size_t AL_LDS_DKV = ((size_t)4 * 64 * AL_LD + 2 * 64 * AL_LP + 3 * 64) * 4;        // K | V | Q | dO | P^T | dS^T | m, 1/sum, delta
constexpr size_t AL_LDS_DQ = ((size_t)4 * 64 * AL_LD + 64 * AL_LP + 3 * 64) * 4;             // Q | dO | K | V | dS | m, 1/sum, delta

// e^x for x <= 0.  x log2(e) is split into its rounded product and the residual (the rounding error of the product plus the low part of
// log2 e), which enters to first order: with logits of +-100 the plain exp2(x * log2e) is off by |x| 2^-24 in the exponent.
__device__ __forceinline__ float al_exp(float x) {
    x = fmaxf(x, -128.0f);                                               // e^-128 is 0 in fp32; keeps the residual finite
    const float L2E = 1.44269502162933350f, L2E_LO = 1.92596299e-8f;
    const float hi = x * L2E;
    const float lo = fmaf(x, L2E_LO, fmaf(x, L2E, -hi));
    const float e = __builtin_amdgcn_exp2f(hi);
    return fmaf(e, lo * 0.693147180559945f, e);
}

// tokens [t0, t0 + 64) of the sequence, 32 columns from src (already offset to the head's first column) -> tile [64][AL_LD], times mul
__device__ __forceinline__ void al_stage(float* dst, const float* src, size_t stride, long row0, long tok_p, int t0, float mul) {
    for (int i = threadIdx.x; i < 64 * 8; i += 256) {
        const int t = i >> 3, c = (i & 7) * 4;
        const size_t row = (size_t)(row0 + (long)(t0 + t) * tok_p);
        const float4 v = *reinterpret_cast<const float4*>(src + row * stride + c);
        *reinterpret_cast<float4*>(dst + t * AL_LD + c) = make_float4(v.x * mul, v.y * mul, v.z * mul, v.w * mul);
    }
}

// the three row scalars of tokens [t0, t0 + 64) from the rows' dq slots -> st [3][64]
__device__ __forceinline__ void al_stage_stats(float* st, const AttnBwdArgs& P, long row0, int t0, int h) {
    if (threadIdx.x < 64) {
        const size_t row = (size_t)(row0 + (long)(t0 + (int)threadIdx.x) * P.tok_p);
        const float* s = P.dq + row * P.dstride + h * 32;
        st[threadIdx.x] = s[0]; st[64 + threadIdx.x] = s[1]; st[128 + threadIdx.x] = s[2];
    }
}

// acc += A B^T over K: a = &A[lp][q], b = &B[lp][q], both with the reduction index contiguous
template <int K>
__device__ __forceinline__ void al_mma_nt(f32x4& acc, const float* a, const float* b) {
#pragma unroll
    for (int k = 0; k < K; k += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[k], b[k], acc, 0, 0, 0);
}
// acc += A B over K: a = &A[lp][q], b = &B[q][lp] with B rows of LDB floats
template <int K, int LDB>
__device__ __forceinline__ void al_mma_nn(f32x4& acc, const float* a, const float* b) {
#pragma unroll
    for (int k = 0; k < K; k += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[k], b[k * LDB], acc, 0, 0, 0);
}

struct AlGeo { long row0; int tile, h, nt, w, lp, q; };
__device__ __forceinline__ AlGeo al_geo(const AttnBwdArgs& P) {
    AlGeo g;
    g.nt = P.L >> 6;
    const long s = blockIdx.x / g.nt;
    g.tile = (int)(blockIdx.x - s * g.nt); g.h = blockIdx.y;
    g.row0 = (s / P.inner) * P.outer_p + (s % P.inner);
    const int lane = threadIdx.x & 63;
    g.w = threadIdx.x >> 6; g.lp = lane & 15; g.q = lane >> 4;
    return g;
}

__global__ __launch_bounds__(256) void attn_long_bwd_stats_kernel(AttnBwdArgs P) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* Qs = sm; float* Ks = Qs + 64 * AL_LD; float* Vs = Ks + 64 * AL_LD; float* Ps = Vs + 64 * AL_LD;
    const AlGeo g = al_geo(P);
    const int HD = P.heads * 32, w = g.w, lp = g.lp, q = g.q;
    const float* qb = P.qkv + g.h * 32;
    al_stage(Qs, qb, (size_t)3 * HD, g.row0, P.tok_p, g.tile * 64, P.scale);
    const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 o[2] = {z, z};
    float m[4] = {-3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f}, l[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < g.nt; ++j) {
        __syncthreads();                                                 // the previous tile's readers of K, V, P are done
        al_stage(Ks, qb + HD, (size_t)3 * HD, g.row0, P.tok_p, j * 64, 1.0f);
        al_stage(Vs, qb + 2 * HD, (size_t)3 * HD, g.row0, P.tok_p, j * 64, 1.0f);
        __syncthreads();
        f32x4 sc[4];                                                     // sc[c][e] = S[query 16w + 4q + e][key 16c + lp]
#pragma unroll
        for (int c = 0; c < 4; ++c) { sc[c] = z; al_mma_nt<32>(sc[c], Qs + (16 * w + lp) * AL_LD + q, Ks + (16 * c + lp) * AL_LD + q); }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float mx = max16(fmaxf(fmaxf(sc[0][e], sc[1][e]), fmaxf(sc[2][e], sc[3][e])));
            const float mn = fmaxf(m[e], mx), corr = al_exp(m[e] - mn);
            float sum = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float p = al_exp(sc[c][e] - mn);
                sum += p;
                Ps[(16 * w + 4 * q + e) * AL_LP + 16 * c + lp] = p;
            }
            l[e] = fmaf(l[e], corr, reduce16(sum));
            m[e] = mn; o[0][e] *= corr; o[1][e] *= corr;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 2; ++t) al_mma_nn<64, AL_LD>(o[t], Ps + (16 * w + lp) * AL_LP + q, Vs + q * AL_LD + 16 * t + lp);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float inv = 1.0f / l[e];
        const size_t row = (size_t)(g.row0 + (long)(g.tile * 64 + 16 * w + 4 * q + e) * P.tok_p);
        float dl = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const size_t o_ = row * HD + g.h * 32 + 16 * t + lp;
            const float ov = o[t][e] * inv;
            P.O[o_] = ov;
            dl = fmaf(P.dO[o_], ov, dl);
        }
        dl = reduce16(dl);
        if (lp == 0) { float* s = P.dq + row * P.dstride + g.h * 32; s[0] = m[e]; s[1] = inv; s[2] = dl; }
    }
}

__global__ __launch_bounds__(256) void attn_long_bwd_dkv_kernel(AttnBwdArgs P) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* Ks = sm; float* Vs = Ks + 64 * AL_LD; float* Qs = Vs + 64 * AL_LD; float* Ds = Qs + 64 * AL_LD;
    float* Pt = Ds + 64 * AL_LD; float* St = Pt + 64 * AL_LP; float* stat = St + 64 * AL_LP;
    const AlGeo g = al_geo(P);
    const int HD = P.heads * 32, w = g.w, lp = g.lp, q = g.q;
    const float* qb = P.qkv + g.h * 32;
    al_stage(Ks, qb + HD, (size_t)3 * HD, g.row0, P.tok_p, g.tile * 64, 1.0f);
    al_stage(Vs, qb + 2 * HD, (size_t)3 * HD, g.row0, P.tok_p, g.tile * 64, 1.0f);
    const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 dk[2] = {z, z}, dv[2] = {z, z};
    for (int i = 0; i < g.nt; ++i) {
        __syncthreads();                                                 // the previous tile's readers are done
        al_stage(Qs, qb, (size_t)3 * HD, g.row0, P.tok_p, i * 64, P.scale);
        al_stage(Ds, P.dO + g.h * 32, (size_t)HD, g.row0, P.tok_p, i * 64, 1.0f);
        al_stage_stats(stat, P, g.row0, i * 64, g.h);
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 4; ++c) {                                    // [key 16w + 4q + e][query 16c + lp]
            f32x4 s = z, dp = z;
            al_mma_nt<32>(s, Ks + (16 * w + lp) * AL_LD + q, Qs + (16 * c + lp) * AL_LD + q);
            al_mma_nt<32>(dp, Vs + (16 * w + lp) * AL_LD + q, Ds + (16 * c + lp) * AL_LD + q);
            const float mm = stat[16 * c + lp], inv = stat[64 + 16 * c + lp], dl = stat[128 + 16 * c + lp];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float p = al_exp(s[e] - mm) * inv;
                Pt[(16 * w + 4 * q + e) * AL_LP + 16 * c + lp] = p;
                St[(16 * w + 4 * q + e) * AL_LP + 16 * c + lp] = p * (dp[e] - dl);
            }
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            al_mma_nn<64, AL_LD>(dv[t], Pt + (16 * w + lp) * AL_LP + q, Ds + q * AL_LD + 16 * t + lp);
            al_mma_nn<64, AL_LD>(dk[t], St + (16 * w + lp) * AL_LP + q, Qs + q * AL_LD + 16 * t + lp);      // (Qs holds scale * q)
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const size_t row = (size_t)(g.row0 + (long)(g.tile * 64 + 16 * w + 4 * q + e) * P.tok_p);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const size_t g_ = row * P.dstride + g.h * 32 + 16 * t + lp;
            P.dk[g_] = dk[t][e]; P.dv[g_] = dv[t][e];
        }
    }
}

__global__ __launch_bounds__(256) void attn_long_bwd_dq_kernel(AttnBwdArgs P) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* Qs = sm; float* Ds = Qs + 64 * AL_LD; float* Ks = Ds + 64 * AL_LD; float* Vs = Ks + 64 * AL_LD;
    float* Ss = Vs + 64 * AL_LD; float* stat = Ss + 64 * AL_LP;
    const AlGeo g = al_geo(P);
    const int HD = P.heads * 32, w = g.w, lp = g.lp, q = g.q;
    const float* qb = P.qkv + g.h * 32;
    al_stage(Qs, qb, (size_t)3 * HD, g.row0, P.tok_p, g.tile * 64, P.scale);
    al_stage(Ds, P.dO + g.h * 32, (size_t)HD, g.row0, P.tok_p, g.tile * 64, 1.0f);
    al_stage_stats(stat, P, g.row0, g.tile * 64, g.h);                   // read here, before this workgroup stores dq over them
    const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 dq[2] = {z, z};
    for (int j = 0; j < g.nt; ++j) {
        __syncthreads();
        al_stage(Ks, qb + HD, (size_t)3 * HD, g.row0, P.tok_p, j * 64, 1.0f);
        al_stage(Vs, qb + 2 * HD, (size_t)3 * HD, g.row0, P.tok_p, j * 64, 1.0f);
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 4; ++c) {                                    // [query 16w + 4q + e][key 16c + lp]
            f32x4 s = z, dp = z;
            al_mma_nt<32>(s, Qs + (16 * w + lp) * AL_LD + q, Ks + (16 * c + lp) * AL_LD + q);
            al_mma_nt<32>(dp, Ds + (16 * w + lp) * AL_LD + q, Vs + (16 * c + lp) * AL_LD + q);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = 16 * w + 4 * q + e;
                const float p = al_exp(s[e] - stat[r]) * stat[64 + r];
                Ss[r * AL_LP + 16 * c + lp] = p * (dp[e] - stat[128 + r]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 2; ++t) al_mma_nn<64, AL_LD>(dq[t], Ss + (16 * w + lp) * AL_LP + q, Ks + q * AL_LD + 16 * t + lp);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const size_t row = (size_t)(g.row0 + (long)(g.tile * 64 + 16 * w + 4 * q + e) * P.tok_p);
#pragma unroll
        for (int t = 0; t < 2; ++t) P.dq[row * P.dstride + g.h * 32 + 16 * t + lp] = dq[t][e] * P.scale;
    }
}

bool attn_bwd_long_served(int L) { return L > 64 && L <= 640 && L % 64 == 0; }

hipError_t launch_attn_core_bwd_long(const AttnBwdArgs& a, hipStream_t st) {
    if (!attn_bwd_long_served(a.L) || a.bias || a.focus || a.io_bf16 || a.nseq < 1 || a.heads < 1 || a.heads > 65535) return hipErrorInvalidValue;
    const long nt = a.L / 64;
    if (a.nseq >= (1L << 31) / nt) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(a.nseq * nt), (unsigned)a.heads);
    const double mm = 2.0 * a.nseq * a.heads * (double)a.L * a.L * 32, el = (double)a.nseq * a.L * a.heads * 32 * 4;     // one L x L x 32 product; one tensor
    hipError_t e = LaunchScope(st, "attn_long_bwd_stats_kernel", 2 * mm, 5 * el + 2 * el * (double)nt, "L%d nseq%ld heads%d", a.L, a.nseq, a.heads)
                       .launch(attn_long_bwd_stats_kernel, grid, dim3(256), AL_LDS_STATS, a);
    if (e != hipSuccess) return e;
    e = LaunchScope(st, "attn_long_bwd_dkv_kernel", 4 * mm, 4 * el + 2 * el * (double)nt, "L%d nseq%ld heads%d", a.L, a.nseq, a.heads)
            .launch(attn_long_bwd_dkv_kernel, grid, dim3(256), AL_LDS_DKV, a);
    if (e != hipSuccess) return e;
    return LaunchScope(st, "attn_long_bwd_dq_kernel", 3 * mm, 3 * el + 2 * el * (double)nt, "L%d nseq%ld heads%d", a.L, a.nseq, a.heads)
        .launch(attn_long_bwd_dq_kernel, grid, dim3(256), AL_LDS_DQ, a);
}

}  // namespace vdx
