// Temporally correlated noise prior (gfx950; EXTENSION, no reference code: Ge et al. 2023, "Preserve Your Own Correlation", sec. 3.2, the
// mixed noise model).  Over a [B,C,F,H,W] tensor
//   z[b,c,f,h,w] = a s[b,c,h,w] + b e[b,c,f,h,w],   s, e ~ N(0, 1),   a^2 + b^2 = 1
// so every element is N(0, 1) and two frames of one clip correlate with a^2 at the same pixel.  Both components are the project's Philox
// stream (vdx_philox.h): e is element (b, c, f, hw) of draw d of the [B,C,F,H,W] tensor, exactly vdx_randn's; s is element (b, c, hw) of
// draw VDX_DRAW_SHARED + d of the [B,C,H,W] tensor, indexed as vdx_randn would index it.  The two products and the sum are rounded on
// their own, so the result is the fp32 expression a * S + b * E over vdx_randn's two tensors bit for bit.
//
//   randn_mixed ......... the tensor itself (q_sample's eps, x_T)
//   p_sample_mixed ...... p_sample_kernel with z generated in the kernel that way (the ancestral step of the mixed chain)
#include "vdx_common.h"
#include "vdx_internal.h"
#include "vdx_philox.h"
#include "vdx_pstep.h"

namespace vdx {

// (plain operators under contract(off), as cfg_g of diffusion.hip: no fused multiply-add, packed or not)
__device__ __forceinline__ float mix_elem(float a, float s, float b, float e) {
#pragma clang fp contract(off)
    const float p = a * s;
    const float q = b * e;
    return p + q;
}

__device__ __forceinline__ float lane_of(const float4& z, unsigned lane) {
    return lane == 0 ? z.x : lane == 1 ? z.y : lane == 2 ? z.z : z.w;
}

// s[k] = the shared normal of element i0 + k (k < 4, i0 % 4 == 0) of the whole [B*C][F][hw] tensor of n elements; elements at or past n
// get 0.  fhw = F * hw.  Element (bc, f, p) reads element j = bc * hw + p of the shared tensor: counter j / 4, lane j % 4.  With
// hw % 4 == 0 the four elements lie in one frame and are one quad of the shared tensor: one Philox evaluation.  Otherwise a quad may
// straddle frames or channels and up to four counters are evaluated; the values are the same function of (j, seed, draw) on both paths.
__device__ __forceinline__ void shared4(float (&s)[4], long i0, long n, long fhw, long hw, bool quad_aligned, unsigned long long seed,
                                        unsigned long long draw) {
    if (quad_aligned) {
        const long bc = i0 / fhw, r = i0 - bc * fhw;
        const long j = bc * hw + r % hw;
        const float4 z = randn4((unsigned long long)(j >> 2), seed, draw);
        s[0] = z.x; s[1] = z.y; s[2] = z.z; s[3] = z.w;
        return;
    }
    unsigned long long have = ~0ull;
    float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long i = i0 + k;
        s[k] = 0.f;
        if (i >= n) continue;
        const long bc = i / fhw, r = i - bc * fhw;
        const long j = bc * hw + r % hw;
        const unsigned long long ctr = (unsigned long long)(j >> 2);
        if (ctr != have) { z = randn4(ctr, seed, draw); have = ctr; }
        s[k] = lane_of(z, (unsigned)(j & 3));
    }
}

__global__ __launch_bounds__(256) void randn_mixed_kernel(float* __restrict__ out, long n, long fhw, long hw, float a, float b,
                                                          unsigned long long seed, unsigned long long draw,
                                                          const unsigned long long* __restrict__ dev_draw) {
    if (dev_draw) draw += *dev_draw;
    const bool quad_aligned = (hw & 3) == 0;
    const long nq = (n + 3) / 4;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long)gridDim.x * blockDim.x) {
        const float4 e = randn4((unsigned long long)q, seed, draw);
        float s[4];
        shared4(s, 4 * q, n, fhw, hw, quad_aligned, seed, VDX_DRAW_SHARED + draw);
        const float v[4] = {mix_elem(a, s[0], b, e.x), mix_elem(a, s[1], b, e.y), mix_elem(a, s[2], b, e.z), mix_elem(a, s[3], b, e.w)};
        if (4 * q + 3 < n) *reinterpret_cast<float4*>(out + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
        else { for (int k = 0; 4 * q + k < n; ++k) out[4 * q + k] = v[k]; }
    }
}

// one reverse step with z = a s + b e drawn here: p_sample_kernel's arithmetic (p_step_coef and p_step_elem_rn, p_step_elem in the
// roundings p_sample_kernel is compiled to; the same affine), the noise of randn_mixed_kernel at draw P.offset + *P.dev_offset.  per_sample % 4 == 0; float4 x / out (they may alias: every thread reads its
// quad before it writes it); P.noise is not read.
__global__ __launch_bounds__(256) void p_sample_mixed_kernel(PSampleArgs P, MixArgs M) {
    const int b = blockIdx.y;
    const PStepCoef kc = p_step_coef(P, b, P.t[b]);
    unsigned long long off = P.offset;
    if (P.dev_offset) off += *P.dev_offset;
    const long per = P.per_sample, fhw = P.per_sample / P.C;
    const long n = (long)gridDim.y * per;
    const bool quad_aligned = (M.hw & 3) == 0;
    const size_t base = (size_t)b * per;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; 4 * q < per; q += (long)gridDim.x * blockDim.x) {
        const long i = 4 * q;
        const float4 x4 = *reinterpret_cast<const float4*>(P.x + base + i);
        const float xv[4] = {x4.x, x4.y, x4.z, x4.w};
        float ev[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long e = i + k, c = e / fhw, r = e - c * fhw;                 // [C,F,H,W] -> channel-last [F,H,W,C]
            ev[k] = P.eps[base + r * P.C + c];
        }
        const float4 z = randn4((unsigned long long)(base / 4 + q), P.seed, off);   // element index of the whole tensor
        const float zv[4] = {z.x, z.y, z.z, z.w};
        float s[4];
        shared4(s, (long)base + i, n, fhw, M.hw, quad_aligned, P.seed, VDX_DRAW_SHARED + off);
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float v = p_step_elem_rn(kc, xv[k], ev[k], mix_elem(M.a, s[k], M.b, zv[k]));
            o[k] = fmaf(P.post_scale, v, P.post_shift);
        }
        *reinterpret_cast<float4*>(P.out + base + i) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------

hipError_t launch_randn_mixed(float* out, int B, int C, const MixArgs& m, unsigned long long seed, unsigned long long draw,
                              const unsigned long long* dev_draw, hipStream_t st) {
    const long fhw = (long)m.F * m.hw, n = (long)B * C * fhw;
    return LaunchScope(st, "randn_mixed_kernel", 0.0, 4.0 * n, "B%d C%d F%d hw%ld", B, C, m.F, m.hw)
        .launch(randn_mixed_kernel, dim3(ew_blocks((n + 3) / 4)), dim3(256), 0, out, n, fhw, m.hw, m.a, m.b, seed, draw, dev_draw);
}

hipError_t launch_p_sample_mixed(const PSampleArgs& a, const MixArgs& m, int B, hipStream_t st) {
    return LaunchScope(st, "p_sample_mixed_kernel", 0.0, 12.0 * B * a.per_sample, "B%d px%ld F%d", B, a.per_sample, m.F)
        .launch(p_sample_mixed_kernel, dim3(ew_blocks(a.per_sample / 4), B), dim3(256), 0, a, m);
}

}  // namespace vdx
