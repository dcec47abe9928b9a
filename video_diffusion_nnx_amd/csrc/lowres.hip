// Cascaded super-resolution (gfx950): the device work around a denoiser with channels = 2 C, out_dim = C whose input is
// xin [B,2C,F,S,S] = [ x_t | u ], u = aug(up(2 lo - 1)) with lo [B,C,F/ft,S/fs,S/fs] in [0, 1] the low-resolution clip
// (vdx.h: "Cascaded super-resolution"; EXTENSION, no reference code: Ho et al. 2021, "Cascaded Diffusion Models").
//
//   lowres_down ...... box mean of a clip over ft x fs x fs blocks: the training pair's low-resolution half
//   lowres_input ..... one pass that writes both halves of xin: planes [0, C) = q_sample's expression on x0, planes [C, 2C) = the
//                      upsampled, optionally noise-augmented low-resolution clip (x0 == NULL: the second half alone, for sampling)
//   lowres_pack ...... img [B,C,F,S,S] -> planes [0, C) of xin: the first launch of a captured super-resolution sampling step
// up = separable linear interpolation with half-pixel centres and clamped neighbours (torch's trilinear, align_corners=False).
#include "vdx_common.h"
#include "vdx_internal.h"
#include "vdx_philox.h"

namespace vdx {

// the two taps and the weight of the second one for output index d of an axis upsampled by `factor` from `in` entries:
// src = (d + 0.5) / factor - 0.5 = num / (2 factor) with num = 2 d + 1 - factor, floored in integers; the weight is rounded once
struct LerpTap { int i0, i1; float w1; };

__device__ __forceinline__ LerpTap lerp_tap(int d, int factor, int in) {
    const int num = 2 * d + 1 - factor, den = 2 * factor;
    LerpTap l;
    l.i0 = num > 0 ? num / den : 0;
    l.w1 = num > 0 ? (float)(num - den * l.i0) / (float)den : 0.f;
    l.i1 = min(l.i0 + 1, in - 1);
    return l;
}

// (explicit fmaf here and below: the contraction does not depend on what the vectoriser pairs up, so every path writes the same bits)
__device__ __forceinline__ float lerp2(float a, float b, float w1) { return fmaf(w1, b, (1.0f - w1) * a); }

// q_sample_kernel's expression as its float4 body compiles: fma(a, x0 pre_scale + pre_shift, s n) with s n rounded
__device__ __forceinline__ float q_elem(float a, float s, float x, float n, float pre_scale, float pre_shift) {
    return fmaf(a, fmaf(x, pre_scale, pre_shift), s * n);
}

// up(2 lo - 1) at (f, r, w) of one [f_in, s_in, s_in] plane: normalise, then columns, rows, frames
__device__ __forceinline__ float lowres_up(const float* __restrict__ plane, int s_in, const LerpTap& tf, const LerpTap& tr, const LerpTap& tw) {
    float vf[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const float* fr = plane + (long)(a ? tf.i1 : tf.i0) * s_in * s_in;
        float vr[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float* row = fr + (long)(c ? tr.i1 : tr.i0) * s_in;
            vr[c] = lerp2(fmaf(row[tw.i0], 2.0f, -1.0f), fmaf(row[tw.i1], 2.0f, -1.0f), tw.w1);
        }
        vf[a] = lerp2(vr[0], vr[1], tr.w1);
    }
    return lerp2(vf[0], vf[1], tf.w1);
}

__device__ __forceinline__ bool aligned16(const void* p) { return ((unsigned long long)p & 15ull) == 0; }

// One pass over both halves of xin.  Grid (x, B); a thread takes quads of four consecutive elements (along W) of its sample, guarded
// element by element as p_sample_kernel guards them: any per_sample, any S, sample bases off 16 bytes (the float4 forms only where the
// address allows them).  The augmentation noise is Philox(seed, draw) over the element index of [B,C,F,S,S] as randn_kernel lays it out
// (quad e / 4, lane e % 4), so a sample whose base is no multiple of 4 reads its four normals from two neighbouring counters.
__global__ __launch_bounds__(256) void lowres_input_kernel(LowresArgs P) {
    const int b = blockIdx.y;
    const int S = P.S, F = P.F, s_in = S / P.fs, f_in = F / P.ft;
    const long hw = (long)S * S, fhw = (long)F * hw, per = (long)P.C * fhw;
    const long lo_plane = (long)f_in * s_in * s_in;
    const size_t base = (size_t)b * per;                            // the sample in [B,C,F,S,S]
    float* __restrict__ row = P.xin + 2 * base;                     // its 2 C planes
    const float* __restrict__ lo_b = P.lo + (size_t)b * P.C * lo_plane;
    float qa = 0.f, qs = 0.f;
    if (P.x0) { const int tb = min(max(P.t[b], 0), P.T - 1); qa = P.sqrt_ac[tb]; qs = P.sqrt_1mac[tb]; }
    const int sb = P.aug ? min(P.aug[b], P.T - 1) : -1;            // < 0: no augmentation, u = up exactly
    float ga = 1.f, gb = 0.f;
    if (sb >= 0) { ga = P.sqrt_ac[sb]; gb = P.sqrt_1mac[sb]; }
    const unsigned sh = (unsigned)(base & 3);
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; 4 * q < per; q += (long)gridDim.x * blockDim.x) {
        const long i = 4 * q;
        const bool full = i + 3 < per;
        if (P.x0) {
            // x_t = a (x0 pre_scale + pre_shift) + s noise, vdx_q_sample's bits (q_elem)
            const float* x0 = P.x0 + base + i;
            const float* nz = P.noise + base + i;
            float* o = row + i;
            if (full && aligned16(x0) && aligned16(nz) && aligned16(o)) {
                const float4 x = *reinterpret_cast<const float4*>(x0);
                const float4 n = *reinterpret_cast<const float4*>(nz);
                float4 v;
                v.x = q_elem(qa, qs, x.x, n.x, P.pre_scale, P.pre_shift); v.y = q_elem(qa, qs, x.y, n.y, P.pre_scale, P.pre_shift);
                v.z = q_elem(qa, qs, x.z, n.z, P.pre_scale, P.pre_shift); v.w = q_elem(qa, qs, x.w, n.w, P.pre_scale, P.pre_shift);
                *reinterpret_cast<float4*>(o) = v;
            } else {
                for (int k = 0; k < 4 && i + k < per; ++k) o[k] = q_elem(qa, qs, x0[k], nz[k], P.pre_scale, P.pre_shift);
            }
        }
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (sb >= 0) {
            const unsigned long long ctr = (unsigned long long)((base + i) >> 2);
            const float4 za = randn4(ctr, P.seed, P.draw);
            float zz[8] = {za.x, za.y, za.z, za.w, 0.f, 0.f, 0.f, 0.f};
            if (sh) { const float4 zb = randn4(ctr + 1, P.seed, P.draw); zz[4] = zb.x; zz[5] = zb.y; zz[6] = zb.z; zz[7] = zb.w; }
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = k; j < k + 4; ++j) if ((unsigned)j == sh + k) z[k] = zz[j];      // (selects: no indexed private array)
        }
        // (c, f, r, w) of the quad's first element, then stepped along W with carries
        int c = (int)(i / fhw);
        long rem = i - (long)c * fhw;
        int f = (int)(rem / hw);
        rem -= (long)f * hw;
        int r = (int)(rem / S), w = (int)(rem - (long)r * S);
        float u[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i + k < per) {
                const float up = lowres_up(lo_b + (long)c * lo_plane, s_in, lerp_tap(f, P.ft, f_in), lerp_tap(r, P.fs, s_in), lerp_tap(w, P.fs, s_in));
                u[k] = sb >= 0 ? fmaf(ga, up, gb * z[k]) : up;
            }
            if (++w == S) { w = 0; if (++r == S) { r = 0; if (++f == F) { f = 0; ++c; } } }
        }
        float* o = row + per + i;
        if (full && aligned16(o)) *reinterpret_cast<float4*>(o) = make_float4(u[0], u[1], u[2], u[3]);
        else for (int k = 0; k < 4 && i + k < per; ++k) o[k] = u[k];
    }
}

// lo[b,c,fo,ro,wo] = mean of x over the ft x fs x fs block: fp32 sum in (frame, row, column) order, one multiply by 1 / n
// (ft = fs = 1: the input's bits)
__global__ __launch_bounds__(256) void lowres_down_kernel(const float* __restrict__ x, float* __restrict__ lo, long n_out, int F, int S, int ft,
                                                          int fs, float inv_n) {
    const int s_out = S / fs, f_out = F / ft;
    for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < n_out; o += (long)gridDim.x * blockDim.x) {
        const int wo = (int)(o % s_out);
        long rest = o / s_out;
        const int ro = (int)(rest % s_out);
        rest /= s_out;
        const int fo = (int)(rest % f_out);
        const long bc = rest / f_out;
        const float* src = x + ((bc * F + (long)fo * ft) * S + (long)ro * fs) * S + (long)wo * fs;
        float acc = 0.f;
        for (int df = 0; df < ft; ++df)
            for (int dr = 0; dr < fs; ++dr)
                for (int dc = 0; dc < fs; ++dc) {
                    const float v = src[((long)df * S + dr) * S + dc];
                    acc = (df | dr | dc) ? acc + v : v;
                }
        lo[o] = acc * inv_n;
    }
}

// xin[b, 0 : per] = img[b, :] (row pitch 2 per); planes [C, 2C) of xin are not touched.  vec: per % 4 == 0 and both bases 16-byte aligned
__global__ __launch_bounds__(256) void lowres_pack_kernel(const float* __restrict__ img, float* __restrict__ xin, long per, int vec) {
    const float* src = img + (size_t)blockIdx.y * per;
    float* dst = xin + 2 * (size_t)blockIdx.y * per;
    const long stride = (long)gridDim.x * blockDim.x, first = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (vec) {
        for (long q = first; 4 * q < per; q += stride) reinterpret_cast<float4*>(dst)[q] = reinterpret_cast<const float4*>(src)[q];
    } else {
        for (long i = first; i < per; i += stride) dst[i] = src[i];
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------

static int lr_blocks(long work_items) { return (int)std::max<long>(1, std::min<long>((work_items + 255) / 256, 2048)); }

hipError_t launch_lowres_down(const float* x, float* lo, int B, int C, int F, int S, int ft, int fs, hipStream_t st) {
    const long n_out = (long)B * C * (F / ft) * (S / fs) * (S / fs), n_in = (long)B * C * F * S * S;
    return LaunchScope(st, "lowres_down_kernel", 0.0, 4.0 * (n_in + n_out), "B%d C%d F%d S%d ft%d fs%d", B, C, F, S, ft, fs)
        .launch(lowres_down_kernel, dim3(lr_blocks(n_out)), dim3(256), 0, x, lo, n_out, F, S, ft, fs, 1.0f / (float)(ft * fs * fs));
}

hipError_t launch_lowres_input(const LowresArgs& a, int B, hipStream_t st) {
    const long per = (long)a.C * a.F * a.S * a.S;
    return LaunchScope(st, "lowres_input_kernel", 0.0, (a.x0 ? 16.0 : 4.0) * B * per, "B%d C%d F%d S%d ft%d fs%d %s%s", B, a.C, a.F, a.S, a.ft,
                       a.fs, a.x0 ? "q_sample+up" : "up", a.aug ? " aug" : "")
        .launch(lowres_input_kernel, dim3(lr_blocks((per + 3) / 4), B), dim3(256), 0, a);
}

hipError_t launch_lowres_pack(const float* img, float* xin, int B, long per_sample, hipStream_t st) {
    const int vec = per_sample % 4 == 0 && (uintptr_t)img % 16 == 0 && (uintptr_t)xin % 16 == 0;
    return LaunchScope(st, "lowres_pack_kernel", 0.0, 8.0 * B * per_sample, "B%d px%ld %s", B, per_sample, vec ? "float4" : "scalar")
        .launch(lowres_pack_kernel, dim3(lr_blocks(vec ? per_sample / 4 : per_sample), B), dim3(256), 0, img, xin, per_sample, vec);
}

}  // namespace vdx
