// Self-conditioning (vdx.h: "Self-conditioning"; EXTENSION, no reference code: Chen et al. 2022, "Analog Bits", section 2.2).  The
// denoiser has channels = 2 C, out_dim = C; its input is xin [B,2C,F,H,W] = [ x_t | x0~ ] with x0~ its own previous estimate of x0
// (zero where there is none).
//   selfcond_x0 ... x0~ = clip(sqrt(1 / ac_t) x_t - sqrt(1 / ac_t - 1) eps_hat) written into planes [C, 2C) of xin: one streaming launch
//                   behind the forward (and behind v_to_eps / the dynamic threshold), so that the next forward reads it
#include "vdx_common.h"
#include "vdx_internal.h"

namespace vdx {

__device__ __forceinline__ bool sc_aligned16(const void* p) { return ((unsigned long long)p & 15ull) == 0; }

// Grid (x, B); a thread takes quads of four consecutive elements of its sample's [C,F,H,W], guarded element by element as
// lowres_input_kernel guards them: any per_sample, any C, sample bases off 16 bytes (the float4 forms only where the quad is whole and
// its address allows them).  eps is channel-last and indexed as p_sample_kernel indexes it.  The two products and the difference are
// rounded to fp32 one by one, whichever path an element takes: p_step_elem_rn's x0.
__global__ __launch_bounds__(256) void selfcond_x0_kernel(SelfcondArgs P) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int tb = min(max(P.t[b], 0), P.T - 1);
    const float k_recip = P.tables[tb], k_recipm1 = P.tables[P.T + tb];
    const float s = P.thres ? P.thres[b] : 1.0f;
    const int Cc = P.C;
    const long per = P.per_sample, fhw = per / Cc;
    const float* __restrict__ x = P.x + (size_t)b * P.x_pitch;
    const size_t base = (size_t)b * per;                            // the sample in eps [B,F,H,W,C]
    float* __restrict__ dst = P.xin + 2 * base + per;               // planes [C, 2C) of the sample's 2 C
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; 4 * q < per; q += (long)gridDim.x * blockDim.x) {
        const long i = 4 * q;
        const bool full = i + 3 < per;
        float xv[4], ev[4];
        if (full && sc_aligned16(x + i)) {
            const float4 x4 = *reinterpret_cast<const float4*>(x + i);
            xv[0] = x4.x; xv[1] = x4.y; xv[2] = x4.z; xv[3] = x4.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) xv[k] = i + k < per ? x[i + k] : 0.f;
        }
        if (Cc == 1 && full && sc_aligned16(P.eps + base + i)) {     // (channel-last is then x's own order)
            const float4 e4 = *reinterpret_cast<const float4*>(P.eps + base + i);
            ev[0] = e4.x; ev[1] = e4.y; ev[2] = e4.z; ev[3] = e4.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long e = i + k;
                ev[k] = 0.f;
                if (e < per) {
                    const long c = e / fhw, r = e - c * fhw;        // [C,F,H,W] -> channel-last [F,H,W,C]
                    ev[k] = P.eps[base + (size_t)r * Cc + c];
                }
            }
        }
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float t1 = k_recip * xv[k];
            const float t2 = k_recipm1 * ev[k];
            float x0 = t1 - t2;
            if (P.clip) x0 = fminf(fmaxf(x0, -s), s) / s;
            o[k] = x0;
        }
        if (full && sc_aligned16(dst + i)) *reinterpret_cast<float4*>(dst + i) = make_float4(o[0], o[1], o[2], o[3]);
        else for (int k = 0; k < 4 && i + k < per; ++k) dst[i + k] = o[k];
    }
}

hipError_t launch_selfcond_x0(const SelfcondArgs& a, int B, hipStream_t st) {
    return LaunchScope(st, "selfcond_x0_kernel", 0.0, 12.0 * B * a.per_sample, "B%d px%ld C%d pitch%ld clip %d thres %d", B, a.per_sample, a.C,
                       a.x_pitch, a.clip, a.thres ? 1 : 0)
        .launch(selfcond_x0_kernel, dim3(ew_blocks((a.per_sample + 3) / 4), B), dim3(256), 0, a);
}

}  // namespace vdx
