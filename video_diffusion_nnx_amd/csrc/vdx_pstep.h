// The per-element arithmetic of one ancestral reverse step, shared by p_sample_kernel and p_sample_masked_kernel (diffusion.hip) and
// p_sample_mixed_kernel (mixnoise.hip).  Device code only.
#pragma once
#include "vdx_internal.h"

namespace vdx {

struct PStepCoef { float k_recip, k_recipm1, c1, c2, sigma, s; int clip; };

__device__ __forceinline__ PStepCoef p_step_coef(const PSampleArgs& P, int b, int tb) {
    PStepCoef k;
    k.k_recip = P.tables[tb]; k.k_recipm1 = P.tables[P.T + tb];
    k.c1 = P.tables[2 * P.T + tb]; k.c2 = P.tables[3 * P.T + tb];
    k.sigma = (tb == 0) ? 0.f : expf(0.5f * P.tables[4 * P.T + tb]);
    k.s = P.thres ? P.thres[b] : 1.0f;
    k.clip = P.clip;
    return k;
}

__device__ __forceinline__ float p_step_elem(const PStepCoef& k, float x, float eps, float z) {
    float x0 = k.k_recip * x - k.k_recipm1 * eps;                      // predict_start_from_noise  (:133-136)
    if (k.clip) x0 = fminf(fmaxf(x0, -k.s), k.s) / k.s;                 // :220
    const float mean = k.c1 * x0 + k.c2 * x;                           // q_posterior (:153-156)
    return mean + k.sigma * z;                                         // :261
}

// p_step_elem with every rounding spelled out, in the order p_sample_kernel is compiled to (lv_step_elem of diffusion.hip states the
// same order): the two products of x0, c2 x and sigma z are rounded on their own, only c1 x0 + (c2 x) is fused.  For a kernel whose z is
// not a load -- p_sample_mixed_kernel forms it in registers -- the compiler would otherwise fuse sigma z into the sum, and that kernel has
// to give p_sample_kernel's bits on the same z.
__device__ __forceinline__ float p_step_elem_rn(const PStepCoef& k, float x, float eps, float z) {
#pragma clang fp contract(off)
    const float t1 = k.k_recip * x;
    const float t2 = k.k_recipm1 * eps;
    float x0 = t1 - t2;
    if (k.clip) x0 = fminf(fmaxf(x0, -k.s), k.s) / k.s;
    const float m2 = k.c2 * x;
    const float mean = fmaf(k.c1, x0, m2);
    const float sz = k.sigma * z;
    return sz + mean;
}

}  // namespace vdx
