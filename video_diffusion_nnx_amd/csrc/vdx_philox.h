// The counter-based N(0,1) stream of the diffusion kernels (Philox4x32-10 + Box-Muller; restated for parity in oracle/philox_ref.py),
// shared by diffusion.hip and lowres.hip.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace vdx {

struct Philox { unsigned c[4]; };

__device__ __forceinline__ Philox philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned hi0 = (unsigned)(p0 >> 32), lo0 = (unsigned)p0, hi1 = (unsigned)(p1 >> 32), lo1 = (unsigned)p1;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    Philox o; o.c[0] = c0; o.c[1] = c1; o.c[2] = c2; o.c[3] = c3;
    return o;
}

// four normals of counter i of draw `offset` (see oracle/philox_ref.py for the exact definition)
__device__ __forceinline__ float4 randn4(unsigned long long i, unsigned long long seed, unsigned long long offset) {
    const Philox r = philox4x32_10((unsigned)i, (unsigned)(i >> 32), (unsigned)offset, (unsigned)(offset >> 32), (unsigned)seed, (unsigned)(seed >> 32));
    float u[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = ((float)(r.c[k] >> 8) + 0.5f) * 5.9604644775390625e-08f;   // 2^-24
    float4 z;
    const float r0 = sqrtf(-2.0f * logf(u[0])), r1 = sqrtf(-2.0f * logf(u[2]));
    float s0, c0, s1, c1;
    sincosf(6.283185307179586f * u[1], &s0, &c0);
    sincosf(6.283185307179586f * u[3], &s1, &c1);
    z.x = r0 * c0; z.y = r0 * s0; z.z = r1 * c1; z.w = r1 * s1;
    return z;
}

}  // namespace vdx
