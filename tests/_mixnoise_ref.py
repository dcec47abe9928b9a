"""The mixed noise prior (vdx.h: "Mixed noise"; Ge et al. 2023, "Preserve Your Own Correlation", sec. 3.2) restated on the CPU for
tests/test_host_mixnoise.py and tests/test_gpu_mixnoise.py: z = a s + b e over [B,C,F,H,W] with s shared by the frames of a clip, both
components oracle/philox_ref.py's stream (composed here, not restated).  Nothing in this module needs a GPU or libvdx.  A plain module:
nothing here is collected."""
import functools

import numpy as np
import torch

from oracle import philox_ref
from oracle.diffusion_ref import DiffusionRef, schedule

DRAW_SHARED = 1 << 60                            # VDX_DRAW_SHARED


def coef64(alpha):
    """(a, b) = (alpha, 1) / sqrt(1 + alpha^2) in double."""
    h = float(np.hypot(1.0, float(alpha)))
    return float(alpha) / h, 1.0 / h


def coef32(alpha):
    """The two weights rounded once to fp32: what the kernels receive."""
    a, b = coef64(alpha)
    return np.float32(a), np.float32(b)


def rho(alpha):
    return float(alpha) ** 2 / (1.0 + float(alpha) ** 2)


@functools.lru_cache(None)
def components(shape, seed, draw, dtype=np.float32):
    """(s [B,C,1,H,W], e [B,C,F,H,W]) of draw `draw`: e is randn's element of the whole tensor, s the stream's draw DRAW_SHARED + draw
    indexed as randn would index a [B,C,H,W] tensor.  Computed once per argument set and left unchanged."""
    B, C, Fr, H, W = shape
    assert 0 <= draw < DRAW_SHARED
    e = philox_ref.randn(B * C * Fr * H * W, seed, draw, dtype).reshape(shape)
    s = philox_ref.randn(B * C * H * W, seed, DRAW_SHARED + draw, dtype).reshape(B, C, 1, H, W)
    return s, e


def mixed_randn(shape, seed, draw, alpha):
    """The definition in fp32 numpy: the two products and the sum rounded one by one."""
    a, b = coef32(alpha)
    s, e = components(tuple(shape), seed, draw)
    return (a * s).astype(np.float32) + (b * e).astype(np.float32)


def mixed_randn64(shape, seed, draw, alpha):
    """The same in fp64 (the stream's uniforms through fp64 log / cos / sin), with the fp32 weights the kernels receive, widened."""
    a, b = (float(v) for v in coef32(alpha))
    s, e = components(tuple(shape), seed, draw, np.float64)
    return a * s + b * e


def frame_covariance(frames, alpha):
    """Sigma = b^2 I + a^2 1 1^T over the frames, fp64."""
    a, b = coef64(alpha)
    return b * b * np.eye(frames) + a * a * np.ones((frames, frames))


def ancestral_chain64(denoise, x_T, zs, *, image_size, num_frames, channels, timesteps):
    """The ancestral chain in fp64 from x_T with the list zs of per-step noise tensors (step k, t = T - 1 - k, uses zs[k]):
    oracle DiffusionRef.p_sample_loop, so (x_0 + 1) / 2."""
    ref = DiffusionRef(denoise, image_size=image_size, num_frames=num_frames, channels=channels, timesteps=timesteps, dtype=torch.float64)
    with torch.no_grad():
        return ref.p_sample_loop(x_T.double(), [z.double() for z in zs])


def posterior_step_covariance(T, t, cov_xt, cov_z):
    """Cov(x_{t-1}) over the frames of one pixel for x_{t-1} = coef2_t x_t + sqrt(beta~_t) z -- the ancestral step with x0 = 0 and the
    exact posterior mean -- from Cov(x_t) and Cov(z), in fp64 with the fp64 schedule.  Returns (covariance, schedule)."""
    s = schedule(T, np.float64)
    c2, pv = s['posterior_mean_coef2'][t], s['posterior_variance'][t]
    return c2 * c2 * cov_xt + pv * cov_z, s
