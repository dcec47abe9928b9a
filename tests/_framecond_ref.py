"""fp64 restatements of frame-conditioned training and clean-context sampling (EXTENSION: RaMViD, Hoeppe et al. 2022; no reference
code), written from the contracts in include/vdx.h on top of oracle.diffusion_ref.DiffusionRef, oracle.unet3d_ref and
oracle.philox_ref: the masked q_sample, the masked loss and its gradient, the masked p_losses, and the three masked chains with the
known region kept clean.  A plain module: nothing here is collected."""
import numpy as np
import torch

import _dpm_ref as D
from oracle import philox_ref, unet3d_ref as R  # noqa: F401  (R: the UNet oracle, for the tests that import it from here)
from oracle.diffusion_ref import DiffusionRef, extract  # noqa: F401


def z(shape, seed, draw):
    return torch.from_numpy(philox_ref.randn(int(np.prod(shape)), seed, draw)).double().reshape(tuple(shape))


def expand(mask, shape):
    """[F] / [B,F] / element mask -> bool [B,C,F,H,W]."""
    m = torch.as_tensor(mask) != 0
    B, _, Fr, _, _ = shape
    if m.dim() == 1:
        m = m.reshape(1, 1, Fr, 1, 1)
    elif m.dim() == 2:
        m = m.reshape(B, 1, Fr, 1, 1)
    return m.expand(*shape)


def q_sample_masked(ref, x0n, t, noise, m):
    """m ? x0n : sqrt_ac[t] x0n + sqrt(1 - ac[t]) noise; x0n is the normalised clip."""
    return torch.where(m, x0n, ref.q_sample(x0n, t, noise))


def loss_sum_count(pred, noise, m, l2):
    """(sum, count) over the mask-0 elements; pred channel-first like noise."""
    d = (pred - noise)[~m]
    return ((d * d).sum() if l2 else d.abs().sum()), int((~m).sum())


def masked_mean(pred, noise, m, l2):
    s, n = loss_sum_count(pred, noise, m, l2)
    return s / max(n, 1)


def loss_grad(pred, noise, m, l2):
    """d masked_mean / d pred (channel-first), by hand: 2 d / n or sign(d) / n off the mask, 0 on it."""
    n = max(int((~m).sum()), 1)
    d = pred - noise
    g = 2 * d / n if l2 else torch.sign(d) / n
    return torch.where(m, torch.zeros_like(g), g)


def p_losses(ref, x, t, noise, m):
    """GaussianDiffusion.__call__ / p_losses with a frame mask and explicit t / noise: x in [0, 1], m bool [B,C,F,H,W] or None (the
    reference objective)."""
    x0n = x * 2 - 1
    x_in = ref.q_sample(x0n, t, noise) if m is None else q_sample_masked(ref, x0n, t, noise, m)
    pred = ref.denoise(x_in, t).permute(0, 4, 1, 2, 3)
    l2 = ref.loss_type == 'l2'
    if m is None:
        return ((pred - noise) ** 2).mean() if l2 else (pred - noise).abs().mean()
    return masked_mean(pred, noise, m, l2)


# ---- clean-context chains: the masked loops of vdx.h with the known region equal to `known` at the start and after every step ----

def clean_loop(ref, video, m, seed):
    """Ancestral chain: x = m ? k : x_T, then per step x = m ? k : p_sample(x, Philox(seed, 1 + s))."""
    T, shape = ref.num_timesteps, tuple(video.shape)
    k, m = 2 * video.double() - 1, m.bool()
    x = torch.where(m, k, z(shape, seed, 0))
    for s, i in enumerate(reversed(range(T))):
        x = torch.where(m, k, ref.p_sample(x, torch.full((shape[0],), i), z(shape, seed, 1 + s)))
    return (x + 1) / 2


def clean_ddim(ref, video, m, seed, S):
    T, shape = ref.num_timesteps, tuple(video.shape)
    seq = D.time_sequence(T, S)
    ac = ref.tab['alphas_cumprod']
    k, m = 2 * video.double() - 1, m.bool()
    x = torch.where(m, k, z(shape, seed, 0))
    for j in range(S):
        t, tn = int(seq[j]), int(seq[j + 1])
        eps = ref.denoise(x, torch.full((shape[0],), t)).permute(0, 4, 1, 2, 3)
        a_t = ac[t]
        a_n = ac[tn] if tn >= 0 else torch.ones((), dtype=ac.dtype)
        x0 = ((x - (1 - a_t).sqrt() * eps) / a_t.sqrt()).clamp(-1, 1)
        xp = a_n.sqrt() * x0 + (1 - a_n).sqrt() * (x - a_t.sqrt() * x0) / (1 - a_t).sqrt()
        x = torch.where(m, k, xp)
    return (x + 1) / 2


def clean_dpm(ref, video, m, seed, S, order=2):
    shape = tuple(video.shape)
    seq = D.time_sequence(ref.num_timesteps, S)
    ac = ref.tab['alphas_cumprod']
    k, m = 2 * video.double() - 1, m.bool()
    x = torch.where(m, k, z(shape, seed, 0))
    hist = None
    for j in range(S):
        t = int(seq[j])
        eps = ref.denoise(x, torch.full((shape[0],), t)).permute(0, 4, 1, 2, 3)
        xp, hist = D.dpm_step(x, eps, hist, ac, seq, j, order, True, None)
        x = torch.where(m, k, xp)
    return (x + 1) / 2
