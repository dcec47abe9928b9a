"""GaussianDiffusion -- host-side mirror of the reference class (/root/reference/gaussian_diffusion.py:23-502).

Same constructor / method surface; `key` arguments are integer seeds of the library's counter-based
Philox stream (JAX PRNGKeys are not reproducible outside JAX).  The heavy methods
(q_sample, p_sample, p_sample_loop, p_losses, __call__) run hand-written HIP through libvdx.so; the
closed-form accessors (q_mean_variance, predict_start_from_noise, q_posterior) are table look-ups.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from . import timestep_sampler as TS
from .unet3d import Unet3D

_vp = C.c_void_p
_u64 = C.c_uint64
vdx_randn = L._sig('vdx_randn', C.c_int, [_vp, C.c_long, _u64, _u64, _vp, _vp])
vdx_q_sample = L._sig('vdx_q_sample', C.c_int, [_vp] * 6 + [C.c_int, C.c_long, C.c_float, C.c_float, _vp])
vdx_p_sample_step = L._sig('vdx_p_sample_step', C.c_int, [_vp] * 5 + [C.c_int, _vp, _u64, _u64, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_long, _vp])
vdx_loss_sum = L._sig('vdx_loss_sum', C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_long, C.c_int, _vp])
vdx_q_sample_masked = L._sig('vdx_q_sample_masked', C.c_int, [_vp] * 7 + [C.c_int, C.c_long, C.c_float, C.c_float, _vp])
vdx_loss_masked_scratch_doubles = L._sig('vdx_loss_masked_scratch_doubles', C.c_size_t, [])
vdx_loss_sum_masked = L._sig('vdx_loss_sum_masked', C.c_int, [_vp] * 5 + [C.c_int, C.c_int, C.c_long, C.c_int, _vp])
vdx_affine = L._sig('vdx_affine', C.c_int, [_vp, _vp, C.c_long, C.c_float, C.c_float, _vp])
vdx_p_sample_loop = L._sig('vdx_p_sample_loop', C.c_int, [_vp] * 8 + [C.c_int, C.c_int, _vp, _u64, C.c_int, _vp, C.c_size_t, C.c_int, C.c_int, _vp])
vdx_p_sample_loop_dyn = L._sig('vdx_p_sample_loop_dyn', C.c_int, [_vp] * 8 + [C.c_int, C.c_int, _vp, _u64, C.c_int, C.c_float, _vp, _vp, C.c_size_t,
                                                                 C.c_int, C.c_int, _vp])
vdx_dynamic_threshold = L._sig('vdx_dynamic_threshold', C.c_int, [_vp] * 4 + [C.c_int, C.c_float, _vp, C.c_int, C.c_int, C.c_long, _vp])
vdx_ddim_step = L._sig('vdx_ddim_step', C.c_int, [_vp] * 7 + [C.c_int, C.c_int, C.c_int, C.c_long, _vp])
vdx_ddim_sample_loop = L._sig('vdx_ddim_sample_loop', C.c_int, [_vp] * 9 + [C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_size_t, C.c_int, C.c_int, _vp])
vdx_ddim_sample_loop_dyn = L._sig('vdx_ddim_sample_loop_dyn', C.c_int, [_vp] * 9 + [C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_float, _vp, _vp, C.c_size_t,
                                                                       C.c_int, C.c_int, _vp])
vdx_inpaint_init = L._sig('vdx_inpaint_init', C.c_int, [_vp] * 4 + [C.c_int, C.c_int, C.c_long, _vp])
vdx_p_sample_step_masked = L._sig('vdx_p_sample_step_masked', C.c_int, [_vp] * 5 + [C.c_int, _vp, _vp, _vp, C.c_int, _u64, _u64, _vp, _vp, C.c_int,
                                                                             C.c_int, C.c_int, C.c_long, _vp])
vdx_p_sample_loop_masked = L._sig('vdx_p_sample_loop_masked', C.c_int, [_vp] * 8 + [C.c_int, C.c_int, _vp, _u64, C.c_int, C.c_float, _vp, _vp, _vp, _vp,
                                                                             C.c_int, _vp, C.c_size_t, C.c_int, C.c_int, _vp])
vdx_ddim_step_masked = L._sig('vdx_ddim_step_masked', C.c_int, [_vp] * 7 + [C.c_int] + [_vp] * 3 + [C.c_int, _u64, C.c_int, C.c_int, C.c_long, _vp])
vdx_ddim_sample_loop_masked = L._sig('vdx_ddim_sample_loop_masked', C.c_int, [_vp] * 9 + [C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_float]
                                     + [_vp] * 4 + [_u64, _vp, C.c_size_t, C.c_int, C.c_int, _vp])
vdx_dpm_step = L._sig('vdx_dpm_step', C.c_int, [_vp] * 8 + [C.c_int, C.c_int, C.c_int, C.c_int, C.c_long, _vp])
vdx_dpm_step_masked = L._sig('vdx_dpm_step_masked', C.c_int, [_vp] * 8 + [C.c_int, C.c_int] + [_vp] * 3 + [C.c_int, _u64, C.c_int, C.c_int, C.c_long, _vp])
vdx_dpm_sample_loop = L._sig('vdx_dpm_sample_loop', C.c_int, [_vp] * 10 + [C.c_int, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, C.c_float, _vp, _vp,
                                                             C.c_size_t, C.c_int, C.c_int, _vp])
vdx_dpm_sample_loop_masked = L._sig('vdx_dpm_sample_loop_masked', C.c_int, [_vp] * 10 + [C.c_int, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, C.c_float]
                                    + [_vp] * 4 + [_u64, _vp, C.c_size_t, C.c_int, C.c_int, _vp])


vdx_loss_grad = L._sig('vdx_loss_grad', C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_long, C.c_int, _vp])
vdx_loss_grad_masked = L._sig('vdx_loss_grad_masked', C.c_int, [_vp] * 5 + [C.c_int, C.c_int, C.c_long, C.c_int, _vp])


# The loop entry points by (chain, variant): fourteen of the library's sixteen (the other two, vdx_p_sample_loop and vdx_ddim_sample_loop,
# are the plain _dyn entries with percentile 0).  'mixed' and 'lv' exist for the ancestral chain only; the two deterministic chains
# change under the mixed prior in x_T alone and run their plain / guided entries.
_LOOPS = {('ddpm', 'plain'): vdx_p_sample_loop_dyn, ('ddpm', 'masked'): vdx_p_sample_loop_masked, ('ddpm', 'guided'): L.vdx_p_sample_loop_guided,
          ('ddpm', 'mixed'): L.vdx_p_sample_loop_mixed, ('ddpm', 'sr'): L.vdx_p_sample_loop_sr, ('ddpm', 'lv'): L.vdx_p_sample_loop_lv,
          ('ddim', 'plain'): vdx_ddim_sample_loop_dyn, ('ddim', 'masked'): vdx_ddim_sample_loop_masked, ('ddim', 'guided'): L.vdx_ddim_sample_loop_guided,
          ('ddim', 'sr'): L.vdx_ddim_sample_loop_sr,
          ('dpm', 'plain'): vdx_dpm_sample_loop, ('dpm', 'masked'): vdx_dpm_sample_loop_masked, ('dpm', 'guided'): L.vdx_dpm_sample_loop_guided,
          ('dpm', 'sr'): L.vdx_dpm_sample_loop_sr}
_CFG = ' cond_scale rescale scratch'
_LOOP_EXTRA = {'plain': '', 'sr': '', 'lv': '', 'guided': _CFG, 'mixed': _CFG + ' mix_a mix_b', 'masked': ' known mask mtab'}


def loop_args(chain: str, variant: str, named: dict) -> list:
    """The positional arguments of the entry _LOOPS[chain, variant] out of `named` (argument name -> value), in the order include/vdx.h
    declares them: head | chain block | variant block | tail."""
    sig = 'h params packed img' + (' xin' if variant == 'sr' else '') + ' eps' + (' hist' if chain == 'dpm' else '') + ' t_dev step_dev'
    if variant == 'lv':
        sig += ' lv_tab seq seq_len timesteps nsteps cond seed clip post_scale post_shift'
    elif chain == 'ddpm':
        sig += ' tables timesteps nsteps cond seed clip percentile thres'
    else:
        sig += ' ac seq seq_len nsteps cond clip' + (' order' if chain == 'dpm' else '') + ' tables timesteps percentile thres'
    sig += _LOOP_EXTRA[variant] + ((' resample' if chain == 'ddpm' else ' seed') if variant == 'masked' else '')
    return [named[n] for n in (sig + ' ws ws_bytes batch use_graph stream').split()]


def extend_plan(have: int, num_new: int, num_frames: int, context_frames: int):
    """The windows of GaussianDiffusion.extend as (ctx, new) pairs: a window of `num_frames` holds the last ctx = min(context_frames,
    frames so far) frames as known frames and keeps the next new = min(num_frames - ctx, frames still missing) generated ones."""
    if not 1 <= context_frames < num_frames:
        raise ValueError(f'context_frames must be in [1, {num_frames - 1}], got {context_frames}')
    if have < 1 or num_new < 0:
        raise ValueError(f'need at least one given frame and num_new >= 0, got {have}, {num_new}')
    plan = []
    while num_new > 0:
        ctx = min(context_frames, have)
        new = min(num_frames - ctx, num_new)
        plan.append((ctx, new))
        have, num_new = have + new, num_new - new
    return plan


def frame_mask(mask, shape) -> torch.Tensor:
    """The element mask of `inpaint` (1 = known) as contiguous uint8 of `shape` = [B,C,F,H,W], on `mask`'s device.  `mask` is [F]
    (the same frames of every video), [B,F] (per video) or anything that broadcasts to `shape`; bool or uint8."""
    B, _, Fr, _, _ = shape
    m = torch.as_tensor(mask)
    if m.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f'mask must be bool or uint8, got {m.dtype}')
    if m.dim() == 1 and m.shape[0] == Fr:
        m = m.reshape(1, 1, Fr, 1, 1)
    elif m.dim() == 2 and tuple(m.shape) == (B, Fr):
        m = m.reshape(B, 1, Fr, 1, 1)
    else:
        try:
            ok = torch.broadcast_shapes(tuple(m.shape), tuple(shape)) == torch.Size(shape)
        except RuntimeError:
            ok = False
        if not ok:
            raise ValueError(f'mask of shape {tuple(m.shape)} is neither [F], [B, F] nor broadcastable to {tuple(shape)}')
    return (m != 0).to(torch.uint8).expand(*shape).contiguous()


_frame_mask = frame_mask      # (methods below take a `frame_mask` keyword)


def ddim_time_sequence(timesteps: int, steps: int) -> np.ndarray:
    """The S + 1 times of an S-step DDIM chain over a T-step schedule: T-1 = t_0 > t_1 > ... > t_{S-1} >= 0, then -1 (= the data).
    Evenly spaced as linspace(-1, T-1, S+1), the usual choice (denoising-diffusion-pytorch); the reference has no DDIM."""
    assert 1 <= steps <= timesteps
    return np.ascontiguousarray(np.linspace(-1, timesteps - 1, steps + 1).astype(np.int32)[::-1])


def check_dpm_args(timesteps: int, dpm_steps, dpm_order=2, ddim_steps=None, resample_steps: int = 1) -> None:
    """The argument rules of the DPM-Solver++ paths (dpm_steps is not None), checked before any device work."""
    if dpm_steps is None:
        return
    if ddim_steps:
        raise ValueError('dpm_steps and ddim_steps are two samplers: give one of them')
    if int(resample_steps) > 1:
        raise ValueError('resampling (resample_steps > 1) is defined for the ancestral chain only, not with dpm_steps')
    if dpm_order not in (1, 2):
        raise ValueError(f'dpm_order must be 1 or 2, got {dpm_order}')
    if not 1 <= int(dpm_steps) <= int(timesteps):
        raise ValueError(f'dpm_steps must be in [1, {int(timesteps)}], got {dpm_steps}')


def chain_choice(timesteps: int, ddim_steps=None, dpm_steps=None, dpm_order=2, resample_steps: int = 1):
    """(chain, steps) of the sampler keywords, after check_dpm_args: ('dpm', S) with dpm_steps, ('ddim', S) with ddim_steps, else the
    T-step ancestral chain ('ddpm', 0)."""
    check_dpm_args(timesteps, dpm_steps, dpm_order, ddim_steps, resample_steps)
    return ('dpm', int(dpm_steps)) if dpm_steps is not None else ('ddim', int(ddim_steps)) if ddim_steps else ('ddpm', 0)


def check_guidance_rescale(guidance_rescale) -> float:
    """The guidance rescale phi of the guided loops (Lin et al. 2023, sec. 3.4) as a float; outside [0, 1] raises ValueError."""
    phi = float(guidance_rescale)
    if not 0.0 <= phi <= 1.0:
        raise ValueError(f'guidance_rescale must be in [0, 1], got {guidance_rescale}')
    return phi


TABLE_NAMES = (
    'alphas_cumprod', 'sqrt_alphas_cumprod', 'sqrt_one_minus_alphas_cumprod', 'log_one_minus_alphas_cumprod',
    'sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod', 'posterior_variance',
    'posterior_log_variance_clipped', 'posterior_mean_coef1', 'posterior_mean_coef2',
)


def cosine_beta_schedule(timesteps: int, s: float = 0.008) -> np.ndarray:
    """reference utils.py:241-256; float32 arithmetic (JAX x64 is off in the reference)."""
    f = np.float32
    x = np.linspace(0, timesteps, timesteps + 1, dtype=np.float32)
    ac = np.cos(((x / f(timesteps)) + f(s)) / f(1 + s) * f(np.pi) * f(0.5)) ** 2
    ac = (ac / ac[0]).astype(np.float32)
    betas = f(1) - (ac[1:] / ac[:-1])
    return np.clip(betas, f(0), f(0.9999)).astype(np.float32)


def make_tables(timesteps: int) -> dict:
    """The ten schedule tables of reference gaussian_diffusion.py:78-98 (float32)."""
    f = np.float32
    betas = cosine_beta_schedule(timesteps)
    alphas = f(1) - betas
    ac = np.cumprod(alphas, axis=0, dtype=np.float32)
    ac_prev = np.concatenate([np.ones(1, np.float32), ac[:-1]])
    pv = betas * (f(1) - ac_prev) / (f(1) - ac)
    with np.errstate(divide='ignore'):
        t = {
            'alphas_cumprod': ac, 'sqrt_alphas_cumprod': np.sqrt(ac), 'sqrt_one_minus_alphas_cumprod': np.sqrt(f(1) - ac),
            'log_one_minus_alphas_cumprod': np.log(f(1) - ac), 'sqrt_recip_alphas_cumprod': np.sqrt(f(1) / ac),
            'sqrt_recipm1_alphas_cumprod': np.sqrt(f(1) / ac - f(1)), 'posterior_variance': pv,
            'posterior_log_variance_clipped': np.log(np.maximum(pv, f(1e-20))),
            'posterior_mean_coef1': betas * np.sqrt(ac_prev) / (f(1) - ac),
            'posterior_mean_coef2': (f(1) - ac_prev) * np.sqrt(alphas) / (f(1) - ac),
        }
    return {k: v.astype(np.float32) for k, v in t.items()}


VLB_ROWS = L.VLB_ROWS


def make_vlb_tables(timesteps: int) -> np.ndarray:
    """The [VLB_ROWS, T] float64 table of the evaluation kernels (vdx.h: "Held-out evaluation").  Rows 0-5 and 8 are make_tables' fp32
    values, widened: the numbers the sampling kernels use, so the bound is that of the model that samples.  Row 6, w_t = coef1_t^2 /
    (2 post_var_t ln 2), and row 7, the decoder's log-variance log post_var_max(t, 1), are formed from them in float64; w_0 = 0 (level
    0 is the decoder term)."""
    if int(timesteps) < 2:
        raise ValueError(f'the variational bound needs timesteps >= 2, got {timesteps}')
    tabs = {k: v.astype(np.float64) for k, v in make_tables(int(timesteps)).items()}
    pv, c1 = tabs['posterior_variance'], tabs['posterior_mean_coef1']
    w = np.zeros_like(pv)
    w[1:] = c1[1:] ** 2 / (2.0 * pv[1:] * np.log(2.0))
    dec = np.log(np.concatenate([pv[1:2], pv[1:]]))
    return np.ascontiguousarray(np.stack([tabs['sqrt_alphas_cumprod'], tabs['sqrt_one_minus_alphas_cumprod'], tabs['sqrt_recip_alphas_cumprod'],
                                          tabs['sqrt_recipm1_alphas_cumprod'], c1, tabs['posterior_mean_coef2'], w, dec, tabs['alphas_cumprod']]))


LV_ROWS = L.LV_ROWS


def make_lv_tables(timesteps: int, seq=None) -> dict:
    """The float64 tables of the learned-variance paths (vdx.h: "Learned variances"; Nichol & Dhariwal 2021), level by level of an
    S-level chain over the T-step schedule.  seq: the increasing levels the chain keeps (None: all T).  From the project's betas
    (cosine_beta_schedule, widened) alpha_bar = cumprod(1 - beta) in float64, then for every chain -- the full one included, so that
    seq = range(T) is the unrespaced table bit for bit -- alpha_bar'_i = alpha_bar[seq_i], beta'_i = 1 - alpha_bar'_i / alpha_bar'_{i-1}
    (alpha_bar'_{-1} = 1) and everything else from those two: the posterior coefficients c1, c2, sqrt(1 / alpha_bar'),
    sqrt(1 / alpha_bar' - 1), max_log = log beta' and min_log = log beta~' with min_log[0] = log beta~'_1 (the Improved-DDPM convention;
    a one-level chain has no beta~'_1 and takes max_log[0]: level 0 adds no noise).  The network is still called with t = seq_i.
    Returns the named float64 arrays [S] plus 'seq' (int32 [S]), 'step' (float32 [6, S]: the rows of vdx_p_sample_step_lv) and 'tab64'
    (float64 [LV_ROWS, S]: the rows of vdx_hybrid_loss / vdx_vlb_terms_lv).  The fp32 tables of make_tables are not touched."""
    T = int(timesteps)
    if T < 1:
        raise ValueError(f'timesteps must be >= 1, got {timesteps}')
    lv = np.arange(T, dtype=np.int64) if seq is None else np.asarray(list(seq), dtype=np.int64).reshape(-1)
    if lv.size < 1 or lv.size > T or lv[0] < 0 or lv[-1] >= T or np.any(np.diff(lv) <= 0):
        raise ValueError(f'seq must be an increasing sequence of 1 to {T} levels in [0, {T - 1}]')
    ac_all = np.cumprod(1.0 - cosine_beta_schedule(T).astype(np.float64))
    ac = ac_all[lv]
    ac_prev = np.concatenate([np.ones(1), ac[:-1]])
    betas = 1.0 - ac / ac_prev
    pv = betas * (1.0 - ac_prev) / (1.0 - ac)
    max_log = np.log(betas)
    min_log = np.log(np.concatenate([pv[1:2], pv[1:]])) if lv.size > 1 else max_log.copy()
    t = {'betas': betas, 'alphas_cumprod': ac, 'sqrt_alphas_cumprod': np.sqrt(ac), 'sqrt_one_minus_alphas_cumprod': np.sqrt(1.0 - ac),
         'sqrt_recip_alphas_cumprod': np.sqrt(1.0 / ac), 'sqrt_recipm1_alphas_cumprod': np.sqrt(1.0 / ac - 1.0),
         'posterior_mean_coef1': betas * np.sqrt(ac_prev) / (1.0 - ac), 'posterior_mean_coef2': (1.0 - ac_prev) * np.sqrt(1.0 - betas) / (1.0 - ac),
         'max_log': max_log, 'min_log': min_log}
    step_rows = ('sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod', 'posterior_mean_coef1', 'posterior_mean_coef2', 'max_log', 'min_log')
    t['tab64'] = np.ascontiguousarray(np.stack([t['sqrt_alphas_cumprod'], t['sqrt_one_minus_alphas_cumprod']] + [t[k] for k in step_rows] + [ac]))
    t['step'] = np.ascontiguousarray(np.stack([t[k] for k in step_rows]).astype(np.float32))
    t['seq'] = lv.astype(np.int32)
    return t


def lv_time_sequence(timesteps: int, steps=None) -> np.ndarray:
    """The S + 1 entries of the learned-variance chain's device sequence: its levels descending, then -1 (steps None: all T levels;
    an int S: the ddim_time_sequence(T, S) ones).  Its first S entries reversed are make_lv_tables' seq."""
    if steps is None:
        steps = int(timesteps)
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not 1 <= int(steps) <= int(timesteps):
        raise ValueError(f'steps must be None or an int in [1, {int(timesteps)}], got {steps!r}')
    return ddim_time_sequence(int(timesteps), int(steps))


def vlb_time_sequence(timesteps: int, steps=None) -> np.ndarray:
    """The levels calc_bpd_loop visits, then -1: every level T-1 .. 0 (steps None) or the ddim_time_sequence(T, steps) ones."""
    if steps is None:
        return np.ascontiguousarray(np.arange(int(timesteps) - 1, -2, -1, dtype=np.int32))
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not 1 <= int(steps) <= int(timesteps):
        raise ValueError(f'timesteps must be None or an int in [1, {int(timesteps)}], got {steps!r}')
    return ddim_time_sequence(int(timesteps), int(steps))


def split_key(key: int, num: int = 2):
    """Deterministic seed derivation standing in for jax.random.split (splitmix64 of (key, index))."""
    out = []
    for i in range(num):
        z = (int(key) * 0x9E3779B97F4A7C15 + (i + 1) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        out.append(z ^ (z >> 31))
    return out


def lowres_aug_key(key: int) -> int:
    """Key of the super-resolution augmentation (the level draw and the noise) under a loss key: child 4 of it.  p_losses'
    `_, noise_key, _ = split(key, 3)` takes children 1-3 (the train step gives 1 to the condition dropout and 3 to the focus-present
    draw), so no other stream moves."""
    return split_key(key, 4)[3]


def lowres_aug_levels(batch: int, aug_max: int, key: int) -> torch.Tensor:
    """The augmentation levels of one batch: int32 [batch], uniform on {0..aug_max-1}, drawn on the host under `key`."""
    g = torch.Generator().manual_seed(int(key) & 0x7FFFFFFFFFFFFFFF)
    return torch.randint(0, int(aug_max), (int(batch),), generator=g, dtype=torch.int32)


def self_cond_key(key: int) -> int:
    """Key of the self-conditioning coin under a loss key: child 5 of it (children 1-4: lowres_aug_key), so no other stream moves."""
    return split_key(key, 5)[4]


def self_cond_draw(p: float, generator=None) -> bool:
    """The coin of one micro-batch of self-conditioned training (Chen et al. 2022, sec. 2.2: "with probability 50%"): True = the step runs
    the first forward and conditions on its estimate.  One coin per micro-batch, not per sample: every sample then costs the same, and so
    does every rank.  Pure host function of (p, generator state); p = 0 is never True, p = 1 always."""
    if isinstance(p, bool) or not 0.0 <= float(p) <= 1.0:
        raise ValueError(f'self_cond_prob must be in [0, 1], got {p}')
    return bool(float(torch.rand((), generator=generator)) < float(p))


def dist_rank_world():
    """(rank, world) of the default torch.distributed group, (0, 1) outside one."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def shard_key(key: int, rank: int, world: int) -> int:
    """Philox seed of rank `rank`'s shard of a data-parallel sampling batch: a function of (key, rank) only, so the videos a rank
    draws do not depend on how many other ranks there are; one rank keeps `key` itself."""
    return int(key) & 0xFFFFFFFFFFFFFFFF if world == 1 else split_key(key, rank + 1)[-1]


def extract(a: torch.Tensor, t: torch.Tensor, x_shape) -> torch.Tensor:
    """reference utils.py:225-238."""
    b = t.shape[0]
    return a.gather(-1, t.long()).reshape(b, *((1,) * (len(x_shape) - 1)))


def _stage(x, dtype, dev) -> torch.Tensor:
    """`x` as a contiguous tensor of `dtype` (None: its own) on `dev`.  A host tensor goes through pinned memory and a non-blocking copy:
    a pageable host-to-device copy waits for the stream to drain -- one host sync per train step that kept the launch queue from
    running ahead of the GPU."""
    x = torch.as_tensor(x)
    x = x if dtype is None else x.to(dtype)
    if x.device.type == 'cpu' and dev.type == 'cuda':
        x = x.pin_memory().to(dev, non_blocking=True)
    return x.to(dev).contiguous()


def is_list_str(x) -> bool:
    """reference utils.py:282-293 (an empty list/tuple counts as a list of strings)."""
    return isinstance(x, (list, tuple)) and all(type(el) == str for el in x)


def check_lowres_cond(lowres_cond, num_frames: int, image_size: int):
    """(ft, fs) of a super-resolution diffusion's lowres_cond: two integers >= 1 that divide num_frames and image_size."""
    try:
        ft, fs = lowres_cond
    except (TypeError, ValueError):
        raise ValueError(f'lowres_cond must be a pair (temporal factor, spatial factor), got {lowres_cond!r}') from None
    for name, v in (('temporal', ft), ('spatial', fs)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 1:
            raise ValueError(f'lowres_cond: the {name} factor must be an integer >= 1, got {v!r}')
    if int(num_frames) % int(ft) or int(image_size) % int(fs):
        raise ValueError(f'lowres_cond ({ft}, {fs}): the temporal factor must divide num_frames = {num_frames} and the spatial one '
                         f'image_size = {image_size}')
    return int(ft), int(fs)


def check_frame_noise_alpha(alpha) -> float:
    """PYoCo's mixed-noise parameter as a float: a finite number >= 0 (0 = i.i.d. noise); anything else (a bool included) raises
    ValueError."""
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.integer, np.floating)):
        raise ValueError(f'frame_noise_alpha must be a finite number >= 0, got {alpha!r}')
    al = float(alpha)
    if not (al >= 0.0 and al != float('inf')):
        raise ValueError(f'frame_noise_alpha must be a finite number >= 0, got {alpha!r}')
    return al


def mixed_noise_coef(alpha):
    """(a, b) = (alpha, 1) / sqrt(1 + alpha^2) of the mixed noise z = a s + b e (Ge et al. 2023, sec. 3.2), formed in double and rounded
    once to fp32 (returned as Python floats holding the fp32 values: what the kernels receive)."""
    al = check_frame_noise_alpha(alpha)
    h = float(np.hypot(1.0, al))
    return float(np.float32(al / h)), float(np.float32(1.0 / h))


OBJECTIVES = ('pred_noise', 'pred_v')


def check_objective(objective) -> str:
    """What the network predicts: 'pred_noise' (eps, the reference) or 'pred_v' (v = sqrt(ac) eps - sqrt(1 - ac) x0); anything else raises
    ValueError."""
    if not isinstance(objective, str) or objective not in OBJECTIVES:
        raise ValueError(f"objective must be 'pred_noise' or 'pred_v', got {objective!r}")
    return objective


def check_min_snr_gamma(gamma):
    """The min-SNR clamp gamma as a float, or None (no loss weighting): a finite number > 0; anything else (a bool included) raises
    ValueError."""
    if gamma is None:
        return None
    if isinstance(gamma, bool) or not isinstance(gamma, (int, float, np.integer, np.floating)):
        raise ValueError(f'min_snr_gamma must be None or a finite number > 0, got {gamma!r}')
    g = float(gamma)
    if not (g > 0.0 and g != float('inf')):
        raise ValueError(f'min_snr_gamma must be None or a finite number > 0, got {gamma!r}')
    return g


def min_snr_weights(timesteps: int, objective: str = 'pred_noise', gamma=None):
    """The loss weight of every level as float64 [T] (Hang et al. 2023, min-SNR-gamma), or None without gamma.  SNR_t = ac_t / (1 - ac_t)
    from make_tables' alphas_cumprod widened to double (the numbers q_sample noises with); the weight is the one on the x0 loss,
    min(SNR, gamma), restated for what the network predicts: pred_noise min(SNR, gamma) / SNR, pred_v min(SNR, gamma) / (SNR + 1).  Both
    are <= 1, and w_v = w_eps SNR / (SNR + 1)."""
    objective, g = check_objective(objective), check_min_snr_gamma(gamma)
    if g is None:
        return None
    ac = make_tables(int(timesteps))['alphas_cumprod'].astype(np.float64)
    snr = ac / (1.0 - ac)
    return np.minimum(snr, g) / (snr + 1.0 if objective == 'pred_v' else snr)


class GaussianDiffusion:
    # the objective's switches (instance attributes only when they are on: a plain instance keeps the attributes it had)
    objective = 'pred_noise'
    min_snr_gamma = None
    _loss_w = None
    # super-resolution switches (instance attributes only on a super-resolution diffusion: a plain one keeps the attributes it had)
    lowres_cond = None
    lowres_aug_max = 0
    # mixed-noise switch (instance attributes only when it is on, likewise)
    frame_noise_alpha = 0.0
    # self-conditioning switch (an instance attribute only when it is on, likewise)
    self_condition = False

    def __init__(self, denoise_fn: Unet3D, *, image_size: int, num_frames: int, text_use_bert_cls: bool = False,
                 channels: int = 3, timesteps: int = 1000, loss_type: str = 'l1', use_dynamic_thres: bool = False,
                 dynamic_thres_percentile: float = 0.9, sample_act_bf16: bool = True, learned_variance: bool = False,
                 vlb_weight: Optional[float] = None, lowres_cond=None, lowres_aug_max: int = 0, frame_noise_alpha: float = 0.0,
                 objective: str = 'pred_noise', min_snr_gamma: Optional[float] = None, self_condition: bool = False):
        # self_condition = True (extension, off by default; Chen et al. 2022, "Analog Bits", sec. 2.2): the denoiser has channels =
        # 2 * channels and out_dim = channels; its input is [ x_t | x0~ ], x0~ = its own previous estimate of x0, clipped (zero where there
        # is none).  Training runs a first, gradient-free forward on [ x_t | 0 ] for a fraction Trainer.self_cond_prob of the steps and
        # regresses from [ x_t | x0~ ] (train_step.forward_backward); the sampling chains feed the estimate of step k to step k + 1 inside
        # the captured step (the handle's self-condition state, _sampling; the super-resolution loop entries, which carry xin).  Not stored
        # in checkpoints, the stem's shape is.  vdx.h: "Self-conditioning".
        if not isinstance(self_condition, (bool, np.bool_)):
            raise ValueError(f'self_condition must be True or False, got {self_condition!r}')
        if self_condition:
            if lowres_cond is not None:
                raise ValueError('self_condition does not support lowres_cond yet (a follow-up; DESIGN.md 9): the denoiser would take '
                                 '3 * channels input planes')
            if learned_variance:
                raise ValueError('self_condition does not support learned_variance yet (a follow-up; DESIGN.md 9): the learned-variance loops '
                                 'have no xin')
            if check_frame_noise_alpha(frame_noise_alpha) > 0:
                raise ValueError('self_condition does not support frame_noise_alpha yet (a follow-up; DESIGN.md 9): the loops over xin have no '
                                 'mixed-noise step')
            if getattr(denoise_fn, 'channels', None) != 2 * channels or getattr(denoise_fn, 'out_dim', None) != channels:
                raise ValueError(f'self_condition needs a denoiser with channels == 2 * channels = {2 * channels} and out_dim == channels = '
                                 f'{channels}, got channels {getattr(denoise_fn, "channels", None)}, out_dim {getattr(denoise_fn, "out_dim", None)}')
            self.self_condition = True
        # objective = 'pred_v' (extension, off by default; Salimans & Ho 2022, "Progressive Distillation"): the network predicts
        # v = sqrt(ac_t) eps - sqrt(1 - ac_t) x0, well conditioned at both ends of the schedule.  Training regresses on v (vdx_v_loss);
        # everywhere else the network output is converted once, in place, to eps_hat = sqrt(ac_t) v_hat + sqrt(1 - ac_t) x_t directly behind
        # the forward (_eps_from_out; in the captured loops the handle's prediction state, _sampling) and everything downstream is the
        # eps-model it was.  min_snr_gamma = gamma (extension, off by default; Hang et al. 2023): the loss of a sample at level t is weighted
        # with min_snr_weights, for either objective.  Neither is stored in checkpoints: sample a model with the objective it was trained
        # with.  vdx.h: "v-prediction".
        objective, gamma = check_objective(objective), check_min_snr_gamma(min_snr_gamma)
        for name, on in (("objective='pred_v'", objective == 'pred_v'), ('min_snr_gamma', gamma is not None)):
            if on and learned_variance:
                raise ValueError(f'{name} does not support learned_variance yet (a follow-up; DESIGN.md 9): the hybrid loss and the '
                                 'learned-variance loops take eps_hat | v of an eps-model')
        if objective == 'pred_v':
            self.objective = objective
        if gamma is not None:
            self.min_snr_gamma = gamma
        # frame_noise_alpha = alpha (extension, off by default; Ge et al. 2023, "Preserve Your Own Correlation", sec. 3.2, the mixed noise
        # model): every noise tensor drawn by key -- q_sample's eps, x_T, the z of the ancestral steps -- is z = a s + b e with s shared by
        # the frames of a clip, a = alpha / sqrt(1 + alpha^2), b = 1 / sqrt(1 + alpha^2): still N(0, 1) per element, two frames correlate
        # with frame_noise_corr = a^2 at the same pixel.  The model is trained and sampled under that prior (noise(); vdx.h: "Mixed
        # noise").  Like the other switches it is not stored in checkpoints: sample a model with the alpha it was trained with.  0: no new
        # state, no new path.
        alpha = check_frame_noise_alpha(frame_noise_alpha)
        if alpha > 0:
            if learned_variance:
                raise ValueError('frame_noise_alpha does not support learned_variance yet (a follow-up; DESIGN.md 9): the KL of the hybrid loss '
                                 'needs the inverse frame covariance')
            if lowres_cond is not None:
                raise ValueError('frame_noise_alpha does not support lowres_cond yet (a follow-up; DESIGN.md 9): the super-resolution loops have '
                                 'no mixed-noise entry')
            self.frame_noise_alpha = alpha
            self._mix = mixed_noise_coef(alpha)
        # lowres_cond = (ft, fs) (extension, off by default; Ho et al. 2021, "Cascaded Diffusion Models"): the second stage of a cascade.
        # The denoiser has channels = 2 * channels and out_dim = channels; its input is [ x_t | u ], u = the low-resolution clip
        # [B,C,F/ft,S/fs,S/fs] normalised, upsampled linearly and, in training, noised to a level drawn from {0..lowres_aug_max-1}
        # (blind noise conditioning augmentation; 0 = none).  vdx.h: "Cascaded super-resolution".
        if lowres_cond is not None:
            ft_fs = check_lowres_cond(lowres_cond, num_frames, image_size)
            if learned_variance:
                raise ValueError('lowres_cond does not support learned_variance yet (a follow-up; DESIGN.md 9)')
            if getattr(denoise_fn, 'channels', None) != 2 * channels or getattr(denoise_fn, 'out_dim', None) != channels:
                raise ValueError(f'lowres_cond needs a denoiser with channels == 2 * channels = {2 * channels} and out_dim == channels = '
                                 f'{channels}, got channels {getattr(denoise_fn, "channels", None)}, out_dim {getattr(denoise_fn, "out_dim", None)}')
            if isinstance(lowres_aug_max, bool) or not isinstance(lowres_aug_max, (int, np.integer)) or not 0 <= int(lowres_aug_max) <= int(timesteps):
                raise ValueError(f'lowres_aug_max must be an integer in [0, {int(timesteps)}], got {lowres_aug_max!r}')
            self.lowres_cond = ft_fs
            self.lowres_aug_max = int(lowres_aug_max)
        elif lowres_aug_max:
            raise ValueError('lowres_aug_max is the augmentation range of a super-resolution diffusion: it needs lowres_cond=(ft, fs)')
        # sample_act_bf16 (extension): with a mode='bf16' Unet3D the sampling loops store the UNet's inter-kernel activations
        # as bf16 (vdx_set_activation_storage); training forwards are unaffected
        self.sample_act_bf16 = sample_act_bf16
        # learned_variance (extension, off by default; Nichol & Dhariwal 2021): the denoiser has out_dim = 2 * channels, eps_hat | v, and
        # log sigma^2 = f log beta + (1 - f) log beta~ with f = (v + 1) / 2.  Training minimises the hybrid loss L_simple + vlb_weight * L_vlb
        # (vlb_weight defaults to timesteps / 1000, lambda = 0.001 on the T-term sum; last_loss_terms keeps the device doubles (mse, vb) of
        # the last loss), sampling and calc_bpd_loop use the model's variance; steps=S samples with the respaced S-level chain.
        self.learned_variance = bool(learned_variance)
        self.vlb_weight = None
        self.last_loss_terms = None
        if self.learned_variance:
            if getattr(denoise_fn, 'out_dim', None) != 2 * channels:
                raise ValueError(f'learned_variance needs a denoiser with out_dim == 2 * channels = {2 * channels}, got '
                                 f'{getattr(denoise_fn, "out_dim", None)}')
            if use_dynamic_thres:
                raise ValueError('learned_variance does not support use_dynamic_thres (a follow-up)')
            if int(timesteps) < 2:
                raise ValueError(f'learned_variance needs timesteps >= 2, got {timesteps}')
            self.vlb_weight = float(timesteps) / 1000.0 if vlb_weight is None else float(vlb_weight)
            self._lv_cache = {}
        elif vlb_weight is not None:
            raise ValueError('vlb_weight is the weight of the hybrid loss: it needs learned_variance=True')
        self.channels = channels
        self.image_size = image_size
        self.num_frames = num_frames
        self.denoise_fn = denoise_fn
        self.loss_type = loss_type
        self.text_use_bert_cls = text_use_bert_cls
        self.use_dynamic_thres = use_dynamic_thres
        self.dynamic_thres_percentile = dynamic_thres_percentile
        self.num_timesteps = int(timesteps)
        self.device = denoise_fn.device
        tabs = make_tables(self.num_timesteps)
        for name in TABLE_NAMES:
            setattr(self, name, torch.from_numpy(tabs[name]).to(self.device))
        # the five tables the reverse step needs, stacked [5][T] for the kernel
        self._ptab = torch.stack([self.sqrt_recip_alphas_cumprod, self.sqrt_recipm1_alphas_cumprod, self.posterior_mean_coef1,
                                  self.posterior_mean_coef2, self.posterior_log_variance_clipped]).contiguous()
        # the factors of the masked (inpainting) steps, stacked [4][T]: sqrt_ac | sqrt(1 - ac) | sqrt(alpha) | sqrt(beta)
        betas = cosine_beta_schedule(self.num_timesteps)
        self._mtab = torch.from_numpy(np.stack([tabs['sqrt_alphas_cumprod'], tabs['sqrt_one_minus_alphas_cumprod'],
                                                np.sqrt(np.float32(1) - betas), np.sqrt(betas)]).astype(np.float32)).to(self.device)
        # the same with rows 0, 1 = (1, 0): the masked kernels' `row0 * known + row1 * z` is then `known` itself at every level -- the
        # clean context frames a frame-conditioned (RaMViD) denoiser was trained on (inpaint(clean_context=True))
        self._mtab_clean = self._mtab.clone()
        self._mtab_clean[0] = 1.0
        self._mtab_clean[1] = 0.0
        self._sample_stream = None
        if self.min_snr_gamma is not None:
            self._loss_w = torch.from_numpy(min_snr_weights(self.num_timesteps, self.objective, self.min_snr_gamma)).to(self.device)

    # -- closed forms (table look-ups) -------------------------------------------------------------
    def q_mean_variance(self, x_start, t):
        mean = extract(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start
        variance = extract(1.0 - self.alphas_cumprod, t, x_start.shape)
        log_variance = extract(self.log_one_minus_alphas_cumprod, t, x_start.shape)
        return mean, variance, log_variance

    def predict_start_from_noise(self, x_t, t, noise):
        return (extract(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t
                - extract(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape) * noise)

    def predict_v(self, x_start, t, noise):
        """The target of the pred_v objective: v = sqrt(ac_t) noise - sqrt(1 - ac_t) x_start."""
        return (extract(self.sqrt_alphas_cumprod, t, x_start.shape) * noise
                - extract(self.sqrt_one_minus_alphas_cumprod, t, x_start.shape) * x_start)

    def predict_start_from_v(self, x_t, t, v):
        return (extract(self.sqrt_alphas_cumprod, t, x_t.shape) * x_t
                - extract(self.sqrt_one_minus_alphas_cumprod, t, x_t.shape) * v)

    def predict_noise_from_v(self, x_t, t, v):
        return (extract(self.sqrt_alphas_cumprod, t, x_t.shape) * v
                + extract(self.sqrt_one_minus_alphas_cumprod, t, x_t.shape) * x_t)

    @property
    def loss_weights(self):
        """The min-SNR loss weights as a float64 [T] device tensor (min_snr_weights), or None without min_snr_gamma."""
        return self._loss_w

    def q_posterior(self, x_start, x_t, t):
        mean = (extract(self.posterior_mean_coef1, t, x_t.shape) * x_start + extract(self.posterior_mean_coef2, t, x_t.shape) * x_t)
        return mean, extract(self.posterior_variance, t, x_t.shape), extract(self.posterior_log_variance_clipped, t, x_t.shape)

    # -- helpers -----------------------------------------------------------------------------------
    def _dev(self, x, dtype=torch.float32):
        return torch.as_tensor(x).to(self.device, dtype).contiguous()

    def randn(self, shape, key: int, offset: int = 0) -> torch.Tensor:
        out = torch.empty(tuple(shape), dtype=torch.float32, device=self.device)
        L.check(vdx_randn(L.ptr(out), out.numel(), int(key) & 0xFFFFFFFFFFFFFFFF, offset, 0, L.stream_ptr()))
        return out

    @property
    def frame_noise_corr(self) -> float:
        """rho = alpha^2 / (1 + alpha^2): the correlation of two frames of one clip's noise at the same pixel (0 = i.i.d.)."""
        al = self.frame_noise_alpha
        return al * al / (1.0 + al * al) if al < 1e150 else 1.0

    def noise(self, shape, key: int, draw: int = 0, *, out=None) -> torch.Tensor:
        """The noise tensor of `shape` = [B,C,F,H,W] at draw `draw` of stream `key` under the diffusion's prior: randn with
        frame_noise_alpha = 0 (the same launch), else the mixed noise a s + b e (vdx_randn_mixed: e = randn's tensor, s = the stream's draw
        VDX_DRAW_SHARED + draw over [B,C,H,W]).  Everything that draws noise by key goes through here.  out: a contiguous float32 device
        tensor whose first prod(shape) elements receive it (the guided chains' 2B-row buffer)."""
        shape = tuple(int(n) for n in shape)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        n = int(np.prod(shape))
        seed = int(key) & 0xFFFFFFFFFFFFFFFF
        if not self.frame_noise_alpha:
            L.check(vdx_randn(L.ptr(out), n, seed, draw, 0, L.stream_ptr()))
            return out
        if len(shape) != 5:
            raise ValueError(f'frame_noise_alpha: the mixed noise is defined over [B, C, F, H, W], got shape {shape}')
        B, C, Fr, H, W = shape
        L.check(L.vdx_randn_mixed(L.ptr(out), B, C, Fr, H * W, self._mix[0], self._mix[1], seed, draw, 0, L.stream_ptr()))
        return out

    # the optional features that refuse what they do not serve yet: message prefix, "is it on"
    _FEATURES = {'learned_variance': ('learned_variance', lambda gd: gd.learned_variance),
                 'lowres_cond': ('lowres_cond (super-resolution)', lambda gd: gd.lowres_cond is not None),
                 'frame_noise_alpha': ('frame_noise_alpha', lambda gd: bool(gd.frame_noise_alpha)),
                 'objective': ("objective='pred_v' / min_snr_gamma", lambda gd: gd.objective == 'pred_v' or gd.min_snr_gamma is not None),
                 'self_condition': ('self_condition', lambda gd: gd.self_condition)}

    def _refuse(self, feature, **given):
        """ValueError for the first of the keywords `given` that is in use (not None / False / its neutral value) while `feature` is on:
        what the feature does not serve yet (follow-ups)."""
        prefix, on = self._FEATURES[feature]
        if not on(self):
            return
        off = dict(cond_scale=1.0, guidance_rescale=0.0)
        for name, val in given.items():
            if val is None or val is False or (name in off and float(val) == off[name]):
                continue
            raise ValueError(f'{prefix} does not support {name} yet (a follow-up; DESIGN.md 9)')

    def _dev_mask(self, mask, shape):
        """frame_mask(mask, shape) on the device; an element mask that is already there goes through untouched."""
        if torch.is_tensor(mask) and mask.dtype == torch.uint8 and mask.device == self.device and mask.shape == torch.Size(shape) \
                and mask.is_contiguous():
            return mask
        return _frame_mask(mask, tuple(shape)).to(self.device)

    def _per_sample(self, x):
        return x.numel() // x.shape[0]

    def _eps_from_out(self, out, x, t32):
        """eps_hat of the network output `out` [rows,F,H,W,C] at x_t = `x` [rows,C,F,H,W], levels t32: `out` itself for pred_noise; for
        pred_v `out` is overwritten with sqrt(ac_t) out + sqrt(1 - ac_t) x (vdx_v_to_eps, one launch) and returned.  Every eager consumer
        of the network output goes through here; the captured loops run the same kernel inside their step (_sampling)."""
        if self.objective != 'pred_v':
            return out
        L.check(L.vdx_v_to_eps(L.ptr(out), L.ptr(x), L.ptr(t32), L.ptr(self.sqrt_alphas_cumprod), L.ptr(self.sqrt_one_minus_alphas_cumprod),
                               self.num_timesteps, x.shape[0], self.channels, self._per_sample(x), L.stream_ptr()))
        return out

    def _dynamic_threshold(self, x, t, eps_hat):
        """Imagen dynamic thresholding (reference :205-217): s = max(quantile(|x0_hat| per sample, percentile), 1), exact radix
        select on the device (vdx_dynamic_threshold)."""
        s = torch.empty(x.shape[0], dtype=torch.float32, device=self.device)
        L.check(vdx_dynamic_threshold(L.ptr(x), L.ptr(eps_hat), L.ptr(t), L.ptr(self._ptab), self.num_timesteps,
                                      float(self.dynamic_thres_percentile), L.ptr(s), x.shape[0], self.channels, self._per_sample(x),
                                      L.stream_ptr()))
        return s

    # -- self-conditioning ---------------------------------------------------------------------------
    def _self_cond_x0(self, x, x_pitch, eps_hat, t32, xin, *, thres=None, clip: bool = True):
        """x0~ of (x_t, eps_hat) at levels t32 into planes [C, 2C) of xin [B,2C,F,H,W] (vdx_selfcond_x0, one launch).  x: a device
        tensor whose sample b starts x_pitch floats after sample b - 1 (img with pitch per_sample, or xin itself with 2 per_sample)."""
        B, per = xin.shape[0], xin.numel() // xin.shape[0] // 2
        L.check(L.vdx_selfcond_x0(x.data_ptr(), int(x_pitch), L.ptr(eps_hat), L.ptr(t32), L.ptr(self._ptab), self.num_timesteps, L.ptr(thres),
                                  int(bool(clip)), L.ptr(xin), B, self.channels, per, L.stream_ptr()))
        return xin

    def self_cond_estimate(self, x, t, out, *, clip_denoised: bool = True, xin=None):
        """The self-condition x0~ [B,C,F,H,W] of the network output `out` [B,F,H,W,C] at x_t = `x`, levels t: clip(sqrt(1 / ac_t) x -
        sqrt(1 / ac_t - 1) eps_hat), clipped statically or, with use_dynamic_thres, by the dynamic threshold -- what the captured chains
        feed to their next step.  pred_v: `out` is converted to eps_hat in place first (_eps_from_out).  xin: an [B,2C,F,H,W] input whose
        second half receives the estimate (the first is not touched); the result is then a view of it."""
        if not self.self_condition:
            raise ValueError('self_cond_estimate needs a self-conditioned diffusion (self_condition=True)')
        x, t32 = self._dev(x), self._dev(t, torch.int32)
        eps_hat = self._eps_from_out(out, x, t32)
        thres = self._dynamic_threshold(x, t32, eps_hat) if (clip_denoised and self.use_dynamic_thres) else None
        buf = torch.empty((x.shape[0], 2 * self.channels) + tuple(x.shape[2:]), dtype=torch.float32, device=self.device) if xin is None else xin
        if tuple(buf.shape) != (x.shape[0], 2 * self.channels) + tuple(x.shape[2:]) or buf.dtype != torch.float32:
            raise ValueError(f'xin must be float32 [{x.shape[0]}, {2 * self.channels}, ...] over the shape of x, got {tuple(buf.shape)}')
        self._self_cond_x0(x, self._per_sample(x), eps_hat, t32, buf, thres=thres, clip=clip_denoised)
        est = buf[:, self.channels:]
        return est if xin is not None else est.contiguous()

    def self_cond_input(self, x_t, t32, self_cond, forward):
        """The training input xin [B,2C,F,H,W] = [ x_t | x0~ ] of a self-conditioned denoiser: zeros with x_t packed into the first half
        (vdx_lowres_pack), then by `self_cond`: False -- x0~ = 0; True -- pass 1: out = forward(xin), the very call pass 2 makes (same
        condition, masks and activation storage), converted to eps_hat for pred_v, and x0~ = the statically clipped estimate written
        into the second half (vdx_selfcond_x0 with x = the first half of xin, pitch 2 per_sample); a [B,C,F,H,W] tensor -- a ready
        estimate.  The estimate is a constant of the step: the backward runs from what the forward on the finished xin records."""
        from . import ops
        xin = torch.zeros((x_t.shape[0], 2 * self.channels) + tuple(x_t.shape[2:]), dtype=torch.float32, device=self.device)
        ops.lowres_pack(x_t, xin)
        if torch.is_tensor(self_cond):
            if tuple(self_cond.shape) != tuple(x_t.shape):
                raise ValueError(f'self_cond must be None, False, True or a {tuple(x_t.shape)} tensor, got shape {tuple(self_cond.shape)}')
            xin[:, self.channels:].copy_(self_cond.to(self.device, torch.float32))
        elif self_cond:
            eps_hat = self._eps_from_out(forward(xin), x_t, t32)
            self._self_cond_x0(xin, 2 * self._per_sample(x_t), eps_hat, t32, xin, clip=True)
        return xin

    def _self_cond_eps(self, x, t32, x_self_cond, cond):
        """The network output of a self-conditioned denoiser on [ x | x0~ ] (x_self_cond None: zeros)."""
        if x_self_cond is None:
            sc = torch.zeros_like(x)
        else:
            sc = self._dev(x_self_cond)
            if tuple(sc.shape) != tuple(x.shape):
                raise ValueError(f'x_self_cond must have the shape of x {tuple(x.shape)}, got {tuple(sc.shape)}')
        if is_list_str(cond):
            raise NotImplementedError('pass text conditioning as a ready embedding tensor')
        return self.denoise_fn(torch.cat([x, sc], dim=1), t32, cond=cond)

    # -- learned variances ---------------------------------------------------------------------------
    def _lv_tables(self, steps=None):
        """(descending device sequence [S + 1], float32 step table [6, S], S) of the S-level learned-variance chain, kept per S: the
        captured step bakes the addresses in."""
        seq_host = lv_time_sequence(self.num_timesteps, steps)
        S = len(seq_host) - 1
        if S not in self._lv_cache:
            tabs = make_lv_tables(self.num_timesteps, seq_host[:-1][::-1])
            self._lv_cache[S] = (torch.from_numpy(seq_host).to(self.device), torch.from_numpy(tabs['step']).to(self.device))
        return self._lv_cache[S] + (S,)

    def _lv_tab64(self):
        """The [LV_ROWS, T] float64 table of the hybrid loss and the bound, on the device."""
        if 'tab64' not in self._lv_cache:
            self._lv_cache['tab64'] = torch.from_numpy(make_lv_tables(self.num_timesteps)['tab64']).to(self.device)
        return self._lv_cache['tab64']

    def _lv_out(self, x, t32, cond):
        if is_list_str(cond):
            raise NotImplementedError('pass text conditioning as a ready embedding tensor')
        return self.denoise_fn(x, t32, cond=cond)

    # -- cascaded super-resolution -------------------------------------------------------------------
    def _sr_need_lowres(self, who, instead):
        if self.lowres_cond is not None:
            raise ValueError(f'lowres_cond (super-resolution): {who} has no low-resolution clip to condition on; use {instead}')

    def _sr_lowres(self, lowres, batch=None):
        """`lowres` checked against [B, C, F/ft, S/fs, S/fs] (before any device work) -> its shape."""
        if self.lowres_cond is None:
            raise ValueError('lowres needs a super-resolution diffusion (lowres_cond=(ft, fs))')
        ft, fs = self.lowres_cond
        want = (self.channels, self.num_frames // ft, self.image_size // fs, self.image_size // fs)
        shape = tuple(lowres.shape)
        if len(shape) != 5 or shape[1:] != want or (batch is not None and shape[0] != batch):
            raise ValueError(f'lowres must be [{"B" if batch is None else batch}, {want[0]}, {want[1]}, {want[2]}, {want[3]}], got {shape}')
        return shape

    def _sr_levels(self, aug_level, B):
        """The augmentation levels of a batch as host int32 [B] or None (none): an int (every sample) or [B] values in [-1, T-1]."""
        if aug_level is None:
            return None
        lv = torch.as_tensor(aug_level).to(torch.int32).reshape(-1).cpu()
        if lv.numel() == 1:
            lv = lv.expand(B).contiguous()
        if lv.numel() != B or int(lv.min()) < -1 or int(lv.max()) >= self.num_timesteps:
            raise ValueError(f'the augmentation level must be an int or [{B}] values in [-1, {self.num_timesteps - 1}], got {aug_level!r}')
        return lv

    def lowres_condition(self, lowres, key=None, aug_level=None, *, draw: int = 0, out=None):
        """u = aug(up(2 lowres - 1)) [B,C,F,S,S] of the low-resolution clip `lowres` [B,C,F/ft,S/fs,S/fs] in [0, 1] (vdx_lowres_input,
        the sampling-time form).  aug_level: None (none), an int or [B] levels (-1 = none for that sample); the noise is Philox(key,
        draw) in randn's layout (the sampling chains use draw VDX_DRAW_LOWRES of their seed).  out: an xin [B,2C,F,S,S] whose second
        half receives u (the first half is not touched); the result is then a view of it."""
        from . import ops
        B = self._sr_lowres(lowres)[0]
        lv = self._sr_levels(aug_level, B)
        if lv is not None and key is None:
            raise ValueError('an augmentation level needs a key for its noise')
        ft, fs = self.lowres_cond
        xin = ops.lowres_input(self._dev(lowres), ft, fs, tables=(self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod),
                               aug_levels=None if lv is None else lv.to(self.device), seed=int(key or 0), draw=draw, out=out)
        u = xin[:, self.channels:]
        return u if out is not None else u.contiguous()

    def sr_input(self, x_start, t32, noise, *, lowres=None, aug_levels=None, key: int = 0, _pre=(1.0, 0.0)):
        """The training input xin [B,2C,F,S,S] of a super-resolution denoiser in two launches: lowres = the box mean of the raw clip
        x_start (vdx_lowres_down; skipped when `lowres` is given), then q_sample of x_start * _pre[0] + _pre[1] into the first half and
        aug(up(2 lowres - 1)) into the second (vdx_lowres_input; the augmentation noise is Philox(key, draw 0)).  x_start, t32, noise on
        the device; aug_levels: host or device int32 [B] or None."""
        from . import ops
        ft, fs = self.lowres_cond
        lo = ops.lowres_down(x_start, ft, fs) if lowres is None else self._dev(lowres)
        lv = None if aug_levels is None else _stage(aug_levels, torch.int32, self.device)
        return ops.lowres_input(lo, ft, fs, x0=x_start, t=t32, noise=noise, tables=(self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod),
                                aug_levels=lv, seed=key, draw=0, pre=_pre)

    def _sr_eps(self, x, t32, lowres_cond, cond):
        """eps_hat of a super-resolution denoiser on [ x | u ]."""
        if lowres_cond is None:
            raise ValueError('a super-resolution diffusion needs lowres_cond=u (lowres_condition(lowres)) here')
        u = self._dev(lowres_cond)
        if tuple(u.shape) != tuple(x.shape):
            raise ValueError(f'lowres_cond must have the shape of x {tuple(x.shape)}, got {tuple(u.shape)}')
        if is_list_str(cond):
            raise NotImplementedError('pass text conditioning as a ready embedding tensor')
        return self.denoise_fn(torch.cat([x, u], dim=1), t32, cond=cond)

    def upsample(self, key, lowres, *, aug_level=None, cond=None, ddim_steps: Optional[int] = None, dpm_steps: Optional[int] = None,
                 dpm_order: int = 2, use_graph: bool = True, x_T=None):
        """The second stage of a cascade (EXTENSION): sample [B,C,F,S,S] in [0, 1] conditioned on the low-resolution clip `lowres`
        [B,C,F/ft,S/fs,S/fs] in [0, 1] (a base model's sample, say) with the T-step ancestral chain, an S-step DDIM chain (ddim_steps)
        or an S-step DPM-Solver++(2M) chain (dpm_steps, dpm_order).  aug_level: the noise conditioning augmentation level at sampling
        time (None = none; an int or [B] levels in [-1, T-1]), drawn as Philox(key, VDX_DRAW_LOWRES).  Single process: no rank sharding."""
        self._refuse('self_condition', upsample=True)
        if self.lowres_cond is None:
            raise ValueError('upsample needs a super-resolution diffusion (lowres_cond=(ft, fs))')
        lowres = torch.as_tensor(lowres)
        B = self._sr_lowres(lowres)[0]
        self._sr_levels(aug_level, B)                                     # (its range check, before any device work)
        chain, steps = chain_choice(self.num_timesteps, ddim_steps, dpm_steps, dpm_order)
        if ddim_steps:
            ddim_time_sequence(self.num_timesteps, ddim_steps)
        if x_T is not None and tuple(x_T.shape) != (B, self.channels, self.num_frames, self.image_size, self.image_size):
            raise ValueError(f'x_T must be [{B}, {self.channels}, {self.num_frames}, {self.image_size}, {self.image_size}], got {tuple(x_T.shape)}')
        with self._sampling(None, B):
            return self._run_chain(chain, B, key, steps=steps, order=dpm_order, cond=cond, use_graph=use_graph, x_T=x_T, lowres=lowres,
                                   aug_level=aug_level)

    def model_log_variance(self, out2, t):
        """log sigma^2 [B,C,F,H,W] of the network output out2 [B,F,H,W,2C] at levels t of the full chain (torch, on out2's device)."""
        tab = self._lv_tab64()
        v = out2[..., self.channels:].permute(0, 4, 1, 2, 3).double()
        f = 0.5 * (v + 1.0)
        shape = (-1, 1, 1, 1, 1)
        return (f * tab[6][t.long()].reshape(shape) + (1.0 - f) * tab[7][t.long()].reshape(shape)).float()

    def hybrid_loss(self, x_start, noise, out2, t32, *, want_grad: bool = False, _pre=(1.0, 0.0), iw=None):
        """(loss, d_out): the hybrid loss of the network output out2 [B,F,H,W,2C] as a float32 device scalar and, with want_grad, its
        gradient in out2 (vdx_hybrid_loss: one pass, no host read).  last_loss_terms = the device doubles (mse, vb).  iw (float64 [B] on
        the device; loss-aware timestep sampling): the totals and the gradient carry the importance weights (vdx_hybrid_loss_w), the
        per-sample pairs stay unweighted."""
        B = x_start.shape[0]
        scratch = torch.empty(L.vdx_hybrid_scratch_doubles(B), dtype=torch.float64, device=self.device)
        out = torch.empty(2 * B + 3, dtype=torch.float64, device=self.device)
        d_out = torch.empty_like(out2) if want_grad else None
        if iw is None:
            L.check(L.vdx_hybrid_loss(L.ptr(x_start), L.ptr(noise), L.ptr(out2), L.ptr(t32), L.ptr(self._lv_tab64()), self.num_timesteps,
                                      float(_pre[0]), float(_pre[1]), int(self.loss_type == 'l2'), self.vlb_weight, int(want_grad), L.ptr(d_out),
                                      L.ptr(scratch), L.ptr(out), B, self.channels, self._per_sample(x_start), L.stream_ptr()))
        else:
            L.check(L.vdx_hybrid_loss_w(L.ptr(x_start), L.ptr(noise), L.ptr(out2), L.ptr(t32), L.ptr(self._lv_tab64()), self.num_timesteps,
                                        float(_pre[0]), float(_pre[1]), int(self.loss_type == 'l2'), self.vlb_weight, int(want_grad),
                                        L.ptr(d_out), L.ptr(scratch), L.ptr(out), B, self.channels, self._per_sample(x_start), L.ptr(iw),
                                        L.stream_ptr()))
        self.last_loss_terms = out[2 * B:2 * B + 2]
        self.last_loss_per_sample = out[:2 * B].reshape(B, 2)
        return out[2 * B + 2].to(torch.float32).reshape(()), d_out

    # -- reverse process ---------------------------------------------------------------------------
    def _p_step(self, x, t, clip_denoised, cond, cond_scale, lowres_cond, key=0, noise=None, zero_noise=False, x_self_cond=None):
        """One eager reverse step -> (x_{t-1}, t on the device, the network output of a learned-variance diffusion or None).  The noise
        is `noise` when given, zero with zero_noise (the fused step is then the posterior mean), else drawn inside the step kernel as
        Philox(key, draw 0) under the diffusion's prior."""
        self._refuse('lowres_cond', cond_scale=cond_scale)
        self._refuse('self_condition', cond_scale=cond_scale)
        if not self.self_condition and x_self_cond is not None:
            raise ValueError('x_self_cond needs a self-conditioned diffusion (self_condition=True)')
        if self.lowres_cond is None and lowres_cond is not None:
            raise ValueError('lowres_cond needs a super-resolution diffusion (lowres_cond=(ft, fs))')
        x = self._dev(x)
        t32 = self._dev(t, torch.int32)
        self._refuse('learned_variance', cond_scale=cond_scale)
        seed = int(key or 0) & 0xFFFFFFFFFFFFFFFF
        out = torch.empty_like(x)
        nz = torch.zeros_like(x) if zero_noise else (None if noise is None else self._dev(noise))
        size = lambda: (x.shape[0], self.channels, self._per_sample(x), L.stream_ptr())        # (the tail of every step entry)
        if self.learned_variance:
            out2 = self._lv_out(x, t32, cond)
            L.check(L.vdx_p_sample_step_lv(L.ptr(x), L.ptr(out2), L.ptr(out), L.ptr(t32), L.ptr(self._lv_tables(None)[1]), self.num_timesteps,
                                           0, 0, L.ptr(nz), seed, 0, 0, int(clip_denoised), 1.0, 0.0, *size()))
            return out, t32, out2
        eps_hat = self._sr_eps(x, t32, lowres_cond, cond) if self.lowres_cond is not None else \
            self._self_cond_eps(x, t32, x_self_cond, cond) if self.self_condition else \
            self.denoise_fn.forward_with_cond_scale(x, t32, cond=cond, cond_scale=cond_scale)
        eps_hat = self._eps_from_out(eps_hat, x, t32)
        thres = self._dynamic_threshold(x, t32, eps_hat) if (clip_denoised and self.use_dynamic_thres) else None
        if nz is None and self.frame_noise_alpha:                         # z = a s + b e drawn inside the step kernel
            L.check(L.vdx_p_sample_step_mixed(L.ptr(x), L.ptr(eps_hat), L.ptr(out), L.ptr(t32), L.ptr(self._ptab), self.num_timesteps,
                                              x.shape[2], self._mix[0], self._mix[1], seed, 0, 0, L.ptr(thres), int(clip_denoised), *size()))
        else:
            L.check(vdx_p_sample_step(L.ptr(x), L.ptr(eps_hat), L.ptr(out), L.ptr(t32), L.ptr(self._ptab), self.num_timesteps, L.ptr(nz),
                                      seed, 0, 0, L.ptr(thres), int(clip_denoised), *size()))
        return out, t32, None

    def p_mean_variance(self, x, t, clip_denoised: bool, cond=None, cond_scale: float = 1.0, *, lowres_cond=None, x_self_cond=None):
        """reference :162-228 (returns (mean, variance, log_variance)): the reverse step with z = 0, and the variance look-ups.
        learned_variance: the model's variance, per element.  lowres_cond (a super-resolution diffusion only, and required there):
        u = lowres_condition(lowres), the network sees [ x | u ].  x_self_cond (a self-conditioned diffusion only): the estimate x0~ of
        the previous step (self_cond_estimate), the network sees [ x | x0~ ]; None = zeros."""
        mean, t32, out2 = self._p_step(x, t, clip_denoised, cond, cond_scale, lowres_cond, zero_noise=True, x_self_cond=x_self_cond)
        if out2 is not None:
            logvar = self.model_log_variance(out2, t32)
            return mean, logvar.exp(), logvar
        return mean, extract(self.posterior_variance, t32, mean.shape), extract(self.posterior_log_variance_clipped, t32, mean.shape)

    def p_sample(self, x, t, key, cond=None, cond_scale: float = 1.0, clip_denoised: bool = True, *, noise=None, lowres_cond=None,
                 x_self_cond=None):
        """reference :231-261.  `key`: seed of the noise draw (ignored when explicit `noise` is given).  lowres_cond / x_self_cond: as
        p_mean_variance."""
        return self._p_step(x, t, clip_denoised, cond, cond_scale, lowres_cond, key, noise, x_self_cond=x_self_cond)[0]

    # -- the sampling loops ------------------------------------------------------------------------
    @contextlib.contextmanager
    def _sampling(self, focus_present=None, batch: int = 0):
        """What every sampling loop runs inside: the side stream (ordered after the current one, and the current one after it on
        the way out) as the current stream, and the UNet's sampling-time activation storage, put back whatever happens.
        focus_present (True, or a [n] mask with batch % n == 0; needs Unet3D(focus_present=True)): the network's focus-present state
        for the loop -- "image mode" sampling from a jointly trained checkpoint (Unet3D docstring)."""
        unet = self.denoise_fn
        if focus_present is not None and focus_present is not False:
            if not unet.focus_present:
                raise ValueError('focus_present sampling needs Unet3D(focus_present=True)')
            unet._focus = unet.resolve_focus(batch, focus_present)
        if self._sample_stream is None:
            self._sample_stream = torch.cuda.Stream(device=self.device)
        cur, st = torch.cuda.current_stream(self.device), self._sample_stream
        st.wait_stream(cur)
        keep_storage = unet.act_bf16
        unet.act_bf16 = bool(self.sample_act_bf16 and unet.mode == 'bf16')
        # pred_v: the handle's loops convert the network output behind the forward (vdx_set_prediction); kind 0 goes back on the way out,
        # so a network shared with another diffusion is that diffusion's eps-model again
        # self_condition: likewise the handle's self-condition state (vdx_set_self_condition): the step of the loops over xin writes x0~
        # behind the forward; off again on the way out, so a network shared with a super-resolution diffusion runs that one's step again
        h = unet.handle(self.num_frames, self.image_size) if self.objective == 'pred_v' else None
        hs = unet.handle(self.num_frames, self.image_size) if self.self_condition else None
        try:
            if h is not None:
                L.check(L.vdx_set_prediction(h.ptr, 1, L.ptr(self.sqrt_alphas_cumprod), L.ptr(self.sqrt_one_minus_alphas_cumprod),
                                             self.num_timesteps))
            if hs is not None:
                L.check(L.vdx_set_self_condition(hs.ptr, 1, L.ptr(self._ptab), self.num_timesteps))
            with torch.cuda.stream(st):
                yield
        finally:
            if h is not None:
                L.check(L.vdx_set_prediction(h.ptr, 0, None, None, 0))
            if hs is not None:
                L.check(L.vdx_set_self_condition(hs.ptr, 0, None, 0))
            unet.act_bf16 = keep_storage
            unet._focus = None
        cur.wait_stream(st)

    _chain_buf = None      # the kept buffer set of the masked / super-resolution chains (an instance attribute once there is one)

    def _chain_bufs(self, B, rows=None, *, xin=False, known=False, hist=False, seq_host=None, keep=None):
        """The device buffers of one chain of B videos over `rows` network rows (default B; 2B under guidance), by name: img, eps, t
        [rows], step, thres (with use_dynamic_thres) and, on request, xin [B,2C,...] (zeroed), known + mask, hist [B] and seq (the
        upload of seq_host).  keep: a key, (variant, B, chain, steps), under which the set is kept across calls -- a captured step bakes
        addresses in, so a second call with the same key, seed and stream replays the cached graph; one set is kept, so a call under
        another key (the other sequence chain with the same S, say) allocates anew.  None: fresh tensors."""
        if keep is not None and self._chain_buf is not None and self._chain_buf['key'] == keep:
            return self._chain_buf
        dev, unet, rows = self.device, self.denoise_fn, rows or B
        one = (B, self.channels, self.num_frames, self.image_size, self.image_size)
        shape = (rows, self.channels, self.num_frames, self.image_size, self.image_size)
        new = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device=dev)
        buf = dict(key=keep, img=new(shape), eps=new(rows, self.num_frames, self.image_size, self.image_size, unet.out_dim),
                   t=new(rows, dtype=torch.int32), step=new(1, dtype=torch.int64), thres=new(B) if self.use_dynamic_thres else None,
                   xin=torch.zeros((B, 2 * self.channels) + shape[2:], dtype=torch.float32, device=dev) if xin else None,
                   known=new(one) if known else None, mask=new(one, dtype=torch.uint8) if known else None,
                   hist=new(one) if hist else None, seq=None if seq_host is None else torch.from_numpy(seq_host).to(dev))
        if keep is not None:
            self._chain_buf = buf
        return buf

    def _chain_net(self, rows, cond):
        """(cond on the device or None, handle, workspace) of a chain over `rows` network rows, the handle's activation storage set.  A
        condition is used un-masked (the reference drops it, Q10); a network without one ignores it."""
        unet = self.denoise_fn
        condd = None if (cond is None or not unet.has_cond) else self._dev(cond)
        h = unet.handle(self.num_frames, self.image_size)
        unet.apply_activation_storage(h)
        return condd, h, unet.workspace(rows, self.num_frames, self.image_size)

    def _run_chain(self, chain, B, key, *, steps=0, order=2, cond=None, cond_scale=1.0, guidance_rescale=0.0, use_graph=True, x_T=None,
                   masked=None, lowres=None, aug_level=None):
        """One whole chain on the current stream (inside _sampling()): chain 'ddpm' (the T-step ancestral one) | 'ddim' | 'dpm' (the
        two over ddim_time_sequence(T, steps)) -> the entry _LOOPS[chain, variant], captured in a hipGraph (use_graph) or run eagerly by
        the same step function.  x_T = noise(shape, key, 0) unless given (Philox(key, draw 0)), step k draws 1 + k.  The variants:
          plain
          guided  cond given, the network has a condition, cond_scale != 1 (classifier-free guidance, EXTENSION, parity unpinned: the
                  reference's p_sample_loop drops cond): one forward over 2B rows (conditioned | null embedding) per step, so img / eps /
                  t hold 2B rows and the first B are the result.
          mixed   frame_noise_alpha > 0 on the ancestral chain, plain or guided (the guided entry's arguments + (a, b)); the two
                  deterministic chains change in x_T only.
          masked  masked = (video, element mask, mask table, resample_steps): the loop of inpaint() on kept buffers; masked and guided
                  together run eagerly (_masked_guided_steps).
          sr      lowres given (a super-resolution diffusion): u is written once into the second half of xin (vdx_lowres_input,
                  augmentation draw VDX_DRAW_LOWRES of the seed), the captured step is lowres_pack -> forward(xin) -> the plain step on
                  img; kept buffers.  A self-conditioned diffusion runs the same entries: the second half of xin is zeroed here and
                  the step (the handle's self-condition state, _sampling) writes x0~ into it behind the forward, for the next one.
          lv      a learned-variance diffusion: steps = S (None: T) levels of the respaced ancestral chain; unnormalize_img is folded into
                  the last step (post_scale = post_shift = 0.5), every other variant runs it as a launch of its own.
        Returns unnormalize_img(x_0) [B,C,F,H,W] in [0, 1]."""
        unet, T = self.denoise_fn, self.num_timesteps
        seed = int(key) & 0xFFFFFFFFFFFFFFFF
        shape = (B, self.channels, self.num_frames, self.image_size, self.image_size)
        guided = cond is not None and unet.has_cond and cond_scale != 1
        if self.self_condition and (guided or masked is not None or lowres is not None):
            raise ValueError('self_condition runs the plain chains over xin: no guidance, no known region, no low-resolution clip')
        variant = 'sr' if (lowres is not None or self.self_condition) else 'lv' if self.learned_variance else 'masked' if masked is not None else \
            'guided' if guided else 'plain'
        named = {}
        if variant == 'lv':
            seq, lv_tab, steps = self._lv_tables(steps)
            seq_host = None
            named.update(lv_tab=L.ptr(lv_tab), post_scale=0.5, post_shift=0.5)
        else:
            seq_host = None if chain == 'ddpm' else ddim_time_sequence(T, steps)
        # (the lv chain's sequence is lv_time_sequence's, whose first level is T - 1 for every S: no read of the device sequence for it)
        t0 = T - 1 if seq_host is None else int(seq_host[0])
        rows = 2 * B if variant == 'guided' else B                 # what the forward covers
        buf = self._chain_bufs(B, rows, xin=variant == 'sr', known=variant == 'masked', hist=chain == 'dpm', seq_host=seq_host,
                               keep=(variant, B, chain, steps) if variant in ('masked', 'sr') else None)
        img = buf['img']
        # the start state: x_T in the first B rows (and, for the captured loops below, every row at level t0, step 0)
        if x_T is None:
            self.noise(shape, seed, 0, out=img)
        else:
            img[:B].copy_(self._dev(x_T))
        nsteps = T if (chain == 'ddpm' and variant != 'lv') else steps
        if variant == 'masked':
            video, m, mtab, U = masked
            known, mk = buf['known'], buf['mask']
            L.check(vdx_affine(L.ptr(self._dev(video)), L.ptr(known), img.numel(), 2.0, -1.0, L.stream_ptr()))      # normalize_img
            mk.copy_(m)
            L.check(vdx_inpaint_init(L.ptr(img), L.ptr(known), L.ptr(mk), L.ptr(mtab), T, t0, img.numel(), L.stream_ptr()))
            named.update(known=L.ptr(known), mask=L.ptr(mk), mtab=L.ptr(mtab), resample=U)
            nsteps *= U if chain == 'ddpm' else 1
        elif self.self_condition:
            buf['xin'][:, self.channels:].zero_()                         # x0~ = 0 at step 0 (the buffers are kept across calls)
        elif variant == 'sr':
            self.lowres_condition(lowres, seed, aug_level, draw=L.DRAW_LOWRES, out=buf['xin'])
        if guided and variant == 'masked':
            self._masked_guided_steps(chain, buf, seq_host, cond, cond_scale, order, U, mtab, seed)
        else:
            buf['t'].fill_(t0)
            buf['step'].zero_()
            condd, h, ws = self._chain_net(rows, cond)
            named.update(cond_scale=1.0, rescale=0.0, scratch=0)
            if variant == 'guided':
                assert tuple(condd.shape) == (B, unet.cond_dim), f'cond must be [{B}, {unet.cond_dim}], got {tuple(condd.shape)}'
                scratch = torch.empty(L.vdx_cfg_scratch_doubles(B), dtype=torch.float64, device=self.device)
                named.update(cond_scale=float(cond_scale), rescale=float(guidance_rescale), scratch=L.ptr(scratch))
            entry = variant
            if chain == 'ddpm' and self.frame_noise_alpha and variant in ('plain', 'guided'):
                entry = 'mixed'
                named.update(mix_a=self._mix[0], mix_b=self._mix[1])
            named.update(h=h.ptr, params=L.ptr(unet.flat_params), packed=L.ptr(unet.packed()), img=L.ptr(img), xin=L.ptr(buf['xin']),
                         eps=L.ptr(buf['eps']), hist=L.ptr(buf['hist']), t_dev=L.ptr(buf['t']), step_dev=L.ptr(buf['step']),
                         tables=L.ptr(self._ptab), timesteps=T, nsteps=nsteps, cond=L.ptr(condd), seed=seed, clip=1, order=order,
                         percentile=float(self.dynamic_thres_percentile) if self.use_dynamic_thres else 0.0, thres=L.ptr(buf['thres']),
                         ac=L.ptr(self.alphas_cumprod), seq=L.ptr(seq if variant == 'lv' else buf['seq']), seq_len=steps,
                         ws=L.ptr(ws), ws_bytes=ws.numel(), batch=B, use_graph=int(use_graph), stream=L.stream_ptr())
            L.check(_LOOPS[chain, entry](*loop_args(chain, entry, named)))
        if variant == 'lv':
            return img
        img = img[:B]
        out = torch.empty_like(img)
        L.check(vdx_affine(L.ptr(img), L.ptr(out), img.numel(), 0.5, 0.5, L.stream_ptr()))     # unnormalize_img
        return out

    def _masked_guided_steps(self, chain, buf, seq_host, cond, cond_scale, order, U, mtab, seed):
        """The masked chain under guidance, in place on buf['img']: two forwards per step (forward_with_cond_scale) and the masked step
        kernels, eagerly, with the step numbering of the captured loops."""
        unet, T = self.denoise_fn, self.num_timesteps
        img, known, mk = buf['img'], buf['known'], buf['mask']
        B, per = img.shape[0], self._per_sample(img)

        def eps_and_thres(t):
            eps_hat = self._eps_from_out(unet.forward_with_cond_scale(img, t, cond=cond, cond_scale=cond_scale), img, t)
            return eps_hat, (self._dynamic_threshold(img, t, eps_hat) if self.use_dynamic_thres else None)

        if chain == 'ddpm':
            s = 0
            for i in reversed(range(T)):
                t = torch.full((B,), i, dtype=torch.int32, device=self.device)
                for _ in range(U):
                    eps_hat, th = eps_and_thres(t)
                    L.check(vdx_p_sample_step_masked(L.ptr(img), L.ptr(eps_hat), L.ptr(img), L.ptr(t), L.ptr(self._ptab), T, L.ptr(known),
                                                     L.ptr(mk), L.ptr(mtab), U, seed, s, 0, L.ptr(th), 1, B, self.channels, per, L.stream_ptr()))
                    s += 1
            return
        for j in range(len(seq_host) - 1):
            t = torch.full((B,), int(seq_host[j]), dtype=torch.int32, device=self.device)
            eps_hat, th = eps_and_thres(t)
            buf['step'].fill_(j)
            if chain == 'dpm':
                L.check(vdx_dpm_step_masked(L.ptr(img), L.ptr(eps_hat), L.ptr(img), L.ptr(buf['hist']), L.ptr(self.alphas_cumprod),
                                            L.ptr(buf['seq']), L.ptr(buf['step']), L.ptr(th), 1, order, L.ptr(known), L.ptr(mk),
                                            L.ptr(mtab), T, seed, B, self.channels, per, L.stream_ptr()))
            else:
                L.check(vdx_ddim_step_masked(L.ptr(img), L.ptr(eps_hat), L.ptr(img), L.ptr(self.alphas_cumprod), L.ptr(buf['seq']),
                                             L.ptr(buf['step']), L.ptr(th), 1, L.ptr(known), L.ptr(mk), L.ptr(mtab), T, seed,
                                             B, self.channels, per, L.stream_ptr()))

    def p_sample_loop(self, shape, key, cond=None, cond_scale: float = 1.0, *, use_graph: bool = True, x_T=None,
                      guidance_rescale: float = 0.0, focus_present=None, steps: Optional[int] = None):
        """reference :264-320.  As there, the caller's spatial `shape` is replaced by the model's own (Q10).

        x_T = Philox(key, draw 0); step k (t = T-1-k) uses draw 1+k.  Returns unnormalize_img(x_0) in [0,1].
        With cond given and cond_scale != 1 the loop is the guided one (classifier-free guidance: one forward over 2B samples per
        step, inside the captured step like the unguided loop; _run_chain) -- an EXTENSION, parity unpinned: the reference drops cond
        here.  guidance_rescale phi in [0, 1] (extension; Lin et al. 2023, sec. 3.4): the guided eps is scaled per sample by
        phi std(eps(c)) / std(eps_guided) + 1 - phi; 0 = off.
        steps (learned_variance only): sample with the respaced S-level ancestral chain (make_lv_tables) instead of all T levels.
        """
        guidance_rescale = check_guidance_rescale(guidance_rescale)
        self._sr_need_lowres('p_sample_loop', 'upsample(key, lowres)')
        self._refuse('self_condition', cond_scale=cond_scale, guidance_rescale=guidance_rescale)
        if self.learned_variance:
            self._refuse('learned_variance', cond_scale=cond_scale, guidance_rescale=guidance_rescale, focus_present=focus_present)
            lv_time_sequence(self.num_timesteps, steps)                   # (its range check, before any device work)
            with self._sampling(None, int(shape[0])):
                return self._run_chain('ddpm', int(shape[0]), key, steps=steps, cond=cond, use_graph=use_graph, x_T=x_T)
        if steps is not None:
            raise ValueError('steps is the respaced chain of a learned_variance diffusion; use ddim_steps / dpm_steps otherwise')
        with self._sampling(focus_present, int(shape[0])):
            return self._run_chain('ddpm', int(shape[0]), key, cond=cond, cond_scale=cond_scale, guidance_rescale=guidance_rescale,
                                   use_graph=use_graph, x_T=x_T)

    def ddim_sample_loop(self, shape, key, steps: int = 100, cond=None, cond_scale: float = 1.0, *, use_graph: bool = True, x_T=None,
                         guidance_rescale: float = 0.0, focus_present=None):
        """DDIM sampling with eta = 0 in `steps` network evaluations (EXTENSION, BASELINE.json configs[3]; the reference has ancestral
        sampling only).  x_T = Philox(key, draw 0), deterministic afterwards.  Returns unnormalize_img(x_0) in [0, 1].  cond with
        cond_scale != 1 and guidance_rescale: as p_sample_loop (the guided loop, captured too)."""
        self._refuse('learned_variance', ddim_steps=steps)
        self._sr_need_lowres('ddim_sample_loop', 'upsample(key, lowres, ddim_steps=S)')
        guidance_rescale = check_guidance_rescale(guidance_rescale)
        self._refuse('self_condition', cond_scale=cond_scale, guidance_rescale=guidance_rescale)
        ddim_time_sequence(self.num_timesteps, steps)                     # (its range check, before any device work)
        with self._sampling(focus_present, int(shape[0])):
            return self._run_chain('ddim', int(shape[0]), key, steps=int(steps), cond=cond, cond_scale=cond_scale,
                                   guidance_rescale=guidance_rescale, use_graph=use_graph, x_T=x_T)

    def dpm_sample_loop(self, shape, key, steps: int = 20, order: int = 2, cond=None, cond_scale: float = 1.0, *, use_graph: bool = True,
                        x_T=None, guidance_rescale: float = 0.0, focus_present=None):
        """DPM-Solver++(2M) sampling in `steps` network evaluations (EXTENSION, parity unpinned: no reference code; Lu et al. 2022,
        data-prediction multistep form, the step of vdx.h).  order 2 reaches in 15-25 steps what DDIM (= order 1) needs about 100 for;
        the cost per step is DDIM's plus one history tensor.  x_T = Philox(key, draw 0), deterministic afterwards.  Returns
        unnormalize_img(x_0) in [0, 1].  cond with cond_scale != 1 and guidance_rescale: as p_sample_loop (the guided loop, captured too)."""
        self._refuse('learned_variance', dpm_steps=steps)
        self._sr_need_lowres('dpm_sample_loop', 'upsample(key, lowres, dpm_steps=S)')
        check_dpm_args(self.num_timesteps, steps, order)
        guidance_rescale = check_guidance_rescale(guidance_rescale)
        self._refuse('self_condition', cond_scale=cond_scale, guidance_rescale=guidance_rescale)
        with self._sampling(focus_present, int(shape[0])):
            return self._run_chain('dpm', int(shape[0]), key, steps=int(steps), order=order, cond=cond, cond_scale=cond_scale,
                                   guidance_rescale=guidance_rescale, use_graph=use_graph, x_T=x_T)

    def calc_bpd_loop(self, x, key, *, cond=None, clip_denoised: bool = True, timesteps: Optional[int] = None, use_graph: bool = True,
                      focus_present=None):
        """The variational bound of held-out videos x [B,C,F,H,W] in [0, 1] in bits per dimension, term by term (EXTENSION, no reference
        code: Ho et al. 2020, eq. 5; Nichol & Dhariwal 2021, calc_bpd_loop; the math is vdx.h's "Held-out evaluation").  One network
        evaluation per level inside a captured step (vdx_vlb_loop), the noise of step k = Philox(key, draw 1 + k), the per-sample sums
        deterministic.  timesteps None: all T levels, T-1 .. 0; an int S: the ddim_time_sequence(T, S) levels, a cheap per-t curve.
        cond is used un-masked, as the unguided sampling loops use it.  Returns CPU float64 tensors: vb, mse, xstart_mse [B,S] (column
        k = level t[k]), t [S], prior_bpd [B] and total_bpd [B] = prior_bpd + sum_t vb, None unless every level was visited.
        The model's variance is the posterior variance p_sample uses; the dynamic threshold has no place in the bound.
        learned_variance: the KL and decoder terms use the model's own log sigma^2 (vdx_vlb_loop_lv)."""
        self._refuse('learned_variance', focus_present=focus_present)
        self._refuse('lowres_cond', calc_bpd_loop=True)
        self._refuse('frame_noise_alpha', calc_bpd_loop=True)             # (the KL terms need the inverse frame covariance)
        self._refuse('self_condition', calc_bpd_loop=True)                # (the bound of a chain that feeds on its own estimates: a follow-up)
        return self._bpd_chain(x, key, cond, clip_denoised, timesteps, use_graph, focus_present, None)

    def _bpd_chain(self, x, key, cond, clip_denoised, timesteps, use_graph, focus_present, pieces):
        """calc_bpd_loop; pieces: the step counts of the vdx_vlb_loop calls the chain is issued in (None: one call over all of it)."""
        if self.use_dynamic_thres:
            raise ValueError('calc_bpd_loop evaluates the statically clipped x0 only: a diffusion with use_dynamic_thres is not supported')
        unet, T, dev = self.denoise_fn, self.num_timesteps, self.device
        seq_host = vlb_time_sequence(T, timesteps)
        S = len(seq_host) - 1
        x = torch.as_tensor(x)
        shape = (self.channels, self.num_frames, self.image_size, self.image_size)
        if x.dim() != 5 or tuple(x.shape[1:]) != shape:
            raise ValueError(f'x must be [B, {shape[0]}, {shape[1]}, {shape[2]}, {shape[3]}], got {tuple(x.shape)}')
        from . import ops
        B, seed = x.shape[0], int(key) & 0xFFFFFFFFFFFFFFFF
        tab = self._lv_tab64() if self.learned_variance else torch.from_numpy(make_vlb_tables(T)).to(dev)
        vlb_loop = L.vdx_vlb_loop_lv if self.learned_variance else L.vdx_vlb_loop
        with self._sampling(focus_present, B):
            xd = self._dev(x)
            prior = ops.vlb_prior(xd, tab)
            buf = self._chain_bufs(B, seq_host=seq_host)                  # (img serves as x_t)
            buf['t'].fill_(int(seq_host[0]))
            buf['step'].zero_()
            partial = torch.empty(L.vdx_vlb_scratch_doubles(B), dtype=torch.float64, device=dev)
            out = torch.empty(S, B, 3, dtype=torch.float64, device=dev)
            condd, h, ws = self._chain_net(B, cond)
            for n in (pieces or (S,)):
                L.check(vlb_loop(h.ptr, L.ptr(unet.flat_params), L.ptr(unet.packed()), L.ptr(xd), L.ptr(buf['img']), L.ptr(buf['eps']),
                                 L.ptr(buf['t']), L.ptr(buf['step']), L.ptr(tab), T, L.ptr(buf['seq']), S, int(n), L.ptr(condd), seed,
                                 int(bool(clip_denoised)), L.ptr(partial), L.ptr(out), L.ptr(ws), ws.numel(), B, int(use_graph), L.stream_ptr()))
            res = out.cpu()
            prior = prior.cpu()
        vb = res[:, :, 0].t().contiguous()
        return dict(vb=vb, mse=res[:, :, 1].t().contiguous(), xstart_mse=res[:, :, 2].t().contiguous(),
                    t=torch.from_numpy(seq_host[:-1].astype(np.int64)), prior_bpd=prior,
                    total_bpd=prior + vb.sum(1) if S == T else None)

    @staticmethod
    def _shard(key, batch, *tensors):
        """This rank's share of a data-parallel sampling batch: (key, batch, *tensors) with the rank's rows of every tensor that is not
        None and its own Philox stream shard_key(key, rank); outside a group (one rank) everything as given."""
        rank, world = dist_rank_world()
        if world == 1:
            return (key, batch) + tensors
        assert batch % world == 0, 'batch_size must be divisible by number of devices'      # as reference trainer.py:163
        per = batch // world
        return (shard_key(key, rank, world), per) + tuple(None if t is None else t[rank * per:(rank + 1) * per] for t in tensors)

    def sample(self, key, cond=None, cond_scale: float = 1.0, batch_size: int = 16, *, ddim_steps: Optional[int] = None,
               dpm_steps: Optional[int] = None, dpm_order: int = 2, guidance_rescale: float = 0.0, focus_present=None,
               steps: Optional[int] = None, lowres=None, lowres_aug_level=None, **kw):
        """reference :323-357.  lowres (a super-resolution diffusion only, and required there): the low-resolution clips; the call is
        upsample(key, lowres, aug_level=lowres_aug_level, ...) -- single process, no rank sharding.  ddim_steps (extension): sample with an S-step DDIM chain instead of the T-step ancestral one.
        dpm_steps (extension): an S-step DPM-Solver++(2M) chain of order dpm_order (dpm_sample_loop); not together with ddim_steps.
        guidance_rescale (extension): the rescale phi in [0, 1] of the guided loops (cond given, cond_scale != 1; p_sample_loop).
        steps (extension, learned_variance only): the respaced S-level ancestral chain with the model's variance (p_sample_loop).

        Data parallel (reference :278-298: the batch is split over the local devices, `P('data')`): inside an initialised
        torch.distributed group of W > 1 ranks, `batch_size` (and `cond`) describe the GLOBAL batch; rank r draws videos
        [r * per, (r + 1) * per), per = batch_size / W, from its own Philox stream shard_key(key, r) and returns ITS shard --
        no data-path collective.  W = 1 uses `key` itself (single-process behaviour unchanged)."""
        self._refuse('learned_variance', cond_scale=cond_scale, ddim_steps=ddim_steps, dpm_steps=dpm_steps, guidance_rescale=guidance_rescale,
                     focus_present=focus_present)
        self._refuse('self_condition', cond_scale=cond_scale, guidance_rescale=guidance_rescale)
        if self.lowres_cond is not None:
            self._refuse('lowres_cond', cond_scale=cond_scale, guidance_rescale=guidance_rescale, focus_present=focus_present, steps=steps)
            if lowres is None:
                raise ValueError('lowres_cond (super-resolution): sample needs lowres=[B, C, F/ft, S/fs, S/fs], the clips to upsample')
            return self.upsample(key, lowres, aug_level=lowres_aug_level, cond=cond, ddim_steps=ddim_steps, dpm_steps=dpm_steps,
                                 dpm_order=dpm_order, **{k: v for k, v in kw.items() if k in ('use_graph', 'x_T')})
        if lowres is not None or lowres_aug_level is not None:
            raise ValueError('lowres / lowres_aug_level need a super-resolution diffusion (lowres_cond=(ft, fs))')
        if steps is not None:
            if not self.learned_variance:
                raise ValueError('steps is the respaced chain of a learned_variance diffusion; use ddim_steps / dpm_steps otherwise')
            lv_time_sequence(self.num_timesteps, steps)                       # (its range check, before any device work)
            kw['steps'] = int(steps)
        chain, chain_steps = chain_choice(self.num_timesteps, ddim_steps, dpm_steps, dpm_order)
        kw['guidance_rescale'] = check_guidance_rescale(guidance_rescale)
        if is_list_str(cond):
            raise NotImplementedError('text -> BERT embedding needs the external video_diffusion_pytorch.text (network fetch); '
                                      'pass a ready [B, 768] tensor instead')
        if cond is not None:
            batch_size = cond.shape[0]
        # focus_present (extension): True, or a [batch] mask sharded over the ranks with the batch -- the loops' focus_present
        fp = focus_present if isinstance(focus_present, (bool, type(None))) else torch.as_tensor(focus_present)
        if isinstance(fp, torch.Tensor) and fp.shape != (batch_size,):
            raise ValueError(f'focus_present must be True or a [{batch_size}] mask, got {tuple(fp.shape)}')
        key, batch_size, cond, fp_shard = self._shard(key, batch_size, cond, fp if isinstance(fp, torch.Tensor) else None)
        kw['focus_present'] = fp_shard if isinstance(fp, torch.Tensor) else fp
        shape = (batch_size, self.channels, self.num_frames, self.image_size, self.image_size)
        if chain == 'dpm':
            return self.dpm_sample_loop(shape, key, steps=chain_steps, order=dpm_order, cond=cond, cond_scale=cond_scale, **kw)
        if chain == 'ddim':
            return self.ddim_sample_loop(shape, key, steps=chain_steps, cond=cond, cond_scale=cond_scale, **kw)
        return self.p_sample_loop(shape, key, cond=cond, cond_scale=cond_scale, **kw)

    def inpaint(self, key, video, mask, *, cond=None, cond_scale: float = 1.0, ddim_steps: Optional[int] = None, resample_steps: int = 1,
                use_graph: bool = True, x_T=None, dpm_steps: Optional[int] = None, dpm_order: int = 2, clean_context: bool = False, focus_present=None):
        """Frame-conditioned sampling (EXTENSION): generate the unknown part of `video` ([B,C,F,H,W] in [0,1]) with the
        unconditionally trained denoiser by the replacement method (Ho et al. 2022, sec. 3.1); resample_steps U > 1 adds RePaint
        resampling (Lugmayr et al. 2022, ancestral chain only).  mask: [F], [B,F] or broadcastable to `video`, bool / uint8, 1 = known
        (frame_mask).  ddim_steps S: an S-step DDIM chain (eta = 0) instead of the T-step ancestral one; dpm_steps S: an S-step
        DPM-Solver++(2M) chain of order dpm_order (vdx_dpm_step_masked).  The known region of the result is `video` up to one affine
        rounding; an all-zero mask with U = 1 is p_sample_loop / ddim_sample_loop / dpm_sample_loop.
        Data parallel as sample(): `video` (and `mask`, `cond`, `x_T`) are the GLOBAL batch, rank r returns its rows, drawn with
        shard_key(key, r).  Draws: vdx.h (VDX_DRAW_KNOWN, VDX_DRAW_RENOISE).
        clean_context=True is for a denoiser trained with frame conditioning (Trainer.frame_cond_max > 0; RaMViD, Hoeppe et al. 2022):
        the known region is `video` itself, un-noised, in the start tensor and after every step of all three chains (the same kernels
        with the (1, 0) mask table, vdx.h), as such a network saw its context frames in training.  Not with resample_steps > 1."""
        self._refuse('learned_variance', inpaint=True)
        self._refuse('lowres_cond', inpaint=True)
        self._refuse('frame_noise_alpha', inpaint=True)       # (the known region's noise would have to share s with the generated frames)
        self._refuse('self_condition', inpaint=True)          # (there is no masked loop over xin)
        if focus_present is not None:
            raise ValueError('inpaint / extend do not take focus_present (frame-conditioned sampling of a focus-present sample is out of scope)')
        opts = self._inpaint_options(video, dict(cond_scale=cond_scale, ddim_steps=ddim_steps, resample_steps=resample_steps, use_graph=use_graph,
                                                 x_T=x_T, dpm_steps=dpm_steps, dpm_order=dpm_order, clean_context=clean_context))
        m = frame_mask(mask, tuple(video.shape))
        key, _, video, m, cond, opts['x_T'] = self._shard(key, video.shape[0], video, m, cond, x_T)
        return self._inpaint_local(key, video, m, cond, **opts)

    def _inpaint_options(self, video, kw):
        """The sampler options of inpaint() / extend() out of the keywords `kw`, resolved and checked once, before any device work:
        the keywords of _inpaint_local.  `video`: a tensor of the shape one call of the loop works on."""
        o = dict(cond_scale=kw.get('cond_scale', 1.0), use_graph=kw.get('use_graph', True), x_T=kw.get('x_T'),
                 resample_steps=kw.get('resample_steps', 1), dpm_order=kw.get('dpm_order', 2), clean_context=bool(kw.get('clean_context', False)))
        ddim_steps, dpm_steps = kw.get('ddim_steps'), kw.get('dpm_steps')
        if int(o['resample_steps']) < 1:
            raise ValueError(f"resample_steps must be >= 1, got {o['resample_steps']}")
        if o['clean_context'] and int(o['resample_steps']) > 1:
            raise ValueError('clean_context keeps the known frames un-noised; resampling (resample_steps > 1) re-noises the whole tensor')
        o['chain'], o['steps'] = chain_choice(self.num_timesteps, ddim_steps, dpm_steps, o['dpm_order'], o['resample_steps'])
        if ddim_steps and int(o['resample_steps']) > 1:
            raise ValueError('resampling (resample_steps > 1) is defined for the ancestral chain only, not with ddim_steps')
        shape = tuple(video.shape)
        if len(shape) != 5 or shape[1:] != (self.channels, self.num_frames, self.image_size, self.image_size):
            raise ValueError(f'video must be [B, {self.channels}, {self.num_frames}, {self.image_size}, {self.image_size}], got {shape}')
        if o['x_T'] is not None and tuple(o['x_T'].shape) != shape:
            raise ValueError(f"x_T must have the shape of video {shape}, got {tuple(o['x_T'].shape)}")
        o['resample_steps'] = int(o['resample_steps'])
        return o

    def _inpaint_local(self, key, video, m, cond, *, chain, steps, cond_scale, resample_steps, use_graph, x_T, dpm_order, clean_context):
        """inpaint() on this rank's rows, with the options of _inpaint_options."""
        mtab = self._mtab_clean if clean_context else self._mtab      # (1, 0) rows: the known region is `known` at every level
        with self._sampling():
            return self._run_chain(chain, video.shape[0], key, steps=steps, order=dpm_order, cond=cond, cond_scale=cond_scale,
                                   use_graph=use_graph, x_T=x_T, masked=(video, m, mtab, resample_steps))

    def extend(self, key, video, num_new_frames: int, *, context_frames: Optional[int] = None, **inpaint_kw):
        """Grow `video` ([B,C,F0,H,W] in [0,1], any F0 >= 1) by `num_new_frames` frames, autoregressively (EXTENSION): window w
        holds the last `ctx` frames so far as known frames and generates the next ones with inpaint() (extend_plan; context_frames
        defaults to num_frames // 2).  Window keys: split_key(key, n_windows).  Returns [B,C,F0 + N,H,W]; its first F0 frames are
        `video` itself.  Data parallel as sample(): sharded once (rows and shard_key), not per window.  clean_context=True (with a
        frame-conditioned denoiser): every window keeps its context frames un-noised, see inpaint()."""
        self._refuse('learned_variance', extend=True)
        self._refuse('lowres_cond', extend=True)
        self._refuse('frame_noise_alpha', extend=True)
        self._refuse('self_condition', extend=True)
        ctx = self.num_frames // 2 if context_frames is None else int(context_frames)
        video = torch.as_tensor(video)
        if video.dim() != 5 or tuple(video.shape[1:2] + video.shape[3:]) != (self.channels, self.image_size, self.image_size):
            raise ValueError(f'video must be [B, {self.channels}, F, {self.image_size}, {self.image_size}], got {tuple(video.shape)}')
        plan = extend_plan(video.shape[2], int(num_new_frames), self.num_frames, ctx)
        # (a keyword inpaint() does not have is ignored here, as it always was; with nothing to generate nothing is checked either)
        opts = self._inpaint_options(video.new_zeros((video.shape[0], self.channels, self.num_frames, self.image_size, self.image_size)),
                                     inpaint_kw) if plan else None
        key, _, video, cond = self._shard(key, video.shape[0], video, inpaint_kw.get('cond'))
        video = self._dev(video)
        B, F0 = video.shape[0], video.shape[2]
        clip = torch.empty(B, self.channels, F0 + int(num_new_frames), self.image_size, self.image_size, device=self.device)
        clip[:, :, :F0] = video
        window = torch.zeros(B, self.channels, self.num_frames, self.image_size, self.image_size, device=self.device)
        have = F0
        for (c, n), k in zip(plan, split_key(key, len(plan))):
            window[:, :, :c] = clip[:, :, have - c:have]
            frames = torch.arange(self.num_frames, device=self.device) < c
            m = frame_mask(frames, tuple(window.shape))
            out = self._inpaint_local(k, window, m, cond, **opts)
            clip[:, :, have:have + n] = out[:, :, c:c + n]
            have += n
        return clip

    def interpolate(self, x1, x2, t: Optional[int] = None, lam: float = 0.5, key: int = 0):
        """reference :360-398 with the intended behaviour (the reference omits the mandatory keys, Q18)."""
        b = x1.shape[0]
        t = t if t is not None else self.num_timesteps - 1
        assert x1.shape == x2.shape and 0.0 <= lam <= 1.0
        tb = torch.full((b,), t, dtype=torch.int32, device=self.device)
        k1, k2, k3 = split_key(key, 3)
        img = (1 - lam) * self.q_sample(x1, tb, k1) + lam * self.q_sample(x2, tb, k2)
        for n, i in enumerate(reversed(range(0, t))):
            img = self.p_sample(img, torch.full((b,), i, dtype=torch.int32, device=self.device), split_key(k3, n + 1)[-1])
        return img

    # -- forward process / loss ----------------------------------------------------------------------
    def q_sample(self, x_start, t, key=None, noise=None, *, frame_mask=None, _pre=(1.0, 0.0)):
        """reference :401-420.  frame_mask (extension, frame-conditioned training): [F], [B,F] or anything frame_mask() takes, 1 = the
        element stays clean (x_start, normalised), 0 = noised to level t (vdx_q_sample_masked); None = the reference's q_sample."""
        x_start = self._dev(x_start)
        t32 = self._dev(t, torch.int32)
        if noise is None:
            assert key is not None, 'A key must be provided to q_sample if noise is not.'
            noise = self.noise(x_start.shape, key, 0)
        noise = self._dev(noise)
        out = torch.empty_like(x_start)
        if frame_mask is not None:
            mk = self._dev_mask(frame_mask, x_start.shape)
            L.check(vdx_q_sample_masked(L.ptr(x_start), L.ptr(t32), L.ptr(noise), L.ptr(mk), L.ptr(out), L.ptr(self.sqrt_alphas_cumprod),
                                        L.ptr(self.sqrt_one_minus_alphas_cumprod), x_start.shape[0], self._per_sample(x_start),
                                        float(_pre[0]), float(_pre[1]), L.stream_ptr()))
            return out
        L.check(vdx_q_sample(L.ptr(x_start), L.ptr(t32), L.ptr(noise), L.ptr(out), L.ptr(self.sqrt_alphas_cumprod),
                             L.ptr(self.sqrt_one_minus_alphas_cumprod), x_start.shape[0], self._per_sample(x_start),
                             float(_pre[0]), float(_pre[1]), L.stream_ptr()))
        return out

    def p_losses(self, x_start, t, key=None, cond=None, noise=None, *, frame_mask=None, _pre=(1.0, 0.0), lowres=None, aug_levels=None,
                 self_cond=None, self_cond_prob: float = 0.5, **kwargs):
        """reference :423-470 (forward value; the training step with gradients lives in trainer.py).  frame_mask (extension, RaMViD
        frame conditioning; forms as q_sample's): the masked frames enter the denoiser clean and the loss is the mean over the other
        elements, sum / max(count, 1), formed on the device (vdx_loss_sum_masked).  self_cond (a self-conditioned diffusion only): None
        -- the coin of the two-pass objective is drawn with probability self_cond_prob under self_cond_key(key) (without a key: False);
        False / True / a ready [B,C,F,H,W] estimate: self_cond_input."""
        if self.loss_type not in ('l1', 'l2'):
            raise ValueError(f'Unsupported loss type: {self.loss_type}')
        self._refuse('learned_variance', frame_mask=frame_mask, focus_present=kwargs.get('focus_present_mask'))
        self._refuse('lowres_cond', frame_mask=frame_mask, focus_present=kwargs.get('focus_present_mask'))
        self._refuse('objective', frame_mask=frame_mask)                  # (the masked loss is a (sum, count) form without levels)
        self._refuse('self_condition', frame_mask=frame_mask)
        if self_cond is not None and not self.self_condition:
            raise ValueError('self_cond needs a self-conditioned diffusion (self_condition=True)')
        if self.lowres_cond is None and (lowres is not None or aug_levels is not None):
            raise ValueError('lowres / aug_levels need a super-resolution diffusion (lowres_cond=(ft, fs))')
        if self.lowres_cond is not None:
            if lowres is not None:
                self._sr_lowres(lowres, x_start.shape[0])
            aug_levels = self._sr_levels(aug_levels, x_start.shape[0])
        x_start = self._dev(x_start)
        t32 = self._dev(t, torch.int32)
        if noise is None:
            assert key is not None
            _, noise_key, _ = split_key(key, 3)
            noise = self.noise(x_start.shape, noise_key, 0)
        noise = self._dev(noise)
        if is_list_str(cond):
            raise NotImplementedError('pass text conditioning as a ready embedding tensor')
        mk = None if frame_mask is None else self._dev_mask(frame_mask, x_start.shape)
        x_noisy, _ = self._net_input(x_start, t32, noise, mask=mk, lowres=lowres, aug_levels=aug_levels,
                                     aug_key=None if key is None else lowres_aug_key(key), _pre=_pre)
        if self.self_condition:
            # the coin of the two-pass objective: given, or drawn under child 5 of the loss key with probability self_cond_prob
            if self_cond is None:
                g = None if key is None else torch.Generator().manual_seed(self_cond_key(key) & 0x7FFFFFFFFFFFFFFF)
                self_cond = False if key is None else self_cond_draw(self_cond_prob, g)
            x_noisy = self.self_cond_input(x_noisy, t32, self_cond, lambda xin: self.denoise_fn(xin, t32, cond=cond, **kwargs))
        eps_hat = self.denoise_fn(x_noisy, t32, cond=cond, **kwargs)
        return self.loss_and_grad(eps_hat, x_start, noise, t32, mask=mk, _pre=_pre)[0]

    def _net_input(self, x_start, t32, noise, *, mask=None, lowres=None, aug_levels=None, aug_key=None, _pre=(1.0, 0.0)):
        """(network input, augmentation levels) of the objective, everything on the device: q_sample of x_start (masked with `mask`) or,
        for a super-resolution diffusion, xin = [ x_t | aug(up(2 lowres - 1)) ] (sr_input): lowres defaults to the box mean of the raw
        clip, aug_levels to a host draw from {0..lowres_aug_max-1} under aug_key (none with lowres_aug_max = 0), and the augmentation
        noise is Philox(aug_key, draw 0)."""
        if self.lowres_cond is None:
            return self.q_sample(x_start, t32, noise=noise, frame_mask=mask, _pre=_pre), None
        if aug_levels is None and self.lowres_aug_max > 0:
            assert aug_key is not None, 'A key must be provided to p_losses for the augmentation draw.'
            aug_levels = lowres_aug_levels(x_start.shape[0], self.lowres_aug_max, aug_key)
        return self.sr_input(x_start, t32, noise, lowres=lowres, aug_levels=aug_levels, key=aug_key or 0, _pre=_pre), aug_levels

    def loss_and_grad(self, eps_hat, x_start, noise, t32, *, mask=None, iw=None, want_grad: bool = False, _pre=(1.0, 0.0)):
        """(loss, d_eps): the objective of the network output eps_hat as a float32 device scalar and, with want_grad, its gradient in
        eps_hat (else None); the host reads nothing.  By what is on:
          learned_variance  the hybrid loss of eps_hat | v (hybrid_loss: last_loss_terms, last_loss_per_sample; iw -> vdx_hybrid_loss_w)
          mask              the mean over the mask-0 elements (masked_loss, vdx_loss_grad_masked: the count stays on the device)
          iw                float64 [B] importance weights (loss-aware timestep sampling): the weighted mean and gradient from one
                            vdx_loss_weighted pass; last_loss_per_sample = the unweighted per-sample losses
          pred_v / min_snr_gamma   eps_hat is the network output against the v target (pred_v) or the noise, weighted per level with
                            loss_weights and per sample with iw, from one vdx_v_loss pass; last_loss_per_sample = w_b * (the sample's
                            mean) and the loss is (1 / B) sum_b iw_b of them: what is optimised
          otherwise         the plain mean (vdx_loss_sum, vdx_loss_grad)"""
        if self.learned_variance:
            return self.hybrid_loss(x_start, noise, eps_hat, t32, want_grad=want_grad, _pre=_pre, iw=iw)
        B, fhw, l2 = x_start.shape[0], self._per_sample(x_start) // self.channels, int(self.loss_type == 'l2')
        if self.objective == 'pred_v' or self._loss_w is not None:
            if mask is not None:
                self._refuse('objective', frame_mask=True)
            scratch = torch.empty(L.vdx_v_loss_scratch_doubles(B), dtype=torch.float64, device=self.device)
            out = torch.empty(B + 1, dtype=torch.float64, device=self.device)
            d_out = torch.empty_like(eps_hat) if want_grad else None
            L.check(L.vdx_v_loss(L.ptr(eps_hat), L.ptr(x_start), L.ptr(noise), L.ptr(t32), L.ptr(self.sqrt_alphas_cumprod),
                                 L.ptr(self.sqrt_one_minus_alphas_cumprod), L.ptr(self._loss_w), L.ptr(iw), self.num_timesteps,
                                 int(self.objective == 'pred_v'), float(_pre[0]), float(_pre[1]), l2, L.ptr(d_out), L.ptr(scratch), L.ptr(out),
                                 B, self.channels, fhw, L.stream_ptr()))
            self.last_loss_per_sample = out[:B]
            return out[B].to(torch.float32).reshape(()), d_out
        if mask is None and iw is not None:
            out, d_eps = TS.loss_weighted(eps_hat, noise, iw, l2=bool(l2), want_grad=want_grad)
            self.last_loss_per_sample = out[:B]
            return out[B].to(torch.float32).reshape(()), d_eps
        d_eps = torch.empty_like(eps_hat) if want_grad else None
        if mask is not None:
            loss, acc = self.masked_loss(eps_hat, noise, mask)                # acc = device (sum, count | scratch)
            if want_grad:
                L.check(vdx_loss_grad_masked(L.ptr(eps_hat), L.ptr(noise), L.ptr(mask), acc.data_ptr() + 8, L.ptr(d_eps), B, self.channels,
                                             fhw, l2, L.stream_ptr()))
            return loss, d_eps
        acc = torch.zeros(1, dtype=torch.float64, device=self.device)
        L.check(vdx_loss_sum(L.ptr(eps_hat), L.ptr(noise), L.ptr(acc), B, self.channels, fhw, l2, L.stream_ptr()))
        if want_grad:
            L.check(vdx_loss_grad(L.ptr(eps_hat), L.ptr(noise), L.ptr(d_eps), B, self.channels, fhw, l2, L.stream_ptr()))
        return (acc / float(x_start.numel())).to(torch.float32).reshape(()), d_eps

    def masked_loss(self, eps_hat, noise, mk):
        """(loss, acc) of the masked objective: acc[0:2] = device doubles (sum, count) over the mask-0 elements (vdx_loss_sum_masked, the
        rest of acc is its scratch) and loss = sum / max(count, 1) as a float32 device scalar; the host reads nothing."""
        B = noise.shape[0]
        fhw = self._per_sample(noise) // self.channels
        acc = torch.empty(2 + vdx_loss_masked_scratch_doubles(), dtype=torch.float64, device=self.device)
        L.check(vdx_loss_sum_masked(L.ptr(eps_hat), L.ptr(noise), L.ptr(mk), acc.data_ptr() + 16, acc.data_ptr(), B, self.channels, fhw,
                                    int(self.loss_type == 'l2'), L.stream_ptr()))
        return (acc[0] / acc[1].clamp_min(1.0)).to(torch.float32).reshape(()), acc

    def __call__(self, x, key, *args, **kwargs):
        """reference :473-502: random t, normalize_img, p_losses (a frame_mask keyword goes there)."""
        b, c, f, h, w = x.shape
        assert (c, f, h, w) == (self.channels, self.num_frames, self.image_size, self.image_size), \
            f'expected [b, {self.channels}, {self.num_frames}, {self.image_size}, {self.image_size}], got {tuple(x.shape)}'
        _, t_key, loss_key = split_key(key, 3)
        g = torch.Generator().manual_seed(t_key & 0x7FFFFFFFFFFFFFFF)
        t = torch.randint(0, self.num_timesteps, (b,), generator=g, dtype=torch.int32)
        return self.p_losses(x, t, loss_key, *args, _pre=(2.0, -1.0), **kwargs)      # normalize_img folded into q_sample
