"""Loss-aware timestep sampling, resident on the device (extension: Nichol & Dhariwal 2021, "Improved DDPM", section 3.3; improved-diffusion's
LossSecondMomentResampler.  vdx.h: "Loss-aware timestep sampling"; the fp64 restatement is tests/_tsampler_ref.py).

t is drawn with probability p_t ~ sqrt(E[l_t^2]), estimated from the last `history_per_term` losses seen at each level, mixed with
`uniform_prob` of the uniform distribution; every sample's loss is weighted by 1 / (T p_t), so the objective stays the uniform one in
expectation.  Until every level has a full history the draw is uniform and every weight exactly 1.  The history, the probabilities, the
draw and the weights live in device memory: draw() and update() only enqueue launches on the current stream."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L

_vp, _u64 = C.c_void_p, C.c_uint64
vdx_tsampler_draw = L._sig('vdx_tsampler_draw', C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_double, _vp, _u64, _u64, _vp, _vp, _vp, C.c_int, _vp])
vdx_tsampler_update = L._sig('vdx_tsampler_update', C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp])
vdx_loss_weighted_scratch_doubles = L._sig('vdx_loss_weighted_scratch_doubles', C.c_size_t, [C.c_int])
vdx_loss_weighted = L._sig('vdx_loss_weighted', C.c_int, [_vp] * 6 + [C.c_int, C.c_int, C.c_long, C.c_int, _vp])

MAX_TIMESTEPS = 4096                     # the LDS budget of vdx_tsampler_draw's one workgroup
MAX_HISTORY = 32
SAMPLERS = ('uniform', 'loss-second-moment')


def validate(timesteps: int, history_per_term: int, uniform_prob: float) -> None:
    """The rules of vdx_tsampler_draw, as ValueErrors."""
    if not 1 <= int(timesteps) <= MAX_TIMESTEPS:
        raise ValueError(f'the loss-second-moment sampler serves 1 <= timesteps <= {MAX_TIMESTEPS}, got {timesteps}')
    if not 1 <= int(history_per_term) <= MAX_HISTORY:
        raise ValueError(f'sampler_history must be in [1, {MAX_HISTORY}], got {history_per_term}')
    if not 0.0 < float(uniform_prob) <= 1.0:
        raise ValueError(f'sampler_uniform_prob must be in (0, 1], got {uniform_prob}')


class LossSecondMomentSampler:
    def __init__(self, timesteps: int, history_per_term: int = 10, uniform_prob: float = 0.001, device='cuda'):
        validate(timesteps, history_per_term, uniform_prob)
        self.timesteps, self.history_per_term, self.uniform_prob = int(timesteps), int(history_per_term), float(uniform_prob)
        self.device = torch.device(device)
        self.hist = torch.zeros(self.timesteps, self.history_per_term, dtype=torch.float64, device=self.device)
        self.count = torch.zeros(self.timesteps, dtype=torch.int32, device=self.device)

    def draw(self, batch: int, key: int, draw: int = 0, t=None):
        """(t int32 [batch], iw float64 [batch]) on the device: sample b from Philox(key, draw) at counter b.  With `t` (int32 [batch] on
        the device) nothing is drawn: only the weights of the given levels under the current probabilities."""
        t_out = torch.empty(int(batch), dtype=torch.int32, device=self.device)
        iw = torch.empty(int(batch), dtype=torch.float64, device=self.device)
        if t is not None:
            t = torch.as_tensor(t).to(self.device, torch.int32).contiguous()
            assert t.shape == (int(batch),), f't must be [{batch}], got {tuple(t.shape)}'
        L.check(vdx_tsampler_draw(L.ptr(self.hist), L.ptr(self.count), self.timesteps, self.history_per_term, self.uniform_prob, L.ptr(t),
                                  int(key) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFFFFFFFFFF, L.ptr(t_out), L.ptr(iw), 0, int(batch),
                                  L.stream_ptr()))
        return t_out, iw

    def update(self, entries) -> None:
        """entries float64 [n, 2] = (t, loss) on the device, applied in index order (non-finite and out-of-range entries are skipped)."""
        e = torch.as_tensor(entries).to(self.device, torch.float64).contiguous()
        assert e.dim() == 2 and e.shape[1] == 2, f'entries must be [n, 2], got {tuple(e.shape)}'
        L.check(vdx_tsampler_update(L.ptr(self.hist), L.ptr(self.count), self.timesteps, self.history_per_term, L.ptr(e), e.shape[0],
                                    L.stream_ptr()))

    def probabilities(self) -> torch.Tensor:
        """p float64 [timesteps] on the device, as the next draw would use it."""
        p = torch.empty(self.timesteps, dtype=torch.float64, device=self.device)
        t_out = torch.empty(1, dtype=torch.int32, device=self.device)
        iw = torch.empty(1, dtype=torch.float64, device=self.device)
        L.check(vdx_tsampler_draw(L.ptr(self.hist), L.ptr(self.count), self.timesteps, self.history_per_term, self.uniform_prob, 0, 0, 0,
                                  L.ptr(t_out), L.ptr(iw), L.ptr(p), 1, L.stream_ptr()))
        return p

    def state(self):
        """Copies of (hist float64 [T, H], count int32 [T]), on the device."""
        return self.hist.clone(), self.count.clone()

    def load_state(self, hist, count) -> None:
        hist, count = torch.as_tensor(hist), torch.as_tensor(count)
        if tuple(hist.shape) != tuple(self.hist.shape) or tuple(count.shape) != tuple(self.count.shape):
            raise ValueError(f'state must be hist {tuple(self.hist.shape)} and count {tuple(self.count.shape)}, got {tuple(hist.shape)} and '
                             f'{tuple(count.shape)}')
        self.hist.copy_(hist.to(torch.float64))
        self.count.copy_(count.to(torch.int32))

    @property
    def warm(self) -> bool:
        """Every level has a full history (a host read of a device-side fact: the step itself never asks)."""
        return bool((self.count >= self.history_per_term).all().item())


def loss_weighted(eps_hat, noise, iw=None, *, l2: bool = False, want_grad: bool = True):
    """(out float64 [B + 1] = per-sample mean losses then (1 / B) sum_b iw_b l_b, d_eps float32 like eps_hat or None) of eps_hat
    [B,F,H,W,C] (channel-last) against noise [B,C,F,H,W] in one pass (vdx_loss_weighted); iw float64 [B] or None (all 1)."""
    assert eps_hat.dtype == torch.float32 and noise.dtype == torch.float32 and noise.dim() == 5
    B, Cc = noise.shape[0], noise.shape[1]
    fhw = noise.numel() // (B * Cc)
    scratch = torch.empty(vdx_loss_weighted_scratch_doubles(B), dtype=torch.float64, device=noise.device)
    out = torch.empty(B + 1, dtype=torch.float64, device=noise.device)
    d_eps = torch.empty_like(eps_hat) if want_grad else None
    L.check(vdx_loss_weighted(L.ptr(eps_hat), L.ptr(noise), L.ptr(iw), L.ptr(d_eps), L.ptr(scratch), L.ptr(out), B, Cc, fhw, int(bool(l2)),
                              L.stream_ptr()))
    return out, d_eps
