"""fp64 restatement of the DPM-Solver++(2M) sampler (Lu et al. 2022, data-prediction multistep form), written from the contract in
include/vdx.h: the step, the unmasked loop and the masked loop.  EXTENSION, PARITY UNPINNED: the reference has no such sampler, so
tests/test_host_dpm.py pins this restatement itself against the exact solution of the probability-flow ODE for Gaussian data.  A plain
module: nothing here is collected."""
import numpy as np
import torch

from oracle import philox_ref, unet3d_ref as R  # noqa: F401  (R: the UNet oracle, for the tests that import it from here)

DRAW_KNOWN = 1 << 62


def time_sequence(T, S):
    """ddim_time_sequence restated: S + 1 times, T-1 first, -1 (= the data) last."""
    return np.linspace(-1, T - 1, S + 1).astype(np.int64)[::-1]


def lam(a):
    return 0.5 * torch.log(a / (1 - a))


def extrapolation_weight(ac, seq, k):
    """c of step k >= 1 with seq[k+1] >= 0."""
    ls, ln, lp = lam(ac[int(seq[k])]), lam(ac[int(seq[k + 1])]), lam(ac[int(seq[k - 1])])
    return ((ln - ls) / (2 * (ls - lp))).item()


def dpm_step(x, eps, hist, ac, seq, k, order=2, clip=True, thres=None):
    """One step: x [B,C,F,H,W], eps channel-first like x, hist = the previous step's x0 (unused at k == 0 or order 1), ac = the fp64
    image of the fp32 alphas_cumprod table, thres [B] or None (static +-1).  Returns (out, x0); x0 is the next hist."""
    s, n = int(seq[k]), int(seq[k + 1])
    a_s = ac[s]
    x0 = (x - (1 - a_s).sqrt() * eps) / a_s.sqrt()
    if clip:
        th = torch.ones(x.shape[0], dtype=x.dtype) if thres is None else thres.to(x.dtype)
        th = th.reshape(-1, 1, 1, 1, 1)
        x0 = torch.maximum(torch.minimum(x0, th), -th) / th
    if n < 0:
        return x0, x0
    a_n = ac[n]
    h = lam(a_n) - lam(a_s)
    d = x0
    if k > 0 and order == 2:
        c = h / (2 * (lam(a_s) - lam(ac[int(seq[k - 1])])))
        d = (1 + c) * x0 - c * hist
    out = ((1 - a_n) / (1 - a_s)).sqrt() * x - a_n.sqrt() * torch.expm1(-h) * d
    return out, x0


def _threshold(ref, x, eps, t):
    """The dynamic threshold of the captured step: the quantile of |x0_hat| with x0_hat from the sqrt_recip tables (as the kernel)."""
    if not ref.use_dynamic_thres:
        return None
    x0 = ref.predict_start_from_noise(x, torch.full((x.shape[0],), t), eps)
    return torch.quantile(x0.abs().reshape(x.shape[0], -1), ref.dynamic_thres_percentile, dim=-1).clamp_min(1.0)


def dpm_loop(ref, x_T, S, order=2, clip=True, steps=None):
    """The unmasked chain around ref.denoise (a DiffusionRef in fp64); returns x_0 in [-1, 1].  steps: stop after that many."""
    seq = time_sequence(ref.num_timesteps, S)
    ac = ref.tab['alphas_cumprod']
    x, hist = x_T.to(ac.dtype), None
    for k in range(S if steps is None else steps):
        t = int(seq[k])
        eps = ref.denoise(x, torch.full((x.shape[0],), t)).permute(0, 4, 1, 2, 3)
        x, hist = dpm_step(x, eps, hist, ac, seq, k, order, clip, _threshold(ref, x, eps, t) if clip else None)
    return x


def dpm_loop_masked(ref, video, m, seed, S, order=2):
    """The masked chain (inpaint(dpm_steps=S)): x_T = Philox(seed, 0), init merge at seq[0], then per step the dpm step and the merge of
    the known region noised to the next level with draw DRAW_KNOWN + k.  Returns the video in [0, 1]."""
    shape = tuple(video.shape)

    def z(draw):
        return torch.from_numpy(philox_ref.randn(int(np.prod(shape)), seed, draw)).double().reshape(shape)

    seq = time_sequence(ref.num_timesteps, S)
    ac = ref.tab['alphas_cumprod']
    kn0, m = 2 * video.double() - 1, m.bool()
    x = z(0)
    x = torch.where(m, ac[int(seq[0])].sqrt() * kn0 + (1 - ac[int(seq[0])]).sqrt() * x, x)
    hist = None
    for k in range(S):
        t, tn = int(seq[k]), int(seq[k + 1])
        eps = ref.denoise(x, torch.full((shape[0],), t)).permute(0, 4, 1, 2, 3)
        xp, hist = dpm_step(x, eps, hist, ac, seq, k, order, True, _threshold(ref, x, eps, t))
        kn = kn0 if tn < 0 else ac[tn].sqrt() * kn0 + (1 - ac[tn]).sqrt() * z(DRAW_KNOWN + k)
        x = torch.where(m, kn, xp)
    return (x + 1) / 2


# ---- the analytic check: data ~ N(0, var I), whose optimal denoiser and probability-flow ODE solution are closed forms ----

def gaussian_eps(x, a, var=0.25):
    """The optimal eps prediction at alpha_bar = a for N(0, var I) data: x0_hat = E[x0 | x] = alpha var / (alpha^2 var + sigma^2) x."""
    x0 = a.sqrt() * var / (a * var + (1 - a)) * x
    return (x - a.sqrt() * x0) / (1 - a).sqrt()


def gaussian_exact(x_T, a_T, var=0.25):
    """The ODE solution at the data end: the marginal std goes from sqrt(a_T var + 1 - a_T) to sqrt(var), x scales with it."""
    return x_T * (var / (a_T * var + (1 - a_T))).sqrt()


def gaussian_chain(ac, x_T, S, order, step=dpm_step, var=0.25):
    """An S-step chain over ac with the analytic denoiser, no clipping; `step` has dpm_step's signature.  Returns x_0."""
    seq = time_sequence(ac.shape[0], S)
    x, hist = x_T, None
    for k in range(S):
        x, hist = step(x, gaussian_eps(x, ac[int(seq[k])], var), hist, ac, seq, k, order, False)
    return x


def rel_err(x, exact):
    return ((x - exact).norm() / exact.norm()).item()
