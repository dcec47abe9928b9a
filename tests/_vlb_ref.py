"""fp64 restatement of the variational bound's terms (Ho et al. 2020, eq. 5; Nichol & Dhariwal 2021, calc_bpd_loop), written from the
two papers for tests/test_host_vlb.py and tests/test_gpu_vlb.py: the GENERAL normal_kl between the true posterior and the model's, the
discretized Gaussian log-likelihood of the decoder, the prior KL.  dt = torch.float32 evaluates the same expressions in fp32: the floor
the GPU bounds are built on.  For the decoder (which the kernel evaluates in double) the fp32 switch rounds what the kernel receives as
fp32 (x0, x_t, x0_hat) and keeps the likelihood itself in double: the fp32-input rounding effect.  Nothing here needs a GPU or libvdx.
The table of doubles is the project's own (make_vlb_tables: the fp32 schedule values widened, w_t and the decoder's log-variance formed
from them); tests/test_host_vlb.py::test_make_vlb_tables holds it to the closed form.  A plain module: nothing here is collected."""
import functools
import math

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
LN2 = math.log(2.0)
ROWS = dict(sqrt_ac=0, sqrt_1mac=1, sqrt_recip=2, sqrt_recipm1=3, coef1=4, coef2=5, w=6, dec_logvar=7, ac=8)


def normal_kl(mean1, logvar1, mean2, logvar2):
    """KL(N(mean1, exp logvar1) || N(mean2, exp logvar2)) in nats, the general form."""
    return 0.5 * (-1.0 + logvar2 - logvar1 + torch.exp(logvar1 - logvar2) + (mean1 - mean2) ** 2 * torch.exp(-logvar2))


def phi(z):
    return 0.5 * torch.special.erfc(-z / math.sqrt(2.0))


def discretized_log_likelihood(x0, mean, logvar):
    """log of the N(mean, exp logvar) mass on the 8-bit bin of x0 (half-width 1/255), open-ended below -0.999 and above 0.999, floored
    at 1e-12; where both tails are small the difference is taken between the complements."""
    inv = torch.exp(-0.5 * logvar)
    zp, zm = (x0 - mean + 1.0 / 255.0) * inv, (x0 - mean - 1.0 / 255.0) * inv
    mid = torch.where(zm > 0, phi(-zm) - phi(-zp), phi(zp) - phi(zm))
    p = torch.where(x0 < -0.999, phi(zp), torch.where(x0 > 0.999, phi(-zm), mid))
    return torch.log(p.clamp_min(1e-12))


def _col(tab, row, t, dt):
    return torch.from_numpy(np.asarray(tab[ROWS[row]])).to(dt)[t.long()].reshape(-1, 1, 1, 1, 1)


def x_t(x, eps, t, tab, dt=F64):
    """sqrt_ac[t] (2 x - 1) + sqrt(1 - ac[t]) eps."""
    return _col(tab, 'sqrt_ac', t, dt) * (x.to(dt) * 2 - 1) + _col(tab, 'sqrt_1mac', t, dt) * eps.to(dt)


def terms(x, eps_hat, eps, t, tab, clip=True, dt=F64, dec_logvar0=None):
    """x [B,C,F,H,W] in [0, 1], eps_hat / eps [B,C,F,H,W] (channel-first), t [B] -> (vb, mse, xstart_mse), each [B] float64: the means
    over the elements of a sample, vb in bits.  dec_logvar0: another log-variance for the decoder than the table's log post_var_1."""
    x0 = x.to(dt) * 2 - 1
    e, eh = eps.to(dt), eps_hat.to(dt)
    xt = x_t(x, eps, t, tab, dt)
    xh = _col(tab, 'sqrt_recip', t, dt) * xt - _col(tab, 'sqrt_recipm1', t, dt) * eh
    if clip:
        xh = xh.clamp(-1.0, 1.0)
    c1, c2 = _col(tab, 'coef1', t, dt), _col(tab, 'coef2', t, dt)
    logvar = _col(tab, 'dec_logvar', t, dt)                                # log post_var_t for t >= 1
    kl = normal_kl(c1 * x0 + c2 * xt, logvar, c1 * xh + c2 * xt, logvar) / LN2
    d = F64                                                                # the decoder: double on (possibly fp32-rounded) inputs
    mu = _col(tab, 'coef1', t, d) * xh.to(d) + _col(tab, 'coef2', t, d) * xt.to(d)
    dec = _col(tab, 'dec_logvar', t, d) if dec_logvar0 is None else torch.full((), float(dec_logvar0), dtype=d)
    nll = -discretized_log_likelihood(x0.to(d), mu, dec) / LN2
    mean = lambda v: v.reshape(v.shape[0], -1).mean(1).to(F64)
    vb = torch.where(t == 0, mean(nll), mean(kl))
    return vb, mean((eh - e) ** 2), mean((xh - x0) ** 2)


def prior(x, tab, dt=F64):
    """KL(q(x_{T-1} | x0) || N(0, 1)) per sample in bits/dim, by the general normal_kl."""
    x0 = x.to(dt) * 2 - 1
    ac = torch.tensor(float(tab[ROWS['ac']][-1]), dtype=dt)
    zero = torch.zeros((), dtype=dt)
    kl = normal_kl(ac.sqrt() * x0, torch.log(1 - ac), zero, zero) / LN2
    return kl.reshape(kl.shape[0], -1).mean(1).to(F64)


def rel(a, b):
    """|a - b| / |b| per entry, float64 (0 where both are 0)."""
    a, b = a.double(), b.double()
    return torch.where(b == 0, (a - b).abs(), (a - b).abs() / b.abs().clamp_min(1e-300))


# ---- the kernel-level cases of tests/test_gpu_vlb.py, and their bounds (tests/test_host_vlb.py proves the bounds can tell) --------------
T_CASE = 1000
VLB_BLOCKS, THREADS = 64, 256                                             # kVlbBlocks (csrc/diffusion.hip), workgroup size
SWEEP = VLB_BLOCKS * THREADS * 4                                          # floats per sample one sweep of the fixed grid covers: 65 536
CASES = {
    'STRADDLE': ((3, 4, 1, 3, 3), (0, 1, T_CASE - 1)),                    # per_sample 36, fhw odd: quads straddle channels, most of the grid idle
    'C3': ((2, 3, 2, 4, 4), (0, T_CASE // 2)),                            # the channel-last transposition at C = 3
    'WRAP': ((2, 4, 1, 1, (SWEEP + 4) // 4), (0, T_CASE - 1)),            # per_sample 65 540: one quad in the second sweep; fhw odd
}


@functools.lru_cache(None)
def tables(T=T_CASE):
    from video_diffusion_nnx_amd.gaussian_diffusion import make_vlb_tables
    return make_vlb_tables(T)


@functools.lru_cache(None)
def case(name):
    """x in [0, 1] with exact 0.0 and 1.0 and bf16-representable interior values; eps; eps_hat = eps + 0.3 N(0, 1), channel-last (so
    x0_hat leaves [-1, 1] at the high levels and stays inside at the low ones); t.  Computed once, left unchanged."""
    shape, t = CASES[name]
    B, C, Fr, H, W = shape
    g = torch.Generator().manual_seed(11 + len(name))
    x = torch.rand(shape, generator=g).to(torch.bfloat16).float()
    flat = x.view(B, -1)
    flat[:, 0], flat[:, 1], flat[:, -1], flat[:, -2] = 0.0, 1.0, 1.0, 0.0
    eps = torch.randn(shape, generator=g)
    eps_hat = (eps + 0.3 * torch.randn(shape, generator=g)).permute(0, 2, 3, 4, 1).contiguous()      # [B,F,H,W,C]
    return dict(x=x, eps=eps, eps_hat=eps_hat, t=torch.tensor(t, dtype=torch.int32), shape=shape)


def cf(eps_hat):
    """channel-last [B,F,H,W,C] -> [B,C,F,H,W]."""
    return eps_hat.permute(0, 4, 1, 2, 3)


@functools.lru_cache(None)
def case_ref(name, clip, dt=F64):
    c = case(name)
    return terms(c['x'], cf(c['eps_hat']), c['eps'], c['t'], tables(), clip, dt)


def term_bounds(ref32, ref64, t):
    """Per-sample absolute bounds [3][B] for (vb, mse, xstart_mse): 8 x the error of the fp32 evaluation against fp64 on the same case.
    Relative for the KL terms and the two MSEs (the worst sample's relative error x each sample's own value); for the vb of a t = 0
    sample, the decoder term, absolute: 8 x the worst t = 0 sample's fp32-input rounding effect."""
    out = []
    for k in range(3):
        r32, r64 = ref32[k].double(), ref64[k].double()
        kl = (t > 0) if k == 0 else torch.ones_like(t, dtype=torch.bool)
        b = torch.zeros_like(r64)
        if kl.any():
            b = torch.where(kl, 8.0 * rel(r32, r64)[kl].max() * r64.abs(), b)
        if (~kl).any():
            b = torch.where(~kl, 8.0 * (r32 - r64).abs()[~kl].max(), b)
        out.append(b)
    return torch.stack(out)
