"""fp64 restatement of the learned-variance paths (Nichol & Dhariwal 2021, "Improved DDPM"; vdx.h: "Learned variances"), written from the
paper for tests/test_host_learned_variance.py and tests/test_gpu_learned_variance.py: the (respaced) tables, the interpolated
log-variance, the reverse step, the hybrid loss with eps_hat detached inside the variational term, and the bound's terms with the
model's variance.  Gradients come from autograd; closed_form_grads restates the formulas the kernel uses, and the host tests hold the two
(and central differences) together.  The shared pieces (the general normal_kl, the discretized decoder likelihood, x_t) are
tests/_vlb_ref.py's.  dt = torch.float32 evaluates the same expressions in fp32: the floor the GPU bounds are built on.  Nothing here needs
a GPU or libvdx.  A plain module: nothing here is collected."""
import functools
import math

import numpy as np
import torch

import _vlb_ref as V

F32, F64 = torch.float32, torch.float64
LN2 = math.log(2.0)
ROWS = dict(sqrt_ac=0, sqrt_1mac=1, sqrt_recip=2, sqrt_recipm1=3, coef1=4, coef2=5, max_log=6, min_log=7, ac=8)
STEP_ROWS = dict(sqrt_recip=0, sqrt_recipm1=1, coef1=2, coef2=3, max_log=4, min_log=5)


def ref_tables(timesteps, seq=None):
    """[9, S] float64 (ROWS) of the chain over the levels `seq` (None: all) of the project's beta schedule, from the definitions:
    alpha_bar' = alpha_bar[seq], beta' = 1 - alpha_bar'_i / alpha_bar'_{i-1}, the rest from those; min_log[0] = log beta~'_1."""
    from video_diffusion_nnx_amd.gaussian_diffusion import cosine_beta_schedule
    betas = torch.from_numpy(cosine_beta_schedule(int(timesteps)).astype(np.float64))
    ac_all = torch.cumprod(1.0 - betas, 0)
    idx = torch.arange(int(timesteps)) if seq is None else torch.as_tensor(np.asarray(list(seq)), dtype=torch.long)
    ac = ac_all[idx]
    ac_prev = torch.cat([torch.ones(1, dtype=F64), ac[:-1]])
    b = 1.0 - ac / ac_prev
    pv = b * (1.0 - ac_prev) / (1.0 - ac)
    min_log = torch.log(torch.cat([pv[1:2], pv[1:]])) if len(idx) > 1 else torch.log(b)
    return torch.stack([ac.sqrt(), (1.0 - ac).sqrt(), (1.0 / ac).sqrt(), (1.0 / ac - 1.0).sqrt(), b * ac_prev.sqrt() / (1.0 - ac),
                        (1.0 - ac_prev) * (1.0 - b).sqrt() / (1.0 - ac), torch.log(b), min_log, ac]).numpy()


def _col(tab, row, t, dt, rows=ROWS):
    return torch.from_numpy(np.asarray(tab[rows[row]], dtype=np.float64)).to(dt)[t.long()].reshape(-1, 1, 1, 1, 1)


def split(out2, C):
    """channel-last [B,F,H,W,2C] -> (eps_hat, v), each [B,C,F,H,W]."""
    o = out2.permute(0, 4, 1, 2, 3)
    return o[:, :C], o[:, C:]


def log_variance(v, max_log, min_log):
    f = (v + 1.0) / 2.0
    return f * max_log + (1.0 - f) * min_log


def step(x, eps_hat, v, z, lvl, step_tab, clip=True, dt=F64):
    """One reverse step at the levels lvl [B] of the [6, S] step table: mu + 1[lvl != 0] exp(0.5 log sigma^2) z."""
    c = lambda r: _col(step_tab, r, lvl, dt, STEP_ROWS)
    x, eps_hat, v, z = x.to(dt), eps_hat.to(dt), v.to(dt), z.to(dt)
    xh = c('sqrt_recip') * x - c('sqrt_recipm1') * eps_hat
    if clip:
        xh = xh.clamp(-1.0, 1.0)
    mean = c('coef1') * xh + c('coef2') * x
    sigma = torch.exp(0.5 * log_variance(v, c('max_log'), c('min_log')))
    return mean + (lvl != 0).to(dt).reshape(-1, 1, 1, 1, 1) * sigma * z


def xt_of(x0, eps, t, tab, dt=F64):
    """x_t with the coefficients the kernels use: the table's doubles rounded to fp32, widened again."""
    a = _col(tab, 'sqrt_ac', t, F32).to(dt)
    s = _col(tab, 'sqrt_1mac', t, F32).to(dt)
    return a * x0.to(dt) + s * eps.to(dt)


def vb_elements(x0, xt, eps_hat, v, t, tab, clip=False, dt=F64):
    """The variational term per element in bits [B,C,F,H,W]: KL(q(x_{t-1} | x_t, x0) || N(mu, sigma^2)) for t >= 1 by the general
    normal_kl, the discretized decoder for t = 0; x0_hat -- and so mu -- from eps_hat as given (the caller detaches)."""
    c = lambda r: _col(tab, r, t, dt)
    xh = c('sqrt_recip') * xt - c('sqrt_recipm1') * eps_hat
    if clip:
        xh = xh.clamp(-1.0, 1.0)
    mu_true, mu = c('coef1') * x0 + c('coef2') * xt, c('coef1') * xh + c('coef2') * xt
    lv = log_variance(v, c('max_log'), c('min_log'))
    kl = V.normal_kl(mu_true, c('min_log').expand_as(lv), mu, lv) / LN2           # min_log[t] = log beta~_t for t >= 1
    nll = -V.discretized_log_likelihood(x0.double(), mu.double(), lv.double()).to(dt) / LN2
    return torch.where((t == 0).reshape(-1, 1, 1, 1, 1), nll, kl), xh


def hybrid(x0, eps, out2, t, tab, l2=False, w=1.0, dt=F64):
    """The hybrid loss of out2 [B,F,H,W,2C] (a leaf that may require grad): dict(loss, mse, vb scalars; mse_b, vb_b [B]) with eps_hat
    detached inside vb."""
    C = x0.shape[1]
    o = out2.to(dt)
    eh, v = split(o, C)
    x0, e = x0.to(dt), eps.to(dt)
    xt = xt_of(x0, eps, t, tab, dt)
    d = eh - e
    mse_el = d * d if l2 else d.abs()
    vb_el, _ = vb_elements(x0, xt, eh.detach(), v, t, tab, False, dt)
    mean_b = lambda u: u.reshape(u.shape[0], -1).mean(1)
    mse, vb = mse_el.mean(), vb_el.mean()
    return dict(loss=mse + w * vb, mse=mse, vb=vb, mse_b=mean_b(mse_el), vb_b=mean_b(vb_el))


def hybrid_grad(x0, eps, out2, t, tab, l2=False, w=1.0):
    """(values, dL/d out2 [B,F,H,W,2C]) in fp64 through autograd."""
    o = out2.double().clone().requires_grad_(True)
    r = hybrid(x0, eps, o, t, tab, l2, w)
    g, = torch.autograd.grad(r['loss'], o)
    return {k: u.detach() for k, u in r.items()}, g


def closed_form_grads(x0, eps, out2, t, tab, l2=False, w=1.0):
    """dL/d out2 by the closed forms the kernel uses (fp64): the eps_hat half 2 d / N or sign(d) / N; the v half
    d vb / d log sigma^2 * 0.5 (max_log - min_log) * w / (N ln 2) with d KL / d log sigma^2 = 0.5 (1 - e^D - (mu~ - mu)^2 e^{-log sigma^2}),
    D = log beta~_t - log sigma^2, and at t = 0 0.5 (phi(z+) z+ - phi(z-) z-) / P without the absent term on a tail, 0 where P is floored."""
    C = x0.shape[1]
    o = out2.double()
    eh, v = split(o, C)
    x0, e = x0.double(), eps.double()
    n = float(x0.numel())
    c = lambda r: _col(tab, r, t, F64)
    xt = xt_of(x0, eps, t, tab)
    d = eh - e
    g_eps = (2.0 * d if l2 else torch.sign(d)) / n
    xh = c('sqrt_recip') * xt - c('sqrt_recipm1') * eh
    lv = log_variance(v, c('max_log'), c('min_log'))
    dmu = c('coef1') * (x0 - xh)
    delta = c('min_log') - lv
    d_kl = 0.5 * (1.0 - torch.exp(delta) - dmu * dmu * torch.exp(-lv))
    mu = c('coef1') * xh + c('coef2') * xt
    inv = torch.exp(-0.5 * lv)
    zp, zm = (x0 - mu + 1.0 / 255.0) * inv, (x0 - mu - 1.0 / 255.0) * inv
    pdf = lambda z: torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    lo, hi = x0 < -0.999, x0 > 0.999
    p = torch.where(lo, V.phi(zp), torch.where(hi, V.phi(-zm), torch.where(zm > 0, V.phi(-zm) - V.phi(-zp), V.phi(zp) - V.phi(zm))))
    num = torch.where(lo, pdf(zp) * zp, torch.where(hi, -pdf(zm) * zm, pdf(zp) * zp - pdf(zm) * zm))
    d_dec = torch.where(p > 1e-12, 0.5 * num / p.clamp_min(1e-300), torch.zeros_like(p))
    d_lv = torch.where((t == 0).reshape(-1, 1, 1, 1, 1), d_dec, d_kl)
    g_v = d_lv * 0.5 * (c('max_log') - c('min_log')) * (w / (n * LN2))
    return torch.cat([g_eps, g_v], 1).permute(0, 2, 3, 4, 1).contiguous()


def bound_terms(x, out2, eps, t, tab, clip=True, dt=F64):
    """calc_bpd's per-level terms with the model's variance: x [B,C,F,H,W] in [0, 1] -> (vb, mse, xstart_mse) [B] float64."""
    C = x.shape[1]
    eh, v = split(out2.to(dt), C)
    x0 = x.to(dt) * 2 - 1
    xt = xt_of(x0, eps, t, tab, dt)
    vb_el, xh = vb_elements(x0, xt, eh, v, t, tab, clip, dt)
    mean = lambda u: u.reshape(u.shape[0], -1).mean(1).to(F64)
    return mean(vb_el), mean((eh - eps.to(dt)) ** 2), mean((xh - x0) ** 2)


# ---- the kernel-level cases of tests/test_gpu_learned_variance.py ------------------------------------------------------------------------
T_CASE = 1000
EW_SWEEP = 2048 * 256 * 4                                                 # elements per sample one sweep of ew_blocks()'s capped grid covers
HYBRID_CASES = {
    'C1': (4, 1, (2, 16, 16)),                                            # per_sample 512
    'C3_ODD': (4, 3, (2, 5, 7)),                                          # fhw 70, per_sample 210: not a multiple of 4, quads straddle channels
    'WRAP': (4, 1, (1, 1, 2100004)),                                      # one sample past the step kernels' grid cap (tests/_step_cases.py WRAP)
}


@functools.lru_cache(None)
def tables(T=T_CASE):
    from video_diffusion_nnx_amd.gaussian_diffusion import make_lv_tables
    return make_lv_tables(T)


@functools.lru_cache(None)
def hybrid_case(name):
    """x0 in [-1, 1] with exact -1 and +1 (the decoder's tails); eps; out2 = (eps + 0.3 N(0, 1) | v), v uniform in [-1, 1] with -3, -1,
    1, 3 planted (extrapolation); t = (0, 1, T-1, random).  Computed once, left unchanged."""
    B, C, fhw = HYBRID_CASES[name]
    shape = (B, C) + fhw
    g = torch.Generator().manual_seed(5 + len(name))
    x0 = (torch.rand(shape, generator=g) * 2 - 1).to(torch.bfloat16).float()
    flat = x0.view(B, -1)
    flat[:, 0], flat[:, 1], flat[:, -1], flat[:, -2] = -1.0, 1.0, 1.0, -1.0
    eps = torch.randn(shape, generator=g)
    eh = eps + 0.3 * torch.randn(shape, generator=g)
    v = torch.rand(shape, generator=g) * 2 - 1
    vf = v.view(B, -1)
    for k, val in enumerate((-3.0, -1.0, 1.0, 3.0)):
        vf[:, k], vf[:, -1 - k] = val, val
    out2 = torch.cat([eh, v], 1).permute(0, 2, 3, 4, 1).contiguous()
    t = torch.tensor([0, 1, T_CASE - 1, int(torch.randint(2, T_CASE - 1, (), generator=g))], dtype=torch.int32)
    return dict(x0=x0, eps=eps, out2=out2, t=t, shape=shape)
