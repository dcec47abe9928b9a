"""Inputs, fp64 references and bounds of tests/test_gpu_step_kernels.py and tests/test_host_step_kernels.py: the kernels around the UNet
(csrc/diffusion.hip, csrc/optim.hip) at the sizes where their grid-stride loops wrap, where a float4 quad straddles two channels and
where sample bases leave their 16-byte boundary.  The references are the project's own restatements (oracle/diffusion_ref.py,
oracle/philox_ref.py, oracle/train_ref.py, tests/_dpm_ref.py, tests/_framecond_ref.py) composed here, not restated.  Nothing in this
module needs a GPU or libvdx.  A plain module: nothing here is collected."""
import functools
from collections import namedtuple

import numpy as np
import torch

import _dpm_ref as D
import _framecond_ref as FR
from oracle import philox_ref, train_ref as TR
from oracle.diffusion_ref import DiffusionRef, schedule

F32, F64 = torch.float32, torch.float64
DRAW_KNOWN, DRAW_RENOISE = 1 << 62, 1 << 63

# ---- shapes: external tensors [B, C, 1, 1, fhw], eps_hat channel-last [B, 1, 1, fhw, C] ----
Shape = namedtuple('Shape', 'name B C fhw')
WRAP = Shape('WRAP', 2, 4, 525001)           # per_sample 2 100 004: 713 quads per sample in the second sweep of a 2048 x 256 grid; fhw odd
STRADDLE = Shape('STRADDLE', 3, 4, 35)       # per_sample 140 = 35 quads, fhw odd: quads 8, 17 and 26 of every sample hold two channels
RAGGED = Shape('RAGGED', 3, 3, 35)           # per_sample 105: sample bases at 4-byte offsets; only the one-element kernels accept it
OLD = Shape('OLD', 3, 3, 128)                # the (3, 3, 2, 8, 8) of the earlier step tests: fhw % 4 == 0 (host proofs only)
SHAPES = {s.name: s for s in (WRAP, STRADDLE, RAGGED, OLD)}

EW_BLOCKS, ADAM_BLOCKS, THREADS = 2048, 4096, 256        # ew_blocks() / launch_adam_ema grid caps, workgroup size
SWEEP4 = EW_BLOCKS * THREADS * 4                         # floats per sample one sweep of a float4 kernel covers: 2 097 152
ADAM_SWEEP = ADAM_BLOCKS * THREADS * 4                   # 4 194 304
N_ADAM, N_ACC, N_RANDN, N_AFFINE = 4197107, 2100003, 2100003, 600001
INVALID = -1                                             # VDX_ERR_INVALID

T_P = 1000                                   # p_sample / p_sample_masked: sqrt_recip_ac[999] ~ 157
T_Q = 10                                     # q_sample, the losses (as their small tests)
T_D, S_DDIM, S_DPM = 1000, 100, 20           # ddim (100 steps) and dpm (20 steps) over T = 1000, as their small tests
DDIM_KS, DPM_KS = (0, 57, 99), (0, 1, 11, 19)
T_DYN = 12

# bounds the project states for these kernels at their small shapes (tests/test_gpu_diffusion.py, test_gpu_inpaint.py, test_gpu_dpm.py)
Q_TOL, RANDN_ATOL, RANDN_RTOL = 1e-6, 3e-6, 1e-5
P_TOL_NOISE, P_TOL_PHILOX, P_TOL_MASKED, P_TOL_T0 = 2e-5, 3e-5, 5e-5, 1e-5
STEP_TOL = 2e-5                              # ddim / dpm: x max(1, |ref|max)
LOSS_TOL, LOSS_MASKED_RTOL = 1e-5, 2e-5
DYN_RTOL = DYN_ATOL = 1e-6
FP32_ULP, U24 = 2.0 ** -23, 2.0 ** -24


def per(sh):
    return sh.C * sh.fhw


def dims(sh):
    return (sh.B, sh.C, 1, 1, sh.fhw)


def eps_dims(sh):
    return (sh.B, 1, 1, sh.fhw, sh.C)


def cf(eps):
    """channel-last [B,F,H,W,C] -> [B,C,F,H,W], as the reference's rearrange."""
    return eps.permute(0, 4, 1, 2, 3)


def t_vec(sh, T):
    """t = 0, mid, T-1 per sample; the two samples of WRAP take the two ends."""
    return torch.tensor([0, T // 2, T - 1] if sh.B == 3 else [0, T - 1])


def thres_vec(sh):
    return torch.tensor([1.0, 1.7, 3.2][:sh.B])


@functools.lru_cache(None)
def step_inputs(name, seed, xscale):
    """x, eps (channel-last), z, hist, known of one shape; (seed 5, scale 2) is the draw of the p_sample tests, (3, 1) that of ddim / dpm."""
    sh = SHAPES[name]
    g = torch.Generator().manual_seed(seed)
    x = xscale * torch.randn(dims(sh), generator=g)
    eps = torch.randn(eps_dims(sh), generator=g)
    z = torch.randn(dims(sh), generator=g)
    hist = torch.randn(dims(sh), generator=g).clamp(-1, 1)
    known = 2 * torch.rand(dims(sh), generator=g) - 1
    return dict(x=x, eps=eps, z=z, hist=hist, known=known)


@functools.lru_cache(None)
def mask(name, kind):
    """uint8 [B,C,1,1,fhw].  'p04': elements with probability 0.4.  'chan': whole channels (two per sample, another pair in each), so
    that with an odd fhw the mask changes inside a quad.  'lanes': quad q of a sample carries lane pattern q % 16, so every single-lane
    pattern (and every other one) occurs.  'zero', 'one': the limits."""
    sh = SHAPES[name]
    if kind == 'zero':
        return torch.zeros(dims(sh), dtype=torch.uint8)
    if kind == 'one':
        return torch.ones(dims(sh), dtype=torch.uint8)
    if kind == 'p04':
        g = torch.Generator().manual_seed(41)
        return (torch.rand(dims(sh), generator=g) < 0.4).to(torch.uint8)
    if kind == 'chan':
        m = torch.zeros(dims(sh), dtype=torch.uint8)
        for b in range(sh.B):
            m[b, b % sh.C] = 1
            m[b, (b + 2) % sh.C] = 1
        return m
    if kind == 'lanes':
        e = torch.arange(per(sh))
        bits = ((e // 4) % 16 >> (e % 4)) & 1
        return bits.to(torch.uint8).reshape(1, *dims(sh)[1:]).expand(*dims(sh)).contiguous()
    raise KeyError(kind)


@functools.lru_cache(None)
def z_philox(sh, seed, draw):
    """The restated Philox draw over the whole tensor, float32 (widen it for the fp64 reference); computed once, left unchanged."""
    return torch.from_numpy(philox_ref.randn(sh.B * per(sh), seed, draw)).reshape(dims(sh))


@functools.lru_cache(None)
def diffusion_ref(T, dt):
    return DiffusionRef(None, image_size=1, num_frames=1, channels=1, timesteps=T, dtype=dt)


def device_tables(T):
    """The arrays the sampling kernels take, from the oracle's float32 schedule: ptab [5][T], mtab [4][T], alphas_cumprod [T]."""
    s = schedule(T, np.float32)
    ptab = np.stack([s['sqrt_recip_alphas_cumprod'], s['sqrt_recipm1_alphas_cumprod'], s['posterior_mean_coef1'], s['posterior_mean_coef2'],
                     s['posterior_log_variance_clipped']]).astype(np.float32)
    mtab = np.stack([s['sqrt_alphas_cumprod'], s['sqrt_one_minus_alphas_cumprod'], np.sqrt(np.float32(1) - s['betas']),
                     np.sqrt(s['betas'])]).astype(np.float32)
    return dict(ptab=torch.from_numpy(ptab), mtab=torch.from_numpy(mtab), ac=torch.from_numpy(s['alphas_cumprod'].copy()),
                sqrt_ac=torch.from_numpy(s['sqrt_alphas_cumprod'].copy()), sqrt_1mac=torch.from_numpy(s['sqrt_one_minus_alphas_cumprod'].copy()))


def time_sequence(T, S):
    return np.ascontiguousarray(D.time_sequence(T, S).astype(np.int32))


# ---- comparison -----------------------------------------------------------------------------------------------------------------------

def _per_sample_max(t):
    return t.abs().reshape(t.shape[0], -1).amax(1)


def check(got, ref64, bound, what):
    """No NaN left in the output and max |got - ref| < bound; prints the figure next to the bound and returns it.  bound: one number, or
    a tensor [B] of per-sample bounds (scaled(), floor_bound()), each held against the worst element of its own sample."""
    got = got.detach().cpu()
    nan = int(torch.isnan(got).sum())
    assert nan == 0, f'{what}: {nan} elements were never written (NaN sentinel left)'
    if torch.is_tensor(bound):
        err = _per_sample_max(got.double() - ref64)
        worst = int((err / bound).argmax())
        print(f'[{what}] max-abs error per sample {[f"{e:.3e}" for e in err.tolist()]}  bounds {[f"{b:.3e}" for b in bound.tolist()]}  '
              f'worst error / bound {(err[worst] / bound[worst]).item():.4f} (sample {worst})')
        assert bool((err < bound).all()), (what, err.tolist(), bound.tolist())
        return err.max().item()
    err = (got.double() - ref64).abs().max().item()
    print(f'[{what}] max-abs error {err:.3e}  bound {bound:.3e}')
    assert err < bound, (what, err, bound)
    return err


def scaled(tol, ref64):
    """tol x max(1, |ref|max), the form of the DDIM step test's bound, with |ref|max taken per SAMPLE ([B]): one sample at t = T - 1 with
    the clip off reaches hundreds and must not loosen the bound of the samples of size 5 beside it."""
    return tol * _per_sample_max(ref64).clamp_min(1.0)


def floor_bound(base, ref32, ref64):
    """The bound of the T = 1000 ancestral steps, relative to max(1, |ref|max) of each sample: the larger of the figure the T = 10 test
    states (`base`) and 8 x the error of the same expression evaluated in fp32 on the CPU against fp64 on the same inputs (the worst
    sample's, each relative to its own scale).  Returns (absolute bounds [B], relative bound, CPU floor)."""
    scale = _per_sample_max(ref64).clamp_min(1.0)
    floor = (_per_sample_max(ref32.double() - ref64) / scale).max().item()
    rel = max(base, 8.0 * floor)
    return rel * scale, rel, floor


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-300)).item()


def small_bound(ref32, ref64):
    """tests/test_gpu_backward_forms.py _small_bound: 4 x the rel-L2 floor of the fp32 CPU evaluation, not below one fp32 ulp."""
    return 4.0 * max(rel_l2(ref32, ref64), FP32_ULP)


def clip_bound(ref32, ref64):
    """tests/test_gpu_grad_controls.py test_adam_clip_kernel_matches_fp64_restatement: 8 x the rel-L2 floor of the fp32 CPU evaluation."""
    return 8.0 * rel_l2(ref32, ref64)


# ---- references: composed from DiffusionRef, _dpm_ref and _framecond_ref ----------------------------------------------------------------

def _clip(x0, clip, thres):
    if not clip:
        return x0
    s = torch.ones(x0.shape[0], dtype=x0.dtype) if thres is None else thres.to(x0.dtype)
    s = s.reshape(-1, 1, 1, 1, 1)
    return torch.maximum(torch.minimum(x0, s), -s) / s


def p_sample_ref(x, eps, z, t, clip, thres, dt, T=T_P):
    """DiffusionRef.p_sample with a given per-sample threshold: (x_{t-1}, posterior mean), in dtype dt."""
    ref = diffusion_ref(T, dt)
    x, e, z = x.to(dt), cf(eps).to(dt), z.to(dt)
    x0 = _clip(ref.predict_start_from_noise(x, t, e), clip, thres)
    mean, _, logvar = ref.q_posterior(x0, x, t)
    nonzero = (1.0 - (t == 0).to(dt)).reshape(-1, 1, 1, 1, 1)
    return mean + nonzero * torch.exp(0.5 * logvar) * z, mean


def p_sample_masked_ref(sh, x, eps, known, m, t, clip, thres, seed, s, U, dt, T=T_P):
    """vdx_p_sample_step_masked's contract: the ancestral step with draw 1 + s, the known region noised to t - 1 with draw
    DRAW_KNOWN + s, and the re-noise with draw DRAW_RENOISE + s when s % U != U - 1."""
    ref = diffusion_ref(T, dt)
    xp, _ = p_sample_ref(x, eps, z_philox(sh, seed, 1 + s), t, clip, thres, dt, T)
    k = known.to(dt)
    kn = torch.where((t > 0).reshape(-1, 1, 1, 1, 1), ref.q_sample(k, (t - 1).clamp_min(0), z_philox(sh, seed, DRAW_KNOWN + s).to(dt)), k)
    out = torch.where(m.bool(), kn, xp)
    if s % U != U - 1:
        beta = ref.tab['betas'][t].reshape(-1, 1, 1, 1, 1)
        out = (1 - beta).sqrt() * out + beta.sqrt() * z_philox(sh, seed, DRAW_RENOISE + s).to(dt)
    return out


def ddim_ref(x, eps, ac, seq, k, clip, thres):
    """The eta = 0 step of DiffusionRef.ddim_sample_loop for one (t, t_next) pair with a given threshold: (out, x0), fp64."""
    t, tn = int(seq[k]), int(seq[k + 1])
    x, e, ac = x.double(), cf(eps).double(), ac.double()
    a_t = ac[t]
    a_n = ac[tn] if tn >= 0 else torch.ones((), dtype=F64)
    x0 = _clip((x - (1 - a_t).sqrt() * e) / a_t.sqrt(), clip, thres)
    return a_n.sqrt() * x0 + (1 - a_n).sqrt() * (x - a_t.sqrt() * x0) / (1 - a_t).sqrt(), x0


def dpm_ref(x, eps, hist, ac, seq, k, order, clip, thres):
    return D.dpm_step(x.double(), cf(eps).double(), hist.double(), ac.double(), seq, k, order, clip, None if thres is None else thres.double())


def known_merge(sh, out, known, m, ac, seq, k, seed):
    """The merge of vdx_ddim_step_masked / vdx_dpm_step_masked: the known region at the next level, draw DRAW_KNOWN + k."""
    tn = int(seq[k + 1])
    kn = known.double()
    if tn >= 0:
        a_n = ac.double()[tn]
        kn = a_n.sqrt() * kn + (1 - a_n).sqrt() * z_philox(sh, seed, DRAW_KNOWN + k).double()
    return torch.where(m.bool(), kn, out)


def q_sample_ref(x, noise, t, m=None, T=T_Q):
    """q_sample on the normalised clip 2 x - 1 (the _pre of __call__), masked by FR.q_sample_masked when m is given; fp64."""
    ref = diffusion_ref(T, F64)
    x0n = x.double() * 2 - 1
    return ref.q_sample(x0n, t, noise.double()) if m is None else FR.q_sample_masked(ref, x0n, t, noise.double(), m.bool())


@functools.lru_cache(None)
def loss_inputs(name):
    """eps_hat channel-last and noise, with a tenth of the elements exact ties (test_loss_grad: the l1 gradient there is 0)."""
    sh = SHAPES[name]
    g = torch.Generator().manual_seed(sh.B + sh.C)
    noise = torch.randn(dims(sh), generator=g)
    eps = torch.randn(eps_dims(sh), generator=g)
    tie = torch.rand(eps_dims(sh), generator=g) < 0.1
    eps = torch.where(tie, noise.permute(0, 2, 3, 4, 1), eps).contiguous()
    return dict(eps=eps, noise=noise, tie=tie)


def loss_mean_ref(eps, noise, l2):
    d = cf(eps).double() - noise.double()
    return ((d * d).mean() if l2 else d.abs().mean()).item()


def loss_grad_ref(eps, noise, l2, dt):
    """Autograd of the oracle's mean loss, as test_loss_grad; channel-last."""
    e = eps.to(dt).requires_grad_(True)
    d = cf(e) - noise.to(dt)
    loss = (d * d).mean() if l2 else d.abs().mean()
    return torch.autograd.grad(loss, e)[0]


def loss_grad_masked_ref(eps, noise, m, l2):
    """(FR.loss_grad channel-first fp64, the bound of test_loss_grad_masked_kernel).  l1: sign(e - n) is exact in fp32, the only error is
    the rounding of 1 / count.  l2: one rounding of e - n, the exact doubling, then 1 / count and the product, one rounding each."""
    e, n, mb = cf(eps).double(), noise.double(), m.bool()
    exp = FR.loss_grad(e, n, mb, l2)
    cnt = max(int((~mb).sum()), 1)
    bound = U24 / cnt * 1.01 if not l2 else (2 * U24 * (e.abs() + n.abs()).max().item() + 3 * U24 * exp.abs().max().item() * cnt) / cnt
    return exp, bound


@functools.lru_cache(None)
def cfg_inputs(name):
    """[2B][per]: test_gpu_cfg.py's rows -- unit normals, mean 3 / std 0.1 (the sums cancel to 1e-3 of their size), a constant."""
    sh = SHAPES[name]
    g = torch.Generator().manual_seed(per(sh))
    c, n = torch.randn(3, per(sh), generator=g), torch.randn(3, per(sh), generator=g)
    c[1], n[1] = 3 + 0.1 * c[1], 3 + 0.1 * n[1]
    c[2], n[2] = 0.5, 0.5
    return torch.cat([c[:sh.B], n[:sh.B]]).contiguous()


def cfg_ref(eps2, B, s, phi):
    """g = n + (c - n) s in three separately rounded float32 operations (torch on the CPU: the expression of
    Unet3D.forward_with_cond_scale), and g x the per-sample rescale factor with the sums and the factor in fp64.  Returns (g float32,
    g * factor float64, factor)."""
    c, n = eps2[:B], eps2[B:]
    g = n + (c - n) * s
    g64, c64 = g.numpy().astype(np.float64), c.numpy().astype(np.float64)
    cnt = c64.shape[1]
    phi64 = float(np.float32(phi))
    ss_c = (c64 * c64).sum(1) - c64.sum(1) ** 2 / cnt
    ss_g = (g64 * g64).sum(1) - g64.sum(1) ** 2 / cnt
    factor = np.ones(B)
    ok = ss_g > 0
    factor[ok] = phi64 * np.sqrt(np.maximum(ss_c[ok], 0) / ss_g[ok]) + (1.0 - phi64)
    return g, g64 * factor[:, None], factor


# ---- optimizer ------------------------------------------------------------------------------------------------------------------------

def _f(v):
    return torch.tensor(v, dtype=F32).item()


ADAM_HYP = dict(lr=_f(1e-4), b1=_f(0.9), b2=_f(0.999), eps=_f(1e-8), step_count=10, grad_scale=0.5, do_ema=True, ema_decay=_f(0.995))
ADAM_MAX_NORM = 1.0


@functools.lru_cache(None)
def adam_inputs(n=N_ADAM):
    """test_adam_ema_six_steps' draw: non-zero moments (from zero, the first step is lr sign(g) and hides any scale)."""
    g = torch.Generator().manual_seed(n)
    p0, m0 = torch.randn(n, generator=g), 0.1 * torch.randn(n, generator=g)
    v0 = 0.01 * torch.rand(n, generator=g) + 1e-6
    e0 = p0 + 0.01 * torch.randn(n, generator=g)
    grad = torch.randn(n, generator=g) * 0.1
    return dict(p=p0, g=grad, m=m0, v=v0, ema=e0)


def adam_ref(dt, max_norm=None):
    """One step of oracle/train_ref.adam_update + ema_update in dtype dt, behind the global-norm clip of the averaged gradient when
    max_norm is given (the reference's clip_grad_norm formula, epsilon 1e-6, norm in double)."""
    I, H = adam_inputs(), ADAM_HYP
    gs = I['g'].to(dt) * H['grad_scale']
    l2 = torch.sqrt((gs.double() ** 2).sum() + 1e-6)
    if max_norm is not None:
        gs = gs * torch.clamp(max_norm / (l2 + 1e-6), max=1.0).to(dt)
    p, m, v = TR.adam_update({'w': I['p'].to(dt)}, {'w': gs}, {'w': I['m'].to(dt)}, {'w': I['v'].to(dt)}, H['step_count'], H['lr'], H['b1'], H['b2'],
                             H['eps'])
    e = TR.ema_update({'w': I['ema'].to(dt)}, p, 1, 0, 1, H['ema_decay'])
    return dict(p=p['w'], dp=p['w'] - I['p'].to(dt), m=m['w'], v=v['w'], ema=e['w'], norm=l2.to(dt).reshape(1))


# ---- dynamic threshold ----------------------------------------------------------------------------------------------------------------

DYN_QS = (0.9, 0.5, 1.0, 0.123)
DYN_GAUSS = ((1, 1), (2, 1), (1023, 1), (1024, 1), (1024, 4), (1025, 1), (4100, 1), (4100, 4), (2100004, 4))      # (per_sample, C)
DYN_B, DYN_T = 3, (0, 5, 11)
DYN_MARGIN = 1.01                           # every asserted quantile is at least this: the clamp at 1 hides nothing
EXACT_QS = (0.5, 0.25, 0.75, 1.0)
EXACT_PERS = (4097, 2100005)                # odd and 1 mod 4: q (n - 1) is an integer for every q above; 4 trips + 1 and 2050 trips + 805
EXACT_PATTERNS = ('equal', 'inside', 'first', 'last', 'lowbyte', 'decades', 'zeros')
EXACT_T = (0, 5, 11, 0, 5, 11, 0)           # sample b of an exact batch carries pattern b at this t


def quantile_rank(q, n):
    """(k_lo, k_hi, frac) of the linearly interpolated quantile at position q (n - 1), q being the float32 the ABI receives."""
    pos = float(np.float32(q)) * (n - 1)
    lo = int(np.floor(pos))
    return lo, min(lo + 1, n - 1), pos - lo


def quantile_ref(v, q, shift=0):
    """The quantile of the 1-D float64 array v: sort, interpolate at q (n - 1).  shift moves both ranks (the host proofs' off-by-one)."""
    s = np.sort(np.asarray(v, dtype=np.float64))
    lo, hi, frac = quantile_rank(q, len(s))
    lo, hi = min(max(lo + shift, 0), len(s) - 1), min(max(hi + shift, 0), len(s) - 1)
    return s[lo] + frac * (s[hi] - s[lo])


@functools.lru_cache(None)
def dyn_tables():
    return device_tables(T_DYN)['ptab']


@functools.lru_cache(None)
def dyn_gauss(per_sample, C):
    """x = 10 N(0,1), eps = N(0,1); fp64 quantiles per (q, sample).  The seed is the first from 8 on at which every asserted quantile
    reaches DYN_MARGIN (it matters for per_sample 1 and 2 only)."""
    fhw = per_sample // C
    t = torch.tensor(DYN_T)
    tab = dyn_tables().double()
    for seed in range(8, 64):
        g = torch.Generator().manual_seed(seed)
        x = 10 * torch.randn(DYN_B, C, 1, 1, fhw, generator=g)
        eps = torch.randn(DYN_B, 1, 1, fhw, C, generator=g)
        x0 = tab[0][t].reshape(-1, 1, 1, 1, 1) * x.double() - tab[1][t].reshape(-1, 1, 1, 1, 1) * cf(eps).double()
        mag = np.sort(x0.abs().reshape(DYN_B, -1).numpy(), axis=1)
        ref = {q: np.array([quantile_ref(mag[b], q) for b in range(DYN_B)]) for q in DYN_QS}
        if min(r.min() for r in ref.values()) >= DYN_MARGIN:
            return dict(x=x, eps=eps, t=t.to(torch.int32), ref=ref, mag=mag, seed=seed)
    raise AssertionError('no seed gives quantiles above the clamp')


def _exact_x(pattern, n, k, rng):
    """float32 magnitudes-with-signs of one exact pattern; k = the wanted rank."""
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(np.float32)
    if pattern == 'equal':
        v = np.full(n, 3.0, np.float32)
    elif pattern in ('inside', 'first', 'last'):
        na = {'inside': k // 2, 'first': k, 'last': k + 1}[pattern]          # how many copies of the smaller value
        v = np.where(np.arange(n) < na, 2.0, 5.0).astype(np.float32)
    elif pattern == 'lowbyte':
        base = np.float32(7.0).view(np.uint32) & np.uint32(0xFFFFFF00)
        v = (base | rng.integers(0, 256, n).astype(np.uint32)).view(np.float32)
    elif pattern == 'decades':
        v = (10.0 ** rng.uniform(-3.0, 30.0, n)).astype(np.float32)
    elif pattern == 'zeros':
        v = (10.0 * np.abs(rng.standard_normal(n)) + 1e-3).astype(np.float32)
        v[rng.random(n) < 0.1] = 0.0
    else:
        raise KeyError(pattern)
    return rng.permutation(v) * sign                                            # -0.0 where v == 0 and the sign is negative


@functools.lru_cache(None)
def dyn_exact(per_sample, q):
    """eps = 0, C = 1: x0_hat = fl(kr x), which numpy reproduces bit for bit.  Sample b carries EXACT_PATTERNS[b] at t = EXACT_T[b].
    Returns x [7,1,1,1,per], t, and per sample the float32 order statistic the kernel must return bit for bit, with its neighbours."""
    k, k_hi, frac = quantile_rank(q, per_sample)
    rng = np.random.default_rng(per_sample + int(q * 100))
    kr = dyn_tables()[0].numpy()
    xs, want, below, above, mags = [], [], [], [], []
    for b, pattern in enumerate(EXACT_PATTERNS):
        x = _exact_x(pattern, per_sample, k, rng)
        mag = np.abs(np.float32(kr[EXACT_T[b]]) * x)                           # one float32 product, as the kernel's kr * x - km * 0
        s = np.sort(mag)
        xs.append(x); want.append(s[k]); below.append(s[max(k - 1, 0)]); above.append(s[min(k + 1, per_sample - 1)]); mags.append(s)
    x = torch.from_numpy(np.stack(xs)).reshape(len(xs), 1, 1, 1, per_sample)
    return dict(x=x, t=torch.tensor(EXACT_T, dtype=torch.int32), want=np.array(want, np.float32), below=np.array(below, np.float32),
                above=np.array(above, np.float32), sorted=mags, k=k, frac=frac)


# ---- emulated faulty kernels (host proofs) ------------------------------------------------------------------------------------------------

def eps_first_lane_channel(sh, eps):
    """What a float4 kernel reads from the channel-last eps_hat when it takes the channel of the quad's FIRST element for all four lanes:
    element e of a sample gets eps[r(e), c(4 (e / 4))].  Returned channel-first, [B,C,1,1,fhw]."""
    e = torch.arange(per(sh))
    c_first, r = (4 * (e // 4)) // sh.fhw, e % sh.fhw
    flat = eps.reshape(sh.B, sh.fhw, sh.C)
    return flat[:, r, c_first].reshape(dims(sh))


def second_sweep(sh):
    """Boolean [B,C,1,1,fhw]: the elements a float4 kernel reaches only on the second trip of its grid-stride loop."""
    e = torch.arange(per(sh)) >= SWEEP4
    return e.reshape(1, *dims(sh)[1:]).expand(*dims(sh))


def miss_second_sweep(sh, out, how):
    """An output whose second sweep was left unwritten ('nan': the sentinel) or holds the first sweep's values ('stale')."""
    flat = out.clone().reshape(sh.B, per(sh))
    n2 = per(sh) - SWEEP4
    flat[:, SWEEP4:] = float('nan') if how == 'nan' else flat[:, :n2]
    return flat.reshape(dims(sh))
