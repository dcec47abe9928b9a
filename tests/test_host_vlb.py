"""CPU tests of the held-out evaluation (GaussianDiffusion.calc_bpd_loop, vdx.h "Held-out evaluation"): the exported symbols, the
table, the fp64 restatement tests/_vlb_ref.py against torch.distributions, known answers, the argument rules of the new entries on a
machine without a device, evaluate.py's flags, and the proofs that the bounds of tests/test_gpu_vlb.py can tell a wrong kernel."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
from torch.distributions import Normal, kl_divergence

import _vlb_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE = -1, -4
F64 = torch.float64


def test_new_symbols_are_exported():
    lib = C.CDLL(os.path.join(ROOT, 'video_diffusion_nnx_amd', 'libvdx.so'))
    for name in ('vdx_vlb_noise', 'vdx_vlb_terms', 'vdx_vlb_prior', 'vdx_vlb_scratch_doubles', 'vdx_vlb_loop'):
        assert hasattr(lib, name), name
    from video_diffusion_nnx_amd import _lib as L, ops
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion, make_vlb_tables
    assert L.vdx_vlb_scratch_doubles(0) == 0 and L.vdx_vlb_scratch_doubles(3) == 3 * V.VLB_BLOCKS * 3
    for name in ('vlb_noise', 'vlb_terms', 'vlb_prior'):
        assert callable(getattr(ops, name))
    assert callable(make_vlb_tables) and callable(GaussianDiffusion.calc_bpd_loop)


@pytest.mark.parametrize('T', [2, 50, 1000])
def test_make_vlb_tables(T):
    from video_diffusion_nnx_amd.gaussian_diffusion import make_tables, make_vlb_tables
    tab, ref = make_vlb_tables(T), make_tables(T)
    assert tab.dtype == np.float64 and tab.shape == (9, T)
    names = ('sqrt_alphas_cumprod', 'sqrt_one_minus_alphas_cumprod', 'sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod',
             'posterior_mean_coef1', 'posterior_mean_coef2')
    for row, name in zip((0, 1, 2, 3, 4, 5, 8), names + ('alphas_cumprod',)):
        assert np.array_equal(tab[row], ref[name].astype(np.float64)), name           # the sampling kernels' fp32 values, widened
    c1, pv = ref['posterior_mean_coef1'].astype(np.float64), ref['posterior_variance'].astype(np.float64)
    w = np.array([math.fsum([c1[t] * c1[t]]) / (2.0 * pv[t] * math.log(2.0)) for t in range(1, T)])
    assert np.allclose(tab[6, 1:], w, rtol=1e-15, atol=0) and tab[6, 0] == 0.0
    assert tab[7, 0] == tab[7, 1] == math.log(pv[1]) and np.array_equal(tab[7, 1:], np.log(pv[1:]))
    assert np.isfinite(tab).all() and (tab[6] >= 0).all()
    with pytest.raises(ValueError):
        make_vlb_tables(1)


def _draw(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=F64), torch.randn(shape, generator=g, dtype=F64), torch.randn(shape, generator=g, dtype=F64)


def test_algebraic_kl_equals_the_general_normal_kl():
    """w_t (x0 - x0_hat)^2, what the kernel adds, against normal_kl(mu~, beta~, mu_theta, beta~) element by element, and against it and
    torch's kl_divergence as the term (the mean).  torch forms 0.5 (1 + d^2 - 1 - log 1): where d^2 is small (x0_hat clipped onto x0 at
    the highest levels) its own elements carry 1e-16 absolute, 1e-11 of the largest term, so torch is held to the mean."""
    tab = V.tables()
    x, eps, eh = _draw((1, 1, 1, 1, 4096))
    x0 = 2 * x - 1
    worst = worst_mean = 0.0
    for t in (1, 2, 10, 500, 998, 999):
        tt = torch.tensor([t])
        col = lambda r: V._col(tab, r, tt, F64)
        xt = V.x_t(x, eps, tt, tab)
        xh = (col('sqrt_recip') * xt - col('sqrt_recipm1') * eh).clamp(-1, 1)
        alg = col('w') * (x0 - xh) ** 2
        m1, m2, lv = col('coef1') * x0 + col('coef2') * xt, col('coef1') * xh + col('coef2') * xt, col('dec_logvar')
        gen = V.normal_kl(m1, lv, m2, lv) / V.LN2
        sd = torch.exp(0.5 * lv)
        tor = kl_divergence(Normal(m1, sd), Normal(m2, sd)) / V.LN2
        scale = alg.abs().max()
        worst = max(worst, ((alg - gen).abs().max() / scale).item())                  # element by element against the general form
        for other in (gen, tor):                                                     # the term itself: the mean over the sample
            worst_mean = max(worst_mean, (abs(alg.mean() - other.mean()) / alg.mean()).item())
    print(f'algebraic KL: worst element vs normal_kl {worst:.2e} of the largest term; worst mean vs normal_kl / torch {worst_mean:.2e}')
    assert worst < 1e-12 and worst_mean < 1e-12


def test_decoder_equals_cdf_differences():
    tab = V.tables()
    lv = torch.tensor(tab[7, 0], dtype=F64)
    sd = torch.exp(0.5 * lv)
    x0 = torch.cat([torch.tensor([-1.0, 1.0, -0.9995, 0.9995, 0.0], dtype=F64), torch.linspace(-1, 1, 255, dtype=F64)])
    for shift in (0.0, 0.5, -2.0, 3.0):                                   # the mean away from x0, in sigmas
        mean = x0 + shift * sd
        got = V.discretized_log_likelihood(x0, mean, lv)
        n = Normal(mean, sd)
        lo, hi = n.cdf(x0 - 1 / 255), n.cdf(x0 + 1 / 255)
        p = torch.where(x0 < -0.999, hi, torch.where(x0 > 0.999, 1 - lo, hi - lo))
        ok = p > 1e-9                                                     # where the cdf difference has not lost its digits
        assert ok.sum() >= 4
        assert torch.allclose(got[ok], torch.log(p[ok]), rtol=0, atol=1e-6), (shift, (got[ok] - torch.log(p[ok])).abs().max())
        assert (got <= 1e-15).all() and (got >= math.log(1e-12) - 1e-12).all()
    # x0 = +-1 exactly: the open-ended bins, everything beyond the edge
    edge = V.discretized_log_likelihood(torch.tensor([-1.0, 1.0], dtype=F64), torch.tensor([-1.3, 1.3], dtype=F64), lv)
    assert torch.allclose(edge, torch.zeros(2, dtype=F64), atol=1e-12)


def test_prior_equals_torch_kl():
    tab = V.tables()
    x, _, _ = _draw((3, 2, 2, 4, 4), 3)
    ac = torch.tensor(tab[8, -1], dtype=F64)
    exp = kl_divergence(Normal(ac.sqrt() * (2 * x - 1), (1 - ac).sqrt()), Normal(torch.zeros((), dtype=F64), torch.ones((), dtype=F64)))
    exp = exp.reshape(3, -1).mean(1) / V.LN2
    closed = (0.5 * (-1 - torch.log(1 - ac) + (1 - ac) + ac * (2 * x - 1) ** 2)).reshape(3, -1).mean(1) / V.LN2      # vdx.h's form
    # at T = 1000 the term is 5e-11 bits, the residue of -1 - log(1 - ac) + (1 - ac) at ac = 2.4e-10: fp64 round-off is 1e-16 absolute
    assert torch.allclose(V.prior(x, tab), exp, rtol=1e-12, atol=1e-15) and torch.allclose(closed, exp, rtol=1e-12, atol=1e-15)
    tab50 = V.tables(50)                                                  # a schedule whose prior is not a residue
    ac = torch.tensor(tab50[8, -1], dtype=F64)
    exp = kl_divergence(Normal(ac.sqrt() * (2 * x - 1), (1 - ac).sqrt()), Normal(torch.zeros((), dtype=F64), torch.ones((), dtype=F64)))
    assert torch.allclose(V.prior(x, tab50), exp.reshape(3, -1).mean(1) / V.LN2, rtol=1e-9, atol=1e-15)


def test_known_answers():
    tab = V.tables()
    x, eps, _ = _draw((3, 1, 2, 4, 4), 5)
    t = torch.tensor([1, 500, 999])
    vb, mse, xs = V.terms(x, eps, eps, t, tab, clip=False)                 # eps_hat = eps: the network is right
    assert (mse == 0).all() and (xs < 1e-9).all() and (vb.abs() < 1e-6).all()      # (the fp32 tables make recip * sqrt_ac 1 to 1e-7 only)
    vb, mse, xs = V.terms(x, torch.zeros_like(eps), eps, t, tab, clip=False)       # eps_hat = 0: x0_hat = recip x_t
    r = lambda v: v.reshape(3, -1).mean(1)
    x0 = 2 * x - 1
    xh = torch.tensor(tab[2])[t].reshape(3, 1, 1, 1, 1) * V.x_t(x, eps, t, tab)
    assert torch.allclose(mse, r(eps ** 2), rtol=1e-14)
    assert torch.allclose(xs, r((xh - x0) ** 2), rtol=1e-12)
    assert torch.allclose(vb, torch.tensor(tab[6])[t] * r((xh - x0) ** 2), rtol=1e-9)
    assert torch.allclose(xs, torch.tensor(tab[3])[t] ** 2 * r(eps ** 2), rtol=1e-4)      # x0_hat - x0 = recipm1 eps up to the tables' rounding
    for name in V.CASES:
        for clip in (True, False):
            for dt in (V.F32, F64):
                assert (V.case_ref(name, clip, dt)[0] >= 0).all(), (name, clip)


# ---- argument validation: every call below is refused before any launch, so none of them reads a buffer ---------------------------------

_host = (C.c_double * 80)()
BUF = (C.addressof(_host) + 15) & ~15
_vp, _u64 = C.c_void_p, C.c_uint64


def _entries():
    from video_diffusion_nnx_amd import _lib as L
    noise = L._sig('vdx_vlb_noise', C.c_int, [_vp] * 4 + [C.c_int, _vp, _u64, _u64, _vp, C.c_int, C.c_long, _vp])
    terms = L._sig('vdx_vlb_terms', C.c_int, [_vp] * 4 + [C.c_int, _vp, _u64, _u64, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_long, _vp])
    prior = L._sig('vdx_vlb_prior', C.c_int, [_vp, _vp, C.c_int, _vp, _vp, C.c_int, C.c_long, _vp])
    return L, noise, terms, prior


NOISE = dict(x=BUF, xt=BUF, t=BUF, tab=BUF, T=10, noise=0, seed=1, draw=0, step_dev=0, batch=2, per=16, stream=0)
TERMS = dict(x=BUF, eps=BUF, t=BUF, tab=BUF, T=10, noise=0, seed=1, draw=0, step_dev=0, clip=1, partial=BUF, out=BUF, batch=2, C=2, per=16, stream=0)
PRIOR = dict(x=BUF, tab=BUF, T=10, partial=BUF, out=BUF, batch=2, per=16, stream=0)
REJECTS = [   # (entry, changed arguments, what the message names)
    ('noise', dict(x=0), 'null'), ('noise', dict(xt=0), 'null'), ('noise', dict(t=0), 'null'), ('noise', dict(tab=0), 'null'),
    ('noise', dict(per=18), 'multiple of 4'), ('noise', dict(x=BUF + 4), '16-byte'), ('noise', dict(xt=BUF + 8), '16-byte'),
    ('noise', dict(noise=BUF + 4), '16-byte'), ('noise', dict(T=1), 'timesteps'), ('noise', dict(batch=0), 'batch'),
    ('noise', dict(tab=BUF + 4), '8-byte'),
    ('terms', dict(x=0), 'null'), ('terms', dict(eps=0), 'null'), ('terms', dict(partial=0), 'null'), ('terms', dict(out=0), 'null'),
    ('terms', dict(per=18), 'multiple of 4'), ('terms', dict(C=3, per=16), 'channels'), ('terms', dict(x=BUF + 4), '16-byte'),
    ('terms', dict(partial=BUF + 4), '8-byte'), ('terms', dict(out=BUF + 4), '8-byte'), ('terms', dict(T=1), 'timesteps'),
    ('terms', dict(C=0), 'channels'),
    ('prior', dict(x=0), 'null'), ('prior', dict(tab=0), 'null'), ('prior', dict(per=6), 'multiple of 4'), ('prior', dict(x=BUF + 8), '16-byte'),
    ('prior', dict(out=BUF + 4), '8-byte'), ('prior', dict(T=1), 'timesteps'),
]


@pytest.mark.parametrize('entry,change,word', REJECTS, ids=[f'{e}-{"-".join(c)}-{i}' for i, (e, c, _) in enumerate(REJECTS)])
def test_single_step_entries_reject(entry, change, word):
    L, noise, terms, prior = _entries()
    fn, base = dict(noise=(noise, NOISE), terms=(terms, TERMS), prior=(prior, PRIOR))[entry]
    rc = fn(*dict(base, **change).values())
    msg = L.vdx_last_error().decode()
    assert rc == INVALID, (rc, msg)
    assert msg.startswith(f'vlb_{entry}: ') and word in msg, msg


LOOP = dict(h=None, params=BUF, packed=BUF, x=BUF, xt=BUF, eps=BUF, t_dev=BUF, step_dev=BUF, tab=BUF, T=10, seq=BUF, seq_len=10, nsteps=1, cond=0,
            seed=3, clip=1, partial=BUF, out=BUF, ws=BUF, ws_bytes=1 << 20, batch=2, use_graph=0, stream=0)
LOOP_REJECTS = [(dict({n: 0}), 'null') for n in ('h', 'params', 'packed', 'x', 'xt', 'eps', 't_dev', 'step_dev', 'tab', 'seq', 'partial', 'out', 'ws')]
LOOP_RULES = [(dict(x=BUF + 4), '16-byte'), (dict(xt=BUF + 8), '16-byte'), (dict(eps=BUF + 4), '16-byte'), (dict(partial=BUF + 4), '8-byte'),
              (dict(out=BUF + 4), '8-byte'), (dict(nsteps=-1), 'nsteps'), (dict(nsteps=11), 'nsteps'), (dict(seq_len=0), 'seq_len'),
              (dict(T=1), 'timesteps'), (dict(batch=0), 'batch')]


def _cpu_unet(**kw):
    from video_diffusion_nnx_amd.unet3d import Unet3D
    return Unet3D(rngs=0, mode='f32', dim=16, channels=1, dim_mults=(1, 2), device='cpu', **kw)


def test_loop_rejects():
    """Nulls come first (VDX_ERR_INVALID), then the handle's device state (VDX_ERR_STATE without a GPU), then the rules -- all of it
    before any launch.  With a device the rule rows are refused by their rule; without one the state check comes before them."""
    from video_diffusion_nnx_amd import _lib as L
    unet = _cpu_unet()
    h = unet.handle(2, 8)
    base = dict(LOOP, h=h.ptr)
    for change, word in LOOP_REJECTS:
        rc = L.vdx_vlb_loop(*dict(base, **change).values())
        msg = L.vdx_last_error().decode()
        assert rc == INVALID and msg.startswith('vlb_loop: ') and word in msg, (change, rc, msg)
    gpu = torch.cuda.is_available()
    odd = _cpu_unet(out_dim=2)
    rules = LOOP_RULES + [(dict(h=odd.handle(2, 8).ptr), 'out_dim')]
    for change, word in rules:
        rc = L.vdx_vlb_loop(*dict(base, **change).values())
        msg = L.vdx_last_error().decode()
        if gpu:
            assert rc == INVALID and msg.startswith('vlb_loop: ') and word in msg, (change, rc, msg)
        else:
            assert rc == STATE and 'without a GPU' in msg, (change, rc, msg)


def test_calc_bpd_loop_argument_checks():
    """Checked before any device work: a CPU-only model raises the ValueError, not a GPU error."""
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion, vlb_time_sequence, ddim_time_sequence
    x = torch.rand(1, 1, 2, 8, 8)
    gd = GaussianDiffusion(_cpu_unet(), image_size=8, num_frames=2, channels=1, timesteps=10, use_dynamic_thres=True)
    with pytest.raises(ValueError, match='use_dynamic_thres'):
        gd.calc_bpd_loop(x, 0)
    gd = GaussianDiffusion(_cpu_unet(), image_size=8, num_frames=2, channels=1, timesteps=10)
    for bad in (0, 11, 2.5, True):
        with pytest.raises(ValueError, match='timesteps'):
            gd.calc_bpd_loop(x, 0, timesteps=bad)
    with pytest.raises(ValueError, match='x must be'):
        gd.calc_bpd_loop(torch.rand(1, 1, 2, 4, 4), 0)
    assert vlb_time_sequence(5).tolist() == [4, 3, 2, 1, 0, -1]
    assert np.array_equal(vlb_time_sequence(50, 10), ddim_time_sequence(50, 10))


def test_evaluate_cli_flags(tmp_path):
    import evaluate
    ok = ['--random-init', '--dataset-path', 'synthetic:4', '--output', str(tmp_path / 'o.json')]
    _, a = evaluate.parse_args(ok)
    assert (a.data_scale, a.eval_steps, a.num_videos, a.batch_size, a.no_clip, a.cond_path, a.mode) == (1.0, None, None, 2, False, None, 'bf16')
    _, a = evaluate.parse_args(ok + ['--eval-steps', '5', '--no-clip', '--data-scale', '0.00392156862', '--load-ema-params', '--step', '3',
                                     '--temporal-pos-bias', '--focus-present', '--num-videos', '3', '--seed', '9', '--mode', 'f32'])
    assert (a.eval_steps, a.no_clip, a.load_ema_params, a.step, a.num_videos, a.seed, a.mode) == (5, True, True, 3, 3, 9, 'f32')
    assert a.temporal_pos_bias and a.focus_present and abs(a.data_scale * 255 - 1) < 1e-6
    for bad in (['--random-init', '--output', 'o.json'],                                       # no --dataset-path
                ['--random-init', '--dataset-path', 'synthetic:4'],                            # no --output
                ['--dataset-path', 'synthetic:4', '--output', 'o.json'],                       # neither --checkpoint-path nor --random-init
                ok + ['--eval-steps', '0'], ok + ['--eval-steps', '-3'], ok + ['--eval-steps', 'x'],
                ok[:-1] + ['o.txt']):
        with pytest.raises(SystemExit):
            evaluate.parse_args(bad)
    ds, n = evaluate.load_videos('synthetic:4', 1, 2, 8, 3)
    assert n == 3 and ds[0].shape == (1, 2, 8, 8)
    # a MovingMNIST array (frames, videos, H, W): frames are cut or padded to num_frames, nothing is resized
    arr = np.random.default_rng(0).integers(0, 256, (3, 5, 8, 8)).astype(np.uint8)
    np.save(tmp_path / 'mm.npy', arr)
    ds, n = evaluate.load_videos(str(tmp_path / 'mm.npy'), 1, 2, 8)
    assert n == 5 and ds[4].shape == (1, 2, 8, 8) and ds[4].dtype == np.float32 and np.array_equal(ds[4][0], arr[:2, 4])
    assert evaluate.load_videos(str(tmp_path / 'mm.npy'), 1, 2, 8, 2)[1] == 2
    for channels, size in ((1, 16), (3, 8)):                            # another image_size or channel count than the file's
        with pytest.raises(ValueError, match='the config asks for'):
            evaluate.load_videos(str(tmp_path / 'mm.npy'), channels, 2, size)
    with pytest.raises(ValueError, match='no videos'):
        evaluate.load_videos('synthetic:0', 1, 2, 8)


# ---- the bounds of tests/test_gpu_vlb.py can tell: each mistake below moves a figure by >= 100 x its bound ------------------------------

def _ratios(wrong, name, clip, what):
    t = V.case(name)['t']
    ref = V.case_ref(name, clip)
    bound = V.term_bounds(V.case_ref(name, clip, V.F32), ref, t)
    diff = torch.stack([(w.double() - r).abs() for w, r in zip(wrong, ref)])
    ratio = diff / bound
    print(f'[{what}: {name} clip={clip}] |wrong - ref| / bound per (quantity, sample): {[[f"{v:.3g}" for v in row] for row in ratio.tolist()]}')
    return ratio


@pytest.mark.parametrize('name', list(V.CASES))
def test_sensitivity_noise_draw_shifted(name):
    """Another draw as eps (1 + k -> 2 + k): x_t and the eps-MSE are those of another noise."""
    from oracle import philox_ref
    c = V.case(name)
    n = c['x'].numel()
    e1 = torch.from_numpy(philox_ref.randn(n, 7, 1)).reshape(c['shape'])
    e2 = torch.from_numpy(philox_ref.randn(n, 7, 2)).reshape(c['shape'])
    eh = V.cf(c['eps_hat']) - c['eps'] + e1                                 # the same network error around the right draw
    ref = V.terms(c['x'], eh, e1, c['t'], V.tables(), True)
    wrong = V.terms(c['x'], eh, e2, c['t'], V.tables(), True)
    bound = V.term_bounds(V.terms(c['x'], eh, e1, c['t'], V.tables(), True, V.F32), ref, c['t'])
    ratio = torch.stack([(w - r).abs() for w, r in zip(wrong, ref)]) / bound
    print(f'[draw shifted: {name}] ratios {[[f"{v:.3g}" for v in row] for row in ratio.tolist()]}')
    assert (ratio >= 100).all()


def test_sensitivity_one_partial_dropped():
    """Workgroup 5 of sample 1's partial left out of the sum: its quads are q with (q mod 64 * 256) // 256 == 5."""
    name = 'WRAP'
    c = V.case(name)
    per = c['x'].numel() // c['x'].shape[0]
    q = torch.arange(per) // 4
    keep = ((q % (V.VLB_BLOCKS * V.THREADS)) // V.THREADS != 5).reshape(c['shape'][1:])
    for clip in (True, False):
        full = V.case_ref(name, clip)
        # the terms of sample 1 summed without the dropped workgroup's elements, channel by channel
        C_ = c['shape'][1]
        sums = [torch.zeros((), dtype=F64) for _ in range(3)]
        for ch in range(C_):
            idx = torch.nonzero(keep[ch, 0, 0]).flatten()
            part = V.terms(c['x'][1:2, ch:ch + 1][..., idx], V.cf(c['eps_hat'])[1:2, ch:ch + 1][..., idx], c['eps'][1:2, ch:ch + 1][..., idx],
                           c['t'][1:2], V.tables(), clip)
            for k in range(3):
                sums[k] = sums[k] + part[k][0] * idx.numel()
        wrong = [torch.stack([full[k][0], sums[k] / per]) for k in range(3)]
        ratio = _ratios(wrong, name, clip, 'partial dropped')
        assert (ratio[:, 1] >= 100).all()


@pytest.mark.parametrize('clip', [True, False])
def test_sensitivity_eps_hat_read_channel_first(clip):
    name = 'C3'
    c = V.case(name)
    as_cf = c['eps_hat'].reshape(c['shape'])                               # the channel-last buffer's floats taken as [B,C,F,H,W]
    wrong = V.terms(c['x'], as_cf, c['eps'], c['t'], V.tables(), clip)
    assert (_ratios(wrong, name, clip, 'eps_hat channel-first') >= 100).all()


@pytest.mark.parametrize('name', list(V.CASES))
def test_sensitivity_decoder_variance_of_level_0(name):
    """The t = 0 branch with posterior_log_variance_clipped[0] = log 1e-20 instead of log post_var_1: a delta function."""
    from video_diffusion_nnx_amd.gaussian_diffusion import make_tables
    lv0 = float(make_tables(V.T_CASE)['posterior_log_variance_clipped'][0])
    assert lv0 < -40
    c = V.case(name)
    wrong = V.terms(c['x'], V.cf(c['eps_hat']), c['eps'], c['t'], V.tables(), True, dec_logvar0=lv0)
    ratio = _ratios(wrong, name, True, 'decoder log-variance of level 0')
    assert (ratio[0][c['t'] == 0] >= 100).all()
