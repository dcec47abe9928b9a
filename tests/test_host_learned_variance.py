"""Learned reverse-process variances on the host (no GPU): the tables, the fp64 restatement tests/_lv_ref.py against itself (closed-form
gradients = autograd = central differences, the equal-variance and analytic cases) and the plumbing (symbols, refusals on a CPU handle, YAML
and command-line switches, the defaults)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lv_ref as R          # noqa: E402
import _vlb_ref as V         # noqa: E402

F64 = torch.float64
INVALID, STATE = -1, -4
BUF = 1 << 20


# ---- tables --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('T', [2, 50, 1000])
def test_full_sequence_is_the_unrespaced_table_bitwise(T):
    from video_diffusion_nnx_amd.gaussian_diffusion import make_lv_tables
    a, b = make_lv_tables(T), make_lv_tables(T, range(T))
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    assert a['step'].shape == (6, T) and a['step'].dtype == np.float32 and a['tab64'].shape == (9, T) and a['tab64'].dtype == np.float64


def test_tables_follow_the_definitions():
    from video_diffusion_nnx_amd.gaussian_diffusion import cosine_beta_schedule, ddim_time_sequence, lv_time_sequence, make_lv_tables, make_tables
    T = 1000
    t = make_lv_tables(T)
    assert np.allclose(t['tab64'], R.ref_tables(T), rtol=1e-13, atol=0)
    # the full chain's beta' is the schedule's beta up to the rounding of alpha_bar; the fp32 tables are the same numbers in fp32
    assert np.allclose(t['betas'], cosine_beta_schedule(T).astype(np.float64), rtol=1e-12)
    old = make_tables(T)
    # (1 - alpha_bar in fp32 at the first levels, alpha_bar = 1 - 4e-5: one fp32 rounding of alpha_bar is 2^-24 / 4e-5 = 1.5e-3 of it)
    assert np.allclose(t['posterior_mean_coef1'], old['posterior_mean_coef1'], rtol=5e-3)
    assert np.allclose(t['min_log'][1:], old['posterior_log_variance_clipped'][1:], atol=5e-3)
    assert t['min_log'][0] == t['min_log'][1] and t['min_log'][0] > -20          # log beta~_1, not the clipped log 1e-20
    assert np.all(t['max_log'] >= t['min_log'])
    # respacing: alpha_bar' is picked from the full chain and telescopes through beta'
    seq = ddim_time_sequence(T, 50)[:-1][::-1]
    r = make_lv_tables(T, seq)
    assert r['seq'].tolist() == seq.tolist() and np.array_equal(lv_time_sequence(T, 50), ddim_time_sequence(T, 50))
    assert np.array_equal(r['alphas_cumprod'], t['alphas_cumprod'][seq])
    assert np.allclose(np.cumprod(1.0 - r['betas']), r['alphas_cumprod'], rtol=1e-12)
    assert np.allclose(r['tab64'], R.ref_tables(T, seq), rtol=1e-13, atol=0)
    assert np.all(r['betas'] >= t['betas'][seq] - 1e-15)                           # a longer stride adds more noise
    assert lv_time_sequence(5).tolist() == [4, 3, 2, 1, 0, -1]
    one = make_lv_tables(10, [9])
    assert one['step'].shape == (6, 1) and one['min_log'][0] == one['max_log'][0]
    for bad in ([], [3, 3], [5, 2], [-1, 2], [0, 10], range(11)):
        with pytest.raises(ValueError, match='seq'):
            make_lv_tables(10, bad)
    for bad in (0, 11, 2.5, True):
        with pytest.raises(ValueError, match='steps'):
            lv_time_sequence(10, bad)


# ---- the reference against itself ---------------------------------------------------------------------------------------------------------

def _small_case(C=2, seed=0, T=50):
    g = torch.Generator().manual_seed(seed)
    shape = (4, C, 2, 3, 3)
    x0 = torch.rand(shape, generator=g, dtype=F64) * 2 - 1
    x0.view(4, -1)[:, 0], x0.view(4, -1)[:, 1] = -1.0, 1.0
    eps = torch.randn(shape, generator=g, dtype=F64)
    eh = eps + 0.3 * torch.randn(shape, generator=g, dtype=F64)
    v = torch.rand(shape, generator=g, dtype=F64) * 8 - 4                            # far outside [-1, 1]: extrapolation
    out2 = torch.cat([eh, v], 1).permute(0, 2, 3, 4, 1).contiguous()
    t = torch.tensor([0, 1, T - 1, T // 2], dtype=torch.int32)
    from video_diffusion_nnx_amd.gaussian_diffusion import make_lv_tables
    return x0, eps, out2, t, make_lv_tables(T)['tab64']


@pytest.mark.parametrize('l2', [False, True])
def test_closed_form_gradients_equal_autograd_and_central_differences(l2):
    x0, eps, out2, t, tab = _small_case()
    w = 0.37
    _, g_auto = R.hybrid_grad(x0, eps, out2, t, tab, l2, w)
    g_cf = R.closed_form_grads(x0, eps, out2, t, tab, l2, w)
    scale = g_auto.abs().max()
    assert (g_cf - g_auto).abs().max() <= 1e-12 * scale, ((g_cf - g_auto).abs().max(), scale)
    C = x0.shape[1]
    assert g_auto[..., C:].abs().min() > 0                                           # every v receives gradient
    # central differences on a handful of entries of both halves (and of every level)
    flat = out2.reshape(-1)
    h = 1e-6
    for i in torch.linspace(0, flat.numel() - 1, 24).long().tolist():
        hi, lo = flat.clone(), flat.clone()
        hi[i] += h
        lo[i] -= h
        # (a difference quotient cannot see the detach: an eps_hat entry is checked on the simple loss alone, w = 0)
        wi = w if i % (2 * C) >= C else 0.0
        f = lambda z: R.hybrid(x0, eps, z.reshape(out2.shape), t, tab, l2, wi)['loss']
        num = (f(hi) - f(lo)) / (2 * h)
        ref = g_auto.reshape(-1)[i]
        assert abs(num - ref) <= 1e-6 * max(abs(ref), float(scale)), (i, float(num), float(ref))


def test_eps_half_is_detached_inside_the_variational_term():
    """With w the only weight, d loss / d eps_hat is the simple loss's gradient whatever w is."""
    x0, eps, out2, t, tab = _small_case()
    C = x0.shape[1]
    g0 = R.hybrid_grad(x0, eps, out2, t, tab, True, 0.0)[1]
    g1 = R.hybrid_grad(x0, eps, out2, t, tab, True, 5.0)[1]
    assert torch.equal(g0[..., :C], g1[..., :C]) and g0[..., C:].abs().max() == 0 and g1[..., C:].abs().max() > 0


def test_kl_vanishes_at_equal_moments():
    x0, eps, out2, t, tab = _small_case()
    C = x0.shape[1]
    xt = R.xt_of(x0, eps, t, tab)
    # eps_hat = eps exactly reproduces x0_hat = x0 up to rounding; v = -1 is the posterior variance
    col = lambda r: R._col(tab, r, t, F64)
    eh = (col('sqrt_recip') * xt - x0) / col('sqrt_recipm1')
    vb, _ = R.vb_elements(x0, xt, eh, -torch.ones_like(x0), t, tab)
    assert vb[1:].abs().max() < 1e-9, vb[1:].abs().max()                             # t >= 1 rows


# the two CPU references at v = -1, t >= 1: |lv - fixed| / fixed per sample measured 7.75e-15 at worst (fp64 rounding of two different
# expressions of the same KL: the general normal_kl at equal variances against w_t (x0_hat - x0)^2) -> 4 x that
EQUAL_VARIANCE_BOUND = 3.1e-14


def test_posterior_variance_reduces_to_the_fixed_variance_bound():
    T = 1000
    c = R.hybrid_case('C3_ODD')
    tab = R.tables(T)['tab64']
    t = torch.tensor([1, 2, T - 1, 400], dtype=torch.int32)
    x = (c['x0'].double() + 1) / 2                                                    # _vlb_ref takes x in [0, 1]
    eh, _ = R.split(c['out2'].double(), 3)
    out2 = torch.cat([eh, -torch.ones_like(eh)], 1).permute(0, 2, 3, 4, 1)
    vb_lv = R.bound_terms(x, out2, c['eps'], t, tab, clip=True)[0]
    # the same chain in _vlb_ref's layout: w_t = coef1^2 / (2 beta~_t ln 2), the coefficients of x_t rounded to fp32 as the kernels take them
    vtab = np.array(tab, copy=True)
    vtab[0], vtab[1] = vtab[0].astype(np.float32), vtab[1].astype(np.float32)
    vtab[6] = tab[4] ** 2 / (2.0 * np.exp(tab[7]) * math.log(2.0))
    vtab[7] = tab[7]
    vb_fixed, _, xstart_mse = V.terms(x, eh, c['eps'], t, vtab, clip=True)
    assert torch.equal(vb_lv, vb_fixed)            # (_vlb_ref evaluates the same general normal_kl: at equal variances the same operations)
    vb_fixed = torch.from_numpy(vtab[6])[t.long()] * xstart_mse                        # the closed form the fixed-variance kernel uses
    err = ((vb_lv - vb_fixed).abs() / vb_fixed).max().item()
    print(f'equal variances: lv reference vs fixed-variance reference, worst relative distance {err:.2e} (bound {EQUAL_VARIANCE_BOUND:.1e})')
    assert err < EQUAL_VARIANCE_BOUND


def test_minimising_vb_over_v_recovers_the_analytic_posterior_variance():
    """x0 ~ N(0, s^2) in one dimension: the optimal eps_hat is E[eps | x_t] = sqrt(1 - ac) x_t / (ac s^2 + 1 - ac), the reverse
    conditional q(x_{t-1} | x_t) is Gaussian with variance beta~_t + coef1^2 Var(x0 | x_t), Var(x0 | x_t) = s^2 (1 - ac) / (ac s^2 + 1 - ac),
    and the v that minimises the expected variational term is the one whose sigma^2 equals it."""
    T, s, n = 100, 0.5, 400000
    tab = R.tables(T)['tab64']
    g = torch.Generator().manual_seed(3)
    for lvl in (5, 40, 90):
        t = torch.tensor([lvl], dtype=torch.int32)
        x0 = (s * torch.randn(n, generator=g, dtype=F64)).reshape(1, 1, 1, 1, n)
        eps = torch.randn(n, generator=g, dtype=F64).reshape(1, 1, 1, 1, n)
        ac, c1, max_log, min_log = (float(tab[R.ROWS[k]][lvl]) for k in ('ac', 'coef1', 'max_log', 'min_log'))
        a32, s32 = float(np.float32(tab[0][lvl])), float(np.float32(tab[1][lvl]))
        xt = a32 * x0 + s32 * eps
        eh = math.sqrt(1 - ac) * xt / (ac * s * s + 1 - ac)
        f = lambda v: float(R.vb_elements(x0, xt, eh, torch.full_like(x0, v), t, tab)[0].mean())
        lo, hi = -6.0, 6.0                                                               # golden section: vb is unimodal in log sigma^2
        gr = (math.sqrt(5) - 1) / 2
        for _ in range(60):
            m1, m2 = hi - gr * (hi - lo), lo + gr * (hi - lo)
            lo, hi = (lo, m2) if f(m1) < f(m2) else (m1, hi)
        v_star = 0.5 * (lo + hi)
        got = float(R.log_variance(torch.tensor(v_star, dtype=F64), max_log, min_log))
        want = math.log(math.exp(min_log) + c1 * c1 * s * s * (1 - ac) / (ac * s * s + 1 - ac))
        # Monte-Carlo: the sample mean of (mu~ - mu)^2 has relative error about sqrt(2 / n) = 2.2e-3; 4 x that on sigma^2, in the log
        assert abs(got - want) < 4 * math.sqrt(2.0 / n), (lvl, got, want)


def test_step_at_v_minus_one_is_the_fixed_variance_step():
    """The reference step with v = -1 on the fp32 tables of the ancestral sampler is DiffusionRef's p_sample arithmetic."""
    from video_diffusion_nnx_amd.gaussian_diffusion import make_tables
    T = 20
    old = make_tables(T)
    step_tab = np.stack([old['sqrt_recip_alphas_cumprod'], old['sqrt_recipm1_alphas_cumprod'], old['posterior_mean_coef1'],
                         old['posterior_mean_coef2'], np.zeros(T, np.float32), old['posterior_log_variance_clipped']]).astype(np.float64)
    g = torch.Generator().manual_seed(0)
    x, eh, z = (torch.randn(3, 1, 2, 4, 4, generator=g, dtype=F64) for _ in range(3))
    lvl = torch.tensor([0, 7, T - 1])
    got = R.step(x, eh, -torch.ones_like(x), z, lvl, step_tab)
    c = lambda k: torch.from_numpy(old[k].astype(np.float64))[lvl].reshape(-1, 1, 1, 1, 1)
    xh = (c('sqrt_recip_alphas_cumprod') * x - c('sqrt_recipm1_alphas_cumprod') * eh).clamp(-1, 1)
    want = c('posterior_mean_coef1') * xh + c('posterior_mean_coef2') * x \
        + (lvl != 0).double().reshape(-1, 1, 1, 1, 1) * torch.exp(0.5 * c('posterior_log_variance_clipped')) * z
    assert torch.allclose(got, want, rtol=0, atol=1e-14)
    assert torch.equal(got[0], (c('posterior_mean_coef1') * xh + c('posterior_mean_coef2') * x)[0])      # level 0 adds no noise


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------------

def test_symbols_and_signatures():
    from video_diffusion_nnx_amd import _lib as L
    vp, u64 = C.c_void_p, C.c_uint64
    want = {
        'vdx_p_sample_step_lv': [vp] * 5 + [C.c_int, u64, vp, vp, u64, u64, vp, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_long, vp],
        'vdx_p_sample_loop_lv': [vp] * 9 + [C.c_int] * 3 + [vp, u64, C.c_int, C.c_float, C.c_float, vp, C.c_size_t, C.c_int, C.c_int, vp],
        'vdx_hybrid_loss': [vp] * 5 + [C.c_int, C.c_float, C.c_float, C.c_int, C.c_double, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_long, vp],
        'vdx_vlb_terms_lv': [vp] * 4 + [C.c_int, vp, u64, u64, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_long, vp],
        'vdx_vlb_loop_lv': list(L.vdx_vlb_loop.argtypes),
        'vdx_final_conv_backward_wide': [vp, C.c_int] + [vp] * 5 + [C.c_long, C.c_int, C.c_int, vp, C.c_size_t, vp],
    }
    for name, args in want.items():
        fn = getattr(L, name)
        assert getattr(L.lib, name) is not None and list(fn.argtypes) == args and fn.restype is C.c_int, name
    assert L.vdx_hybrid_scratch_doubles(3) == 3 * 64 * 3 + 6 and L.vdx_hybrid_scratch_doubles(0) == 0 and L.LV_ROWS == 9
    # the header declares them with the argument counts bound above
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'vdx.h')).read()
    for name, args in want.items():
        decl = hdr[hdr.index(f'int {name}('):]
        assert decl[:decl.index(');')].count(',') + 1 == len(args), name


def _cpu_unet(**kw):
    from video_diffusion_nnx_amd.unet3d import Unet3D
    return Unet3D(rngs=0, mode='f32', dim=16, channels=kw.pop('channels', 1), dim_mults=(1, 2), device='cpu', **kw)


STEP = dict(x=BUF, out2=BUF, out=BUF, level=0, tab=BUF, S=4, step=0, step_dev=0, noise=BUF, seed=1, offset=0, dev_offset=0, clip=1, ps=1.0, sh=0.0,
            batch=2, C=2, per=16, stream=0)
HYB = dict(x=BUF, noise=BUF, out2=BUF, t=BUF, tab=BUF, T=10, ps=2.0, sh=-1.0, l2=1, w=0.01, want=1, d_out=BUF, scratch=BUF, out=BUF, batch=2, C=2,
           per=16, stream=0)
TERMS = dict(x=BUF, out2=BUF, t=BUF, tab=BUF, T=10, noise=0, seed=1, draw=0, step_dev=0, clip=1, partial=BUF, out=BUF, batch=2, C=2, per=16, stream=0)
REJECTS = [
    ('p_sample_step_lv', STEP, dict(x=0), 'null'), ('p_sample_step_lv', STEP, dict(out2=0), 'null'), ('p_sample_step_lv', STEP, dict(tab=0), 'null'),
    ('p_sample_step_lv', STEP, dict(S=0), 'S must be in [1, timesteps]'), ('p_sample_step_lv', STEP, dict(step=4), 'step must be below S'),
    ('p_sample_step_lv', STEP, dict(noise=0, per=18), 'per_sample % 4'), ('p_sample_step_lv', STEP, dict(C=3), 'multiple of channels'),
    ('p_sample_step_lv', STEP, dict(batch=0), 'batch'),
    ('hybrid_loss', HYB, dict(x=0), 'null'), ('hybrid_loss', HYB, dict(out2=0), 'null'), ('hybrid_loss', HYB, dict(scratch=0), 'null'),
    ('hybrid_loss', HYB, dict(d_out=0), 'want_grad'), ('hybrid_loss', HYB, dict(T=1), 'timesteps'), ('hybrid_loss', HYB, dict(C=3), 'multiple of channels'),
    ('hybrid_loss', HYB, dict(x=BUF + 4), '16-byte'), ('hybrid_loss', HYB, dict(out=BUF + 4), '8-byte'), ('hybrid_loss', HYB, dict(batch=0), 'batch'),
    ('vlb_terms_lv', TERMS, dict(out2=0), 'null'), ('vlb_terms_lv', TERMS, dict(per=18), 'multiple of 4'), ('vlb_terms_lv', TERMS, dict(T=1), 'timesteps'),
    ('vlb_terms_lv', TERMS, dict(partial=BUF + 4), '8-byte'),
]


@pytest.mark.parametrize('entry,base,change,word', REJECTS, ids=[f'{e}-{"-".join(c)}-{i}' for i, (e, _, c, _) in enumerate(REJECTS)])
def test_single_step_entries_reject_before_any_launch(entry, base, change, word):
    from video_diffusion_nnx_amd import _lib as L
    rc = getattr(L, 'vdx_' + entry)(*dict(base, **change).values())
    msg = L.vdx_last_error().decode()
    assert rc == INVALID and msg.startswith(entry + ': ') and word in msg, (rc, msg)


LOOP = dict(h=None, params=BUF, packed=BUF, img=BUF, out2=BUF, t_dev=BUF, step_dev=BUF, tab=BUF, seq=BUF, S=4, T=10, nsteps=1, cond=0, seed=3, clip=1,
            ps=0.5, sh=0.5, ws=BUF, ws_bytes=1 << 20, batch=2, use_graph=0, stream=0)


def test_sampling_loop_rejects_on_a_cpu_handle():
    """Nulls, the out_dim rule and the S rule are refused by name before the handle's device state is looked at; nothing is launched."""
    from video_diffusion_nnx_amd import _lib as L
    lv, plain = _cpu_unet(out_dim=2), _cpu_unet()
    base = dict(LOOP, h=lv.handle(2, 8).ptr)
    call = lambda **ch: (L.vdx_p_sample_loop_lv(*dict(base, **ch).values()), L.vdx_last_error().decode())
    for n in ('h', 'params', 'packed', 'img', 'out2', 't_dev', 'step_dev', 'tab', 'seq', 'ws'):
        rc, msg = call(**{n: 0})
        assert rc == INVALID and msg.startswith('p_sample_loop_lv: ') and 'null' in msg, (n, rc, msg)
    for ch, word in ((dict(h=plain.handle(2, 8).ptr), 'out_dim must equal 2 * channels'), (dict(h=_cpu_unet(out_dim=3).handle(2, 8).ptr), 'out_dim'),
                     (dict(S=0), 'S must be in [1, timesteps]'), (dict(S=11), 'S must be in [1, timesteps]'), (dict(nsteps=5), 'nsteps'),
                     (dict(nsteps=-1), 'nsteps'), (dict(batch=0), 'batch')):
        rc, msg = call(**ch)
        assert rc == INVALID and msg.startswith('p_sample_loop_lv: ') and word in msg, (ch, rc, msg)
    rc, msg = call()
    assert rc == STATE and 'without a GPU' in msg, (rc, msg)
    # the evaluation loop keeps vdx_vlb_loop's order: nulls, then the device state
    vl = dict(h=lv.handle(2, 8).ptr, params=BUF, packed=BUF, x=BUF, xt=BUF, eps=BUF, t_dev=BUF, step_dev=BUF, tab=BUF, T=10, seq=BUF, seq_len=10, nsteps=1,
              cond=0, seed=3, clip=1, partial=BUF, out=BUF, ws=BUF, ws_bytes=1 << 20, batch=2, use_graph=0, stream=0)
    rc = L.vdx_vlb_loop_lv(*dict(vl, x=0).values())
    assert rc == INVALID and L.vdx_last_error().decode().startswith('vlb_loop_lv: ')
    rc = L.vdx_vlb_loop_lv(*vl.values())
    msg = L.vdx_last_error().decode()
    if torch.cuda.is_available():
        rc = L.vdx_vlb_loop_lv(*dict(vl, h=plain.handle(2, 8).ptr).values())
        msg = L.vdx_last_error().decode()
        assert rc == INVALID and 'out_dim must equal 2 * channels' in msg, (rc, msg)
    else:
        assert rc == STATE and 'without a GPU' in msg, (rc, msg)
    # the existing loops still refuse this network (on a CPU handle the sampling loops' rules come first)
    from video_diffusion_nnx_amd.gaussian_diffusion import vdx_p_sample_loop
    rc = vdx_p_sample_loop(lv.handle(2, 8).ptr, BUF, BUF, BUF, BUF, BUF, BUF, BUF, 10, 1, 0, 3, 1, BUF, 1 << 20, 2, 0, 0)
    msg = L.vdx_last_error().decode()
    assert rc in (INVALID, STATE) and (rc == STATE or 'out_dim must equal channels' in msg), (rc, msg)


OLD_ATTRIBUTES = ['_mtab', '_mtab_clean', '_ptab', '_sample_stream', 'alphas_cumprod', 'channels', 'denoise_fn', 'device', 'dynamic_thres_percentile',
                  'image_size', 'log_one_minus_alphas_cumprod', 'loss_type', 'num_frames', 'num_timesteps', 'posterior_log_variance_clipped',
                  'posterior_mean_coef1', 'posterior_mean_coef2', 'posterior_variance', 'sample_act_bf16', 'sqrt_alphas_cumprod',
                  'sqrt_one_minus_alphas_cumprod', 'sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod', 'text_use_bert_cls', 'use_dynamic_thres']


def test_constructor_switch_and_defaults():
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion, make_tables
    kw = dict(image_size=8, num_frames=2, channels=1, timesteps=10)
    gd = GaussianDiffusion(_cpu_unet(), **kw)
    assert sorted(vars(gd)) == sorted(OLD_ATTRIBUTES + ['learned_variance', 'vlb_weight', 'last_loss_terms'])
    assert gd.learned_variance is False and gd.vlb_weight is None and gd.last_loss_terms is None
    tabs = make_tables(10)
    for k, val in tabs.items():
        assert torch.equal(getattr(gd, k), torch.from_numpy(val)), k
    assert (gd.loss_type, gd.use_dynamic_thres, gd.dynamic_thres_percentile, gd.sample_act_bf16, gd.num_timesteps) == ('l1', False, 0.9, True, 10)
    with pytest.raises(ValueError, match='out_dim == 2 \\* channels'):
        GaussianDiffusion(_cpu_unet(), learned_variance=True, **kw)
    with pytest.raises(ValueError, match='out_dim == 2 \\* channels'):
        GaussianDiffusion(_cpu_unet(channels=3, out_dim=3), learned_variance=True, **dict(kw, channels=3))
    with pytest.raises(ValueError, match='needs learned_variance'):
        GaussianDiffusion(_cpu_unet(), vlb_weight=0.1, **kw)
    with pytest.raises(ValueError, match='use_dynamic_thres'):
        GaussianDiffusion(_cpu_unet(out_dim=2), learned_variance=True, use_dynamic_thres=True, **kw)
    on = GaussianDiffusion(_cpu_unet(out_dim=2), learned_variance=True, **dict(kw, timesteps=250))
    assert on.learned_variance and on.vlb_weight == 0.25
    assert GaussianDiffusion(_cpu_unet(out_dim=2), learned_variance=True, vlb_weight=0.5, **kw).vlb_weight == 0.5
    assert GaussianDiffusion(_cpu_unet(channels=3, out_dim=6), learned_variance=True, **dict(kw, channels=3)).learned_variance


def test_unsupported_combinations_raise_before_any_device_work():
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    kw = dict(image_size=8, num_frames=2, channels=1, timesteps=10)
    gd = GaussianDiffusion(_cpu_unet(out_dim=2), learned_variance=True, **kw)
    shape, x = (1, 1, 2, 8, 8), torch.rand(1, 1, 2, 8, 8)
    calls = {
        'cond_scale': lambda: gd.p_sample_loop(shape, 0, cond=torch.zeros(1, 4), cond_scale=2.0),
        'ddim_steps': lambda: gd.sample(0, batch_size=1, ddim_steps=4),
        'dpm_steps': lambda: gd.sample(0, batch_size=1, dpm_steps=4),
        'ddim_steps ': lambda: gd.ddim_sample_loop(shape, 0, steps=4),
        'dpm_steps ': lambda: gd.dpm_sample_loop(shape, 0, steps=4),
        'inpaint': lambda: gd.inpaint(0, x, torch.tensor([1, 0], dtype=torch.uint8)),
        'extend': lambda: gd.extend(0, x, 2),
        'focus_present': lambda: gd.sample(0, batch_size=1, focus_present=True),
        'frame_mask': lambda: gd.p_losses(x, torch.zeros(1, dtype=torch.int32), 0, frame_mask=torch.tensor([1, 0], dtype=torch.uint8)),
        'focus_present ': lambda: gd.calc_bpd_loop(x, 0, focus_present=True),
    }
    for word, fn in calls.items():
        with pytest.raises(ValueError, match=f'learned_variance does not support {word.strip()}'):
            fn()
    for bad in (0, 11, 2.5):
        with pytest.raises(ValueError, match='steps'):
            gd.sample(0, batch_size=1, steps=bad)
    plain = GaussianDiffusion(_cpu_unet(), **kw)
    with pytest.raises(ValueError, match='learned_variance'):
        plain.sample(0, batch_size=1, steps=4)
    with pytest.raises(ValueError, match='learned_variance'):
        plain.p_sample_loop(shape, 0, steps=4)


def test_yaml_and_command_line_switches(tmp_path):
    import yaml
    import sample
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(sample.__file__), 'configs', 'config_v1_0.yaml')))
    cfg['unet'].update(dim=16, dim_mults=[1, 2])
    import video_diffusion_nnx_amd.unet3d as U
    made = {}
    real = U.Unet3D

    class CpuUnet(real):
        def __init__(self, *a, **k):
            made.update(k)
            super().__init__(*a, device='cpu', **k)

    U.Unet3D = CpuUnet
    try:
        unet, gd = sample.build_models(cfg, 'f32')
        assert unet.out_dim == cfg['unet']['channels'] and gd.learned_variance is False and 'out_dim' not in made        # an absent key means off
        cfg['diffusion']['learned_variance'] = True
        unet, gd = sample.build_models(cfg, 'f32')
        assert unet.out_dim == 2 * cfg['unet']['channels'] and gd.learned_variance and gd.vlb_weight == cfg['diffusion']['timesteps'] / 1000.0
        cfg['diffusion']['vlb_weight'] = 0.125
        assert sample.build_models(cfg, 'f32')[1].vlb_weight == 0.125
        cfg['diffusion']['learned_variance'] = False
        del cfg['diffusion']['vlb_weight']
        assert sample.build_models(cfg, 'f32')[1].learned_variance is False
    finally:
        U.Unet3D = real
    a = sample.build_parser().parse_args(['--random-init', '--steps', '50'])
    assert a.steps == 50 and sample.build_parser().parse_args(['--random-init']).steps is None
    for clash in (['--ddim-steps', '4'], ['--dpm-steps', '4']):
        with pytest.raises(SystemExit):
            sample.main(['--random-init', '--steps', '4', '--output-path', str(tmp_path)] + clash)
