"""The v-prediction objective and the min-SNR loss weights on the host (no GPU): the algebra and the weights in float64 over the
project's own schedule, a DDIM chain driven by the exact v against the one driven by the exact eps, and the plumbing -- constructor
rules and refusals, that a plain diffusion has no new attribute, the C entries against the header, the handle's prediction state on a
CPU handle, the YAML keys and the command-line flags."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _vpred_ref as V          # noqa: E402
from _launch_hook import launches          # noqa: E402
from test_host_superres import PARENT_ATTRIBUTES          # noqa: E402  (the instance attributes of a plain diffusion)

INVALID, STATE = -1, -4
BUF = 1 << 20
T = 1000


def _ac():
    from video_diffusion_nnx_amd.gaussian_diffusion import make_tables
    return make_tables(T)['alphas_cumprod'].astype(np.float64)


# ---- the algebra -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('t', [0, 1, 500, T - 1])
def test_eps_and_x0_from_the_exact_v(t):
    a, s = V.coefs(_ac()[t])
    assert abs(a * a + s * s - 1.0) <= 2.0 ** -52
    rng = np.random.default_rng(t)
    x0, eps = rng.uniform(-1.0, 1.0, 4096), rng.standard_normal(4096)
    x_t = a * x0 + s * eps
    v = V.v_target(a, s, x0, eps)
    assert np.abs(V.eps_from_v(a, s, x_t, v) - eps).max() <= 1e-12
    assert np.abs(V.x0_from_v(a, s, x_t, v) - x0).max() <= 1e-12


def test_table_lookups_agree_with_the_algebra():
    """predict_v / predict_start_from_v / predict_noise_from_v are the fp32 look-ups of the same three lines."""
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    gd = GaussianDiffusion(_cpu_unet(), image_size=8, num_frames=4, channels=1, timesteps=T, objective='pred_v')
    g = torch.Generator().manual_seed(0)
    x0, eps = torch.rand(4, 1, 4, 8, 8, generator=g) * 2 - 1, torch.randn(4, 1, 4, 8, 8, generator=g)
    t = torch.tensor([0, 1, 500, T - 1])
    x_t = gd.sqrt_alphas_cumprod[t].reshape(-1, 1, 1, 1, 1) * x0 + gd.sqrt_one_minus_alphas_cumprod[t].reshape(-1, 1, 1, 1, 1) * eps
    v = gd.predict_v(x0, t, eps)
    a, s = V.coefs(_ac()[t.numpy()])
    want = V.v_target(a.reshape(-1, 1, 1, 1, 1), s.reshape(-1, 1, 1, 1, 1), x0.double().numpy(), eps.double().numpy())
    assert np.abs(v.double().numpy() - want).max() < 1e-6
    # sqrt_ac^2 + sqrt_1mac^2 = 1 to fp32 rounding only, so the round trip holds to a few ulps of the values
    assert (gd.predict_noise_from_v(x_t, t, v) - eps).abs().max() < 1e-5
    assert (gd.predict_start_from_v(x_t, t, v) - x0).abs().max() < 1e-5


# ---- the weights -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('gamma', [1.0, 5.0, 20.0])
def test_weights_are_the_closed_forms(gamma):
    from video_diffusion_nnx_amd.gaussian_diffusion import min_snr_weights
    ac = _ac()
    r = V.snr(ac)
    assert np.all(r > 0) and np.all(np.diff(r) < 0)
    w_e, w_v = min_snr_weights(T, 'pred_noise', gamma), min_snr_weights(T, 'pred_v', gamma)
    assert w_e.dtype == np.float64 and w_e.shape == (T,) and w_v.dtype == np.float64 and w_v.shape == (T,)
    assert np.array_equal(w_e, V.weights_eps(ac, gamma)) and np.array_equal(w_v, V.weights_v(ac, gamma))
    assert np.all(w_e > 0) and np.all(w_e <= 1.0) and np.all(w_v > 0) and np.all(w_v <= 1.0)
    assert np.all(w_e[r <= gamma] == 1.0) and np.all(w_e[r > gamma] < 1.0)          # 1 ... below the clamp
    assert np.abs(w_v - w_e * r / (r + 1.0)).max() <= 1e-15
    # where the clamp binds both are gamma over their own scale
    hi = r > gamma
    assert hi.any() and np.abs(w_e[hi] - gamma / r[hi]).max() <= 1e-15 and np.abs(w_v[hi] - gamma / (r[hi] + 1.0)).max() <= 1e-15


def test_weights_without_clamp_and_without_gamma():
    from video_diffusion_nnx_amd.gaussian_diffusion import min_snr_weights
    ac = _ac()
    r = V.snr(ac)
    big = 1e300                                                               # gamma -> infinity
    assert np.array_equal(min_snr_weights(T, 'pred_noise', big), np.ones(T))
    assert np.abs(min_snr_weights(T, 'pred_v', big) - r / (r + 1.0)).max() <= 1e-15
    assert np.abs(min_snr_weights(T, 'pred_v', big) - ac).max() <= 1e-15      # SNR / (SNR + 1) = ac
    assert min_snr_weights(T, 'pred_v', None) is None and min_snr_weights(T, 'pred_noise', None) is None


# ---- the chain -------------------------------------------------------------------------------------------------------------------------------

def _gaussian_chains(timesteps, steps, m=0.3, sd=0.5, n=4096):
    """(chain driven by the exact eps, chain driven by the exact v, sqrt(ac) of the first level) for data x0 ~ N(m, sd^2) per element,
    where E[eps | x_t] and E[x0 | x_t], and with them the exact v, are closed forms."""
    from video_diffusion_nnx_amd.gaussian_diffusion import ddim_time_sequence, make_tables
    ac = make_tables(timesteps)['alphas_cumprod'].astype(np.float64)
    seq = [int(t) for t in ddim_time_sequence(timesteps, steps)[:-1]]
    assert len(seq) == steps and seq[0] == timesteps - 1

    def exact(x, t):
        a, s = V.coefs(ac[t])
        var = a * a * sd * sd + s * s
        return s * (x - a * m) / var, m + a * sd * sd * (x - a * m) / var       # E[eps | x], E[x0 | x]

    def by_eps(x, t):
        return exact(x, t)[0]

    def by_v(x, t):
        a, s = V.coefs(ac[t])
        e, x0 = exact(x, t)
        return V.eps_from_v(a, s, x, V.v_target(a, s, x0, e))

    x_T = np.random.default_rng(0).standard_normal(n)
    return V.ddim_chain(x_T, ac, seq, by_eps), V.ddim_chain(x_T, ac, seq, by_v), float(np.sqrt(ac[seq[0]]))


def test_ddim_chain_by_the_exact_v_is_the_chain_by_the_exact_eps():
    """Ten DDIM steps driven by eps_from_v(exact v) end where the ten driven by the exact eps end, to 1e-12.

    The chain is the ten levels of the project's ten-level cosine schedule.  Which schedule matters: the two drivers hand the chain
    eps values that differ by a rounding (about 2^-52 |eps|), and the DDIM step's x0 = (x_t - s eps) / a multiplies that by
    1 / a = 1 / sqrt(ac) of the level -- the ill conditioning of eps-prediction that v-prediction is there to avoid.  With ten levels
    the first one has sqrt(ac) = 1.6e-3 and the chains agree to 2e-14.  Over the T = 1000 tables the first level has sqrt(ac) = 1.6e-5
    (the last beta is clipped at 0.9999) and a ten-step chain from it agrees to 3.8e-12 only: that is the float64 accuracy of the
    eps-driven chain itself, not a property of v; the figure is printed below and held against 1e-12 / the ratio of the two sqrt(ac)."""
    one, two, a10 = _gaussian_chains(10, 10)
    err = np.abs(one - two).max()
    print(f'T = 10: sqrt(ac) of the first level = {a10:.3e}, max |chain(v) - chain(eps)| = {err:.3e}')
    assert err <= 1e-12
    assert np.isfinite(one).all() and abs(one.mean() - 0.3) < 0.1             # (a ten-step chain: near the data's mean, no more is claimed)
    big1, big2, a1000 = _gaussian_chains(1000, 10)
    err1000 = np.abs(big1 - big2).max()
    print(f'T = 1000: sqrt(ac) of the first level = {a1000:.3e}, max |chain(v) - chain(eps)| = {err1000:.3e}')
    assert err1000 <= 1e-12 * a10 / a1000


# ---- the Python surface on a CPU handle --------------------------------------------------------------------------------------------------------

def _cpu_unet(**kw):
    from video_diffusion_nnx_amd.unet3d import Unet3D
    return Unet3D(rngs=0, mode='f32', dim=16, channels=kw.pop('channels', 1), dim_mults=(1, 2), device='cpu', **kw)


KW = dict(image_size=8, num_frames=4, channels=1, timesteps=10)


def test_a_plain_instance_has_no_new_attribute():
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    for kw in ({}, dict(objective='pred_noise'), dict(min_snr_gamma=None), dict(objective='pred_noise', min_snr_gamma=None)):
        gd = GaussianDiffusion(_cpu_unet(), **kw, **KW)
        assert sorted(vars(gd)) == sorted(PARENT_ATTRIBUTES), kw
        assert gd.objective == 'pred_noise' and gd.min_snr_gamma is None and gd.loss_weights is None
    on = GaussianDiffusion(_cpu_unet(), objective='pred_v', **KW)
    assert sorted(vars(on)) == sorted(PARENT_ATTRIBUTES + ['objective']) and on.loss_weights is None
    both = GaussianDiffusion(_cpu_unet(), objective='pred_v', min_snr_gamma=5, **KW)
    assert sorted(vars(both)) == sorted(PARENT_ATTRIBUTES + ['objective', 'min_snr_gamma', '_loss_w'])
    assert both.min_snr_gamma == 5.0 and both.loss_weights.dtype == torch.float64 and tuple(both.loss_weights.shape) == (10,)
    eps_w = GaussianDiffusion(_cpu_unet(), min_snr_gamma=5.0, **KW)
    assert sorted(vars(eps_w)) == sorted(PARENT_ATTRIBUTES + ['min_snr_gamma', '_loss_w']) and eps_w.objective == 'pred_noise'
    from video_diffusion_nnx_amd.gaussian_diffusion import make_tables
    ac = make_tables(10)['alphas_cumprod'].astype(np.float64)
    assert np.array_equal(both.loss_weights.numpy(), V.weights_v(ac, 5.0)) and np.array_equal(eps_w.loss_weights.numpy(), V.weights_eps(ac, 5.0))


def test_constructor_validation_and_refusals():
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion, check_min_snr_gamma, check_objective
    for bad in ('pred_x0', 'v', '', None, 1, True, ['pred_v']):
        with pytest.raises(ValueError, match="objective must be 'pred_noise' or 'pred_v'"):
            GaussianDiffusion(_cpu_unet(), objective=bad, **KW)
    for bad in (0, 0.0, -1.0, float('nan'), float('inf'), float('-inf'), True, False, '5', [5.0]):
        with pytest.raises(ValueError, match='min_snr_gamma must be None or a finite number > 0'):
            GaussianDiffusion(_cpu_unet(), min_snr_gamma=bad, **KW)
    assert check_min_snr_gamma(np.float32(0.5)) == 0.5 and check_min_snr_gamma(5) == 5.0 and check_min_snr_gamma(None) is None
    assert check_objective('pred_v') == 'pred_v'
    # at construction: learned variances
    with pytest.raises(ValueError, match="objective='pred_v' does not support learned_variance yet \\(a follow-up; DESIGN.md 9\\)"):
        GaussianDiffusion(_cpu_unet(out_dim=2), objective='pred_v', learned_variance=True, **KW)
    with pytest.raises(ValueError, match='min_snr_gamma does not support learned_variance yet \\(a follow-up; DESIGN.md 9\\)'):
        GaussianDiffusion(_cpu_unet(out_dim=2), min_snr_gamma=5.0, learned_variance=True, **KW)
    assert GaussianDiffusion(_cpu_unet(out_dim=2), objective='pred_noise', learned_variance=True, **KW).learned_variance
    # in training, before any device work: the masked loss, for pred_v and for the weights
    x, t = torch.rand(2, 1, 4, 8, 8), torch.tensor([1, 2])
    mask = torch.tensor([1, 0, 0, 0], dtype=torch.uint8)
    with launches() as seen:
        for kw in (dict(objective='pred_v'), dict(min_snr_gamma=5.0), dict(objective='pred_v', min_snr_gamma=5.0)):
            gd = GaussianDiffusion(_cpu_unet(), **kw, **KW)
            with pytest.raises(ValueError, match="objective='pred_v' / min_snr_gamma does not support frame_mask yet \\(a follow-up; DESIGN.md 9\\)"):
                gd.p_losses(x, t, 0, frame_mask=mask)
    assert seen == []


# ---- the C entries -----------------------------------------------------------------------------------------------------------------------------

ENTRIES = {'vdx_v_to_eps': 10, 'vdx_v_loss_scratch_doubles': 1, 'vdx_v_loss': 20, 'vdx_set_prediction': 5, 'vdx_get_prediction': 1}


def test_entries_exist_and_match_the_header():
    from video_diffusion_nnx_amd import _lib as L
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'vdx.h')).read()
    assert '/* v-prediction (EXTENSION' in hdr
    for name, nargs in ENTRIES.items():
        assert hasattr(L.lib, name), name                                    # exported
        fn = getattr(L, name)
        assert len(fn.argtypes) == nargs, name
        decl = hdr[max(hdr.find(f'\nint {name}('), hdr.find(f'\nsize_t {name}(')):]           # (the declaration, not the prose)
        assert decl.startswith('\n'), name
        assert decl[:decl.index(');')].count(',') + 1 == nargs, name
    assert L.vdx_v_loss_scratch_doubles(0) == 0 and L.vdx_v_loss_scratch_doubles(3) == 3 * L.vdx_v_loss_scratch_doubles(1) > 0


def test_set_prediction_on_a_cpu_handle():
    from video_diffusion_nnx_amd import _lib as L
    h = _cpu_unet().handle(4, 8).ptr
    assert L.vdx_get_prediction(h) == 0 and L.vdx_get_prediction(None) == 0
    for args in ((2, BUF, BUF, 10), (-1, BUF, BUF, 10), (1, 0, BUF, 10), (1, BUF, 0, 10), (1, BUF, BUF, 0), (1, BUF, BUF, -3)):
        assert L.vdx_set_prediction(h, *args) == INVALID, args
        assert L.vdx_last_error().decode().startswith('set_prediction: ')
        assert L.vdx_get_prediction(h) == 0
    assert L.vdx_set_prediction(None, 0, 0, 0, 0) == INVALID
    assert L.vdx_set_prediction(h, 0, 0, 0, 0) == 0 and L.vdx_get_prediction(h) == 0
    assert L.vdx_set_prediction(h, 1, BUF, BUF + 4000, 10) == 0 and L.vdx_get_prediction(h) == 1       # (pointers are kept, not read)
    assert L.vdx_set_prediction(h, 0, BUF, BUF, 10) == 0 and L.vdx_get_prediction(h) == 0               # kind 0 is always accepted


TO_EPS = dict(out=BUF, x=BUF, t=BUF, sa=BUF, s1=BUF, T=10, rows=2, C=3, per=3 * 7, stream=0)
LOSS = dict(out=BUF, x0=BUF, noise=BUF, t=BUF, sa=BUF, s1=BUF, wtab=BUF, iw=BUF, T=10, kind=1, ps=2.0, sh=-1.0, l2=0, d_out=BUF, scratch=BUF,
            result=BUF, batch=2, C=3, fhw=7, stream=0)
REJECTS = [
    *[('v_to_eps', TO_EPS, {k: 0}, 'null tensor') for k in ('out', 'x', 't', 'sa', 's1')],
    *[('v_to_eps', TO_EPS, {k: 0}, 'must be >= 1') for k in ('T', 'rows', 'C', 'per')],
    ('v_to_eps', TO_EPS, dict(rows=-1), 'must be >= 1'), ('v_to_eps', TO_EPS, dict(per=22), 'multiple of channels'),
    *[('v_loss', LOSS, {k: 0}, 'null tensor') for k in ('out', 'noise', 'scratch', 'result')],
    *[('v_loss', LOSS, {k: 0}, 'kind 1 needs') for k in ('x0', 'sa', 's1')],
    ('v_loss', LOSS, dict(t=0), 'levels'), ('v_loss', LOSS, dict(T=0), 'levels'), ('v_loss', LOSS, dict(kind=0, t=0), 'levels'),
    ('v_loss', LOSS, dict(kind=2), 'kind 0'), ('v_loss', LOSS, dict(kind=-1), 'kind 0'),
    *[('v_loss', LOSS, {k: 0}, 'must be >= 1') for k in ('batch', 'C', 'fhw')],
    *[('v_loss', LOSS, {k: BUF + 4}, '8-byte') for k in ('wtab', 'iw', 'scratch', 'result')],
]
ENTRY_OF = {'v_to_eps': 'vdx_v_to_eps', 'v_loss': 'vdx_v_loss'}


@pytest.mark.parametrize('entry,base,change,word', REJECTS, ids=[f'{e}-{"-".join(c)}-{i}' for i, (e, _, c, _) in enumerate(REJECTS)])
def test_kernel_entries_reject_before_any_launch(entry, base, change, word):
    from video_diffusion_nnx_amd import _lib as L
    with launches() as seen:
        rc = getattr(L, ENTRY_OF[entry])(*dict(base, **change).values())
    msg = L.vdx_last_error().decode()
    assert rc == INVALID and msg.startswith(entry + ': ') and word in msg, (rc, msg)
    assert seen == []


def test_lv_loops_refuse_a_v_predicting_handle():
    """VDX_ERR_STATE by name before anything else is looked at (a CPU handle would be refused as such otherwise)."""
    from video_diffusion_nnx_amd import _lib as L
    h = _cpu_unet(out_dim=2).handle(4, 8).ptr
    assert L.vdx_set_prediction(h, 1, BUF, BUF, 10) == 0
    sample = dict(h=h, params=BUF, packed=BUF, img=BUF, out2=BUF, t_dev=BUF, step_dev=BUF, tab=BUF, seq=BUF, S=4, T=10, nsteps=1, cond=0, seed=3,
                  clip=1, ps=0.5, sh=0.5, ws=BUF, ws_bytes=1 << 20, batch=2, use_graph=0, stream=0)
    bound = dict(h=h, params=BUF, packed=BUF, x=BUF, xt=BUF, out2=BUF, t_dev=BUF, step_dev=BUF, tab=BUF, T=10, seq=BUF, S=4, nsteps=1, cond=0,
                 seed=3, clip=1, partial=BUF, out=BUF, ws=BUF, ws_bytes=1 << 20, batch=2, use_graph=0, stream=0)
    with launches() as seen:
        for fn, args, who in ((L.vdx_p_sample_loop_lv, sample, 'p_sample_loop_lv'), (L.vdx_vlb_loop_lv, bound, 'vlb_loop_lv')):
            rc, msg = fn(*args.values()), L.vdx_last_error().decode()
            assert rc == STATE and msg.startswith(who + ': ') and 'v-prediction' in msg, (rc, msg)
        assert L.vdx_set_prediction(h, 0, 0, 0, 0) == 0
        for fn, args, who in ((L.vdx_p_sample_loop_lv, sample, 'p_sample_loop_lv'), (L.vdx_vlb_loop_lv, bound, 'vlb_loop_lv')):
            rc, msg = fn(*args.values()), L.vdx_last_error().decode()
            assert rc == STATE and 'without a GPU' in msg, (rc, msg)          # (what a CPU handle was refused for before)
    assert seen == []


# ---- YAML and command line ---------------------------------------------------------------------------------------------------------------------

def test_yaml_keys_and_flags(tmp_path):
    import yaml
    import evaluate
    import sample
    import train
    config = os.path.join(os.path.dirname(sample.__file__), 'configs', 'config_v1_0.yaml')
    cfg = yaml.safe_load(open(config))
    cfg['unet'].update(dim=16, dim_mults=[1, 2])
    import video_diffusion_nnx_amd.unet3d as U
    real = U.Unet3D

    class CpuUnet(real):
        def __init__(self, *a, **k):
            super().__init__(*a, device='cpu', **k)

    U.Unet3D = CpuUnet
    try:
        gd = sample.build_models(cfg, 'f32')[1]
        assert gd.objective == 'pred_noise' and gd.min_snr_gamma is None                      # absent keys mean off
        assert not {'objective', 'min_snr_gamma', '_loss_w'} & set(vars(gd))
        cfg['diffusion']['objective'] = 'pred_v'
        gd = sample.build_models(cfg, 'f32')[1]
        assert gd.objective == 'pred_v' and gd.loss_weights is None
        cfg['diffusion']['min_snr_gamma'] = 5
        gd = sample.build_models(cfg, 'f32')[1]
        assert gd.objective == 'pred_v' and gd.min_snr_gamma == 5.0 and gd.loss_weights is not None
        assert sample.build_models(cfg, 'f32', objective='pred_noise')[1].objective == 'pred_noise'   # the flag overrides the key
        assert sample.build_models(cfg, 'f32', min_snr_gamma=2.0)[1].min_snr_gamma == 2.0
        del cfg['diffusion']['objective'], cfg['diffusion']['min_snr_gamma']
        assert sample.build_models(cfg, 'f32', objective='pred_v', min_snr_gamma=3.0)[1].min_snr_gamma == 3.0
        for key, bad, word in (('objective', 'pred_x0', 'objective must be'), ('min_snr_gamma', -1.0, 'min_snr_gamma must be'),
                               ('min_snr_gamma', True, 'min_snr_gamma must be')):
            cfg['diffusion'][key] = bad
            with pytest.raises(ValueError, match=word):
                sample.build_models(cfg, 'f32')
            del cfg['diffusion'][key]
        cfg['diffusion'].update(objective='pred_v', learned_variance=True)
        with pytest.raises(ValueError, match='does not support learned_variance yet'):
            sample.build_models(cfg, 'f32')
        # ... which the command-line tools report through their parsers
        path = tmp_path / 'lv.yaml'
        path.write_text(yaml.safe_dump(cfg))
        with pytest.raises(SystemExit):
            sample.main(['--config', str(path), '--random-init', '--mode', 'f32', '--output-path', str(tmp_path)])
        with pytest.raises(SystemExit):
            train.main(['--config', str(path), '--mode', 'f32'])
    finally:
        U.Unet3D = real
    a = sample.build_parser().parse_args(['--random-init', '--objective', 'pred_v'])
    assert a.objective == 'pred_v' and sample.build_parser().parse_args(['--random-init']).objective is None
    flags = dict(train.FLAGS)
    assert flags['--objective']['choices'] == ('pred_noise', 'pred_v') and flags['--objective']['default'] is None
    assert flags['--min_snr_gamma']['type'] is float and flags['--min_snr_gamma']['default'] is None
    assert '--objective' not in dict(evaluate.FLAGS) and '--min_snr_gamma' not in dict(sample.FLAGS)     # evaluation reads the YAML key
    with pytest.raises(SystemExit):
        sample.build_parser().parse_args(['--random-init', '--objective', 'pred_x0'])
    for bad in (['--objective', 'x0'], ['--min_snr_gamma', '0'], ['--min_snr_gamma', '-2'], ['--min_snr_gamma', 'nan'], ['--min_snr_gamma', 'inf']):
        with pytest.raises(SystemExit):
            train.main(['--config', config] + bad)
    for doc in (sample.__doc__, train.__doc__, sample.build_models.__doc__, evaluate.__doc__):
        assert 'pred_v' in doc
    assert 'min_snr_gamma' in train.__doc__ and 'min_snr_gamma' in sample.build_models.__doc__
    assert 'not stored in checkpoints' in flags['--objective']['help'] and 'Checkpoints do not store them' in sample.build_models.__doc__
