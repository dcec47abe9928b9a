"""The mixed noise prior on the host (no GPU): the weights, the statistics of the restated stream tests/_mixnoise_ref.py, the posterior
algebra that says why the ancestral step needs correlated z, and the plumbing -- the C entries and their refusals, constructor rules, the
refusals before any device work on a CPU handle, the YAML key and the command-line flags, and that alpha = 0 is the diffusion it was."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mixnoise_ref as M          # noqa: E402
from _launch_hook import launches          # noqa: E402
from test_host_superres import PARENT_ATTRIBUTES          # noqa: E402  (the instance attributes of a plain diffusion)

INVALID, STATE = -1, -4
BUF = 1 << 20
ALPHAS = (0.5, 1.0, 2.0)


# ---- the weights ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('alpha', ALPHAS + (0.0, 1e-3, 37.5, 1e30))
def test_mixed_noise_coef(alpha):
    from video_diffusion_nnx_amd.gaussian_diffusion import mixed_noise_coef
    a, b = mixed_noise_coef(alpha)
    assert isinstance(a, float) and isinstance(b, float)
    assert a == float(np.float32(a)) and b == float(np.float32(b))           # fp32 values
    a64, b64 = M.coef64(alpha)
    assert a == float(np.float32(a64)) and b == float(np.float32(b64))       # double, rounded once
    assert abs(a * a + b * b - 1.0) <= 2.0 ** -23                            # each weight is off by at most 2^-25 relative: one fp32 rounding
    assert abs(a * a - M.rho(alpha)) <= 2.0 ** -23
    if alpha == 0.0:
        assert (a, b) == (0.0, 1.0)


@pytest.mark.parametrize('alpha', ALPHAS)
def test_frame_noise_corr(alpha):
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    gd = GaussianDiffusion(_cpu_unet(), frame_noise_alpha=alpha, **KW)
    assert gd.frame_noise_alpha == alpha
    assert abs(gd.frame_noise_corr - {0.5: 0.2, 1.0: 0.5, 2.0: 0.8}[alpha]) < 1e-15
    assert GaussianDiffusion(_cpu_unet(), **KW).frame_noise_corr == 0.0


# ---- the statistics of the reference ---------------------------------------------------------------------------------------------------------

STAT_SHAPE = (2, 2, 4, 32, 32)
STREAMS = ((7, 0), (7, 3), (0x1234567890ABCDEF, 1))


@pytest.mark.parametrize('seed,draw', STREAMS, ids=[f'{s:x}-{d}' for s, d in STREAMS])
@pytest.mark.parametrize('alpha', ALPHAS)
def test_reference_frame_correlation(alpha, seed, draw):
    """Every frame pair's sample correlation over the 2 * 2 * 32 * 32 = 4096 (b, c, pixel) positions lies within 4 standard errors of
    rho, SE = (1 - rho^2) / sqrt(4096); each element is N(0, 1).  (Worst case of the nine streams: 2.61 SE.)"""
    z = M.mixed_randn(STAT_SHAPE, seed, draw, alpha)
    assert z.dtype == np.float32 and z.shape == STAT_SHAPE
    z64 = M.mixed_randn64(STAT_SHAPE, seed, draw, alpha)
    assert np.abs(z - z64).max() < 1e-5                                      # the two forms are one definition
    rho, Fr = M.rho(alpha), STAT_SHAPE[2]
    frames = np.moveaxis(z.astype(np.float64), 2, 0).reshape(Fr, -1)         # [F][4096]
    n = frames.shape[1]
    assert n == 4096
    se = (1.0 - rho * rho) / math.sqrt(n)
    worst = 0.0
    for i in range(Fr):
        for j in range(i + 1, Fr):
            r = np.corrcoef(frames[i], frames[j])[0, 1]
            worst = max(worst, abs(r - rho) / se)
    print(f'[alpha {alpha} seed {seed:x} draw {draw}] worst |r - rho| / SE = {worst:.2f}')
    assert worst < 4.0
    assert abs(frames.mean()) < 4.0 / math.sqrt(frames.size) and abs(frames.var() - 1.0) < 0.05


def test_reference_draws_do_not_collide():
    """The shared component is the stream's draw DRAW_SHARED + d of a [B,C,H,W] tensor; another draw moves both components."""
    shape = (2, 1, 3, 3, 3)
    s0, e0 = M.components(shape, 7, 0)
    s1, e1 = M.components(shape, 7, 1)
    assert s0.shape == (2, 1, 1, 3, 3) and e0.shape == shape
    from oracle import philox_ref
    assert np.array_equal(e0.reshape(-1), philox_ref.randn(54, 7, 0))
    assert np.array_equal(s0.reshape(-1), philox_ref.randn(18, 7, (1 << 60) + 0))
    assert not np.array_equal(s0, s1) and not np.array_equal(e0, e1)
    assert M.DRAW_SHARED == 1 << 60 and M.DRAW_SHARED not in (1 << 61, 1 << 62, 1 << 63)
    # alpha = 0 is randn itself
    assert np.array_equal(M.mixed_randn(shape, 7, 0, 0.0), e0)


# ---- the posterior algebra -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('alpha', ALPHAS)
@pytest.mark.parametrize('T', [10, 1000])
def test_ancestral_step_needs_correlated_z(T, alpha):
    """x_t ~ N(0, (1 - ac_t) Sigma) with x0 = 0 and the exact posterior mean: z ~ N(0, Sigma) gives Cov(x_{t-1}) = (1 - ac_{t-1}) Sigma
    to rounding; z ~ N(0, I) leaves a cross-frame error of exactly beta~_t a^2."""
    Fr = 4
    sigma = M.frame_covariance(Fr, alpha)
    a, _ = M.coef64(alpha)
    off = ~np.eye(Fr, dtype=bool)
    for t in (1, T // 2, T - 1):
        _, s = M.posterior_step_covariance(T, t, sigma, sigma)
        ac, ac_prev, pv = s['alphas_cumprod'][t], s['alphas_cumprod'][t - 1], s['posterior_variance'][t]
        good, _ = M.posterior_step_covariance(T, t, (1.0 - ac) * sigma, sigma)
        want = (1.0 - ac_prev) * sigma
        assert np.abs(good - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (t, good, want)
        iid, _ = M.posterior_step_covariance(T, t, (1.0 - ac) * sigma, np.eye(Fr))
        err = iid - want
        assert np.abs(err[off] + pv * a * a).max() <= 1e-12, (t, err)          # every frame pair: - beta~_t a^2
        assert pv * a * a > 1e-9                                              # (and that is not nothing)


# ---- the Python surface on a CPU handle ---------------------------------------------------------------------------------------------------

def _cpu_unet(**kw):
    from video_diffusion_nnx_amd.unet3d import Unet3D
    return Unet3D(rngs=0, mode='f32', dim=16, channels=kw.pop('channels', 1), dim_mults=(1, 2), device='cpu', **kw)


KW = dict(image_size=8, num_frames=4, channels=1, timesteps=10)


def test_alpha_zero_is_the_diffusion_it_was():
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    for kw in ({}, dict(frame_noise_alpha=0.0), dict(frame_noise_alpha=0)):
        gd = GaussianDiffusion(_cpu_unet(), **kw, **KW)
        assert sorted(vars(gd)) == sorted(PARENT_ATTRIBUTES), kw
        assert gd.frame_noise_alpha == 0.0 and gd.frame_noise_corr == 0.0
    on = GaussianDiffusion(_cpu_unet(), frame_noise_alpha=1.0, **KW)
    assert sorted(vars(on)) == sorted(PARENT_ATTRIBUTES + ['frame_noise_alpha', '_mix'])
    assert on._mix == (float(np.float32(math.sqrt(0.5))),) * 2


def test_constructor_validation_and_the_five_refusals():
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion, check_frame_noise_alpha, mixed_noise_coef
    for bad in (-1.0, -1e-9, float('nan'), float('inf'), float('-inf'), True, False, '1', None, [1.0]):
        with pytest.raises(ValueError, match='frame_noise_alpha must be a finite number >= 0'):
            GaussianDiffusion(_cpu_unet(), frame_noise_alpha=bad, **KW)
        with pytest.raises(ValueError, match='frame_noise_alpha'):
            mixed_noise_coef(bad)
    assert check_frame_noise_alpha(np.float32(0.5)) == 0.5 and check_frame_noise_alpha(2) == 2.0
    # at construction: learned variances and super-resolution
    with pytest.raises(ValueError, match='frame_noise_alpha does not support learned_variance yet \\(a follow-up'):
        GaussianDiffusion(_cpu_unet(out_dim=2), frame_noise_alpha=1.0, learned_variance=True, **KW)
    with pytest.raises(ValueError, match='frame_noise_alpha does not support lowres_cond yet \\(a follow-up'):
        GaussianDiffusion(_cpu_unet(channels=2, out_dim=1), frame_noise_alpha=1.0, lowres_cond=(2, 2), **KW)
    # ... which alpha = 0 leaves alone
    assert GaussianDiffusion(_cpu_unet(out_dim=2), frame_noise_alpha=0.0, learned_variance=True, **KW).learned_variance
    assert GaussianDiffusion(_cpu_unet(channels=2, out_dim=1), frame_noise_alpha=0.0, lowres_cond=(2, 2), **KW).lowres_cond == (2, 2)
    # at the call, before any device work (a CPU handle would fail loudly otherwise)
    gd = GaussianDiffusion(_cpu_unet(), frame_noise_alpha=1.0, **KW)
    x = torch.rand(1, 1, 4, 8, 8)
    calls = {'calc_bpd_loop': lambda: gd.calc_bpd_loop(x, 0),
             'inpaint': lambda: gd.inpaint(0, x, torch.tensor([1, 0, 0, 0], dtype=torch.uint8)),
             'extend': lambda: gd.extend(0, x, 2)}
    with launches() as seen:
        for word, fn in calls.items():
            with pytest.raises(ValueError, match=f'frame_noise_alpha does not support {word} yet \\(a follow-up'):
                fn()
        with pytest.raises(ValueError, match='defined over \\[B, C, F, H, W\\]'):
            gd.noise((4, 4), 0)
    assert seen == []


# ---- the C entries ------------------------------------------------------------------------------------------------------------------------

ENTRIES = {'vdx_randn_mixed': 11, 'vdx_p_sample_step_mixed': 18, 'vdx_p_sample_loop_mixed': 25}


def test_entries_exist_and_match_the_header():
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd import gaussian_diffusion as G
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'vdx.h')).read()
    assert '#define VDX_DRAW_SHARED (1ull << 60)' in hdr and L.DRAW_SHARED == 1 << 60
    for name, nargs in ENTRIES.items():
        assert hasattr(L.lib, name), name                                    # exported
        fn = getattr(L, name)
        assert len(fn.argtypes) == nargs, name
        decl = hdr[hdr.index(f'int {name}('):]
        assert decl[:decl.index(');')].count(',') + 1 == nargs, name
    # the step: vdx_p_sample_step's arguments with (frames, a, b) where noise stands; the loop: the guided loop's plus (a, b)
    step, mixed = list(G.vdx_p_sample_step.argtypes), list(L.vdx_p_sample_step_mixed.argtypes)
    assert mixed[:6] == step[:6] and mixed[9:] == step[7:] and mixed[6:9] == [L.c_int, L.c_float, L.c_float]
    guided, loop = list(L.vdx_p_sample_loop_guided.argtypes), list(L.vdx_p_sample_loop_mixed.argtypes)
    assert loop[:18] == guided[:18] and loop[18:20] == [L.c_float, L.c_float] and loop[20:] == guided[18:]


A, B_ = float(np.float32(0.6)), float(np.float32(0.8))
RANDN = dict(out=BUF, batch=2, C=3, F=4, hw=9, a=A, b=B_, seed=1, draw=0, dev=0, stream=0)
STEP = dict(x=BUF, eps=BUF, out=BUF, t=BUF, tab=BUF, T=10, F=4, a=A, b=B_, seed=1, off=0, dev=0, thres=0, clip=1, batch=2, C=3, per=3 * 4 * 16, stream=0)
WEIGHTS = [dict(a=-A), dict(b=-B_), dict(a=float('nan')), dict(b=float('nan')), dict(a=float('inf')), dict(b=float('-inf')),
           dict(a=0.6, b=0.81), dict(a=0.0, b=0.0), dict(a=1.0, b=1.0), dict(a=0.6, b=0.7999)]
REJECTS = [
    ('randn_mixed', RANDN, dict(out=0), 'null out'), ('randn_mixed', RANDN, dict(batch=0), 'must be >= 1'),
    ('randn_mixed', RANDN, dict(C=0), 'must be >= 1'), ('randn_mixed', RANDN, dict(F=0), 'must be >= 1'), ('randn_mixed', RANDN, dict(hw=0), 'must be >= 1'),
    ('randn_mixed', RANDN, dict(batch=-3), 'must be >= 1'), ('randn_mixed', RANDN, dict(draw=1 << 60), 'below 2^60'),
    ('randn_mixed', RANDN, dict(draw=(1 << 62) + 5), 'below 2^60'), ('randn_mixed', RANDN, dict(out=BUF + 4), '16-byte'),
    *[('randn_mixed', RANDN, w, 'a^2 + b^2 = 1') for w in WEIGHTS],
    *[('p_sample_mixed', STEP, {k: 0}, 'bad argument') for k in ('x', 'eps', 'out', 't', 'tab', 'T', 'F', 'batch', 'C', 'per')],
    ('p_sample_mixed', STEP, dict(per=3 * 4 * 16 + 4), 'multiple of channels * frames'), ('p_sample_mixed', STEP, dict(F=5), 'multiple of channels * frames'),
    ('p_sample_mixed', STEP, dict(C=1, F=2, per=6), 'per_sample % 4 == 0'), ('p_sample_mixed', STEP, dict(off=1 << 60), 'below 2^60'),
    ('p_sample_mixed', STEP, dict(x=BUF + 8), '16-byte'), ('p_sample_mixed', STEP, dict(out=BUF + 4), '16-byte'),
    *[('p_sample_mixed', STEP, w, 'a^2 + b^2 = 1') for w in WEIGHTS],
]
ENTRY_OF = {'randn_mixed': 'vdx_randn_mixed', 'p_sample_mixed': 'vdx_p_sample_step_mixed'}


@pytest.mark.parametrize('entry,base,change,word', REJECTS, ids=[f'{e}-{"-".join(c)}-{i}' for i, (e, _, c, _) in enumerate(REJECTS)])
def test_kernel_entries_reject_before_any_launch(entry, base, change, word):
    from video_diffusion_nnx_amd import _lib as L
    with launches() as seen:
        rc = getattr(L, ENTRY_OF[entry])(*dict(base, **change).values())
    msg = L.vdx_last_error().decode()
    assert rc == INVALID and msg.startswith(entry + ': ') and word in msg, (rc, msg)
    assert seen == []


LOOP = dict(h=None, params=BUF, packed=BUF, img=BUF, eps=BUF, t_dev=BUF, step_dev=BUF, tab=BUF, T=10, nsteps=1, cond=0, seed=3, clip=1, perc=0.0,
            thres=0, cond_scale=1.0, rescale=0.0, scratch=0, a=A, b=B_, ws=BUF, ws_bytes=1 << 20, batch=2, use_graph=0, stream=0)


def test_loop_rejects_on_a_cpu_handle():
    """The weights first, then the shared builder's null rules under the loop's own name, the guided ones when cond_scale != 1 and a
    scratch make it the guided loop; a CPU handle is VDX_ERR_STATE; nothing is launched."""
    from video_diffusion_nnx_amd import _lib as L
    base = dict(LOOP, h=_cpu_unet().handle(4, 8).ptr)
    fn = L.vdx_p_sample_loop_mixed
    with launches() as seen:
        call = lambda **ch: (fn(*dict(base, **ch).values()), L.vdx_last_error().decode())
        for w in WEIGHTS:
            rc, msg = call(**w)
            assert rc == INVALID and msg.startswith('p_sample_loop_mixed: ') and 'a^2 + b^2 = 1' in msg, (w, rc, msg)
        for n in ('h', 'params', 'packed', 'img', 'eps', 't_dev', 'step_dev', 'tab', 'ws'):
            rc, msg = call(**{n: 0})
            assert rc == INVALID and msg.startswith('p_sample_loop_mixed: ') and 'null' in msg, (n, rc, msg)
        # cond_scale != 1 with a scratch: the guided loop, which needs cond; without a scratch, or at scale 1, the plain one, which
        # does not (the null rules come before the handle's device state is looked at, the other rules after it, as in every loop)
        rc, msg = call(cond_scale=2.0, scratch=BUF)
        assert rc == INVALID and msg.startswith('p_sample_loop_mixed: ') and 'null' in msg, (rc, msg)
        for plain in (dict(cond_scale=2.0, scratch=0), dict(cond_scale=1.0, scratch=BUF), dict(cond_scale=2.0, scratch=BUF, cond=BUF)):
            rc, msg = call(**plain)
            assert rc == STATE and msg.startswith('p_sample_loop_mixed: ') and 'without a GPU' in msg, (plain, rc, msg)
        rc, msg = call()
        assert rc == STATE and msg.startswith('p_sample_loop_mixed: ') and 'without a GPU' in msg, (rc, msg)
    assert seen == []


# ---- YAML and command line ------------------------------------------------------------------------------------------------------------------

def test_yaml_key_and_flags(tmp_path):
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
        assert gd.frame_noise_alpha == 0.0 and 'frame_noise_alpha' not in vars(gd)            # an absent key means off
        cfg['diffusion']['frame_noise_alpha'] = 0
        assert 'frame_noise_alpha' not in vars(sample.build_models(cfg, 'f32')[1])
        cfg['diffusion']['frame_noise_alpha'] = 2.0
        gd = sample.build_models(cfg, 'f32')[1]
        assert gd.frame_noise_alpha == 2.0 and abs(gd.frame_noise_corr - 0.8) < 1e-15
        assert sample.build_models(cfg, 'f32', frame_noise_alpha=0.5)[1].frame_noise_alpha == 0.5       # the flag overrides the key
        assert sample.build_models(cfg, 'f32', frame_noise_alpha=0.0)[1].frame_noise_alpha == 0.0       # ... also to switch it off
        for bad in (-1.0, float('nan'), True):
            cfg['diffusion']['frame_noise_alpha'] = bad
            with pytest.raises(ValueError, match='frame_noise_alpha must be'):
                sample.build_models(cfg, 'f32')
        cfg['diffusion']['frame_noise_alpha'] = 1.0
        cfg['diffusion']['learned_variance'] = True
        with pytest.raises(ValueError, match='does not support learned_variance yet'):
            sample.build_models(cfg, 'f32')
        del cfg['diffusion']['learned_variance']
        cfg['diffusion']['lowres_cond'] = dict(temporal=2, spatial=2)
        with pytest.raises(ValueError, match='does not support lowres_cond yet'):
            sample.build_models(cfg, 'f32')
        del cfg['diffusion']['lowres_cond']
        # evaluate.py reports the refusal of calc_bpd_loop through the parser, before it looks at the data
        path = tmp_path / 'mixed.yaml'
        path.write_text(yaml.safe_dump(cfg))
        with pytest.raises(SystemExit):
            evaluate.main(['--config', str(path), '--random-init', '--mode', 'f32', '--dataset-path', 'synthetic:2', '--output', str(tmp_path / 'o.json')])
    finally:
        U.Unet3D = real
    a = sample.build_parser().parse_args(['--random-init', '--frame-noise-alpha', '1.5'])
    assert a.frame_noise_alpha == 1.5 and sample.build_parser().parse_args(['--random-init']).frame_noise_alpha is None
    flags = dict(train.FLAGS)
    assert flags['--frame_noise_alpha']['type'] is float and flags['--frame_noise_alpha']['default'] is None
    assert '--frame-noise-alpha' not in dict(evaluate.FLAGS)                 # evaluation takes the YAML key only, to refuse it
    for bad in (['--frame-noise-alpha', '-1'], ['--frame-noise-alpha', 'nan'], ['--frame-noise-alpha', '1', '--context', 'c.npy']):
        with pytest.raises(SystemExit):
            sample.main(['--random-init', '--output-path', str(tmp_path)] + bad)
    with pytest.raises(SystemExit):
        train.main(['--config', config, '--frame_noise_alpha', '-2'])
    for doc in (sample.__doc__, train.__doc__, sample.build_models.__doc__):
        assert 'frame_noise_alpha' in doc.replace('-', '_')
    assert 'not stored in checkpoints' in flags['--frame_noise_alpha']['help'] and 'Checkpoints do not store it' in sample.build_models.__doc__
