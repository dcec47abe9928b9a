"""Self-conditioning on the host (no GPU): the new C entries against the header and what they refuse on a CPU handle, the handle's
self-condition state and the loops that refuse it by name, the constructor rules and call-time refusals of
GaussianDiffusion(self_condition=True), that a plain diffusion gains no attribute, the coin's key and draw next to the unchanged key tree,
the restatement tests/_selfcond_ref.py against its own fp64 form, and the YAML keys and command-line flags."""
import itertools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _selfcond_ref as R          # noqa: E402
from _launch_hook import launches          # noqa: E402
from test_host_superres import DDIM_LOOP, DPM_LOOP, P_LOOP, PARENT_ATTRIBUTES          # noqa: E402

INVALID, STATE = -1, -4
BUF = 1 << 20


def _cpu_unet(**kw):
    from video_diffusion_nnx_amd.unet3d import Unet3D
    return Unet3D(rngs=0, mode='f32', dim=16, channels=kw.pop('channels', 1), dim_mults=(1, 2), device='cpu', **kw)


KW = dict(image_size=8, num_frames=4, channels=1, timesteps=10)
SHAPE = (2, 1, 4, 8, 8)


def _sc(**kw):
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    return GaussianDiffusion(_cpu_unet(channels=2, out_dim=1), self_condition=True, **dict(KW, **kw))


# ---- the C entries ----------------------------------------------------------------------------------------------------------------------------

ENTRIES = {'vdx_selfcond_x0': 13, 'vdx_set_self_condition': 4, 'vdx_get_self_condition': 1}


def test_entries_exist_and_match_the_header():
    from video_diffusion_nnx_amd import _lib as L
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'vdx.h')).read()
    assert '/* Self-conditioning (EXTENSION' in hdr
    for name, nargs in ENTRIES.items():
        assert hasattr(L.lib, name), name                                    # exported
        assert len(getattr(L, name).argtypes) == nargs, name
        decl = hdr[hdr.find(f'\nint {name}('):]                              # (the declaration, not the prose)
        assert decl.startswith('\n'), name
        assert decl[:decl.index(');')].count(',') + 1 == nargs, name


def test_set_self_condition_on_a_cpu_handle():
    from video_diffusion_nnx_amd import _lib as L
    unet = _cpu_unet(channels=2, out_dim=1)
    h = unet.handle(4, 8).ptr
    assert L.vdx_get_self_condition(h) == 0 and L.vdx_get_self_condition(None) == 0
    for args in ((2, BUF, 10), (-1, BUF, 10), (1, 0, 10), (1, BUF, 0), (1, BUF, -3)):
        assert L.vdx_set_self_condition(h, *args) == INVALID, args
        assert L.vdx_last_error().decode().startswith('set_self_condition: ')
        assert L.vdx_get_self_condition(h) == 0
    assert L.vdx_set_self_condition(None, 0, 0, 0) == INVALID
    assert L.vdx_set_self_condition(h, 0, 0, 0) == 0 and L.vdx_get_self_condition(h) == 0
    assert L.vdx_set_self_condition(h, 1, BUF, 10) == 0 and L.vdx_get_self_condition(h) == 1            # (the pointer is kept, not read)
    assert L.vdx_get_prediction(h) == 0                                                                 # (a state of its own)
    assert L.vdx_set_self_condition(h, 0, BUF, 10) == 0 and L.vdx_get_self_condition(h) == 0            # off is always accepted


X0 = dict(x=BUF, pitch=21, eps=BUF, t=BUF, tab=BUF, T=10, thres=0, clip=1, xin=BUF, batch=2, C=3, per=21, stream=0)
REJECTS = [
    *[(X0, {k: 0}, 'null tensor') for k in ('x', 'eps', 't', 'tab', 'xin')],
    *[(X0, {k: 0}, 'must be >= 1') for k in ('T', 'batch', 'C')],
    (X0, dict(per=0, pitch=0), 'must be >= 1'), (X0, dict(batch=-1), 'must be >= 1'), (X0, dict(per=22, pitch=22), 'multiple of channels'),
    (X0, dict(pitch=20), 'x_pitch'), (X0, dict(x=BUF + 2), '4-byte'), (X0, dict(xin=BUF + 1), '4-byte'),
]


@pytest.mark.parametrize('base,change,word', REJECTS, ids=[f'{"-".join(c)}-{i}' for i, (_, c, _) in enumerate(REJECTS)])
def test_selfcond_x0_rejects_before_any_launch(base, change, word):
    from video_diffusion_nnx_amd import _lib as L
    with launches() as seen:
        rc = L.vdx_selfcond_x0(*dict(base, **change).values())
    msg = L.vdx_last_error().decode()
    assert rc == INVALID and msg.startswith('selfcond_x0: ') and word in msg, (rc, msg)
    assert seen == []


def test_loops_refuse_by_name_while_the_state_is_on():
    """VDX_ERR_STATE by name before the handle's device state is looked at: every loop without xin, the learned-variance loop and both
    evaluation loops; the three loops over xin go on to what a CPU handle is refused for.  Off again: everything as before."""
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd import gaussian_diffusion as G
    nets = _cpu_unet(), _cpu_unet(channels=2, out_dim=1), _cpu_unet(out_dim=2)          # (kept alive: a handle belongs to its network)
    plain, sr, lv = (n.handle(4, 8).ptr for n in nets)
    drop = lambda d: {k: v for k, v in d.items() if k != 'xin'}
    sample_lv = dict(h=lv, params=BUF, packed=BUF, img=BUF, out2=BUF, t_dev=BUF, step_dev=BUF, tab=BUF, seq=BUF, S=4, T=10, nsteps=1, cond=0, seed=3,
                     clip=1, ps=0.5, sh=0.5, ws=BUF, ws_bytes=1 << 20, batch=2, use_graph=0, stream=0)
    bound = dict(h=plain, params=BUF, packed=BUF, x=BUF, xt=BUF, out2=BUF, t_dev=BUF, step_dev=BUF, tab=BUF, T=10, seq=BUF, S=4, nsteps=1, cond=0,
                 seed=3, clip=1, partial=BUF, out=BUF, ws=BUF, ws_bytes=1 << 20, batch=2, use_graph=0, stream=0)
    without_xin = ((G.vdx_p_sample_loop_dyn, dict(drop(P_LOOP), h=plain), 'p_sample_loop'), (G.vdx_ddim_sample_loop_dyn, dict(drop(DDIM_LOOP), h=plain), 'ddim_sample_loop'),
                   (G.vdx_dpm_sample_loop, dict(drop(DPM_LOOP), h=plain), 'dpm_sample_loop'), (L.vdx_p_sample_loop_lv, sample_lv, 'p_sample_loop_lv'),
                   (L.vdx_vlb_loop, bound, 'vlb_loop'), (L.vdx_vlb_loop_lv, dict(bound, h=lv), 'vlb_loop_lv'))
    with_xin = ((L.vdx_p_sample_loop_sr, dict(P_LOOP, h=sr)), (L.vdx_ddim_sample_loop_sr, dict(DDIM_LOOP, h=sr)), (L.vdx_dpm_sample_loop_sr, dict(DPM_LOOP, h=sr)))
    with launches() as seen:
        for h in (plain, sr, lv):
            assert L.vdx_set_self_condition(h, 1, BUF, 10) == 0
        for fn, args, who in without_xin:
            rc, msg = fn(*args.values()), L.vdx_last_error().decode()
            assert rc == STATE and msg.startswith(who) and 'self-conditioning (vdx_set_self_condition)' in msg, (who, rc, msg)
        for fn, args in with_xin:
            rc, msg = fn(*args.values()), L.vdx_last_error().decode()
            assert rc == STATE and 'without a GPU' in msg, (rc, msg)
        for h in (plain, sr, lv):
            assert L.vdx_set_self_condition(h, 0, 0, 0) == 0
        for fn, args, who in without_xin:
            rc, msg = fn(*args.values()), L.vdx_last_error().decode()
            assert rc == STATE and 'without a GPU' in msg, (who, rc, msg)      # (what a CPU handle was refused for before)
    assert seen == []


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------------

def test_a_plain_instance_has_no_new_attribute():
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    for kw in ({}, dict(self_condition=False)):
        gd = GaussianDiffusion(_cpu_unet(), **kw, **KW)
        assert sorted(vars(gd)) == sorted(PARENT_ATTRIBUTES), kw
        assert gd.self_condition is False
    on = _sc()
    assert sorted(vars(on)) == sorted(PARENT_ATTRIBUTES + ['self_condition']) and on.self_condition is True
    both = _sc(objective='pred_v', use_dynamic_thres=True)
    assert sorted(vars(both)) == sorted(PARENT_ATTRIBUTES + ['self_condition', 'objective'])


def test_constructor_rules():
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    for unet in (_cpu_unet(), _cpu_unet(channels=2, out_dim=2), _cpu_unet(channels=4, out_dim=1)):
        with pytest.raises(ValueError, match=r'self_condition needs a denoiser with channels == 2 \* channels = 2 and out_dim == channels = 1'):
            GaussianDiffusion(unet, self_condition=True, **KW)
    wide = lambda **k: _cpu_unet(channels=2, **dict(dict(out_dim=1), **k))
    with pytest.raises(ValueError, match=r'self_condition does not support lowres_cond yet \(a follow-up; DESIGN.md 9\)'):
        GaussianDiffusion(wide(), self_condition=True, lowres_cond=(2, 2), **KW)
    with pytest.raises(ValueError, match=r'self_condition does not support learned_variance yet \(a follow-up; DESIGN.md 9\)'):
        GaussianDiffusion(wide(out_dim=2), self_condition=True, learned_variance=True, **KW)
    with pytest.raises(ValueError, match=r'self_condition does not support frame_noise_alpha yet \(a follow-up; DESIGN.md 9\)'):
        GaussianDiffusion(wide(), self_condition=True, frame_noise_alpha=1.0, **KW)
    for bad in (1, 0, 'yes', None):
        with pytest.raises(ValueError, match='self_condition must be True or False'):
            GaussianDiffusion(wide(), self_condition=bad, **KW)
    assert GaussianDiffusion(wide(), self_condition=True, frame_noise_alpha=0.0, objective='pred_v', min_snr_gamma=5.0, **KW).self_condition


X, T_ = torch.rand(SHAPE), torch.tensor([1, 2])
MASK = torch.tensor([1, 0, 0, 0], dtype=torch.bool)
REFUSALS = [
    ('cond_scale', lambda gd: gd.sample(0, cond_scale=2.0)),
    ('cond_scale', lambda gd: gd.p_sample_loop(SHAPE, 0, cond_scale=2.0)),
    ('cond_scale', lambda gd: gd.ddim_sample_loop(SHAPE, 0, steps=2, cond_scale=2.0)),
    ('cond_scale', lambda gd: gd.dpm_sample_loop(SHAPE, 0, steps=2, cond_scale=2.0)),
    ('cond_scale', lambda gd: gd.p_sample(X, T_, 0, cond_scale=2.0)),
    ('cond_scale', lambda gd: gd.p_mean_variance(X, T_, True, cond_scale=2.0)),
    ('inpaint', lambda gd: gd.inpaint(0, X, MASK)),
    ('extend', lambda gd: gd.extend(0, X, 2)),
    ('upsample', lambda gd: gd.upsample(0, torch.rand(2, 1, 2, 4, 4))),
    ('calc_bpd_loop', lambda gd: gd.calc_bpd_loop(X, 0)),
    ('frame_mask', lambda gd: gd.p_losses(X, T_, 0, frame_mask=MASK)),
]


def test_call_time_refusals_by_name():
    gd = _sc()
    with launches() as seen:
        for keyword, call in REFUSALS:
            with pytest.raises(ValueError) as e:
                call(gd)
            assert str(e.value) == f'self_condition does not support {keyword} yet (a follow-up; DESIGN.md 9)', keyword
        with pytest.raises(ValueError, match='super-resolution diffusion'):
            gd.sample(0, lowres=torch.rand(2, 1, 2, 4, 4))
        with pytest.raises(ValueError, match='x_self_cond must have the shape of x'):
            gd.p_sample(X, T_, 0, x_self_cond=torch.zeros(2, 1, 4, 8, 4))
    assert seen == []
    # and a plain diffusion refuses the new arguments
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    plain = GaussianDiffusion(_cpu_unet(), **KW)
    for fn in (lambda: plain.p_sample(X, T_, 0, x_self_cond=X), lambda: plain.p_mean_variance(X, T_, True, x_self_cond=X),
               lambda: plain.self_cond_estimate(X, T_, X), lambda: plain.p_losses(X, T_, 0, self_cond=True)):
        with pytest.raises(ValueError, match='self-conditioned diffusion'):
            fn()
    assert plain._refuse('self_condition', cond_scale=2.0, inpaint=True) is None


def test_trainer_rules(tmp_path):
    from video_diffusion_nnx_amd.trainer import Trainer
    kw = dict(dataset_path='synthetic:4', train_batch_size=2, train_num_steps=1, results_folder=str(tmp_path / 'res'))
    assert Trainer.self_cond_prob == 0.5
    tr = Trainer(_sc(), str(tmp_path), **kw)
    assert 'self_cond_prob' not in vars(tr) and tr.last_self_cond is None

    class Bad(Trainer):
        self_cond_prob = 1.5

    with pytest.raises(ValueError, match=r'self_cond_prob must be in \[0, 1\]'):
        Bad(_sc(), str(tmp_path), **kw)

    class Framed(Trainer):
        frame_cond_max = 2

    with pytest.raises(ValueError, match=r'self_condition does not support frame_mask yet \(a follow-up; DESIGN.md 9\)'):
        Framed(_sc(), str(tmp_path), **kw)
    with launches() as seen:
        with pytest.raises(ValueError, match=r'self_condition does not support frame_mask yet \(a follow-up; DESIGN.md 9\)'):
            tr.train_step(torch.rand(SHAPE), 0, frame_mask=MASK)
        from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
        plain = Trainer(GaussianDiffusion(_cpu_unet(), **KW), str(tmp_path / 'p'), **kw)
        with pytest.raises(ValueError, match='self-conditioned diffusion'):
            plain.train_step(torch.rand(SHAPE), 0, self_cond=True)
    assert seen == []


# ---- keys and draws ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('seed', [0, 1, 2 ** 63 + 5])
def test_the_coin_has_a_key_of_its_own(seed):
    from video_diffusion_nnx_amd import train_step as S
    from video_diffusion_nnx_amd.gaussian_diffusion import self_cond_key, split_key
    child = lambda k, i: split_key(k, i)[-1]
    assert S.StepKeys._fields == ('t', 'noise', 'frame_cond', 'cond_drop', 'focus_present', 'lowres_aug')
    for rank, step, j in itertools.product((0, 3), (0, 1, 1000), (0, 1, 4)):
        micro = child(child(seed, rank + 1), step + 1)
        if j > 0:
            micro = child(micro, 3 + j)
        loss = child(micro, 3)
        keys = S.step_keys(seed, rank, step, j)
        # step_keys is what it was: restated from split_key alone
        assert keys == S.StepKeys(child(micro, 2), child(loss, 2), child(micro, 1), child(loss, 1), child(loss, 3), child(loss, 4))
        k = S.self_cond_key(seed, rank, step, j)
        assert k == child(loss, 5) == self_cond_key(loss) and k not in keys
        assert k == S.self_cond_key(seed, rank, step, j)                     # stable
        if j == 0:
            assert k == S.self_cond_key(seed, rank, step)


def test_the_draw():
    from video_diffusion_nnx_amd import train_step as S
    gen = lambda key: torch.Generator().manual_seed(key & 0x7FFFFFFFFFFFFFFF)
    coins = []
    for step in range(200):
        key0 = S.self_cond_key(7, 0, step)
        assert S.self_cond_draw(0.0, gen(key0)) is False and S.self_cond_draw(1.0, gen(key0)) is True
        c = S.self_cond_draw(0.5, gen(key0))
        # every rank draws under rank 0's key: rank 1 of the same step has the same coin whatever its own key is
        assert S.self_cond_key(7, 1, step) != key0 and S.self_cond_draw(0.5, gen(S.self_cond_key(7, 0, step))) is c
        coins.append(c)
    assert 60 <= sum(coins) <= 140                                           # (200 fair coins: 100 +- 5.7 sigma)
    for bad in (-0.1, 1.1, True, float('nan')):
        with pytest.raises(ValueError, match=r'self_cond_prob must be in \[0, 1\]'):
            S.self_cond_draw(bad)


def test_train_step_draws_under_rank_0s_key(tmp_path, monkeypatch):
    """forward_backward on 'rank 1' asks self_cond_draw for the coin with the generator of rank 0's key (everything behind it needs a GPU
    and is cut off here)."""
    from video_diffusion_nnx_amd import train_step as S
    from video_diffusion_nnx_amd.trainer import Trainer
    tr = Trainer(_sc(), str(tmp_path), rng_seed=7, dataset_path='synthetic:4', train_batch_size=2, train_num_steps=1, results_folder=str(tmp_path / 'res'))
    tr.rank = 1
    seen = []

    class Stop(Exception):
        pass

    def draw(p, generator=None):
        seen.append((p, generator.initial_seed()))
        raise Stop

    monkeypatch.setattr(S, 'self_cond_draw', draw)
    monkeypatch.setattr(tr.model, 'noise', lambda shape, key, draw=0, out=None: torch.zeros(shape))
    with pytest.raises(Stop):
        S.forward_backward(tr, torch.rand(SHAPE), 5, j=2)
    assert seen == [(0.5, S.self_cond_key(7, 0, 5, 2) & 0x7FFFFFFFFFFFFFFF)]
    assert tr.last_noise_key == S.step_keys(7, 1, 5, 2).noise               # (the other streams are rank 1's own)


# ---- the restatement --------------------------------------------------------------------------------------------------------------------------

def test_the_restatement_against_its_fp64_form():
    """fp32 against fp64 on the same inputs: three roundings of values up to |k_recip x| + |k_recipm1 eps| -- two products, half an ulp
    each, and the difference, half an ulp of a result no larger than their sum -- so 1.5 ulp of that sum, 2^-23 relative; the clip
    divides by s >= 1 and adds half an ulp of a value <= 1."""
    from video_diffusion_nnx_amd.gaussian_diffusion import make_tables
    tabs = make_tables(10)
    tables = torch.from_numpy(tabs['sqrt_recip_alphas_cumprod']), torch.from_numpy(tabs['sqrt_recipm1_alphas_cumprod'])
    tables = torch.stack(list(tables) + [torch.zeros(10)] * 3)
    g = torch.Generator().manual_seed(0)
    x, eps = torch.randn(3, 2, 2, 3, 5, generator=g), torch.randn(3, 2, 3, 5, 2, generator=g)
    t = torch.tensor([0, 4, 12])                                             # (12 reads level 9)
    s = torch.tensor([1.0, 1.5, 3.0])
    kr, km = tables[0][t.clamp(0, 9)].double(), tables[1][t.clamp(0, 9)].double()
    size = (kr.reshape(-1, 1, 1, 1, 1) * x.double()).abs() + (km.reshape(-1, 1, 1, 1, 1) * R.to_channel_first(eps).double()).abs()
    for clip, thres in ((False, None), (True, None), (True, s)):
        a = R.x0_estimate(x, eps, t, tables, clip=clip, thres=thres)
        b = R.x0_estimate(x, eps, t, tables, clip=clip, thres=thres, dtype=torch.float64)
        assert a.dtype == torch.float32 and b.dtype == torch.float64 and a.shape == x.shape
        assert ((a.double() - b).abs() <= 1.5 * 2.0 ** -23 * size + 2.0 ** -24).all()
        if clip:
            assert a.abs().max() <= 1.0 and (a.abs() == 1.0).any()
    assert torch.equal(R.x0_estimate(x[2:], eps[2:], torch.tensor([9]), tables), R.x0_estimate(x[2:], eps[2:], torch.tensor([12]), tables))


# ---- YAML and command line --------------------------------------------------------------------------------------------------------------------

def test_yaml_keys_and_flags(tmp_path):
    import yaml
    import evaluate
    import sample
    import train
    from video_diffusion_nnx_amd.trainer import Trainer
    config = os.path.join(os.path.dirname(sample.__file__), 'configs', 'config_v1_0.yaml')
    cfg = yaml.safe_load(open(config))
    cfg['unet'].update(dim=16, dim_mults=[1, 2])
    C = cfg['diffusion']['channels']
    import video_diffusion_nnx_amd.unet3d as U
    real = U.Unet3D

    class CpuUnet(real):
        def __init__(self, *a, **k):
            super().__init__(*a, device='cpu', **k)

    U.Unet3D = CpuUnet
    keep = Trainer.self_cond_prob
    try:
        unet, gd = sample.build_models(cfg, 'f32')
        assert gd.self_condition is False and 'self_condition' not in vars(gd) and unet.channels == C       # absent keys mean off
        cfg['diffusion']['self_condition'] = True
        unet, gd = sample.build_models(cfg, 'f32')
        assert gd.self_condition is True and (unet.channels, unet.out_dim) == (2 * C, C) and gd.channels == C
        cfg['diffusion']['self_condition'] = False
        assert sample.build_models(cfg, 'f32')[0].channels == C
        unet, gd = sample.build_models(cfg, 'f32', self_condition=True)                                      # the flag switches it on as well
        assert gd.self_condition is True and unet.channels == 2 * C
        del cfg['diffusion']['self_condition']
        for key, value in (('learned_variance', True), ('lowres_cond', dict(temporal=1, spatial=2)), ('frame_noise_alpha', 1.0)):
            cfg['diffusion'][key] = value
            with pytest.raises(ValueError, match=f'self_condition does not support {key} yet'):
                sample.build_models(cfg, 'f32', self_condition=True)
            del cfg['diffusion'][key]
        cfg['diffusion']['self_condition'] = 'yes'
        with pytest.raises(ValueError, match='self_condition must be True or False'):
            sample.build_models(cfg, 'f32')
        # the command-line tools report the rules through their parsers
        cfg['diffusion'].update(self_condition=True, learned_variance=True)
        path = tmp_path / 'lv.yaml'
        path.write_text(yaml.safe_dump(cfg))
        with pytest.raises(SystemExit):
            sample.main(['--config', str(path), '--random-init', '--mode', 'f32', '--output-path', str(tmp_path)])
        with pytest.raises(SystemExit):
            train.main(['--config', str(path), '--mode', 'f32'])
        del cfg['diffusion']['learned_variance']
        path = tmp_path / 'sc.yaml'
        path.write_text(yaml.safe_dump(cfg))
        with pytest.raises(SystemExit):                                      # evaluate.py refuses by name
            evaluate.main(['--config', str(path), '--random-init', '--mode', 'f32', '--dataset-path', 'synthetic:2', '--output', str(tmp_path / 'o.json')])
        for bad in (['--self_cond_prob', '1.5'], ['--self_cond_prob', '-0.1'], ['--frame_cond_max', '2']):
            with pytest.raises(SystemExit):
                train.main(['--config', str(path), '--mode', 'f32'] + bad)
        with pytest.raises(SystemExit):                                      # the probability without the switch
            train.main(['--config', config, '--mode', 'f32', '--self_cond_prob', '0.3'])
        assert Trainer.self_cond_prob == keep
    finally:
        U.Unet3D = real
        Trainer.self_cond_prob = keep
    a = sample.build_parser().parse_args(['--random-init', '--self-condition'])
    assert a.self_condition is True and sample.build_parser().parse_args(['--random-init']).self_condition is False
    for clash in (['--context', 'c.npy'], ['--lowres-path', 'x.npy'], ['--steps', '4']):
        with pytest.raises(SystemExit):
            sample.main(['--random-init', '--output-path', str(tmp_path), '--self-condition'] + clash)
    flags = dict(train.FLAGS)
    assert flags['--self_condition']['action'] == 'store_true' and flags['--self_cond_prob']['type'] is float and flags['--self_cond_prob']['default'] is None
    assert '--self-condition' not in dict(evaluate.FLAGS)                    # evaluation reads the YAML key, to refuse it
    for doc in (sample.__doc__, train.__doc__, sample.build_models.__doc__, evaluate.__doc__):
        assert 'self_condition' in doc
    assert 'self_cond_prob' in train.__doc__ and 'not stored in checkpoints' in flags['--self_condition']['help']
