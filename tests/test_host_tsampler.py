"""CPU tests of loss-aware timestep sampling (vdx.h: "Loss-aware timestep sampling"): the symbols, the refusals of
vdx_tsampler_draw before any launch, the Trainer / train.py / YAML switches, the key the draw runs under, and the fp64 reference sampler of
tests/_tsampler_ref.py itself (cold and warm probabilities, unbiasedness, the variance it buys, the update's semantics)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tsampler_ref as TR               # noqa: E402
from _launch_hook import launches        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def test_symbols_resolve_and_are_declared():
    from video_diffusion_nnx_amd import _lib as L, timestep_sampler as TS
    hdr = open(os.path.join(ROOT, 'include', 'vdx.h')).read()
    for name in ('vdx_tsampler_draw', 'vdx_tsampler_update', 'vdx_loss_weighted', 'vdx_loss_weighted_scratch_doubles', 'vdx_hybrid_loss_w'):
        assert hasattr(L.lib, name) and f' {name}(' in hdr, name
    assert 'Loss-aware timestep sampling' in hdr
    assert TS.vdx_loss_weighted_scratch_doubles(3) == 3 * 64 and TS.vdx_loss_weighted_scratch_doubles(0) == 0
    assert callable(L.vdx_hybrid_loss_w) and callable(TS.vdx_tsampler_draw) and callable(TS.vdx_tsampler_update) and callable(TS.vdx_loss_weighted)


def test_draw_refusals_come_before_any_launch():
    from video_diffusion_nnx_amd import _lib as L, timestep_sampler as TS
    hist = torch.zeros(8, 2, dtype=torch.float64)
    count = torch.zeros(8, dtype=torch.int32)
    t, iw = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.float64)

    def call(T=8, H=2, eps=0.001, batch=4):
        return TS.vdx_tsampler_draw(hist.data_ptr(), count.data_ptr(), T, H, eps, 0, 1, 0, t.data_ptr(), iw.data_ptr(), 0, batch, 0)
    with launches() as rec:
        for kw, word in ((dict(T=0), 'timesteps'), (dict(T=4097), 'timesteps'), (dict(H=0), 'history'), (dict(H=33), 'history'),
                         (dict(eps=0.0), 'uniform_prob'), (dict(eps=-0.5), 'uniform_prob'), (dict(eps=1.5), 'uniform_prob'),
                         (dict(batch=0), 'batch')):
            assert call(**kw) == INVALID, kw
            assert word in L.vdx_last_error().decode(), (kw, L.vdx_last_error())
    assert rec == []
    assert TS.vdx_tsampler_update(hist.data_ptr(), count.data_ptr(), 4097, 2, 0, 0, 0) == INVALID
    assert TS.vdx_tsampler_update(hist.data_ptr(), count.data_ptr(), 8, 33, 0, 0, 0) == INVALID
    assert TS.vdx_tsampler_update(hist.data_ptr(), count.data_ptr(), 8, 2, 0, 0, 0) == 0             # no entries: nothing to do
    for bad in (dict(timesteps=0), dict(timesteps=4097), dict(timesteps=8, history_per_term=0), dict(timesteps=8, history_per_term=33),
                dict(timesteps=8, uniform_prob=0.0), dict(timesteps=8, uniform_prob=1.01)):
        with pytest.raises(ValueError):
            TS.LossSecondMomentSampler(device='cpu', **bad)
    s = TS.LossSecondMomentSampler(8, device='cpu')
    assert s.history_per_term == 10 and s.uniform_prob == 0.001 and s.hist.shape == (8, 10) and s.hist.dtype == torch.float64
    assert s.count.dtype == torch.int32 and not s.warm
    s.load_state(torch.ones(8, 10), torch.full((8,), 10))
    assert s.warm and s.state()[0].data_ptr() != s.hist.data_ptr()
    with pytest.raises(ValueError):
        s.load_state(torch.ones(8, 9), torch.full((8,), 9))


def _trainer(tmp_path, T=8, **kw):
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.trainer import Trainer
    from video_diffusion_nnx_amd.unet3d import Unet3D
    unet = Unet3D(dim=16, rngs=0, channels=1, device='cpu')
    gd = GaussianDiffusion(unet, image_size=8, num_frames=2, channels=1, timesteps=T)
    return Trainer(gd, str(tmp_path), dataset_path='synthetic:8', train_batch_size=2, train_num_steps=2, checkpoint_every_steps=100,
                   results_folder=str(tmp_path / 'res'), **kw)


def test_trainer_switches(tmp_path, monkeypatch):
    from video_diffusion_nnx_amd.trainer import Trainer
    assert (Trainer.timestep_sampler, Trainer.sampler_history, Trainer.sampler_uniform_prob) == ('uniform', 10, 0.001)
    tr = _trainer(tmp_path / 'a')
    assert tr.sampler is None and tr.last_iw is None and tr.last_loss_per_sample is None
    monkeypatch.setattr(Trainer, 'timestep_sampler', 'loss-second-moment')
    monkeypatch.setattr(Trainer, 'sampler_history', 3)
    monkeypatch.setattr(Trainer, 'sampler_uniform_prob', 0.01)
    tr = _trainer(tmp_path / 'b')
    assert (tr.sampler.timesteps, tr.sampler.history_per_term, tr.sampler.uniform_prob) == (8, 3, 0.01)
    for name, bad in (('timestep_sampler', 'importance'), ('sampler_history', 0), ('sampler_history', 33), ('sampler_uniform_prob', 0.0),
                      ('sampler_uniform_prob', 1.5)):
        with monkeypatch.context() as m:
            m.setattr(Trainer, name, bad)
            with pytest.raises(ValueError, match=name):
                _trainer(tmp_path / 'c')
    with monkeypatch.context() as m:                                                  # frame-conditioned training: no per-sample masked loss yet
        m.setattr(Trainer, 'frame_cond_max', 1)
        with pytest.raises(ValueError, match='frame'):
            _trainer(tmp_path / 'd')
    with pytest.raises(ValueError, match='4096'):                                     # the LDS budget of the draw's one workgroup
        _trainer(tmp_path / 'e', T=5000)
    # history and probability are validated whatever the sampler
    monkeypatch.setattr(Trainer, 'timestep_sampler', 'uniform')
    monkeypatch.setattr(Trainer, 'sampler_history', 0)
    with pytest.raises(ValueError, match='sampler_history'):
        _trainer(tmp_path / 'f')


def test_frame_mask_is_refused_before_any_work(tmp_path, monkeypatch):
    from video_diffusion_nnx_amd.trainer import Trainer
    monkeypatch.setattr(Trainer, 'timestep_sampler', 'loss-second-moment')
    tr = _trainer(tmp_path)
    with launches() as rec:
        with pytest.raises(ValueError, match='frame'):
            tr.train_step(torch.rand(2, 1, 2, 8, 8), 0, frame_mask=torch.tensor([1, 0]))
    assert rec == []


def test_yaml_keys_and_flags(monkeypatch, tmp_path):
    import sample
    import train
    from video_diffusion_nnx_amd.trainer import Trainer
    with open(os.path.join(ROOT, 'configs', 'config_v2_2.yaml')) as fh:
        cfg = yaml.safe_load(fh)
    assert not {'timestep_sampler', 'sampler_history', 'sampler_uniform_prob'} & set(cfg['trainer'])
    flags = dict(train.FLAGS)
    assert flags['--timestep_sampler']['choices'] == ('uniform', 'loss-second-moment') and flags['--timestep_sampler']['default'] is None
    assert '--sampler_history' in flags and '--sampler_uniform_prob' in flags and 'timestep_sampler' in train.__doc__
    monkeypatch.setattr(sample, 'build_models', lambda c, mode, **kw: (None, None))
    seen = {}

    class Stop(Exception):
        pass

    def stop(self, *a, **kw):
        seen.update(kw)
        raise Stop()
    monkeypatch.setattr(Trainer, '__init__', stop)
    for name, val in (('timestep_sampler', 'uniform'), ('sampler_history', 10), ('sampler_uniform_prob', 0.001)):
        monkeypatch.setattr(Trainer, name, val)
    path = tmp_path / 'c.yaml'
    path.write_text(yaml.safe_dump(cfg))
    with pytest.raises(Stop):
        train.main(['--config', str(path)])
    assert (Trainer.timestep_sampler, Trainer.sampler_history, Trainer.sampler_uniform_prob) == ('uniform', 10, 0.001)      # absent = off
    with pytest.raises(Stop):
        train.main(['--config', str(path), '--timestep_sampler', 'loss-second-moment', '--sampler_history', '4', '--sampler_uniform_prob', '0.05'])
    assert (Trainer.timestep_sampler, Trainer.sampler_history, Trainer.sampler_uniform_prob) == ('loss-second-moment', 4, 0.05)
    for name, val in (('timestep_sampler', 'uniform'), ('sampler_history', 10), ('sampler_uniform_prob', 0.001)):
        monkeypatch.setattr(Trainer, name, val)
    cfg['trainer'].update(timestep_sampler='loss-second-moment', sampler_history=7, sampler_uniform_prob=0.5)
    path.write_text(yaml.safe_dump(cfg))
    with pytest.raises(Stop):
        train.main(['--config', str(path)])
    assert (Trainer.timestep_sampler, Trainer.sampler_history, Trainer.sampler_uniform_prob) == ('loss-second-moment', 7, 0.5)
    assert not {'timestep_sampler', 'sampler_history', 'sampler_uniform_prob'} & set(seen)       # popped: not constructor arguments
    with pytest.raises(Stop):
        train.main(['--config', str(path), '--timestep_sampler', 'uniform'])                    # the flag wins
    assert Trainer.timestep_sampler == 'uniform'
    for argv in (['--sampler_history', '0'], ['--sampler_history', '33'], ['--sampler_uniform_prob', '0'], ['--timestep_sampler', 'other']):
        with pytest.raises(SystemExit):
            train.main(['--config', str(path)] + argv)


def test_the_draw_runs_under_t_key_and_moves_no_other_key(tmp_path, monkeypatch):
    """forward_backward hands micro_step_keys' t_key (draw 0) to the sampler; the noise key and the keys of the other draws are functions of
    (seed, rank, step, j) alone, so the switch cannot move them."""
    from video_diffusion_nnx_amd import train_step as S
    from video_diffusion_nnx_amd.trainer import Trainer
    monkeypatch.setattr(Trainer, 'timestep_sampler', 'loss-second-moment')
    tr = _trainer(tmp_path, rng_seed=5)
    seen = []

    class Stop(Exception):
        pass

    def draw(batch, key, draw=0, t=None):
        seen.append((batch, key, draw, t))
        raise Stop()
    tr.sampler.draw = draw
    others = [f(5, 0, 3, j) for j in (0, 2) for f in (S.frame_cond_key, S.cond_drop_key, S.focus_present_key, S.lowres_aug_key)]
    for j in (0, 2):
        with pytest.raises(Stop):
            S.forward_backward(tr, torch.rand(2, 1, 2, 8, 8), 3, j=j)
    t_keys = [S.micro_step_keys(5, 0, 3, j)[0] for j in (0, 2)]
    assert [(b, k, d) for b, k, d, _ in seen] == [(2, t_keys[0], 0), (2, t_keys[1], 0)] and all(t is None for *_, t in seen)
    assert t_keys[0] != t_keys[1]
    assert others == [f(5, 0, 3, j) for j in (0, 2) for f in (S.frame_cond_key, S.cond_drop_key, S.focus_present_key, S.lowres_aug_key)]
    assert len({*others, *t_keys, *(S.micro_step_keys(5, 0, 3, j)[1] for j in (0, 2))}) == 12


# ---- the reference sampler ---------------------------------------------------------------------------------------------------------------

def test_reference_cold_is_uniform_with_unit_weights():
    r = TR.RefSampler(5, H=3)
    r.update([(t, 1.0 + t) for t in range(5) for _ in range(3)][:-1])                 # one slot of one level still empty
    assert not r.warm and np.array_equal(r.probabilities(), np.full(5, 0.2))
    t, iw = r.draw(64, key=7)
    assert np.array_equal(iw, np.ones(64)) and t.min() >= 0 and t.max() <= 4 and len(set(t.tolist())) == 5
    u = r.uniforms(64, 7)
    assert np.array_equal(t, np.minimum(np.floor(u * 5), 4).astype(np.int32)) and (u > 0).all() and (u < 1).all()
    _, iw = r.draw(3, key=7, t=[0, 4, 2])
    assert np.array_equal(iw, np.ones(3))


def test_reference_warm_three_levels_by_hand():
    r = TR.RefSampler(3, H=2, eps=0.1)
    r.update([(0, 3.0), (0, 4.0), (1, 0.0), (1, 0.0), (2, 6.0), (2, 8.0)])
    assert r.warm
    # w = sqrt((9 + 16) / 2), 0, sqrt((36 + 64) / 2) = 5 / sqrt 2 * (1, 0, 2): w / W = 1/3, 0, 2/3
    want = np.array([1 / 3, 0.0, 2 / 3]) * 0.9 + 0.1 / 3
    p = r.probabilities()
    assert np.allclose(p, want, rtol=1e-15, atol=0) and abs(p.sum() - 1.0) < 1e-15
    t, iw = r.draw(4, key=1, t=[0, 1, 2, 1])
    assert np.allclose(iw, 1.0 / (3 * want[[0, 1, 2, 1]]), rtol=1e-15)
    # the draw: the first level whose inclusive prefix sum exceeds u
    u, cum = r.uniforms(200, 9), np.cumsum(p)
    t, iw = r.draw(200, key=9)
    assert np.array_equal(t, [int(np.argmax(cum > x)) for x in u]) and set(t.tolist()) == {0, 1, 2}
    assert np.array_equal(iw, 1.0 / (3 * p[t]))
    # an all-zero history is uniform, not a division by zero
    z = TR.RefSampler(3, H=2)
    z.load_state(np.zeros((3, 2)), np.full(3, 2))
    assert z.warm and np.array_equal(z.probabilities(), np.full(3, 1 / 3))
    z.load_state(np.full((3, 2), 1e200), np.full(3, 2))                                # the squares overflow
    assert np.array_equal(z.probabilities(), np.full(3, 1 / 3))


def test_reference_is_unbiased():
    g = np.random.default_rng(0)
    T = 50
    r = TR.RefSampler(T, H=4, eps=0.01)
    r.load_state(np.exp(g.normal(size=(T, 4)) * 3), np.full(T, 4))
    p = r.probabilities()
    _, iw = r.draw(T, key=0, t=np.arange(T))
    f = g.normal(size=T)
    assert abs(np.sum(p * iw * f) - np.mean(f)) <= 1e-15
    assert abs(p.sum() - 1.0) <= 1e-14 and (p >= 0.01 / T * (1 - 1e-12)).all()


def test_reference_variance_is_below_uniform_on_a_steep_profile():
    """Per-level losses whose second moment spans 1e4 (the shape of the curves evaluate.py writes): the importance estimator's closed-form
    variance, with p from a history drawn from that profile, is below the uniform estimator's."""
    g = np.random.default_rng(1)
    T, H = 100, 10
    scale = 10.0 ** np.linspace(0.0, -2.0, T)                                          # E[l^2] ~ scale^2: 1 .. 1e-4
    mean, std = scale, 0.5 * scale
    f2 = mean ** 2 + std ** 2
    r = TR.RefSampler(T, H=H)
    r.load_state(mean[:, None] + std[:, None] * g.normal(size=(T, H)), np.full(T, H))
    p = r.probabilities()
    v_imp = TR.estimator_variances(p, f2, mean)
    v_uni = TR.estimator_variances(np.full(T, 1.0 / T), f2, mean)
    assert f2.max() / f2.min() >= 1e4 * (1 - 1e-12)
    assert 0 < v_imp < 0.5 * v_uni, (v_imp, v_uni)


def test_reference_update_semantics():
    r = TR.RefSampler(4, H=3)
    r.update([(1, 1.0), (1, 2.0), (2, 9.0), (1, 3.0)])                                  # duplicates of one level, in index order
    assert r.count.tolist() == [0, 3, 1, 0] and r.hist[1].tolist() == [1.0, 2.0, 3.0] and r.hist[2, 0] == 9.0
    r2 = TR.RefSampler(4, H=3)
    r2.update([(1, 1.0), (1, 2.0)])
    assert r2.count[1] == 2                                                             # H - 1
    r2.update([(1, 3.0)])
    assert r2.count[1] == 3 and r2.hist[1].tolist() == [1.0, 2.0, 3.0]                  # H
    r2.update([(1, 4.0), (1, 5.0)])
    assert r2.count[1] == 3 and r2.hist[1].tolist() == [3.0, 4.0, 5.0]                  # shifted twice
    before = (r2.hist.copy(), r2.count.copy())
    r2.update([(0, float('nan')), (0, float('inf')), (0, -float('inf')), (-1, 1.0), (4, 1.0), (float('nan'), 1.0)])
    assert np.array_equal(r2.hist, before[0]) and np.array_equal(r2.count, before[1])    # skipped: one NaN step does not poison the sampler
    r2.update([(0, float('nan')), (0, 7.0)])
    assert r2.count[0] == 1 and r2.hist[0, 0] == 7.0
