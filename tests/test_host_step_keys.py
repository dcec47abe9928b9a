"""The host layer's shared pieces, without a GPU: the key tree of one train step (train_step.step_keys), the one refusal helper
(GaussianDiffusion._refuse) with every message it has to keep, and the one (chain, steps) choice (gaussian_diffusion.chain_choice)."""
import itertools

import pytest
import torch


# ---- 1. the key tree ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('seed', [0, 1, 2 ** 63 + 5])
def test_step_keys_are_the_tree(seed):
    """Restated from split_key alone, by child index (1-based: child i of k is split_key(k, i)[-1])."""
    from video_diffusion_nnx_amd import train_step as S
    from video_diffusion_nnx_amd.gaussian_diffusion import split_key
    child = lambda k, i: split_key(k, i)[-1]
    for rank, step, j in itertools.product((0, 3), (0, 1, 1000), (0, 1, 4)):
        micro = child(child(seed, rank + 1), step + 1)
        if j > 0:
            micro = child(micro, 3 + j)
        loss = child(micro, 3)
        want = dict(frame_cond=child(micro, 1), t=child(micro, 2), cond_drop=child(loss, 1), noise=child(loss, 2),
                    focus_present=child(loss, 3), lowres_aug=child(loss, 4))
        keys = S.step_keys(seed, rank, step, j)
        assert keys._fields == ('t', 'noise', 'frame_cond', 'cond_drop', 'focus_present', 'lowres_aug')
        assert keys._asdict() == want, (seed, rank, step, j)
        assert len(set(keys)) == 6, (seed, rank, step, j)
        args = (seed, rank, step, j)
        assert S.micro_step_keys(*args) == (keys.t, keys.noise)
        assert S.frame_cond_key(*args) == keys.frame_cond and S.cond_drop_key(*args) == keys.cond_drop
        assert S.focus_present_key(*args) == keys.focus_present and S.lowres_aug_key(*args) == keys.lowres_aug
        if j == 0:
            assert S.step_keys(seed, rank, step) == keys


# ---- 2. the refusals ------------------------------------------------------------------------------------------------------------------------

def _cpu_unet(**kw):
    from video_diffusion_nnx_amd.unet3d import Unet3D
    return Unet3D(rngs=0, mode='f32', dim=16, channels=kw.pop('channels', 1), dim_mults=(1, 2), device='cpu', **kw)


KW = dict(image_size=8, num_frames=4, channels=1, timesteps=10)
SHAPE = (2, 1, 4, 8, 8)


def _gd(feature=None):
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    if feature == 'learned_variance':
        return GaussianDiffusion(_cpu_unet(out_dim=2), learned_variance=True, **KW)
    if feature == 'lowres_cond':
        return GaussianDiffusion(_cpu_unet(channels=2, out_dim=1), lowres_cond=(2, 2), **KW)
    if feature == 'frame_noise_alpha':
        return GaussianDiffusion(_cpu_unet(), frame_noise_alpha=1.0, **KW)
    return GaussianDiffusion(_cpu_unet(), **KW)


PREFIX = {'learned_variance': 'learned_variance', 'lowres_cond': 'lowres_cond (super-resolution)', 'frame_noise_alpha': 'frame_noise_alpha'}
X, T_ = torch.rand(SHAPE), torch.tensor([1, 2])
LOW = torch.rand(2, 1, 2, 4, 4)
# (feature, keyword, a value in use, the public call that refuses it before any device work)
REFUSALS = [
    ('learned_variance', 'cond_scale', 2.0, lambda gd: gd.p_sample_loop(SHAPE, 0, cond_scale=2.0)),
    ('learned_variance', 'cond_scale', 2.0, lambda gd: gd.p_sample(X, T_, 0, cond_scale=2.0)),
    ('learned_variance', 'cond_scale', 2.0, lambda gd: gd.p_mean_variance(X, T_, True, cond_scale=2.0)),
    ('learned_variance', 'cond_scale', 2.0, lambda gd: gd.sample(0, cond_scale=2.0)),
    ('learned_variance', 'guidance_rescale', 0.5, lambda gd: gd.p_sample_loop(SHAPE, 0, guidance_rescale=0.5)),
    ('learned_variance', 'guidance_rescale', 0.5, lambda gd: gd.sample(0, guidance_rescale=0.5)),
    ('learned_variance', 'focus_present', True, lambda gd: gd.p_sample_loop(SHAPE, 0, focus_present=True)),
    ('learned_variance', 'focus_present', True, lambda gd: gd.calc_bpd_loop(X, 0, focus_present=True)),
    ('learned_variance', 'focus_present', True, lambda gd: gd.sample(0, focus_present=True)),
    ('learned_variance', 'focus_present', True, lambda gd: gd.p_losses(X, T_, 0, focus_present_mask=True)),
    ('learned_variance', 'ddim_steps', 2, lambda gd: gd.ddim_sample_loop(SHAPE, 0, steps=2)),
    ('learned_variance', 'ddim_steps', 2, lambda gd: gd.sample(0, ddim_steps=2)),
    ('learned_variance', 'dpm_steps', 2, lambda gd: gd.dpm_sample_loop(SHAPE, 0, steps=2)),
    ('learned_variance', 'dpm_steps', 2, lambda gd: gd.sample(0, dpm_steps=2)),
    ('learned_variance', 'inpaint', True, lambda gd: gd.inpaint(0, X, torch.tensor([1, 0, 0, 0], dtype=torch.bool))),
    ('learned_variance', 'extend', True, lambda gd: gd.extend(0, X, 2)),
    ('learned_variance', 'frame_mask', [1, 0, 0, 0], lambda gd: gd.p_losses(X, T_, 0, frame_mask=torch.tensor([1, 0, 0, 0], dtype=torch.bool))),
    ('lowres_cond', 'cond_scale', 2.0, lambda gd: gd.p_sample(X, T_, 0, cond_scale=2.0, lowres_cond=X)),
    ('lowres_cond', 'cond_scale', 2.0, lambda gd: gd.p_mean_variance(X, T_, True, cond_scale=2.0, lowres_cond=X)),
    ('lowres_cond', 'cond_scale', 2.0, lambda gd: gd.sample(0, cond_scale=2.0, lowres=LOW)),
    ('lowres_cond', 'guidance_rescale', 0.5, lambda gd: gd.sample(0, guidance_rescale=0.5, lowres=LOW)),
    ('lowres_cond', 'focus_present', True, lambda gd: gd.sample(0, focus_present=True, lowres=LOW)),
    ('lowres_cond', 'focus_present', True, lambda gd: gd.p_losses(X, T_, 0, focus_present_mask=True)),
    ('lowres_cond', 'steps', 2, lambda gd: gd.sample(0, steps=2, lowres=LOW)),
    ('lowres_cond', 'calc_bpd_loop', True, lambda gd: gd.calc_bpd_loop(X, 0)),
    ('lowres_cond', 'inpaint', True, lambda gd: gd.inpaint(0, X, torch.tensor([1, 0, 0, 0], dtype=torch.bool))),
    ('lowres_cond', 'extend', True, lambda gd: gd.extend(0, X, 2)),
    ('lowres_cond', 'frame_mask', [1, 0, 0, 0], lambda gd: gd.p_losses(X, T_, 0, frame_mask=torch.tensor([1, 0, 0, 0], dtype=torch.bool))),
    ('frame_noise_alpha', 'calc_bpd_loop', True, lambda gd: gd.calc_bpd_loop(X, 0)),
    ('frame_noise_alpha', 'inpaint', True, lambda gd: gd.inpaint(0, X, torch.tensor([1, 0, 0, 0], dtype=torch.bool))),
    ('frame_noise_alpha', 'extend', True, lambda gd: gd.extend(0, X, 2)),
]


@pytest.fixture(scope='module')
def diffusions():
    return {f: _gd(f) for f in (None, *PREFIX)}


def _text(feature, keyword):
    return f'{PREFIX[feature]} does not support {keyword} yet (a follow-up; DESIGN.md 9)'


def test_every_refusal_keeps_its_text(diffusions):
    assert {(f, k) for f, k, _, _ in REFUSALS} == {
        *(('learned_variance', k) for k in ('cond_scale', 'guidance_rescale', 'focus_present', 'ddim_steps', 'dpm_steps', 'inpaint', 'extend', 'frame_mask')),
        *(('lowres_cond', k) for k in ('cond_scale', 'guidance_rescale', 'focus_present', 'steps', 'calc_bpd_loop', 'inpaint', 'extend', 'frame_mask')),
        *(('frame_noise_alpha', k) for k in ('calc_bpd_loop', 'inpaint', 'extend'))}
    for feature, keyword, value, call in REFUSALS:
        gd = diffusions[feature]
        for raises in (lambda: gd._refuse(feature, **{keyword: value}), lambda: call(gd)):
            with pytest.raises(ValueError) as e:
                raises()
            assert str(e.value) == _text(feature, keyword), (feature, keyword)


def test_refuse_lets_the_rest_through(diffusions):
    for feature in PREFIX:
        # the feature is off: nothing is refused, whatever is given
        assert diffusions[None]._refuse(feature, cond_scale=2.0, inpaint=True, frame_mask=[1]) is None
        for other in PREFIX:
            if other != feature:
                assert diffusions[other]._refuse(feature, inpaint=True) is None
        # the feature is on: None, False and the neutral values of the two guidance numbers are "not in use"
        gd = diffusions[feature]
        assert gd._refuse(feature, cond_scale=1.0, guidance_rescale=0.0, focus_present=None, frame_mask=None, inpaint=False, steps=None) is None
        assert gd._refuse(feature, cond_scale=1, guidance_rescale=0) is None
        # the first keyword in use is the one named
        with pytest.raises(ValueError, match='does not support extend yet'):
            gd._refuse(feature, cond_scale=1.0, extend=True, inpaint=True)
    with pytest.raises(KeyError):
        diffusions[None]._refuse('no_such_feature', inpaint=True)


# ---- 3. the chain choice --------------------------------------------------------------------------------------------------------------------

def test_chain_choice():
    from video_diffusion_nnx_amd.gaussian_diffusion import chain_choice, check_dpm_args
    assert chain_choice(10) == ('ddpm', 0)
    assert chain_choice(10, None, None, 2, 3) == ('ddpm', 0)                # resampling is the ancestral chain's
    assert chain_choice(10, 0, None) == ('ddpm', 0)                          # ddim_steps = 0 is "not given", as in sample()
    for S in (1, 4, 10):
        assert chain_choice(10, S) == ('ddim', S) and chain_choice(10, ddim_steps=S) == ('ddim', S)
        for order in (1, 2):
            assert chain_choice(10, None, S, order) == ('dpm', S)
    assert chain_choice(10, None, 4.0) == ('dpm', 4) and isinstance(chain_choice(10, None, 4.0)[1], int)
    bad = [dict(ddim_steps=3, dpm_steps=3), dict(dpm_steps=3, resample_steps=2), dict(dpm_steps=3, dpm_order=3), dict(dpm_steps=3, dpm_order=0),
           dict(dpm_steps=0), dict(dpm_steps=11)]
    for kw in bad:
        with pytest.raises(ValueError) as want:
            check_dpm_args(10, kw.get('dpm_steps'), kw.get('dpm_order', 2), kw.get('ddim_steps'), kw.get('resample_steps', 1))
        with pytest.raises(ValueError) as got:
            chain_choice(10, **kw)
        assert str(got.value) == str(want.value), kw


def test_the_three_callers_use_the_choice(diffusions, monkeypatch):
    """upsample, inpaint / extend and sample hand their sampler keywords to chain_choice: what it refuses, they refuse."""
    gd, sr = diffusions[None], diffusions['lowres_cond']
    mask = torch.tensor([1, 0, 0, 0], dtype=torch.bool)
    for call in (lambda **kw: gd.sample(0, batch_size=2, **kw), lambda **kw: gd.inpaint(0, X, mask, **kw), lambda **kw: gd.extend(0, X, 2, **kw),
                 lambda **kw: sr.upsample(0, LOW, **kw)):
        with pytest.raises(ValueError, match='two samplers'):
            call(ddim_steps=2, dpm_steps=2)
        with pytest.raises(ValueError, match='dpm_order must be 1 or 2'):
            call(dpm_steps=2, dpm_order=3)
    o = gd._inpaint_options(X, dict(dpm_steps=3))
    assert (o['chain'], o['steps']) == ('dpm', 3)
    o = gd._inpaint_options(X, dict(ddim_steps=4))
    assert (o['chain'], o['steps']) == ('ddim', 4)
    o = gd._inpaint_options(X, dict(resample_steps=2))
    assert (o['chain'], o['steps']) == ('ddpm', 0)


def test_loop_args_spell_the_signatures():
    """The driver's positional arguments by name are the signatures of tests/_sample_loop_sigs.py for the nine entries listed there, and
    as many as the C prototype takes for every entry of the table."""
    from _sample_loop_sigs import SIGS
    from video_diffusion_nnx_amd import gaussian_diffusion as G
    names = {n: n for sig in SIGS.values() for n in sig.split()}
    names.update({n: n for n in 'xin lv_tab post_scale post_shift mix_a mix_b'.split()})
    entry = {'ddpm': 'p_sample_loop', 'ddim': 'ddim_sample_loop', 'dpm': 'dpm_sample_loop'}
    for (chain, variant), fn in G._LOOPS.items():
        args = G.loop_args(chain, variant, names)
        assert len(args) == len(fn.argtypes), (chain, variant)
        if variant in ('plain', 'masked', 'guided'):
            name = entry[chain] + {'plain': '' if chain == 'dpm' else '_dyn', 'masked': '_masked', 'guided': '_guided'}[variant]
            assert args == SIGS[name].split(), (chain, variant)
            assert fn is (getattr(G, 'vdx_' + name, None) or getattr(G.L, 'vdx_' + name))
    assert sorted({v for _, v in G._LOOPS}) == ['guided', 'lv', 'masked', 'mixed', 'plain', 'sr'] and len(G._LOOPS) == 14
    assert G.loop_args('ddpm', 'mixed', names) == G.loop_args('ddpm', 'guided', names)[:-5] + ['mix_a', 'mix_b'] + G.loop_args('ddpm', 'guided', names)[-5:]
    assert G.loop_args('ddim', 'sr', names) == [n for n in G.loop_args('ddim', 'plain', names)[:4]] + ['xin'] + G.loop_args('ddim', 'plain', names)[4:]
