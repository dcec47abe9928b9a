"""Cascaded super-resolution on the host (no GPU): the fp64 restatement tests/_sr_ref.py against torch's interpolate and against two wrong
maps (what the GPU bound can see), and the plumbing -- constructor rules, refusals before any device work on a CPU handle, the C entries,
the YAML key and the command-line flags, and that a plain diffusion is what it was."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sr_ref as R          # noqa: E402
from _launch_hook import launches          # noqa: E402

INVALID, STATE = -1, -4
BUF = 1 << 20


# ---- the reference -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape,C', [(sh, C) for sh in R.SHAPES for C in (1, 3)] + [(R.BIG, 1)], ids=str)
def test_closed_form_is_torch_trilinear_half_pixel(shape, C):
    f, s, ft, fs = shape
    lo = R.make_lo(2, C, f, s, seed=f * 100 + s)
    a, b = R.up(lo, ft, fs), R.up_interpolate(lo, ft, fs)
    assert a.dtype == torch.float64 and a.shape == (2, C, f * ft, s * fs, s * fs) == b.shape
    assert (a - b).abs().max().item() <= 1e-14
    assert a.min().item() >= -1.0 and a.max().item() <= 1.0
    if (ft, fs) == (1, 1):
        assert torch.equal(a, 2.0 * lo.double() - 1.0)                     # the identity, exactly


@pytest.mark.parametrize('shape', [sh for sh in R.SHAPES if sh[2:] != (1, 1)], ids=str)
@pytest.mark.parametrize('wrong', ['align_corners', 'nearest'])
def test_bound_sees_the_wrong_maps(shape, wrong):
    """The mistakes that matter -- corners on corners instead of half-pixel centres, nearest neighbours instead of linear weights -- move
    the result by more than 1000 times the bound the kernel is held to."""
    f, s, ft, fs = shape
    lo = R.make_lo(2, 1, f, s, seed=5)
    err = (R.up(lo, ft, fs, wrong) - R.up(lo, ft, fs)).abs().max().item()
    assert err > 1000 * R.UP_BOUND, err


def test_down_and_aug_restatements():
    x = R.make_lo(2, 3, 4, 6, seed=1)
    assert torch.equal(R.down(x, 1, 1), x.double())
    d = R.down(x, 2, 3)
    assert d.shape == (2, 3, 2, 2, 2)
    assert abs(d[1, 2, 1, 0, 1].item() - x[1, 2, 2:4, 0:3, 3:6].double().mean().item()) < 1e-15
    u, z = torch.rand(2, 1, 2, 2, 2, dtype=torch.float64), torch.randn(2, 1, 2, 2, 2, dtype=torch.float64)
    out = R.aug(u, z, torch.tensor([1.0, 0.6], dtype=torch.float64), torch.tensor([0.0, 0.8], dtype=torch.float64))
    assert torch.equal(out[0], u[0]) and torch.allclose(out[1], 0.6 * u[1] + 0.8 * z[1], rtol=0, atol=1e-15)


# ---- the Python surface on a CPU handle ---------------------------------------------------------------------------------------------------

def _cpu_unet(**kw):
    from video_diffusion_nnx_amd.unet3d import Unet3D
    return Unet3D(rngs=0, mode='f32', dim=16, channels=kw.pop('channels', 1), dim_mults=(1, 2), device='cpu', **kw)


KW = dict(image_size=8, num_frames=4, channels=1, timesteps=10)
PARENT_ATTRIBUTES = ['_mtab', '_mtab_clean', '_ptab', '_sample_stream', 'alphas_cumprod', 'channels', 'denoise_fn', 'device', 'dynamic_thres_percentile',
                     'image_size', 'log_one_minus_alphas_cumprod', 'loss_type', 'num_frames', 'num_timesteps', 'posterior_log_variance_clipped',
                     'posterior_mean_coef1', 'posterior_mean_coef2', 'posterior_variance', 'sample_act_bf16', 'sqrt_alphas_cumprod',
                     'sqrt_one_minus_alphas_cumprod', 'sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod', 'text_use_bert_cls',
                     'use_dynamic_thres', 'learned_variance', 'vlb_weight', 'last_loss_terms']


def test_plain_diffusion_is_what_it_was():
    """lowres_cond=None (the default): the attributes of the instance and the draw keys of the train step are the parent's."""
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.train_step import cond_drop_key, focus_present_key, frame_cond_key, lowres_aug_key, micro_step_keys
    gd = GaussianDiffusion(_cpu_unet(), **KW)
    assert sorted(vars(gd)) == sorted(PARENT_ATTRIBUTES)
    assert gd.lowres_cond is None and gd.lowres_aug_max == 0
    assert sorted(vars(GaussianDiffusion(_cpu_unet(), lowres_cond=None, lowres_aug_max=0, **KW))) == sorted(PARENT_ATTRIBUTES)
    assert micro_step_keys(0, 0, 0) == (14889105232075457852, 1822111540196760150)
    assert micro_step_keys(7, 1, 5, 2) == (16534647458640461104, 4927238774316359071)
    # the augmentation has a key of its own: no other draw of the micro-step uses it
    keys = [lowres_aug_key(7, 1, 5, 2), cond_drop_key(7, 1, 5, 2), focus_present_key(7, 1, 5, 2), frame_cond_key(7, 1, 5, 2), *micro_step_keys(7, 1, 5, 2)]
    assert len(set(keys)) == len(keys)
    assert lowres_aug_key(7, 1, 5, 2) != lowres_aug_key(7, 1, 5, 0) != lowres_aug_key(7, 1, 6, 0)


def test_constructor_rules():
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    sr = lambda **k: _cpu_unet(channels=2, out_dim=1, **k)
    on = GaussianDiffusion(sr(), lowres_cond=(2, 2), lowres_aug_max=5, **KW)
    assert on.lowres_cond == (2, 2) and on.lowres_aug_max == 5
    assert sorted(vars(on)) == sorted(PARENT_ATTRIBUTES + ['lowres_cond', 'lowres_aug_max'])
    assert GaussianDiffusion(sr(), lowres_cond=(1, 1), **KW).lowres_cond == (1, 1)          # plain concat conditioning
    assert GaussianDiffusion(sr(), lowres_cond=[4, 8], **KW).lowres_cond == (4, 8)
    assert GaussianDiffusion(_cpu_unet(channels=6, out_dim=3), lowres_cond=(1, 2), **dict(KW, channels=3)).lowres_aug_max == 0
    for bad in ((0, 2), (2, 0), (2.0, 2), (True, 2), (2,), 2, (2, 2, 2), (-1, 1)):
        with pytest.raises(ValueError, match='lowres_cond'):
            GaussianDiffusion(sr(), lowres_cond=bad, **KW)
    for bad in ((3, 2), (2, 3), (8, 1), (1, 16)):                            # F = 4, S = 8
        with pytest.raises(ValueError, match='must divide'):
            GaussianDiffusion(sr(), lowres_cond=bad, **KW)
    for unet in (_cpu_unet(), _cpu_unet(channels=2), _cpu_unet(channels=2, out_dim=2), _cpu_unet(channels=3, out_dim=1), _cpu_unet(out_dim=2)):
        with pytest.raises(ValueError, match='channels == 2 \\* channels'):
            GaussianDiffusion(unet, lowres_cond=(2, 2), **KW)
    with pytest.raises(ValueError, match='learned_variance'):
        GaussianDiffusion(_cpu_unet(channels=2, out_dim=2), lowres_cond=(2, 2), learned_variance=True, **KW)
    for bad in (-1, 11, 2.5, True):
        with pytest.raises(ValueError, match='lowres_aug_max'):
            GaussianDiffusion(sr(), lowres_cond=(2, 2), lowres_aug_max=bad, **KW)
    with pytest.raises(ValueError, match='needs lowres_cond'):
        GaussianDiffusion(_cpu_unet(), lowres_aug_max=3, **KW)


def test_unsupported_combinations_raise_before_any_device_work():
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    gd = GaussianDiffusion(_cpu_unet(channels=2, out_dim=1), lowres_cond=(2, 2), lowres_aug_max=4, **KW)
    shape, x, lo = (1, 1, 4, 8, 8), torch.rand(1, 1, 4, 8, 8), torch.rand(1, 1, 2, 4, 4)
    t0 = torch.zeros(1, dtype=torch.int32)
    follow_ups = {
        'cond_scale': lambda: gd.sample(0, lowres=lo, cond=torch.zeros(1, 4), cond_scale=2.0),
        'cond_scale ': lambda: gd.p_sample(x, t0, 0, cond_scale=2.0, lowres_cond=x),
        'cond_scale  ': lambda: gd.p_mean_variance(x, t0, True, cond_scale=2.0, lowres_cond=x),
        'inpaint': lambda: gd.inpaint(0, x, torch.tensor([1, 0, 0, 0], dtype=torch.uint8)),
        'extend': lambda: gd.extend(0, x, 2),
        'frame_mask': lambda: gd.p_losses(x, t0, 0, frame_mask=torch.tensor([1, 0, 0, 0], dtype=torch.uint8)),
        'frame_mask ': lambda: gd(x, 0, frame_mask=torch.tensor([1, 0, 0, 0], dtype=torch.uint8)),
        'focus_present': lambda: gd.sample(0, lowres=lo, focus_present=True),
        'focus_present ': lambda: gd.p_losses(x, t0, 0, focus_present_mask=torch.ones(1, dtype=torch.uint8)),
        'calc_bpd_loop': lambda: gd.calc_bpd_loop(x, 0),
        'steps': lambda: gd.sample(0, lowres=lo, steps=4),
    }
    for word, fn in follow_ups.items():
        with pytest.raises(ValueError, match=f'does not support {word.strip()} yet \\(a follow-up'):
            fn()
    no_lowres = {
        'sample needs lowres': lambda: gd.sample(0, batch_size=1),
        'p_sample_loop has no low-resolution clip': lambda: gd.p_sample_loop(shape, 0),
        'ddim_sample_loop has no low-resolution clip': lambda: gd.ddim_sample_loop(shape, 0, steps=4),
        'dpm_sample_loop has no low-resolution clip': lambda: gd.dpm_sample_loop(shape, 0, steps=4),
        'needs lowres_cond=u': lambda: gd.p_sample(x, t0, 0),
    }
    for word, fn in no_lowres.items():
        with pytest.raises(ValueError, match=word):
            fn()
    # shapes, levels and sampler arguments are checked before anything touches a device
    for bad in (torch.rand(1, 1, 4, 4, 4), torch.rand(1, 2, 2, 4, 4), torch.rand(1, 1, 2, 8, 8), torch.rand(1, 2, 4, 4)):
        with pytest.raises(ValueError, match='lowres must be'):
            gd.upsample(0, bad)
    with pytest.raises(ValueError, match='lowres must be \\[1,'):
        gd.p_losses(x, t0, 0, lowres=torch.rand(2, 1, 2, 4, 4))
    for bad in (10, -2, [0, 1]):
        with pytest.raises(ValueError, match='augmentation level'):
            gd.upsample(0, lo, aug_level=bad)
    with pytest.raises(ValueError, match='augmentation level'):
        gd.p_losses(x, t0, 0, aug_levels=[10])
    with pytest.raises(ValueError, match='needs a key'):
        gd.lowres_condition(lo, None, 3)
    with pytest.raises(ValueError, match='two samplers'):
        gd.upsample(0, lo, ddim_steps=4, dpm_steps=4)
    with pytest.raises(ValueError, match='dpm_steps'):
        gd.upsample(0, lo, dpm_steps=11)
    with pytest.raises(ValueError, match='x_T must be'):
        gd.upsample(0, lo, x_T=torch.zeros(1, 1, 4, 4, 4))
    # and a plain diffusion refuses the new arguments
    plain = GaussianDiffusion(_cpu_unet(), **KW)
    for fn in (lambda: plain.upsample(0, lo), lambda: plain.sample(0, lowres=lo), lambda: plain.sample(0, batch_size=1, lowres_aug_level=2),
               lambda: plain.lowres_condition(lo), lambda: plain.p_sample(x, t0, 0, lowres_cond=x), lambda: plain.p_losses(x, t0, 0, lowres=lo),
               lambda: plain.p_losses(x, t0, 0, aug_levels=[0])):
        with pytest.raises(ValueError, match='super-resolution diffusion'):
            fn()


def test_augmentation_levels_are_a_host_draw_under_their_own_key():
    from video_diffusion_nnx_amd.gaussian_diffusion import lowres_aug_key, lowres_aug_levels, split_key
    lv = lowres_aug_levels(64, 7, 123)
    assert lv.dtype == torch.int32 and lv.shape == (64,) and int(lv.min()) >= 0 and int(lv.max()) <= 6 and len(set(lv.tolist())) == 7
    assert torch.equal(lv, lowres_aug_levels(64, 7, 123)) and not torch.equal(lv, lowres_aug_levels(64, 7, 124))
    assert lowres_aug_levels(5, 1, 9).tolist() == [0] * 5
    assert lowres_aug_key(99) not in split_key(99, 3)                      # children 1-3 of a loss key belong to other draws


# ---- the C entries ------------------------------------------------------------------------------------------------------------------------

ENTRIES = {'vdx_lowres_down': 9, 'vdx_lowres_input': 20, 'vdx_lowres_pack': 5, 'vdx_p_sample_loop_sr': 21, 'vdx_ddim_sample_loop_sr': 23,
           'vdx_dpm_sample_loop_sr': 25}


def test_entries_exist_and_match_the_header():
    from video_diffusion_nnx_amd import _lib as L
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'vdx.h')).read()
    assert '#define VDX_DRAW_LOWRES (1ull << 61)' in hdr and L.DRAW_LOWRES == 1 << 61
    for name, nargs in ENTRIES.items():
        fn = getattr(L, name)
        assert len(fn.argtypes) == nargs, name
        decl = hdr[hdr.index(f'int {name}('):]
        assert decl[:decl.index(');')].count(',') + 1 == nargs, name
    # the _sr loops: the arguments of the _dyn forms plus xin
    from video_diffusion_nnx_amd import gaussian_diffusion as G
    for sr, dyn in ((L.vdx_p_sample_loop_sr, G.vdx_p_sample_loop_dyn), (L.vdx_ddim_sample_loop_sr, G.vdx_ddim_sample_loop_dyn),
                    (L.vdx_dpm_sample_loop_sr, G.vdx_dpm_sample_loop)):
        assert len(sr.argtypes) == len(dyn.argtypes) + 1
        assert list(sr.argtypes[:4]) + list(sr.argtypes[5:]) == list(dyn.argtypes)


DOWN = dict(x=BUF, lo=BUF, batch=2, C=1, F=4, S=8, ft=2, fs=2, stream=0)
INPUT = dict(x0=BUF, t=BUF, noise=BUF, lo=BUF, aug=BUF, xin=BUF, sa=BUF, sm=BUF, T=10, seed=1, draw=0, ps=2.0, sh=-1.0, batch=2, C=1, F=4, S=8, ft=2, fs=2,
             stream=0)
PACK = dict(img=BUF, xin=BUF, batch=2, per=256, stream=0)
REJECTS = [
    ('lowres_down', DOWN, dict(x=0), 'null'), ('lowres_down', DOWN, dict(lo=0), 'null'), ('lowres_down', DOWN, dict(batch=0), 'batch'),
    ('lowres_down', DOWN, dict(ft=0), 'factors'), ('lowres_down', DOWN, dict(ft=3), 'must divide'), ('lowres_down', DOWN, dict(fs=3), 'must divide'),
    ('lowres_input', INPUT, dict(lo=0), 'null'), ('lowres_input', INPUT, dict(xin=0), 'null'), ('lowres_input', INPUT, dict(t=0), 'x0 needs t and noise'),
    ('lowres_input', INPUT, dict(noise=0), 'x0 needs t and noise'), ('lowres_input', INPUT, dict(sa=0), 'need the tables'),
    ('lowres_input', INPUT, dict(x0=0, t=0, noise=0, sm=0), 'need the tables'), ('lowres_input', INPUT, dict(T=0), 'need the tables'),
    ('lowres_input', INPUT, dict(fs=0), 'factors'), ('lowres_input', INPUT, dict(ft=3), 'must divide'), ('lowres_input', INPUT, dict(C=0), 'channels'),
    ('lowres_input', INPUT, dict(xin=BUF + 2), '4-byte'), ('lowres_input', INPUT, dict(lo=BUF + 1), '4-byte'),
    ('lowres_pack', PACK, dict(img=0), 'null'), ('lowres_pack', PACK, dict(xin=0), 'null'), ('lowres_pack', PACK, dict(per=0), 'per_sample'),
    ('lowres_pack', PACK, dict(batch=0), 'batch'), ('lowres_pack', PACK, dict(img=BUF + 2), '4-byte'),
]


@pytest.mark.parametrize('entry,base,change,word', REJECTS, ids=[f'{e}-{"-".join(c)}-{i}' for i, (e, _, c, _) in enumerate(REJECTS)])
def test_kernel_entries_reject_before_any_launch(entry, base, change, word):
    from video_diffusion_nnx_amd import _lib as L
    with launches() as seen:
        rc = getattr(L, 'vdx_' + entry)(*dict(base, **change).values())
    msg = L.vdx_last_error().decode()
    assert rc == INVALID and msg.startswith(entry + ': ') and word in msg, (rc, msg)
    assert seen == []


P_LOOP = dict(h=None, params=BUF, packed=BUF, img=BUF, xin=BUF, eps=BUF, t_dev=BUF, step_dev=BUF, tab=BUF, T=10, nsteps=1, cond=0, seed=3, clip=1, perc=0.0,
              thres=0, ws=BUF, ws_bytes=1 << 20, batch=2, use_graph=0, stream=0)
DDIM_LOOP = dict(h=None, params=BUF, packed=BUF, img=BUF, xin=BUF, eps=BUF, t_dev=BUF, step_dev=BUF, ac=BUF, seq=BUF, seq_len=4, nsteps=1, cond=0, clip=1,
                 tab=0, T=0, perc=0.0, thres=0, ws=BUF, ws_bytes=1 << 20, batch=2, use_graph=0, stream=0)
DPM_LOOP = dict(h=None, params=BUF, packed=BUF, img=BUF, xin=BUF, eps=BUF, hist=BUF, t_dev=BUF, step_dev=BUF, ac=BUF, seq=BUF, seq_len=4, nsteps=1, cond=0,
                clip=1, order=2, tab=0, T=0, perc=0.0, thres=0, ws=BUF, ws_bytes=1 << 20, batch=2, use_graph=0, stream=0)
LOOPS = [('p_sample_loop_sr', P_LOOP, ('h', 'params', 'packed', 'img', 'xin', 'eps', 't_dev', 'step_dev', 'tab', 'ws')),
         ('ddim_sample_loop_sr', DDIM_LOOP, ('h', 'params', 'packed', 'img', 'xin', 'eps', 't_dev', 'step_dev', 'ac', 'seq', 'ws')),
         ('dpm_sample_loop_sr', DPM_LOOP, ('h', 'params', 'packed', 'img', 'xin', 'eps', 't_dev', 'step_dev', 'ac', 'seq', 'ws'))]


@pytest.mark.parametrize('entry,base,nulls', LOOPS, ids=[e for e, _, _ in LOOPS])
def test_loops_reject_on_a_cpu_handle(entry, base, nulls):
    """Nulls and the channel rule are refused by name before the handle's device state is looked at, misalignment after it (as the other
    loops order their rules); a CPU handle is VDX_ERR_STATE; nothing is launched."""
    from video_diffusion_nnx_amd import _lib as L
    sr, plain, lv = _cpu_unet(channels=2, out_dim=1), _cpu_unet(), _cpu_unet(out_dim=2)
    base = dict(base, h=sr.handle(4, 8).ptr)
    fn = getattr(L, 'vdx_' + entry)
    with launches() as seen:
        call = lambda **ch: (fn(*dict(base, **ch).values()), L.vdx_last_error().decode())
        for n in nulls:
            rc, msg = call(**{n: 0})
            assert rc == INVALID and msg.startswith(entry + ': ') and 'null' in msg, (n, rc, msg)
        for other in (plain, lv, _cpu_unet(channels=2, out_dim=2), _cpu_unet(channels=4, out_dim=1)):
            rc, msg = call(h=other.handle(4, 8).ptr)
            assert rc == INVALID and msg.startswith(entry + ': ') and 'channels must equal 2 * out_dim' in msg, (rc, msg)
        rc, msg = call()
        assert rc == STATE and msg.startswith(entry + ': ') and 'without a GPU' in msg, (rc, msg)
        if torch.cuda.is_available():                                      # a device handle reaches the alignment rule
            from video_diffusion_nnx_amd.unet3d import Unet3D
            dev = Unet3D(rngs=0, mode='f32', dim=16, channels=2, out_dim=1, dim_mults=(1, 2))
            for ch in (dict(img=BUF + 4), dict(xin=BUF + 8)):
                rc, msg = call(h=dev.handle(4, 8).ptr, **ch)
                assert rc == INVALID and 'img / xin must be 16-byte aligned' in msg, (rc, msg)
        # the eleven loops above keep refusing such a network
        from video_diffusion_nnx_amd.gaussian_diffusion import vdx_p_sample_loop
        rc = vdx_p_sample_loop(base['h'], BUF, BUF, BUF, BUF, BUF, BUF, BUF, 10, 1, 0, 3, 1, BUF, 1 << 20, 2, 0, 0)
        msg = L.vdx_last_error().decode()
        assert rc in (INVALID, STATE) and (rc == STATE or 'out_dim must equal channels' in msg), (rc, msg)
    assert seen == []


# ---- YAML and command line ------------------------------------------------------------------------------------------------------------------

def test_yaml_key_and_flags(tmp_path):
    import numpy as np
    import yaml
    import sample
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(sample.__file__), 'configs', 'config_v1_0.yaml')))
    cfg['unet'].update(dim=16, dim_mults=[1, 2])
    import video_diffusion_nnx_amd.unet3d as U
    made = {}
    real = U.Unet3D

    class CpuUnet(real):
        def __init__(self, *a, **k):
            made.clear()
            made.update(k)
            super().__init__(*a, device='cpu', **k)

    U.Unet3D = CpuUnet
    C, Fr, S = cfg['diffusion']['channels'], cfg['diffusion']['num_frames'], cfg['diffusion']['image_size']
    try:
        unet, gd = sample.build_models(cfg, 'f32')
        assert gd.lowres_cond is None and unet.channels == C and 'out_dim' not in made and made['channels'] == C      # an absent key means off
        cfg['diffusion']['lowres_cond'] = dict(temporal=2, spatial=4, aug_max=100)
        unet, gd = sample.build_models(cfg, 'f32')
        assert (unet.channels, unet.out_dim) == (2 * C, C) and gd.lowres_cond == (2, 4) and gd.lowres_aug_max == 100 and gd.channels == C
        cfg['diffusion']['lowres_cond'] = dict(temporal=1, spatial=2)
        assert sample.build_models(cfg, 'f32')[1].lowres_aug_max == 0
        cfg['diffusion']['lowres_cond'] = dict(temporal=2, spatial=S + 1)
        with pytest.raises(ValueError, match='must divide'):
            sample.build_models(cfg, 'f32')
        cfg['diffusion']['lowres_cond'] = dict(temporal=2, spatial=2)
        cfg['diffusion']['learned_variance'] = True
        with pytest.raises(ValueError, match='learned_variance'):
            sample.build_models(cfg, 'f32')
    finally:
        U.Unet3D = real
    p = sample.build_parser()
    a = p.parse_args(['--random-init', '--lowres-path', 'x.npy', '--lowres-aug-level', '30', '--save-npy'])
    assert (a.lowres_path, a.lowres_aug_level, a.save_npy) == ('x.npy', 30, True)
    a = p.parse_args(['--random-init'])
    assert (a.lowres_path, a.lowres_aug_level, a.save_npy) == (None, None, False)
    for clash in (['--lowres-path', 'x.npy', '--context', 'c.npy'], ['--lowres-path', 'x.npy', '--cond-path', 'c.npy'],
                  ['--lowres-path', 'x.npy', '--steps', '4'], ['--lowres-aug-level', '3']):
        with pytest.raises(SystemExit):
            sample.main(['--random-init', '--output-path', str(tmp_path)] + clash)
    # the file's shape is checked against the config's
    good = np.zeros((3, C, Fr // 2, S // 4, S // 4), np.uint8) + 255
    path = tmp_path / 'lo.npy'
    np.save(path, good)
    lo = sample.load_lowres(str(path), good.shape[1:])
    assert lo.dtype == np.float32 and lo.shape == good.shape and float(lo.max()) == 1.0
    with pytest.raises(ValueError, match='--lowres-path must hold'):
        sample.load_lowres(str(path), (C, Fr, S, S))
