"""CPU tests of the focus-present mask (Unet3D(focus_present=True)): the fp64 references of tests/_focus_ref.py against the
closed forms they stand for, the proof that the GPU bounds of tests/test_gpu_focus.py tell a wrong-sample mask, the host-side mask draw
and its key, the CLI / YAML plumbing and the Python errors.  No GPU."""
import os

import pytest
import torch
import yaml

import _focus_ref as FR
import _posbias_ref as PB
from oracle import unet3d_ref as R

F64 = torch.float64
SHAPES = [(3, 16, 3, 2, 64, 8), (2, 10, 3, 3, 32, 8), (2, 3, 2, 2, 128, 8), (2, 16, 2, 2, 512, 8), (2, 16, 2, 2, 528, 8), (3, 20, 3, 3, 16, 4),
          (2, 40, 2, 2, 64, 8)]
MASKS = {3: [1, 0, 1], 2: [0, 1]}


def _mha(C, heads, g):
    HD = heads * 32
    return (torch.randn(C, 3 * HD, generator=g, dtype=F64) / C ** 0.5, torch.randn(3 * HD, generator=g, dtype=F64) * 0.2,
            torch.randn(HD, C, generator=g, dtype=F64) / HD ** 0.5, torch.randn(C, generator=g, dtype=F64) * 0.2)


def _rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@pytest.mark.parametrize('shape', SHAPES, ids=str)
@pytest.mark.parametrize('biased', [False, True])
def test_masked_softmax_is_the_present_block_and_leaves_the_rest_alone(shape, biased):
    B, Fr, H, W, C, heads = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, Fr, H, W, C, generator=g, dtype=F64)
    w = _mha(C, heads, g)
    bias = PB.bias_table(torch.randn(32, heads, generator=g, dtype=F64), Fr) if biased else None
    focus = torch.tensor(MASKS[B])
    br, y = FR.attention_block_focus(x, *w, focus, bias=bias, heads=heads)
    pr, yp = FR.present_block(x, *w, heads=heads)
    plain, _ = PB.attention_block_bias(x, *w, bias, heads, True)
    for b in range(B):
        if focus[b]:
            assert (br[b] - pr[b]).abs().max().item() <= 1e-12                 # masked softmax == out(v): the bias has no effect there
            assert _rel(br[b], plain[b]) > 0.4                                  # ... and the mask moves the branch by most of its norm
        else:
            assert torch.equal(br[b], plain[b])                                 # unmasked samples: the unmasked block, bit for bit
    # all-present: every sample
    ball, _ = FR.attention_block_focus(x, *w, torch.ones(1), bias=bias, heads=heads)
    assert (ball - pr).abs().max().item() <= 1e-12
    # emulated rounding points: O == rd(v) exactly for a masked sample
    be, _ = FR.attention_block_focus(x, *w, focus, bias=bias, heads=heads, emulate=True)
    pe, _ = FR.present_block(x, *w, heads=heads, emulate=True)
    for b in range(B):
        if focus[b]:
            assert torch.equal(be[b], pe[b])


def test_wrong_sample_fault_is_caught_by_the_tightest_gpu_bound():
    """The 'next_sample' fault (sample b masked by the flag of b + 1) moves the branch by far more than any bound test_gpu_focus.py uses
    (the widest is 4e-2 on bf16 tensors; the case must move it by more than 10 x that)."""
    for shape in SHAPES:
        B, Fr, H, W, C, heads = shape
        g = torch.Generator().manual_seed(sum(shape))
        x = torch.randn(B, Fr, H, W, C, generator=g, dtype=F64)
        w = _mha(C, heads, g)
        focus = torch.tensor(MASKS[B])
        good, _ = FR.attention_block_focus(x, *w, focus, heads=heads)
        bad, _ = FR.attention_block_focus(x, *w, focus, heads=heads, fault='next_sample')
        wrong = [b for b in range(B) if focus[b] != focus[(b + 1) % B]]
        assert wrong
        for b in wrong:
            assert _rel(bad[b], good[b]) > 10 * 4e-2, (shape, b)


def test_core_backward_closed_form_matches_autograd_and_is_exact_on_masked_samples():
    B, Fr, HW, heads = 3, 6, 4, 8
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B * Fr * HW, 3 * heads * 32, generator=g, dtype=F64).requires_grad_(True)
    d_o = torch.randn(B * Fr * HW, heads * 32, generator=g, dtype=F64)
    bias = torch.randn(heads, Fr, Fr, generator=g, dtype=F64).requires_grad_(True)
    focus = torch.tensor([1, 0, 1])
    s = qkv.reshape(B, Fr, HW, 3, heads, 32).permute(0, 2, 1, 3, 4, 5)
    q, k, v = s[..., 0, :, :] / 32 ** 0.5, s[..., 1, :, :], s[..., 2, :, :]
    S = torch.einsum('bsihd,bsjhd->bshij', q, k) + bias
    S = torch.where((focus != 0).reshape(B, 1, 1, 1, 1) & ~torch.eye(Fr, dtype=torch.bool), torch.full_like(S, FR.NEG), S)
    o = torch.einsum('bshij,bsjhd->bsihd', torch.softmax(S, -1), v)
    o_rows = o.permute(0, 2, 1, 3, 4).reshape(-1, heads * 32)
    gq, gb = torch.autograd.grad(o_rows, (qkv, bias), d_o)
    o_c, dqkv_c, db_c = FR.attn_core_focus(qkv.detach(), d_o, focus, B, Fr, HW, heads, bias=bias.detach())
    assert torch.allclose(o_c, o_rows.detach(), atol=1e-12) and torch.allclose(dqkv_c, gq, atol=1e-12) and torch.allclose(db_c, gb, atol=1e-12)
    HD = heads * 32
    rows = torch.arange(B * Fr * HW).reshape(B, Fr * HW)
    for b in (0, 2):
        r = rows[b]
        assert (dqkv_c[r, :2 * HD] == 0).all() and torch.equal(dqkv_c[r, 2 * HD:], d_o[r]) and torch.equal(o_c[r], qkv.detach()[r, 2 * HD:])
    # dBias comes from the unmasked sample alone
    _, _, db1 = PB.attn_core_bias(qkv.detach()[rows[1]], d_o[rows[1]], bias.detach(), 1, Fr, HW, heads, True)
    assert torch.allclose(db_c, db1, atol=1e-12)


def test_patched_network_masks_nine_blocks_and_not_the_init_block():
    cfg = R.UnetConfig(dim=16, channels=1, dim_mults=(1, 2))
    p = R.random_params(cfg, seed=3, dtype=F64)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 1, 4, 8, 8, generator=g, dtype=F64)
    t = torch.tensor([3, 500, 900])
    plain = R.unet_forward(p, cfg, x, t)
    assert torch.equal(FR.unet_forward_focus(p, cfg, x, t, torch.zeros(3)), plain)
    y = FR.unet_forward_focus(p, cfg, x, t, torch.tensor([1, 0, 1]))
    assert torch.equal(y[1], plain[1])                     # samples do not mix: the unmasked one is the unpatched oracle's
    assert _rel(y[0], plain[0]) > 1e-3 and _rel(y[2], plain[2]) > 1e-3
    with FR.patched(torch.tensor([1, 0, 1]), fault='init_too'):
        y_init = R.unet_forward(p, cfg, x, t)
    assert _rel(y_init[0], y[0]) > 1e-3                     # masking the init block too is a different network
    # the all-present network through the oracle's own stand-alone semantics: out(v) in every one of the nine blocks
    seen = []
    real = FR.temporal_attention_focus(torch.ones(1))

    def spy(pp, prefix, xx, dh):
        seen.append(prefix)
        return real(pp, prefix, xx, dh)
    from unittest import mock
    with mock.patch.object(R, 'temporal_attention', spy):
        R.unet_forward(p, cfg, x, t)
    assert len(seen) == 2 + 2 * len(cfg.dim_mults) and seen[0] == 'init_temporal_attn'


def test_mask_draw_and_key_independence():
    from video_diffusion_nnx_amd import train_step as TS
    assert TS.focus_present_draw(7, 0.0).sum() == 0 and TS.focus_present_draw(7, 1.0).sum() == 7
    g1, g2 = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    a, b = TS.focus_present_draw(64, 0.5, g1), TS.focus_present_draw(64, 0.5, g2)
    assert torch.equal(a, b) and a.dtype == torch.uint8 and 10 < int(a.sum()) < 54
    with pytest.raises(ValueError):
        TS.focus_present_draw(4, 1.5)
    keys = set()
    for seed, rank, step, j in ((0, 0, 0, 0), (0, 0, 1, 0), (0, 1, 0, 0), (3, 0, 0, 0), (0, 0, 0, 1), (0, 0, 5, 2)):
        t_key, noise_key = TS.micro_step_keys(seed, rank, step, j)
        four = {t_key, noise_key, TS.frame_cond_key(seed, rank, step, j), TS.cond_drop_key(seed, rank, step, j)}
        k = TS.focus_present_key(seed, rank, step, j)
        assert len(four) == 4 and k not in four, (seed, rank, step, j)
        keys.add(k)
    assert len(keys) == 6                                   # ... and it moves with seed, rank, step and micro-step


def _capture_unet(monkeypatch):
    from video_diffusion_nnx_amd import unet3d
    seen = {}
    real = unet3d.Unet3D

    def fake(*a, **kw):
        seen.update(kw)
        return real(*a, **{**kw, 'device': 'cpu'})

    monkeypatch.setattr(unet3d, 'Unet3D', fake)
    return seen


def test_yaml_keys_and_flags(monkeypatch, tmp_path):
    import sample
    import train
    from video_diffusion_nnx_amd.trainer import Trainer
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'configs', 'config_v2_2.yaml')) as fh:
        cfg = yaml.safe_load(fh)
    seen = _capture_unet(monkeypatch)
    assert 'focus_present' not in cfg['unet'] and 'prob_focus_present' not in cfg['trainer']
    unet, _ = sample.build_models(cfg, 'bf16')
    assert seen['focus_present'] is False and unet.focus_present is False                  # absent = off
    cfg['unet']['focus_present'] = True
    unet, _ = sample.build_models(cfg, 'bf16')
    assert seen['focus_present'] is True and unet.focus_present is True
    cfg['unet']['focus_present'] = False
    sample.build_models(cfg, 'bf16', focus_present=True)                                    # the flag
    assert seen['focus_present'] is True
    assert sample.build_parser().parse_args(['--random-init', '--focus-present']).focus_present is True
    assert sample.build_parser().parse_args(['--random-init']).focus_present is False
    assert any(f == '--focus_present' and kw.get('action') == 'store_true' for f, kw in train.FLAGS)
    assert any(f == '--prob_focus_present' for f, _ in train.FLAGS)
    # train.py hands the flag to build_models and the probability (flag or YAML) to the Trainer
    calls = []
    monkeypatch.setattr(sample, 'build_models', lambda c, mode, **kw: (calls.append(kw), (None, None))[1])

    class Stop(Exception):
        pass

    def stop(*a, **kw):
        raise Stop()
    monkeypatch.setattr(Trainer, '__init__', stop)
    monkeypatch.setattr(Trainer, 'prob_focus_present', 0.0)
    path = tmp_path / 'c.yaml'
    path.write_text(yaml.safe_dump(cfg))
    with pytest.raises(Stop):
        train.main(['--config', str(path), '--focus_present', '--prob_focus_present', '0.25'])
    assert calls[-1].get('focus_present') is True and Trainer.prob_focus_present == 0.25
    monkeypatch.setattr(Trainer, 'prob_focus_present', 0.0)
    with pytest.raises(Stop):
        train.main(['--config', str(path)])
    assert 'focus_present' not in calls[-1] and Trainer.prob_focus_present == 0.0
    with pytest.raises(SystemExit):
        train.main(['--config', str(path), '--prob_focus_present', '0.25'])                 # needs the switch
    cfg['unet']['focus_present'] = True
    cfg['trainer']['prob_focus_present'] = 0.5
    path.write_text(yaml.safe_dump(cfg))
    with pytest.raises(Stop):
        train.main(['--config', str(path)])
    assert Trainer.prob_focus_present == 0.5


def test_python_errors_and_resolution():
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.unet3d import Unet3D
    with pytest.raises(ValueError):
        Unet3D(dim=16, rngs=0, channels=1, device='cpu', mode='bf16', attn_fp8=True, focus_present=True)
    u = Unet3D(dim=16, rngs=0, channels=1, device='cpu')
    assert u.focus_present is False
    assert u.resolve_focus(3, torch.tensor([1, 0, 1]), 1.0) is None                          # off: accepted and ignored
    u.focus_present = True
    assert u.resolve_focus(3) is None and u.resolve_focus(3, None, 0.0) is None
    assert u.resolve_focus(3, None, 1.0) is True
    m = u.resolve_focus(6, torch.tensor([True, False, True]), 0.0)                            # a [B] mask serves 2B rows; the mask wins over p
    assert m.dtype == torch.uint8 and m.tolist() == [1, 0, 1]
    drawn = u.resolve_focus(64, None, 0.5, torch.Generator().manual_seed(1))
    assert drawn.shape == (64,) and 0 < int(drawn.sum()) < 64
    with pytest.raises(ValueError):
        u.resolve_focus(3, torch.tensor([1, 0]))                                              # wrong length
    with pytest.raises(ValueError):
        u.resolve_focus(3, torch.ones(3, 1))
    u.attn_fp8 = True
    with pytest.raises(ValueError):
        u.apply_activation_storage(u._layout_handle)
    u.attn_fp8 = False
    gd = GaussianDiffusion(u, image_size=16, num_frames=4, channels=1, timesteps=4)
    video = torch.zeros(1, 1, 4, 16, 16)
    with pytest.raises(ValueError):
        gd.inpaint(0, video, torch.tensor([1, 0, 0, 0]), focus_present=True)
    with pytest.raises(ValueError):
        gd.extend(0, video[:, :, :2], 2, focus_present=True)
    # no new parameter, no new checkpoint key
    assert [n for n, _, _ in u.param_table] == [n for n, _, _ in Unet3D(dim=16, rngs=0, channels=1, device='cpu', focus_present=True).param_table]


def test_c_abi_setter_errors_without_a_gpu():
    """vdx_set_focus_present's argument and state checks come before any device work: a bad mode, mode 2 without a mask and more than 64
    frames are VDX_ERR_INVALID (-1); mode 0 is always accepted; a valid request on a handle made without a GPU is VDX_ERR_STATE (-4)."""
    from video_diffusion_nnx_amd import unet3d as U
    u = U.Unet3D(dim=16, rngs=0, channels=1, device='cpu')
    h = u.handle(4, 16)
    assert U.vdx_get_focus_present(h.ptr) == 0
    assert U.vdx_set_focus_present(h.ptr, 0, None, 0) == 0
    assert U.vdx_set_focus_present(h.ptr, 3, None, 0) == -1
    assert U.vdx_set_focus_present(h.ptr, 2, None, 2) == -1
    assert U.vdx_set_focus_present(h.ptr, 2, 4096, 0) == -1
    if not torch.cuda.is_available():
        assert U.vdx_set_focus_present(h.ptr, 1, None, 0) == -4
    assert U.vdx_set_focus_present(u.handle(65, 16).ptr, 1, None, 0) == -1
    assert U.vdx_get_focus_present(h.ptr) == 0
