"""CPU tests of the temporal relative position bias (Unet3D(temporal_pos_bias=True)): the host's bucket map against the
oracle's, the patched fp64 reference (tests/_posbias_ref.py) and the symmetry it breaks, the sensitivity of the emulation the GPU tests
lean on, and the CLI / YAML plumbing."""
import os
import sys

import pytest
import torch
import yaml

import _posbias_ref as PB
from oracle import unet3d_ref as R

F64 = torch.float64


def test_bucket_map_equals_the_oracle():
    from video_diffusion_nnx_amd.unet3d import relative_position_buckets
    for n in range(1, 65):
        got = relative_position_buckets(n)
        assert got.dtype == torch.int64 and got.shape == (n, n)
        assert torch.equal(got, PB.buckets_ref(n)), n
        assert int(got.min()) >= 0 and int(got.max()) < 32


def test_bucket_map_known_answers():
    from video_diffusion_nnx_amd.unet3d import relative_position_buckets
    b = relative_position_buckets(16)
    future = [0, 1, 2, 3, 4, 5, 6, 7, 8, 8, 8, 8, 9, 9, 9, 9]          # key j = i + offset: offsets 0..7 exact, 8..11 -> 8, 12..15 -> 9
    assert b[0].tolist() == future
    assert b[:, 0].tolist() == [0] + [16 + v for v in future[1:]]      # keys in the past: + 16
    for i in range(16):
        for j in range(16):
            assert int(b[i, j]) == (future[j - i] if j >= i else 16 + future[i - j])
    assert not torch.equal(b, b.t())                                     # asymmetric between past and future keys
    # exact powers sit on a bucket boundary (one float32 ulp decides): pinned against the oracle above, named here
    b64 = relative_position_buckets(64)
    assert int(b64[0, 16]) == int(PB.buckets_ref(64)[0, 16]) and int(b64[32, 0]) == int(PB.buckets_ref(64)[32, 0])


def _tiny(seed=0, frames=5):
    cfg = R.UnetConfig(dim=16, channels=1)
    p = R.random_params(cfg, seed, dtype=F64)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(1, 1, frames, 16, 16, generator=g, dtype=F64)
    t = torch.tensor([7])
    return cfg, p, x, t


def test_patched_reference_with_zero_embedding_is_the_reference():
    cfg, p, x, t = _tiny()
    p = dict(p)
    p['time_rel_pos_bias.relative_attention_bias.embedding'] = torch.zeros(32, cfg.attn_heads, dtype=F64)
    assert torch.equal(PB.unet_forward_pos(p, cfg, x, t), R.unet_forward(p, cfg, x, t))
    assert R.temporal_attention is not PB.temporal_attention_pos        # the patch is gone after the call


def test_frame_permutation_equivariance_and_what_breaks_it():
    cfg, p, x, t = _tiny()
    perm = torch.tensor([3, 0, 4, 1, 2])
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()
    plain = rel(R.unet_forward(p, cfg, x[:, :, perm], t), R.unet_forward(p, cfg, x, t)[:, perm])
    biased = rel(PB.unet_forward_pos(p, cfg, x[:, :, perm], t), PB.unet_forward_pos(p, cfg, x, t)[:, perm])
    print(f'frame permutation: reference {plain:.3e}, with the position bias {biased:.3e}')
    assert plain <= 1e-12                      # the reference network cannot tell frame order
    assert biased > 1e-3                       # the biased one can


@pytest.mark.parametrize('operand,bound', [('bf16', 1.5e-2), ('f16', None)])
def test_emulation_sees_a_transposed_or_post_softmax_bias(operand, bound):
    """The GPU tests hold the biased block to TOL (bf16: 1.5e-2 of the branch) or 3 x the emulation's own distance (f16).  A kernel that
    read bias[h, j, i], or added the bias after the softmax, must land far outside: more than 10 x the bound."""
    B, Fr, H, W, C, heads = 1, 16, 3, 2, 64, 8
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, Fr, H, W, C, generator=g, dtype=F64)
    wqkv = torch.randn(C, 3 * heads * 32, generator=g, dtype=F64) / C ** 0.5 * 2
    bqkv = torch.randn(3 * heads * 32, generator=g, dtype=F64) * 0.2
    wo = torch.randn(heads * 32, C, generator=g, dtype=F64) / (heads * 32) ** 0.5
    bo = torch.randn(C, generator=g, dtype=F64) * 0.2
    bias = PB.bias_table(torch.randn(32, heads, generator=g, dtype=F64), Fr)
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()
    ref, _ = PB.attention_block_bias(x, wqkv, bqkv, wo, bo, bias, heads, True)
    emu, _ = PB.attention_block_bias(x, wqkv, bqkv, wo, bo, bias, heads, True, emulate=True, operand=operand)
    if bound is None:
        bound = 3.0 * rel(emu, ref)
    assert rel(emu, ref) < bound
    for fault in ('transpose', 'post_softmax'):
        bad, _ = PB.attention_block_bias(x, wqkv, bqkv, wo, bo, bias, heads, True, emulate=True, operand=operand, fault=fault)
        print(f'{operand} {fault}: {rel(bad, ref):.3e} against bound {bound:.3e}')
        assert rel(bad, ref) > 10 * bound, (fault, rel(bad, ref), bound)
    none, _ = PB.attention_block_bias(x, wqkv, bqkv, wo, bo, None, heads, True)
    assert rel(none, ref) > 10 * bound          # and a kernel that ignored the bias


def test_core_backward_helper_is_its_own_autograd():
    """attn_core_bias's closed forms (o, dq|dk|dv, dBias) against autograd of the forward they claim to differentiate."""
    B, Fr, HW, heads = 2, 5, 3, 4
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B * Fr * HW, 3 * heads * 32, generator=g, dtype=F64).requires_grad_(True)
    d_o = torch.randn(B * Fr * HW, heads * 32, generator=g, dtype=F64)
    bias = torch.randn(heads, Fr, Fr, generator=g, dtype=F64).requires_grad_(True)
    s = qkv.reshape(B, Fr, HW, 3, heads, 32).permute(0, 2, 1, 3, 4, 5)
    q, k, v = s[..., 0, :, :] / 32 ** 0.5, s[..., 1, :, :], s[..., 2, :, :]
    o = torch.einsum('bshij,bsjhd->bsihd', torch.softmax(torch.einsum('bsihd,bsjhd->bshij', q, k) + bias, -1), v)
    o_rows = o.permute(0, 2, 1, 3, 4).reshape(-1, heads * 32)
    gq, gb = torch.autograd.grad(o_rows, (qkv, bias), d_o)
    o_c, dqkv_c, db_c = PB.attn_core_bias(qkv.detach(), d_o, bias.detach(), B, Fr, HW, heads, True)
    assert torch.allclose(o_c, o_rows.detach(), atol=1e-12) and torch.allclose(dqkv_c, gq, atol=1e-12) and torch.allclose(db_c, gb, atol=1e-12)


def _capture_unet(monkeypatch):
    from video_diffusion_nnx_amd import unet3d
    seen = {}
    real = unet3d.Unet3D

    def fake(*a, **kw):
        seen.update(kw)
        return real(*a, **{**kw, 'device': 'cpu'})

    monkeypatch.setattr(unet3d, 'Unet3D', fake)
    return seen


def test_yaml_key_and_flags_reach_unet3d(monkeypatch, tmp_path):
    import sample
    import train
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'configs', 'config_v2_2.yaml')) as fh:
        cfg = yaml.safe_load(fh)
    seen = _capture_unet(monkeypatch)
    assert 'temporal_pos_bias' not in cfg['unet']
    unet, _ = sample.build_models(cfg, 'bf16')
    assert seen['temporal_pos_bias'] is False and unet.temporal_pos_bias is False          # absent = off
    cfg['unet']['temporal_pos_bias'] = True
    unet, _ = sample.build_models(cfg, 'bf16')
    assert seen['temporal_pos_bias'] is True and unet.temporal_pos_bias is True
    cfg['unet']['temporal_pos_bias'] = False
    unet, _ = sample.build_models(cfg, 'bf16', temporal_pos_bias=True)                      # the flag
    assert seen['temporal_pos_bias'] is True
    # each CLI in its own flag style
    assert sample.build_parser().parse_args(['--random-init', '--temporal-pos-bias']).temporal_pos_bias is True
    assert sample.build_parser().parse_args(['--random-init']).temporal_pos_bias is False
    assert any(f == '--temporal_pos_bias' and kw.get('action') == 'store_true' for f, kw in train.FLAGS)
    # train.py hands the flag to build_models
    calls = []
    monkeypatch.setattr(sample, 'build_models', lambda c, mode, **kw: (calls.append(kw), (_ for _ in ()).throw(SystemExit(0)))[1])
    path = tmp_path / 'c.yaml'
    path.write_text(yaml.safe_dump(cfg))
    for argv, want in ((['--config', str(path), '--temporal_pos_bias'], True), (['--config', str(path)], False)):
        with pytest.raises(SystemExit):
            train.main(argv)
        assert calls[-1].get('temporal_pos_bias', False) is want


def test_switch_is_keyword_only_settable_and_excludes_fp8():
    from video_diffusion_nnx_amd.unet3d import Unet3D
    u = Unet3D(dim=16, rngs=0, channels=1, device='cpu')
    assert u.temporal_pos_bias is False
    u.temporal_pos_bias = True
    assert Unet3D(dim=16, rngs=0, channels=1, device='cpu', temporal_pos_bias=True).temporal_pos_bias is True
    with pytest.raises(ValueError):
        Unet3D(dim=16, rngs=0, channels=1, device='cpu', attn_fp8=True, temporal_pos_bias=True)
    with pytest.raises(TypeError):
        Unet3D(16, 0, (1, 2, 4, 8), None, None, 1, 8, 32, False, None, 7, True, 'resnet', 8, False, 'bf16', None, False, True)
    # no new parameter, no new checkpoint key
    names = [n for n, _, _ in u.param_table]
    assert names.count('time_rel_pos_bias.relative_attention_bias.embedding') == 1
    assert names == [n for n, _, _ in Unet3D(dim=16, rngs=0, channels=1, device='cpu', temporal_pos_bias=True).param_table]


def test_train_step_bounds_tell_a_wrong_embedding_gradient():
    """The bf16 bounds of tests/test_gpu_posbias.py::test_one_train_step (PB.adam_first_step_bound at the bf16 gradient tolerance) are far
    below what a wrong gradient gives: signs at random sit at sqrt(2), and the embedding's gradient with past and future keys swapped (what
    a transposed dBias scatters) flips about half of the signs that move."""
    from oracle import train_ref
    from oracle.diffusion_ref import DiffusionRef
    cfg = R.UnetConfig(dim=16, channels=1, dim_mults=(1, 2))
    p0 = R.random_params(cfg, seed=1, dtype=F64)
    g = torch.Generator().manual_seed(0)
    batch = torch.rand(2, 1, 4, 8, 8, generator=g, dtype=F64)
    noise = torch.randn(batch.shape, generator=g, dtype=F64)
    ref = lambda params: DiffusionRef(lambda a, b: PB.unet_forward_pos(params, cfg, a, b), image_size=8, num_frames=4, channels=1, timesteps=50,
                                      loss_type='l2', dtype=F64).loss(batch, torch.tensor([7, 33]), noise)
    _, grads = train_ref.loss_and_grads(p0, ref)
    emb = 'time_rel_pos_bias.relative_attention_bias.embedding'
    all_b, emb_b = PB.adam_first_step_bound(grads, 7e-2), PB.adam_first_step_bound({emb: grads[emb]}, 7e-2)
    assert 0 < all_b < 0.5 * 2 ** 0.5 and 0 < emb_b < 0.5 * 2 ** 0.5, (all_b, emb_b)      # under half of what signs at random give
    ge = grads[emb]
    swapped = torch.cat([ge[16:], ge[:16]])
    assert ((ge.sign() - swapped.sign()).norm() / ge.sign().norm()).item() > 2 * emb_b
    # a gradient inside the tolerance stays inside the bound: bf16-rounded weights move the gradient by about 1e-2
    _, g16 = train_ref.loss_and_grads({k: v.bfloat16().double() for k, v in p0.items()}, ref)
    cat = lambda d: torch.cat([d[k].reshape(-1) for k in grads])
    assert ((cat(g16) - cat(grads)).norm() / cat(grads).norm()).item() < 7e-2
    assert ((cat(g16).sign() - cat(grads).sign()).norm() / cat(grads).sign().norm()).item() < all_b
