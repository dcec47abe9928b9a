"""GPU parity of the whole Unet3D forward (C ABI vdx_unet_forward) vs oracle/unet3d_ref.py, plus the committed
golden fixtures.  Tolerances: f32 mode 2e-5 relative L2 (fp32 restatement itself is 2e-6 from fp64);
bf16 mode (bf16 MFMA operands, fp32 accumulate/storage) 2e-2."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet3d_ref as R

TOL = {'f32': 2e-5, 'bf16': 2e-2}


def _rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _build(kw, mode, seed=5):
    from video_diffusion_nnx_amd.unet3d import Unet3D
    cfg = R.UnetConfig(**kw)
    p = R.random_params(cfg, seed=seed, dtype=torch.float64)
    m = Unet3D(rngs=0, mode=mode, **kw)
    m.load_state_dict({k: v.float() for k, v in p.items()})
    return cfg, p, m


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
@pytest.mark.parametrize('kw,shape', [
    (dict(dim=16, channels=3, cond_dim=32), (1, 3, 4, 16, 16)),          # reference test_unet3d.py config
    (dict(dim=16, channels=3), (2, 3, 4, 16, 16)),
    (dict(dim=32, channels=1), (1, 1, 10, 32, 32)),                      # YAML-like: F = 10 (padded attention)
    (dict(dim=16, channels=1, dim_mults=(1, 2), use_sparse_linear_attn=False), (1, 1, 3, 8, 8)),
    (dict(dim=64, channels=1), (3, 1, 5, 32, 32)),                       # C = 256 / 512 levels with ragged sequence groups (per-head kernels)
])
def test_unet_forward_parity(mode, kw, shape):
    cfg, p, m = _build(kw, mode)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(*shape, generator=g)
    t = torch.randint(0, 1000, (shape[0],), generator=g)
    cond = torch.randn(shape[0], cfg.cond_in, generator=g) if cfg.has_cond else None
    y = m(x, t, cond=cond)
    torch.cuda.synchronize()
    taps = {}
    ref = R.unet_forward(p, cfg, x.double(), t, cond=None if cond is None else cond.double(), taps=taps)
    # per-block report (first divergence is the useful one when this fails)
    B, Fr, S = shape[0], shape[2], shape[3]
    worst = []
    for name, tv in taps.items():
        if name == 'temb':
            continue
        got = m.slot(name, B, Fr, S).cpu().double().reshape(tv.shape)
        worst.append((name, _rel(got, tv)))
    bad = [(n, r) for n, r in worst if r > TOL[mode]]
    assert not bad, f'{mode}: first diverging blocks {bad[:4]}'
    assert y.shape == ref.shape
    assert _rel(y.cpu().double(), ref) < TOL[mode]


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
@pytest.mark.parametrize('tag', ['tiny_cond', 'tiny_nocond'])
def test_golden_fixture(mode, tag):
    z = np.load(os.path.join(os.path.dirname(__file__), 'golden', f'unet_{tag}.npz'))
    kw = dict(dim=16, channels=3, cond_dim=32) if tag == 'tiny_cond' else dict(dim=16, channels=3)
    _, _, m = _build(kw, mode, seed=int(z['weight_seed']))
    cond = torch.from_numpy(z['cond']) if tag == 'tiny_cond' else None
    y = m(torch.from_numpy(z['x']), torch.from_numpy(z['t']), cond=cond)
    assert _rel(y.cpu().double(), torch.from_numpy(z['eps_fp64'])) < TOL[mode]


def test_cfg_and_cond_mask():
    cfg, p, m = _build(dict(dim=16, channels=3, cond_dim=32), 'f32')
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 3, 4, 16, 16, generator=g)
    t = torch.tensor([3, 700])
    cond = torch.randn(2, 32, generator=g)
    y = m.forward_with_cond_scale(x, t, cond=cond, cond_scale=2.0)
    ref = R.forward_with_cond_scale(p, cfg, x.double(), t, cond=cond.double(), cond_scale=2.0)
    assert _rel(y.cpu().double(), ref) < 5e-5
    mask = torch.tensor([True, False])
    y2 = m(x, t, cond=cond, cond_mask=mask)
    ref2 = R.unet_forward(p, cfg, x.double(), t, cond=cond.double(), cond_mask=mask)
    assert _rel(y2.cpu().double(), ref2) < 2e-5
    with pytest.raises(AssertionError):
        m(x, t)


def test_north_star_shape_f32_and_bf16():
    """config N (dim 64, 16f x 64 x 64, C=1), B=1: the benchmark shape, checked against the CPU restatement."""
    kw = dict(dim=64, channels=1)
    cfg = R.UnetConfig(**kw)
    p = R.random_params(cfg, seed=9, dtype=torch.float32)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 1, 16, 64, 64, generator=g)
    t = torch.tensor([500])
    ref = R.unet_forward(p, cfg, x, t).double()
    from video_diffusion_nnx_amd.unet3d import Unet3D
    for mode in ('f32', 'bf16'):
        m = Unet3D(rngs=0, mode=mode, **kw)
        m.load_state_dict(p)
        y = m(x, t)
        assert _rel(y.cpu().double(), ref) < (5e-5 if mode == 'f32' else 2e-2), mode


# ---- bf16 activation storage (vdx_set_activation_storage): what GaussianDiffusion's sampling loops use in bf16 mode ----
# Every inter-kernel activation is rounded to bf16 once per kernel boundary (~30 boundaries on the residual path), on top of
# the bf16 MFMA operands.  Stated tolerance: 3e-2 relative L2 on the eps prediction vs the fp64 oracle.
TOL_ACT16 = 3e-2


@pytest.mark.parametrize('kw,shape', [
    (dict(dim=16, channels=3, cond_dim=32), (1, 3, 4, 16, 16)),
    (dict(dim=16, channels=3), (2, 3, 4, 16, 16)),
    (dict(dim=32, channels=1), (1, 1, 10, 32, 32)),
    (dict(dim=16, channels=1, dim_mults=(1, 2), use_sparse_linear_attn=False), (1, 1, 3, 8, 8)),
    (dict(dim=64, channels=1), (3, 1, 5, 32, 32)),                       # C = 256 / 512 levels with ragged sequence groups (per-head kernels)
])
def test_unet_forward_bf16_storage(kw, shape):
    cfg, p, m = _build(kw, 'bf16')
    g = torch.Generator().manual_seed(1)
    x = torch.randn(*shape, generator=g)
    t = torch.randint(0, 1000, (shape[0],), generator=g)
    cond = torch.randn(shape[0], cfg.cond_in, generator=g) if cfg.has_cond else None
    y32 = m(x, t, cond=cond).clone()
    m.act_bf16 = True
    y16 = m(x, t, cond=cond)
    ref = R.unet_forward(p, cfg, x.double(), t, cond=None if cond is None else cond.double())
    assert _rel(y16.cpu().double(), ref) < TOL_ACT16
    assert _rel(y16.cpu().double(), y32.cpu().double()) < TOL_ACT16
    with pytest.raises(RuntimeError):
        m.slot('init_conv', shape[0], shape[2], shape[3])
    m.act_bf16 = False                                   # and back: fp32 storage again -- the forward is bit-reproducible run to run
    assert torch.equal(m(x, t, cond=cond), y32)          # (test_bf16_forward_is_bit_reproducible), so switching storage leaves no trace
    assert m.slot('init_conv', shape[0], shape[2], shape[3]).numel() > 0


def test_bf16_storage_needs_bf16_mode_and_blocks_backward():
    _, _, m = _build(dict(dim=16, channels=3), 'f32')
    m.act_bf16 = True
    with pytest.raises(ValueError):
        m(torch.randn(1, 3, 4, 16, 16), torch.tensor([5]))
    _, _, mb = _build(dict(dim=16, channels=3), 'bf16')
    mb.act_bf16 = True
    y = mb(torch.randn(1, 3, 4, 16, 16), torch.tensor([5]))
    from video_diffusion_nnx_amd._lib import VdxError
    with pytest.raises(VdxError):
        mb.backward(torch.ones_like(y), torch.zeros_like(mb.flat_params))


def test_north_star_shape_bf16_storage():
    """B = 4: 1024 level-0 tiles, so the persistent 64-channel conv kernels, the one-wave-per-head attention / SLA kernels and the
    16-byte tail all run in place, exactly as in the benchmark."""
    kw = dict(dim=64, channels=1)
    cfg = R.UnetConfig(**kw)
    p = R.random_params(cfg, seed=9, dtype=torch.float32)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(4, 1, 16, 64, 64, generator=g)
    t = torch.tensor([500, 20, 999, 0])
    ref = R.unet_forward(p, cfg, x, t).double()
    from video_diffusion_nnx_amd.unet3d import Unet3D
    m = Unet3D(rngs=0, mode='bf16', **kw)
    m.load_state_dict(p)
    m.act_bf16 = True
    assert _rel(m(x, t).cpu().double(), ref) < TOL_ACT16
    m.act_bf16 = False                                   # fp32 storage at the same batch: conv64p (fp32 inputs) and conv64q (bf16 y1) mixed
    assert _rel(m(x, t).cpu().double(), ref) < TOL['bf16']


def test_north_star_shape_bf16_storage_batch8():
    """B = 8: the tail kernels are capped at 8192 workgroups, so at this batch every workgroup of the level-0 tails walks two pixel
    passes (the multi-pass loop of resblock_tail16_kernel), and the weight-resident kernels walk longer tile ranges."""
    kw = dict(dim=64, channels=1)
    cfg = R.UnetConfig(**kw)
    p = R.random_params(cfg, seed=11, dtype=torch.float32)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(8, 1, 16, 64, 64, generator=g)
    t = torch.tensor([500, 20, 999, 0, 1, 250, 750, 998])
    idx = [0, 4, 7]                                      # the UNet is per-sample independent: three of the eight samples against the oracle
    ref = R.unet_forward(p, cfg, x[idx], t[idx]).double()
    from video_diffusion_nnx_amd.unet3d import Unet3D
    m = Unet3D(rngs=0, mode='bf16', **kw)
    m.load_state_dict(p)
    m.act_bf16 = True
    y = m(x, t).cpu().double()
    assert torch.isfinite(y).all()
    assert _rel(y[idx], ref) < TOL_ACT16


@pytest.mark.parametrize('kw,shape', [(dict(dim=16, channels=3), (2, 3, 4, 16, 16)), (dict(dim=64, channels=1), (2, 1, 16, 64, 64))])
def test_bf16_forward_is_bit_reproducible(kw, shape):
    """GroupNorm partial sums (fp32 per wave / tile) meet in f64 -- LDS and global atomics whose result does not depend on arrival
    order, since a few thousand floats add exactly in double -- so two runs of the same bf16-mode forward give identical bits, in both
    storage formats (round 1: fp32 LDS atomics, ~3e-3 run-to-run jitter at the output)."""
    cfg, p, m = _build(kw, 'bf16')
    g = torch.Generator().manual_seed(3)
    x = torch.randn(*shape, generator=g)
    t = torch.randint(0, 1000, (shape[0],), generator=g)
    for act16 in (False, True):
        m.act_bf16 = act16
        runs = [m(x, t).clone() for _ in range(3)]
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2]), f'act_bf16={act16}'
    m.act_bf16 = False
