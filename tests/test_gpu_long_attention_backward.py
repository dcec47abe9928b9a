"""Backward of the bottleneck spatial attention over MORE than 64 tokens (csrc/attn_long_bwd.hip: stats -> dkv -> dq, exact fp32 on
the matrix cores in every mode), served for multiples of 64 up to 640 tokens: the core through ops.attention_core_backward /
attention_core_backward_io, the whole-network gradients of a two-level UNet at 32 x 32 (16 x 16 = 256 tokens in the bottleneck) against
fp64 autograd through the oracle, their bit reproducibility, and one train step against the oracle's.

Inputs of the core are bf16-representable (as in test_gpu_backward_forms.py), the reference is the fp64 closed form of tests/_parity.py
(tests/test_host_long_attention.py pins the tiled algebra to it and shows that a dropped key tile is more than 4000x above the per-sequence bound).
Bounds: the project's figure for the exact-fp32 core (test_gpu_conv_backward.py: o 1e-5, dq / dk / dv 2e-5 rel-L2), also per sequence and
per (sequence, head).  The closed form evaluated in fp32 on the CPU is at 2.3e-7 .. 3.6e-7 on these inputs (peaked case: 4.4e-7 / 1.2e-6),
so the bounds leave 16x .. 50x over plain fp32 round-off."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _bwd_parity_routes as BR
import _parity as P
from _launch_hook import assert_launches, launches, nan_outputs
from oracle import philox_ref, train_ref, unet3d_ref as R
from oracle.diffusion_ref import DiffusionRef

DEV = 'cuda:0'
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
SENTINEL = -768.0
PAD = 64
TOL_O, TOL_G = 1e-5, 2e-5
NEW = ['attn_long_bwd_stats_kernel', 'attn_long_bwd_dkv_kernel', 'attn_long_bwd_dq_kernel']

# (B, Fr, H, W, heads): 128 tokens = two tiles; 256 = the network's own count, 6 sequences; 576 = an odd number of tiles, 2 heads; 640 = the cap
CASES = [(1, 2, 8, 16, 8), (2, 3, 16, 16, 8), (1, 2, 24, 24, 2), (1, 1, 20, 32, 4)]


def _dev(t, dtype=F32):
    return t.detach().to(dtype).to(DEV).contiguous()


@functools.lru_cache(maxsize=None)
def _case(B, Fr, H, W, heads, peaked=False):
    g = torch.Generator().manual_seed(B + Fr + H)
    npix, HD = B * Fr * H * W, heads * 32
    qkv = torch.randn(npix, 3 * HD, generator=g)
    d_o = P.bf16r(torch.randn(npix, HD, generator=g))
    if peaked:
        qkv[:, :HD] *= 16.0                       # logits up to about +-99: exp overflows fp32 without the running maximum
    qkv = P.bf16r(qkv)
    o_ref, g_ref = P.attn_core(qkv, d_o, B, Fr, H * W, heads, False)
    return qkv, d_o, o_ref, g_ref


def _seq_head(t, nseq, L, heads):
    """[rows][parts * heads * 32] -> [nseq, heads, L * parts * 32]"""
    return t.reshape(nseq, L, -1, heads, 32).permute(0, 3, 1, 2, 4).reshape(nseq, heads, -1)


def _judge(o, dqkv, o_ref, g_ref, B, Fr, L, heads, what):
    HD, nseq = heads * 32, B * Fr
    o, dqkv = o.cpu().double(), dqkv.cpu().double()
    assert torch.isfinite(o).all() and torch.isfinite(dqkv).all(), what + ': an output element was not written'
    ro, rg = P.rel(o, o_ref), P.rel(dqkv, g_ref)
    parts = {nm: P.rel(dqkv[:, a * HD:(a + 1) * HD], g_ref[:, a * HD:(a + 1) * HD]) for a, nm in enumerate(('dq', 'dk', 'dv'))}
    print(f'[long attn] {what}: o {ro:.3e} (bound {TOL_O:.0e}), dq|dk|dv {rg:.3e}, ' + ', '.join(f'{k} {v:.3e}' for k, v in parts.items()) + f' (bound {TOL_G:.0e})')
    assert ro < TOL_O and rg < TOL_G, what
    for nm, r in parts.items():
        assert r < TOL_G, (what, nm, r)
    seq = lambda t: t.reshape(nseq, -1)
    P.assert_groups(seq(o), seq(o_ref), (nseq,), TOL_G, what + ' o per sequence')
    P.assert_groups(seq(dqkv), seq(g_ref), (nseq,), TOL_G, what + ' dq|dk|dv per sequence')
    P.assert_groups(_seq_head(o, nseq, L, heads), _seq_head(o_ref, nseq, L, heads), (nseq, heads), TOL_G, what + ' o per (sequence, head)')
    P.assert_groups(_seq_head(dqkv, nseq, L, heads), _seq_head(g_ref, nseq, L, heads), (nseq, heads), TOL_G, what + ' dq|dk|dv per (sequence, head)')


def _expect(L, nseq, heads):
    return [(k, [f'L{L} nseq{nseq} heads{heads}']) for k in NEW]


def _run_core(case, peaked=False):
    from video_diffusion_nnx_amd import ops
    B, Fr, H, W, heads = case
    L, HD, npix = H * W, heads * 32, B * Fr * H * W
    qkv, d_o, o_ref, g_ref = _case(*case, peaked)
    what = f'{case}{" peaked" if peaked else ""}'
    with launches() as rec, nan_outputs():
        o, dq, dk, dv = ops.attention_core_backward(_dev(qkv), _dev(d_o), B, Fr, H, W, heads, False)
        torch.cuda.synchronize()
    assert_launches(rec, _expect(L, B * Fr, heads), what)
    BR.assert_chain(BR.cid('long', case, 'separate'), rec)
    assert 'attn_core_bwd_kernel' not in [k for k, _ in rec]
    _judge(o, torch.cat([dq, dk, dv], dim=1), o_ref, g_ref, B, Fr, L, heads, what + ' separate')
    for pad in (0, PAD):
        with launches() as rec, nan_outputs():
            o, dqkv = ops.attention_core_backward_io(_dev(qkv), _dev(d_o), B, Fr, H, W, heads, False,
                                                     sentinel=SENTINEL if pad else None, pad_cols=pad)
            torch.cuda.synchronize()
        assert_launches(rec, _expect(L, B * Fr, heads), what)
        BR.assert_chain(BR.cid('long', case, 'io', pad), rec)
        dqkv = dqkv.cpu()
        if pad:
            assert torch.equal(dqkv[:, 3 * HD:], torch.full((npix, pad), SENTINEL)), what + ': columns behind dq|dk|dv were written'
        _judge(o, dqkv[:, :3 * HD], o_ref, g_ref, B, Fr, L, heads, what + f' interleaved pad={pad}')


@pytest.mark.parametrize('case', CASES)
def test_core(case):
    _run_core(case)


def test_core_peaked_softmax():
    _run_core(CASES[1], peaked=True)


def test_core_is_bit_reproducible():
    from video_diffusion_nnx_amd import ops
    B, Fr, H, W, heads = CASES[1]
    qkv, d_o, _, _ = _case(*CASES[1])
    q, d = _dev(qkv), _dev(d_o)
    runs = []
    for _ in range(3):
        with nan_outputs():
            runs.append([t.clone() for t in ops.attention_core_backward(q, d, B, Fr, H, W, heads, False)])
    torch.cuda.synchronize()
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            assert torch.equal(a, b)


def test_unserved_lengths_are_rejected_before_any_launch():
    from video_diffusion_nnx_amd import ops
    from video_diffusion_nnx_amd._lib import VdxError
    z = lambda rows, cols, dt=F32: torch.zeros(rows, cols, dtype=dt, device=DEV)

    def refused(fn, what, rule):
        with launches() as rec:
            with pytest.raises(VdxError, match=rule):            # the message names the rule
                fn()
        assert rec == [], (what, rec)

    for B, Fr, H, W, temporal, what, rule in [(1, 1, 12, 12, False, '144 tokens', 'multiples of 64 up to 640'), (1, 1, 22, 32, False, '704 tokens', 'multiples of 64 up to 640'),
                                              (1, 128, 2, 2, True, '128 frames', 'more than 64 frames')]:
        rows = B * Fr * H * W
        refused(lambda: ops.attention_core_backward(z(rows, 768), z(rows, 256), B, Fr, H, W, 8, temporal), what, rule)
        refused(lambda: ops.attention_core_backward_io(z(rows, 768), z(rows, 256), B, Fr, H, W, 8, temporal), what + ' (interleaved)', rule)
    rows = 2 * 8 * 16
    refused(lambda: ops.attention_core_backward_io(z(rows, 768, BF), z(rows, 256, BF), 1, 2, 8, 16, 8, False), 'bf16 tensors at 128 tokens', 'bf16 tensors need')
    refused(lambda: ops.attention_core_backward_bias(z(rows, 768), z(rows, 256), torch.zeros(8, 128, 128), 1, 2, 8, 16, 8, False), 'bias form at 128 tokens', 'at most 64 tokens')
    refused(lambda: ops.attention_core_backward_focus(z(rows, 768), z(rows, 256), [1], 1, 2, 8, 16, 8, False), 'focus form at 128 tokens', 'at most 64 tokens')


def test_64_tokens_keep_their_kernel():
    from video_diffusion_nnx_amd import ops
    B, Fr, H, W, heads = 1, 2, 8, 8, 8
    g = torch.Generator().manual_seed(B + Fr + H)
    npix, HD = B * Fr * H * W, heads * 32
    qkv, d_o = P.bf16r(torch.randn(npix, 3 * HD, generator=g)), P.bf16r(torch.randn(npix, HD, generator=g))
    o_ref, g_ref = P.attn_core(qkv, d_o, B, Fr, H * W, heads, False)
    with launches() as rec, nan_outputs():
        o, dq, dk, dv = ops.attention_core_backward(_dev(qkv), _dev(d_o), B, Fr, H, W, heads, False)
        torch.cuda.synchronize()
    assert_launches(rec, [('attn_core_bwd_kernel', ['L64 nseq2 heads8'])], '64 tokens')
    BR.assert_chain(BR.cid('long', '64 tokens'), rec)
    assert P.rel(o.cpu(), o_ref) < TOL_O and P.rel(torch.cat([dq, dk, dv], dim=1).cpu(), g_ref) < TOL_G


# ---- the network: dim 16, two levels, 32 x 32 frames -> a 16 x 16 = 256-token bottleneck over 4 sequences ------------------------------

NET_KW = dict(dim=16, channels=1, dim_mults=(1, 2))
NET_SHAPE = (2, 1, 2, 32, 32)


def _rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@functools.lru_cache(maxsize=None)
def _net_ref():
    cfg = R.UnetConfig(**NET_KW)
    p64 = R.random_params(cfg, seed=7, dtype=F64)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(*NET_SHAPE, generator=g)
    t = torch.randint(0, 1000, (NET_SHAPE[0],), generator=g)
    leaves = {k: v.clone().requires_grad_(True) for k, v in p64.items()}
    ref_out = R.unet_forward(leaves, cfg, x.double(), t)
    d_out = torch.randn(ref_out.shape, generator=g)
    ref = torch.autograd.grad(ref_out, list(leaves.values()), d_out.double(), allow_unused=True)
    ref_grads = {k: (torch.zeros_like(v) if gr is None else gr) for (k, v), gr in zip(leaves.items(), ref)}
    return p64, x, t, d_out, ref_grads


@pytest.mark.parametrize('mode,tol', [('f32', 2e-4), ('bf16', 6e-2), ('bf16+act16', 7e-2)])
def test_unet_backward_parity_256_token_bottleneck(mode, tol):
    from video_diffusion_nnx_amd.unet3d import Unet3D
    p64, x, t, d_out, ref_grads = _net_ref()
    m = Unet3D(rngs=0, mode=mode.split('+')[0], **NET_KW)
    m.load_state_dict({k: v.float() for k, v in p64.items()})
    m.act_bf16 = 2 if mode.endswith('+act16') else False
    y = m(x, t)
    assert y.shape == d_out.shape
    grads = torch.zeros_like(m.flat_params)
    ns = m.num_stages
    with launches() as rec:                          # the reverse pass in three pieces (the staged interface)
        m.backward(d_out.to(m.device), grads, ns - 1, ns - 1)
        m.backward(d_out.to(m.device), grads, ns - 2, 2)
        m.backward(d_out.to(m.device), grads, 1, 0)
        torch.cuda.synchronize()
    assert [(k, s) for k, s in rec if k in NEW] == [(k, 'L256 nseq4 heads8') for k in NEW], [r for r in rec if r[0].startswith('attn_')]
    rows = []
    for name, shape, off in m.param_table:
        got = grads[off:off + int(np.prod(shape))].cpu().double().reshape(shape)
        ref = ref_grads[name].double()
        rows.append((name, _rel(got, ref), ref.norm().item(), got.norm().item()))
    total_ref = torch.cat([ref_grads[n].reshape(-1) for n, _, _ in m.param_table])
    total_got = torch.cat([grads[o:o + int(np.prod(s))].cpu().double() for _, s, o in m.param_table])
    scale = total_ref.norm().item()
    bad = [(n, r) for n, r, nr, ng in rows if nr > 1e-6 * scale and r > tol * 5]
    dead = [(n, ng) for n, r, nr, ng in rows if nr <= 1e-6 * scale and ng > 1e-4 * scale]
    exact = [(n, ng) for n, r, nr, ng in rows if ('.fn.norm.' in n or n.startswith('time_rel_pos_bias')) and ng != 0.0]
    assert not exact, f'dead parameters received gradient: {exact[:5]}'
    assert not dead, f'zero-gradient parameters received a large gradient: {dead[:5]}'
    assert not bad, f'{mode}: worst per-tensor gradients {sorted(bad, key=lambda z: -z[1])[:6]}'
    rt = _rel(total_got, total_ref)
    proj = [(n, r) for n, r, _, _ in rows if n.startswith('mid_spatial_attn') and n.endswith('.kernel')]
    print(f'network gradients, 256-token bottleneck, {mode}: all {rt:.3e} (bound {tol:.0e}); ' + ', '.join(f'{n} {r:.3e}' for n, r in proj))
    assert len(proj) == 4, [n for n, _, _ in m.param_table if n.startswith('mid_spatial_attn')]
    if mode == 'f32':
        for n, r in proj:
            assert r < tol, (n, r)
    assert rt < tol, rt


@pytest.mark.parametrize('mode', ['f32', 'bf16', 'bf16+act16'])
def test_backward_is_bit_reproducible_256_token_bottleneck(mode):
    from video_diffusion_nnx_amd.unet3d import Unet3D
    m = Unet3D(rngs=5, mode=mode.split('+')[0], **NET_KW)
    m.act_bf16 = 2 if mode.endswith('+act16') else False
    g = torch.Generator().manual_seed(4)
    x = torch.randn(*NET_SHAPE, generator=g)
    t = torch.randint(0, 1000, (NET_SHAPE[0],), generator=g)
    y = m(x, t)
    d_out = torch.randn(y.shape, generator=g).to(m.device)
    ns = m.num_stages
    runs = []
    for i in range(3):
        grads = torch.full_like(m.flat_params, float(i))          # (the head stage zeroes the buffer)
        if i == 1:
            m.backward(d_out, grads, ns - 1, ns - 2)
            m.backward(d_out, grads, ns - 3, 0)
        else:
            m.backward(d_out, grads)
        torch.cuda.synchronize()
        runs.append(grads.clone())
    assert torch.isfinite(runs[0]).all() and runs[0].abs().max() > 0
    for i in (1, 2):
        diff = (runs[i] != runs[0]).sum().item()
        assert diff == 0, f'{mode}: run {i} differs from run 0 in {diff} of {runs[0].numel()} gradient elements'


def _mk(tmp_path, mode):
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.trainer import Trainer
    from video_diffusion_nnx_amd.unet3d import Unet3D
    unet = Unet3D(rngs=1, mode=mode, **NET_KW)
    gd = GaussianDiffusion(unet, image_size=32, num_frames=2, channels=1, timesteps=50, loss_type='l2')
    tr = Trainer(gd, str(tmp_path), dataset_path='synthetic:8', train_batch_size=2, train_num_steps=3, train_lr=1e-3,
                 checkpoint_every_steps=2, results_folder=str(tmp_path / 'res'), step_start_ema=0, update_ema_every=1, ema_decay=0.9)
    return unet, gd, tr


def test_one_train_step_matches_oracle_32px(tmp_path):
    unet, gd, tr = _mk(tmp_path, 'f32')
    cfg = R.UnetConfig(**NET_KW)
    p0 = {k: v.detach().cpu().double().clone() for k, v in unet.state_dict().items()}
    g = torch.Generator().manual_seed(0)
    batch = torch.rand(*NET_SHAPE, generator=g)
    loss_dev = tr.train_step(batch, step=0)
    torch.cuda.synchronize()
    t = tr.last_t.cpu().long()
    noise = torch.from_numpy(philox_ref.randn(batch.numel(), tr.last_noise_key, 0)).double().reshape(batch.shape)

    def loss_fn(params):
        ref = DiffusionRef(lambda a, b: R.unet_forward(params, cfg, a, b), image_size=32, num_frames=2, channels=1, timesteps=50,
                           loss_type='l2', dtype=F64)
        return ref.loss(batch.double(), t, noise)
    ref_loss, grads = train_ref.loss_and_grads(p0, loss_fn)
    assert abs(loss_dev.item() - ref_loss.item()) < 2e-5 * max(1.0, abs(ref_loss.item()))
    zeros = {k: torch.zeros_like(v) for k, v in p0.items()}
    lr = train_ref.lr_schedule(0, 1e-3)
    p1, m1, v1 = train_ref.adam_update(p0, grads, zeros, zeros, count=0, lr=lr)
    ema1 = train_ref.ema_update(p0, p1, step=0, step_start_ema=0, update_ema_every=1, decay=0.9)
    got = {k: v.detach().cpu().double() for k, v in unet.state_dict().items()}
    # Adam's first step is lr * sign(g) (|update| = lr): compare the UPDATE, tolerating sign flips of ~zero gradients
    num = sum(((got[k] - p0[k]) - (p1[k] - p0[k])).pow(2).sum() for k in p0)
    den = sum((p1[k] - p0[k]).pow(2).sum() for k in p0)
    assert (num / den).sqrt().item() < 2e-2, (num / den).sqrt().item()
    ema_got = {n: tr.ema[o:o + int(np.prod(s))].cpu().double().reshape(s) for n, s, o in unet.param_table}
    num = sum((ema_got[k] - ema1[k]).pow(2).sum() for k in p0)
    den = sum((ema1[k] - p0[k]).pow(2).sum() for k in p0)
    assert (num / den).sqrt().item() < 2e-2
    assert tr.opt_count == 1


def test_two_bf16_train_steps_32px(tmp_path):
    """bf16 operands + bf16 activation storage (Trainer's default for a bf16-mode network): two steps, finite loss and parameters."""
    unet, gd, tr = _mk(tmp_path, 'bf16')
    assert tr.train_act_bf16
    g = torch.Generator().manual_seed(0)
    for step in range(2):
        loss = tr.train_step(torch.rand(*NET_SHAPE, generator=g), step=step)
        assert np.isfinite(loss.item())
    torch.cuda.synchronize()
    assert torch.isfinite(unet.flat_params).all() and tr.opt_count == 2
