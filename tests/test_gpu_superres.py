"""Cascaded super-resolution on the GPU (vdx.h: "Cascaded super-resolution"): the three kernels of csrc/lowres.hip against the fp64
restatement tests/_sr_ref.py and against the existing kernels they must agree with bit for bit, the forward of a channels = 2 C,
out_dim = C network against the oracle, the three captured loops against the chain stepped by hand from public pieces, and the train step
against the same step done by hand.  Bounds: stated by the contract (bit equality), by the number format (n 2^-24 for the box mean; 1e-6
for the interpolation: at most 16 roundings of values <= 1) or the project's forward bounds (4e-6 f32, 8e-3 bf16)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sr_ref as R                       # noqa: E402
from _launch_hook import launches        # noqa: E402
from oracle import unet3d_ref as U       # noqa: E402

DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
T = 10


def _dev(t, dtype=None):
    return t.detach().to(dtype or t.dtype).to(DEV).contiguous()


def _ulp32(v64):
    r = v64.float().abs()
    return (torch.nextafter(r, torch.full_like(r, float('inf'))) - r).double()


@functools.lru_cache(None)
def _tables():
    from video_diffusion_nnx_amd.gaussian_diffusion import make_tables
    t = make_tables(T)
    return _dev(torch.from_numpy(t['sqrt_alphas_cumprod'])), _dev(torch.from_numpy(t['sqrt_one_minus_alphas_cumprod']))


def _randn(shape, seed, draw):
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd.gaussian_diffusion import vdx_randn
    out = torch.empty(shape, dtype=F32, device=DEV)
    L.check(vdx_randn(L.ptr(out), out.numel(), seed, draw, 0, L.stream_ptr()))
    return out


# ---- 1. lowres_down ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('ft,fs', [(2, 2), (1, 4), (3, 3), (1, 1)])
def test_lowres_down(ft, fs):
    from video_diffusion_nnx_amd import ops
    x = R.make_lo(2, 3, 2 * ft, 3 * fs, seed=ft * 10 + fs)                 # [2,3,F,S,S] in [0, 1]; S = 9 for (3, 3)
    with launches() as rec:
        lo = ops.lowres_down(_dev(x), ft, fs)
    torch.cuda.synchronize()
    assert [k for k, _ in rec] == ['lowres_down_kernel']
    assert lo.shape == (2, 3, 2, 3, 3)
    n = ft * fs * fs
    err = (lo.cpu().double() - R.down(x, ft, fs)).abs().max().item()
    print(f'[down ({ft},{fs})] n = {n}: max |lo - fp64| = {err:.3e} (bound {n * 2.0 ** -24:.3e})')
    assert err <= n * 2.0 ** -24
    if n == 1:
        assert torch.equal(lo.cpu(), x)
    assert torch.equal(ops.lowres_down(_dev(x), ft, fs), lo)


# ---- 2. lowres_input, the second half ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def _up_ref(shape, C):
    f, s, ft, fs = shape
    lo = R.make_lo(2, C, f, s, seed=f * 100 + s + C)
    return lo, R.up(lo, ft, fs)


@pytest.mark.parametrize('shape,C', [(sh, C) for sh in R.SHAPES for C in (1, 3)] + [(R.BIG, 1)], ids=str)
def test_lowres_input_up(shape, C):
    from video_diffusion_nnx_amd import ops
    f, s, ft, fs = shape
    lo, ref = _up_ref(shape, C)
    sentinel = 7.25
    xin = torch.full((2, 2 * C, f * ft, s * fs, s * fs), sentinel, dtype=F32, device=DEV)
    with launches() as rec:
        ops.lowres_input(_dev(lo), ft, fs, out=xin)
    torch.cuda.synchronize()
    assert [k for k, _ in rec] == ['lowres_input_kernel']
    got = xin.cpu()
    assert (got[:, :C] == sentinel).all(), 'the sampling-time form wrote into the first half'
    err = (got[:, C:].double() - ref).abs().max().item()
    print(f'[up {shape} C={C}] per_sample {ref[0].numel()}: max |u - fp64| = {err:.3e} (bound {R.UP_BOUND:.0e})')
    assert err <= R.UP_BOUND
    if (ft, fs) == (1, 1):
        assert torch.equal(got[:, C:], 2 * lo - 1)                          # the identity: bit-equal to 2 lo - 1


@pytest.mark.parametrize('shape,C', [(R.ODD, 1), (R.ODD, 3), ((2, 4, 2, 2), 1), ((4, 8, 1, 1), 3)], ids=str)
def test_lowres_input_augmentation(shape, C):
    """Levels -1, 0 and T - 1 mixed within one batch: u = a up + b randn(shape, key, 0) from the kernel's own un-augmented output, one fp32
    rounding per operation -- the product b z and the fused multiply-add: half an ulp of each, together at most one ulp of the larger of
    |a up|, |b z| and |u|; held to 2.  At level -1 the bits of the un-augmented output."""
    from video_diffusion_nnx_amd import ops
    f, s, ft, fs = shape
    B, key = 3, 0x1234_5678_9ABC
    lo = _dev(R.make_lo(B, C, f, s, seed=3))
    sa, sm = _tables()
    plain = ops.lowres_input(lo, ft, fs)[:, C:]
    levels = torch.tensor([T - 1, -1, 0], dtype=torch.int32)
    got = ops.lowres_input(lo, ft, fs, tables=(sa, sm), aug_levels=_dev(levels), seed=key, draw=0)[:, C:]
    torch.cuda.synchronize()
    z = _randn(plain.shape, key, 0).cpu().double()
    assert torch.equal(got[1], plain[1]), 'level -1 is not the un-augmented output bit for bit'
    for b, lv in ((0, T - 1), (2, 0)):
        a, bb = sa[lv].item(), sm[lv].item()
        up, zz = plain[b].cpu().double(), z[b]
        ref = a * up + bb * zz
        scale = torch.maximum(torch.maximum((a * up).abs(), (bb * zz).abs()), ref.abs())
        ulps = ((got[b].cpu().double() - ref).abs() / _ulp32(scale)).max().item()
        print(f'[aug {shape} C={C}] level {lv}: worst {ulps:.3f} ulp (bound 2)')
        assert ulps <= 2.0
        assert not torch.equal(got[b], plain[b])
    # another draw index is another noise; the same call twice is the same bits
    other = ops.lowres_input(lo, ft, fs, tables=(sa, sm), aug_levels=_dev(levels), seed=key, draw=1)[:, C:]
    again = ops.lowres_input(lo, ft, fs, tables=(sa, sm), aug_levels=_dev(levels), seed=key, draw=0)[:, C:]
    assert torch.equal(again, got) and not torch.equal(other[0], got[0]) and torch.equal(other[1], got[1])


# ---- 3. lowres_input, the first half ----------------------------------------------------------------------------------------------------------

NET_SHAPE = (2, 4, 2, 2)          # lo [B,1,2,4,4] -> F = 4, S = 8: the network shape of the tests below


@pytest.mark.parametrize('shape,C', [(R.ODD, 1), (R.ODD, 3), (NET_SHAPE, 1)], ids=str)
def test_lowres_input_first_half_is_q_sample(shape, C):
    """Planes [0, C) against vdx_q_sample on the same x0, t, noise and pre-scale.  vdx_q_sample takes per_sample % 4 == 0 only; at the odd
    shape (per_sample = 486 C) its rows are padded to the next multiple of 4 and the padding dropped: the same kernel, element for element."""
    from video_diffusion_nnx_amd import _lib as L, ops
    from video_diffusion_nnx_amd.gaussian_diffusion import vdx_q_sample
    f, s, ft, fs = shape
    B = 2
    g = torch.Generator().manual_seed(11)
    full = (B, C, f * ft, s * fs, s * fs)
    x0, noise = torch.rand(full, generator=g), torch.randn(full, generator=g)
    t = torch.tensor([T - 1, 3], dtype=torch.int32)
    sa, sm = _tables()
    lo = _dev(R.make_lo(B, C, f, s, seed=4))
    xin = ops.lowres_input(lo, ft, fs, x0=_dev(x0), t=_dev(t), noise=_dev(noise), tables=(sa, sm), pre=(2.0, -1.0))
    per = x0[0].numel()
    pad = (-per) % 4
    xp = torch.zeros(B, per + pad)
    npad = torch.zeros(B, per + pad)
    xp[:, :per], npad[:, :per] = x0.reshape(B, -1), noise.reshape(B, -1)
    xp, npad = _dev(xp), _dev(npad)
    out = torch.empty_like(xp)
    L.check(vdx_q_sample(L.ptr(xp), L.ptr(_dev(t)), L.ptr(npad), L.ptr(out), L.ptr(sa), L.ptr(sm), B, per + pad, 2.0, -1.0, L.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(xin[:, :C].reshape(B, -1), out[:, :per]), 'first half is not vdx_q_sample bit for bit'
    # and the second half is what the sampling-time form writes
    assert torch.equal(xin[:, C:], ops.lowres_input(lo, ft, fs)[:, C:])


# ---- 4. lowres_pack ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('per', [486, 256])
def test_lowres_pack(per):
    from video_diffusion_nnx_amd import ops
    B = 3
    g = torch.Generator().manual_seed(per)
    img = _dev(torch.randn(B, 1, 1, 1, per, generator=g))
    xin = torch.full((B, 2, 1, 1, per), -3.5, dtype=F32, device=DEV)
    with launches() as rec:
        ops.lowres_pack(img, xin)
    torch.cuda.synchronize()
    assert [k for k, _ in rec] == ['lowres_pack_kernel'] and ('float4' if per % 4 == 0 else 'scalar') in rec[0][1], rec
    assert torch.equal(xin[:, :1], img) and (xin[:, 1:] == -3.5).all()
    # a base off 16 bytes takes the scalar form and writes the same bits
    buf = torch.full((B * 2 * per + 1,), -3.5, dtype=F32, device=DEV)
    off = buf[1:].view(B, 2, 1, 1, per)
    from video_diffusion_nnx_amd import _lib as L
    with launches() as rec:
        L.check(L.vdx_lowres_pack(L.ptr(img), off.data_ptr(), B, per, L.stream_ptr()))
    torch.cuda.synchronize()
    assert 'scalar' in rec[0][1] and torch.equal(off[:, :1], img) and (off[:, 1:] == -3.5).all() and buf[0].item() == -3.5


# ---- 5. forward parity --------------------------------------------------------------------------------------------------------------------------

NET_KW = dict(dim=16, dim_mults=(1, 2), channels=2, out_dim=1)
SHAPE = (2, 1, 4, 8, 8)


@functools.lru_cache(None)
def _params():
    return U.random_params(U.UnetConfig(**NET_KW), seed=1, dtype=F64)


def _net(mode='f32'):
    from video_diffusion_nnx_amd.unet3d import Unet3D
    unet = Unet3D(rngs=0, mode=mode, **NET_KW)
    unet.load_state_dict({k: v.float() for k, v in _params().items()})
    return unet


def _gd(unet=None, **kw):
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    kw.setdefault('lowres_cond', (2, 2))
    return GaussianDiffusion(unet or _net(), image_size=8, num_frames=4, channels=1, timesteps=T, **kw)


def test_forward_parity_on_a_kernel_built_input():
    from video_diffusion_nnx_amd import ops
    unet = _net()
    g = torch.Generator().manual_seed(2)
    x0, noise = torch.rand(SHAPE, generator=g), torch.randn(SHAPE, generator=g)
    t = torch.tensor([T - 1, 2], dtype=torch.int32)
    sa, sm = _tables()
    lo = ops.lowres_down(_dev(x0), 2, 2)
    xin = ops.lowres_input(lo, 2, 2, x0=_dev(x0), t=_dev(t), noise=_dev(noise), tables=(sa, sm), aug_levels=_dev(torch.tensor([4, -1], dtype=torch.int32)),
                           seed=9, pre=(2.0, -1.0))
    with launches() as rec:
        eps = unet(xin, _dev(t))
    torch.cuda.synchronize()
    assert any(k.startswith('init_conv') and 'mfma' not in k for k, _ in rec), rec      # Cin = 2: the generic stem
    ref = U.unet_forward(_params(), U.UnetConfig(**NET_KW), xin.cpu().double(), t.long())
    rel = ((eps.cpu().double() - ref).norm() / ref.norm()).item()
    print(f'[forward] eps_hat [2,4,8,8,1] on xin [2,2,4,8,8]: rel-L2 vs oracle {rel:.3e} (bound 4e-6)')
    assert eps.shape == (2, 4, 8, 8, 1) and rel <= 4e-6


# ---- 6. the loops -----------------------------------------------------------------------------------------------------------------------------

def _hand_chain(gd, chain, lo, seed, aug_level, steps=4):
    """The chain stepped by hand from existing public pieces: lowres_condition, torch.cat, unet(xin, t) and the existing step entries."""
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd import gaussian_diffusion as G
    unet = gd.denoise_fn
    B, per = SHAPE[0], int(np.prod(SHAPE[1:]))
    u = gd.lowres_condition(lo, seed, aug_level, draw=L.DRAW_LOWRES)
    img = gd.randn(SHAPE, seed, 0)
    hist = torch.empty_like(img)
    step_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
    seq_host = None if chain == 'ddpm' else G.ddim_time_sequence(T, steps)
    seq = None if seq_host is None else _dev(torch.from_numpy(seq_host))
    for k in range(T if chain == 'ddpm' else steps):
        t = torch.full((B,), T - 1 - k if chain == 'ddpm' else int(seq_host[k]), dtype=torch.int32, device=DEV)
        eps = unet(torch.cat([img, u], dim=1), t)
        step_dev.fill_(k)
        if chain == 'ddpm':
            L.check(G.vdx_p_sample_step(L.ptr(img), L.ptr(eps), L.ptr(img), L.ptr(t), L.ptr(gd._ptab), T, 0, seed, 1 + k, 0, 0, 1, B, 1, per, L.stream_ptr()))
        elif chain == 'ddim':
            L.check(G.vdx_ddim_step(L.ptr(img), L.ptr(eps), L.ptr(img), L.ptr(gd.alphas_cumprod), L.ptr(seq), L.ptr(step_dev), 0, 1, B, 1, per,
                                    L.stream_ptr()))
        else:
            L.check(G.vdx_dpm_step(L.ptr(img), L.ptr(eps), L.ptr(img), L.ptr(hist), L.ptr(gd.alphas_cumprod), L.ptr(seq), L.ptr(step_dev), 0, 1, 2, B, 1,
                                   per, L.stream_ptr()))
    out = torch.empty_like(img)
    L.check(G.vdx_affine(L.ptr(img), L.ptr(out), img.numel(), 0.5, 0.5, L.stream_ptr()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('chain', ['ddpm', 'ddim', 'dpm'])
def test_loops(chain):
    """Captured = eager = the hand-stepped chain, bit for bit; replay on other clips; no eviction; one pack launch per step.  The plain
    model whose p_sample_loop brackets the test has a handle of its own: a handle belongs to one network, and the plain loops refuse the
    super-resolution one (tests/test_host_superres.py), so "unchanged bits before and after" is checked across handles in one process and
    "no graph was evicted" on the super-resolution handle itself, by running another chain's loop in between."""
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.unet3d import Unet3D
    gd = _gd(lowres_aug_max=T)
    plain_unet = Unet3D(rngs=3, mode='f32', dim=16, dim_mults=(1, 2), channels=1)
    plain = GaussianDiffusion(plain_unet, image_size=8, num_frames=4, channels=1, timesteps=T)
    before = plain.p_sample_loop(SHAPE, 5)
    kw = {'ddpm': {}, 'ddim': dict(ddim_steps=4), 'dpm': dict(dpm_steps=4, dpm_order=2)}[chain]
    nsteps = T if chain == 'ddpm' else 4
    lo1, lo2 = R.make_lo(2, 1, 2, 4, seed=1), R.make_lo(2, 1, 2, 4, seed=2)
    seed, aug = 21, [3, -1]
    with launches() as rec:
        eager = gd.upsample(seed, lo1, aug_level=aug, use_graph=False, **kw)
    torch.cuda.synchronize()
    names = [k for k, _ in rec]
    assert names.count('lowres_pack_kernel') == nsteps, names                # exactly one per step
    assert names.count('lowres_input_kernel') == 1 and names.index('lowres_input_kernel') < names.index('lowres_pack_kernel'), names   # before the loop
    step_kernel = {'ddpm': 'p_sample_kernel', 'ddim': 'ddim_step_kernel', 'dpm': 'dpm_step_kernel'}[chain]
    assert names.count(step_kernel) == nsteps, names                         # the unchanged step kernel
    hand = _hand_chain(gd, chain, lo1, seed, aug)
    assert torch.equal(eager, hand), f'{chain}: the eager loop is not the hand-stepped chain bit for bit'
    graph = gd.upsample(seed, lo1, aug_level=aug, use_graph=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(graph, eager), f'{chain}: captured != eager'
    assert eager.shape == SHAPE and torch.isfinite(eager).all() and eager.min() >= 0 and eager.max() <= 1
    # another clip in the same buffers: the cached graph is replayed (nothing of the step is launched again)
    with launches() as rec:
        second = gd.upsample(seed, lo2, aug_level=aug, use_graph=True, **kw)
    torch.cuda.synchronize()
    names = [k for k, _ in rec]
    assert 'lowres_pack_kernel' not in names and step_kernel not in names and names.count('lowres_input_kernel') == 1, names
    assert torch.equal(second, _hand_chain(gd, chain, lo2, seed, aug)) and not torch.equal(second, graph)
    # sample(lowres=...) is upsample
    assert torch.equal(gd.sample(seed, lowres=lo2, lowres_aug_level=aug, **kw), second)
    # the other chains' graphs on this handle survive: run another chain, then this one replays still
    other = {'ddpm': dict(ddim_steps=4), 'ddim': dict(dpm_steps=4), 'dpm': {}}[chain]
    gd2 = _gd(gd.denoise_fn, lowres_aug_max=T)
    gd2.upsample(seed, lo1, use_graph=True, **other)
    with launches() as rec:
        third = gd.upsample(seed, lo2, aug_level=aug, use_graph=True, **kw)
    torch.cuda.synchronize()
    assert 'lowres_pack_kernel' not in [k for k, _ in rec] and torch.equal(third, second)
    # a plain model in the same process: unchanged bits before and after
    after = plain.p_sample_loop(SHAPE, 5)
    torch.cuda.synchronize()
    assert torch.equal(before, after)


def test_p_sample_with_lowres_cond_is_the_step_of_the_loop():
    gd = _gd()
    lo = R.make_lo(2, 1, 2, 4, seed=1)
    u = gd.lowres_condition(lo)
    assert u.shape == SHAPE and u.is_contiguous()
    x = gd.randn(SHAPE, 4, 0)
    t = torch.tensor([T - 1, 0])
    out = gd.p_sample(x, t, 8, lowres_cond=u)
    mean, var, logvar = gd.p_mean_variance(x, t, True, lowres_cond=u)
    torch.cuda.synchronize()
    assert out.shape == SHAPE and torch.isfinite(out).all() and torch.equal(out[1], mean[1]) and not torch.equal(out[0], mean[0])    # t = 0 adds no noise


# ---- 7. the train step ------------------------------------------------------------------------------------------------------------------------

def _trainer(tmp_path, gd):
    from video_diffusion_nnx_amd.trainer import Trainer
    return Trainer(gd, str(tmp_path), dataset_path='synthetic:8', train_batch_size=2, train_num_steps=3, train_lr=1e-3,
                   checkpoint_every_steps=2, results_folder=str(tmp_path / 'res'), step_start_ema=0, update_ema_every=1, ema_decay=0.9)


def _train_inputs():
    g = torch.Generator().manual_seed(0)
    return torch.rand(SHAPE, generator=g), torch.tensor([T - 1, 1], dtype=torch.int32), torch.randn(SHAPE, generator=g)


def test_train_step_is_the_step_done_by_hand(tmp_path):
    from video_diffusion_nnx_amd import _lib as L, ops
    from video_diffusion_nnx_amd.gaussian_diffusion import vdx_loss_sum
    from video_diffusion_nnx_amd.train_step import lowres_aug_key, vdx_loss_grad
    batch, t, noise = _train_inputs()
    levels = torch.tensor([5, -1], dtype=torch.int32)
    runs = []
    for r in range(2):
        gd = _gd(lowres_aug_max=T, loss_type='l2')
        tr = _trainer(tmp_path / str(r), gd)
        with launches() as rec:
            loss = tr.train_step(batch, step=0, t=t, noise=noise, aug_levels=levels)
        torch.cuda.synchronize()
        names = [k for k, _ in rec]
        assert names.count('lowres_down_kernel') == 1 and names.count('lowres_input_kernel') == 1 and 'q_sample_kernel' not in names, names
        assert torch.equal(torch.as_tensor(tr.last_aug_levels), levels) and tr.opt_count == 1
        runs.append((loss.clone(), tr.grads.clone(), gd.denoise_fn.flat_params.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs)), 'two runs are not bit-identical'
    # by hand: ops.lowres_input, unet.forward, the existing loss and gradient kernels, unet.backward
    unet = _net()
    sa, sm = _tables()
    x = _dev(batch)
    lo = ops.lowres_down(x, 2, 2)
    xin = ops.lowres_input(lo, 2, 2, x0=x, t=_dev(t), noise=_dev(noise), tables=(sa, sm), aug_levels=_dev(levels), seed=lowres_aug_key(tr.rng_seed, tr.rank, 0),
                           draw=0, pre=(2.0, -1.0))
    eps = unet(xin, _dev(t))
    fhw = int(np.prod(SHAPE[2:]))
    acc = torch.zeros(1, dtype=F64, device=DEV)
    L.check(vdx_loss_sum(L.ptr(eps), L.ptr(_dev(noise)), L.ptr(acc), 2, 1, fhw, 1, L.stream_ptr()))
    d_eps = torch.empty_like(eps)
    L.check(vdx_loss_grad(L.ptr(eps), L.ptr(_dev(noise)), L.ptr(d_eps), 2, 1, fhw, 1, L.stream_ptr()))
    grads = torch.zeros_like(unet.flat_params)
    unet.backward(d_eps, grads)
    torch.cuda.synchronize()
    hand_loss = (acc / float(batch.numel())).to(F32).reshape(())
    assert torch.equal(hand_loss, runs[0][0]), (hand_loss.item(), runs[0][0].item())
    assert torch.equal(grads, runs[0][1]), 'flat gradients differ from the step done by hand'
    assert grads.abs().max() > 0 and np.isfinite(hand_loss.item())
    # the second half of the stem carries gradient: the network reads u
    off = {n: (o, s) for n, s, o in unet.param_table}
    o, s = off['init_conv.kernel']
    gk = grads[o:o + int(np.prod(s))].reshape(s)
    assert gk[..., 1, :].abs().max() > 0 and gk[..., 0, :].abs().max() > 0


def test_zeroed_conditioning_weights_give_the_plain_network_loss(tmp_path):
    """(ft, fs) = (1, 1), no augmentation, the planes-[C, 2C) slice of the stem kernel zeroed: the loss of the plain C-channel network that
    carries the same remaining weights, within the f32 forward bound."""
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.unet3d import Unet3D
    batch, t, noise = _train_inputs()
    p = {k: v.float().clone() for k, v in _params().items()}
    p['init_conv.kernel'][..., 1, :] = 0.0
    sr_unet = Unet3D(rngs=0, mode='f32', **NET_KW)
    sr_unet.load_state_dict(p)
    plain_unet = Unet3D(rngs=0, mode='f32', **dict(NET_KW, channels=1))
    plain_unet.load_state_dict(dict(p, **{'init_conv.kernel': p['init_conv.kernel'][..., :1, :].contiguous()}))
    sr = _trainer(tmp_path / 'sr', _gd(sr_unet, lowres_cond=(1, 1), loss_type='l2'))
    pl = _trainer(tmp_path / 'plain', GaussianDiffusion(plain_unet, image_size=8, num_frames=4, channels=1, timesteps=T, loss_type='l2'))
    a = sr.train_step(batch, step=0, t=t, noise=noise).item()
    b = pl.train_step(batch, step=0, t=t, noise=noise).item()
    print(f'[zeroed] loss {a:.8f} plain {b:.8f} rel {abs(a - b) / abs(b):.2e} (bound 4e-6)')
    assert sr.last_aug_levels is None and abs(a - b) <= 4e-6 * abs(b)


def test_bf16_train_step(tmp_path):
    batch, t, noise = _train_inputs()
    levels = torch.tensor([5, -1], dtype=torch.int32)
    losses = {}
    for mode in ('f32', 'bf16'):
        tr = _trainer(tmp_path / mode, _gd(_net(mode), lowres_aug_max=T))
        losses[mode] = tr.train_step(batch, step=0, t=t, noise=noise, aug_levels=levels).item()
        torch.cuda.synchronize()
        assert np.isfinite(losses[mode]) and torch.isfinite(tr.unet.flat_params).all()
    rel = abs(losses['bf16'] - losses['f32']) / abs(losses['f32'])
    print(f'[bf16] loss {losses["bf16"]:.6f} f32 {losses["f32"]:.6f} rel {rel:.2e} (bound 8e-3)')
    assert rel <= 8e-3


def test_default_draws_and_accumulation(tmp_path):
    """Without explicit levels they are drawn on the host under the augmentation key; the t and noise streams are the plain trainer's."""
    from video_diffusion_nnx_amd.gaussian_diffusion import lowres_aug_levels
    from video_diffusion_nnx_amd.train_step import lowres_aug_key, micro_step_keys
    gd = _gd(lowres_aug_max=7)
    tr = _trainer(tmp_path, gd)
    batch, _, _ = _train_inputs()
    loss = tr.train_step(batch, step=2)
    torch.cuda.synchronize()
    assert torch.equal(tr.last_aug_levels, lowres_aug_levels(2, 7, lowres_aug_key(tr.rng_seed, tr.rank, 2)))
    assert tr.last_noise_key == micro_step_keys(tr.rng_seed, tr.rank, 2)[1] and np.isfinite(loss.item())
    tr.apply_grad_args, tr.gradient_accumulate_every = True, 2
    loss = tr.train_step_accum([batch, batch.flip(0)], step=3)
    torch.cuda.synchronize()
    assert np.isfinite(loss.item()) and tr.opt_count == 2
    val = gd(batch, 4)                                                      # __call__ / p_losses: its own draws
    explicit = gd.p_losses(batch, torch.tensor([1, 2]), 5, aug_levels=[-1, 3], lowres=torch.rand(2, 1, 2, 4, 4))
    assert np.isfinite(val.item()) and np.isfinite(explicit.item())
