"""Learned reverse-process variances on the GPU (Nichol & Dhariwal 2021; vdx.h: "Learned variances"): the hybrid-loss kernel, the reverse
step with the model's variance, the final-conv backward at 5 and 6 output channels, the captured sampling and evaluation loops on the tiny
rig of tests/test_gpu_sample_loops.py with out_dim = 2 * channels, and training.  The yardstick is tests/_lv_ref.py (fp64, CPU); every
bound comes from that reference evaluated in fp32, from the number formats, or is stated by the kernel's contract (bit equality).

Two of the contract's statements about the gradient tensor cannot both hold for its eps_hat half: "bit-equal to vdx_loss_grad" (fp32
arithmetic: the difference, the reciprocal of the count and the product are each rounded) and "one fp32 rounding of the fp64 value".  The
eps_hat half is held to the first (its own precision is vdx_loss_grad's, tested there), the v half -- formed in double, rounded once -- to the
second."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lv_ref as R                       # noqa: E402
import _vlb_ref as V                      # noqa: E402
from _launch_hook import launches        # noqa: E402
from oracle import philox_ref            # noqa: E402
from oracle import train_ref             # noqa: E402
from oracle import unet3d_ref as U       # noqa: E402
from oracle.diffusion_ref import DiffusionRef      # noqa: E402

DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
OK, INVALID = 0, -1


def _dev(t, dtype=None):
    return t.detach().to(dtype or t.dtype).to(DEV).contiguous()


def _ulp32(ref64):
    """Spacing of fp32 at the fp32 rounding of ref64 (towards the larger magnitude), as float64."""
    r = ref64.float()
    return (torch.nextafter(r.abs(), torch.full_like(r, float('inf'))) - r.abs()).double()


# ---- 1. vdx_hybrid_loss ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def _hybrid_ref(name, l2, w):
    c = R.hybrid_case(name)
    tab = R.tables()['tab64']
    vals, grad = R.hybrid_grad(c['x0'], c['eps'], c['out2'], c['t'], tab, l2, w)
    with torch.no_grad():
        v32 = R.hybrid(c['x0'], c['eps'], c['out2'], c['t'], tab, l2, w, dt=F32)
    return vals, grad, {k: u.double() for k, u in v32.items()}


@pytest.mark.parametrize('l2', [False, True], ids=['l1', 'l2'])
@pytest.mark.parametrize('name', list(R.HYBRID_CASES))
def test_hybrid_loss_kernel(name, l2):
    from video_diffusion_nnx_amd import ops
    from video_diffusion_nnx_amd.train_step import vdx_loss_grad
    from video_diffusion_nnx_amd import _lib as L
    c = R.hybrid_case(name)
    B, C = c['shape'][0], c['shape'][1]
    w = 0.37
    vals, g_ref, v32 = _hybrid_ref(name, l2, w)
    tab = _dev(torch.from_numpy(R.tables()['tab64']))
    x, eps, out2, t = _dev(c['x0']), _dev(c['eps']), _dev(c['out2']), _dev(c['t'])
    runs = []
    for _ in range(2):
        out, d_out = ops.hybrid_loss(x, eps, out2, t, tab, l2=l2, vlb_weight=w, want_grad=True)
        torch.cuda.synchronize()
        runs.append((out.cpu(), d_out.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), 'two runs are not bit-identical'
    out, d_out = runs[0]
    assert torch.isfinite(out).all() and torch.isfinite(d_out).all()
    # the gradient, v half: one fp32 rounding of the fp64 value per element
    gv, rv = d_out[..., C:].double(), g_ref[..., C:]
    ulps = ((gv - rv).abs() / _ulp32(rv)).max().item()
    print(f'[hybrid {name} l2={int(l2)}] v half of d_out: worst |got - fp64| = {ulps:.3f} fp32 ulp (bound 1)')
    assert ulps <= 1.0
    assert (gv != 0).float().mean() > 0.99                                           # the v half carries gradient
    # the gradient, eps_hat half: vdx_loss_grad's bits
    eh = out2[..., :C].contiguous()
    d_eps = torch.empty_like(eh)
    fhw = int(np.prod(c['shape'][2:]))
    L.check(vdx_loss_grad(L.ptr(eh), L.ptr(eps), L.ptr(d_eps), B, C, fhw, int(l2), L.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(d_out[..., :C], d_eps.cpu()), 'eps_hat half of d_out is not vdx_loss_grad bit for bit'
    worst = ((d_out[..., :C].double() - g_ref[..., :C]).abs() / _ulp32(g_ref[..., :C])).max().item()
    print(f'[hybrid {name} l2={int(l2)}] eps_hat half of d_out against fp64: worst {worst:.3f} fp32 ulp (vdx_loss_grad: three fp32 roundings)')
    # the sums: 8 x the error of the same expressions in fp32 on the CPU -- relative per sample for the mse and the KL samples, absolute
    # for the decoder samples (t = 0), as tests/_vlb_ref.term_bounds states it
    got_b = out[:2 * B].reshape(B, 2)
    bounds = V.term_bounds((v32['vb_b'], v32['mse_b'], v32['mse_b']), (vals['vb_b'], vals['mse_b'], vals['mse_b']), c['t'])
    for col, key, row in ((0, 'mse_b', 1), (1, 'vb_b', 0)):
        err = (got_b[:, col] - vals[key]).abs()
        print(f'[hybrid {name} l2={int(l2)}] {key}: |err| {err.tolist()} bound {bounds[row].tolist()} value {vals[key].tolist()}')
        assert (err <= bounds[row]).all(), (key, err, bounds[row])
    for i, key in enumerate(('mse', 'vb', 'loss')):
        tol = 8.0 * max(abs(float(v32[key] - vals[key])), 2.0 ** -52 * abs(float(vals[key])))
        err = abs(float(out[2 * B + i] - vals[key]))
        print(f'[hybrid {name} l2={int(l2)}] {key}: {float(out[2 * B + i]):.12g} ref {float(vals[key]):.12g} |err| {err:.2e} bound {tol:.2e}')
        assert err <= tol
    # the total is the sum of its parts, and no gradient is asked for -> the same sums
    total, parts = float(out[2 * B + 2]), float(out[2 * B] + w * out[2 * B + 1])
    assert abs(total - parts) <= 2.0 ** -52 * abs(total)                             # (the kernel may fuse the multiply-add: one rounding)
    out2nd, none = ops.hybrid_loss(x, eps, out2, t, tab, l2=l2, vlb_weight=w, want_grad=False)
    assert none is None and torch.equal(out2nd.cpu(), out)


# ---- 2. vdx_p_sample_step_lv ------------------------------------------------------------------------------------------------------------------

def _old_tables(T):
    """The [6][T] step table whose rows 0-3 and 5 are the fixed-variance sampler's fp32 tables (row 4, max_log, is never weighted at v = -1)."""
    from video_diffusion_nnx_amd.gaussian_diffusion import make_tables
    o = make_tables(T)
    return np.stack([o['sqrt_recip_alphas_cumprod'], o['sqrt_recipm1_alphas_cumprod'], o['posterior_mean_coef1'], o['posterior_mean_coef2'],
                     np.log(np.maximum(1.0 - o['alphas_cumprod'], 1e-20)).astype(np.float32), o['posterior_log_variance_clipped']]).astype(np.float32)


@pytest.mark.parametrize('explicit', [True, False], ids=['noise', 'philox'])
def test_step_at_v_minus_one_is_p_sample_step_bit_for_bit(explicit):
    """Every level of T = 1000 in one call (sample b at level b): the shared arithmetic and the Philox indexing."""
    from video_diffusion_nnx_amd import ops, _lib as L
    from video_diffusion_nnx_amd.gaussian_diffusion import vdx_p_sample_step
    T = 1000
    for C, fhw in ((1, (1, 4, 4)), (3, (2, 5, 7)) if explicit else (3, (2, 2, 3))):      # per_sample 16; 210 (tail quad) / 36 (philox: % 4)
        g = torch.Generator().manual_seed(7 + C)
        shape = (T, C) + fhw
        x, eh, z = (torch.randn(shape, generator=g) for _ in range(3))
        x[0] *= 3.0                                                                     # the clip takes part
        out2 = _dev(torch.cat([eh, -torch.ones(shape)], 1).permute(0, 2, 3, 4, 1))
        eps_cl = _dev(eh.permute(0, 2, 3, 4, 1))
        lvl = torch.arange(T, dtype=torch.int32, device=DEV)
        tab6 = _dev(torch.from_numpy(_old_tables(T)))
        ptab = _dev(torch.from_numpy(_old_tables(T)[[0, 1, 2, 3, 5]]))
        xd, zd = _dev(x), (_dev(z) if explicit else None)
        for clip in (True, False):
            got = ops.p_sample_step_lv(xd, out2, tab6, level=lvl, noise=zd, seed=11, offset=5, clip=clip)
            want = torch.empty_like(xd)
            L.check(vdx_p_sample_step(L.ptr(xd), L.ptr(eps_cl), L.ptr(want), L.ptr(lvl), L.ptr(ptab), T, L.ptr(zd), 11, 5, 0, 0, int(clip), T, C,
                                      xd[0].numel(), L.stream_ptr()))
            torch.cuda.synchronize()
            bad = (got != want).flatten(1).any(1).nonzero().flatten().tolist()
            assert not bad, f'C={C} clip={clip}: levels {bad[:10]} differ from vdx_p_sample_step'
            assert torch.isfinite(got).all() and (got[1:] != xd[1:]).any()


# general v: the bound is 4 x the per-element error of tests/_lv_ref.step evaluated in fp32 on the CPU against fp64, on these inputs:
# without the clip (x0_hat reaches 1e2 .. 1e3 at the top levels) 1.5e-4 (T = 1000, full chain) and 2.2e-3 (S = 4 of T = 50), the kernel at
# 3.8e-5 and 5.5e-4; computed again in the test, for both clip settings, and printed
def _step_case(S, C=3, fhw=(2, 5, 7), seed=3):
    g = torch.Generator().manual_seed(seed)
    B = 2 * S if S <= 8 else 8
    shape = (B, C) + fhw
    x, eh, z = (torch.randn(shape, generator=g) for _ in range(3))
    v = torch.rand(shape, generator=g) * 2 - 1
    v.view(B, -1)[:, 0], v.view(B, -1)[:, 1] = 3.0, -3.0
    lvl = (torch.arange(B) % S) if S <= 8 else torch.tensor([0, 1, 2, S // 3, S // 2, S - 3, S - 2, S - 1])
    return x, eh, v, z, lvl.to(torch.int32)


@pytest.mark.parametrize('T,S', [(1000, 1000), (50, 4)], ids=['full', 'respaced'])
def test_step_general_v_against_fp64(T, S):
    from video_diffusion_nnx_amd import ops
    from video_diffusion_nnx_amd.gaussian_diffusion import lv_time_sequence, make_lv_tables
    seq = lv_time_sequence(T, S)
    tabs = make_lv_tables(T, seq[:-1][::-1])
    x, eh, v, z, lvl = _step_case(S)
    out2 = _dev(torch.cat([eh, v], 1).permute(0, 2, 3, 4, 1))
    tab6 = _dev(torch.from_numpy(tabs['step']))
    for clip in (True, False):
        ref = R.step(x, eh, v, z, lvl, tabs['step'].astype(np.float64), clip)
        ref32 = R.step(x, eh, v, z, lvl, tabs['step'], clip, dt=F32).double()
        bound = 4.0 * (ref32 - ref).abs().max().item()
        xd = _dev(x)
        got = ops.p_sample_step_lv(xd, out2, tab6, level=_dev(lvl), noise=_dev(z), clip=clip)
        torch.cuda.synchronize()
        err = (got.cpu().double() - ref).abs().max().item()
        print(f'[step T={T} S={S} clip={int(clip)}] max |got - fp64| = {err:.2e} (bound 4 x fp32 CPU = {bound:.2e})')
        assert err <= bound
        # level 0 adds no noise: the noise tensor does not matter there
        zero = ops.p_sample_step_lv(xd, out2, tab6, level=_dev(lvl), noise=torch.zeros_like(xd), clip=clip)
        l0 = (lvl == 0).nonzero().flatten()
        assert len(l0) and torch.equal(zero[l0.to(DEV)], got[l0.to(DEV)]) and not torch.equal(zero, got)
        # x and out may alias
        xa = xd.clone()
        ops.p_sample_step_lv(xa, out2, tab6, level=_dev(lvl), noise=_dev(z), clip=clip, out=xa)
        assert torch.equal(xa, got)
        # the affine of the last step touches level 0 only
        post = ops.p_sample_step_lv(xd, out2, tab6, level=_dev(lvl), noise=_dev(z), clip=clip, post=(0.5, 0.5))
        keep = (lvl != 0).nonzero().flatten().to(DEV)
        assert torch.equal(post[keep], got[keep])
        assert torch.allclose(post[l0.to(DEV)], got[l0.to(DEV)] * 0.5 + 0.5, rtol=0, atol=2.0 ** -22)      # (one fused or two separate roundings)


def test_step_counter_indexing_of_a_respaced_chain():
    """S = 4 of T = 50: step k (host value, device counter, or their sum) is level S - 1 - k of the respaced table."""
    from video_diffusion_nnx_amd import ops
    from video_diffusion_nnx_amd.gaussian_diffusion import lv_time_sequence, make_lv_tables
    T, S = 50, 4
    tabs = make_lv_tables(T, lv_time_sequence(T, S)[:-1][::-1])
    x, eh, v, z, _ = _step_case(S)
    B = x.shape[0]
    out2, tab6, xd, zd = _dev(torch.cat([eh, v], 1).permute(0, 2, 3, 4, 1)), _dev(torch.from_numpy(tabs['step'])), _dev(x), _dev(z)
    for k in range(S):
        by_level = ops.p_sample_step_lv(xd, out2, tab6, level=torch.full((B,), S - 1 - k, dtype=torch.int32, device=DEV), noise=zd)
        for host, dev in ((k, None), (0, k), (1, k - 1) if k else (0, 0)):
            sd = None if dev is None else torch.tensor([dev], dtype=torch.int64, device=DEV)
            got = ops.p_sample_step_lv(xd, out2, tab6, step=host, step_dev=sd, noise=zd)
            assert torch.equal(got, by_level), (k, host, dev)
    # in-kernel noise: draw = offset + *dev_offset of the element-indexed Philox stream
    n = x[:, :1, :, :2, :2].numel()
    xs, o2 = xd[:, :1, :, :2, :2].contiguous(), out2[:, :, :2, :2, [0, 3]].contiguous()
    sd = torch.tensor([2], dtype=torch.int64, device=DEV)
    got = ops.p_sample_step_lv(xs, o2, tab6, step=0, step_dev=sd, seed=9, offset=1, dev_offset=sd)
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd.gaussian_diffusion import vdx_randn
    zz = torch.empty_like(xs)
    L.check(vdx_randn(L.ptr(zz), n, 9, 3, 0, L.stream_ptr()))
    want = ops.p_sample_step_lv(xs, o2, tab6, level=torch.full((B,), S - 3, dtype=torch.int32, device=DEV), noise=zz)
    assert torch.equal(got, want)
    ref = torch.from_numpy(philox_ref.randn(n, 9, 3)).reshape(xs.shape)
    assert torch.allclose(zz.cpu(), ref, atol=3e-6, rtol=1e-5)                        # the draw itself against oracle/philox_ref (tests/_step_cases.py)


# ---- 3. final conv backward at 5 and 6 output channels ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('x16', [False, True])
@pytest.mark.parametrize('D,Cout,lead', [(64, 6, (1, 3, 7, 5)), (16, 5, (1, 3, 7, 5)), (32, 6, (2, 16, 64, 64))])
def test_final_conv_backward_wide(D, Cout, lead, x16):
    """tests/test_gpu_backward_forms.py::test_final_conv_backward at Cout 5 and 6, with its bounds (_small_bound for dx, _sum_bound for the
    sums over the pixels)."""
    import _parity as P
    import test_gpu_backward_forms as FB
    from video_diffusion_nnx_amd import ops
    g = torch.Generator().manual_seed(2 + D)
    x = P.bf16r(torch.randn(*lead, D, generator=g))
    kern, d_out = torch.randn(1, D, Cout, generator=g), torch.randn(*lead, Cout, generator=g)

    def grads(dt, sq=False):
        f = (lambda t: t.to(dt) ** 2) if sq else (lambda t: t.to(dt))
        xx, kk, bb = f(x).requires_grad_(True), kern.to(dt).requires_grad_(True), torch.zeros(Cout, dtype=dt, requires_grad=True)
        return torch.autograd.grad(U.conv_pointwise(xx, kk, bb), (xx, kk, bb), f(d_out))

    ref, ref32 = grads(F64), grads(F32)
    npix = x.numel() // D
    scale = [None] + [t.sqrt() for t in grads(F64, sq=True)[1:]]
    bounds = [FB._small_bound(ref32[0], ref[0])] + [FB._sum_bound(ref32[i], ref[i], scale[i], npix) for i in (1, 2)]
    slots = torch.full((ops.WG_PART_FLOATS,), float('nan'), dtype=F32, device=DEV)
    outs = {}
    for label, scr in (('atomics', None), ('slots', slots), ('slots again', slots)):
        slots.fill_(float('nan'))
        with launches() as rec:
            dx, dw, db = ops.final_conv_backward_wide(_dev(x, torch.bfloat16 if x16 else F32), _dev(d_out), _dev(kern), scratch=scr)
        torch.cuda.synchronize()
        assert [k for k, _ in rec][:2] == ['final_conv_dx_kernel', 'final_conv_dw_kernel'] and f'Cout{Cout}' in rec[1][1], rec
        assert (f'det {int(scr is not None)}') in rec[1][1], rec
        outs[label] = got = (dx.cpu(), dw.cpu().reshape(1, D, Cout), db.cpu())
        for nm, a, b, bd, sc in zip(('dx', 'dw', 'db'), got, ref, bounds, scale):
            rr = P.rel(a, b) if sc is None else FB._sum_err(a, b, sc)
            print(f'[final_conv wide D={D} Cout={Cout} {lead} x16={int(x16)} {label}] {nm}: rel {rr:.3e} (bound {bd:.3e})')
            assert rr < bd, (nm, rr, bd)
    assert all(torch.equal(a, b) for a, b in zip(outs['slots'], outs['slots again'])), 'two runs with slots are not bit-identical'
    # Cout <= 4 through the wide entry: vdx_final_conv_backward's bits
    k4, d4 = _dev(kern[..., :3].contiguous()), _dev(d_out[..., :3].contiguous())
    xd = _dev(x, torch.bfloat16 if x16 else F32)
    a = ops.final_conv_backward_wide(xd, d4, k4, scratch=slots)
    b = ops.final_conv_backward(xd, d4, k4, scratch=slots)
    assert all(torch.equal(u, w) for u, w in zip(a, b))
    with pytest.raises(ops.L.VdxError):
        ops.final_conv_backward_wide(_dev(x), _dev(torch.randn(*lead, 7)), _dev(torch.randn(1, D, 7)))


# ---- 4. the loops on the tiny rig -------------------------------------------------------------------------------------------------------------

KW = dict(dim=16, channels=1, dim_mults=(1, 2))
SHAPE = (2, 1, 4, 8, 8)


@functools.lru_cache(None)
def _net(C=1, seed=0, mode='f32'):
    from video_diffusion_nnx_amd.unet3d import Unet3D
    return Unet3D(rngs=seed, mode=mode, **dict(KW, channels=C), out_dim=2 * C)


def _gd(T, C=1, **kw):
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    return GaussianDiffusion(_net(C), image_size=SHAPE[3], num_frames=SHAPE[2], channels=C, timesteps=T, learned_variance=True, **kw)


def _loop(gd, S, T, seed, use_graph, nsteps=None, bufs=None, post=(1.0, 0.0)):
    """vdx_p_sample_loop_lv on buffers this function owns; returns (img, out2, t_dev, step_dev, launches)."""
    from video_diffusion_nnx_amd import _lib as L
    unet = gd.denoise_fn
    B = SHAPE[0]
    seq, tab, S_ = gd._lv_tables(None if S == T else S)
    assert S_ == S
    if bufs is None:
        img = gd.randn(SHAPE, seed, 0)
        bufs = dict(img=img, out2=torch.zeros(B, SHAPE[2], SHAPE[3], SHAPE[4], unet.out_dim, device=DEV),
                    t=torch.full((B,), int(seq[0]), dtype=torch.int32, device=DEV), step=torch.zeros(1, dtype=torch.int64, device=DEV))
    h = unet.handle(SHAPE[2], SHAPE[3])
    unet.apply_activation_storage(h)
    ws = unet.workspace(B, SHAPE[2], SHAPE[3])
    st = torch.cuda.Stream(device=DEV)
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st), launches() as rec:
        rc = L.vdx_p_sample_loop_lv(h.ptr, L.ptr(unet.flat_params), L.ptr(unet.packed()), L.ptr(bufs['img']), L.ptr(bufs['out2']), L.ptr(bufs['t']),
                                    L.ptr(bufs['step']), L.ptr(tab), L.ptr(seq), S, T, S if nsteps is None else nsteps, 0, seed, 1, post[0], post[1],
                                    L.ptr(ws), ws.numel(), B, int(use_graph), st.cuda_stream)
        st.synchronize()
    assert rc == OK, L.vdx_last_error()
    return bufs, rec


@pytest.mark.parametrize('T,S', [(8, 8), (50, 4)], ids=['T8', 'S4ofT50'])
def test_sampling_loop(T, S):
    from video_diffusion_nnx_amd.gaussian_diffusion import lv_time_sequence, make_lv_tables
    gd = _gd(T)
    eager, rec = _loop(gd, S, T, 3, use_graph=False)
    steps = [k for k, _ in rec if k == 'p_sample_lv_kernel']
    assert len(steps) == S and sum(k == 'ddim_advance_kernel' for k, _ in rec) == S, rec      # once per step
    assert not any(k in ('p_sample_kernel', 'ddim_step_kernel') for k, _ in rec)
    graph, _ = _loop(gd, S, T, 3, use_graph=True)
    again, _ = _loop(gd, S, T, 3, use_graph=True)
    other, _ = _loop(gd, S, T, 4, use_graph=True)
    assert torch.equal(eager['img'], graph['img']) and torch.equal(graph['img'], again['img']), 'graph != eager chain / not seed-deterministic'
    assert not torch.equal(other['img'], graph['img']) and torch.isfinite(graph['img']).all()
    for b in (eager, graph):
        assert b['t'].tolist() == [0] * SHAPE[0] and int(b['step'].item()) == S            # t walks to 0, the counter equals S
    # every step replayed on the CPU from the device's own network output
    seq = lv_time_sequence(T, S)
    tabs = make_lv_tables(T, seq[:-1][::-1])
    bufs, _ = _loop(gd, S, T, 3, use_graph=False, nsteps=0)
    for k in range(S):
        x_in = bufs['img'].cpu()
        assert bufs['t'].tolist() == [int(seq[k])] * SHAPE[0]                                # the network is called with t = seq_i
        bufs, _ = _loop(gd, S, T, 3, use_graph=bool(k % 2), nsteps=1, bufs=bufs)
        eh, v = R.split(bufs['out2'].cpu(), 1)
        z = gd.randn(SHAPE, 3, 1 + k).cpu()                                                  # the device's own draw 1 + k
        lvl = torch.full((SHAPE[0],), S - 1 - k)
        ref = R.step(x_in, eh, v, z, lvl, tabs['step'].astype(np.float64), True)
        ref32 = R.step(x_in, eh, v, z, lvl, tabs['step'], True, dt=F32).double()
        bound = 4.0 * (ref32 - ref).abs().max().item()
        err = (bufs['img'].cpu().double() - ref).abs().max().item()
        print(f'[loop T={T} S={S}] step {k} (t={int(seq[k])}): max |x - fp64 replay| = {err:.2e} (bound {bound:.2e})')
        assert err <= bound
    assert torch.equal(bufs['img'], eager['img'])                                            # issued in pieces: the same chain
    # the affine of the last step
    post, _ = _loop(gd, S, T, 3, use_graph=False, post=(0.5, 0.5))
    assert torch.allclose(post['img'], eager['img'] * 0.5 + 0.5, rtol=0, atol=2.0 ** -23)      # (one fused or two separate roundings)
    # the public method
    vid = gd.p_sample_loop(SHAPE, 3, steps=None if S == T else S)
    torch.cuda.synchronize()
    assert torch.equal(vid, post['img']) and torch.equal(gd.sample(3, batch_size=SHAPE[0], steps=None if S == T else S), vid)


def test_existing_loops_still_refuse_the_network():
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion, vdx_p_sample_loop
    unet = _net()
    plain = GaussianDiffusion(unet, image_size=SHAPE[3], num_frames=SHAPE[2], channels=1, timesteps=8)
    with pytest.raises(L.VdxError, match='out_dim must equal channels'):
        plain.p_sample_loop(SHAPE, 0)
    with pytest.raises(L.VdxError, match='out_dim must equal channels'):
        plain.calc_bpd_loop(torch.rand(SHAPE), 0)
    from video_diffusion_nnx_amd.unet3d import Unet3D
    one = Unet3D(rngs=0, mode='f32', **KW)
    gd = _gd(8)
    h = one.handle(SHAPE[2], SHAPE[3])
    ws = one.workspace(SHAPE[0], SHAPE[2], SHAPE[3])
    seq, tab, _ = gd._lv_tables(None)
    z = torch.zeros(SHAPE, device=DEV)
    o2 = torch.zeros(SHAPE[0], SHAPE[2], SHAPE[3], SHAPE[4], 2, device=DEV)
    t, s = torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    with launches() as rec:
        rc = L.vdx_p_sample_loop_lv(h.ptr, L.ptr(one.flat_params), L.ptr(one.packed()), L.ptr(z), L.ptr(o2), L.ptr(t), L.ptr(s), L.ptr(tab), L.ptr(seq),
                                    8, 8, 1, 0, 1, 1, 1.0, 0.0, L.ptr(ws), ws.numel(), 2, 0, L.stream_ptr())
    assert rc == INVALID and 'out_dim must equal 2 * channels' in L.vdx_last_error().decode() and rec == []


@pytest.mark.parametrize('steps', [None, 4], ids=['all', 'S4'])
def test_calc_bpd_loop_with_learned_variance(steps):
    from video_diffusion_nnx_amd import ops
    T = 12
    gd = _gd(T)
    g = torch.Generator().manual_seed(2)
    x = (torch.rand(SHAPE, generator=g) * 255).round() / 255
    x.view(2, -1)[:, 0], x.view(2, -1)[:, 1] = 0.0, 1.0
    with launches() as rec:
        eager = gd.calc_bpd_loop(x, 5, timesteps=steps, use_graph=False)
    S = T if steps is None else steps
    assert sum(k == 'vlb_term_lv_kernel' for k, _ in rec) == S and not any(k == 'vlb_term_kernel' for k, _ in rec), rec
    graph = gd.calc_bpd_loop(x, 5, timesteps=steps, use_graph=True)
    for k in ('vb', 'mse', 'xstart_mse', 'prior_bpd'):
        assert torch.equal(eager[k], graph[k]), k
    if steps is None:
        assert torch.equal(graph['total_bpd'], graph['prior_bpd'] + graph['vb'].sum(1)) and torch.isfinite(graph['total_bpd']).all()
    else:
        assert graph['total_bpd'] is None
    # the terms against the reference, from the device's own network outputs
    tab64 = R.tables(T)['tab64']
    tabd = _dev(torch.from_numpy(tab64))
    xd = _dev(x)
    for col, lvl in enumerate(graph['t'].tolist()):
        t = torch.full((SHAPE[0],), lvl, dtype=torch.int32)
        xt = ops.vlb_noise(xd, _dev(t), tabd, seed=5, draw=1 + col)
        out2 = gd.denoise_fn(xt, _dev(t))
        got = ops.vlb_terms_lv(xd, out2, _dev(t), tabd, seed=5, draw=1 + col).cpu()
        eps = gd.randn(SHAPE, 5, 1 + col).cpu()                                              # the device's own draw 1 + col
        ref = R.bound_terms(x, out2.cpu(), eps, t, tab64, clip=True)
        ref32 = R.bound_terms(x, out2.cpu(), eps, t, tab64, clip=True, dt=F32)
        bounds = V.term_bounds(ref32, ref, t)
        for j, name in enumerate(('vb', 'mse', 'xstart_mse')):
            err = (got[:, j] - ref[j]).abs()
            assert (err <= bounds[j]).all(), (lvl, name, err, bounds[j])
            assert torch.equal(got[:, j], graph[name][:, col]), (lvl, name)                  # the loop is this step, bit for bit
    assert (graph['vb'] > 0).all()


# ---- 5. training ------------------------------------------------------------------------------------------------------------------------------

TRAIN_KW = dict(dim=16, dim_mults=(1, 2), channels=1, out_dim=2)
TRAIN_SHAPE = (2, 1, 2, 16, 16)


def _mk(tmp_path, mode, C=1, loss_type='l2'):
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.trainer import Trainer
    from video_diffusion_nnx_amd.unet3d import Unet3D
    unet = Unet3D(rngs=1, mode=mode, **dict(TRAIN_KW, channels=C, out_dim=2 * C))
    gd = GaussianDiffusion(unet, image_size=16, num_frames=2, channels=C, timesteps=50, loss_type=loss_type, learned_variance=True)
    tr = Trainer(gd, str(tmp_path), dataset_path='synthetic:8', train_batch_size=2, train_num_steps=3, train_lr=1e-3,
                 checkpoint_every_steps=2, results_folder=str(tmp_path / 'res'), step_start_ema=0, update_ema_every=1, ema_decay=0.9)
    return unet, gd, tr


def test_one_train_step_matches_oracle(tmp_path):
    """tests/test_gpu_long_attention_backward.py::test_one_train_step_matches_oracle_32px with the hybrid loss: the oracle UNet with
    out_dim = 2 and tests/_lv_ref.hybrid under fp64 autograd.  Bounds as there: loss 2e-5 relative, Adam update 2e-2."""
    unet, gd, tr = _mk(tmp_path, 'f32')
    cfg = U.UnetConfig(**TRAIN_KW)
    p0 = {k: v.detach().cpu().double().clone() for k, v in unet.state_dict().items()}
    g = torch.Generator().manual_seed(0)
    batch = torch.rand(*TRAIN_SHAPE, generator=g)
    loss_dev = tr.train_step(batch, step=0)
    torch.cuda.synchronize()
    t = tr.last_t.cpu().long()
    noise = torch.from_numpy(philox_ref.randn(batch.numel(), tr.last_noise_key, 0)).double().reshape(batch.shape)
    tab64 = R.tables(50)['tab64']
    parts = {}

    def loss_fn(params):
        ref = DiffusionRef(lambda a, b: U.unet_forward(params, cfg, a, b), image_size=16, num_frames=2, channels=1, timesteps=50,
                           loss_type='l2', dtype=F64)
        x0 = batch.double() * 2 - 1
        out2 = ref.denoise(ref.q_sample(x0, t, noise), t)
        r = R.hybrid(x0, noise, out2, t.to(torch.int32), tab64, l2=True, w=gd.vlb_weight)
        parts.update(mse=r['mse'].item(), vb=r['vb'].item())
        return r['loss']
    ref_loss, grads = train_ref.loss_and_grads(p0, loss_fn)
    print(f'[train] loss {loss_dev.item():.8f} ref {ref_loss.item():.8f} (mse {parts["mse"]:.6f}, vb {parts["vb"]:.6f} bits, w {gd.vlb_weight})')
    assert abs(loss_dev.item() - ref_loss.item()) < 2e-5 * max(1.0, abs(ref_loss.item()))
    terms = gd.last_loss_terms.cpu()
    assert terms.is_floating_point() and gd.last_loss_terms.device.type == 'cuda'
    assert abs(terms[0].item() - parts['mse']) < 2e-5 * max(1.0, parts['mse']) and abs(terms[1].item() - parts['vb']) < 2e-5 * max(1.0, parts['vb'])
    zeros = {k: torch.zeros_like(v) for k, v in p0.items()}
    lr = train_ref.lr_schedule(0, 1e-3)
    p1, m1, v1 = train_ref.adam_update(p0, grads, zeros, zeros, count=0, lr=lr)
    got = {k: v.detach().cpu().double() for k, v in unet.state_dict().items()}
    num = sum(((got[k] - p0[k]) - (p1[k] - p0[k])).pow(2).sum() for k in p0)
    den = sum((p1[k] - p0[k]).pow(2).sum() for k in p0)
    print(f'[train] Adam update rel-L2 vs oracle {(num / den).sqrt().item():.3e} (bound 2e-2)')
    assert (num / den).sqrt().item() < 2e-2, (num / den).sqrt().item()
    # the v half carries gradient: the variance columns of the final conv
    off = {n: (o, s) for n, s, o in unet.param_table}
    o, s = off['final_conv.layers.1.kernel']
    gk = tr.grads[o:o + int(np.prod(s))].reshape(s).cpu()
    ref_gk = grads['final_conv.layers.1.kernel']
    assert gk[..., 1].abs().max() > 0 and ref_gk[..., 1].abs().max() > 0
    rel = ((gk.double() - ref_gk).norm() / ref_gk.norm()).item()
    print(f'[train] final conv kernel gradient rel-L2 vs oracle {rel:.3e}')
    assert rel < 2e-2 and tr.opt_count == 1


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_train_step_is_bit_reproducible_and_finite(tmp_path, mode):
    """Two steps (bf16: operands + bf16 activation storage, the Trainer's default), twice from the same start: finite and bit-equal."""
    runs = []
    for r in range(2):
        unet, gd, tr = _mk(tmp_path / str(r), mode, loss_type='l1' if mode == 'bf16' else 'l2')
        assert tr.train_act_bf16
        g = torch.Generator().manual_seed(0)
        losses = [tr.train_step(torch.rand(*TRAIN_SHAPE, generator=g), step=s).item() for s in range(2)]
        torch.cuda.synchronize()
        assert all(np.isfinite(losses)) and torch.isfinite(unet.flat_params).all() and tr.opt_count == 2
        runs.append((losses, unet.flat_params.clone(), gd.last_loss_terms.clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


def test_train_step_three_channels_and_accumulation(tmp_path):
    """C = 3, out_dim = 6: the final-conv backward above 4 output channels inside the network; then the accumulation path."""
    unet, gd, tr = _mk(tmp_path, 'f32', C=3)
    g = torch.Generator().manual_seed(0)
    shape = (2, 3) + TRAIN_SHAPE[2:]
    with launches() as rec:
        loss = tr.train_step(torch.rand(*shape, generator=g), step=0)
    torch.cuda.synchronize()
    dw = [s for k, s in rec if k == 'final_conv_dw_kernel']
    assert dw and 'Cout6' in dw[0] and any(k == 'hybrid_loss_kernel' for k, _ in rec) and not any(k == 'loss_grad_kernel' for k, _ in rec)
    off = {n: (o, s) for n, s, o in unet.param_table}
    o, s = off['final_conv.layers.1.kernel']
    gk = tr.grads[o:o + int(np.prod(s))].reshape(s)
    assert np.isfinite(loss.item()) and torch.isfinite(unet.flat_params).all() and (gk.abs().amax(dim=tuple(range(gk.dim() - 1))) > 0).all()
    tr.apply_grad_args, tr.gradient_accumulate_every = True, 2
    loss = tr.train_step_accum([torch.rand(*shape, generator=g) for _ in range(2)], step=1)
    torch.cuda.synchronize()
    assert np.isfinite(loss.item()) and torch.isfinite(unet.flat_params).all() and tr.opt_count == 2
    # p_losses / __call__ return the total and keep the parts
    val = gd(torch.rand(*shape, generator=g), 4)
    mse, vb = gd.last_loss_terms.tolist()
    assert abs(val.item() - (mse + gd.vlb_weight * vb)) <= 1e-6 * abs(val.item())
    mean, var, logvar = gd.p_mean_variance(gd.randn(shape, 1), torch.tensor([3, 40]), True)
    assert mean.shape == var.shape == logvar.shape == shape and torch.isfinite(mean).all() and (var > 0).all()
    out = gd.p_sample(gd.randn(shape, 1), torch.tensor([0, 40]), 2)
    assert torch.isfinite(out).all()
