"""GPU tests of the DPM-Solver++(2M) sampler (EXTENSION, parity unpinned: no reference code): the fused step and its masked form against
the fp64 restatement of tests/_dpm_ref.py (itself pinned by tests/test_host_dpm.py), first order against vdx_ddim_step, second-order
convergence through the kernel, the captured loops against the restated loops on the oracle UNet, graph slots, the dynamic threshold,
guidance and the north-star shape."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _dpm_ref as D
from _dpm_ref import R
from _launch_hook import launches
from oracle import philox_ref
from oracle.diffusion_ref import DiffusionRef

DEV = 'cuda:0'
T_STEP, S_STEP = 1000, 20
B, C, SHAPE = 3, 2, (3, 2, 4, 8, 8)
PER = 2 * 4 * 8 * 8
STEP_KS = (0, 1, 11, 19)                 # first order, the first second-order step, the middle, the step into the data
STEP_TOL = 2e-5                          # x max(1, |ref|max): the DDIM step test's bound


@functools.lru_cache(None)
def _step_inputs():
    from video_diffusion_nnx_amd.gaussian_diffusion import ddim_time_sequence, make_tables
    g = torch.Generator().manual_seed(3)
    x = torch.randn(SHAPE, generator=g)
    eps = torch.randn(B, 4, 8, 8, C, generator=g)                        # channel-last, as the UNet writes it
    hist = torch.randn(SHAPE, generator=g).clamp(-1, 1)
    known = 2 * torch.rand(SHAPE, generator=g) - 1
    mask = (torch.rand(SHAPE, generator=g) < 0.5).to(torch.uint8)
    ac = torch.from_numpy(make_tables(T_STEP)['alphas_cumprod'])
    seq = ddim_time_sequence(T_STEP, S_STEP)
    return dict(x=x, eps=eps, hist=hist, known=known, mask=mask, ac=ac, seq=seq, thres=torch.tensor([1.0, 1.7, 3.2]))


def _run_step(k, order, clip, thres, hist, masked=None, seed=17):
    """vdx_dpm_step(_masked) on the shared inputs at step k; returns (out, hist after) on the host."""
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd.gaussian_diffusion import make_tables, vdx_dpm_step, vdx_dpm_step_masked
    I = _step_inputs()
    xd, ed, acd, seqd = I['x'].to(DEV), I['eps'].to(DEV), I['ac'].to(DEV), torch.from_numpy(I['seq']).to(DEV)
    hd = None if hist is None else hist.to(DEV).clone()
    td = None if thres is None else thres.to(DEV)
    step = torch.full((1,), k, dtype=torch.int64, device=DEV)
    out = torch.empty_like(xd)
    if masked is None:
        L.check(vdx_dpm_step(L.ptr(xd), L.ptr(ed), L.ptr(out), L.ptr(hd), L.ptr(acd), L.ptr(seqd), L.ptr(step), L.ptr(td), int(clip), order,
                             B, C, PER, L.stream_ptr()))
    else:
        tabs = make_tables(T_STEP)
        mtab = torch.from_numpy(np.stack([tabs['sqrt_alphas_cumprod'], tabs['sqrt_one_minus_alphas_cumprod']])).to(DEV).contiguous()
        kd, md = I['known'].to(DEV), masked.to(DEV)
        L.check(vdx_dpm_step_masked(L.ptr(xd), L.ptr(ed), L.ptr(out), L.ptr(hd), L.ptr(acd), L.ptr(seqd), L.ptr(step), L.ptr(td), int(clip), order,
                                    L.ptr(kd), L.ptr(md), L.ptr(mtab), T_STEP, seed, B, C, PER, L.stream_ptr()))
    return out.cpu(), None if hd is None else hd.cpu()


def _ref_step(k, order, clip, thres):
    I = _step_inputs()
    return D.dpm_step(I['x'].double(), I['eps'].permute(0, 4, 1, 2, 3).double(), I['hist'].double(), I['ac'].double(), I['seq'], k, order, clip,
                      None if thres is None else thres.double())


def _close(got, ref, what):
    err, lim = (got.double() - ref).abs().max().item(), STEP_TOL * max(1.0, ref.abs().max().item())
    print(f'{what}: max-abs error {err:.3e}, bound {lim:.3e}')
    assert err < lim, (what, err, lim)


@pytest.mark.parametrize('clip,per_sample_thres', [(True, False), (True, True), (False, False)])
def test_dpm_step_matches_restatement(clip, per_sample_thres):
    thres = _step_inputs()['thres'] if per_sample_thres else None
    for k in STEP_KS:
        out, hist = _run_step(k, 2, clip, thres, _step_inputs()['hist'])
        ref_out, ref_x0 = _ref_step(k, 2, clip, thres)
        _close(out, ref_out, f'out k={k} clip={clip} thres={per_sample_thres}')
        _close(hist, ref_x0, f'hist k={k} clip={clip} thres={per_sample_thres}')
        if k == S_STEP - 1:
            assert torch.equal(out, hist)                                # the step into the data returns x0 itself
            assert not clip or out.abs().max().item() <= 1.0


@pytest.mark.parametrize('clip,per_sample_thres', [(True, False), (True, True), (False, False)])
def test_dpm_first_order_is_the_ddim_step(clip, per_sample_thres):
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd.gaussian_diffusion import vdx_ddim_step
    I = _step_inputs()
    thres = I['thres'] if per_sample_thres else None
    xd, ed, acd, seqd = I['x'].to(DEV), I['eps'].to(DEV), I['ac'].to(DEV), torch.from_numpy(I['seq']).to(DEV)
    td = None if thres is None else thres.to(DEV)
    for k in STEP_KS:
        out, _ = _run_step(k, 1, clip, thres, None)                      # order 1 needs no history tensor
        with_hist, hist = _run_step(k, 1, clip, thres, I['hist'])
        assert torch.equal(out, with_hist)
        _close(hist, _ref_step(k, 1, clip, thres)[1], f'order-1 hist k={k}')
        step = torch.full((1,), k, dtype=torch.int64, device=DEV)
        ddim = torch.empty_like(xd)
        L.check(vdx_ddim_step(L.ptr(xd), L.ptr(ed), L.ptr(ddim), L.ptr(acd), L.ptr(seqd), L.ptr(step), L.ptr(td), int(clip), B, C, PER, L.stream_ptr()))
        _close(out, ddim.cpu().double(), f'order 1 vs ddim k={k} clip={clip} thres={per_sample_thres}')
        _close(out, _ref_step(k, 1, clip, thres)[0], f'order 1 vs restatement k={k}')


def test_dpm_step_rejects_bad_arguments():
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd.gaussian_diffusion import vdx_dpm_step
    x = torch.zeros(1, 1, 1, 2, 4, device=DEV)
    eps, ac = torch.zeros(1, 1, 2, 4, 1, device=DEV), torch.full((4,), 0.5, device=DEV)
    seq = torch.tensor([3, 1, -1], dtype=torch.int32, device=DEV)

    def call(hist, order, per=8, xp=None):
        return vdx_dpm_step(L.ptr(x) if xp is None else xp, L.ptr(eps), L.ptr(x), L.ptr(hist), L.ptr(ac), L.ptr(seq), 0, 0, 1, order, 1, 1, per, L.stream_ptr())
    assert call(torch.zeros_like(x), 2) == 0
    assert call(None, 1) == 0
    assert call(None, 2) != 0                                             # order 2 needs hist
    assert call(torch.zeros_like(x), 3) != 0 and call(torch.zeros_like(x), 0) != 0
    assert call(torch.zeros_like(x), 2, per=6) != 0                       # four elements per thread
    assert call(torch.zeros_like(x), 2, xp=L.ptr(x) + 4) != 0             # float4 alignment
    torch.cuda.synchronize()


def test_dpm_masked_step():
    I = _step_inputs()
    seed = 17
    for k in STEP_KS:
        for clip in (False, True):
            plain, plain_hist = _run_step(k, 2, clip, None, I['hist'])
            zero, zero_hist = _run_step(k, 2, clip, None, I['hist'], masked=torch.zeros_like(I['mask']))
            assert torch.equal(zero, plain) and torch.equal(zero_hist, plain_hist), k        # an all-zero mask: bit for bit
        out, hist = _run_step(k, 2, True, None, I['hist'], masked=I['mask'], seed=seed)
        xp, x0 = _ref_step(k, 2, True, None)
        tn = int(I['seq'][k + 1])
        kn = I['known'].double()
        if tn >= 0:
            a_n = I['ac'].double()[tn]
            z = torch.from_numpy(philox_ref.randn(int(np.prod(SHAPE)), seed, D.DRAW_KNOWN + k)).double().reshape(SHAPE)
            kn = a_n.sqrt() * kn + (1 - a_n).sqrt() * z
        else:
            assert torch.equal(out[I['mask'].bool()], I['known'][I['mask'].bool()])          # the data end: known elements exactly
        _close(out, torch.where(I['mask'].bool(), kn, xp), f'masked out k={k}')
        _close(hist, x0, f'masked hist k={k}')                            # the network's x0 everywhere
        assert torch.equal(hist, plain_hist)


def test_dpm_converges_at_second_order_through_the_kernel():
    """The host test's Gaussian check (sigma^2 = 0.25, T = 1000, no clipping) with vdx_dpm_step as the step and the analytic denoiser
    evaluated in torch on the device."""
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd.gaussian_diffusion import ddim_time_sequence, make_tables, vdx_dpm_step
    shape = (2, 1, 2, 8, 8)
    ac = torch.from_numpy(make_tables(T_STEP)['alphas_cumprod'])
    acd, ac64 = ac.to(DEV), ac.double().to(DEV)
    x_T = torch.randn(shape, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    exact = D.gaussian_exact(x_T, ac.double()[T_STEP - 1])
    err = {}
    for order in (1, 2):
        for S in (10, 20):
            seq = ddim_time_sequence(T_STEP, S)
            seqd = torch.from_numpy(seq).to(DEV)
            x, hist = x_T.float().to(DEV), torch.zeros(shape, device=DEV)
            step = torch.zeros(1, dtype=torch.int64, device=DEV)
            for k in range(S):
                eps = D.gaussian_eps(x.double(), ac64[int(seq[k])]).float().reshape(2, 2, 8, 8, 1).contiguous()
                step.fill_(k)
                L.check(vdx_dpm_step(L.ptr(x), L.ptr(eps), L.ptr(x), L.ptr(hist), L.ptr(acd), L.ptr(seqd), L.ptr(step), 0, 0, order,
                                     2, 1, 2 * 8 * 8, L.stream_ptr()))
            err[order, S] = D.rel_err(x.cpu().double(), exact)
    print('relative L2 error vs the exact ODE solution:', {k: round(v, 4) for k, v in err.items()})
    assert err[2, 20] <= err[1, 20] / 10
    assert err[2, 10] / err[2, 20] >= 4


# ---- the loops: dim 16, channels 1, dim_mults (1, 2), f32, T = 60, S = 12, (2, 1, 4, 8, 8) ----

KW = dict(dim=16, channels=1, dim_mults=(1, 2))
T_LOOP, S_LOOP, LOOP_SHAPE, SEED = 60, 12, (2, 1, 4, 8, 8), 11
LOOP_TOL = 5e-4                          # the DDIM loop test's bound


@functools.lru_cache(None)
def _params():
    cfg = R.UnetConfig(**KW)
    return cfg, R.random_params(cfg, seed=2, dtype=torch.float64)


def _ref(**gkw):
    cfg, p = _params()
    return DiffusionRef(lambda a, b: R.unet_forward(p, cfg, a, b), image_size=8, num_frames=4, channels=1, timesteps=T_LOOP, dtype=torch.float64, **gkw)


def _gd(**gkw):
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.unet3d import Unet3D
    unet = Unet3D(rngs=0, mode='f32', **KW)
    unet.load_state_dict({k: v.float() for k, v in _params()[1].items()})
    return GaussianDiffusion(unet, image_size=8, num_frames=4, channels=1, timesteps=T_LOOP, **gkw)


def _x_T(seed=SEED):
    return torch.from_numpy(philox_ref.randn(int(np.prod(LOOP_SHAPE)), seed, 0)).double().reshape(LOOP_SHAPE)


@functools.lru_cache(None)
def _expected_loop():
    return (D.dpm_loop(_ref(), _x_T(), S_LOOP) + 1) * 0.5


@functools.lru_cache(None)
def _video_and_mask():
    video = torch.rand(LOOP_SHAPE, generator=torch.Generator().manual_seed(7))
    return video, torch.tensor([True, True, False, False])


def _forwards(rec):
    return sum(k.startswith('final_conv') for k, _ in rec), sum(k == 'dpm_step_kernel' for k, _ in rec)


@pytest.mark.parametrize('use_graph', [True, False])
def test_dpm_sample_loop_matches_restated_loop(use_graph):
    gd = _gd()
    with launches() as rec:
        out = gd.dpm_sample_loop(LOOP_SHAPE, SEED, steps=S_LOOP, use_graph=use_graph)
        torch.cuda.synchronize()
    # one UNet forward per step: the eager loop issues S of them; the graph loop issues one eager step and one captured step, the
    # S - 1 replays launch nothing from the host
    assert _forwards(rec) == ((2, 2) if use_graph else (S_LOOP, S_LOOP)), rec
    err = (out.cpu().double() - _expected_loop()).abs().max().item()
    print(f'dpm loop use_graph={use_graph}: max-abs error vs the restated loop {err:.3e}, bound {LOOP_TOL:.1e}')
    assert err < LOOP_TOL, err
    with launches() as rec:
        again = gd.sample(SEED, batch_size=2, dpm_steps=S_LOOP, use_graph=use_graph)      # deterministic given the seed
        torch.cuda.synchronize()
    assert torch.allclose(again, out, atol=1e-5)                 # (f64 atomics of the GroupNorm statistics: last-bit jitter only)
    assert _forwards(rec)[0] in ((0, 2) if use_graph else (S_LOOP,)), rec      # 0: the cached graph was reused (same buffers again)
    first = gd.sample(SEED, batch_size=2, dpm_steps=S_LOOP, dpm_order=1, use_graph=use_graph)
    ddim = gd.sample(SEED, batch_size=2, ddim_steps=S_LOOP, use_graph=use_graph)
    assert (first - ddim).abs().max().item() < 2 * LOOP_TOL      # order 1 is DDIM through the loop too: the closed forms agree to 1e-12
                                                                 # (host test) and each fp32 loop is within LOOP_TOL of its own
    assert (first - out).abs().max().item() > 1e-3               # and order 2 is another sampler


def test_dpm_loop_in_pieces_keeps_the_history():
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd.gaussian_diffusion import ddim_time_sequence, vdx_dpm_sample_loop
    gd = _gd()
    unet = gd.denoise_fn
    Bn = LOOP_SHAPE[0]
    h = unet.handle(4, 8)
    unet.apply_activation_storage(h)
    ws = unet.workspace(Bn, 4, 8)
    seq_host = ddim_time_sequence(T_LOOP, S_LOOP)
    st = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(st):
        seq = torch.from_numpy(seq_host).to(DEV)
        x_T = gd.randn(LOOP_SHAPE, SEED, 0)
        eps = torch.empty(Bn, 4, 8, 8, 1, device=DEV)
        img, hist = torch.empty_like(x_T), torch.empty_like(x_T)

        def chain(pieces, graph):
            img.copy_(x_T)
            hist.fill_(float('nan'))                             # never read before step 0 has written it
            t_dev = torch.full((Bn,), int(seq_host[0]), dtype=torch.int32, device=DEV)
            step_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
            states = []
            for n in pieces:
                L.check(vdx_dpm_sample_loop(h.ptr, L.ptr(unet.flat_params), L.ptr(unet.packed()), L.ptr(img), L.ptr(eps), L.ptr(hist), L.ptr(t_dev),
                                            L.ptr(step_dev), L.ptr(gd.alphas_cumprod), L.ptr(seq), S_LOOP, n, 0, 1, 2, 0, 0, 0.0, 0,
                                            L.ptr(ws), ws.numel(), Bn, graph, L.stream_ptr()))
                st.synchronize()
                states.append((img.clone(), hist.clone(), int(step_dev.item()), t_dev.cpu().tolist()))
            return states
        whole = chain([S_LOOP], 1)
        pieces = chain([5, 7], 1)
        eager = chain([5, 7], 0)
    assert pieces[0][2] == 5 and pieces[0][3] == [int(seq_host[5])] * Bn and pieces[1][2] == S_LOOP
    for other in (pieces, eager):
        assert torch.allclose(other[-1][0], whole[-1][0], atol=1e-5)
    assert torch.allclose(pieces[0][0], eager[0][0], atol=1e-5) and torch.allclose(pieces[0][1], eager[0][1], atol=1e-5)
    assert torch.equal(whole[-1][0], whole[-1][1])               # the step into the data: img = hist = x0
    ref = _ref()
    x5 = D.dpm_loop(ref, _x_T(), S_LOOP, steps=5)
    assert (pieces[0][0].cpu().double() - x5).abs().max().item() < 2 * LOOP_TOL * max(1.0, x5.abs().max().item())    # x, not (x + 1) / 2
    assert ((whole[-1][0].cpu().double() + 1) / 2 - _expected_loop()).abs().max().item() < LOOP_TOL


def test_inpaint_dpm_loop_and_graph_slots():
    gd = _gd()
    video, mask = _video_and_mask()
    before = (gd.ddim_sample_loop(LOOP_SHAPE, SEED, steps=S_LOOP), gd.p_sample_loop(LOOP_SHAPE, SEED),
              gd.inpaint(SEED, video, mask, ddim_steps=S_LOOP), gd.inpaint(SEED, video, mask))
    out = gd.inpaint(SEED, video, mask, dpm_steps=S_LOOP)
    exp = D.dpm_loop_masked(_ref(), video, mask.reshape(1, 1, 4, 1, 1).expand(LOOP_SHAPE), SEED, S_LOOP)
    err = (out.cpu().double() - exp).abs().max().item()
    print(f'masked dpm loop: max-abs error vs the restated loop {err:.3e}, bound {LOOP_TOL:.1e}')
    assert err < LOOP_TOL, err
    assert (out[:, :, :2].cpu() - video[:, :, :2]).abs().max().item() <= 1e-6           # known frames up to the affine rounding
    assert torch.allclose(gd.inpaint(SEED, video, mask, dpm_steps=S_LOOP, use_graph=False), out, atol=1e-5)
    empty = gd.inpaint(SEED, video, torch.zeros(4, dtype=torch.bool), dpm_steps=S_LOOP)
    plain = gd.dpm_sample_loop(LOOP_SHAPE, SEED, steps=S_LOOP)
    assert (empty - plain).abs().max().item() <= 1e-5
    assert (plain.cpu().double() - _expected_loop()).abs().max().item() < LOOP_TOL
    after = (gd.ddim_sample_loop(LOOP_SHAPE, SEED, steps=S_LOOP), gd.p_sample_loop(LOOP_SHAPE, SEED),
             gd.inpaint(SEED, video, mask, ddim_steps=S_LOOP), gd.inpaint(SEED, video, mask))
    for a, b in zip(before, after):                              # the dpm loops have graph slots of their own
        assert torch.allclose(a, b, atol=1e-5)
    ext = gd.extend(SEED, video[:, :, :2], 2, context_frames=2, dpm_steps=S_LOOP)
    assert ext.shape == (2, 1, 4, 8, 8) and torch.equal(ext[:, :, :2].cpu(), video[:, :, :2])


def test_dpm_dynamic_threshold_in_the_graph_loop():
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd.gaussian_diffusion import ddim_time_sequence, vdx_dpm_step
    gd = _gd(use_dynamic_thres=True, dynamic_thres_percentile=0.9)
    out = gd.dpm_sample_loop(LOOP_SHAPE, SEED, steps=S_LOOP)
    # the eager composition: Unet3D forward, vdx_dynamic_threshold, vdx_dpm_step
    seq_host = ddim_time_sequence(T_LOOP, S_LOOP)
    seq = torch.from_numpy(seq_host).to(DEV)
    img = gd.randn(LOOP_SHAPE, SEED, 0)
    hist = torch.empty_like(img)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    seen = []
    for k in range(S_LOOP):
        t = torch.full((2,), int(seq_host[k]), dtype=torch.int32, device=DEV)
        eps = gd.denoise_fn(img, t)
        thres = gd._dynamic_threshold(img, t, eps)
        seen.append(thres.max().item())
        step.fill_(k)
        L.check(vdx_dpm_step(L.ptr(img), L.ptr(eps), L.ptr(img), L.ptr(hist), L.ptr(gd.alphas_cumprod), L.ptr(seq), L.ptr(step), L.ptr(thres), 1, 2,
                             2, 1, 4 * 8 * 8, L.stream_ptr()))
    err = (out - (img + 1) / 2).abs().max().item()
    print(f'dynamic threshold: graph loop vs eager composition {err:.3e}')
    assert err < 1e-5, err                                       # the same kernels on the same inputs: last-bit jitter only
    assert max(seen) > 1.0                                       # the threshold is really above the static clip somewhere
    exp = (D.dpm_loop(_ref(use_dynamic_thres=True, dynamic_thres_percentile=0.9), _x_T(), S_LOOP) + 1) * 0.5
    err = (out.cpu().double() - exp).abs().max().item()
    print(f'dynamic threshold: graph loop vs the restated loop {err:.3e}')
    assert err < 1e-3, err                                       # the bound of the dynamic-threshold DDIM loop
    static = _gd().dpm_sample_loop(LOOP_SHAPE, SEED, steps=S_LOOP)
    assert (static - out).abs().max().item() > 1e-4


def test_dpm_guided_path():
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.unet3d import Unet3D
    unet = Unet3D(rngs=0, mode='f32', dim=16, channels=1, cond_dim=32)
    gd = GaussianDiffusion(unet, image_size=8, num_frames=2, channels=1, timesteps=T_LOOP)
    cond = torch.randn(2, 32, generator=torch.Generator().manual_seed(9)).to(DEV)
    out = gd.sample(5, cond=cond, cond_scale=2.0, dpm_steps=6)
    assert out.shape == (2, 1, 2, 8, 8) and torch.isfinite(out).all()
    assert 0.0 <= out.min().item() and out.max().item() <= 1.0
    assert torch.allclose(gd.sample(5, cond=cond, cond_scale=2.0, dpm_steps=6), out, atol=1e-5)
    assert (gd.sample(6, cond=cond, cond_scale=2.0, dpm_steps=6) - out).abs().max().item() > 1e-3
    assert (gd.sample(5, cond=cond, cond_scale=1.0, dpm_steps=6) - out).abs().max().item() > 1e-4     # guidance does something


def test_dpm_north_star_shape_bf16():
    """dim 64, 16 frames x 64^2, B 2, bf16 operands + bf16 activation storage, T 1000, S 4 through the captured loop."""
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.unet3d import Unet3D
    unet = Unet3D(rngs=0, mode='bf16', dim=64, channels=1)
    gd = GaussianDiffusion(unet, image_size=64, num_frames=16, channels=1, timesteps=1000)
    out = gd.sample(77, batch_size=2, dpm_steps=4)
    assert out.shape == (2, 1, 16, 64, 64) and torch.isfinite(out).all()
    assert 0.0 <= out.min().item() and out.max().item() <= 1.0
    assert torch.allclose(gd.sample(77, batch_size=2, dpm_steps=4), out, atol=1e-5)
    assert unet.act_bf16 is False                                # the sampling-time storage switch is put back
