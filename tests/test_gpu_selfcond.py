"""Self-conditioning on the GPU (vdx.h: "Self-conditioning"): selfcond_x0_kernel bit for bit against the fp32 restatement
tests/_selfcond_ref.py, the three chains captured = eager = stepped by hand from public pieces, and the two-pass train step against the same
step done by hand.  Every bound here is bit equality: the contract states the kernel's roundings one by one, and everything around it is an
existing kernel on the same bits."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _selfcond_ref as R                # noqa: E402
from _launch_hook import launches        # noqa: E402
from oracle import unet3d_ref as U       # noqa: E402

DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
T = 10


def _dev(t, dtype=None):
    return t.detach().to(dtype or t.dtype).to(DEV).contiguous()


@functools.lru_cache(None)
def _tabs():
    """(the [5][T] step tables, sqrt_ac, sqrt_1mac) on the host, float32."""
    from video_diffusion_nnx_amd.gaussian_diffusion import make_tables
    t = {k: torch.from_numpy(v) for k, v in make_tables(T).items()}
    ptab = torch.stack([t['sqrt_recip_alphas_cumprod'], t['sqrt_recipm1_alphas_cumprod'], t['posterior_mean_coef1'], t['posterior_mean_coef2'],
                        t['posterior_log_variance_clipped']]).contiguous()
    return ptab, t['sqrt_alphas_cumprod'], t['sqrt_one_minus_alphas_cumprod']


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------------------------

# (B, C, F, S or (1, fhw)): channel mapping with per % 4 = 2 | C = 1 with sample bases off 16 bytes (per = 75) | 2 100 004 floats per sample:
# the second trip of the grid-stride loop of a 2048 x 256 x 4 grid, fhw odd (tests/_step_cases.py: WRAP)
KSHAPES = {'c3': (2, 3, 2, 5, 5), 'c1': (2, 1, 3, 5, 5), 'wrap': (2, 4, 1, 1, 525001)}
MODES = ('noclip', 'clip', 'thres', 'pred_v', 'clamp')
# (the wrap shape is about the loop, not the arguments: clip / thres / pred_v cover it)
KCASES = [(n, m) for n in KSHAPES for m in MODES if not (n == 'wrap' and m in ('noclip', 'clamp'))]


@functools.lru_cache(None)
def _kernel_inputs(name):
    B, C, Fr, H, W = KSHAPES[name]
    g = torch.Generator().manual_seed(len(name) + C)
    x = torch.randn(B, C, Fr, H, W, generator=g) * 1.5
    out = torch.randn(B, Fr, H, W, C, generator=g)
    return x, out


@pytest.mark.parametrize('in_xin', [False, True], ids=['img', 'xin'])
@pytest.mark.parametrize('name,mode', KCASES)
def test_selfcond_x0_bit_for_bit(name, mode, in_xin):
    """in_xin: x is the first half of the xin buffer itself (pitch 2 per_sample) and the estimate goes into its second half -- the
    training form; otherwise x is a tensor of its own (pitch per_sample) -- the loops' form."""
    from video_diffusion_nnx_amd import _lib as L
    B, C, Fr, H, W = KSHAPES[name]
    per = C * Fr * H * W
    x, out = _kernel_inputs(name)
    ptab, sa, s1 = _tabs()
    t = torch.tensor([-2, T + 3] if mode == 'clamp' else [0, T - 1], dtype=torch.int32)
    thres = torch.tensor([1.25, 2.5]) if mode == 'thres' else None
    clip = mode != 'noclip'
    sentinel = -7.25
    xin = torch.full((B, 2 * C, Fr, H, W), sentinel, dtype=F32, device=DEV)
    xd = _dev(x)
    if in_xin:
        xin[:, :C] = xd
    outd, td = _dev(out), _dev(t)
    # (every device operand has a name: a temporary is released when its pointer has been taken, and the next one may get its block)
    ptabd, sad, s1d, thresd = _dev(ptab), _dev(sa), _dev(s1), None if thres is None else _dev(thres)
    eps_ref = out
    names = ['selfcond_x0_kernel']
    with launches() as rec:
        if mode == 'pred_v':
            L.check(L.vdx_v_to_eps(L.ptr(outd), L.ptr(xd), L.ptr(td), L.ptr(sad), L.ptr(s1d), T, B, C, per, L.stream_ptr()))
            shape = (-1, 1, 1, 1, 1)
            eps_cf = sa[t.long()].reshape(shape) * R.to_channel_first(out) + s1[t.long()].reshape(shape) * x       # vdx.h: fp32, no fma
            eps_ref = eps_cf.permute(0, 2, 3, 4, 1).contiguous()
            names = ['v_to_eps_kernel'] + names
        src, pitch = (xin, 2 * per) if in_xin else (xd, per)
        L.check(L.vdx_selfcond_x0(src.data_ptr(), pitch, L.ptr(outd), L.ptr(td), L.ptr(ptabd), T, L.ptr(thresd), int(clip), L.ptr(xin), B, C, per,
                                  L.stream_ptr()))
    torch.cuda.synchronize()
    assert [k for k, _ in rec] == names, rec
    if mode == 'pred_v':
        assert torch.equal(outd.cpu(), eps_ref), 'v_to_eps is not its fp32 restatement'
    got = xin.cpu()
    want = R.x0_estimate(x, eps_ref, t, ptab, clip=clip, thres=thres)
    assert torch.equal(got[:, C:], want), f'{(got[:, C:] - want).abs().max().item():.3e}'
    assert torch.equal(got[:, :C], x) if in_xin else bool((got[:, :C] == sentinel).all()), 'planes [0, C) were written'
    if clip:
        assert want.abs().max() <= 1.0 and (want.abs() == 1.0).any() and (want.abs() < 1.0).any()     # (the clip binds, and not everywhere)


# ---- 2. the chains ----------------------------------------------------------------------------------------------------------------------------

NET_KW = dict(dim=16, dim_mults=(1, 2), channels=2, out_dim=1)       # the tiny 2C network of tests/test_gpu_superres.py
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
    if 'lowres_cond' not in kw:
        kw.setdefault('self_condition', True)
    return GaussianDiffusion(unet or _net(), image_size=8, num_frames=4, channels=1, timesteps=T, **kw)


def _hand_chain(gd, chain, seed, steps=4):
    """The chain stepped by hand from public pieces: torch.cat([img, x0~]) -> unet -> (the pred_v conversion, the dynamic threshold) ->
    the restated x0~ -> the public step entry."""
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd import gaussian_diffusion as G
    unet = gd.denoise_fn
    B, per = SHAPE[0], int(np.prod(SHAPE[1:]))
    img = gd.randn(SHAPE, seed, 0)
    est = torch.zeros_like(img)
    hist = torch.empty_like(img)
    step_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
    seq_host = None if chain == 'ddpm' else G.ddim_time_sequence(T, steps)
    seq = None if seq_host is None else _dev(torch.from_numpy(seq_host))
    to_eps = gd._eps_from_out if gd.objective == 'pred_v' else None
    thres_of = gd._dynamic_threshold if gd.use_dynamic_thres else None
    for k in range(T if chain == 'ddpm' else steps):
        t = torch.full((B,), T - 1 - k if chain == 'ddpm' else int(seq_host[k]), dtype=torch.int32, device=DEV)
        eps, est, s = R.self_cond_step(unet, img, est, t, gd._ptab, to_eps=to_eps, thres_of=thres_of)
        step_dev.fill_(k)
        if chain == 'ddpm':
            L.check(G.vdx_p_sample_step(L.ptr(img), L.ptr(eps), L.ptr(img), L.ptr(t), L.ptr(gd._ptab), T, 0, seed, 1 + k, 0, L.ptr(s), 1, B, 1, per,
                                        L.stream_ptr()))
        elif chain == 'ddim':
            L.check(G.vdx_ddim_step(L.ptr(img), L.ptr(eps), L.ptr(img), L.ptr(gd.alphas_cumprod), L.ptr(seq), L.ptr(step_dev), L.ptr(s), 1, B, 1, per,
                                    L.stream_ptr()))
        else:
            L.check(G.vdx_dpm_step(L.ptr(img), L.ptr(eps), L.ptr(img), L.ptr(hist), L.ptr(gd.alphas_cumprod), L.ptr(seq), L.ptr(step_dev), L.ptr(s), 1, 2,
                                   B, 1, per, L.stream_ptr()))
    out = torch.empty_like(img)
    L.check(G.vdx_affine(L.ptr(img), L.ptr(out), img.numel(), 0.5, 0.5, L.stream_ptr()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('chain,variant', [('ddpm', 'plain'), ('ddim', 'plain'), ('dpm', 'plain'), ('ddim', 'pred_v'), ('ddpm', 'dyn'), ('dpm', 'dyn')])
def test_chains(chain, variant):
    """Captured == eager == the chain stepped by hand, bit for bit; a second call on the kept buffers reproduces the first (the second
    half of xin is zeroed again); the result is not that of the same network with the state off; a super-resolution diffusion that shares
    the Unet3D gives its old bits before and after."""
    from video_diffusion_nnx_amd import _lib as L
    unet = _net()
    extra = {'plain': {}, 'pred_v': dict(objective='pred_v'), 'dyn': dict(use_dynamic_thres=True, dynamic_thres_percentile=0.7)}[variant]
    gd = _gd(unet, **extra)
    # the same network with the state off: a super-resolution diffusion whose u = up(2 * 0.5 - 1) is zero in every step
    sr = _gd(unet, lowres_cond=(1, 1), **extra)
    half = torch.full(SHAPE, 0.5)
    kw = {'ddpm': {}, 'ddim': dict(ddim_steps=4), 'dpm': dict(dpm_steps=4, dpm_order=2)}[chain]
    nsteps = T if chain == 'ddpm' else 4
    seed = 21
    off_before = sr.upsample(seed, half, **kw)
    with launches() as rec:
        eager = gd.sample(seed, batch_size=2, use_graph=False, **kw)
    torch.cuda.synchronize()
    names = [k for k, _ in rec]
    step_kernel = {'ddpm': 'p_sample_kernel', 'ddim': 'ddim_step_kernel', 'dpm': 'dpm_step_kernel'}[chain]
    assert names.count('selfcond_x0_kernel') == nsteps and names.count('lowres_pack_kernel') == nsteps and names.count(step_kernel) == nsteps, names
    assert 'lowres_input_kernel' not in names
    first = names.index('selfcond_x0_kernel')
    assert names.index('lowres_pack_kernel') < first < names.index(step_kernel), names          # behind the forward, before the step kernel
    if variant == 'pred_v':
        assert names.count('v_to_eps_kernel') == nsteps and names.index('v_to_eps_kernel') < first, names
    h = unet.handle(4, 8)
    assert L.vdx_get_self_condition(h.ptr) == 0 and L.vdx_get_prediction(h.ptr) == 0           # (put back on the way out)
    hand = _hand_chain(gd, chain, seed)
    assert torch.equal(eager, hand), f'{chain} {variant}: the eager loop is not the hand-stepped chain bit for bit'
    graph = gd.sample(seed, batch_size=2, use_graph=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(graph, eager), f'{chain} {variant}: captured != eager'
    assert eager.shape == SHAPE and torch.isfinite(eager).all() and eager.min() >= 0 and eager.max() <= 1
    # the kept buffers hold the last estimate of that chain: a second call starts from zero again, replaying the cached graph
    with launches() as rec:
        again = gd.sample(seed, batch_size=2, use_graph=True, **kw)
    torch.cuda.synchronize()
    assert 'selfcond_x0_kernel' not in [k for k, _ in rec] and torch.equal(again, graph), 'the second call on the kept buffers differs'
    # the loop entries by their own names are the same chain
    loop = {'ddpm': lambda: gd.p_sample_loop(SHAPE, seed), 'ddim': lambda: gd.ddim_sample_loop(SHAPE, seed, steps=4),
            'dpm': lambda: gd.dpm_sample_loop(SHAPE, seed, steps=4)}[chain]
    assert torch.equal(loop(), graph)
    # the state does something, and leaves nothing behind on the shared network
    off_after = sr.upsample(seed, half, **kw)
    torch.cuda.synchronize()
    assert torch.equal(off_before, off_after), 'a super-resolution diffusion on the same Unet3D changed its bits'
    assert not torch.equal(off_after, graph), 'the self-conditioned chain is the chain with the state off'


def test_single_step_api():
    """p_sample / p_mean_variance with x_self_cond are the step of the loop's pieces; None is zeros; self_cond_estimate is the kernel."""
    gd = _gd()
    x = gd.randn(SHAPE, 4, 0)
    t = torch.tensor([T - 1, 0], dtype=torch.int32)
    est0 = torch.zeros_like(x)
    out = gd.denoise_fn(torch.cat([x, est0], dim=1), _dev(t))
    est = gd.self_cond_estimate(x, t, out)
    torch.cuda.synchronize()
    assert est.shape == SHAPE and est.is_contiguous()
    assert torch.equal(est.cpu(), R.x0_estimate(x.cpu(), out.cpu(), t, gd._ptab.cpu()))
    xin = torch.full((2, 2, 4, 8, 8), 3.0, device=DEV)
    view = gd.self_cond_estimate(x, t, out, xin=xin)
    assert torch.equal(view, est) and bool((xin[:, :1] == 3.0).all()) and view.data_ptr() == xin[:, 1:].data_ptr()
    a = gd.p_sample(x, t, 8)
    b = gd.p_sample(x, t, 8, x_self_cond=est0)
    c = gd.p_sample(x, t, 8, x_self_cond=est)
    mean, var, logvar = gd.p_mean_variance(x, t, True, x_self_cond=est)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not torch.equal(a, c) and torch.isfinite(c).all()
    assert torch.equal(c[1], mean[1]) and not torch.equal(c[0], mean[0])                         # t = 0 adds no noise


# ---- 3. the train step ------------------------------------------------------------------------------------------------------------------------

def _trainer(tmp_path, gd, **kw):
    from video_diffusion_nnx_amd.trainer import Trainer
    return Trainer(gd, str(tmp_path), dataset_path='synthetic:8', train_batch_size=2, train_num_steps=3, train_lr=1e-3,
                   checkpoint_every_steps=2, results_folder=str(tmp_path / 'res'), step_start_ema=0, update_ema_every=1, ema_decay=0.9, **kw)


def _train_inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(SHAPE, generator=g), torch.tensor([T - 1, 1], dtype=torch.int32), torch.randn(SHAPE, generator=g)


def _hand_step(batch, t, noise, self_cond, **gd_kw):
    """(loss, flat gradient) of one step done by hand on a fresh network: q_sample, pass 1 -> the restated x0~ (or zeros), pass 2 on the
    fixed xin, the existing loss and gradient kernels, unet.backward."""
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd.gaussian_diffusion import vdx_loss_sum
    from video_diffusion_nnx_amd.train_step import vdx_loss_grad
    unet = _net()
    gd = _gd(unet, loss_type='l2', **gd_kw)
    x, td, nz = _dev(batch), _dev(t), _dev(noise)
    x_t = gd.q_sample(x, td, noise=nz, _pre=(2.0, -1.0))
    est = torch.zeros_like(x_t)
    if self_cond:
        out1 = unet(torch.cat([x_t, est], dim=1), td)
        eps1 = gd._eps_from_out(out1, x_t, td)
        est = _dev(R.x0_estimate(x_t.cpu(), eps1.cpu(), t, gd._ptab.cpu(), clip=True))
    xin = torch.cat([x_t, est], dim=1)
    eps = unet(xin, td)
    if gd_kw:
        loss, d_eps = gd.loss_and_grad(eps, x, nz, td, want_grad=True, _pre=(2.0, -1.0))
    else:
        fhw = int(np.prod(SHAPE[2:]))
        acc = torch.zeros(1, dtype=F64, device=DEV)
        L.check(vdx_loss_sum(L.ptr(eps), L.ptr(nz), L.ptr(acc), 2, 1, fhw, 1, L.stream_ptr()))
        d_eps = torch.empty_like(eps)
        L.check(vdx_loss_grad(L.ptr(eps), L.ptr(nz), L.ptr(d_eps), 2, 1, fhw, 1, L.stream_ptr()))
        loss = (acc / float(batch.numel())).to(F32).reshape(())
    grads = torch.zeros_like(unet.flat_params)
    unet.backward(d_eps, grads)
    torch.cuda.synchronize()
    return loss, grads, xin


@pytest.mark.parametrize('self_cond', [True, False])
@pytest.mark.parametrize('objective', ['pred_noise', 'pred_v'])
def test_train_step_is_the_step_done_by_hand(tmp_path, self_cond, objective):
    gd_kw = dict(objective='pred_v') if objective == 'pred_v' else {}
    batch, t, noise = _train_inputs()
    tr = _trainer(tmp_path, _gd(loss_type='l2', **gd_kw))
    with launches() as rec:
        loss = tr.train_step(batch, step=0, t=t, noise=noise, self_cond=self_cond)
    torch.cuda.synchronize()
    names = [k for k, _ in rec]
    assert names.count('selfcond_x0_kernel') == int(self_cond) and names.count('lowres_pack_kernel') == 1, names
    assert names.count('v_to_eps_kernel') == int(self_cond and objective == 'pred_v'), names
    assert tr.last_self_cond is self_cond and tr.opt_count == 1
    hand_loss, hand_grads, xin = _hand_step(batch, t, noise, self_cond, **gd_kw)
    assert torch.equal(hand_loss, loss), (hand_loss.item(), loss.item())
    assert torch.equal(hand_grads, tr.grads), 'flat gradients differ from the step done by hand'
    assert hand_grads.abs().max() > 0 and np.isfinite(hand_loss.item())
    assert bool((xin[:, 1:] == 0).all()) != self_cond and (not self_cond or xin[:, 1:].abs().max() <= 1.0)
    # a ready estimate is the same step: the tensor pass 1 would have produced
    if self_cond:
        tr2 = _trainer(tmp_path / 'ready', _gd(loss_type='l2', **gd_kw))
        loss2 = tr2.train_step(batch, step=0, t=t, noise=noise, self_cond=xin[:, 1:].clone())
        torch.cuda.synchronize()
        assert torch.equal(loss2, loss) and torch.equal(tr2.grads, tr.grads)
    # the second half of the stem carries gradient exactly when the network saw an estimate
    off = {n: (o, s) for n, s, o in tr.unet.param_table}
    o, s = off['init_conv.kernel']
    gk = tr.grads[o:o + int(np.prod(s))].reshape(s)
    assert gk[..., 0, :].abs().max() > 0 and bool(gk[..., 1, :].abs().max() > 0) == self_cond


def test_the_draw_moves_no_other_stream(tmp_path):
    from video_diffusion_nnx_amd.train_step import self_cond_draw, self_cond_key, step_keys
    batch, _, _ = _train_inputs()
    coins = []
    for step in (4, 5):
        drawn = _trainer(tmp_path / f'd{step}', _gd())
        forced = _trainer(tmp_path / f'f{step}', _gd())
        forced.self_cond_prob = 0.0
        a = drawn.train_step(batch, step=step)
        b = forced.train_step(batch, step=step)
        torch.cuda.synchronize()
        gen = torch.Generator().manual_seed(self_cond_key(drawn.rng_seed, 0, step) & 0x7FFFFFFFFFFFFFFF)
        assert drawn.last_self_cond is self_cond_draw(0.5, gen) and forced.last_self_cond is False
        assert torch.equal(drawn.last_t, forced.last_t) and drawn.last_noise_key == forced.last_noise_key == step_keys(drawn.rng_seed, 0, step).noise
        assert np.isfinite(a.item()) and (torch.equal(a, b) != drawn.last_self_cond)
        coins.append(drawn.last_self_cond)
    assert True in coins and False in coins, coins                           # (steps chosen so that both outcomes occur: seed 0 draws False at 4, True at 5)


def test_accumulation_is_the_mean_of_the_two_hand_made_gradients(tmp_path):
    b0, t0, n0 = _train_inputs(0)
    b1, t1, n1 = _train_inputs(1)
    tr = _trainer(tmp_path, _gd(loss_type='l2'))
    tr.apply_grad_args, tr.gradient_accumulate_every = True, 2
    loss = tr.train_step_accum([b0, b1], step=0, ts=[t0, t1], noises=[n0, n1], self_conds=[True, False])
    torch.cuda.synchronize()
    l0, g0, _ = _hand_step(b0, t0, n0, True)
    l1, g1, _ = _hand_step(b1, t1, n1, False)
    assert tr.opt_count == 1 and tr.last_self_cond is False
    # tr.grads holds the sum of the micro-batch gradients (one fp32 addition per element); the mean is its exact half, folded into Adam's read
    assert torch.equal(tr.grads * 0.5, (g0 + g1) * 0.5), 'the accumulated gradient is not the mean of the two hand-made ones'
    assert torch.equal(loss, torch.stack([l0, l1]).mean())
