"""GPU tests of the mixed noise prior (vdx.h: "Mixed noise"; EXTENSION, parity unpinned: no reference code): the generator against the
restated stream tests/_mixnoise_ref.py and against the device's own vdx_randn tensors, the fused ancestral step against vdx_p_sample_step
on the generator's tensor and against fp64, the captured loop against its eager run, a step-by-step Python loop and the fp64 chain, and
the Python surface around them: alpha = 0 changes nothing, the deterministic chains change in x_T only, the train step in its noise only."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mixnoise_ref as M          # noqa: E402
import _step_cases as S          # noqa: E402
from _launch_hook import launches          # noqa: E402
from oracle import unet3d_ref as R          # noqa: E402

DEV = 'cuda:0'
OK = 0
F32, F64 = torch.float32, torch.float64
ALPHA = 1.0
# [B,C,F,H,W] and what each exercises
SHAPES = {
    'hw_odd': (2, 1, 4, 3, 3),                   # HW odd: quads straddle frames, the shared lane rotates
    'fhw_odd': (3, 4, 3, 3, 3),                  # fhw = 27 odd: quads straddle channels
    'aligned': (2, 3, 2, 4, 4),                  # HW % 4 == 0: one shared counter per quad
    'tails': (1, 3, 3, 1, 5),                    # 45 elements: the total is no multiple of 4
    'one_frame': (1, 1, 1, 4, 4),                # a single frame
    'wrap': (2, 4, 3, 1, 175001),                # per_sample 2 100 012: the second sweep of a 2048 x 256 x 4 grid
}
STEP_SHAPES = [k for k, sh in SHAPES.items() if (sh[1] * sh[2] * sh[3] * sh[4]) % 4 == 0]
SEED = 0x1234567890ABCDEF


def _L():
    from video_diffusion_nnx_amd import _lib as L
    return L


def _G():
    from video_diffusion_nnx_amd import gaussian_diffusion as G
    return G


def _weights(alpha=ALPHA):
    return _G().mixed_noise_coef(alpha)


def _nan(shape):
    return torch.full(tuple(shape), float('nan'), dtype=F32, device=DEV)


def _randn_mixed(shape, seed, draw, alpha=ALPHA, dev_draw=None):
    L = _L()
    B, C, Fr, H, W = shape
    a, b = _weights(alpha)
    out = _nan(shape)
    rc = L.vdx_randn_mixed(L.ptr(out), B, C, Fr, H * W, a, b, seed, draw, L.ptr(dev_draw), L.stream_ptr())
    assert rc == OK, L.vdx_last_error()
    torch.cuda.synchronize()
    return out


def _randn(n, seed, draw):
    L = _L()
    out = _nan((n,))
    L.check(_G().vdx_randn(L.ptr(out), n, seed, draw, 0, L.stream_ptr()))
    torch.cuda.synchronize()
    return out


def _bits(a, b, what):
    assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), f'{what}: the bits differ'


# ---- vdx_randn_mixed --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(SHAPES))
def test_randn_mixed(name):
    """Against the restated stream, element by element under
        a (ATOL + RTOL |s|) + b (ATOL + RTOL |e|) + 2^-23 (|a s| + |b e|)
    -- RANDN_ATOL / RANDN_RTOL of tests/_step_cases.py on either component, plus one fp32 rounding of each product and of the sum (the sum
    is at most |a s| + |b e|) -- and bit for bit against a * S + b * E formed in fp32 from the device's own vdx_randn tensors."""
    shape = SHAPES[name]
    B, C, Fr, H, W = shape
    draw = 3
    got = _randn_mixed(shape, SEED, draw)
    assert not torch.isnan(got).any(), 'elements were never written'
    a, b = _weights()
    s, e = M.components(shape, SEED, draw)
    ref = M.mixed_randn(shape, SEED, draw, ALPHA)
    s64, e64 = np.abs(s.astype(np.float64)), np.abs(e.astype(np.float64))
    bound = a * (S.RANDN_ATOL + S.RANDN_RTOL * s64) + b * (S.RANDN_ATOL + S.RANDN_RTOL * e64) + S.FP32_ULP * (a * s64 + b * e64)
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref.astype(np.float64))
    print(f'[randn_mixed {name}] max error {err.max():.3e}, worst error / bound {(err / bound).max():.4f}')
    assert (err <= bound).all(), (name, float((err / bound).max()))
    # the device's own components: S over [B,C,H,W] at draw VDX_DRAW_SHARED + d, E over the whole tensor at draw d
    Sd = _randn(B * C * H * W, SEED, _L().DRAW_SHARED + draw).reshape(B, C, 1, H, W)
    Ed = _randn(B * C * Fr * H * W, SEED, draw).reshape(shape)
    a32, b32 = torch.tensor(a, dtype=F32, device=DEV), torch.tensor(b, dtype=F32, device=DEV)
    _bits(got, a32 * Sd + b32 * Ed, f'randn_mixed {name} against a * S + b * E of vdx_randn')
    _bits(got, _randn_mixed(shape, SEED, draw), f'randn_mixed {name}, a second call')
    # frames of one clip share s: with alpha -> infinity (a = 1, b = 0) every frame is the shared tensor
    if name == 'hw_odd':
        same = _randn_mixed(shape, SEED, draw, alpha=1e30)
        assert torch.equal(same, Sd.expand(shape).contiguous())


def test_randn_mixed_dev_draw_adds_to_draw():
    shape = SHAPES['fhw_odd']
    two = torch.tensor([2], dtype=torch.int64, device=DEV)
    _bits(_randn_mixed(shape, 7, 1, dev_draw=two), _randn_mixed(shape, 7, 3), 'draw 1 + *dev_draw 2 against draw 3')
    assert not torch.equal(_randn_mixed(shape, 7, 1), _randn_mixed(shape, 7, 3))
    # alpha = 0 (a = 0, b = 1) is vdx_randn's tensor
    _bits(_randn_mixed(shape, 7, 3, alpha=0.0), _randn(int(np.prod(shape)), 7, 3).reshape(shape), 'alpha = 0 against vdx_randn')


# ---- vdx_p_sample_step_mixed --------------------------------------------------------------------------------------------------------------

T_P = S.T_P
LEVELS = (0, T_P // 2, T_P - 1)


@functools.lru_cache(None)
def _step_inputs(name):
    shape = SHAPES[name]
    B, C, Fr, H, W = shape
    g = torch.Generator().manual_seed(5)
    x = 2 * torch.randn(shape, generator=g)
    eps = torch.randn(B, Fr, H, W, C, generator=g)
    return x, eps


def _step(kind, shape, x, eps, t, tabs, thres, clip, *, noise=None, seed=SEED, offset=0, inplace=False):
    L, G = _L(), _G()
    B, C, Fr, H, W = shape
    per = C * Fr * H * W
    xd = x.clone()
    out = xd if inplace else _nan(shape)
    a, b = _weights()
    if kind == 'mixed':
        rc = L.vdx_p_sample_step_mixed(L.ptr(xd), L.ptr(eps), L.ptr(out), L.ptr(t), L.ptr(tabs), T_P, Fr, a, b, seed, offset, 0, L.ptr(thres),
                                       int(clip), B, C, per, L.stream_ptr())
    else:
        rc = G.vdx_p_sample_step(L.ptr(xd), L.ptr(eps), L.ptr(out), L.ptr(t), L.ptr(tabs), T_P, L.ptr(noise), seed, offset, 0, L.ptr(thres),
                                 int(clip), B, C, per, L.stream_ptr())
    assert rc == OK, L.vdx_last_error()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('name', STEP_SHAPES)
def test_p_sample_step_mixed(name):
    """T = 1000; every sample visits t = 0, mid and T - 1 (in as many calls as the batch needs), clip on (with a threshold vector) and
    off.  Bit for bit vdx_p_sample_step on vdx_randn_mixed's tensor; against the fp64 step with the restated z under P_TOL_PHILOX x
    max(1, |ref|max) per sample, the form in which tests/test_gpu_step_kernels.py holds the T = 1000 steps to that figure (sqrt_recip_ac[999]
    ~ 157: one sample at T - 1 with the clip off reaches hundreds)."""
    shape = SHAPES[name]
    B = shape[0]
    draw = 6
    x, eps = _step_inputs(name)
    xd, ed = x.to(DEV), eps.to(DEV)
    tabs = S.device_tables(T_P)['ptab'].to(DEV)
    z_dev = _randn_mixed(shape, SEED, draw)
    z_ref = torch.from_numpy(M.mixed_randn(shape, SEED, draw, ALPHA))
    zeros = torch.zeros(shape, device=DEV)
    for r in range(-(-3 // B)):
        t = torch.tensor([LEVELS[(i + r * B) % 3] for i in range(B)])
        td = t.to(DEV, torch.int32)
        for clip in (True, False):
            thres = torch.tensor([1.0, 1.7, 3.2][:B]) if clip else None
            thd = None if thres is None else thres.to(DEV)
            what = f'p_sample_mixed {name} t={t.tolist()} clip={int(clip)}'
            got = _step('mixed', shape, xd, ed, td, tabs, thd, clip, offset=draw)
            assert not torch.isnan(got).any(), what + ': elements were never written'
            _bits(got, _step('plain', shape, xd, ed, td, tabs, thd, clip, noise=z_dev), what + ' against vdx_p_sample_step on vdx_randn_mixed')
            ref64, _ = S.p_sample_ref(x, eps, z_ref, t, clip, thres, F64)
            S.check(got, ref64, S.scaled(S.P_TOL_PHILOX, ref64), what + ' against fp64')
            _bits(got, _step('mixed', shape, xd, ed, td, tabs, thd, clip, offset=draw, inplace=True), what + ', x and out one buffer')
            # t = 0 adds no noise: those samples are the posterior mean
            mean = _step('plain', shape, xd, ed, td, tabs, thd, clip, noise=zeros)
            for i in range(B):
                if int(t[i]) == 0:
                    _bits(got[i], mean[i], what + f', sample {i} at t = 0 is the posterior mean')
                else:
                    assert not torch.equal(got[i], mean[i])
    assert torch.equal(xd.cpu(), x) and torch.equal(ed.cpu(), eps)


# ---- the loop on the tiny rig of tests/test_gpu_sample_loops.py ---------------------------------------------------------------------------

KW = dict(dim=16, channels=1, dim_mults=(1, 2))
T, SHAPE, B = 6, (2, 1, 4, 8, 8), 2
LOOP_SEED = 2024


class Rig:
    """The network of tests/test_gpu_sample_loops.py with the oracle's random parameters, its handle, and the buffers of the loops (2B
    rows), owned here so that the allocator plays no part in what a graph key sees."""

    def __init__(self, guided):
        from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
        from video_diffusion_nnx_amd.unet3d import Unet3D
        L = self.L = _L()
        kw = dict(KW, **(dict(cond_dim=32) if guided else {}))
        self.guided = guided
        self.cfg = R.UnetConfig(**kw)
        self.params = R.random_params(self.cfg, seed=3, dtype=F64)
        self.unet = Unet3D(rngs=0, mode='f32', **kw)
        self.unet.load_state_dict({k: v.float() for k, v in self.params.items()})
        self.gd = GaussianDiffusion(self.unet, image_size=SHAPE[3], num_frames=SHAPE[2], channels=1, timesteps=T, frame_noise_alpha=ALPHA)
        self.h = self.unet.handle(SHAPE[2], SHAPE[3])
        self.unet.apply_activation_storage(self.h)
        self.rows = 2 * B if guided else B
        self.ws = self.unet.workspace(2 * B, SHAPE[2], SHAPE[3])
        self.st = torch.cuda.Stream(device=DEV)
        z = lambda *s, **k: torch.zeros(*s, device=DEV, **k)
        self.img, self.img_plain = z((2 * B,) + SHAPE[1:]), z((2 * B,) + SHAPE[1:])
        self.eps, self.t_dev, self.step_dev = z(2 * B, SHAPE[2], SHAPE[3], SHAPE[4], 1), z(2 * B, dtype=torch.int32), z(1, dtype=torch.int64)
        self.scratch = z(L.vdx_cfg_scratch_doubles(B), dtype=F64)
        self.cond = torch.randn(B, 32, generator=torch.Generator().manual_seed(9)).to(DEV) if guided else None
        self.x_T = self.gd.noise(SHAPE, LOOP_SEED, 0)
        torch.cuda.synchronize()

    def run(self, mixed, use_graph, nsteps=T):
        """One chain from x_T on the rig's stream: the mixed loop, or the plain / guided loop of the same handle.  Returns (x_0 rows, the
        launches recorded)."""
        L, gd = self.L, self.gd
        img = self.img if mixed else self.img_plain
        with torch.cuda.stream(self.st):
            img.zero_()
            img[:B].copy_(self.x_T)
            self.t_dev.fill_(T - 1)
            self.step_dev.zero_()
            head = (self.h.ptr, L.ptr(self.unet.flat_params), L.ptr(self.unet.packed()), L.ptr(img), L.ptr(self.eps), L.ptr(self.t_dev),
                    L.ptr(self.step_dev), L.ptr(gd._ptab), T, nsteps, L.ptr(self.cond), LOOP_SEED, 1, 0.0, 0)
            cfg = (2.0, 0.0, L.ptr(self.scratch)) if self.guided else (1.0, 0.0, 0)
            tail = (L.ptr(self.ws), self.ws.numel(), B, int(use_graph), self.st.cuda_stream)
            with launches() as rec:
                if mixed:
                    rc = L.vdx_p_sample_loop_mixed(*head, *cfg, *gd._mix, *tail)
                elif self.guided:
                    rc = L.vdx_p_sample_loop_guided(*head, *cfg, *tail)
                else:
                    rc = _G().vdx_p_sample_loop_dyn(*head, *tail)
            assert rc == OK, L.vdx_last_error()
            self.st.synchronize()
        return img[:B].clone(), rec

    def python_loop(self):
        """forward (+ the torch guidance combine) and vdx_p_sample_step_mixed, issued step by step."""
        L, gd = self.L, self.gd
        img = self.x_T.clone()
        for k, i in enumerate(reversed(range(T))):
            t = torch.full((B,), i, dtype=torch.int32, device=DEV)
            eps_hat = self.unet.forward_with_cond_scale(img, t, cond=self.cond, cond_scale=2.0) if self.guided else self.unet(img, t)
            L.check(L.vdx_p_sample_step_mixed(L.ptr(img), L.ptr(eps_hat), L.ptr(img), L.ptr(t), L.ptr(gd._ptab), T, SHAPE[2], *gd._mix, LOOP_SEED,
                                              1 + k, 0, 0, 1, B, 1, int(np.prod(SHAPE[1:])), L.stream_ptr()))
        torch.cuda.synchronize()
        return img

    def fp64_chain(self):
        cond = None if self.cond is None else self.cond.cpu().double()

        def denoise(x, t):
            if not self.guided:
                return R.unet_forward(self.params, self.cfg, x, t)
            c = R.unet_forward(self.params, self.cfg, x, t, cond=cond, cond_mask=torch.zeros(B, dtype=torch.bool))
            n = R.unet_forward(self.params, self.cfg, x, t, cond=cond, cond_mask=torch.ones(B, dtype=torch.bool))
            return n + (c - n) * 2.0
        z = lambda d: torch.from_numpy(M.mixed_randn(SHAPE, LOOP_SEED, d, ALPHA))
        return M.ancestral_chain64(denoise, z(0), [z(1 + k) for k in range(T)], image_size=SHAPE[3], num_frames=SHAPE[2], channels=1, timesteps=T)


def _names(rec):
    return [k for k, _ in rec]


def _forwards(rec):
    return sum(k.startswith('final_conv') for k in _names(rec))


@pytest.mark.parametrize('guided', [False, True], ids=['plain', 'guided'])
def test_mixed_loop(guided):
    r = Rig(guided)
    graph, rec = r.run(True, 1)
    names = _names(rec)
    assert _forwards(rec) == 2, rec                                        # the eager first step and the captured one
    assert names.count('p_sample_mixed_kernel') == 2 and 'p_sample_kernel' not in names and 'randn_mixed_kernel' not in names, names
    assert ('cfg_combine_kernel' in names) == guided and names[-1] == 'advance_kernel', names
    assert torch.isfinite(graph).all() and not torch.equal(graph, r.x_T)
    eager, rec = r.run(True, 0)
    assert _forwards(rec) == T and _names(rec).count('p_sample_mixed_kernel') == T and 'p_sample_kernel' not in _names(rec)
    _bits(graph, eager, 'captured against eager')
    _bits(graph, r.python_loop(), 'captured against the step-by-step Python loop')
    # a second call replays the cached graph; a plain (or guided) loop of the same handle in between keeps its own slot, and so does this one
    again, rec = r.run(True, 1)
    assert rec == [], rec
    _bits(graph, again, 'the replayed graph')
    plain, rec = r.run(False, 1)
    assert _forwards(rec) == 2 and 'p_sample_kernel' in _names(rec) and 'p_sample_mixed_kernel' not in _names(rec), rec
    assert not torch.equal(plain, graph)                                   # i.i.d. z from the same x_T: another chain
    again, rec = r.run(True, 1)
    assert rec == [], rec
    _bits(graph, again, 'the replayed graph after another loop')
    _, rec = r.run(False, 1)
    assert rec == [], rec
    # the fp64 chain with the restated mixed draws, under the bound of test_p_sample_loop_matches_oracle_loop
    exp = r.fp64_chain()
    err = ((graph.cpu().double() + 1.0) * 0.5 - exp).abs().max().item()
    print(f'[mixed loop guided={int(guided)}] max-abs error against the fp64 chain {err:.3e}  bound 2.000e-04')
    assert err < 2e-4
    # the Python surface runs this loop
    with launches() as rec:
        out = r.gd.p_sample_loop(SHAPE, LOOP_SEED, use_graph=False, **(dict(cond=r.cond, cond_scale=2.0) if guided else {}))
    torch.cuda.synchronize()
    assert _names(rec).count('randn_mixed_kernel') == 1 and _names(rec).count('p_sample_mixed_kernel') == T and 'p_sample_kernel' not in _names(rec)
    unnorm = torch.empty_like(graph)
    r.L.check(_G().vdx_affine(r.L.ptr(graph), r.L.ptr(unnorm), graph.numel(), 0.5, 0.5, r.L.stream_ptr()))     # unnormalize_img
    torch.cuda.synchronize()
    _bits(out, unnorm, 'p_sample_loop() against the loop entry')
    _bits(out, r.gd.sample(LOOP_SEED, batch_size=B, **(dict(cond=r.cond, cond_scale=2.0) if guided else {})), 'sample() against p_sample_loop()')


# ---- off means off --------------------------------------------------------------------------------------------------------------------------

def _pair(alpha_kw):
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.unet3d import Unet3D
    unet = Unet3D(rngs=0, mode='f32', **KW)
    mk = lambda **kw: GaussianDiffusion(unet, image_size=SHAPE[3], num_frames=SHAPE[2], channels=1, timesteps=T, **kw)
    return mk(**alpha_kw), mk()


NEW_KERNELS = {'randn_mixed_kernel', 'p_sample_mixed_kernel'}


def test_alpha_zero_changes_nothing():
    zero, absent = _pair(dict(frame_noise_alpha=0.0))
    x = torch.rand(SHAPE, generator=torch.Generator().manual_seed(1))
    t = torch.tensor([1, T - 1])
    with launches() as rec:
        outs = [(gd.sample(5, batch_size=B), gd.sample(5, batch_size=B, ddim_steps=3), gd.p_losses(x, t, 11), gd(x, 12),
                 gd.p_sample(x, t, 13), gd.q_sample(x, t, 14)) for gd in (zero, absent)]
    torch.cuda.synchronize()
    assert not NEW_KERNELS & set(_names(rec)), sorted(NEW_KERNELS & set(_names(rec)))
    for got, want, what in zip(outs[0], outs[1], ('sample', 'sample ddim', 'p_losses', '__call__', 'p_sample', 'q_sample')):
        _bits(got.reshape(-1), want.reshape(-1), f'alpha = 0 against no argument: {what}')
    _bits(zero.noise(SHAPE, 9, 2), absent.randn(SHAPE, 9, 2), 'noise() at alpha = 0 is randn()')


# ---- the surrounding paths ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kw', [dict(ddim_steps=3), dict(dpm_steps=3)], ids=['ddim', 'dpm'])
def test_deterministic_chains_change_in_x_T_only(kw):
    mixed, twin = _pair(dict(frame_noise_alpha=ALPHA))
    with launches() as rec:
        got = mixed.sample(21, batch_size=B, **kw)
    torch.cuda.synchronize()
    assert _names(rec).count('randn_mixed_kernel') == 1 and 'p_sample_mixed_kernel' not in _names(rec)
    x_T = mixed.noise(SHAPE, 21, 0)
    _bits(x_T, _randn_mixed(SHAPE, 21, 0), 'noise() is vdx_randn_mixed')
    _bits(got, twin.sample(21, batch_size=B, x_T=x_T, **kw), 'the mixed chain against the alpha = 0 twin from the mixed x_T')
    assert not torch.equal(got, twin.sample(21, batch_size=B, **kw))
    # q_sample, p_losses and the eager p_sample draw through noise() too
    x = torch.rand(SHAPE, generator=torch.Generator().manual_seed(2))
    t = torch.tensor([2, T - 1])
    _bits(mixed.q_sample(x, t, 31), twin.q_sample(x, t, noise=mixed.noise(SHAPE, 31, 0)), 'q_sample')
    nk = _G().split_key(41, 3)[1]
    _bits(mixed.p_losses(x, t, 41).reshape(1), twin.p_losses(x, t, noise=mixed.noise(SHAPE, nk, 0)).reshape(1), 'p_losses')
    _bits(mixed.p_sample(x, t, 51), twin.p_sample(x, t, None, noise=mixed.noise(SHAPE, 51, 0)), 'p_sample')
    assert not torch.equal(mixed.p_sample(x, t, 51), twin.p_sample(x, t, 51))


TRAIN_KW = dict(dim=16, dim_mults=(1, 2), channels=1)
TRAIN_SHAPE = (2, 1, 2, 16, 16)


def _trainer(path, alpha):
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.trainer import Trainer
    from video_diffusion_nnx_amd.unet3d import Unet3D
    unet = Unet3D(rngs=1, mode='f32', **TRAIN_KW)
    gd = GaussianDiffusion(unet, image_size=16, num_frames=2, channels=1, timesteps=8, loss_type='l2', frame_noise_alpha=alpha)
    return gd, Trainer(gd, str(path), dataset_path='synthetic:8', train_batch_size=2, train_num_steps=8, train_lr=1e-3, checkpoint_every_steps=100,
                       results_folder=str(path / 'res'), step_start_ema=0, update_ema_every=1, ema_decay=0.9)


def test_train_step_changes_in_its_noise_only(tmp_path):
    batch = torch.rand(*TRAIN_SHAPE, generator=torch.Generator().manual_seed(0))
    gd, tr = _trainer(tmp_path / 'a', ALPHA)
    with launches() as rec:
        loss = tr.train_step(batch, 0)
    torch.cuda.synchronize()
    assert _names(rec).count('randn_mixed_kernel') == 1
    grads = tr.grads.clone()
    noise = gd.noise(TRAIN_SHAPE, tr.last_noise_key, 0)
    _bits(noise, _randn_mixed(TRAIN_SHAPE, tr.last_noise_key & 0xFFFFFFFFFFFFFFFF, 0), 'the train step\'s noise is vdx_randn_mixed at draw 0')
    _, twin = _trainer(tmp_path / 'b', ALPHA)
    with launches() as rec:
        loss_twin = twin.train_step(batch, 0, noise=noise)
    torch.cuda.synchronize()
    assert not NEW_KERNELS & set(_names(rec))
    _bits(loss.reshape(1), loss_twin.reshape(1), 'loss: the step against the explicit-noise step')
    _bits(grads, twin.grads, 'gradients: the step against the explicit-noise step')
    assert grads.abs().max() > 0
    _, iid = _trainer(tmp_path / 'c', 0.0)
    with launches() as rec:
        loss_iid = iid.train_step(batch, 0)
    torch.cuda.synchronize()
    assert not NEW_KERNELS & set(_names(rec))
    assert iid.last_noise_key == tr.last_noise_key and torch.equal(iid.last_t.cpu(), tr.last_t.cpu())
    assert not torch.equal(iid.grads, grads) and loss_iid.item() != loss.item()
