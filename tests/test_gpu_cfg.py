"""GPU tests of classifier-free guidance end to end (EXTENSION, parity unpinned: the reference's p_sample_loop drops cond and its
training never drops the condition): the combine kernel against torch / fp64, the captured guided loops against the eager run of the
same step and against the step-by-step loop restated from Unet3D.forward_with_cond_scale, the guidance rescale against an fp64 run,
the conditional train step against fp64 autograd through the oracle, the Trainer switches and the CLI round trip."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import philox_ref, train_ref, unet3d_ref as R
from oracle.diffusion_ref import DiffusionRef

DEV = 'cuda:0'
INVALID = -1                                                             # VDX_ERR_INVALID
EPS24 = 2.0 ** -24

KW = dict(dim=16, channels=3, cond_dim=32)                               # the tiny conditioned network of test_gpu_backward.py
T, B, FRAMES, SIZE = 6, 3, 2, 8                                          # B odd: the halves of 2B are not power-of-two aligned
SHAPE = (B, 3, FRAMES, SIZE, SIZE)
PER = 3 * FRAMES * SIZE * SIZE                                           # 384
SEED = 13


def _rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# ---------------------------------------------------------------- vdx_cfg_combine ----------------------------------------------------------------

def _call(eps2_ptr, out_ptr, s, phi, scratch, batch, per):
    from video_diffusion_nnx_amd import _lib as L
    rc = L.vdx_cfg_combine(eps2_ptr, out_ptr, float(s), float(phi), L.ptr(scratch), batch, per, L.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _scratch(batch, fill=float('nan')):
    from video_diffusion_nnx_amd import _lib as L
    return torch.full((L.vdx_cfg_scratch_doubles(batch),), fill, dtype=torch.float64, device=DEV)


@functools.lru_cache(None)
def _eps2(per):
    """[2 * 3][per]: sample 0 = unit normals, sample 1 = mean 3 / std 0.1 (the sums cancel to 1e-3 of their size), sample 2 = a constant
    (c == n == 0.5, so every sum is exact and std(g) is exactly 0).  Left unchanged by every test."""
    g = torch.Generator().manual_seed(per)
    c, n = torch.randn(3, per, generator=g), torch.randn(3, per, generator=g)
    c[1], n[1] = 3 + 0.1 * c[1], 3 + 0.1 * n[1]
    c[2], n[2] = 0.5, 0.5
    return torch.cat([c, n]).to(DEV)


@pytest.mark.parametrize('per', [4, 384, 65536])
@pytest.mark.parametrize('s', [0.0, 1.0, 2.0, 7.5])
def test_cfg_combine_is_the_torch_expression_bit_for_bit(per, s):
    eps2 = _eps2(per)
    c, n = eps2[:3], eps2[3:]
    exp = n + (c - n) * s                                                 # Unet3D.forward_with_cond_scale's expression
    out = torch.full((3, per), float('nan'), device=DEV)
    assert _call(eps2.data_ptr(), out.data_ptr(), s, 0.0, None, 3, per) == 0
    assert torch.equal(out, exp)
    work = eps2.clone()                                                   # in place: the first half is overwritten, the second untouched
    assert _call(work.data_ptr(), work.data_ptr(), s, 0.0, None, 3, per) == 0
    assert torch.equal(work[:3], exp) and torch.equal(work[3:], n)


def test_cfg_combine_rejects_odd_sizes_and_misaligned_pointers():
    buf = torch.zeros(2 * 3 * 8 + 4, device=DEV)
    out = torch.zeros(3 * 8 + 4, device=DEV)
    sc = _scratch(3)
    assert _call(buf.data_ptr(), out.data_ptr(), 2.0, 0.0, None, 3, 8) == 0
    assert _call(buf.data_ptr(), out.data_ptr(), 2.0, 0.0, None, 3, 6) == INVALID            # per_sample % 4
    assert _call(buf.data_ptr() + 4, out.data_ptr(), 2.0, 0.0, None, 3, 8) == INVALID        # eps2 off by one float
    assert _call(buf.data_ptr(), out.data_ptr() + 4, 2.0, 0.0, None, 3, 8) == INVALID        # out off by one float
    assert _call(buf.data_ptr(), out.data_ptr(), 2.0, 0.7, None, 3, 8) == INVALID            # the rescale needs its scratch
    assert _call(buf.data_ptr(), out.data_ptr(), 2.0, 1.5, sc, 3, 8) == INVALID              # rescale outside [0, 1]
    assert _call(buf.data_ptr(), out.data_ptr(), 2.0, -0.5, sc, 3, 8) == INVALID
    assert _call(0, out.data_ptr(), 2.0, 0.0, None, 3, 8) == INVALID
    assert _call(buf.data_ptr(), out.data_ptr(), 2.0, 0.0, None, 0, 8) == INVALID


def _rescaled_fp64(c, n, s, phi):
    """g in torch fp32 (the kernel's bits, by the test above), the four sums in numpy fp64, the factor in fp64; returns (g, g * factor)."""
    g = (n + (c - n) * s).cpu().numpy().astype(np.float64)
    c64 = c.cpu().numpy().astype(np.float64)
    per = c64.shape[1]
    phi64 = float(np.float32(phi))                                       # the ABI takes the rescale as a float
    ss_c = (c64 * c64).sum(1) - c64.sum(1) ** 2 / per
    ss_g = (g * g).sum(1) - g.sum(1) ** 2 / per
    factor = np.ones(len(g))
    ok = ss_g > 0
    factor[ok] = phi64 * np.sqrt(np.maximum(ss_c[ok], 0) / ss_g[ok]) + (1.0 - phi64)
    return g, g * factor[:, None], factor


@pytest.mark.parametrize('per', [4, 384, 65536])
@pytest.mark.parametrize('phi', [0.7, 1.0])
def test_cfg_combine_rescale(per, phi):
    eps2 = _eps2(per)
    c, n = eps2[:3], eps2[3:]
    s = 7.5
    g, exp, factor = _rescaled_fp64(c, n, s, phi)
    out = torch.full((3, per), float('nan'), device=DEV)
    assert _call(eps2.data_ptr(), out.data_ptr(), s, phi, _scratch(3), 3, per) == 0
    got = out.cpu().numpy().astype(np.float64)
    # one rounding of the factor to float, one of the product; the double sums differ from numpy's by the order of summation only
    err = np.abs(got - exp)
    worst = (err / np.maximum(np.abs(exp), 1e-300)).max()
    print(f'cfg rescale per={per} phi={phi}: factors {factor}, worst relative error {worst / EPS24:.3f} x 2^-24 (bound 3)')
    assert (err <= 3 * EPS24 * np.abs(exp)).all(), worst / EPS24
    assert factor[2] == 1.0 and np.array_equal(got[2], g[2])             # the constant sample: factor exactly 1, out == g
    assert abs(factor[0] - 1.0) > 1e-3 or per == 4                        # and the rescale does something to the others
    # the bits are the same call to call (another scratch content), and in place
    again = torch.empty_like(out)
    assert _call(eps2.data_ptr(), again.data_ptr(), s, phi, _scratch(3, 0.0), 3, per) == 0
    assert torch.equal(again, out)
    work = eps2.clone()
    assert _call(work.data_ptr(), work.data_ptr(), s, phi, _scratch(3), 3, per) == 0
    assert torch.equal(work[:3], out) and torch.equal(work[3:], n)
    # the statistics do not leak across samples: sample k alone gives its bits of the batched call
    for k in range(3):
        one = torch.cat([c[k:k + 1], n[k:k + 1]]).contiguous()
        alone = torch.empty(1, per, device=DEV)
        assert _call(one.data_ptr(), alone.data_ptr(), s, phi, _scratch(1), 1, per) == 0
        assert torch.equal(alone[0], out[k]), k


# ---------------------------------------------------------------- the guided loops ----------------------------------------------------------------

@functools.lru_cache(None)
def _params():
    cfg = R.UnetConfig(**KW)
    return cfg, R.random_params(cfg, seed=3, dtype=torch.float64)


@functools.lru_cache(None)
def _cond():
    return torch.randn(B, 32, generator=torch.Generator().manual_seed(9))


def _gd(mode='f32', **gkw):
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.unet3d import Unet3D
    unet = Unet3D(rngs=0, mode=mode, **KW)
    unet.load_state_dict({k: v.float() for k, v in _params()[1].items()})
    return GaussianDiffusion(unet, image_size=SIZE, num_frames=FRAMES, channels=3, timesteps=T, **gkw)


SAMPLERS = {'ddpm': {}, 'ddim': dict(ddim_steps=4), 'dpm': dict(dpm_steps=4, dpm_order=2)}


def _guided_eps(unet, img, t, cond, s, phi):
    """forward_with_cond_scale's eps; with phi > 0 its 2B forward restated (the same three torch.cat and mask) and the combine done as
    in test_cfg_combine_rescale: g in torch fp32, the four sums and the factor in numpy fp64, g * factor in fp64, rounded once to fp32 for
    the step kernel."""
    if not phi:
        return unet.forward_with_cond_scale(img, t, cond=cond, cond_scale=s)
    mask = torch.zeros(2 * B, dtype=torch.bool, device=DEV)
    mask[B:] = True
    both = unet(torch.cat((img, img), 0), torch.cat((t, t), 0), torch.cat((cond, cond), 0), cond_mask=mask)
    _, exp, _ = _rescaled_fp64(both[:B].reshape(B, -1), both[B:].reshape(B, -1), s, phi)
    return torch.from_numpy(exp.astype(np.float32)).reshape(both[:B].shape).to(DEV)


def _restated(gd, kind, cond, s, phi=0.0):
    """The step-by-step guided loop as it stood before the captured one: forward_with_cond_scale (three torch.cat, one 2B forward, the
    torch combine), the dynamic threshold and vdx_p_sample_step / vdx_ddim_step / vdx_dpm_step, issued from Python.  phi > 0: the same
    loop with the combine of _guided_eps."""
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd import gaussian_diffusion as G
    unet = gd.denoise_fn
    keep = unet.act_bf16
    unet.act_bf16 = bool(gd.sample_act_bf16 and unet.mode == 'bf16')
    try:
        img = gd.randn(SHAPE, SEED, 0)
        per = PER
        if kind == 'ddpm':
            for k, i in enumerate(reversed(range(T))):
                t = torch.full((B,), i, dtype=torch.int32, device=DEV)
                eps_hat = _guided_eps(unet, img, t, cond, s, phi)
                thres = gd._dynamic_threshold(img, t, eps_hat) if gd.use_dynamic_thres else None
                L.check(G.vdx_p_sample_step(L.ptr(img), L.ptr(eps_hat), L.ptr(img), L.ptr(t), L.ptr(gd._ptab), T, 0, SEED, 1 + k, 0,
                                            L.ptr(thres), 1, B, 3, per, L.stream_ptr()))
        else:
            steps = 4
            seq_host = G.ddim_time_sequence(T, steps)
            seq = torch.from_numpy(seq_host).to(DEV)
            hist = torch.empty_like(img)
            step_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
            for k in range(steps):
                t = torch.full((B,), int(seq_host[k]), dtype=torch.int32, device=DEV)
                eps_hat = _guided_eps(unet, img, t, cond, s, phi)
                step_dev.fill_(k)
                thres = gd._dynamic_threshold(img, t, eps_hat) if gd.use_dynamic_thres else None
                if kind == 'ddim':
                    L.check(G.vdx_ddim_step(L.ptr(img), L.ptr(eps_hat), L.ptr(img), L.ptr(gd.alphas_cumprod), L.ptr(seq), L.ptr(step_dev),
                                            L.ptr(thres), 1, B, 3, per, L.stream_ptr()))
                else:
                    L.check(G.vdx_dpm_step(L.ptr(img), L.ptr(eps_hat), L.ptr(img), L.ptr(hist), L.ptr(gd.alphas_cumprod), L.ptr(seq),
                                           L.ptr(step_dev), L.ptr(thres), 1, 2, B, 3, per, L.stream_ptr()))
        out = torch.empty_like(img)
        L.check(G.vdx_affine(L.ptr(img), L.ptr(out), img.numel(), 0.5, 0.5, L.stream_ptr()))
        torch.cuda.synchronize()
    finally:
        unet.act_bf16 = keep
    return out


@pytest.mark.parametrize('dyn', [False, True], ids=['clip', 'dynthres'])
@pytest.mark.parametrize('mode', ['f32', 'bf16'])
@pytest.mark.parametrize('kind', ['ddpm', 'ddim', 'dpm'])
def test_captured_guided_loop_is_the_eager_loop(kind, mode, dyn):
    gd = _gd(mode, use_dynamic_thres=dyn)
    cond = _cond().to(DEV)
    kw = SAMPLERS[kind]
    graph = gd.sample(SEED, cond=cond, cond_scale=2.0, use_graph=True, **kw)
    eager = gd.sample(SEED, cond=cond, cond_scale=2.0, use_graph=False, **kw)
    torch.cuda.synchronize()
    assert tuple(graph.shape) == SHAPE and torch.isfinite(graph).all()
    assert torch.equal(graph, eager)
    assert torch.equal(graph, _restated(gd, kind, cond, 2.0))
    assert torch.equal(gd.sample(SEED, cond=cond, cond_scale=2.0, use_graph=True, **kw), graph)       # the graph again
    other_scale = gd.sample(SEED, cond=cond, cond_scale=3.0, use_graph=True, **kw)
    rescaled = gd.sample(SEED, cond=cond, cond_scale=2.0, guidance_rescale=0.7, use_graph=True, **kw)
    rescaled_eager = gd.sample(SEED, cond=cond, cond_scale=2.0, guidance_rescale=0.7, use_graph=False, **kw)
    torch.cuda.synchronize()
    assert not torch.equal(other_scale, graph) and not torch.equal(rescaled, graph)                  # the graph key sees both
    assert torch.equal(other_scale, _restated(gd, kind, cond, 3.0))
    assert torch.equal(rescaled, rescaled_eager)
    assert torch.equal(gd.sample(SEED, cond=cond, cond_scale=2.0, use_graph=True, **kw), graph)       # and back


def _fp64_loop(s, phi):
    """The ancestral guided chain in fp64 with the oracle UNet: both forwards, g = n + (c - n) s, and for phi > 0 the per-sample factor
    phi std(c) / std(g) + 1 - phi from fp64 standard deviations."""
    cfg, p = _params()
    cond = _cond().double()

    def denoise(x, t):
        c = R.unet_forward(p, cfg, x, t, cond=cond, cond_mask=torch.zeros(B, dtype=torch.bool))
        n = R.unet_forward(p, cfg, x, t, cond=cond, cond_mask=torch.ones(B, dtype=torch.bool))
        g = n + (c - n) * s
        if phi:
            f = phi * c.reshape(B, -1).std(1) / g.reshape(B, -1).std(1) + 1 - phi
            g = g * f.reshape(B, 1, 1, 1, 1)
        return g

    ref = DiffusionRef(denoise, image_size=SIZE, num_frames=FRAMES, channels=3, timesteps=T, dtype=torch.float64)
    n = int(np.prod(SHAPE))
    z = lambda d: torch.from_numpy(philox_ref.randn(n, SEED, d)).double().reshape(SHAPE)
    with torch.no_grad():
        return ref.p_sample_loop(z(0), [z(1 + k) for k in range(T)])


def test_guidance_rescale_loop_against_fp64():
    """The guidance_rescale = 0.7 loop against the restated step-by-step loop (the 2B forward of forward_with_cond_scale and
    vdx_p_sample_step, as in the test above) with the combine done in fp64 as in test_cfg_combine_rescale.  The bound is measured, not
    fixed: d0 = the distance of the phi = 0 captured loop (bit-equal to the restated loop, the test above) from an fp64 run of the same 6
    steps with the oracle UNet; the phi = 0.7 loop must stay within 4 x d0 of its restated loop (the headroom the f16 tests give over
    their emulation).  Both loops see the same fp32 forward, so this bounds what the statistics and the two roundings of the combine do
    to the chain.

    Printed, not asserted: the distance of the phi = 0.7 loop from a full fp64 run with the oracle UNet.  On an MI355X it is 1.236e-04
    where d0 is 1.098e-05: this chain amplifies the forward's fp32 error more with the rescale on.  At the first step (t = 5 of T = 6)
    sqrt_recipm1_alphas_cumprod is 389; with phi = 0 the static clip catches every element of x0_hat there and erases the error of eps,
    with phi = 0.7 eps is smaller and 0.1 % of the elements stay in the linear region.  On the CPU, no HIP code involved, the oracle UNet
    evaluated in fp32 is 1.04e-05 (phi = 0) and 2.15e-04 (phi = 0.7) from the fp64 chain."""
    gd = _gd('f32')
    cond = _cond().to(DEV)
    phi = float(np.float32(0.7))
    plain = gd.p_sample_loop(SHAPE, SEED, cond=cond, cond_scale=2.0)
    resc = gd.p_sample_loop(SHAPE, SEED, cond=cond, cond_scale=2.0, guidance_rescale=0.7)
    restated = _restated(gd, 'ddpm', cond, 2.0, phi)
    ref0, ref7 = _fp64_loop(2.0, 0.0), _fp64_loop(2.0, phi)
    d0 = (plain.cpu().double() - ref0).abs().max().item()
    d7 = (resc - restated).abs().max().item()
    d7_fp64 = (resc.cpu().double() - ref7).abs().max().item()
    moved = (restated - plain).abs().max().item()
    print(f'guided ancestral loop, T = {T}, cond_scale 2: phi = 0 from the fp64 run: {d0:.3e}; phi = 0.7 from the restated loop with the fp64 '
          f'combine: {d7:.3e} (bound 4 x {d0:.3e}); phi = 0.7 from the full fp64 run: {d7_fp64:.3e}; the rescale moves the result by {moved:.3e}')
    assert 0 < d0 < 5e-4                                                  # test_inpaint_guided's bound on the same kind of chain
    assert moved > 100 * d0                                               # a loop that ignored the rescale could not pass
    assert d7 <= 4 * d0, (d7, d0)


# ---------------------------------------------------------------- conditional training ----------------------------------------------------------------

TRAIN_SHAPE = (2, 3, 4, 16, 16)


def _trainer(tmp_path, ukw, frames, size, mode='f32', loss='l2', steps=3, **kw):
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.trainer import Trainer
    from video_diffusion_nnx_amd.unet3d import Unet3D
    unet = Unet3D(rngs=1, mode=mode, **ukw)
    gd = GaussianDiffusion(unet, image_size=size, num_frames=frames, channels=ukw['channels'], timesteps=50, loss_type=loss)
    tr = Trainer(gd, str(tmp_path), dataset_path='synthetic:8', train_batch_size=2, train_num_steps=steps, train_lr=1e-3,
                 checkpoint_every_steps=1000, results_folder=str(tmp_path / 'res'), step_start_ema=0, update_ema_every=1, ema_decay=0.9, **kw)
    return unet, gd, tr


def _oracle_grads(p0, batch, t, noise, cond, mask):
    cfg = R.UnetConfig(**KW)

    def loss_fn(params):
        ref = DiffusionRef(lambda a, b: R.unet_forward(params, cfg, a, b, cond=cond.double(), cond_mask=mask), image_size=16, num_frames=4,
                           channels=3, timesteps=50, loss_type='l2', dtype=torch.float64)
        return ref.loss(batch.double(), t, noise)

    return train_ref.loss_and_grads(p0, loss_fn)


def test_conditional_train_step_matches_oracle(tmp_path):
    """Loss and every gradient of one conditioned train step, cond_mask = [1, 0] (sample 0 on the null embedding), against fp64 autograd
    through the oracle; test_gpu_backward.py's f32 bounds.  With cond_mask = [0, 0] nothing reaches null_cond_emb: exactly zero."""
    unet, gd, tr = _trainer(tmp_path, KW, 4, 16)
    p0 = {k: v.detach().cpu().double().clone() for k, v in unet.state_dict().items()}
    g = torch.Generator().manual_seed(0)
    batch = torch.rand(TRAIN_SHAPE, generator=g)
    cond = torch.randn(2, 32, generator=g)
    mask = torch.tensor([1, 0], dtype=torch.uint8)
    loss_dev = tr.train_step(batch, step=0, cond=cond, cond_mask=mask)
    torch.cuda.synchronize()
    assert torch.equal(torch.as_tensor(tr.last_cond_mask), mask)
    t = tr.last_t.cpu().long()
    noise = torch.from_numpy(philox_ref.randn(batch.numel(), tr.last_noise_key, 0)).double().reshape(batch.shape)
    ref_loss, grads = _oracle_grads(p0, batch, t, noise, cond, mask.bool())
    assert abs(loss_dev.item() - ref_loss.item()) < 2e-5 * max(1.0, abs(ref_loss.item()))
    tol = 2e-4
    table = unet.param_table
    total_ref = torch.cat([grads[n].reshape(-1) for n, _, _ in table])
    total_got = torch.cat([tr.grads[o:o + int(np.prod(s))].cpu().double() for _, s, o in table])
    scale = total_ref.norm().item()
    got = {n: tr.grads[o:o + int(np.prod(s))].cpu().double().reshape(s) for n, s, o in table}
    rows = [(n, _rel(got[n], grads[n]), grads[n].norm().item(), got[n].norm().item()) for n, _, _ in table]
    bad = [(n, r) for n, r, nr, ng in rows if nr > 1e-6 * scale and r > tol * 5]
    dead = [(n, ng) for n, r, nr, ng in rows if nr <= 1e-6 * scale and ng > 1e-4 * scale]
    exact = [(n, ng) for n, r, nr, ng in rows if ('.fn.norm.' in n or n.startswith('time_rel_pos_bias')) and ng != 0.0]
    rel = _rel(total_got, total_ref)
    # the condition's own paths: null_cond_emb, and the rows of the time-MLP consumers that multiply the cond part of the embedding
    time_dim = 4 * KW['dim']
    cond_rows = [(n, _rel(got[n][time_dim:], grads[n][time_dim:]), grads[n][time_dim:].norm().item()) for n, s, _ in table
                 if n.endswith('.mlp.layers.1.kernel') and s[0] == time_dim + 32]
    null_rel = _rel(got['null_cond_emb'], grads['null_cond_emb'])
    print(f'conditional train step: loss {loss_dev.item():.7f} vs {ref_loss.item():.7f}; grads rel-L2 {rel:.3e} (bound {tol:.0e}); '
          f'null_cond_emb {null_rel:.3e}; worst cond rows {max(r for _, r, _ in cond_rows):.3e} over {len(cond_rows)} tensors')
    assert len(cond_rows) == 18 and all(nr > 1e-6 * scale for _, _, nr in cond_rows)
    assert grads['null_cond_emb'].norm().item() > 1e-6 * scale
    assert not exact and not dead, (exact[:5], dead[:5])
    assert not bad, sorted(bad, key=lambda z: -z[1])[:6]
    assert all(r <= tol * 5 for _, r, _ in cond_rows), sorted(cond_rows, key=lambda z: -z[1])[:4]
    assert null_rel <= tol * 5, null_rel
    assert rel < tol, rel
    # the unconditioned half of the picture: with another mask the gradient is another one, and nobody on the null embedding leaves it exactly 0
    _, _, tr2 = _trainer(tmp_path / 'b', KW, 4, 16)
    tr2.train_step(batch, step=0, cond=cond, cond_mask=torch.tensor([0, 0], dtype=torch.uint8))
    torch.cuda.synchronize()
    shape, off = tr2.unet._index['null_cond_emb']
    assert int((tr2.grads[off:off + 32] != 0).sum()) == 0
    assert _rel(tr2.grads.cpu().double(), tr.grads.cpu().double()) > 1e-2


UKW = dict(dim=16, channels=1, dim_mults=(1, 2), cond_dim=32)
TR_SHAPE = (2, 1, 4, 8, 8)


@pytest.fixture()
def cond_file(tmp_path):
    path = tmp_path / 'cond.npy'
    np.save(path, np.random.default_rng(5).standard_normal((8, 32)).astype(np.float32))
    return str(path)


def _cond_run(tmp_path, monkeypatch, cond_file, prob, mode='f32'):
    from video_diffusion_nnx_amd.trainer import Trainer
    from video_diffusion_nnx_amd.train_step import cond_drop_key, cond_drop_mask
    monkeypatch.setattr(Trainer, 'cond_path', cond_file)
    unet, gd, tr = _trainer(tmp_path, UKW, 4, 8, mode=mode)
    tr.null_cond_prob = prob                                             # on the instance: the class default stays 0 for every other test
    conds = np.load(cond_file)
    losses, masks, ts, nkeys = [], [], [], []
    for step in range(3):
        videos, cs = next(tr.dl)                                          # the dataset yields (video, cond_row) pairs
        assert all((conds == c.numpy()).all(1).any() for c in cs)
        losses.append(tr.train_step(videos, step=step, cond=cs).item())
        masks.append(None if tr.last_cond_mask is None else tr.last_cond_mask.clone())
        ts.append(tr.last_t.cpu().clone())
        nkeys.append(tr.last_noise_key)
        if prob > 0:
            gen = torch.Generator().manual_seed(cond_drop_key(tr.rng_seed, tr.rank, step, 0) & 0x7FFFFFFFFFFFFFFF)
            assert torch.equal(masks[-1], cond_drop_mask(2, prob, gen))
    torch.cuda.synchronize()
    assert all(np.isfinite(losses))
    return losses, masks, ts, nkeys, unet.flat_params.clone(), tr.ema.clone(), tr.m.clone(), tr.v.clone()


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_cond_dropout_steps_are_bit_reproducible_and_draw_the_documented_mask(tmp_path, monkeypatch, cond_file, mode):
    a = _cond_run(tmp_path / 'a', monkeypatch, cond_file, 0.5, mode)
    b = _cond_run(tmp_path / 'b', monkeypatch, cond_file, 0.5, mode)
    assert a[0] == b[0], (a[0], b[0])
    for x, y in zip(a[4:], b[4:]):
        assert torch.equal(x, y)
    drawn = torch.stack(a[1])
    assert 0 < int(drawn.sum()) < drawn.numel()                           # both outcomes occur in the six draws
    off = _cond_run(tmp_path / 'c', monkeypatch, cond_file, 0.0, mode)    # the dropout moves neither t nor the noise
    assert off[1] == [None] * 3
    assert all(torch.equal(x, y) for x, y in zip(a[2], off[2])) and a[3] == off[3]
    assert a[0] != off[0]                                                 # but it changes what is trained


def test_null_cond_prob_is_inert_without_a_condition(tmp_path):
    ends = []
    for touched in (True, False):
        unet, gd, tr = _trainer(tmp_path / f't{int(touched)}', dict(dim=16, channels=1, dim_mults=(1, 2)), 4, 8, mode='bf16')
        if touched:
            tr.null_cond_prob = 0.9
        g = torch.Generator().manual_seed(5)
        losses = [tr.train_step(torch.rand(TR_SHAPE, generator=g), step=step).item() for step in range(2)]
        torch.cuda.synchronize()
        assert tr.last_cond_mask is None
        ends.append((losses, unet.flat_params.clone(), tr.ema.clone()))
    assert ends[0][0] == ends[1][0]
    assert torch.equal(ends[0][1], ends[1][1]) and torch.equal(ends[0][2], ends[1][2])


def test_cond_accumulation_is_the_mean_of_the_single_gradients(tmp_path):
    g = torch.Generator().manual_seed(11)
    x = torch.rand(4, 1, 4, 8, 8, generator=g)
    t = torch.randint(0, 50, (4,), generator=g)
    noise = torch.randn(4, 1, 4, 8, 8, generator=g)
    cond = torch.randn(4, 32, generator=g)
    masks = [torch.tensor([1, 0], dtype=torch.uint8), torch.tensor([0, 0], dtype=torch.uint8)]
    _, _, A = _trainer(tmp_path / 'a', UKW, 4, 8, gradient_accumulate_every=2)
    A.apply_grad_args = True
    la = A.train_step_accum([x[:2], x[2:]], 0, ts=[t[:2], t[2:]], noises=[noise[:2], noise[2:]], conds=[cond[:2], cond[2:]], cond_masks=masks)
    singles, losses = [], []
    for j in range(2):
        _, _, S = _trainer(tmp_path / f's{j}', UKW, 4, 8)
        sl = slice(2 * j, 2 * j + 2)
        losses.append(S.train_step(x[sl], 0, t=t[sl], noise=noise[sl], cond=cond[sl], cond_mask=masks[j]).item())
        singles.append(S.grads.clone())
    torch.cuda.synchronize()
    rel = _rel(A.grads / 2, (singles[0] + singles[1]) / 2)
    print(f'[cond accum K=2 vs the two single steps] grads rel-L2 {rel:.3e}  loss {la.item():.7f} vs {np.mean(losses):.7f}')
    assert rel <= 2e-5, rel                                              # test_accumulation_equals_large_batch's comparison
    assert abs(la.item() - np.mean(losses)) <= 1e-5 * abs(np.mean(losses))
    assert _rel(singles[0], singles[1]) > 0.1


# ---------------------------------------------------------------- CLI ----------------------------------------------------------------

def test_cli_train_with_cond_then_guided_sample(tmp_path, monkeypatch):
    import json
    import yaml
    import sample
    import train
    from video_diffusion_nnx_amd import media
    from video_diffusion_nnx_amd.trainer import Trainer
    monkeypatch.setattr(Trainer, 'cond_path', None)                       # train.py sets the class attributes: undone after the test
    monkeypatch.setattr(Trainer, 'null_cond_prob', 0.0)
    cfg = {
        'rng_seed': 3,
        'unet': dict(dim=16, dim_mults=[1, 2], channels=1, rngs_seed=0, use_bert_text_cond=True),
        'diffusion': dict(image_size=16, num_frames=4, channels=1, timesteps=6, loss_type='l2'),
        'trainer': dict(folder=str(tmp_path / 'res'), dataset_path='synthetic:8', num_frames=4, train_batch_size=2, train_lr=1e-3,
                        train_num_steps=3, step_start_ema=1, update_ema_every=1, checkpoint_every_steps=2, results_folder=str(tmp_path / 'res'),
                        checkpoint_dir_path=str(tmp_path / 'ckpt'), tensorboard_dir=str(tmp_path / 'tb')),
    }
    cfg_path = tmp_path / 'cfg.yaml'
    cfg_path.write_text(yaml.safe_dump(cfg))
    rng = np.random.default_rng(1)
    np.save(tmp_path / 'train_cond.npy', rng.standard_normal((8, 768)).astype(np.float32))
    np.save(tmp_path / 'sample_cond.npy', rng.standard_normal((2, 768)).astype(np.float32))
    train.main(['--config', str(cfg_path), '--mode', 'f32', '--cond_path', str(tmp_path / 'train_cond.npy'), '--null_cond_prob', '0.5'])
    assert Trainer.cond_path == str(tmp_path / 'train_cond.npy') and Trainer.null_cond_prob == 0.5
    scalars = [json.loads(l) for l in (tmp_path / 'tb' / 'scalars_rank0.jsonl').read_text().splitlines()]
    losses = [s['value'] for s in scalars if s['tag'] == 'loss/train']
    assert len(losses) == 3 and all(0 < v < 10 for v in losses)
    seen = []
    to_uint8 = media.videos_to_uint8
    monkeypatch.setattr(media, 'videos_to_uint8', lambda v, **kw: seen.append(np.asarray(v)) or to_uint8(v, **kw))
    out = tmp_path / 'gifs'
    sample.main(['--config', str(cfg_path), '--checkpoint-path', str(tmp_path / 'ckpt'), '--step', '2', '--seed', '1', '--output-path', str(out),
                 '--mode', 'f32', '--cond-path', str(tmp_path / 'sample_cond.npy'), '--dpm-steps', '4', '--guidance-rescale', '0.7'])
    assert len(seen) == 1 and seen[0].shape == (2, 1, 4, 16, 16) and np.isfinite(seen[0]).all()
    assert seen[0].min() >= 0.0 and seen[0].max() <= 1.0 and seen[0].std() > 0
    gifs = sorted(out.glob('sample_*.gif'))
    assert len(gifs) == 2 and all(g.stat().st_size > 100 for g in gifs)
