"""GPU tests of frame-conditioned training and clean-context sampling (EXTENSION: RaMViD, Hoeppe et al. 2022): the three masked
kernels against their contracts in include/vdx.h, p_losses and one train step against the fp64 restatement of tests/_framecond_ref.py
with the oracle UNet, the Trainer's mask draw / reproducibility / accumulation / off switch, a short masked training run, the three
clean-context chains against their restated chains, and train -> extend."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _framecond_ref as FR
from _framecond_ref import R
from oracle import philox_ref, train_ref
from oracle.diffusion_ref import DiffusionRef

DEV = 'cuda:0'
INVALID = -1                                                             # VDX_ERR_INVALID


def _rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# ---------------------------------------------------------------- kernels ----------------------------------------------------------------
# channels = 3 (the channel-last gather of eps_hat does something), 2 frames of 8 x 8, element mask with p = 0.4, t = 0, mid, T-1

K_T, K_B, K_C, K_SHAPE = 10, 3, 3, (3, 3, 2, 8, 8)
K_FHW = 2 * 8 * 8


@functools.lru_cache(None)
def _kin():
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.unet3d import Unet3D
    gd = GaussianDiffusion(Unet3D(rngs=0, mode='f32', dim=16, channels=K_C), image_size=8, num_frames=2, channels=K_C, timesteps=K_T)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(K_SHAPE, generator=g)
    noise = torch.randn(K_SHAPE, generator=g)
    eps = torch.randn(K_B, 2, 8, 8, K_C, generator=g)
    m = (torch.rand(K_SHAPE, generator=g) < 0.4).to(torch.uint8)
    t = torch.tensor([0, 4, 9], dtype=torch.int32)
    return dict(gd=gd, x=x, noise=noise, eps=eps, m=m, t=t, xd=x.to(DEV), nd=noise.to(DEV), ed=eps.to(DEV), md=m.to(DEV), td=t.to(DEV))


def _q_masked(I, mask_dev, x_ptr=None, mask_ptr=None, per=None):
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd.gaussian_diffusion import vdx_q_sample_masked
    gd = I['gd']
    out = torch.empty_like(I['xd'])
    rc = vdx_q_sample_masked(x_ptr or L.ptr(I['xd']), L.ptr(I['td']), L.ptr(I['nd']), mask_ptr or L.ptr(mask_dev), L.ptr(out),
                             L.ptr(gd.sqrt_alphas_cumprod), L.ptr(gd.sqrt_one_minus_alphas_cumprod), K_B, per or I['x'].numel() // K_B, 2.0, -1.0,
                             L.stream_ptr())
    return rc, out


def test_q_sample_masked_kernel():
    I = _kin()
    gd, x, m = I['gd'], I['x'], I['m'].bool()
    plain = gd.q_sample(I['xd'], I['td'], noise=I['nd'], _pre=(2.0, -1.0)).cpu()
    norm = x * 2 - 1                                                     # == fmaf(x, 2, -1): x * 2 is exact, one rounding either way
    rc, out = _q_masked(I, I['md'])
    assert rc == 0
    out = out.cpu()
    assert torch.equal(out[m], norm[m])                                  # context elements: the normalised input, exactly
    assert torch.equal(out[~m], plain[~m])                               # the others: vdx_q_sample's bits
    assert not torch.equal(out, plain)
    # the public method with an element mask, a [B,F] mask and an [F] mask
    assert torch.equal(gd.q_sample(I['xd'], I['td'], noise=I['nd'], frame_mask=I['m'], _pre=(2.0, -1.0)).cpu(), out)
    bf = torch.tensor([[1, 0], [0, 0], [1, 1]], dtype=torch.uint8)
    got = gd.q_sample(I['xd'], I['td'], noise=I['nd'], frame_mask=bf, _pre=(2.0, -1.0)).cpu()
    assert torch.equal(got, torch.where(FR.expand(bf, K_SHAPE), norm, plain))
    got = gd.q_sample(I['xd'], I['td'], noise=I['nd'], frame_mask=torch.tensor([False, True]), _pre=(2.0, -1.0)).cpu()
    assert torch.equal(got[:, :, 1], norm[:, :, 1]) and torch.equal(got[:, :, 0], plain[:, :, 0])
    # the limits
    assert torch.equal(_q_masked(I, torch.zeros_like(I['md']))[1].cpu(), plain)
    assert torch.equal(_q_masked(I, torch.ones_like(I['md']))[1].cpu(), norm)
    # against the fp64 restatement (the bound test_gpu_diffusion.py puts on q_sample)
    ref = DiffusionRef(None, image_size=8, num_frames=2, channels=K_C, timesteps=K_T, dtype=torch.float64)
    exp = FR.q_sample_masked(ref, x.double() * 2 - 1, I['t'].long(), I['noise'].double(), m)
    np.testing.assert_allclose(out.double(), exp, atol=1e-5)


def test_q_sample_masked_rejects_misaligned_and_odd_sizes():
    from video_diffusion_nnx_amd import _lib as L
    I = _kin()
    assert _q_masked(I, I['md'], x_ptr=L.ptr(I['xd']) + 4)[0] == INVALID     # float tensor off its 16-byte boundary
    assert _q_masked(I, I['md'], mask_ptr=L.ptr(I['md']) + 1)[0] == INVALID  # mask off its 4-byte boundary
    assert _q_masked(I, I['md'], per=382)[0] == INVALID                      # per_sample % 4 != 0
    assert b'q_sample_masked' in L.vdx_last_error()


def _loss_masked(I, mask_dev, l2, scratch_fill):
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd.gaussian_diffusion import vdx_loss_masked_scratch_doubles, vdx_loss_sum_masked
    acc = torch.full((2 + vdx_loss_masked_scratch_doubles(),), scratch_fill, dtype=torch.float64, device=DEV)
    L.check(vdx_loss_sum_masked(L.ptr(I['ed']), L.ptr(I['nd']), L.ptr(mask_dev), acc.data_ptr() + 16, acc.data_ptr(), K_B, K_C, K_FHW, int(l2),
                                L.stream_ptr()))
    return acc


@pytest.mark.parametrize('l2', [False, True])
def test_loss_sum_masked_kernel(l2):
    I = _kin()
    m = I['m'].bool()
    pred = I['eps'].permute(0, 4, 1, 2, 3).double()
    exp_sum, exp_n = FR.loss_sum_count(pred, I['noise'].double(), m, l2)
    a = _loss_masked(I, I['md'], l2, float('nan'))                       # the kernels own the scratch: nothing in it is read first
    b = _loss_masked(I, I['md'], l2, 0.0)
    got_sum, got_n = a[0].item(), a[1].item()
    print(f'masked loss sum ({"l2" if l2 else "l1"}): {got_sum!r} vs fp64 {exp_sum.item()!r}, count {got_n} vs {exp_n}')
    assert got_n == exp_n == int((I['m'] == 0).sum())
    assert abs(got_sum - exp_sum.item()) <= 2e-5 * abs(exp_sum.item())
    assert torch.equal(a[:2].view(torch.int64), b[:2].view(torch.int64))  # two runs: equal bits
    full = _loss_masked(I, torch.ones_like(I['md']), l2, float('nan'))
    assert full[0].item() == 0.0 and full[1].item() == 0.0
    I['gd'].loss_type = 'l2' if l2 else 'l1'
    try:
        loss, _ = I['gd'].masked_loss(I['ed'], I['nd'], torch.ones_like(I['md']))
    finally:
        I['gd'].loss_type = 'l1'
    assert loss.item() == 0.0                                             # sum / max(count, 1): finite


@pytest.mark.parametrize('l2', [False, True])
def test_loss_grad_masked_kernel(l2):
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd.train_step import vdx_loss_grad, vdx_loss_grad_masked
    I = _kin()
    m = I['m'].bool()

    def run(mask_dev):
        acc = _loss_masked(I, mask_dev, l2, 0.0)
        d = torch.full_like(I['ed'], float('nan'))
        L.check(vdx_loss_grad_masked(L.ptr(I['ed']), L.ptr(I['nd']), L.ptr(mask_dev), acc.data_ptr() + 8, L.ptr(d), K_B, K_C, K_FHW, int(l2),
                                     L.stream_ptr()))
        return d.cpu()
    got = run(I['md']).permute(0, 4, 1, 2, 3)                            # channel-last -> [B,C,F,H,W]
    assert torch.isfinite(got).all() and (got[m] == 0.0).all() and (got[~m] != 0.0).any()
    e, n = I['eps'].permute(0, 4, 1, 2, 3).double(), I['noise'].double()
    exp = FR.loss_grad(e, n, m, l2)
    cnt = int((~m).sum())
    u = 2.0 ** -24
    # l1: sign(e - n) is exact in fp32 (a rounded difference keeps its sign), so the only error is the rounding of 1 / count.
    # l2: one rounding of e - n (at most u * (|e| + |n|)), the exact doubling, then 1 / count and the product, one rounding each.
    bound = u / cnt * 1.01 if not l2 else (2 * u * (e.abs() + n.abs()).max().item() + 3 * u * exp.abs().max().item() * cnt) / cnt
    err = (got.double() - exp).abs().max().item()
    print(f'masked loss grad ({"l2" if l2 else "l1"}): max-abs error {err:.3e}, bound {bound:.3e}')
    assert err <= bound
    plain = torch.empty_like(I['ed'])
    L.check(vdx_loss_grad(L.ptr(I['ed']), L.ptr(I['nd']), L.ptr(plain), K_B, K_C, K_FHW, int(l2), L.stream_ptr()))
    assert torch.equal(run(torch.zeros_like(I['md'])), plain.cpu())      # an all-zero mask is vdx_loss_grad bit for bit
    assert (run(torch.ones_like(I['md'])) == 0.0).all()                  # count 0: inv = 1, every element masked


# ---------------------------------------------------------------- p_losses and one train step ----------------------------------------------------------------

UKW = dict(dim=16, channels=1, dim_mults=(1, 2))
TR_SHAPE = (2, 1, 4, 8, 8)
HALF = torch.tensor([[1, 1, 0, 0], [0, 1, 0, 1]], dtype=torch.uint8)     # half the frames known, different ones per sample


def _mk(tmp_path, mode='f32', loss='l2', steps=3, **kw):
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.trainer import Trainer
    from video_diffusion_nnx_amd.unet3d import Unet3D
    unet = Unet3D(rngs=1, mode=mode, **UKW)
    gd = GaussianDiffusion(unet, image_size=8, num_frames=4, channels=1, timesteps=50, loss_type=loss)
    tr = Trainer(gd, str(tmp_path), dataset_path='synthetic:8', train_batch_size=2, train_num_steps=steps, train_lr=1e-3,
                 checkpoint_every_steps=1000, results_folder=str(tmp_path / 'res'), step_start_ema=0, update_ema_every=1, ema_decay=0.9, **kw)
    return unet, gd, tr


def _ref(params, loss):
    cfg = R.UnetConfig(**UKW)
    return DiffusionRef(lambda a, b: R.unet_forward(params, cfg, a, b), image_size=8, num_frames=4, channels=1, timesteps=50, loss_type=loss,
                        dtype=torch.float64)


@pytest.mark.parametrize('loss', ['l2', 'l1'])
def test_p_losses_with_frame_mask(tmp_path, loss):
    unet, gd, _ = _mk(tmp_path, loss=loss)
    p0 = {k: v.detach().cpu().double() for k, v in unet.state_dict().items()}
    g = torch.Generator().manual_seed(2)
    x = torch.rand(TR_SHAPE, generator=g)
    noise = torch.randn(TR_SHAPE, generator=g)
    t = torch.tensor([7, 41])
    ref = _ref(p0, loss)
    with torch.no_grad():
        exp_m = FR.p_losses(ref, x.double(), t, noise.double(), FR.expand(HALF, TR_SHAPE)).item()
        exp_u = FR.p_losses(ref, x.double(), t, noise.double(), None).item()
    got_m = gd.p_losses(x, t, noise=noise, frame_mask=HALF, _pre=(2.0, -1.0))
    got_u = gd.p_losses(x, t, noise=noise, _pre=(2.0, -1.0))
    assert got_m.is_cuda and got_m.dtype == torch.float32 and got_m.dim() == 0
    print(f'p_losses {loss}: masked {got_m.item():.7f} vs {exp_m:.7f}; unmasked {got_u.item():.7f} vs {exp_u:.7f}')
    assert abs(got_m.item() - exp_m) < 2e-5 * max(1.0, abs(exp_m))
    assert abs(got_u.item() - exp_u) < 2e-5 * max(1.0, abs(exp_u))      # frame_mask=None: the reference objective, as before
    assert abs(exp_m - exp_u) > 1e-3                                     # the two objectives differ on these inputs
    # __call__ forwards the keyword; an all-zero mask is the unmasked mean up to the order of the sum
    assert gd(x, 5, frame_mask=HALF).item() != gd(x, 5).item()
    zero = gd.p_losses(x, t, noise=noise, frame_mask=torch.zeros(4, dtype=torch.bool), _pre=(2.0, -1.0)).item()
    assert abs(zero - got_u.item()) <= 1e-6 * abs(got_u.item())


@pytest.mark.parametrize('loss', ['l2', 'l1'])
def test_one_masked_train_step_matches_oracle(tmp_path, loss):
    """Loss, gradient, Adam and EMA of one train step with half the frames known, against fp64 autograd through the restatement.
    Sensitivity, measured on the CPU when the inputs were chosen: the oracle gradient of the UNMASKED objective on the same inputs is
    0.51 (l2) / 0.58 (l1) relative L2 away from the masked one, over 2000 times the 2e-4 bound (the test asserts >= 10x), so code that
    ignores the mask cannot pass; the smallest |eps_hat - noise| off the mask is 8e-3, far from a sign flip of the l1 gradient."""
    unet, gd, tr = _mk(tmp_path, loss=loss)
    p0 = {k: v.detach().cpu().double().clone() for k, v in unet.state_dict().items()}
    batch = torch.rand(TR_SHAPE, generator=torch.Generator().manual_seed(0))
    loss_dev = tr.train_step(batch, step=0, frame_mask=HALF)
    torch.cuda.synchronize()
    assert torch.equal(torch.as_tensor(tr.last_frame_mask), HALF)
    t = tr.last_t.cpu().long()
    noise = torch.from_numpy(philox_ref.randn(batch.numel(), tr.last_noise_key, 0)).double().reshape(batch.shape)
    m = FR.expand(HALF, TR_SHAPE)
    ref_loss, grads = train_ref.loss_and_grads(p0, lambda params: FR.p_losses(_ref(params, loss), batch.double(), t, noise, m))
    assert abs(loss_dev.item() - ref_loss.item()) < 2e-5 * max(1.0, abs(ref_loss.item()))
    # the gradient: test_gpu_backward.py's f32 bounds (2e-4 total relative L2, its per-parameter rule)
    tol = 2e-4
    table = unet.param_table
    total_ref = torch.cat([grads[n].reshape(-1) for n, _, _ in table])
    total_got = torch.cat([tr.grads[o:o + int(np.prod(s))].cpu().double() for _, s, o in table])
    scale = total_ref.norm().item()
    rows = []
    for name, shape, off in table:
        got = tr.grads[off:off + int(np.prod(shape))].cpu().double().reshape(shape)
        rows.append((name, _rel(got, grads[name]), grads[name].norm().item(), got.norm().item()))
    bad = [(n, r) for n, r, nr, ng in rows if nr > 1e-6 * scale and r > tol * 5]
    dead = [(n, ng) for n, r, nr, ng in rows if nr <= 1e-6 * scale and ng > 1e-4 * scale]
    exact = [(n, ng) for n, r, nr, ng in rows if ('.fn.norm.' in n or n.startswith('time_rel_pos_bias')) and ng != 0.0]
    rel = _rel(total_got, total_ref)
    _, grads_unmasked = train_ref.loss_and_grads(p0, lambda params: FR.p_losses(_ref(params, loss), batch.double(), t, noise, None))
    miss = _rel(torch.cat([grads_unmasked[n].reshape(-1) for n, _, _ in table]), total_ref)
    print(f'masked train step {loss}: grads rel-L2 {rel:.3e} (bound {tol:.0e}); the unmasked objective is {miss:.3e} away')
    assert miss >= 10 * tol, miss
    assert not exact and not dead, (exact[:5], dead[:5])
    assert not bad, sorted(bad, key=lambda z: -z[1])[:6]
    assert rel < tol, rel
    # Adam / EMA as test_one_train_step_matches_oracle
    zeros = {k: torch.zeros_like(v) for k, v in p0.items()}
    p1, _, _ = train_ref.adam_update(p0, grads, zeros, zeros, count=0, lr=train_ref.lr_schedule(0, 1e-3))
    ema1 = train_ref.ema_update(p0, p1, step=0, step_start_ema=0, update_ema_every=1, decay=0.9)
    got = {k: v.detach().cpu().double() for k, v in unet.state_dict().items()}
    num = sum(((got[k] - p0[k]) - (p1[k] - p0[k])).pow(2).sum() for k in p0)
    den = sum((p1[k] - p0[k]).pow(2).sum() for k in p0)
    assert (num / den).sqrt().item() < 2e-2, (num / den).sqrt().item()
    ema_got = {n: tr.ema[o:o + int(np.prod(s))].cpu().double().reshape(s) for n, s, o in table}
    num = sum((ema_got[k] - ema1[k]).pow(2).sum() for k in p0)
    den = sum((ema1[k] - p0[k]).pow(2).sum() for k in p0)
    assert (num / den).sqrt().item() < 2e-2
    assert tr.opt_count == 1


# ---------------------------------------------------------------- Trainer ----------------------------------------------------------------

@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_frame_cond_steps_are_bit_reproducible_and_draw_the_documented_mask(tmp_path, mode):
    from video_diffusion_nnx_amd.train_step import frame_cond_key, frame_cond_masks
    ends = []
    for run in range(2):
        unet, gd, tr = _mk(tmp_path / f'r{run}', mode=mode)
        tr.frame_cond_max = 2                                           # on the instance: the class default stays 0 for every other test
        g = torch.Generator().manual_seed(5)
        losses, masks = [], []
        for step in range(3):
            losses.append(tr.train_step(torch.rand(TR_SHAPE, generator=g), step=step).item())
            masks.append(tr.last_frame_mask.clone())
            gen = torch.Generator().manual_seed(frame_cond_key(tr.rng_seed, tr.rank, step, 0) & 0x7FFFFFFFFFFFFFFF)
            assert torch.equal(masks[-1], frame_cond_masks(2, 4, 2, 0.25, 'random', gen))
        torch.cuda.synchronize()
        assert all(np.isfinite(losses)) and sum(int(m.sum()) for m in masks) > 0
        ends.append((losses, unet.flat_params.clone(), tr.ema.clone(), tr.m.clone(), tr.v.clone()))
    assert ends[0][0] == ends[1][0], (ends[0][0], ends[1][0])
    for a, b in zip(ends[0][1:], ends[1][1:]):
        assert torch.equal(a, b)


def test_frame_cond_accumulation_is_the_mean_of_the_single_gradients(tmp_path):
    g = torch.Generator().manual_seed(11)
    x = torch.rand(4, 1, 4, 8, 8, generator=g)
    t = torch.randint(0, 50, (4,), generator=g)
    noise = torch.randn(4, 1, 4, 8, 8, generator=g)
    masks = [HALF, torch.tensor([[0, 0, 0, 0], [1, 0, 1, 1]], dtype=torch.uint8)]      # 4 and 5 noised frames: two different counts
    _, _, A = _mk(tmp_path / 'a', gradient_accumulate_every=2)
    A.apply_grad_args = True
    la = A.train_step_accum([x[:2], x[2:]], 0, ts=[t[:2], t[2:]], noises=[noise[:2], noise[2:]], frame_masks=masks)
    singles, losses = [], []
    for j in range(2):
        _, _, S = _mk(tmp_path / f's{j}')
        losses.append(S.train_step(x[2 * j:2 * j + 2], 0, t=t[2 * j:2 * j + 2], noise=noise[2 * j:2 * j + 2], frame_mask=masks[j]).item())
        singles.append(S.grads.clone())
    torch.cuda.synchronize()
    rel = _rel(A.grads / 2, (singles[0] + singles[1]) / 2)
    print(f'[masked accum K=2 vs the two single steps] grads rel-L2 {rel:.3e}  loss {la.item():.7f} vs {np.mean(losses):.7f}')
    assert rel <= 2e-5, rel                                              # test_accumulation_equals_large_batch's comparison
    assert abs(la.item() - np.mean(losses)) <= 1e-5 * abs(np.mean(losses))
    assert _rel(singles[0], singles[1]) > 0.1


def test_frame_cond_off_is_bit_equal_to_an_untouched_trainer(tmp_path):
    ends = []
    for touched in (True, False):
        unet, gd, tr = _mk(tmp_path / f't{int(touched)}', mode='bf16')
        if touched:
            tr.frame_cond_max, tr.frame_cond_uncond_prob, tr.frame_cond_mode = 0, 0.9, 'prefix'
        g = torch.Generator().manual_seed(5)
        losses = [tr.train_step(torch.rand(TR_SHAPE, generator=g), step=step).item() for step in range(2)]
        torch.cuda.synchronize()
        assert tr.last_frame_mask is None
        ends.append((losses, unet.flat_params.clone(), tr.ema.clone()))
    assert ends[0][0] == ends[1][0]
    assert torch.equal(ends[0][1], ends[1][1]) and torch.equal(ends[0][2], ends[1][2])


# ---------------------------------------------------------------- short run, train -> sample ----------------------------------------------------------------

RUN_STEPS = 30


@pytest.fixture(scope='module')
def short_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('framecond_run')
    unet, gd, tr = _mk(tmp, mode='bf16', steps=RUN_STEPS)
    tr.frame_cond_max = 2
    losses = []
    tr.train(log_fn=lambda d: losses.append(d['loss']))
    return unet, gd, tr, losses


def test_short_frame_conditioned_run_decreases_loss(short_run):
    """The setup of test_short_training_run_decreases_loss (bf16, synthetic:8, lr 1e-3) with frame_cond_max = 2 and that test's
    criterion, last-5 mean < 0.7 x first-5 mean, at the same 30 steps."""
    unet, gd, tr, losses = short_run
    print('masked run: first 5', [round(v, 4) for v in losses[:5]], 'last 5', [round(v, 4) for v in losses[-5:]])
    assert len(losses) == RUN_STEPS and all(np.isfinite(losses))
    assert np.mean(losses[-5:]) < 0.7 * np.mean(losses[:5]), (losses[:5], losses[-5:])
    assert torch.isfinite(unet.flat_params).all() and tr.last_frame_mask is not None


def test_train_then_extend_with_clean_context(short_run):
    """No quality claim at this size: shape, range, finiteness, the context verbatim, determinism."""
    unet, gd, tr, _ = short_run
    video = torch.rand(2, 1, 2, 8, 8, generator=torch.Generator().manual_seed(3))
    out = gd.extend(9, video, 4, context_frames=2, dpm_steps=4, clean_context=True)
    assert out.shape == (2, 1, 6, 8, 8) and torch.isfinite(out).all()
    assert 0.0 <= out.min().item() and out.max().item() <= 1.0
    assert torch.equal(out[:, :, :2].cpu(), video)
    assert torch.equal(out, gd.extend(9, video, 4, context_frames=2, dpm_steps=4, clean_context=True))


# ---------------------------------------------------------------- clean-context sampling ----------------------------------------------------------------

def _gd(kw, T, frames, pseed):
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.unet3d import Unet3D
    cfg = R.UnetConfig(**kw)
    p = R.random_params(cfg, seed=pseed, dtype=torch.float64)
    unet = Unet3D(rngs=0, mode='f32', **kw)
    unet.load_state_dict({k: v.float() for k, v in p.items()})
    gd = GaussianDiffusion(unet, image_size=8, num_frames=frames, channels=kw['channels'], timesteps=T)
    ref = DiffusionRef(lambda a, b: R.unet_forward(p, cfg, a, b), image_size=8, num_frames=frames, channels=kw['channels'], timesteps=T,
                       dtype=torch.float64)
    return gd, ref


A_T, A_SHAPE, A_SEED = 6, (2, 1, 2, 8, 8), 2024                          # test_inpaint_ddpm_loop_matches_restated_loop's chain


@functools.lru_cache(None)
def _ancestral():
    gd, ref = _gd(dict(dim=16, channels=1), A_T, 2, 3)
    video = torch.rand(A_SHAPE, generator=torch.Generator().manual_seed(4))
    mask = torch.tensor([True, False])
    with torch.no_grad():
        exp = FR.clean_loop(ref, video, FR.expand(mask, A_SHAPE), A_SEED)
    return gd, video, mask, exp


@pytest.mark.parametrize('use_graph', [True, False])
def test_clean_context_ddpm_loop_matches_restated_loop(use_graph):
    gd, video, mask, exp = _ancestral()
    out = gd.inpaint(A_SEED, video, mask, use_graph=use_graph, clean_context=True)
    assert torch.equal(out, gd.inpaint(A_SEED, video, mask, use_graph=not use_graph, clean_context=True))     # graph == eager
    assert torch.equal(out, gd.inpaint(A_SEED, video, mask, use_graph=use_graph, clean_context=True))         # two runs agree
    np.testing.assert_allclose(out.cpu().double(), exp, atol=2e-4)
    assert (out[:, :, 0].cpu() - video[:, :, 0]).abs().max().item() <= 1e-6
    noisy = gd.inpaint(A_SEED, video, mask, use_graph=use_graph)         # the replacement method on the same seed: another chain
    assert (noisy - out)[:, :, 1].abs().max().item() > 1e-2
    assert (noisy[:, :, 0].cpu() - video[:, :, 0]).abs().max().item() <= 1e-6


S_T, S_STEPS, S_SHAPE, S_SEED = 60, 12, (2, 1, 4, 8, 8), 11              # the DDIM / DPM masked-loop tests' chain


@functools.lru_cache(None)
def _strided():
    gd, ref = _gd(dict(dim=16, channels=1, dim_mults=(1, 2)), S_T, 4, 2)
    video = torch.rand(S_SHAPE, generator=torch.Generator().manual_seed(7))
    return gd, ref, video, torch.tensor([True, True, False, False])


def test_clean_context_ddim_loop_matches_restated_loop():
    gd, ref, video, mask = _strided()
    out = gd.inpaint(S_SEED, video, mask, ddim_steps=S_STEPS, clean_context=True)
    assert torch.equal(out, gd.inpaint(S_SEED, video, mask, ddim_steps=S_STEPS, clean_context=True, use_graph=False))
    assert torch.equal(out, gd.inpaint(S_SEED, video, mask, ddim_steps=S_STEPS, clean_context=True))
    with torch.no_grad():
        exp = FR.clean_ddim(ref, video, FR.expand(mask, S_SHAPE), S_SEED, S_STEPS)
    err = (out.cpu().double() - exp).abs().max().item()
    print(f'clean-context ddim loop: max-abs error {err:.3e}')
    assert err < 5e-4, err
    assert (out[:, :, :2].cpu() - video[:, :, :2]).abs().max().item() <= 1e-6
    assert (gd.inpaint(S_SEED, video, mask, ddim_steps=S_STEPS) - out)[:, :, 2:].abs().max().item() > 1e-2


def test_clean_context_dpm_loop_matches_restated_loop():
    gd, ref, video, mask = _strided()
    out = gd.inpaint(S_SEED, video, mask, dpm_steps=S_STEPS, clean_context=True)
    assert torch.allclose(gd.inpaint(S_SEED, video, mask, dpm_steps=S_STEPS, clean_context=True, use_graph=False), out, atol=1e-5)
    assert torch.allclose(gd.inpaint(S_SEED, video, mask, dpm_steps=S_STEPS, clean_context=True), out, atol=1e-5)
    with torch.no_grad():
        exp = FR.clean_dpm(ref, video, FR.expand(mask, S_SHAPE), S_SEED, S_STEPS)
    err = (out.cpu().double() - exp).abs().max().item()
    print(f'clean-context dpm loop: max-abs error {err:.3e}')
    assert err < 5e-4, err
    assert (out[:, :, :2].cpu() - video[:, :, :2]).abs().max().item() <= 1e-6
    assert (gd.inpaint(S_SEED, video, mask, dpm_steps=S_STEPS) - out)[:, :, 2:].abs().max().item() > 1e-2


def test_extend_with_clean_context_keeps_the_given_frames():
    gd, _, video, _ = _strided()
    out = gd.extend(404, video[:, :, :2], 5, context_frames=2, ddim_steps=4, clean_context=True)
    assert out.shape == (2, 1, 7, 8, 8) and torch.isfinite(out).all()
    assert torch.equal(out[:, :, :2].cpu(), video[:, :, :2])            # the given frames, verbatim
    assert torch.equal(out, gd.extend(404, video[:, :, :2], 5, context_frames=2, ddim_steps=4, clean_context=True))
    assert not torch.equal(out, gd.extend(404, video[:, :, :2], 5, context_frames=2, ddim_steps=4))
    with pytest.raises(ValueError):
        gd.extend(404, video[:, :, :2], 5, context_frames=2, clean_context=True, resample_steps=2)
