"""GPU tests of frame-conditioned sampling (GaussianDiffusion.inpaint / extend, sample.py --context): the masked reverse steps
against their formulas, the loops against the chains restated from oracle/diffusion_ref.py + philox_ref.py with the oracle UNet as
denoiser, the empty / full mask limits, guidance, data-parallel sharding, the captured step at the north-star shape and the CLI."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import philox_ref, unet3d_ref as R
from oracle.diffusion_ref import DiffusionRef

DEV = 'cuda:0'
DRAW_KNOWN, DRAW_RENOISE = 1 << 62, 1 << 63


def _z(shape, seed, draw):
    return torch.from_numpy(philox_ref.randn(int(np.prod(shape)), seed, draw)).double().reshape(shape)


def _gd(kw, T, frames=2, pseed=3):
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.unet3d import Unet3D
    cfg = R.UnetConfig(**kw)
    p = R.random_params(cfg, seed=pseed, dtype=torch.float64)
    unet = Unet3D(rngs=0, mode='f32', **kw)
    unet.load_state_dict({k: v.float() for k, v in p.items()})
    return GaussianDiffusion(unet, image_size=8, num_frames=frames, channels=kw['channels'], timesteps=T), cfg, p


def restated_loop(ref, video, m, seed, U=1):
    """The masked ancestral chain of vdx.h in fp64: init merge, then per (i, u) p_sample, merge, optional re-noise."""
    T, shape = ref.num_timesteps, tuple(video.shape)
    B = shape[0]
    k, m = 2 * video.double() - 1, m.bool()
    x = _z(shape, seed, 0)
    x = torch.where(m, ref.q_sample(k, torch.full((B,), T - 1), x), x)
    s = 0
    for i in reversed(range(T)):
        t = torch.full((B,), i)
        for u in range(U):
            xp = ref.p_sample(x, t, _z(shape, seed, 1 + s))
            kn = k if i == 0 else ref.q_sample(k, t - 1, _z(shape, seed, DRAW_KNOWN + s))
            x = torch.where(m, kn, xp)
            if u < U - 1:
                beta = ref.tab['betas'][i]
                x = (1 - beta).sqrt() * x + beta.sqrt() * _z(shape, seed, DRAW_RENOISE + s)
            s += 1
    return (x + 1) / 2


def restated_ddim(ref, video, m, seed, S):
    """The masked DDIM chain of vdx.h in fp64 (eta = 0, static clip)."""
    T, shape = ref.num_timesteps, tuple(video.shape)
    B = shape[0]
    seq = np.linspace(-1, T - 1, S + 1).astype(np.int64)[::-1]
    ac = ref.tab['alphas_cumprod']
    k, m = 2 * video.double() - 1, m.bool()
    x = _z(shape, seed, 0)
    x = torch.where(m, ac[seq[0]].sqrt() * k + (1 - ac[seq[0]]).sqrt() * x, x)
    for j in range(S):
        t, tn = int(seq[j]), int(seq[j + 1])
        eps = ref.denoise(x, torch.full((B,), t)).permute(0, 4, 1, 2, 3)
        a_t = ac[t]
        a_n = ac[tn] if tn >= 0 else torch.ones((), dtype=ac.dtype)
        x0 = ((x - (1 - a_t).sqrt() * eps) / a_t.sqrt()).clamp(-1, 1)
        xp = a_n.sqrt() * x0 + (1 - a_n).sqrt() * (x - a_t.sqrt() * x0) / (1 - a_t).sqrt()
        kn = k if tn < 0 else a_n.sqrt() * k + (1 - a_n).sqrt() * _z(shape, seed, DRAW_KNOWN + j)
        x = torch.where(m, kn, xp)
    return (x + 1) / 2


@pytest.mark.parametrize('clip', [True, False])
def test_masked_step_elementwise(clip):
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion, vdx_p_sample_step, vdx_p_sample_step_masked
    from video_diffusion_nnx_amd.unet3d import Unet3D
    T, B, shape = 10, 3, (3, 3, 2, 8, 8)
    gd = GaussianDiffusion(Unet3D(rngs=0, mode='f32', dim=16, channels=3), image_size=8, num_frames=2, channels=3, timesteps=T)
    ref = DiffusionRef(None, image_size=8, num_frames=2, channels=3, timesteps=T, dtype=torch.float64)
    g = torch.Generator().manual_seed(5)
    x = 2 * torch.randn(shape, generator=g)
    eps = torch.randn(B, 2, 8, 8, 3, generator=g)
    k = 2 * torch.rand(shape, generator=g) - 1
    m = (torch.rand(shape, generator=g) < 0.4).to(torch.uint8)
    t = torch.tensor([0, 4, 9])                                          # t = 0, mid, T-1
    seed, per = 91, x.numel() // B
    xd, ed, kd, md, td = x.to(DEV), eps.to(DEV), k.to(DEV), m.to(DEV), t.to(DEV, torch.int32)

    def run(mask, U, step, step_dev=None):
        out = torch.empty_like(xd)
        L.check(vdx_p_sample_step_masked(L.ptr(xd), L.ptr(ed), L.ptr(out), L.ptr(td), L.ptr(gd._ptab), T, L.ptr(kd), L.ptr(mask), L.ptr(gd._mtab),
                                         U, seed, step, L.ptr(step_dev), 0, int(clip), B, 3, per, L.stream_ptr()))
        return out.cpu()

    for U, s in ((1, 7), (3, 4), (3, 5)):                               # U = 3: s = 4 re-noises (4 % 3 != 2), s = 5 does not
        got = run(md, U, s).double()
        xp = ref.p_sample(x.double(), t, _z(shape, seed, 1 + s), clip_denoised=clip, eps_pred=eps.double())
        kn = torch.where((t > 0).reshape(-1, 1, 1, 1, 1), ref.q_sample(k.double(), (t - 1).clamp_min(0), _z(shape, seed, DRAW_KNOWN + s)),
                         k.double())
        exp = torch.where(m.bool(), kn, xp)
        if s % U != U - 1:
            beta = ref.tab['betas'][t].reshape(-1, 1, 1, 1, 1)
            exp = (1 - beta).sqrt() * exp + beta.sqrt() * _z(shape, seed, DRAW_RENOISE + s)
        else:
            assert torch.equal(got[0][m[0].bool()], k[0][m[0].bool()].double())      # known elements at t = 0 are k exactly
        np.testing.assert_allclose(got, exp, atol=5e-5)
    # s from the device counter: step 2 + *step_dev 5 == explicit step 7
    assert torch.equal(run(md, 1, 2, torch.full((1,), 5, dtype=torch.int64, device=DEV)), run(md, 1, 7))
    # an all-zero mask (U = 1) is the unconditional step at the same draw, bit for bit
    plain = torch.empty_like(xd)
    L.check(vdx_p_sample_step(L.ptr(xd), L.ptr(ed), L.ptr(plain), L.ptr(td), L.ptr(gd._ptab), T, 0, seed, 1 + 7, 0, 0, int(clip), B, 3, per,
                              L.stream_ptr()))
    assert torch.equal(run(torch.zeros_like(md), 1, 7), plain.cpu())


def test_masked_ddim_step_elementwise():
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion, ddim_time_sequence, vdx_ddim_step, vdx_ddim_step_masked
    from video_diffusion_nnx_amd.unet3d import Unet3D
    T, B, C, shape = 1000, 3, 2, (3, 2, 4, 8, 8)
    gd = GaussianDiffusion(Unet3D(rngs=0, mode='f32', dim=16, channels=C), image_size=8, num_frames=4, channels=C, timesteps=T)
    seq = ddim_time_sequence(T, 100)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(shape, generator=g)
    eps = torch.randn(B, 4, 8, 8, C, generator=g)
    k = 2 * torch.rand(shape, generator=g) - 1
    m = (torch.rand(shape, generator=g) < 0.5).to(torch.uint8)
    seed, per = 17, x.numel() // B
    xd, ed, kd, md, seqd = x.to(DEV), eps.to(DEV), k.to(DEV), m.to(DEV), torch.from_numpy(seq).to(DEV)
    ac = gd.alphas_cumprod.cpu().double()
    for j in (0, 57, 99):                                               # first, middle, last (seq[j+1] = -1: the data itself)
        step = torch.full((1,), j, dtype=torch.int64, device=DEV)

        def run(mask):
            out = torch.empty_like(xd)
            L.check(vdx_ddim_step_masked(L.ptr(xd), L.ptr(ed), L.ptr(out), L.ptr(gd.alphas_cumprod), L.ptr(seqd), L.ptr(step), 0, 1, L.ptr(kd),
                                         L.ptr(mask), L.ptr(gd._mtab), T, seed, B, C, per, L.stream_ptr()))
            return out.cpu()
        got = run(md).double()
        t, tn = int(seq[j]), int(seq[j + 1])
        a_t, a_n = ac[t], (ac[tn] if tn >= 0 else torch.tensor(1.0, dtype=torch.float64))
        e = eps.permute(0, 4, 1, 2, 3).double()
        x0 = ((x.double() - (1 - a_t).sqrt() * e) / a_t.sqrt()).clamp(-1, 1)
        xp = a_n.sqrt() * x0 + (1 - a_n).sqrt() * (x.double() - a_t.sqrt() * x0) / (1 - a_t).sqrt()
        kn = k.double() if tn < 0 else a_n.sqrt() * k.double() + (1 - a_n).sqrt() * _z(shape, seed, DRAW_KNOWN + j)
        exp = torch.where(m.bool(), kn, xp)
        assert (got - exp).abs().max().item() < 2e-5 * max(1.0, exp.abs().max().item()), j
        if tn < 0:
            assert torch.equal(got[m.bool()], k[m.bool()].double())
        plain = torch.empty_like(xd)
        L.check(vdx_ddim_step(L.ptr(xd), L.ptr(ed), L.ptr(plain), L.ptr(gd.alphas_cumprod), L.ptr(seqd), L.ptr(step), 0, 1, B, C, per, L.stream_ptr()))
        assert torch.equal(run(torch.zeros_like(md)), plain.cpu())     # an all-zero mask is the unconditional DDIM step


@pytest.mark.parametrize('use_graph', [True, False])
def test_inpaint_ddpm_loop_matches_restated_loop(use_graph):
    kw = dict(dim=16, channels=1)
    T, B, shape, seed = 6, 2, (2, 1, 2, 8, 8), 2024
    gd, cfg, p = _gd(kw, T)
    video = torch.rand(shape, generator=torch.Generator().manual_seed(4))
    mask = torch.tensor([True, False])                                   # first frame known
    out = gd.inpaint(seed, video, mask, use_graph=use_graph)
    assert torch.equal(out, gd.inpaint(seed, video, mask, use_graph=not use_graph))     # graph == eager
    assert torch.equal(out, gd.inpaint(seed, video, mask, use_graph=use_graph))         # two runs agree
    ref = DiffusionRef(lambda a, b: R.unet_forward(p, cfg, a, b), image_size=8, num_frames=2, channels=1, timesteps=T, dtype=torch.float64)
    exp = restated_loop(ref, video, mask.reshape(1, 1, 2, 1, 1).expand(shape), seed)
    np.testing.assert_allclose(out.cpu().double(), exp, atol=2e-4)
    assert (out[:, :, 0].cpu() - video[:, :, 0]).abs().max().item() <= 1e-6


def test_inpaint_resample_loop_matches_restated_loop():
    kw = dict(dim=16, channels=1)
    T, U, shape, seed = 4, 3, (2, 1, 2, 8, 8), 77
    gd, cfg, p = _gd(kw, T)
    video = torch.rand(shape, generator=torch.Generator().manual_seed(6))
    mask = torch.tensor([[True, False], [False, True]])                  # [B, F]: a different known frame per video
    out = gd.inpaint(seed, video, mask, resample_steps=U)
    ref = DiffusionRef(lambda a, b: R.unet_forward(p, cfg, a, b), image_size=8, num_frames=2, channels=1, timesteps=T, dtype=torch.float64)
    exp = restated_loop(ref, video, mask.reshape(2, 1, 2, 1, 1).expand(shape), seed, U)
    np.testing.assert_allclose(out.cpu().double(), exp, atol=3e-4)
    assert (out[0, :, 0].cpu() - video[0, :, 0]).abs().max().item() <= 1e-6
    assert (out[1, :, 1].cpu() - video[1, :, 1]).abs().max().item() <= 1e-6


@pytest.mark.parametrize('use_graph', [True, False])
def test_inpaint_ddim_loop_matches_restated_loop(use_graph):
    kw = dict(dim=16, channels=1, dim_mults=(1, 2))
    T, S, shape, seed = 60, 12, (2, 1, 4, 8, 8), 11
    gd, cfg, p = _gd(kw, T, frames=4, pseed=2)
    video = torch.rand(shape, generator=torch.Generator().manual_seed(7))
    mask = torch.tensor([True, True, False, False])
    out = gd.inpaint(seed, video, mask, ddim_steps=S, use_graph=use_graph)
    ref = DiffusionRef(lambda a, b: R.unet_forward(p, cfg, a, b), image_size=8, num_frames=4, channels=1, timesteps=T, dtype=torch.float64)
    exp = restated_ddim(ref, video, mask.reshape(1, 1, 4, 1, 1).expand(shape), seed, S)
    err = (out.cpu().double() - exp).abs().max().item()
    assert err < 5e-4, err
    assert (out[:, :, :2].cpu() - video[:, :, :2]).abs().max().item() <= 1e-6
    with pytest.raises(ValueError):
        gd.inpaint(seed, video, mask, ddim_steps=S, resample_steps=2)


def test_empty_and_full_masks():
    kw = dict(dim=16, channels=1)
    T, shape, seed = 6, (2, 1, 2, 8, 8), 31
    gd, _, _ = _gd(kw, T)
    video = torch.rand(shape, generator=torch.Generator().manual_seed(8))
    empty = gd.inpaint(seed, video, torch.zeros(2, dtype=torch.bool))
    assert torch.equal(empty, gd.p_sample_loop(shape, seed))            # same draws, same arithmetic
    empty_d = gd.inpaint(seed, video, torch.zeros(2, dtype=torch.bool), ddim_steps=3)
    assert (empty_d - gd.ddim_sample_loop(shape, seed, steps=3)).abs().max().item() <= 1e-5
    for kw_ in (dict(resample_steps=2), dict(ddim_steps=3)):
        full = gd.inpaint(seed, video, torch.ones(shape, dtype=torch.uint8), **kw_)
        assert (full.cpu() - video).abs().max().item() <= 1e-6
    # the dynamic threshold inside the masked loop: an empty mask is p_sample_loop with the same threshold
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    gdt = GaussianDiffusion(gd.denoise_fn, image_size=8, num_frames=2, channels=1, timesteps=T, use_dynamic_thres=True)
    assert torch.equal(gdt.inpaint(seed, video, torch.zeros(2, dtype=torch.bool)), gdt.p_sample_loop(shape, seed))


def test_inpaint_guided():
    kw = dict(dim=16, channels=1, cond_dim=32)
    T, B, shape, seed = 4, 2, (2, 1, 2, 8, 8), 5
    gd, cfg, p = _gd(kw, T)
    cond = torch.randn(B, 32, generator=torch.Generator().manual_seed(9))
    video = torch.rand(shape, generator=torch.Generator().manual_seed(10))
    mask = torch.tensor([False, True])
    out = gd.inpaint(seed, video, mask, cond=cond.to(DEV), cond_scale=2.0)
    ref = DiffusionRef(lambda a, b: R.forward_with_cond_scale(p, cfg, a, b, cond=cond.double(), cond_scale=2.0), image_size=8, num_frames=2,
                       channels=1, timesteps=T, dtype=torch.float64)
    exp = restated_loop(ref, video, mask.reshape(1, 1, 2, 1, 1).expand(shape), seed)
    np.testing.assert_allclose(out.cpu().double(), exp, atol=5e-4)
    empty = gd.inpaint(seed, video, torch.zeros(2, dtype=torch.bool), cond=cond.to(DEV), cond_scale=2.0)
    assert torch.equal(empty, gd.p_sample_loop(shape, seed, cond=cond.to(DEV), cond_scale=2.0))


def test_inpaint_shards_like_sample(monkeypatch):
    import video_diffusion_nnx_amd.gaussian_diffusion as G
    gd, _, _ = _gd(dict(dim=16, channels=1), 4)
    g = torch.Generator().manual_seed(12)
    video = torch.rand(4, 1, 2, 8, 8, generator=g)
    mask = torch.rand(4, 2, generator=g) < 0.5
    for r in range(2):
        monkeypatch.setattr(G, 'dist_rank_world', lambda r=r: (r, 2))
        got = gd.inpaint(21, video, mask)
        monkeypatch.setattr(G, 'dist_rank_world', lambda: (0, 1))
        assert got.shape == (2, 1, 2, 8, 8)
        assert torch.equal(got, gd.inpaint(G.shard_key(21, r, 2), video[2 * r:2 * r + 2], mask[2 * r:2 * r + 2]))
        monkeypatch.setattr(G, 'dist_rank_world', lambda r=r: (r, 2))
        ext = gd.extend(21, video[:, :, :1], 2, context_frames=1)          # sharded once: rows + shard key, then the windows
        monkeypatch.setattr(G, 'dist_rank_world', lambda: (0, 1))
        assert torch.equal(ext, gd.extend(G.shard_key(21, r, 2), video[2 * r:2 * r + 2, :, :1], 2, context_frames=1))


def test_extend_autoregressive():
    from video_diffusion_nnx_amd.gaussian_diffusion import extend_plan, split_key
    gd, _, _ = _gd(dict(dim=16, channels=1), 4, frames=4)
    B, seed = 2, 404
    video = torch.rand(B, 1, 2, 8, 8, generator=torch.Generator().manual_seed(13))
    out = gd.extend(seed, video, 5, context_frames=2)
    assert out.shape == (B, 1, 7, 8, 8)
    assert torch.equal(out[:, :, :2].cpu(), video)                      # the given frames, verbatim
    plan = extend_plan(2, 5, 4, 2)
    assert plan == [(2, 2), (2, 2), (2, 1)]
    clip, have = video.to(DEV), 2
    for (c, n), k in zip(plan, split_key(seed, len(plan))):             # the windows replayed by hand with the documented keys
        win = torch.zeros(B, 1, 4, 8, 8, device=DEV)
        win[:, :, :c] = clip[:, :, have - c:have]
        o = gd.inpaint(k, win, torch.arange(4) < c)
        clip = torch.cat([clip, o[:, :, c:c + n]], 2)
        have += n
    assert torch.equal(out, clip)
    assert torch.equal(out, gd.extend(seed, video, 5, context_frames=2))      # deterministic


def test_inpaint_north_star_shape_bf16():
    """dim 64, 16f x 64^2, B 2, bf16 operands + bf16 activation storage, T 8, U 2, 8 frames known: 3 graph-replayed masked steps
    equal 3 eager ones bitwise; the device counter ends at T*U with t = 0; the result is finite, in [0, 1], known frames exact."""
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion, frame_mask, vdx_inpaint_init, vdx_p_sample_loop_masked
    from video_diffusion_nnx_amd.unet3d import Unet3D
    T, U, B, Fr, S = 8, 2, 2, 16, 64
    unet = Unet3D(rngs=0, mode='bf16', dim=64, channels=1)
    gd = GaussianDiffusion(unet, image_size=S, num_frames=Fr, channels=1, timesteps=T)
    shape = (B, 1, Fr, S, S)
    video = torch.rand(shape, generator=torch.Generator().manual_seed(15))
    frames = torch.arange(Fr) < 8
    h = unet.handle(Fr, S)
    unet.act_bf16 = True
    unet.apply_activation_storage(h)
    ws = unet.workspace(B, Fr, S)
    st = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(st):
        known = (2 * video - 1).to(DEV)
        mask = frame_mask(frames, shape).to(DEV)
        x_T = gd.randn(shape, 77, 0)
        eps = torch.empty(B, Fr, S, S, 1, device=DEV)

        def chain(n_list, graph):
            img = x_T.clone()
            L.check(vdx_inpaint_init(L.ptr(img), L.ptr(known), L.ptr(mask), L.ptr(gd._mtab), T, T - 1, img.numel(), L.stream_ptr()))
            t_dev = torch.full((B,), T - 1, dtype=torch.int32, device=DEV)
            step_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
            states = []
            for n in n_list:
                L.check(vdx_p_sample_loop_masked(h.ptr, L.ptr(unet.flat_params), L.ptr(unet.packed()), L.ptr(img), L.ptr(eps), L.ptr(t_dev),
                                                 L.ptr(step_dev), L.ptr(gd._ptab), T, n, 0, 77, 1, 0.0, 0, L.ptr(known), L.ptr(mask), L.ptr(gd._mtab),
                                                 U, L.ptr(ws), ws.numel(), B, graph, L.stream_ptr()))
                st.synchronize()
                states.append((img.clone(), t_dev.clone().cpu(), int(step_dev.item())))
            return states
        eager = chain([3], 0)
        graph = chain([3, T * U - 3], 1)
    unet.act_bf16 = False
    assert torch.equal(eager[0][0], graph[0][0]), 'graph replay != eager loop after 3 masked steps'
    assert graph[0][2] == 3 and graph[0][1].tolist() == [T - 2] * B    # s = 1 dropped t once; s = 0, 2 re-noised at the same level
    assert graph[1][2] == T * U and graph[1][1].tolist() == [0] * B
    x0 = graph[1][0]
    assert torch.isfinite(x0).all() and x0.abs().max().item() <= 1.0
    assert torch.equal(x0[:, :, :8], known[:, :, :8])                  # known frames exact
    out = gd.inpaint(77, video, frames, resample_steps=U)
    assert torch.allclose(out, (x0 + 1) * 0.5, rtol=0, atol=1e-6)
    assert 0.0 <= out.min().item() and out.max().item() <= 1.0
    assert (out[:, :, :8].cpu() - video[:, :, :8]).abs().max().item() <= 1e-6


def test_sample_cli_context(tmp_path):
    import yaml
    from PIL import Image
    import sample
    cfg = {'unet': dict(dim=16, dim_mults=[1, 2], channels=1, rngs_seed=0, use_bert_text_cond=False),
           'diffusion': dict(image_size=16, num_frames=4, channels=1, timesteps=6, loss_type='l2'), 'trainer': {}}
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    ctx = np.random.default_rng(0).random((2, 1, 3, 16, 16)).astype(np.float32)     # random: PIL merges identical consecutive frames
    np.save(tmp_path / 'clip.npy', ctx)
    out = tmp_path / 'gifs'
    sample.main(['--config', str(tmp_path / 'cfg.yaml'), '--random-init', '--context', str(tmp_path / 'clip.npy'), '--context-frames', '2',
                 '--extend-frames', '3', '--mode', 'f32', '--output-path', str(out)])
    gifs = sorted(out.glob('sample_*.gif'))
    assert [g.name for g in gifs] == ['sample_0.gif', 'sample_1.gif']
    assert all(Image.open(g).n_frames == 4 + 3 for g in gifs)
