"""CPU tests of the host side of frame-conditioned sampling: mask broadcasting and argument checks of GaussianDiffusion.inpaint."""
import numpy as np
import pytest
import torch


def test_frame_mask_broadcasts_and_rejects():
    from video_diffusion_nnx_amd.gaussian_diffusion import frame_mask
    shape = (2, 3, 4, 8, 8)
    m = frame_mask(torch.tensor([True, False, True, False]), shape)
    assert m.dtype == torch.uint8 and tuple(m.shape) == shape and m.is_contiguous()
    assert m[:, :, 0].all() and m[:, :, 2].all() and not m[:, :, 1].any() and not m[:, :, 3].any()
    m2 = frame_mask(torch.tensor([[1, 0, 0, 0], [1, 7, 0, 0]], dtype=torch.uint8), shape)     # [B, F]; any nonzero byte is known
    assert m2[1, :, 1].all() and not m2[0, :, 1].any() and m2.max().item() == 1
    full = torch.zeros(shape, dtype=torch.bool)
    full[..., :4, :] = True
    assert torch.equal(frame_mask(full, shape), full.to(torch.uint8))
    assert frame_mask(np.ones((1, 1, 1, 8, 1), np.bool_), shape).all()
    for bad in (torch.ones(5, dtype=torch.bool), torch.ones(3, 4, dtype=torch.bool), torch.ones(2, 3, 4, 8, 9, dtype=torch.bool),
                torch.ones(4), torch.ones(1, 2, 3, 4, 8, 8, dtype=torch.bool)):
        with pytest.raises(ValueError):
            frame_mask(bad, shape)


def test_inpaint_rejects_bad_arguments_before_any_device_work():
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.unet3d import Unet3D
    gd = GaussianDiffusion(Unet3D(dim=16, rngs=0, channels=1, device='cpu'), image_size=8, num_frames=2, channels=1, timesteps=4)
    video = torch.rand(2, 1, 2, 8, 8)
    with pytest.raises(ValueError):
        gd.inpaint(0, video, torch.tensor([True, False]), resample_steps=0)
    with pytest.raises(ValueError):
        gd.inpaint(0, torch.rand(2, 1, 3, 8, 8), torch.tensor([True, False, True]))
    with pytest.raises(ValueError):
        gd.inpaint(0, video, torch.tensor([1.0, 0.0]))
    assert gd._mtab.shape == (4, 4)
    np.testing.assert_allclose((gd._mtab[2] ** 2 + gd._mtab[3] ** 2).numpy(), 1.0, atol=1e-6)   # sqrt(alpha)^2 + sqrt(beta)^2


def test_inpaint_rejects_ddim_resampling_and_a_wrong_x_T():
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.unet3d import Unet3D
    gd = GaussianDiffusion(Unet3D(dim=16, rngs=0, channels=1, device='cpu'), image_size=8, num_frames=2, channels=1, timesteps=4)
    video = torch.rand(2, 1, 2, 8, 8)
    with pytest.raises(ValueError):
        gd.inpaint(0, video, torch.tensor([True, False]), ddim_steps=2, resample_steps=2)
    for bad in (torch.zeros(3, 1, 2, 8, 8), torch.zeros(2, 1, 2, 8, 4)):
        with pytest.raises(ValueError):
            gd.inpaint(0, video, torch.tensor([True, False]), x_T=bad)
    with pytest.raises(ValueError):
        gd.extend(0, video[:, :, :1], 2, context_frames=2)              # context must leave a frame to generate


def test_extend_window_plan():
    from video_diffusion_nnx_amd.gaussian_diffusion import extend_plan
    assert extend_plan(2, 5, 4, 2) == [(2, 2), (2, 2), (2, 1)]
    assert extend_plan(5, 15, 10, 5) == [(5, 5)] * 3
    assert extend_plan(1, 3, 4, 2) == [(1, 3)]                          # fewer frames than the context: all of them
    assert extend_plan(3, 0, 4, 2) == []
    for args in ((2, 5, 4, 0), (2, 5, 4, 4), (0, 5, 4, 2), (2, -1, 4, 2)):
        with pytest.raises(ValueError):
            extend_plan(*args)


def test_sample_context_flags_parse_and_load(tmp_path):
    import sample
    a = sample.build_parser().parse_args(['--context', 'c.npy', '--context-frames', '5', '--extend-frames', '10', '--resample-steps', '2'])
    assert (a.context, a.context_frames, a.extend_frames, a.resample_steps) == ('c.npy', 5, 10, 2)
    a = sample.build_parser().parse_args([])
    assert a.context is None and a.context_frames is None and a.extend_frames == 0 and a.resample_steps == 1
    v = (np.random.default_rng(1).random((2, 1, 6, 8, 8)) * 255).astype(np.uint8)
    np.save(tmp_path / 'c.npy', v)
    ctx, n_new = sample.load_context(tmp_path / 'c.npy', 4, context_frames=3, extend_frames=2)
    assert ctx.shape == (2, 1, 3, 8, 8) and ctx.dtype == np.float32 and n_new == 4 + 2 - 3
    np.testing.assert_allclose(ctx, v[:, :, :3] / 255.0, rtol=1e-6)
    f = np.random.default_rng(2).random((1, 1, 5, 8, 8)).astype(np.float32)
    np.save(tmp_path / 'f.npy', f)
    ctx, n_new = sample.load_context(tmp_path / 'f.npy', 10, extend_frames=10)        # default: every frame of the file
    assert np.array_equal(ctx, f) and n_new == 15
    np.save(tmp_path / 'bad.npy', f[0])
    for path, k, n in (('bad.npy', None, 0), ('f.npy', 6, 0), ('f.npy', 0, 0), ('f.npy', 5, -1)):
        with pytest.raises(ValueError):
            sample.load_context(tmp_path / path, 4 if k != 6 else 10, context_frames=k, extend_frames=n)
