"""CPU tests of the host side of frame-conditioned training and clean-context sampling: the exported symbols, the context-mask draw,
the key derivation, the CLI flags, the argument checks and the (1, 0) mask table."""
import ctypes
import os

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_exported():
    lib = ctypes.CDLL(os.path.join(ROOT, 'video_diffusion_nnx_amd', 'libvdx.so'))
    for name in ('vdx_q_sample_masked', 'vdx_loss_sum_masked', 'vdx_loss_grad_masked', 'vdx_loss_masked_scratch_doubles'):
        assert hasattr(lib, name), name
    fn = lib.vdx_loss_masked_scratch_doubles
    fn.restype = ctypes.c_size_t
    assert fn() >= 2 and fn() % 2 == 0                                   # (sum, count) pairs


def _masks(seed, **kw):
    from video_diffusion_nnx_amd.train_step import frame_cond_masks
    args = dict(batch=64, frames=6, k_max=3, uncond_prob=0.25, mode='random')
    args.update(kw)
    return frame_cond_masks(generator=torch.Generator().manual_seed(seed), **args)


def test_frame_cond_masks_distribution_and_determinism():
    m = _masks(1)
    assert m.dtype == torch.uint8 and tuple(m.shape) == (64, 6) and int(m.max()) == 1
    assert torch.equal(m, _masks(1)) and not torch.equal(m, _masks(2))  # a function of the generator seed
    known = m.sum(1)
    assert int(known.min()) == 0 and int(known.max()) == 3               # 64 rows at p_U = 0.25: both ends occur
    assert set(known.tolist()) <= {0, 1, 2, 3}
    rows = {tuple(r) for r in m.tolist() if sum(r) == 2}
    assert len(rows) > 1                                                 # 'random' does not always pick the same frames
    known = _masks(3, uncond_prob=0.0).sum(1)
    assert int(known.min()) >= 1 and int(known.max()) <= 3
    assert set(known.tolist()) == {1, 2, 3}                              # K ~ U{1..k_max}: 64 rows reach every value
    assert int(_masks(4, uncond_prob=1.0).sum()) == 0
    # k_max = frames - 1 still leaves a frame to learn from in every row
    assert int(_masks(5, frames=4, k_max=3, uncond_prob=0.0).sum(1).max()) <= 3


def test_frame_cond_masks_prefix_mode():
    m = _masks(6, mode='prefix', uncond_prob=0.1)
    for row in m.tolist():
        k = sum(row)
        assert 0 <= k <= 3 and row == [1] * k + [0] * (6 - k)
    assert len({sum(r) for r in m.tolist()}) > 2


def test_frame_cond_masks_reject_bad_arguments():
    from video_diffusion_nnx_amd.train_step import frame_cond_masks
    for k_max in (0, 4, 5, -1):                                          # 1 <= k_max <= frames - 1
        with pytest.raises(ValueError):
            frame_cond_masks(2, 4, k_max, 0.25, 'random', torch.Generator().manual_seed(0))
    with pytest.raises(ValueError):
        frame_cond_masks(2, 4, 2, 0.25, 'suffix', torch.Generator().manual_seed(0))
    with pytest.raises(ValueError):
        frame_cond_masks(2, 4, 2, 1.5, 'random', torch.Generator().manual_seed(0))
    assert tuple(frame_cond_masks(2, 4, 3, 0.25, 'random', torch.Generator().manual_seed(0)).shape) == (2, 4)


# (seed, rank, step, j) -> (t_key, noise_key) as the commit before frame conditioning returned them
RECORDED_KEYS = {
    (0, 0, 0, 0): (14889105232075457852, 1822111540196760150),
    (0, 0, 1, 0): (13224488989955454292, 17701553212694975379),
    (7, 1, 3, 0): (11595800749956405367, 9120156581778173839),
    (7, 1, 3, 2): (16869804886407263296, 13047859069775898528),
    (123456789, 3, 1000, 1): (14171614853370180354, 2185619051986813659),
}


def test_training_keys_are_unchanged_and_the_mask_key_is_new():
    from video_diffusion_nnx_amd.gaussian_diffusion import split_key
    from video_diffusion_nnx_amd.train_step import frame_cond_key, micro_step_keys
    for args, keys in RECORDED_KEYS.items():
        assert micro_step_keys(*args) == keys, args
        seed, rank, step, j = args
        step_key = split_key(split_key(seed, rank + 1)[-1], step + 1)[-1]
        micro = step_key if j == 0 else split_key(step_key, 3 + j)[-1]
        mk = frame_cond_key(*args)
        assert mk == split_key(micro, 3)[0]                              # child 1 of the micro-step key: the one the split discards
        _, t_key, loss_key = split_key(micro, 3)
        used = {t_key, loss_key, *keys, *split_key(loss_key, 3), *(split_key(step_key, 3 + jj)[-1] for jj in range(1, 9))}
        assert mk not in used


def test_trainer_class_defaults_are_off():
    from video_diffusion_nnx_amd.trainer import Trainer
    assert (Trainer.frame_cond_max, Trainer.frame_cond_uncond_prob, Trainer.frame_cond_mode) == (0, 0.25, 'random')


def test_train_cli_sets_frame_cond_attributes(tmp_path, monkeypatch):
    import sample
    import train
    from video_diffusion_nnx_amd import trainer as trainer_mod
    seen = []

    class FakeTrainer:
        apply_grad_args = False
        frame_cond_max = 0
        frame_cond_uncond_prob = 0.25
        frame_cond_mode = 'random'

        def __init__(self, **kw):
            cls = type(self)
            seen.append((cls.frame_cond_max, cls.frame_cond_uncond_prob, cls.frame_cond_mode))

        def train(self):
            pass
    cfg = {'unet': {}, 'diffusion': {'num_frames': 4}, 'trainer': dict(folder=str(tmp_path))}
    path = tmp_path / 'cfg.yaml'
    path.write_text(yaml.safe_dump(cfg))
    monkeypatch.setattr(sample, 'build_models', lambda cfg, mode: (None, None))
    monkeypatch.setattr(trainer_mod, 'Trainer', FakeTrainer)
    train.main(['--config', str(path)])
    assert seen == [(0, 0.25, 'random')]
    train.main(['--config', str(path), '--frame_cond_max', '3', '--frame_cond_uncond_prob', '0.5', '--frame_cond_mode', 'prefix'])
    assert seen[-1] == (3, 0.5, 'prefix')
    for bad in (['--frame_cond_max', '4'], ['--frame_cond_max', '-1'], ['--frame_cond_uncond_prob', '2'], ['--frame_cond_mode', 'suffix']):
        with pytest.raises(SystemExit):
            train.main(['--config', str(path)] + bad)


def test_sample_cli_clean_context_argument_errors(capsys):
    import sample
    a = sample.build_parser().parse_args(['--context', 'c.npy', '--clean-context'])
    assert a.clean_context is True and sample.build_parser().parse_args([]).clean_context is False
    for argv in (['--random-init', '--clean-context'],
                 ['--random-init', '--context', 'c.npy', '--clean-context', '--resample-steps', '2']):
        with pytest.raises(SystemExit) as e:
            sample.main(argv)
        assert e.value.code == 2
        assert '--clean-context' in capsys.readouterr().err


def _cpu_gd(T=4):
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.unet3d import Unet3D
    return GaussianDiffusion(Unet3D(dim=16, rngs=0, channels=1, device='cpu'), image_size=8, num_frames=2, channels=1, timesteps=T)


def test_clean_context_rejects_resampling_before_any_device_work():
    gd = _cpu_gd()
    video = torch.rand(2, 1, 2, 8, 8)
    with pytest.raises(ValueError, match='clean_context'):
        gd.inpaint(0, video, torch.tensor([True, False]), clean_context=True, resample_steps=2)
    with pytest.raises(ValueError, match='clean_context'):
        gd.extend(0, video[:, :, :1], 2, context_frames=1, clean_context=True, resample_steps=2)


def test_clean_mask_table_rows():
    from video_diffusion_nnx_amd.gaussian_diffusion import cosine_beta_schedule
    gd = _cpu_gd(T=7)
    tab = gd._mtab_clean
    assert tab.shape == (4, 7) and tab.dtype == torch.float32
    assert torch.equal(tab[0], torch.ones(7)) and torch.equal(tab[1], torch.zeros(7))
    betas = cosine_beta_schedule(7)
    assert torch.equal(tab[2], torch.from_numpy(np.sqrt(np.float32(1) - betas))) and torch.equal(tab[3], torch.from_numpy(np.sqrt(betas)))
    assert torch.equal(tab[2:], gd._mtab[2:]) and not torch.equal(tab[:2], gd._mtab[:2])      # the replacement-method table is untouched
