"""CPU tests of the host side of classifier-free guidance end to end: the exported symbols, the condition-dropout draw and its key,
the (video, cond) dataset pairing, the cond-file checks, the tuple batches of the prefetcher, the CLI flags and the guidance_rescale
range check."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_exported():
    lib = ctypes.CDLL(os.path.join(ROOT, 'video_diffusion_nnx_amd', 'libvdx.so'))
    for name in ('vdx_cfg_combine', 'vdx_cfg_scratch_doubles', 'vdx_p_sample_loop_guided', 'vdx_ddim_sample_loop_guided',
                 'vdx_dpm_sample_loop_guided'):
        assert hasattr(lib, name), name
    from video_diffusion_nnx_amd import _lib as L
    n1, n3 = L.vdx_cfg_scratch_doubles(1), L.vdx_cfg_scratch_doubles(3)
    assert n1 >= 4 + 1 + 1 and n3 >= 3 * n1 - 3                         # four sums and a factor per sample, plus the 2B-byte mask
    assert L.vdx_cfg_scratch_doubles(0) == 0
    from video_diffusion_nnx_amd import train_step, datasets
    for name in ('cond_drop_mask', 'cond_drop_key'):
        assert callable(getattr(train_step, name))
    for name in ('CondPairs', 'load_cond_file'):
        assert callable(getattr(datasets, name))


def test_cond_drop_mask():
    from video_diffusion_nnx_amd.train_step import cond_drop_mask
    g = lambda s: torch.Generator().manual_seed(s)
    m0, m1 = cond_drop_mask(64, 0.0, g(1)), cond_drop_mask(64, 1.0, g(1))
    assert m0.dtype == m1.dtype == torch.uint8 and tuple(m0.shape) == tuple(m1.shape) == (64,)
    assert int(m0.sum()) == 0 and int(m1.sum()) == 64
    a, b, c = cond_drop_mask(64, 0.5, g(2)), cond_drop_mask(64, 0.5, g(2)), cond_drop_mask(64, 0.5, g(3))
    assert torch.equal(a, b) and not torch.equal(a, c)                    # a function of the generator state
    assert 0 < int(a.sum()) < 64 and set(a.tolist()) <= {0, 1}
    assert abs(float(cond_drop_mask(4096, 0.25, g(4)).float().mean()) - 0.25) < 0.04      # 6 sigma of Bernoulli(0.25) over 4096 draws
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            cond_drop_mask(4, bad, g(0))


def test_cond_drop_key_is_a_stream_of_its_own():
    from video_diffusion_nnx_amd.gaussian_diffusion import split_key
    from video_diffusion_nnx_amd.train_step import cond_drop_key, frame_cond_key, micro_step_keys
    seen = set()
    for seed, rank, step, j in ((0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0), (0, 1, 0, 0), (7, 0, 3, 2), (7, 3, 3, 0), (123456789, 5, 999, 3)):
        ck = cond_drop_key(seed, rank, step, j)
        t_key, noise_key = micro_step_keys(seed, rank, step, j)
        assert ck not in (t_key, noise_key, frame_cond_key(seed, rank, step, j))
        # child 1 of the loss key: the child micro_step_keys' `_, noise_key, _ = split_key(loss_key, 3)` discards
        step_key = split_key(split_key(seed, rank + 1)[-1], step + 1)[-1]
        if j > 0:
            step_key = split_key(step_key, 3 + j)[-1]
        loss_key = split_key(step_key, 3)[2]
        assert split_key(loss_key, 3)[1] == noise_key and split_key(loss_key, 3)[0] == ck
        assert ck not in seen
        seen.add(ck)


def _conds(n, dim, seed=0):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)


def test_dataset_pairing_survives_a_shuffled_loader():
    from video_diffusion_nnx_amd.datasets import CondPairs, SyntheticVideo
    ds = SyntheticVideo(8, 1, 2, 4, seed=3)
    conds = _conds(8, 5)
    pairs = CondPairs(ds, conds)
    assert len(pairs) == 8
    dl = torch.utils.data.DataLoader(pairs, batch_size=4, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(1))
    rows = 0
    order = []
    for videos, cs in dl:
        assert tuple(videos.shape) == (4, 1, 2, 4, 4) and tuple(cs.shape) == (4, 5)
        for v, c in zip(videos, cs):
            i = int(np.flatnonzero((conds == c.numpy()).all(1))[0])      # the row this condition came from ...
            assert np.array_equal(v.numpy(), ds[i])                       # ... belongs to this video
            order.append(i)
            rows += 1
    assert rows == 8 and sorted(order) == list(range(8)) and order != list(range(8))
    with pytest.raises(ValueError):
        CondPairs(ds, conds[:7])


def _cpu_trainer(tmp_path, monkeypatch, cond_path, cond_dim=6, prob=0.0):
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.trainer import Trainer
    from video_diffusion_nnx_amd.unet3d import Unet3D
    monkeypatch.setattr(Trainer, 'cond_path', cond_path)
    monkeypatch.setattr(Trainer, 'null_cond_prob', prob)
    unet = Unet3D(dim=16, rngs=0, channels=1, cond_dim=cond_dim, device='cpu')
    gd = GaussianDiffusion(unet, image_size=8, num_frames=2, channels=1, timesteps=10)
    return Trainer(gd, str(tmp_path), dataset_path='synthetic:8', train_batch_size=2, train_num_steps=2, checkpoint_every_steps=100,
                   results_folder=str(tmp_path / 'res'))


def test_trainer_cond_path_checks_and_pairs(tmp_path, monkeypatch):
    from video_diffusion_nnx_amd.trainer import Trainer
    assert Trainer.cond_path is None and Trainer.null_cond_prob == 0.0   # off by default
    good, wrong_n, wrong_dim = tmp_path / 'c.npy', tmp_path / 'n.npy', tmp_path / 'd.npy'
    np.save(good, _conds(8, 6))
    np.save(wrong_n, _conds(7, 6))
    np.save(wrong_dim, _conds(8, 5))
    for bad in (wrong_n, wrong_dim):
        with pytest.raises(ValueError):
            _cpu_trainer(tmp_path, monkeypatch, str(bad))
    with pytest.raises(ValueError):
        _cpu_trainer(tmp_path, monkeypatch, str(good), prob=1.5)
    tr = _cpu_trainer(tmp_path, monkeypatch, str(good), prob=0.5)
    videos, cs = next(tr.dl)
    assert tuple(videos.shape) == (2, 1, 2, 8, 8) and tuple(cs.shape) == (2, 6) and cs.dtype == torch.float32
    conds = np.load(good)
    for v, c in zip(videos, cs):
        i = int(np.flatnonzero((conds == c.numpy()).all(1))[0])
        assert np.array_equal(v.numpy(), tr.ds.videos[i])
    # train() hands the pair on: the video as the batch, the row as cond=
    calls = []
    monkeypatch.setattr(tr, 'train_step', lambda batch, step, cond=None: calls.append((tuple(batch.shape), tuple(cond.shape))) or torch.tensor(1.0))
    monkeypatch.setattr(tr, '_save', lambda step: None)
    tr.train()
    assert calls == [((2, 1, 2, 8, 8), (2, 6))] * 2


def test_prefetcher_passes_tuples_through_on_cpu():
    from video_diffusion_nnx_amd.datasets import DevicePrefetcher
    a = [np.full((4, 3), i, np.float64) for i in range(3)]
    b = [np.full((4, 2), 10 + i, np.float32) for i in range(3)]
    out = list(DevicePrefetcher(iter(zip(a, b)), 'cpu', select=lambda t: t[1:3]))
    assert len(out) == 3
    for i, item in enumerate(out):
        assert isinstance(item, tuple) and len(item) == 2
        assert tuple(item[0].shape) == (2, 3) and tuple(item[1].shape) == (2, 2)
        assert item[0].dtype == item[1].dtype == torch.float32
        assert float(item[0][0, 0]) == i and float(item[1][0, 0]) == 10 + i
    lists = list(DevicePrefetcher(iter([[a[0], b[0]]]), 'cpu'))
    assert isinstance(lists[0], tuple) and len(lists[0]) == 2
    single = list(DevicePrefetcher(iter(a), 'cpu', select=lambda t: t[:1]))      # a single-tensor batch: a tensor, as before
    assert all(torch.is_tensor(s) and tuple(s.shape) == (1, 3) for s in single) and len(single) == 3


def test_cli_flags_parse():
    import argparse
    import sample
    import train
    a = sample.build_parser().parse_args(['--random-init', '--cond-path', 'c.npy'])
    assert a.cond_path == 'c.npy' and a.cond_scale == 2.0 and a.guidance_rescale == 0.0
    a = sample.build_parser().parse_args(['--random-init', '--cond-path', 'c.npy', '--cond-scale', '7.5', '--guidance-rescale', '0.7', '--dpm-steps', '4'])
    assert (a.cond_scale, a.guidance_rescale, a.dpm_steps) == (7.5, 0.7, 4)
    assert sample.build_parser().parse_args(['--random-init']).cond_path is None
    ap = argparse.ArgumentParser()
    for flag, kw in train.FLAGS:
        ap.add_argument(flag, **kw)
    t = ap.parse_args(['--cond_path', 'c.npy', '--null_cond_prob', '0.2'])
    assert t.cond_path == 'c.npy' and t.null_cond_prob == 0.2
    t = ap.parse_args([])
    assert t.cond_path is None and t.null_cond_prob is None


def test_sample_cli_rejects_cond_path_without_a_conditioned_config(tmp_path):
    import sample
    import yaml
    cfg = {'unet': dict(dim=16, dim_mults=[1, 2], channels=1, rngs_seed=0, use_bert_text_cond=False),
           'diffusion': dict(image_size=8, num_frames=2, channels=1, timesteps=4, loss_type='l2')}
    path = tmp_path / 'cfg.yaml'
    path.write_text(yaml.safe_dump(cfg))
    np.save(tmp_path / 'c.npy', _conds(2, 768))
    with pytest.raises(SystemExit):
        sample.main(['--config', str(path), '--random-init', '--cond-path', str(tmp_path / 'c.npy'), '--output-path', str(tmp_path / 'o')])
    with pytest.raises(SystemExit):
        sample.main(['--config', str(path), '--random-init', '--guidance-rescale', '1.5', '--output-path', str(tmp_path / 'o')])
    with pytest.raises(ValueError):
        sample.load_cond(str(tmp_path / 'c.npy'), 32)
    assert sample.load_cond(str(tmp_path / 'c.npy'), 768).shape == (2, 768)


def test_guidance_rescale_range_check():
    import inspect
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion, check_guidance_rescale
    assert check_guidance_rescale(0) == 0.0 and check_guidance_rescale(0.7) == 0.7 and check_guidance_rescale(1) == 1.0
    for bad in (-0.01, 1.01, float('nan')):
        with pytest.raises(ValueError):
            check_guidance_rescale(bad)
    for name in ('p_sample_loop', 'ddim_sample_loop', 'dpm_sample_loop', 'sample'):
        assert inspect.signature(getattr(GaussianDiffusion, name)).parameters['guidance_rescale'].default == 0.0, name
    for name in ('inpaint', 'extend'):
        assert 'guidance_rescale' not in inspect.signature(getattr(GaussianDiffusion, name)).parameters, name
    # the loops check before any device work: a CPU-only model raises the ValueError, not a GPU error
    from video_diffusion_nnx_amd.unet3d import Unet3D
    gd = GaussianDiffusion(Unet3D(dim=16, rngs=0, channels=1, cond_dim=8, device='cpu'), image_size=8, num_frames=2, channels=1, timesteps=4)
    shape = (1, 1, 2, 8, 8)
    for call in (lambda: gd.p_sample_loop(shape, 0, guidance_rescale=2.0), lambda: gd.ddim_sample_loop(shape, 0, steps=2, guidance_rescale=-1.0),
                 lambda: gd.dpm_sample_loop(shape, 0, steps=2, guidance_rescale=1.5), lambda: gd.sample(0, batch_size=1, guidance_rescale=3.0)):
        with pytest.raises(ValueError):
            call()
