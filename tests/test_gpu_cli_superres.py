"""End-to-end CLI run of a two-stage cascade on the GPU: train.py two steps of a super-resolution stage (diffusion.lowres_cond in the YAML) on
synthetic data, sample.py --save-npy from a tiny base configuration, then sample.py --lowres-path on the base samples with the trained
second stage.  Tiny shapes; artefacts only -- the numbers are held in tests/test_gpu_superres.py."""
import json
import pathlib
import sys

import numpy as np
import pytest
import yaml

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

pytestmark = pytest.mark.gpu


def tiny_cfg(tmp, image_size, num_frames, **diffusion):
    return {
        'rng_seed': 3,
        'unet': dict(dim=16, dim_mults=[1, 2], channels=1, rngs_seed=0, use_bert_text_cond=False),
        'diffusion': dict(image_size=image_size, num_frames=num_frames, channels=1, timesteps=6, loss_type='l2', **diffusion),
        'trainer': dict(folder=str(tmp / 'res'), dataset_path='synthetic:8', num_frames=num_frames, train_batch_size=2, train_lr=1e-3,
                        train_num_steps=2, gradient_accumulate_every=1, step_start_ema=1, update_ema_every=1,
                        save_and_sample_every=100, checkpoint_every_steps=1, results_folder=str(tmp / 'res'),
                        checkpoint_dir_path=str(tmp / 'ckpt'), tensorboard_dir=str(tmp / 'tb'), max_to_keep=5,
                        add_loss_plot=False, lr_decay_start_step=10, lr_decay_steps=10, lr_decay_coeff=0.1,
                        max_grad_norm=1e7, num_sample_rows=1, cond_scale=2.0, sample_text=None, use_path_as_cond=False,
                        resume_training_step=0),
    }


def test_train_base_sample_upsample(tmp_path):
    import sample
    import train
    sr_path, base_path = tmp_path / 'sr.yaml', tmp_path / 'base.yaml'
    sr_path.write_text(yaml.safe_dump(tiny_cfg(tmp_path, 16, 4, lowres_cond=dict(temporal=2, spatial=2, aug_max=3))))
    base_path.write_text(yaml.safe_dump(tiny_cfg(tmp_path / 'base', 8, 2)))
    # stage 2 trains on its own box-mean pairs
    train.main(['--config', str(sr_path), '--mode', 'f32'])
    assert sorted(p.name for p in (tmp_path / 'ckpt').iterdir()), 'no checkpoint written'
    scalars = [json.loads(l) for l in (tmp_path / 'tb' / 'scalars_rank0.jsonl').read_text().splitlines()]
    losses = [s['value'] for s in scalars if s['tag'] == 'loss/train']
    assert len(losses) == 2 and all(np.isfinite(v) and v > 0 for v in losses)
    # stage 1 writes its samples as an array
    base_out = tmp_path / 'base_gifs'
    sample.main(['--config', str(base_path), '--random-init', '--mode', 'f32', '--batch-size', '2', '--seed', '1', '--output-path', str(base_out),
                 '--save-npy'])
    lo = np.load(base_out / 'samples.npy')
    assert lo.dtype == np.float32 and lo.shape == (2, 1, 2, 8, 8) and lo.min() >= 0.0 and lo.max() <= 1.0
    assert len(list(base_out.glob('sample_*.gif'))) == 2
    # stage 2 upsamples them
    out = tmp_path / 'gifs'
    common = ['--config', str(sr_path), '--checkpoint-path', str(tmp_path / 'ckpt'), '--step', '1', '--mode', 'f32', '--seed', '2']
    sample.main(common + ['--lowres-path', str(base_out / 'samples.npy'), '--lowres-aug-level', '1', '--output-path', str(out), '--save-npy'])
    vid = np.load(out / 'samples.npy')
    assert vid.dtype == np.float32 and vid.shape == (2, 1, 4, 16, 16) and np.isfinite(vid).all() and vid.min() >= 0.0 and vid.max() <= 1.0
    gifs = sorted(out.glob('sample_*.gif'))
    assert len(gifs) == 2 and all(g.stat().st_size > 100 for g in gifs)
    # the short samplers serve the second stage too
    sample.main(common + ['--lowres-path', str(base_out / 'samples.npy'), '--dpm-steps', '3', '--output-path', str(tmp_path / 'dpm')])
    assert len(list((tmp_path / 'dpm').glob('sample_*.gif'))) == 2
    # a super-resolution config without clips, and clips for a plain config, exit by name
    with pytest.raises(SystemExit):
        sample.main(common + ['--batch-size', '1', '--output-path', str(tmp_path / 'bad')])
    with pytest.raises(SystemExit):
        sample.main(['--config', str(base_path), '--random-init', '--mode', 'f32', '--lowres-path', str(base_out / 'samples.npy'),
                     '--output-path', str(tmp_path / 'bad')])
