"""End-to-end CLI run on the GPU with self-conditioning switched on by the flags: train.py --self_condition two steps on synthetic
data, then sample.py --self-condition --ddim-steps 3 from the checkpoint (--save-npy: the samples are finite and in [0, 1]).  Each tool
runs as a fresh child process under its own time limit, and the sequence stops at the first non-zero status.  Tiny shapes; artefacts
only -- the numbers are held in tests/test_gpu_selfcond.py.  The configuration of tests/test_gpu_cli_vpred.py with the other switch on."""
import json
import pathlib
import subprocess
import sys

import numpy as np
import pytest
import yaml

ROOT = pathlib.Path(__file__).resolve().parents[1]

pytestmark = pytest.mark.gpu


def tiny_cfg(tmp):
    return {
        'rng_seed': 3,
        'unet': dict(dim=16, dim_mults=[1, 2], channels=1, rngs_seed=0, use_bert_text_cond=False),
        'diffusion': dict(image_size=16, num_frames=4, channels=1, timesteps=6, loss_type='l2'),
        'trainer': dict(folder=str(tmp / 'res'), dataset_path='synthetic:8', num_frames=4, train_batch_size=2, train_lr=1e-3,
                        train_num_steps=2, gradient_accumulate_every=1, step_start_ema=1, update_ema_every=1,
                        save_and_sample_every=100, checkpoint_every_steps=1, results_folder=str(tmp / 'res'),
                        checkpoint_dir_path=str(tmp / 'ckpt'), tensorboard_dir=str(tmp / 'tb'), max_to_keep=5,
                        add_loss_plot=False, lr_decay_start_step=10, lr_decay_steps=10, lr_decay_coeff=0.1,
                        max_grad_norm=1e7, num_sample_rows=1, cond_scale=2.0, sample_text=None, use_path_as_cond=False,
                        resume_training_step=0),
    }


def _tool(name, *args, limit=120):
    """One tool as a fresh child process; its status must be 0."""
    done = subprocess.run([sys.executable, str(ROOT / name), *args], cwd=str(ROOT), timeout=limit, capture_output=True, text=True)
    assert done.returncode == 0, f'{name} exited with {done.returncode}:\n{done.stdout[-2000:]}\n{done.stderr[-4000:]}'
    return done


def test_train_then_sample(tmp_path):
    cfg_path = tmp_path / 'cfg.yaml'
    cfg_path.write_text(yaml.safe_dump(tiny_cfg(tmp_path)))
    _tool('train.py', '--config', str(cfg_path), '--mode', 'f32', '--self_condition', '--self_cond_prob', '1.0')
    assert sorted(p.name for p in (tmp_path / 'ckpt').iterdir()), 'no checkpoint written'
    scalars = [json.loads(l) for l in (tmp_path / 'tb' / 'scalars_rank0.jsonl').read_text().splitlines()]
    losses = [s['value'] for s in scalars if s['tag'] == 'loss/train']
    assert len(losses) == 2 and all(np.isfinite(v) and v > 0 for v in losses)
    out = tmp_path / 'gifs'
    _tool('sample.py', '--config', str(cfg_path), '--checkpoint-path', str(tmp_path / 'ckpt'), '--step', '1', '--mode', 'f32', '--batch-size', '2',
          '--seed', '1', '--output-path', str(out), '--self-condition', '--ddim-steps', '3', '--save-npy')
    gifs = sorted(out.glob('sample_*.gif'))
    assert len(gifs) == 2 and all(g.stat().st_size > 100 for g in gifs)
    videos = np.load(out / 'samples.npy')
    assert videos.shape == (2, 1, 4, 16, 16) and np.isfinite(videos).all() and videos.min() >= 0.0 and videos.max() <= 1.0
