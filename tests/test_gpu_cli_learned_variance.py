"""End-to-end CLI run on the GPU with a learned-variance YAML (diffusion.learned_variance: true): train.py a few steps on synthetic data,
sample.py --steps 4 from the checkpoint, evaluate.py on the same config.  Tiny shapes; artefacts only -- the numbers are held in
tests/test_gpu_learned_variance.py.  The configuration of tests/test_gpu_cli.py with the switch on."""
import json
import pathlib
import sys

import numpy as np
import pytest
import yaml

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

pytestmark = pytest.mark.gpu


def tiny_cfg(tmp):
    return {
        'rng_seed': 3,
        'unet': dict(dim=16, dim_mults=[1, 2], channels=1, rngs_seed=0, use_bert_text_cond=False),
        'diffusion': dict(image_size=16, num_frames=4, channels=1, timesteps=6, loss_type='l2', learned_variance=True, vlb_weight=0.05),
        'trainer': dict(folder=str(tmp / 'res'), dataset_path='synthetic:8', num_frames=4, train_batch_size=2, train_lr=1e-3,
                        train_num_steps=3, gradient_accumulate_every=2, step_start_ema=1, update_ema_every=1,
                        save_and_sample_every=100, checkpoint_every_steps=2, results_folder=str(tmp / 'res'),
                        checkpoint_dir_path=str(tmp / 'ckpt'), tensorboard_dir=str(tmp / 'tb'), max_to_keep=5,
                        add_loss_plot=False, lr_decay_start_step=10, lr_decay_steps=10, lr_decay_coeff=0.1,
                        max_grad_norm=1e7, num_sample_rows=1, cond_scale=2.0, sample_text=None, use_path_as_cond=False,
                        resume_training_step=0),
    }


def test_train_sample_evaluate(tmp_path):
    import evaluate
    import sample
    import train
    cfg = tiny_cfg(tmp_path)
    cfg_path = tmp_path / 'cfg.yaml'
    cfg_path.write_text(yaml.safe_dump(cfg))
    train.main(['--config', str(cfg_path), '--mode', 'f32'])
    assert sorted(p.name for p in (tmp_path / 'ckpt').iterdir()), 'no checkpoint written'
    scalars = [json.loads(l) for l in (tmp_path / 'tb' / 'scalars_rank0.jsonl').read_text().splitlines()]
    losses = [s['value'] for s in scalars if s['tag'] == 'loss/train']
    # (6 levels: beta of the last one is 0.9999, and an untrained v puts hundreds of bits on its KL -- finite and positive is the check)
    assert len(losses) == 3 and all(np.isfinite(v) and v > 0 for v in losses)
    out = tmp_path / 'gifs'
    common = ['--config', str(cfg_path), '--checkpoint-path', str(tmp_path / 'ckpt'), '--step', '2', '--mode', 'f32']
    sample.main(common + ['--batch-size', '2', '--seed', '1', '--output-path', str(out), '--steps', '4', '--load-ema-params'])
    gifs = sorted(out.glob('sample_*.gif'))
    assert len(gifs) == 2 and all(g.stat().st_size > 100 for g in gifs)
    sample.main(common + ['--batch-size', '1', '--seed', '1', '--output-path', str(tmp_path / 'full')])            # all T levels
    assert len(list((tmp_path / 'full').glob('sample_*.gif'))) == 1
    res = tmp_path / 'bpd.json'
    evaluate.main(common + ['--dataset-path', 'synthetic:2', '--output', str(res)])
    doc = json.loads(res.read_text())
    assert np.isfinite(doc['total_bpd']) and len(doc['t']) == 6
    assert abs(doc['total_bpd'] - (doc['prior_bpd'] + sum(doc['vb']))) < 1e-9 * abs(doc['total_bpd'])
    # the switch is not in the checkpoint: the final conv's shape is, and a config without the switch fails loudly on it
    cfg['diffusion'].pop('learned_variance')
    cfg['diffusion'].pop('vlb_weight')
    (tmp_path / 'plain.yaml').write_text(yaml.safe_dump(cfg))
    with pytest.raises(Exception, match='final_conv|shape|size'):
        sample.main(['--config', str(tmp_path / 'plain.yaml'), '--checkpoint-path', str(tmp_path / 'ckpt'), '--step', '2', '--mode', 'f32',
                     '--batch-size', '1', '--output-path', str(tmp_path / 'bad')])
    # sampler switches the learned-variance chain does not serve are refused by name
    with pytest.raises(ValueError, match='learned_variance does not support ddim_steps'):
        sample.main(common + ['--batch-size', '1', '--output-path', str(tmp_path / 'bad'), '--ddim-steps', '3'])
