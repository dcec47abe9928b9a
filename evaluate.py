"""Held-out evaluation CLI: the variational bound of a checkpoint on data it has not seen, in bits per dimension, with the per-level
curves (GaussianDiffusion.calc_bpd_loop; an extension, the reference has no evaluation).  Takes sample.py's model flags (--config,
--checkpoint-path, --step, --load-ema-params, --random-init, --mode, --timesteps, --temporal-pos-bias, --focus-present) and
--dataset-path FILE.npy | synthetic:N  (a MovingMNIST array as the trainer reads it, or N seeded uniform videos),
--data-scale S  (the loader keeps raw values, as the reference does: give 0.00392156862 for 0..255 data; the bound is defined on [0, 1]),
--num-videos N, --batch-size B, --seed, --eval-steps S (S evenly spaced levels instead of all T: the per-level curves only, no total),
--no-clip, --cond-path FILE.npy (float32 [N, cond_dim], row i the condition of video i), --output FILE.json.
Writes one JSON document: total_bpd and prior_bpd (means over the videos; total_bpd is null with --eval-steps below T), the length-S
arrays t, vb, mse and xstart_mse (means over the videos), num_videos, mode and seed.  One process: the evaluation is not sharded.
A config with diffusion.frame_noise_alpha > 0 (the mixed noise prior) is refused: the bound under a frame-correlated prior is a follow-up.
A config with diffusion.self_condition: true (self-conditioning) is refused by name as well: the bound has no form for it yet.
A config with diffusion.objective: pred_v evaluates a v-predicting network: the loop converts its output to eps_hat behind every forward."""
import argparse
import json
import logging
import os
import pathlib

import yaml

import sample

FLAGS = tuple((f, kw) for f, kw in sample.FLAGS
              if f in ('--config', '--checkpoint-path', '--step', '--load-ema-params', '--mode', '--random-init', '--timesteps',
                       '--temporal-pos-bias')) + (
    ('--seed', dict(type=int, default=0, help='Philox seed of the noise draws (step k of every batch uses draw 1 + k)')),
    ('--batch-size', dict(type=int, default=2, help='videos per pass')),
    ('--dataset-path', dict(type=str, required=True, help='MovingMNIST .npy, or synthetic:N')),
    ('--data-scale', dict(type=float, default=1.0, help='factor that takes the stored values to [0, 1] (0.00392156862 for 0..255 data)')),
    ('--num-videos', dict(type=int, default=None, help='evaluate the first N videos (default: all)')),
    ('--eval-steps', dict(type=int, default=None, help='S evenly spaced noise levels instead of all T (curves only, no total)')),
    ('--no-clip', dict(action='store_true', help='do not clamp the predicted x0 to [-1, 1]')),
    ('--cond-path', dict(type=str, default=None, help='float32 [N, cond_dim] .npy, row i = the condition of video i (used un-masked)')),
    ('--focus-present', dict(action='store_true', help='evaluate a jointly trained checkpoint in "image mode"')),
    ('--output', dict(type=str, required=True, help='the .json file to write')),
)


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    for flag, kw in FLAGS:
        ap.add_argument(flag, **kw)
    return ap


def parse_args(argv=None):
    """The parsed flags, with the rules that need no file checked (argparse's error: SystemExit)."""
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.checkpoint_path is None and not a.random_init:
        ap.error('--checkpoint-path is required (or pass --random-init)')
    if a.eval_steps is not None and a.eval_steps < 1:
        ap.error(f'--eval-steps must be >= 1, got {a.eval_steps}')
    if a.batch_size < 1 or (a.num_videos is not None and a.num_videos < 1):
        ap.error('--batch-size and --num-videos must be >= 1')
    if not a.output.endswith('.json'):
        ap.error('--output must be a .json file')
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        ap.error('evaluate.py runs as a single process (the evaluation is not sharded over ranks)')
    return ap, a


def load_videos(path, channels, num_frames, image_size, num_videos=None):
    """--dataset-path -> (a dataset of (channels, num_frames, image_size, image_size) float32 items, the number of them to evaluate);
    ValueError when there is none or the items have another shape."""
    from video_diffusion_nnx_amd.datasets import MovingMNIST, SyntheticVideo
    if path.startswith('synthetic:'):
        ds = SyntheticVideo(int(path.split(':', 1)[1]), channels, num_frames, image_size)
    else:
        ds = MovingMNIST(path, image_size, channels=channels, num_frames=num_frames)
    n = len(ds) if num_videos is None else min(int(num_videos), len(ds))
    if n < 1:
        raise ValueError(f'{path}: no videos')
    want, got = (channels, num_frames, image_size, image_size), tuple(ds[0].shape)      # (the loader neither resizes nor adds channels)
    if got != want:
        raise ValueError(f'{path}: items are {got}, the config asks for {want} (channels, num_frames, image_size, image_size)')
    return ds, n


def main(argv=None):
    logging.basicConfig(level=logging.INFO, force=True)
    ap, a = parse_args(argv)
    import numpy as np
    import torch
    from video_diffusion_nnx_amd.checkpoint import load_checkpoint

    with open(a.config) as fh:
        cfg = yaml.safe_load(fh)
    if a.cond_path and not cfg['unet'].get('use_bert_text_cond'):
        ap.error('--cond-path needs a config whose unet.use_bert_text_cond is true (a conditioned network)')
    unet, gd = sample.build_models(cfg, a.mode, a.timesteps, temporal_pos_bias=a.temporal_pos_bias,
                                   **(dict(focus_present=True) if a.focus_present else {}))
    if gd.frame_noise_alpha:
        ap.error('frame_noise_alpha does not support calc_bpd_loop yet (a follow-up; DESIGN.md 9): the bound of a model trained under the mixed '
                 'noise prior needs the inverse frame covariance in its KL terms')
    if gd.self_condition:
        ap.error('self_condition does not support calc_bpd_loop yet (a follow-up; DESIGN.md 9): the bound of a chain that feeds on its own '
                 'estimates is not defined here')
    if a.eval_steps is not None and a.eval_steps > gd.num_timesteps:
        ap.error(f'--eval-steps must be in [1, {gd.num_timesteps}], got {a.eval_steps}')
    if not a.random_init:
        ckpt = pathlib.Path(a.checkpoint_path).resolve()
        gd, _ = load_checkpoint(gd, a.step, str(ckpt), load_ema_params=a.load_ema_params)
        logging.info('restored step %d from %s', a.step, ckpt)
    try:
        ds, n = load_videos(a.dataset_path, gd.channels, gd.num_frames, gd.image_size, a.num_videos)
        conds = sample.load_cond(a.cond_path, unet.cond_dim) if a.cond_path else None
        if conds is not None and conds.shape[0] < n:
            raise ValueError(f'--cond-path holds {conds.shape[0]} rows for {n} videos')
    except ValueError as e:
        ap.error(str(e))
    sums, prior, total = None, 0.0, 0.0
    for first in range(0, n, a.batch_size):
        idx = range(first, min(first + a.batch_size, n))
        x = torch.from_numpy(np.stack([np.asarray(ds[i], dtype=np.float32) for i in idx]) * np.float32(a.data_scale))
        cond = None if conds is None else torch.from_numpy(conds[idx.start:idx.stop])
        r = gd.calc_bpd_loop(x, a.seed, cond=cond, clip_denoised=not a.no_clip, timesteps=a.eval_steps,
                             **(dict(focus_present=True) if a.focus_present else {}))
        part = torch.stack([r['vb'].sum(0), r['mse'].sum(0), r['xstart_mse'].sum(0)])
        sums = part if sums is None else sums + part
        prior += float(r['prior_bpd'].sum())
        total = None if r['total_bpd'] is None else total + float(r['total_bpd'].sum())
        t = r['t']
        logging.info('videos %d..%d of %d', idx.start, idx.stop - 1, n)
    doc = dict(total_bpd=None if total is None else total / n, prior_bpd=prior / n, t=t.tolist(), vb=(sums[0] / n).tolist(),
               mse=(sums[1] / n).tolist(), xstart_mse=(sums[2] / n).tolist(), num_videos=n, mode=a.mode, seed=a.seed)
    out = pathlib.Path(a.output)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(doc, indent=1) + '\n')
    logging.info('wrote %s', out)
    return doc


if __name__ == '__main__':
    main()
