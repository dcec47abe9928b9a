"""Training CLI for the MI355X path.  Accepts the reference CLI's flags (reference train.py:23-42: --config,
--resume_step, --rng_seed) and its YAML schema (unet / diffusion / trainer sections).  Keys a YAML leaves out fall back
to the Trainer defaults (the reference indexes them and raises KeyError for its own v1_0..v2_2 files).
Multi-GPU: `python -m torch.distributed.run --nproc-per-node N train.py --config ...` = one process per GPU over RCCL;
`train_batch_size` stays the GLOBAL batch and is split over ranks like the reference splits it over devices.
Extensions: --mode {bf16,f32}; --train_num_steps N; --dataset_path P (e.g. synthetic:64); --apply_grad_args (gradient accumulation and
global-norm clipping as the YAML's trainer section asks; without it both keys are ignored, as in the reference);
--frame_cond_max K [--frame_cond_uncond_prob P] [--frame_cond_mode random|prefix] (frame-conditioned training, RaMViD: up to K random
context frames per sample enter the network clean and carry no loss; sample such a model with sample.py --context ... --clean-context);
--cond_path P.npy [--null_cond_prob 0.1] (conditional training for classifier-free guidance: row i of the float32 [N, cond_dim] file is
the condition of video i; every sample's condition is replaced by the null embedding with the given probability; needs a config with
use_bert_text_cond; sample with sample.py --cond-path); --temporal_pos_bias (or unet.temporal_pos_bias: true in the YAML: the temporal
attention blocks add the relative position bias before the softmax, so the network can learn frame order; sample with
sample.py --temporal-pos-bias or the same YAML key); --focus_present [--prob_focus_present P] (or unet.focus_present: true and
trainer.prob_focus_present: P in the YAML; joint image-video training: with probability P a sample is trained as a bag of images, each
frame attending to itself only in the temporal blocks; sample.py --focus-present draws frames in that image mode);
diffusion.lowres_cond: {temporal: ft, spatial: fs, aug_max: L} in the YAML (no flag; sample.build_models reads it): the second stage of
a cascade -- the network is trained on [ x_t | the batch's own ft x fs x fs box mean, upsampled and noised to a level below L ]; sample
such a model with sample.py --lowres-path; not with --frame_cond_max or --focus_present);
--timestep_sampler {uniform,loss-second-moment} [--sampler_history H] [--sampler_uniform_prob P] (or trainer.timestep_sampler /
sampler_history / sampler_uniform_prob in the YAML; absent = uniform: Improved DDPM's loss-aware sampler -- t is drawn on the device with
probability ~ the root of the second moment of the last H losses seen at each level, mixed with P of the uniform distribution, and each
sample's loss is weighted by 1 / (T p_t); uniform until every level has H losses; the state is not checkpointed, a resumed run restarts it
cold; not with --frame_cond_max);
--frame_noise_alpha A (or diffusion.frame_noise_alpha: A in the YAML, absent = 0: train under the mixed noise prior of "Preserve Your Own
Correlation" -- the noise of a clip's frames shares a component, correlation A^2 / (1 + A^2); nothing else in the step changes; not stored
in checkpoints: sample with sample.py --frame-noise-alpha A or the same YAML key; not with learned-variance or super-resolution configs);
--objective pred_v [--min_snr_gamma 5] (or diffusion.objective / diffusion.min_snr_gamma in the YAML, absent = pred_noise, unweighted: the
network is trained to predict v = sqrt(ac) eps - sqrt(1 - ac) x0, and with gamma a sample's loss at level t is weighted with the min-SNR
weight min(SNR_t, gamma) / (SNR_t + 1) -- for pred_noise min(SNR_t, gamma) / SNR_t; not stored in checkpoints: sample with sample.py
--objective pred_v or the same YAML key; not with learned-variance configs or --frame_cond_max);
--self_condition [--self_cond_prob P] (or diffusion.self_condition: true and trainer.self_cond_prob: P in the YAML, absent = off, P = 0.5:
self-conditioning of "Analog Bits" -- the stem takes 2 * channels planes, [ x_t | the network's own clipped estimate of x0 ]; with
probability P a step first runs the network on [ x_t | 0 ], without gradient, for that estimate, otherwise it trains on [ x_t | 0 ]; not
stored in checkpoints, the stem's shape is: sample with sample.py --self-condition or the same YAML key; not with learned-variance or
super-resolution configs, --frame_noise_alpha or --frame_cond_max)."""
import argparse
import logging
import os
import pathlib

import yaml

HERE = pathlib.Path(__file__).resolve().parent
FLAGS = (
    ('--config', dict(type=str, default=str(HERE / 'configs' / 'config.yaml'), help='YAML with unet / diffusion / trainer sections')),
    ('--resume_step', dict(type=int, default=0, help='restore params + EMA of this step first (optimizer state restarts)')),
    ('--rng_seed', dict(type=int, default=None, help='master seed; default: config rng_seed, else 0')),
    ('--mode', dict(choices=('bf16', 'f16', 'f32'), default='bf16', help='MFMA operand precision')),
    ('--train_num_steps', dict(type=int, default=None, help='override trainer.train_num_steps')),
    ('--dataset_path', dict(type=str, default=None, help='override trainer.dataset_path')),
    ('--apply_grad_args', dict(action='store_true', help="honour the trainer section's gradient_accumulate_every and max_grad_norm")),
    ('--frame_cond_max', dict(type=int, default=None, help='frame-conditioned training: up to K clean context frames per sample (0 = off)')),
    ('--frame_cond_uncond_prob', dict(type=float, default=None, help='with --frame_cond_max: probability of a sample without context (0.25)')),
    ('--frame_cond_mode', dict(choices=('random', 'prefix'), default=None, help="with --frame_cond_max: any K frames, or the first K")),
    ('--temporal_pos_bias', dict(action='store_true', help='temporal attention adds the relative position bias before the softmax: the network '
                                                           'learns frame order (also unet.temporal_pos_bias in the YAML; not stored in checkpoints)')),
    ('--focus_present', dict(action='store_true', help='joint image-video training: the network honours the focus-present mask (also '
                                                       'unet.focus_present in the YAML; not stored in checkpoints)')),
    ('--prob_focus_present', dict(type=float, default=None, help='with --focus_present: probability that a sample is trained as a bag of '
                                                                 'images (also trainer.prob_focus_present in the YAML; default 0)')),
    ('--cond_path', dict(type=str, default=None, help='conditional training: float32 [N, cond_dim] .npy, row i = the condition of video i')),
    ('--null_cond_prob', dict(type=float, default=None, help='with --cond_path: probability of training a sample on the null embedding (0.1)')),
    ('--timestep_sampler', dict(choices=('uniform', 'loss-second-moment'), default=None,
                                help='how t is drawn: uniformly (default), or on the device by the second moment of the per-level loss '
                                     'history with importance weights (also trainer.timestep_sampler in the YAML)')),
    ('--sampler_history', dict(type=int, default=None, help='with loss-second-moment: losses kept per level, 1..32 (10)')),
    ('--sampler_uniform_prob', dict(type=float, default=None, help='with loss-second-moment: share of the uniform distribution, (0, 1] (0.001)')),
    ('--frame_noise_alpha', dict(type=float, default=None, help='mixed noise prior: the training noise of a clip\'s frames shares a component, '
                                                                'correlation A^2 / (1 + A^2) (overrides diffusion.frame_noise_alpha in the YAML; '
                                                                '0 = i.i.d.; not stored in checkpoints)')),
    ('--objective', dict(choices=('pred_noise', 'pred_v'), default=None, help='what the network is trained to predict (overrides '
                                                                              'diffusion.objective in the YAML; not stored in checkpoints)')),
    ('--min_snr_gamma', dict(type=float, default=None, help='min-SNR-gamma loss weighting, gamma > 0 (5 is the usual choice; overrides '
                                                            'diffusion.min_snr_gamma in the YAML; absent = unweighted)')),
    ('--self_condition', dict(action='store_true', help='self-conditioning: the network also sees its own previous estimate of x0 (also '
                                                        'diffusion.self_condition in the YAML; not stored in checkpoints)')),
    ('--self_cond_prob', dict(type=float, default=None, help='with --self_condition: probability that a step runs the first, gradient-free '
                                                             'forward (also trainer.self_cond_prob in the YAML; default 0.5)')),
)


def main(argv=None):
    logging.basicConfig(level=logging.INFO, format='%(levelname)s:%(name)s:%(message)s', force=True)
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    for flag, kw in FLAGS:
        ap.add_argument(flag, **kw)
    a = ap.parse_args(argv)

    import torch
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world > 1:
        import torch.distributed as dist
        local = int(os.environ.get('LOCAL_RANK', '0'))
        torch.cuda.set_device(local)
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        dist.init_process_group('nccl', device_id=torch.device('cuda', local))

    from sample import build_models
    from video_diffusion_nnx_amd.trainer import Trainer

    with open(a.config) as fh:
        cfg = yaml.safe_load(fh)
    seed = a.rng_seed if a.rng_seed is not None else cfg.get('rng_seed', 0)
    logging.info('config %s, master seed %s', a.config, seed)
    # (the keyword only when the flag is given: callers that replace build_models with a (cfg, mode) function keep working)
    if a.frame_noise_alpha is not None and not (0.0 <= a.frame_noise_alpha < float('inf')):
        ap.error(f'--frame_noise_alpha must be a finite number >= 0, got {a.frame_noise_alpha}')
    if a.min_snr_gamma is not None and not (0.0 < a.min_snr_gamma < float('inf')):
        ap.error(f'--min_snr_gamma must be a finite number > 0, got {a.min_snr_gamma}')
    try:
        _, gd = build_models(cfg, a.mode, **(dict(temporal_pos_bias=True) if a.temporal_pos_bias else {}),
                             **(dict(focus_present=True) if a.focus_present else {}),
                             **(dict(frame_noise_alpha=a.frame_noise_alpha) if a.frame_noise_alpha is not None else {}),
                             **(dict(objective=a.objective) if a.objective is not None else {}),
                             **(dict(min_snr_gamma=a.min_snr_gamma) if a.min_snr_gamma is not None else {}),
                             **(dict(self_condition=True) if a.self_condition else {}))
    except ValueError as e:
        if not any(w in str(e) for w in ('objective', 'min_snr_gamma', 'self_condition')):
            raise
        ap.error(str(e))
    tc = dict(cfg['trainer'])
    p_fp = tc.pop('prob_focus_present', None)        # (a Trainer attribute, not a constructor argument)
    if a.prob_focus_present is not None:
        if not (a.focus_present or cfg['unet'].get('focus_present')):
            ap.error('--prob_focus_present needs --focus_present (or unet.focus_present: true in the YAML)')
        p_fp = a.prob_focus_present
    if p_fp is not None:
        if not 0.0 <= float(p_fp) <= 1.0:
            ap.error(f'prob_focus_present must be in [0, 1], got {p_fp}')
        Trainer.prob_focus_present = float(p_fp)
    # loss-aware timestep sampling: Trainer attributes as well; absent = off
    ts_kind, ts_hist, ts_prob = tc.pop('timestep_sampler', None), tc.pop('sampler_history', None), tc.pop('sampler_uniform_prob', None)
    ts_kind = a.timestep_sampler if a.timestep_sampler is not None else ts_kind
    ts_hist = a.sampler_history if a.sampler_history is not None else ts_hist
    ts_prob = a.sampler_uniform_prob if a.sampler_uniform_prob is not None else ts_prob
    if ts_kind is not None:
        if ts_kind not in ('uniform', 'loss-second-moment'):
            ap.error(f"timestep_sampler must be 'uniform' or 'loss-second-moment', got {ts_kind!r}")
        Trainer.timestep_sampler = ts_kind
    if ts_hist is not None:
        if not 1 <= int(ts_hist) <= 32:
            ap.error(f'sampler_history must be in [1, 32], got {ts_hist}')
        Trainer.sampler_history = int(ts_hist)
    if ts_prob is not None:
        if not 0.0 < float(ts_prob) <= 1.0:
            ap.error(f'sampler_uniform_prob must be in (0, 1], got {ts_prob}')
        Trainer.sampler_uniform_prob = float(ts_prob)
    # self-conditioned training: a Trainer attribute as well; absent = 0.5, used with a self-conditioned diffusion only
    p_sc = tc.pop('self_cond_prob', None)
    if a.self_cond_prob is not None:
        if not getattr(gd, 'self_condition', False):      # (callers that replace build_models may hand no diffusion on)
            ap.error('--self_cond_prob needs --self_condition (or diffusion.self_condition: true in the YAML)')
        p_sc = a.self_cond_prob
    if p_sc is not None:
        if isinstance(p_sc, bool) or not 0.0 <= float(p_sc) <= 1.0:
            ap.error(f'self_cond_prob must be in [0, 1], got {p_sc}')
        Trainer.self_cond_prob = float(p_sc)
    if a.train_num_steps is not None:
        tc['train_num_steps'] = a.train_num_steps
    if a.dataset_path is not None:
        tc['dataset_path'] = a.dataset_path
    if a.apply_grad_args:
        Trainer.apply_grad_args = True
    if a.frame_cond_max is not None:
        frames = cfg.get('diffusion', {}).get('num_frames')
        if a.frame_cond_max < 0 or (frames is not None and a.frame_cond_max > frames - 1):
            ap.error(f'--frame_cond_max must be in [0, num_frames - 1], got {a.frame_cond_max}')
        if a.frame_cond_max > 0 and getattr(gd, 'self_condition', False):
            ap.error('self_condition does not support frame_mask yet (a follow-up; DESIGN.md 9): not with --frame_cond_max')
        Trainer.frame_cond_max = a.frame_cond_max
    if a.frame_cond_uncond_prob is not None:
        if not 0.0 <= a.frame_cond_uncond_prob <= 1.0:
            ap.error(f'--frame_cond_uncond_prob must be in [0, 1], got {a.frame_cond_uncond_prob}')
        Trainer.frame_cond_uncond_prob = a.frame_cond_uncond_prob
    if a.frame_cond_mode is not None:
        Trainer.frame_cond_mode = a.frame_cond_mode
    if a.null_cond_prob is not None and a.cond_path is None:
        ap.error('--null_cond_prob needs --cond_path')
    if a.cond_path is not None:
        if not cfg['unet'].get('use_bert_text_cond'):
            ap.error('--cond_path needs a config whose unet.use_bert_text_cond is true (a conditioned network)')
        p = 0.1 if a.null_cond_prob is None else a.null_cond_prob
        if not 0.0 <= p <= 1.0:
            ap.error(f'--null_cond_prob must be in [0, 1], got {p}')
        Trainer.cond_path, Trainer.null_cond_prob = a.cond_path, p
    tc.pop('resume_training_step', None)             # the command-line flag wins, as in the reference
    trainer = Trainer(diffusion_model=gd, folder=tc.pop('folder'), resume_training_step=a.resume_step, rng_seed=seed, **tc)
    trainer.train()
    logging.info('done')
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
