"""Sampling CLI for the MI355X path.  Accepts the reference CLI's flags (reference sample.py:19-62: --config,
--output-path, --checkpoint-path, --step, --seed, --batch-size, --load-ema-params) and its YAML schema, then runs
GaussianDiffusion.sample on the GPU and writes one GIF per video (batch-global min-max to uint8, 120 ms/frame).
Extensions: --mode {bf16,f16,f32}; --random-init (no checkpoint); --timesteps N (shorter chain for smoke runs); --ddim-steps S;
--dpm-steps S [--dpm-order 1|2] (DPM-Solver++(2M) chain; not together with --ddim-steps);
--attn-fp8 (bf16 mode: QK^T / PV of the <= 16-token attention blocks on fp8 MFMA operands);
--context PATH.npy [--context-frames K] [--extend-frames N] [--resample-steps U] (video prediction / extension from given frames);
--clean-context (with --context, for a checkpoint trained with train.py --frame_cond_max: the given frames stay un-noised at every step);
--cond-path FILE.npy [--cond-scale 2.0] [--guidance-rescale 0.0] (classifier-free guidance with ready-made embeddings: the rows of the
float32 [B, cond_dim] file are the batch; needs a config with use_bert_text_cond; works with --ddim-steps and --dpm-steps);
--lowres-path FILE.npy [--lowres-aug-level s] (the second stage of a cascade: a config with diffusion.lowres_cond upsamples the
[N,C,f,s,s] clips of the file; works with --ddim-steps and --dpm-steps); --save-npy (also write samples.npy, float32 [B,C,F,H,W] in
[0,1], beside the gifs: what a second stage reads with --lowres-path); --frame-noise-alpha A (or diffusion.frame_noise_alpha: A in the
YAML, absent = 0: the mixed noise prior of "Preserve Your Own Correlation" -- x_T and the ancestral steps' noise share a component across
the frames of a clip, correlation A^2 / (1 + A^2); for checkpoints trained with train.py --frame_noise_alpha A; works with --ddim-steps,
--dpm-steps and --cond-path, not with --context, learned-variance or super-resolution configs); --objective pred_v (or diffusion.objective:
pred_v in the YAML, absent = pred_noise: the network predicts v = sqrt(ac) eps - sqrt(1 - ac) x0; for checkpoints trained with train.py
--objective pred_v; works with every sampler and option above except learned-variance configs); --self-condition (or
diffusion.self_condition: true in the YAML, absent = off: self-conditioning of "Analog Bits" -- the stem takes 2 * channels planes and every
step of the chain feeds its clipped estimate of x0 to the next one, inside the captured step; for checkpoints trained with train.py
--self_condition; works with --ddim-steps, --dpm-steps, --objective pred_v, --focus-present and an un-guided --cond-path (--cond-scale 1),
not with --context, --lowres-path, guidance, learned-variance configs or --frame-noise-alpha)."""
import argparse
import logging
import os
import pathlib

import yaml

HERE = pathlib.Path(__file__).resolve().parent
FLAGS = (   # (flag, kwargs)
    ('--config', dict(type=str, default=str(HERE / 'configs' / 'config.yaml'), help='YAML with unet / diffusion / trainer sections')),
    ('--output-path', dict(type=str, default=str(HERE / 'outputs'), help='where the sample_<i>.gif files go')),
    ('--checkpoint-path', dict(type=str, default=None, help='checkpoint directory (required unless --random-init)')),
    ('--step', dict(type=int, default=0, help='which saved step to load')),
    ('--seed', dict(type=int, default=0, help='Philox seed of the sampling chain')),
    ('--batch-size', dict(type=int, default=2, help='videos to draw')),
    ('--load-ema-params', dict(action='store_true', help='sample from the EMA weights')),
    ('--mode', dict(choices=('bf16', 'f16', 'f32'), default='bf16', help='MFMA operand precision')),
    ('--random-init', dict(action='store_true', help='skip the checkpoint, use freshly initialised weights')),
    ('--timesteps', dict(type=int, default=None, help='override diffusion.timesteps')),
    ('--ddim-steps', dict(type=int, default=None, help='sample with an S-step DDIM chain (eta = 0) instead of the T-step ancestral one')),
    ('--dpm-steps', dict(type=int, default=None, help='sample with an S-step DPM-Solver++(2M) chain (about 20 steps do what DDIM needs 100 for); '
                                                      'not together with --ddim-steps')),
    ('--steps', dict(type=int, default=None, help='learned-variance configs (diffusion.learned_variance): sample with the respaced S-level '
                                                  'ancestral chain instead of all T levels')),
    ('--dpm-order', dict(type=int, choices=(1, 2), default=2, help='with --dpm-steps: 2 = second-order multistep, 1 = first order (= DDIM)')),
    ('--attn-fp8', dict(action='store_true', help='bf16 mode: fp8 (e4m3) QK^T / PV in the attention blocks over <= 16 tokens')),
    ('--context', dict(type=str, default=None, help='[B,C,F,H,W] .npy clip (float in [0,1], or uint8 / 255): generate its continuation '
                                                    'instead of sampling from noise; sets the batch')),
    ('--context-frames', dict(type=int, default=None, help='with --context: keep its first K frames (default: all)')),
    ('--extend-frames', dict(type=int, default=0, help='with --context: the videos get num_frames + N frames')),
    ('--resample-steps', dict(type=int, default=1, help='with --context: RePaint resampling steps per noise level (ancestral chain only)')),
    ('--temporal-pos-bias', dict(action='store_true', help='temporal attention adds the relative position bias before the softmax (frame order; '
                                                           'also unet.temporal_pos_bias in the YAML; for checkpoints trained with it)')),
    ('--focus-present', dict(action='store_true', help='"image mode" sampling from a jointly trained checkpoint (train.py --focus_present): in '
                                                       'the temporal blocks every frame attends to itself only; not with --context / --attn-fp8')),
    ('--clean-context', dict(action='store_true', help='with --context: keep the given frames clean at every step (frame-conditioned '
                                                       'checkpoints, train.py --frame_cond_max); not with --resample-steps > 1')),
    ('--cond-path', dict(type=str, default=None, help='float32 [B, cond_dim] .npy of conditions: one video per row (sets the batch); '
                                                      'classifier-free guidance, needs a config with use_bert_text_cond')),
    ('--cond-scale', dict(type=float, default=2.0, help='with --cond-path: guidance scale s in eps(0) + s (eps(c) - eps(0)); 1 = no guidance')),
    ('--guidance-rescale', dict(type=float, default=0.0, help='with --cond-path: guidance rescale phi in [0, 1] (Lin et al. 2023); 0 = off')),
    ('--lowres-path', dict(type=str, default=None, help='super-resolution configs (diffusion.lowres_cond): [N,C,f,s,s] .npy of low-resolution '
                                                        'clips (float in [0,1], or uint8 / 255) to upsample; sets the batch')),
    ('--lowres-aug-level', dict(type=int, default=None, help='with --lowres-path: noise the upsampled clips to level s before conditioning on '
                                                             'them (noise conditioning augmentation at sampling time; default: none)')),
    ('--save-npy', dict(action='store_true', help='also write samples.npy (float32 [B,C,F,H,W] in [0,1]) beside the gifs, for any sampler: '
                                                  'the input of a second stage (--lowres-path)')),
    ('--frame-noise-alpha', dict(type=float, default=None, help='mixed noise prior: the noise of a clip\'s frames shares a component, correlation '
                                                                'A^2 / (1 + A^2) (overrides diffusion.frame_noise_alpha in the YAML; 0 = i.i.d.; for '
                                                                'checkpoints trained with it; not stored in checkpoints); not with --context')),
    ('--objective', dict(choices=('pred_noise', 'pred_v'), default=None, help='what the network predicts (overrides diffusion.objective in the '
                                                                              'YAML; pred_v for checkpoints trained with it; not stored in '
                                                                              'checkpoints)')),
    ('--self-condition', dict(action='store_true', help='self-conditioning: every step feeds its estimate of x0 to the next one (also '
                                                        'diffusion.self_condition in the YAML; for checkpoints trained with it; not stored '
                                                        'in checkpoints); not with --context / --lowres-path / guidance')),
)


def build_models(cfg, mode, timesteps=None, attn_fp8=False, temporal_pos_bias=False, focus_present=False, frame_noise_alpha=None,
                 objective=None, min_snr_gamma=None, self_condition=None):
    """temporal_pos_bias: the command-line flag; the YAML's unet.temporal_pos_bias (absent = false) switches it on as well.  An architecture
    argument like dim: checkpoints do not store it, so a model trained with it is sampled with it.  focus_present: the same for the
    focus-present switch (unet.focus_present in the YAML, absent = false).  diffusion.learned_variance (absent = false; optionally with
    diffusion.vlb_weight): the UNet gets out_dim = 2 * channels (eps | v) and the diffusion the learned-variance paths; checkpoints do not
    store the switch, the final conv's shape does (load_state_dict fails loudly on a mismatch).  diffusion.lowres_cond: {temporal: ft,
    spatial: fs, aug_max: L} (absent = off): a super-resolution stage -- the UNet gets channels = 2 * channels, out_dim = channels and
    the diffusion lowres_cond=(ft, fs), lowres_aug_max=L (aug_max absent = 0); again the conv shapes are what a checkpoint stores.
    diffusion.frame_noise_alpha: A (absent = 0 = off; the keyword, the command-line flag, overrides it): the mixed noise prior of
    GaussianDiffusion(frame_noise_alpha=A) for training and sampling.  Checkpoints do not store it, and no shape depends on it: a model
    trained with it is sampled with the same A.  diffusion.objective: pred_noise | pred_v and diffusion.min_snr_gamma: gamma (absent = off; the
    keywords, the command-line flags, override them): what the network predicts and the min-SNR loss weighting of
    GaussianDiffusion(objective=..., min_snr_gamma=gamma).  Checkpoints do not store them either: a model trained to predict v is sampled
    with objective pred_v.  diffusion.self_condition: true (absent = off; the keyword, the command-line flag, switches it on as well):
    self-conditioning -- the UNet gets channels = 2 * channels, out_dim = channels, as for lowres_cond, and the diffusion
    self_condition=True.  Checkpoints do not store the switch; the stem's shape is what they store."""
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.unet3d import Rngs, Unet3D
    u, d = cfg['unet'], cfg['diffusion']
    lv = bool(d.get('learned_variance', False))
    lv_kw = dict(learned_variance=True, vlb_weight=d.get('vlb_weight')) if lv else {}
    sr = d.get('lowres_cond')
    sr_kw = dict(lowres_cond=(sr['temporal'], sr['spatial']), lowres_aug_max=sr.get('aug_max', 0)) if sr else {}
    fa = d.get('frame_noise_alpha', 0) if frame_noise_alpha is None else frame_noise_alpha
    fa_kw = dict(frame_noise_alpha=fa) if (fa or isinstance(fa, bool)) else {}       # (0 takes the constructor's default: nothing new is passed)
    ob = d.get('objective') if objective is None else objective
    mg = d.get('min_snr_gamma') if min_snr_gamma is None else min_snr_gamma
    ob_kw = dict(**(dict(objective=ob) if ob is not None else {}), **(dict(min_snr_gamma=mg) if mg is not None else {}))
    sc = d.get('self_condition', False) if self_condition is None else self_condition
    sc_kw = dict(self_condition=sc) if (sc or not isinstance(sc, bool)) else {}       # (False takes the constructor's default)
    wide = bool(sr) or sc is True                                                      # the stem of [ x_t | u ] or [ x_t | x0~ ]
    unet = Unet3D(**(dict(out_dim=2 * u['channels']) if lv else dict(out_dim=u['channels']) if wide else {}), dim=u['dim'], rngs=Rngs(u['rngs_seed']),
                  dim_mults=tuple(u['dim_mults']), channels=(2 if wide else 1) * u['channels'],
                  use_bert_text_cond=u['use_bert_text_cond'], mode=mode, attn_fp8=attn_fp8,
                  temporal_pos_bias=bool(temporal_pos_bias or u.get('temporal_pos_bias', False)),
                  focus_present=bool(focus_present or u.get('focus_present', False)))
    gd = GaussianDiffusion(denoise_fn=unet, image_size=d['image_size'], num_frames=d['num_frames'], channels=d['channels'],
                           timesteps=timesteps or d['timesteps'], loss_type=d['loss_type'], **lv_kw, **sr_kw, **fa_kw, **ob_kw, **sc_kw)
    return unet, gd


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    for flag, kw in FLAGS:
        ap.add_argument(flag, **kw)
    return ap


def load_context(path, num_frames, context_frames=None, extend_frames=0):
    """--context: (the first K frames of the clip as float32 [B,C,K,H,W] in [0,1], frames to generate = num_frames + N - K)."""
    import numpy as np
    v = np.load(path)
    if v.ndim != 5:
        raise ValueError(f'--context must hold a [B,C,F,H,W] array, got shape {v.shape}')
    v = v.astype(np.float32) / 255.0 if v.dtype == np.uint8 else v.astype(np.float32)
    k = v.shape[2] if context_frames is None else int(context_frames)
    total = num_frames + int(extend_frames)
    if not 1 <= k <= v.shape[2] or k >= total:
        raise ValueError(f'--context-frames must be in [1, {min(v.shape[2], total - 1)}], got {k}')
    return np.ascontiguousarray(v[:, :, :k]), total - k


def load_lowres(path, shape):
    """--lowres-path: the clips to upsample as float32 [N, *shape] in [0,1] (shape = (C, F/ft, S/fs, S/fs) of the config)."""
    import numpy as np
    v = np.load(path)
    if v.ndim != 5 or v.shape[0] < 1 or tuple(v.shape[1:]) != tuple(shape):
        raise ValueError(f'--lowres-path must hold a [N, {", ".join(str(n) for n in shape)}] array, got shape {v.shape}')
    v = v.astype(np.float32) / 255.0 if v.dtype == np.uint8 else v.astype(np.float32)
    return np.ascontiguousarray(v)


def load_cond(path, cond_dim):
    """--cond-path: the float32 [B, cond_dim] conditions of the batch."""
    import numpy as np
    c = np.load(path)
    if c.ndim != 2 or c.shape[0] < 1 or c.shape[1] != cond_dim:
        raise ValueError(f'--cond-path must hold a [B, {cond_dim}] array, got shape {c.shape}')
    return np.ascontiguousarray(c, dtype=np.float32)


def main(argv=None):
    logging.basicConfig(level=logging.INFO, force=True)
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.checkpoint_path is None and not a.random_init:
        ap.error('--checkpoint-path is required (or pass --random-init)')
    if a.dpm_steps is not None and a.ddim_steps is not None:
        ap.error('--dpm-steps and --ddim-steps are two samplers: give one of them')

    if a.steps is not None and (a.dpm_steps is not None or a.ddim_steps is not None or a.context or a.cond_path):
        ap.error('--steps is the respaced learned-variance chain: not with --ddim-steps / --dpm-steps / --context / --cond-path')
    if a.cond_path and a.context:
        ap.error('--cond-path samples from noise: not together with --context')
    if a.lowres_path and (a.context or a.cond_path or a.steps is not None or a.focus_present):
        ap.error('--lowres-path upsamples given clips: not together with --context / --cond-path / --steps / --focus-present')
    if a.lowres_aug_level is not None and not a.lowres_path:
        ap.error('--lowres-aug-level needs --lowres-path')
    if not 0.0 <= a.guidance_rescale <= 1.0:
        ap.error(f'--guidance-rescale must be in [0, 1], got {a.guidance_rescale}')
    if a.frame_noise_alpha is not None and not (0.0 <= a.frame_noise_alpha < float('inf')):
        ap.error(f'--frame-noise-alpha must be a finite number >= 0, got {a.frame_noise_alpha}')
    if a.frame_noise_alpha and a.context:
        ap.error('--frame-noise-alpha samples from noise: not together with --context (frame-conditioned sampling under the mixed prior is a '
                 'follow-up)')
    if a.self_condition and (a.context or a.lowres_path or a.steps is not None):
        ap.error('--self-condition runs the plain chains: not together with --context / --lowres-path / --steps')
    if a.clean_context and not a.context:
        ap.error('--clean-context needs --context')
    if a.clean_context and a.resample_steps > 1:
        ap.error('--clean-context keeps the given frames un-noised: not with --resample-steps > 1')

    # one process per GPU under `python -m torch.distributed.run --nproc-per-node N sample.py ...` (reference gaussian_diffusion.py:278-298
    # shards the batch over the local devices): every rank draws batch_size / N of the videos and writes its own GIFs
    world, rank = int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('RANK', '0'))
    if world > 1:
        import torch
        import torch.distributed as dist
        if not dist.is_initialized():
            local = int(os.environ.get('LOCAL_RANK', '0'))
            os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
            torch.cuda.set_device(local)
            dist.init_process_group('nccl', device_id=torch.device('cuda', local))
    try:
        _run(a, ap, rank, world)
    finally:
        if world > 1:
            import torch.distributed as dist
            if dist.is_initialized() and os.environ.get('VDX_KEEP_PROCESS_GROUP') != '1':
                dist.destroy_process_group()


def _run(a, ap, rank, world):
    from video_diffusion_nnx_amd.checkpoint import load_checkpoint
    from video_diffusion_nnx_amd.media import video_array_to_gif, videos_to_uint8

    out_dir = pathlib.Path(a.output_path)
    out_dir.mkdir(parents=True, exist_ok=True)
    with open(a.config) as fh:
        cfg = yaml.safe_load(fh)
    logging.info('config %s', a.config)
    if a.cond_path and not cfg['unet'].get('use_bert_text_cond'):
        ap.error('--cond-path needs a config whose unet.use_bert_text_cond is true (a conditioned network)')
    if a.attn_fp8 and (a.temporal_pos_bias or cfg['unet'].get('temporal_pos_bias')):
        ap.error('--attn-fp8 and the temporal position bias exclude each other')
    if a.focus_present and a.attn_fp8:
        ap.error('--attn-fp8 and --focus-present exclude each other')
    if a.focus_present and a.context:
        ap.error('--focus-present samples from noise: not together with --context')
    try:
        unet, gd = build_models(cfg, a.mode, a.timesteps, attn_fp8=a.attn_fp8, temporal_pos_bias=a.temporal_pos_bias,
                                **(dict(focus_present=True) if a.focus_present else {}),
                                **(dict(frame_noise_alpha=a.frame_noise_alpha) if a.frame_noise_alpha is not None else {}),
                                **(dict(objective=a.objective) if a.objective is not None else {}),
                                **(dict(self_condition=True) if a.self_condition else {}))
    except ValueError as e:
        if not any(w in str(e) for w in ('frame_noise_alpha', 'objective', 'min_snr_gamma', 'self_condition')):
            raise
        ap.error(str(e))
    if gd.frame_noise_alpha and a.context:
        ap.error('diffusion.frame_noise_alpha samples from noise: not together with --context (frame-conditioned sampling under the mixed '
                 'prior is a follow-up)')
    if gd.self_condition and (a.context or a.lowres_path or (a.cond_path and a.cond_scale != 1.0)):
        ap.error('self_condition does not support inpaint / extend / upsample / cond_scale yet (a follow-up; DESIGN.md 9): not with '
                 '--context, --lowres-path or --cond-scale other than 1')
    fp_kw = dict(focus_present=True) if a.focus_present else {}
    if a.steps is not None:
        if not gd.learned_variance:
            ap.error('--steps needs a config with diffusion.learned_variance: true')
        fp_kw['steps'] = a.steps
    if bool(a.lowres_path) != (gd.lowres_cond is not None):
        ap.error('--lowres-path and a config with diffusion.lowres_cond go together: a super-resolution model needs the clips to upsample, '
                 'any other model takes none')
    if world > 1 and a.lowres_path:
        ap.error('--lowres-path runs in a single process')
    if not a.random_init:
        ckpt = pathlib.Path(a.checkpoint_path).resolve()
        gd, _ = load_checkpoint(gd, a.step, str(ckpt), load_ema_params=a.load_ema_params)
        logging.info('restored step %d from %s', a.step, ckpt)
    if a.lowres_path:
        import torch
        ft, fs = gd.lowres_cond
        try:
            lowres = load_lowres(a.lowres_path, (gd.channels, gd.num_frames // ft, gd.image_size // fs, gd.image_size // fs))
            videos = gd.sample(a.seed, lowres=torch.from_numpy(lowres), lowres_aug_level=a.lowres_aug_level, ddim_steps=a.ddim_steps,
                               dpm_steps=a.dpm_steps, dpm_order=a.dpm_order)
        except ValueError as e:
            ap.error(str(e))
    elif a.context:
        import torch
        try:
            ctx, n_new = load_context(a.context, gd.num_frames, a.context_frames, a.extend_frames)
        except ValueError as e:
            ap.error(str(e))
        # the first window conditions on every kept frame (up to num_frames - 1), later windows on at least num_frames // 2
        window_ctx = min(max(ctx.shape[2], gd.num_frames // 2), gd.num_frames - 1)
        videos = gd.extend(a.seed, torch.from_numpy(ctx), n_new, context_frames=window_ctx, ddim_steps=a.ddim_steps,
                           resample_steps=a.resample_steps, dpm_steps=a.dpm_steps, dpm_order=a.dpm_order,
                           clean_context=a.clean_context)               # this rank's shard of the global batch
    elif a.cond_path:
        import torch
        try:
            cond = load_cond(a.cond_path, unet.cond_dim)
        except ValueError as e:
            ap.error(str(e))
        videos = gd.sample(a.seed, cond=torch.from_numpy(cond), cond_scale=a.cond_scale, ddim_steps=a.ddim_steps, dpm_steps=a.dpm_steps,
                           dpm_order=a.dpm_order, guidance_rescale=a.guidance_rescale, **fp_kw)      # this rank's shard of the global batch
    else:
        videos = gd.sample(a.seed, batch_size=a.batch_size, ddim_steps=a.ddim_steps, dpm_steps=a.dpm_steps,
                           dpm_order=a.dpm_order, **fp_kw)              # this rank's shard of the global batch
    logging.info('rank %d drew %d videos', rank, len(videos))
    lo_hi = None
    if world > 1:                                      # the uint8 scaling is batch-GLOBAL (reference sample.py:107-110): two scalars cross ranks
        import torch
        import torch.distributed as dist
        mm = torch.stack([videos.min(), -videos.max()])
        dist.all_reduce(mm, op=dist.ReduceOp.MIN)
        lo_hi = (float(mm[0].item()), float(-mm[1].item()))
    first = rank * len(videos)
    if a.save_npy:
        import numpy as np
        target = out_dir / ('samples.npy' if world == 1 else f'samples_rank{rank}.npy')
        np.save(target, videos.cpu().numpy().astype(np.float32))
        logging.info('wrote %s', target)
    for i, frames in enumerate(videos_to_uint8(videos.cpu().numpy(), lo_hi=lo_hi)):
        target = out_dir / f'sample_{first + i}.gif'
        video_array_to_gif(frames, target)
        logging.info('wrote %s', target)


if __name__ == '__main__':
    main()
