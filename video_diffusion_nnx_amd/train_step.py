"""The device side of one train step (reference `_pjit_train_step`, trainer.py:322-392), driven stage by stage so the
gradient all-reduce of finished buckets overlaps the rest of the backward.  Two parts: forward + loss + backward of one micro-batch
(`forward_backward`) and the optimizer tail (`optimizer_tail`); `run_train_step` is one of each, `run_train_step_accum` (behind
Trainer.apply_grad_args) K micro-batches and one tail with optional global-norm clipping."""
from __future__ import annotations

import collections
import ctypes as C

import torch

from . import _lib as L
from .gaussian_diffusion import _stage, frame_mask as expand_frame_mask, split_key
from .gaussian_diffusion import self_cond_draw, self_cond_key as _loss_self_cond_key  # noqa: F401  (self_cond_draw: the coin, re-exported)
# (bound next to the objective now; tests and tools import these three from here)
from .gaussian_diffusion import vdx_loss_grad, vdx_loss_grad_masked, vdx_loss_sum  # noqa: F401

_vp = C.c_void_p
vdx_adam_ema_step = L._sig('vdx_adam_ema_step', C.c_int, [_vp] * 5 + [C.c_long] + [C.c_float] * 4 + [C.c_long, C.c_float, C.c_int, C.c_float, _vp])
vdx_grad_accumulate = L._sig('vdx_grad_accumulate', C.c_int, [_vp, _vp, C.c_long, _vp])
vdx_grad_sqnorm_scratch_doubles = L._sig('vdx_grad_sqnorm_scratch_doubles', C.c_size_t, [])
vdx_grad_sqnorm = L._sig('vdx_grad_sqnorm', C.c_int, [_vp, C.c_long, _vp, _vp, _vp])
vdx_adam_ema_step_clip = L._sig('vdx_adam_ema_step_clip', C.c_int, [_vp] * 5 + [C.c_long] + [C.c_float] * 4 + [C.c_long, C.c_float, C.c_int, C.c_float,
                                                                    _vp, C.c_float, _vp, _vp])
FLT_MAX = 3.4028234663852886e+38


def stage_of_param(name: str, n_levels: int) -> int:
    """Backward stage (== forward position) of a parameter: 0 = stem + time MLP, 1..n = downs, n+1 = mid,
    n+2..2n+1 = ups, 2n+2 = head.  stage_of_param('__count__', n) returns the number of stages."""
    if name == '__count__':
        return 2 * n_levels + 3
    head = name.split('.')[0]
    if head in ('time_rel_pos_bias', 'init_conv', 'init_temporal_attn', 'time_mlp', 'null_cond_emb'):
        return 0
    if head == 'downs':
        return 1 + int(name.split('.')[1])
    if head.startswith('mid_'):
        return n_levels + 1
    if head == 'ups':
        return n_levels + 2 + int(name.split('.')[1])
    if head == 'final_conv':
        return 2 * n_levels + 2
    raise KeyError(name)


StepKeys = collections.namedtuple('StepKeys', 't noise frame_cond cond_drop focus_present lowres_aug')


def step_keys(rng_seed: int, rank: int, step: int, j: int = 0) -> StepKeys:
    """Every key of micro-step j of optimizer step `step`, one stream per (seed, rank), split per step like `key, step_key = split(key)`
    (trainer.py:541) and then as the reference's `__call__` / `p_losses` split:

        step key = split(split(rng_seed, rank + 1)[-1], step + 1)[-1]
          j > 0: the micro-step key is child 3 + j of it (children 1-3 belong to the split below); j = 0: the step key itself
          micro-step key -> child 1  frame_cond     the frame-conditioning mask draw (the child `_, t_key, loss_key` discards)
                            child 2  t              the timesteps (the host randint, or draw 0 of the device sampler)
                            child 3  loss key  ->   child 1  cond_drop      the condition-dropout draw
                                                    child 2  noise          the Philox stream of q_sample's noise
                                                    child 3  focus_present  the focus-present draw
                                                    child 4  lowres_aug     the super-resolution augmentation (levels and noise)

    split(key, n)[i] does not depend on n, so every draw has a child of its own: turning one feature on moves no other stream."""
    key = split_key(split_key(rng_seed, rank + 1)[-1], step + 1)[-1]
    if j > 0:
        key = split_key(key, 3 + j)[-1]
    frame_cond, t, loss_key = split_key(key, 3)
    cond_drop, noise, focus_present, lowres_aug = split_key(loss_key, 4)
    return StepKeys(t, noise, frame_cond, cond_drop, focus_present, lowres_aug)


def micro_step_keys(rng_seed: int, rank: int, step: int, j: int = 0):
    """(t_key, noise_key) of step_keys."""
    return tuple(step_keys(rng_seed, rank, step, j)[:2])


def frame_cond_key(rng_seed: int, rank: int, step: int, j: int = 0) -> int:
    return step_keys(rng_seed, rank, step, j).frame_cond


def cond_drop_key(rng_seed: int, rank: int, step: int, j: int = 0) -> int:
    return step_keys(rng_seed, rank, step, j).cond_drop


def focus_present_key(rng_seed: int, rank: int, step: int, j: int = 0) -> int:
    return step_keys(rng_seed, rank, step, j).focus_present


def lowres_aug_key(rng_seed: int, rank: int, step: int, j: int = 0) -> int:
    return step_keys(rng_seed, rank, step, j).lowres_aug


def self_cond_key(rng_seed: int, rank: int, step: int, j: int = 0) -> int:
    """Key of the self-conditioning coin of micro-step j (a self-conditioned diffusion only): child 5 of the loss key of step_keys' tree.
    split(key, n)[i] does not depend on n, so StepKeys stays as it is and no other stream moves.  The train step draws the coin under
    rank 0's key on every rank: data-parallel ranks then run the same number of forwards per step."""
    key = split_key(split_key(rng_seed, rank + 1)[-1], step + 1)[-1]
    if j > 0:
        key = split_key(key, 3 + j)[-1]
    return _loss_self_cond_key(split_key(key, 3)[-1])


def cond_drop_mask(batch: int, p: float, generator=None) -> torch.Tensor:
    """The condition-dropout mask of one micro-batch (Ho & Salimans 2022): uint8 [batch], Bernoulli(p), 1 = the sample sees the null
    embedding instead of its condition.  Pure host function of (arguments, generator state); p = 0 gives all 0, p = 1 all 1."""
    if not 0.0 <= float(p) <= 1.0:
        raise ValueError(f'null_cond_prob must be in [0, 1], got {p}')
    return (torch.rand(int(batch), generator=generator) < float(p)).to(torch.uint8)


def focus_present_draw(batch: int, p: float, generator=None) -> torch.Tensor:
    """The focus-present mask of one micro-batch (Video Diffusion Models, Ho et al. 2022, section 3.1): uint8 [batch], Bernoulli(p),
    1 = the sample is trained as a bag of images (each frame attends to itself only in the temporal blocks).  Pure host function of
    (arguments, generator state); p = 0 gives all 0, p = 1 all 1."""
    if not 0.0 <= float(p) <= 1.0:
        raise ValueError(f'prob_focus_present must be in [0, 1], got {p}')
    return (torch.rand(int(batch), generator=generator) < float(p)).to(torch.uint8)


def frame_cond_masks(batch: int, frames: int, k_max: int, uncond_prob: float = 0.25, mode: str = 'random', generator=None) -> torch.Tensor:
    """The context-frame masks of one micro-batch of frame-conditioned training (RaMViD, Hoeppe et al. 2022): uint8 [batch, frames],
    1 = the frame enters the network clean and carries no loss.  Per sample: with probability uncond_prob no frame is known (the
    unconditional task, RaMViD's p_U); otherwise K ~ U{1..k_max} frames are, K distinct frames drawn uniformly (mode 'random') or
    frames 0..K-1 (mode 'prefix', the prediction task).  1 <= k_max <= frames - 1, so every sample keeps a frame to learn from.  Pure
    host function of (arguments, generator state); every sample consumes the same three draws whatever its outcome."""
    if mode not in ('random', 'prefix'):
        raise ValueError(f"frame_cond_mode must be 'random' or 'prefix', got {mode!r}")
    if not 1 <= int(k_max) <= int(frames) - 1:
        raise ValueError(f'frame_cond_max must be in [1, {int(frames) - 1}] for {int(frames)} frames, got {k_max}')
    if not 0.0 <= float(uncond_prob) <= 1.0:
        raise ValueError(f'frame_cond_uncond_prob must be in [0, 1], got {uncond_prob}')
    masks = torch.zeros(int(batch), int(frames), dtype=torch.uint8)
    for b in range(int(batch)):
        u = float(torch.rand((), generator=generator))
        k = int(torch.randint(1, int(k_max) + 1, (), generator=generator))
        perm = torch.randperm(int(frames), generator=generator)
        if u < float(uncond_prob):
            continue
        masks[b, torch.arange(k) if mode == 'prefix' else perm[:k]] = 1
    return masks


def forward_backward(tr, batch: torch.Tensor, step: int, t=None, noise=None, *, j: int = 0, grads: torch.Tensor = None,
                     reducer=None, frame_mask=None, cond=None, cond_mask=None, focus_present_mask=None, aug_levels=None,
                     lowres=None, self_cond=None) -> torch.Tensor:
    """loss, grads = value_and_grad(p_losses) (trainer.py:337-361) of one micro-batch; returns the device scalar loss.

    frame_mask ([F], [B,F] or anything gaussian_diffusion.frame_mask takes; default: drawn by frame_cond_masks under frame_cond_key when
    tr.frame_cond_max > 0, else none): frame-conditioned training -- masked q_sample, the UNet forward unchanged, the loss and its
    gradient over the noised elements only (vdx_loss_sum_masked / vdx_loss_grad_masked: the count stays on the device), the backward
    unchanged.  tr.last_frame_mask holds the mask as given or drawn (None without one).

    cond [B, cond_dim] (conditional training, EXTENSION: the reference never drops the condition in training): the condition of every
    sample, handed to the forward; the backward uses what the forward recorded.  cond_mask [B] (1 = null embedding; default: drawn by
    cond_drop_mask under cond_drop_key when tr.null_cond_prob > 0, else none: every sample sees its condition).  tr.last_cond_mask
    holds the mask as given or drawn.  Without cond nothing here runs, whatever tr.null_cond_prob is.

    focus_present_mask [B] (joint image-video training; needs Unet3D(focus_present=True), without it nothing here runs; default: drawn by
    focus_present_draw under focus_present_key when 0 < tr.prob_focus_present, else none): the samples whose temporal blocks see each
    frame alone (Unet3D docstring).  tr.last_focus_mask holds the mask as given or drawn (None without one).

    aug_levels [B] / lowres [B,C,F/ft,S/fs,S/fs] (a super-resolution diffusion, gd.lowres_cond, only): the network input is
    xin = [ x_t | aug(up(2 lowres - 1)) ], built by one vdx_lowres_down (lowres defaults to the box mean of the raw batch) and one
    vdx_lowres_input launch (gd.sr_input); aug_levels defaults to a host draw from {0..gd.lowres_aug_max-1} under lowres_aug_key (none
    when lowres_aug_max is 0; -1 = none for that sample), the augmentation noise is Philox(lowres_aug_key, draw 0).  The forward and the
    staged backward run on xin; the loss, its gradient and everything after them are the plain ones over gd.channels.
    tr.last_aug_levels holds the levels as given or drawn.

    self_cond (a self-conditioned diffusion, gd.self_condition, only; Chen et al. 2022, sec. 2.2): None -- the coin of the micro-batch is
    drawn by self_cond_draw with probability tr.self_cond_prob under RANK 0's self_cond_key on every rank; False / True -- the coin as
    given; a [B,C,F,H,W] tensor -- a ready estimate.  The network input is xin = [ x_t | x0~ ] (gd.self_cond_input): zeros, x_t packed
    into the first half (vdx_lowres_pack) and, when the coin says so, pass 1 -- the same forward call as pass 2, then vdx_v_to_eps for
    pred_v and one vdx_selfcond_x0 launch (static clip) that writes the estimate into the second half.  Pass 2 -- the forward on xin,
    the loss, its gradient and the staged backward -- is the plain step over gd.channels; the estimate is a constant, nothing of pass 1
    is differentiated.  tr.last_self_cond holds the coin (or the tensor).  Refuses frame_mask / frame_cond_max.

    Loss-aware timestep sampling (tr.sampler, Trainer.timestep_sampler = 'loss-second-moment'): t and the importance weights iw come from
    one vdx_tsampler_draw launch under t_key (draw 0) in place of the host randint (an explicit t only gets its weights); the per-sample
    losses, the weighted mean (the returned loss: what is optimised) and the weighted gradient from one vdx_loss_weighted pass (or
    vdx_hybrid_loss_w); after the backward is enqueued the (t_b, l_b) enter the sampler's history (_sampler_update).  No host read is
    added.  tr.last_iw / tr.last_loss_per_sample hold the device tensors of the micro-batch.  Refuses frame_mask / frame_cond_max.

    `grads` (default tr.grads) receives the gradient: the head stage of the backward zeroes it.  With a `reducer` the backward runs
    in stage groups and hands finished buckets of tr.grads to it; when `grads` is a second buffer (micro-steps j >= 1), each finished
    bucket is first added into tr.grads on the current stream.  Without a reducer the backward is one call and nothing is reduced
    (the caller adds `grads` into tr.grads)."""
    gd, unet = tr.model, tr.unet
    dev = tr.device
    grads = tr.grads if grads is None else grads
    x = torch.as_tensor(batch).to(dev, torch.float32).contiguous()
    B = x.shape[0]
    assert tuple(x.shape[1:]) == (gd.channels, gd.num_frames, gd.image_size, gd.image_size), \
        f'expected [b, {gd.channels}, {gd.num_frames}, {gd.image_size}, {gd.image_size}], got {tuple(x.shape)}'     # check_shape (:490)
    keys = step_keys(tr.rng_seed, tr.rank, step, j)
    host_gen = lambda key: torch.Generator().manual_seed(key & 0x7FFFFFFFFFFFFFFF)
    smp = getattr(tr, 'sampler', None)
    if smp is not None and (frame_mask is not None or int(tr.frame_cond_max) > 0):
        raise ValueError('timestep_sampler=loss-second-moment does not serve frame-conditioned training (frame_mask / frame_cond_max): the '
                         'masked loss has no per-sample form')
    if gd.self_condition and (frame_mask is not None or int(tr.frame_cond_max) > 0):
        gd._refuse('self_condition', frame_mask=True)                     # (given, or to be drawn under frame_cond_max)
    if self_cond is not None and not gd.self_condition:
        raise ValueError('self_cond needs a self-conditioned diffusion (self_condition=True)')
    if t is None and smp is None:
        t = torch.randint(0, gd.num_timesteps, (B,), generator=host_gen(keys.t), dtype=torch.int32)
    t = None if t is None else _stage(t, torch.int32, dev)
    iw = None
    if smp is not None:
        # the device draw under the same t key (draw 0) replaces the host randint; an explicit t only gets its weights
        t, iw = smp.draw(B, keys.t, 0, t=t)
    tr.last_iw = iw
    noise = gd.noise(x.shape, keys.noise, 0) if noise is None else torch.as_tensor(noise).to(dev, torch.float32).contiguous()
    tr.last_t, tr.last_noise_key = t, keys.noise
    if frame_mask is None and int(tr.frame_cond_max) > 0:
        frame_mask = frame_cond_masks(B, gd.num_frames, tr.frame_cond_max, tr.frame_cond_uncond_prob, tr.frame_cond_mode, host_gen(keys.frame_cond))
    tr.last_frame_mask = frame_mask
    mk = None if frame_mask is None else expand_frame_mask(_stage(frame_mask, None, dev), tuple(x.shape))
    cm = None
    if cond is not None:
        cond = _stage(cond, torch.float32, dev)
        if cond_mask is None and float(tr.null_cond_prob) > 0:
            cond_mask = cond_drop_mask(B, tr.null_cond_prob, host_gen(keys.cond_drop))
        cm = None if cond_mask is None else _stage(cond_mask, torch.uint8, dev)
    tr.last_cond_mask = cond_mask if cond is not None else None
    fp = None
    if unet.focus_present:
        p_fp = float(getattr(tr, 'prob_focus_present', 0.0))
        if focus_present_mask is None and p_fp > 0:
            focus_present_mask = focus_present_draw(B, p_fp, host_gen(keys.focus_present))
        if focus_present_mask is not None:
            fp = torch.as_tensor(focus_present_mask).to(torch.uint8)
            if fp.shape != (B,):
                raise ValueError(f'focus_present_mask must be [{B}], got {tuple(fp.shape)}')
            if p_fp >= 1 and fp.device.type == 'cpu' and bool(fp.all()):
                fp = True                                                 # p = 1: every sample, the one-launch block (attention_present_kernel)
            elif fp.device.type == 'cpu':
                fp = _stage(fp, None, dev)
    tr.last_focus_mask = focus_present_mask if unet.focus_present else None
    gd._refuse('learned_variance', frame_mask=frame_mask, focus_present=fp)
    gd._refuse('lowres_cond', frame_mask=frame_mask, focus_present=fp)
    gd._refuse('objective', frame_mask=frame_mask)                        # (given, or drawn under frame_cond_max)
    if gd.self_condition:
        if self_cond is None:
            self_cond = self_cond_draw(tr.self_cond_prob, host_gen(self_cond_key(tr.rng_seed, 0, step, j)))
        elif not torch.is_tensor(self_cond):
            self_cond = bool(self_cond)
        tr.last_self_cond = self_cond
    if gd.lowres_cond is None:
        if aug_levels is not None or lowres is not None:
            raise ValueError('aug_levels / lowres need a super-resolution diffusion (lowres_cond=(ft, fs))')
    elif lowres is not None:
        gd._sr_lowres(lowres, B)
    # the (masked) q_sample with normalize_img folded in (:499), or [ x_t | u ] of a super-resolution diffusion
    x_noisy, aug_levels = gd._net_input(x, t, noise, mask=mk, lowres=lowres, aug_levels=aug_levels, aug_key=keys.lowres_aug, _pre=(2.0, -1.0))
    if gd.lowres_cond is not None:
        tr.last_aug_levels = aug_levels
    keep_storage = unet.act_bf16
    unet.act_bf16 = 2 if (unet.mode == 'bf16' and tr.train_act_bf16) else False
    try:
        forward = lambda xin: unet(xin, t, cond=cond, cond_mask=cm, focus_present_mask=fp)
        if gd.self_condition:
            x_noisy = gd.self_cond_input(x_noisy, t, self_cond, forward)
        eps_hat = forward(x_noisy)
    finally:
        unet.act_bf16 = keep_storage
    # the loss (the returned one is what is optimised: the hybrid total, the masked mean, the weighted mean) and its gradient in eps_hat
    loss, d_eps = gd.loss_and_grad(eps_hat, x, noise, t, mask=mk, iw=iw, want_grad=True, _pre=(2.0, -1.0))
    if smp is not None:
        per = gd.last_loss_per_sample                                     # hybrid: the per-sample (mse, vb) pairs
        tr.last_loss_per_sample = per[:, 0] + gd.vlb_weight * per[:, 1] if gd.learned_variance else per
    if reducer is None:
        unet.backward(d_eps, grads)
        _sampler_update(tr, t)
        return loss
    # reverse pass in groups of stages that end where a gradient bucket becomes complete: finished buckets are all-reduced (RCCL)
    # while earlier stages still run.  One call per group, not per stage: a call ends with the main stream waiting for the
    # weight-gradient stream (vdx_unet_backward), which nothing needs between bucket boundaries -- and never on one GPU.
    ns = unet.num_stages
    cuts = sorted({min(max(b[2], 0), ns - 1) for b in tr.buckets} | {0}, reverse=True) if reducer.enabled else [0]
    hi, nxt = ns - 1, 0
    for lo in cuts:
        if lo > hi:
            continue
        unet.backward(d_eps, grads, hi, lo)
        if grads is not tr.grads:
            nxt = _accumulate_ready(tr, grads, nxt, lo)
        for stage in range(hi, lo - 1, -1):
            reducer.stage_done(stage)
        hi = lo - 1
    if grads is not tr.grads:
        _accumulate_ready(tr, grads, nxt, -1)
    _sampler_update(tr, t)
    return loss


def _sampler_update(tr, t: torch.Tensor) -> None:
    """Loss-aware timestep sampling: the (t_b, l_b) of the micro-batch enter the sampler's history, after the backward is enqueued.  On
    more than one rank every rank applies the entries of all ranks, in (rank, sample) order, so that every rank holds the same history
    (torch.distributed.all_gather of the [B][2] entries).  Launches only: the host reads nothing (RCCL; gloo stages device tensors through
    the host, in the one-GPU tests)."""
    smp = getattr(tr, 'sampler', None)
    if smp is None:
        return
    entries = torch.stack([t.to(torch.float64), tr.last_loss_per_sample.to(torch.float64)], 1).contiguous()
    if tr.dist_on and tr.world > 1:
        if tr.comm_backend == 'abi':
            raise ValueError("timestep_sampler=loss-second-moment needs comm_backend='torch' on more than one rank: the C communicator has "
                             'no gather')
        import torch.distributed as dist
        parts = [torch.empty_like(entries) for _ in range(tr.world)]
        dist.all_gather(parts, entries)
        entries = torch.cat(parts, 0)
    smp.update(entries)


def _accumulate_ready(tr, micro: torch.Tensor, nxt: int, stage: int) -> int:
    """tr.grads += micro over the buckets from index `nxt` that are complete once the backward has run `stage` (the test of
    GradBucketReducer.stage_done); buckets are contiguous in ready order, so they go as one range.  Returns the next bucket index."""
    first = nxt
    while nxt < len(tr.buckets) and tr.buckets[nxt][2] >= stage:
        nxt += 1
    if nxt > first:
        lo, hi = tr.buckets[nxt - 1][0], tr.buckets[first][1]
        L.check(vdx_grad_accumulate(tr.grads.data_ptr() + 4 * lo, micro.data_ptr() + 4 * lo, hi - lo, L.stream_ptr()))
    return nxt


def optimizer_tail(tr, step: int, world: int, accum: int = 1, max_grad_norm=None, want_norm: bool = False) -> None:
    """Adam + EMA on the summed gradient in tr.grads (trainer.py:367-382); the mean over ranks and micro-batches is folded into the
    gradient read.  With max_grad_norm (or want_norm) the step goes through the sum of squares of tr.grads and the clipping form of
    the kernel, and tr.last_grad_norm holds the device float of the pre-clip norm; the host reads nothing."""
    unet = tr.unet
    n = unet.flat_params.numel()
    lr = tr.current_lr(tr.opt_count)                                               # schedule at the pre-increment count (B.2)
    do_ema = int(step >= tr.step_start_ema and step % tr.update_ema_every == 0)    # trainer.py:373-374
    grad_scale = 1.0 / (world * accum)
    if max_grad_norm is None and not want_norm:
        L.check(vdx_adam_ema_step(L.ptr(unet.flat_params), L.ptr(tr.grads), L.ptr(tr.m), L.ptr(tr.v), L.ptr(tr.ema), n,
                                  lr, 0.9, 0.999, 1e-8, tr.opt_count, grad_scale, do_ema, tr.ema_decay, L.stream_ptr()))
    else:
        if getattr(tr, '_sqnorm', None) is None:
            tr._sqnorm = torch.empty(vdx_grad_sqnorm_scratch_doubles() + 1, dtype=torch.float64, device=tr.device)
            tr.last_grad_norm = torch.zeros(1, dtype=torch.float32, device=tr.device)
        sq = tr._sqnorm
        L.check(vdx_grad_sqnorm(L.ptr(tr.grads), n, sq.data_ptr() + 8, sq.data_ptr(), L.stream_ptr()))
        L.check(vdx_adam_ema_step_clip(L.ptr(unet.flat_params), L.ptr(tr.grads), L.ptr(tr.m), L.ptr(tr.v), L.ptr(tr.ema), n,
                                       lr, 0.9, 0.999, 1e-8, tr.opt_count, grad_scale, do_ema, tr.ema_decay, sq.data_ptr(),
                                       FLT_MAX if max_grad_norm is None else float(max_grad_norm), L.ptr(tr.last_grad_norm), L.stream_ptr()))
    tr.opt_count += 1
    unet.mark_params_updated()


def run_train_step(tr, batch: torch.Tensor, step: int, t: torch.Tensor = None, noise: torch.Tensor = None, frame_mask=None,
                   cond=None, cond_mask=None, focus_present_mask=None, aug_levels=None, lowres=None, self_cond=None) -> torch.Tensor:
    """loss, grads = value_and_grad(p_losses); Adam; EMA  (trainer.py:337-382) for this rank's shard of the batch.

    `t` [B] / `noise` [B,C,F,H,W] override this rank's own draws (the reference threads `noise` through p_losses the same way,
    gaussian_diffusion.py:423-445); the data-parallel tests use them to give N ranks the shards of ONE global draw.  frame_mask: the
    shard's context-frame mask (forward_backward); each shard divides its loss by its own count of noised elements.  cond / cond_mask:
    the shard's conditions and its condition-dropout mask (forward_backward).  focus_present_mask: the shard's focus-present mask
    (forward_backward).  aug_levels / lowres: the shard's augmentation levels and low-resolution clips of a super-resolution diffusion
    (forward_backward).  self_cond: the coin (or the ready estimate) of a self-conditioned diffusion (forward_backward)."""
    reducer = tr.make_reducer()
    loss = forward_backward(tr, batch, step, t, noise, reducer=reducer, frame_mask=frame_mask, cond=cond, cond_mask=cond_mask,
                            focus_present_mask=focus_present_mask, aug_levels=aug_levels, lowres=lowres, self_cond=self_cond)
    reducer.finish()
    optimizer_tail(tr, step, reducer.world)
    return loss


def run_train_step_accum(tr, batches, step: int, ts=None, noises=None, frame_masks=None, conds=None, cond_masks=None,
                         focus_present_masks=None, self_conds=None) -> torch.Tensor:
    """One optimizer step on the mean gradient of K = len(batches) micro-batches of this rank (Trainer.apply_grad_args).

    Micro-step 0 is run_train_step's path into tr.grads; micro-steps j >= 1 write tr.micro_grads and are added into tr.grads.  Only the
    last micro-step runs the staged backward and starts the all-reduce, bucket by bucket, after the bucket's accumulation: one
    reduction per optimizer step, still overlapped with the backward.  Returns the mean of the K device losses.  frame_masks: optional
    list of K context-frame masks (forward_backward); every micro-batch divides by its own count, then the K gradients are averaged.
    conds / cond_masks: optional lists of K conditions / condition-dropout masks (forward_backward).  focus_present_masks: optional
    list of K focus-present masks (forward_backward).  self_conds: optional list of K self-conditioning coins / estimates
    (forward_backward; default: every micro-step draws its own)."""
    K = len(batches)
    assert K >= 1
    ts, noises, fms, cds, cms, fps, scs = ([None] * K if v is None else v
                                           for v in (ts, noises, frame_masks, conds, cond_masks, focus_present_masks, self_conds))
    if K > 1 and getattr(tr, 'micro_grads', None) is None:
        tr.micro_grads = torch.zeros_like(tr.grads)
    reducer = tr.make_reducer()
    losses = []
    for j in range(K):
        grads = tr.grads if j == 0 else tr.micro_grads
        losses.append(forward_backward(tr, batches[j], step, ts[j], noises[j], j=j, grads=grads, reducer=reducer if j == K - 1 else None,
                                       frame_mask=fms[j], cond=cds[j], cond_mask=cms[j], focus_present_mask=fps[j], self_cond=scs[j]))
        if 0 < j < K - 1:
            L.check(vdx_grad_accumulate(L.ptr(tr.grads), L.ptr(grads), grads.numel(), L.stream_ptr()))
    reducer.finish()
    max_norm = tr.max_grad_norm
    optimizer_tail(tr, step, reducer.world, accum=K, max_grad_norm=max_norm, want_norm=tr.track_grad_norm)
    return losses[0] if K == 1 else torch.stack(losses).mean()
