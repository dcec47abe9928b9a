"""Trainer -- host-side mirror of the reference class (/root/reference/trainer.py:52-628).

Same constructor signature and `.train(prob_focus_present, focus_present_mask, log_fn)` entry.  One train step
(reference `_pjit_train_step`, trainer.py:322-392) = q_sample -> Unet3D forward -> loss -> backward -> gradient
all-reduce -> Adam -> EMA, all on the device through libvdx.so; data parallelism = one process per GPU with
`torch.distributed` (RCCL), the flat gradient buffer reduced in buckets in reverse-layer order so the
all-reduce of early buckets overlaps the rest of the backward.
Accepted-and-unused arguments are the reference's own: folder, num_frames, save_and_sample_every, num_sample_rows,
sample_text, cond_scale, add_loss_plot.  gradient_accumulate_every and max_grad_norm are unused in the reference too (it marks the first
TODO and never calls its clip_grad_norm); here they are honoured behind `Trainer.apply_grad_args = True`: one optimizer step then takes
K = gradient_accumulate_every micro-batches per rank (one all-reduce per optimizer step) and clips the averaged gradient to
max_grad_norm by its global L2 norm, on the device (train_step.run_train_step_accum).
"""
from __future__ import annotations

import json
import logging
import math
import os
import time
from pathlib import Path
from typing import List, Optional, Tuple

import numpy as np
import torch

from .checkpoint import CheckpointManager, load_checkpoint, save_checkpoint
from .utils import cycle, noop


def lr_schedule(step: int, train_lr: float, lr_decay_start_step: int = 0, lr_decay_steps: int = 0, lr_decay_coeff: float = 1.0) -> float:
    """optax.piecewise_interpolate_schedule('cosine', train_lr, {start: 1.0, start + steps: coeff}) (trainer.py:138-145).
    The dict literal's duplicate key collapses when steps == 0; a zero-length interval contributes nothing."""
    bs = {lr_decay_start_step: 1.0}
    bs[lr_decay_start_step + lr_decay_steps] = lr_decay_coeff
    items = sorted(bs.items())
    bounds = [0] + [b for b, _ in items]
    values = [train_lr]
    for _, s in items:
        values.append(values[-1] * s)
    for i in range(len(bounds) - 1):
        lo, hi = bounds[i], bounds[i + 1]
        if lo <= step < hi:
            pct = (step - lo) / (hi - lo)
            return values[i + 1] + (values[i] - values[i + 1]) / 2.0 * (math.cos(math.pi * pct) + 1.0)
    return values[-1]


def make_buckets(param_table, total: int, stage_of, n_stages: int, min_bucket_floats: int = 4 << 20) -> List[Tuple[int, int, int]]:
    """Partition the flat gradient buffer into contiguous (lo, hi, ready_stage) buckets.

    Backward visits stages n_stages-1 .. 0; parameters are laid out in forward order, so a bucket [lo, hi) is complete once
    the backward has finished the LOWEST stage it contains.  Buckets are listed in the order they become ready."""
    edges = []            # (offset, stage) per tensor, forward order
    for name, shape, off in param_table:
        edges.append((off, stage_of(name)))
    buckets = []
    hi = total
    cur_stage = None
    for off, st in reversed(edges):
        cur_stage = st if cur_stage is None else min(cur_stage, st)
        if hi - off >= min_bucket_floats:
            buckets.append((off, hi, cur_stage))
            hi, cur_stage = off, None
    if hi > 0:
        buckets.append((0, hi, 0 if cur_stage is None else min(cur_stage, 0)))
    return buckets


class GradBucketReducer:
    """Sum all-reduce of a flat gradient tensor in buckets (async), averaged by the caller (1/world in the Adam read)."""

    def __init__(self, flat_grads: torch.Tensor, buckets, group=None):
        import torch.distributed as dist
        self.dist = dist
        self.flat, self.buckets, self.group = flat_grads, list(buckets), group
        self.enabled = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
        self.world = dist.get_world_size(group) if self.enabled else 1
        self._work, self._next = [], 0

    def stage_done(self, stage: int):
        """Called after the backward has enqueued stage `stage`: launches every bucket that became complete."""
        while self._next < len(self.buckets) and self.buckets[self._next][2] >= stage:
            lo, hi, _ = self.buckets[self._next]
            if self.enabled:
                self._work.append(self.dist.all_reduce(self.flat[lo:hi], op=self.dist.ReduceOp.SUM, group=self.group, async_op=True))
            self._next += 1

    def finish(self):
        self.stage_done(-1)
        for w in self._work:
            w.wait()
        self._work, self._next = [], 0


class AbiBucketReducer:
    """GradBucketReducer's contract with the collective behind the C ABI: each finished bucket goes through vdx_allreduce_bucket
    (RCCL communicator owned by the vdx handle, csrc/comm.cpp) on a side stream that waits for the stage's kernels through an event;
    the caller's stream waits for the side stream in finish().  SURVEY 8(b): vdx_comm_init / vdx_allreduce_bucket."""

    def __init__(self, flat_grads: torch.Tensor, buckets, handle, world: int, comm_stream):
        self.flat, self.buckets, self.h, self.world, self.cs = flat_grads, list(buckets), handle, world, comm_stream
        self.enabled = True
        self._next = 0

    def stage_done(self, stage: int):
        from .unet3d import vdx_allreduce_bucket
        from . import _lib as L
        ready = []
        while self._next < len(self.buckets) and self.buckets[self._next][2] >= stage:
            ready.append(self.buckets[self._next]); self._next += 1
        if not ready or not self.enabled:
            return
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.flat.device))
        self.cs.wait_event(ev)
        for lo, hi, _ in ready:
            L.check(vdx_allreduce_bucket(self.h.ptr, self.flat.data_ptr() + 4 * lo, hi - lo, self.cs.cuda_stream))

    def finish(self):
        self.stage_done(-1)
        torch.cuda.current_stream(self.flat.device).wait_stream(self.cs)
        self._next = 0


class Trainer:
    # 'torch': torch.distributed.all_reduce per bucket (RCCL under the nccl backend; gloo in the CPU / one-GPU tests).
    # 'abi': the communicator inside libvdx.so (vdx_comm_init / vdx_allreduce_bucket); needs a CUDA device.  VDX_COMM overrides.
    comm_backend = os.environ.get('VDX_COMM', 'torch')
    # mode='bf16' networks: the training forward stores its inter-kernel activations as bf16 (vdx_set_activation_storage(h, 2)) -- the
    # forward then runs on the sampling path's kernels and every activation read of the backward halves; False = fp32 slots
    train_act_bf16 = True
    # gradient all-reduce bucket size (floats): >= 16 MB per RCCL call keeps every xGMI ring step bandwidth-bound; the
    # constructor signature stays the reference's, so this is a class attribute
    min_bucket_floats = 4 << 20
    # False: gradient_accumulate_every and max_grad_norm are stored and ignored, as in the reference.  True: train() takes
    # K = max(1, gradient_accumulate_every) micro-batches per optimizer step (train_step_accum) and clips the averaged gradient to
    # max_grad_norm (None = no clipping).  A class attribute for the same reason as the ones above.
    apply_grad_args = False
    # with apply_grad_args: compute the gradient norm (last_grad_norm, 'grad_norm/train') also when max_grad_norm is None
    track_grad_norm = False
    # Frame-conditioned training (extension; RaMViD, Hoeppe et al. 2022): frame_cond_max = K_max > 0 gives every sample of every
    # (micro-)batch a random set of up to K_max context frames that enter the network clean and carry no loss (train_step.frame_cond_masks,
    # drawn under train_step.frame_cond_key); with probability frame_cond_uncond_prob (RaMViD's p_U) a sample has none.  Mode 'random':
    # any frames (prediction, infilling, extension alike); 'prefix': the first K (prediction).  0 = off: the reference's objective, the
    # kernels and random streams of before.  Sample such a model with inpaint / extend(clean_context=True).  Class attributes for the
    # same reason as the ones above.
    frame_cond_max = 0
    frame_cond_uncond_prob = 0.25
    frame_cond_mode = 'random'
    # Conditional training for classifier-free guidance (extension: the reference's training never drops the condition).  cond_path: a
    # .npy float32 file [N, cond_dim] of ready-made embeddings, row i = the condition of video i of the dataset (synthetic:N included);
    # the dataset then yields (video, cond_row) pairs, so shuffling keeps them together.  null_cond_prob = p > 0 replaces the condition of
    # every sample with probability p by the network's null embedding (train_step.cond_drop_mask, drawn under train_step.cond_drop_key;
    # Ho & Salimans use 0.1-0.2).  Without cond_path nothing changes, whatever null_cond_prob is.  Sample such a model with
    # sample(cond=, cond_scale=) / sample.py --cond-path.  Class attributes for the same reason as the ones above.
    cond_path = None
    null_cond_prob = 0.0
    # Joint image-video training (extension; Video Diffusion Models, Ho et al. 2022, section 3.1; needs Unet3D(focus_present=True), without
    # it nothing changes): every sample is focus-present with probability prob_focus_present -- in the temporal blocks each of its frames
    # attends to itself only, so the sample is trained as a bag of images (train_step.focus_present_draw under
    # train_step.focus_present_key).  train(prob_focus_present, focus_present_mask) override it for that run.
    prob_focus_present = 0.0
    # Loss-aware timestep sampling (extension; Nichol & Dhariwal 2021, section 3.3; timestep_sampler.LossSecondMomentSampler).  'uniform':
    # t is drawn uniformly on the host, the objective, kernels, launches and random streams of before.  'loss-second-moment': t is drawn
    # on the device with p_t ~ sqrt(E[l_t^2]) over the last sampler_history losses seen at each level, mixed with sampler_uniform_prob of
    # the uniform distribution, and every sample's loss is weighted by 1 / (T p_t); uniform with weights 1 until every level has a full
    # history.  The state lives on the device (tr.sampler), is the same on every rank and is not checkpointed: a resumed run restarts it
    # cold, as it restarts Adam's moments.  Class attributes for the same reason as the ones above.
    timestep_sampler = 'uniform'
    sampler_history = 10
    sampler_uniform_prob = 0.001
    # Self-conditioned training (extension; Chen et al. 2022, "Analog Bits", section 2.2; a GaussianDiffusion(self_condition=True) only,
    # without one nothing changes): with probability self_cond_prob a (micro-)step first runs the network on [ x_t | 0 ], without
    # gradient, and then regresses from [ x_t | x0~ ] with x0~ its clipped estimate of x0; otherwise from [ x_t | 0 ]
    # (train_step.self_cond_draw under train_step.self_cond_key of rank 0: one coin per micro-step, the same on every rank).  A step at
    # 0.5 costs half a forward more on average.  A class attribute for the same reason as the ones above.
    self_cond_prob = 0.5

    def __init__(self, diffusion_model, folder: str, *, rng_seed: int = 0, dataset_path: str, num_frames: int = 16,
                 train_batch_size: int = 4, train_lr: float = 1e-4, train_num_steps: int = 100000,
                 gradient_accumulate_every: int = 2, step_start_ema: int = 2000, update_ema_every: int = 10,
                 save_and_sample_every: int = 100000, results_folder: str = './results', num_sample_rows: int = 4,
                 max_grad_norm: Optional[float] = None, use_path_as_cond: bool = False, sample_text: Optional[str] = None,
                 cond_scale: float = 2.0, checkpoint_every_steps: int = 10, checkpoint_dir_path: str = '',
                 add_loss_plot: bool = False, tensorboard_dir: str = '', resume_training_step: int = 0, ema_decay: float = 0.9999,
                 max_to_keep: Optional[int] = None, lr_decay_start_step: int = 0, lr_decay_steps: int = 0, lr_decay_coeff: float = 1.0,
                 profile_flush_step: int = 100, num_model_shards: int = 1):
        import torch.distributed as dist
        assert num_model_shards == 1, 'only data parallelism is supported (the GSPMD "model" axis of trainer.py:407-426 is out of scope)'
        self.model = diffusion_model
        self.unet = diffusion_model.denoise_fn
        self.device = self.unet.device
        self.rng_seed = int(rng_seed)
        self.step_start_ema, self.update_ema_every, self.ema_decay = step_start_ema, update_ema_every, ema_decay
        self.train_lr, self.lr_args = train_lr, (lr_decay_start_step, lr_decay_steps, lr_decay_coeff)
        self.train_num_steps, self.max_grad_norm = train_num_steps, max_grad_norm
        self.use_path_as_cond, self.gradient_accumulate_every = use_path_as_cond, gradient_accumulate_every
        self.profile_flush_step = profile_flush_step
        # ---- data-parallel layout (trainer.py:161-177): the reference's batch is GLOBAL and split over devices ----
        self.dist_on = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size() if self.dist_on else 1
        self.rank = dist.get_rank() if self.dist_on else 0
        assert train_batch_size % self.world == 0, 'batch_size must be divisible by number of devices'     # trainer.py:163
        if self.dist_on and self.device.type == 'cuda':
            # parameters, gradients and workspaces must live on the GPU this rank's process group and HIP stream are bound to
            assert self.device.index == torch.cuda.current_device(), \
                f'Unet3D lives on {self.device} but this rank runs on cuda:{torch.cuda.current_device()}: build the model after torch.cuda.set_device(LOCAL_RANK)'
        self.batch_size = train_batch_size
        self.per_device_bs = train_batch_size // self.world
        # ---- optimizer state: Adam m, v + EMA copy, flat like the parameters ----
        n = self.unet.flat_params.numel()
        self.m = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.v = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.ema = self.unet.flat_params.clone()
        self.grads = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.opt_count = 0                                       # optax count: restarts at 0 on resume
        self.micro_grads = None                                  # second gradient buffer, allocated by the first K > 1 step
        self.last_grad_norm = None                               # device float of the last pre-clip gradient norm
        self.last_frame_mask = None                              # context-frame mask of the last micro-batch (frame_cond_max > 0)
        self.last_cond_mask = None                               # condition-dropout mask of the last micro-batch (null_cond_prob > 0)
        self.last_focus_mask = None                              # focus-present mask of the last micro-batch (prob_focus_present > 0)
        self.last_self_cond = None                               # self-conditioning coin of the last micro-batch (a self-conditioned diffusion)
        from .train_step import stage_of_param
        nlev = len(self.unet.dim_mults)
        self.buckets = make_buckets(self.unet.param_table, n, lambda nm: stage_of_param(nm, nlev), stage_of_param('__count__', nlev),
                                    min_bucket_floats=self.min_bucket_floats)
        # ---- dataset ----
        self.image_size = diffusion_model.image_size
        if str(dataset_path).startswith('synthetic'):
            from .datasets import SyntheticVideo
            n_items = int(str(dataset_path).split(':')[1]) if ':' in str(dataset_path) else 64
            self.ds = SyntheticVideo(n_items, diffusion_model.channels, diffusion_model.num_frames, self.image_size, seed=self.rng_seed)
        else:
            from .datasets import MovingMNIST
            self.ds = MovingMNIST(dataset_path, image_size=(self.image_size, self.image_size), num_frames=diffusion_model.num_frames,
                                  force_num_frames=True)
        assert len(self.ds) > 0, 'Dataset is empty. Check path and format.'
        if not 0.0 <= float(self.null_cond_prob) <= 1.0:
            raise ValueError(f'null_cond_prob must be in [0, 1], got {self.null_cond_prob}')
        if not 0.0 <= float(self.prob_focus_present) <= 1.0:
            raise ValueError(f'prob_focus_present must be in [0, 1], got {self.prob_focus_present}')
        if isinstance(self.self_cond_prob, bool) or not 0.0 <= float(self.self_cond_prob) <= 1.0:
            raise ValueError(f'self_cond_prob must be in [0, 1], got {self.self_cond_prob}')
        if getattr(diffusion_model, 'self_condition', False) and int(self.frame_cond_max) > 0:
            raise ValueError('self_condition does not support frame_mask yet (a follow-up; DESIGN.md 9): frame_cond_max > 0 draws one')
        from . import timestep_sampler as TS
        if self.timestep_sampler not in TS.SAMPLERS:
            raise ValueError(f'timestep_sampler must be one of {TS.SAMPLERS}, got {self.timestep_sampler!r}')
        TS.validate(1, self.sampler_history, self.sampler_uniform_prob)
        self.sampler = None                                      # the device-resident sampler ('loss-second-moment' only)
        self.last_iw = None                                      # importance weights of the last micro-batch (device float64 [B])
        self.last_loss_per_sample = None                         # unweighted per-sample losses of the last micro-batch (device float64 [B])
        if self.timestep_sampler == 'loss-second-moment':
            TS.validate(diffusion_model.num_timesteps, self.sampler_history, self.sampler_uniform_prob)
            if int(self.frame_cond_max) > 0:
                raise ValueError('timestep_sampler=loss-second-moment does not serve frame-conditioned training (frame_cond_max > 0): the '
                                 'masked loss has no per-sample form')
            if self.comm_backend == 'abi' and self.world > 1:
                raise ValueError("timestep_sampler=loss-second-moment needs comm_backend='torch' on more than one rank: the C communicator "
                                 'has no gather')
            self.sampler = TS.LossSecondMomentSampler(diffusion_model.num_timesteps, self.sampler_history, self.sampler_uniform_prob,
                                                      device=self.device)
        if self.cond_path is not None:
            from .datasets import CondPairs, load_cond_file
            self.ds = CondPairs(self.ds, load_cond_file(self.cond_path, len(self.ds), self.unet.cond_dim))
        g = torch.Generator().manual_seed(self.rng_seed)
        self.dl = cycle(torch.utils.data.DataLoader(self.ds, batch_size=self.batch_size, shuffle=True, drop_last=True, generator=g))
        # ---- results / checkpoints / logs ----
        self.results_folder = Path(results_folder).resolve()
        self.results_folder.mkdir(exist_ok=True, parents=True)
        self.checkpoint_dir_path = Path(checkpoint_dir_path).resolve() if checkpoint_dir_path else (self.results_folder / 'checkpoints').resolve()
        self.checkpoint_every_steps = checkpoint_every_steps
        self.ckpt_manager = CheckpointManager(self.checkpoint_dir_path, max_to_keep=max_to_keep) if self.rank == 0 else None
        self.log_dir = Path(tensorboard_dir).resolve() if tensorboard_dir else self.results_folder / 'tensorboard'
        self.log_dir.mkdir(exist_ok=True, parents=True)
        self._scalars = open(self.log_dir / f'scalars_rank{self.rank}.jsonl', 'a') if self.rank == 0 else None
        # ---- resume (params + EMA only; optimizer state re-initialised, as the reference) ----
        self.step = resume_training_step
        if self.step > 0:
            try:
                _, ema_params = load_checkpoint(self.model, self.step, str(self.checkpoint_dir_path))
                sd = self.unet.state_dict()
                for k, vv in ema_params.items():
                    shape, off = self.unet._index[k]
                    self.ema[off:off + vv.numel()] = vv.reshape(-1).to(self.device)
                logging.info(f'Successfully loaded checkpoint state for step {self.step}')
            except FileNotFoundError:
                logging.warning(f'Checkpoint for step {self.step} not found at {self.checkpoint_dir_path}.')
                self.step = 0

    # ------------------------------------------------------------------------------------------------
    def _scalar(self, tag, value, step):
        if self._scalars:
            self._scalars.write(json.dumps({'tag': tag, 'value': float(value), 'step': int(step)}) + '\n')

    def current_lr(self, count: int) -> float:
        return lr_schedule(count, self.train_lr, *self.lr_args)

    def _save(self, step: int):
        if self.ckpt_manager is None:
            return
        try:
            names = [(n, s, o) for n, s, o in self.unet.param_table]
            ema_sd = {n: self.ema[o:o + int(np.prod(s))].view(*s) for n, s, o in names}
            save_checkpoint(self.ckpt_manager, self.unet.state_dict(), ema_sd, step)
        except Exception as e:                                   # reference: log and continue (trainer.py:595-602)
            logging.error(f'Error saving checkpoint at step {step}: {e}')

    def _abi_comm(self):
        """Joins (once) the RCCL communicator of the training handle: rank 0 creates the unique id, the group's own channel carries it."""
        if getattr(self, '_abi', None) is None:
            import ctypes as C
            import torch.distributed as dist
            from .unet3d import vdx_comm_init, vdx_comm_unique_id
            from . import _lib as L
            h = self.unet.handle(self.model.num_frames, self.model.image_size)
            buf = C.create_string_buffer(128)
            if self.rank == 0:
                L.check(vdx_comm_unique_id(buf))
            box = [bytes(buf.raw)]
            if self.dist_on and self.world > 1:
                dist.broadcast_object_list(box, src=0)
            L.check(vdx_comm_init(h.ptr, self.rank, self.world, box[0]))
            self._abi = (h, torch.cuda.Stream(device=self.device))
        return self._abi

    def make_reducer(self):
        if self.comm_backend == 'abi':
            h, cs = self._abi_comm()
            red = AbiBucketReducer(self.grads, self.buckets, h, self.world, cs)
        else:
            red = GradBucketReducer(self.grads, self.buckets)
        if not getattr(self, 'comm_enabled', True):              # timing aid (bench.py: the same step without the collective)
            red.enabled = False
        return red

    def train_step(self, batch: torch.Tensor, step: int, t=None, noise=None, frame_mask=None, cond=None, cond_mask=None,
                   focus_present_mask=None, aug_levels=None, lowres=None, self_cond=None) -> torch.Tensor:
        """One `_pjit_train_step` on this rank's shard of the batch.  Returns the (device) scalar loss of the shard.
        t / noise: optional explicit timesteps / noise of the shard (default: this rank's own Philox draws).  frame_mask: optional
        explicit context-frame mask of the shard ([F] or [B,F], 1 = clean context; default: drawn when frame_cond_max > 0).  cond: the
        shard's conditions [B, cond_dim] (a conditioned UNet needs them); cond_mask: optional explicit condition-dropout mask [B], 1 = null
        embedding (default: drawn when null_cond_prob > 0).  focus_present_mask: optional explicit focus-present mask [B] of the shard
        (Unet3D(focus_present=True); default: drawn when prob_focus_present > 0).  aug_levels / lowres (a super-resolution diffusion,
        GaussianDiffusion(lowres_cond=...), only): optional explicit augmentation levels [B] (-1 = none; default: drawn from
        {0..lowres_aug_max-1}) and low-resolution clips (default: the box mean of the batch).  self_cond (a self-conditioned diffusion,
        GaussianDiffusion(self_condition=True), only): None = the coin of the two-pass step is drawn with probability self_cond_prob;
        False / True = the coin as given; a [B,C,F,H,W] tensor = a ready estimate (train_step.forward_backward)."""
        from .train_step import run_train_step
        return run_train_step(self, batch, step, t=t, noise=noise, frame_mask=frame_mask, cond=cond, cond_mask=cond_mask,
                              focus_present_mask=focus_present_mask, aug_levels=aug_levels, lowres=lowres, self_cond=self_cond)

    @property
    def accum_steps(self) -> int:
        """Micro-batches per optimizer step: gradient_accumulate_every behind apply_grad_args, else 1."""
        return max(1, int(self.gradient_accumulate_every)) if self.apply_grad_args else 1

    def train_step_accum(self, batches, step: int, ts=None, noises=None, frame_masks=None, conds=None, cond_masks=None,
                         focus_present_masks=None, self_conds=None) -> torch.Tensor:
        """One optimizer step on K = len(batches) shards of this rank: the gradient is the mean over the K micro-batches (and the
        ranks), clipped to max_grad_norm when that is set.  Returns the (device) mean of the K losses; `last_grad_norm` holds the
        device float of the pre-clip norm when one was computed.  ts / noises / frame_masks / conds / cond_masks /
        focus_present_masks / self_conds: optional per-micro-batch lists, as train_step's."""
        from .train_step import run_train_step_accum
        assert self.apply_grad_args, 'train_step_accum is the path behind Trainer.apply_grad_args = True'
        return run_train_step_accum(self, list(batches), step, ts=ts, noises=noises, frame_masks=frame_masks, conds=conds,
                                    cond_masks=cond_masks, focus_present_masks=focus_present_masks, self_conds=self_conds)

    def train(self, prob_focus_present: Optional[float] = None, focus_present_mask=None, log_fn=noop):
        """The training loop.  prob_focus_present (default: the attribute of that name) / focus_present_mask ([train_batch_size] mask of
        the GLOBAL batch, used for every step; wins over the probability): joint image-video training, honoured when the network was
        built with Unet3D(focus_present=True) and without effect otherwise, as in the reference."""
        assert callable(log_fn)
        if prob_focus_present is not None:
            if not 0.0 <= float(prob_focus_present) <= 1.0:
                raise ValueError(f'prob_focus_present must be in [0, 1], got {prob_focus_present}')
            self.prob_focus_present = float(prob_focus_present)
        logging.info(f'Starting training loop from step {self.step}...')
        import torch.distributed as dist
        from .datasets import DevicePrefetcher
        lo, hi = self.rank * self.per_device_bs, (self.rank + 1) * self.per_device_bs
        # this rank's shard of every batch (P('data', None), trainer.py:309), staged one batch ahead on a side stream
        shards = DevicePrefetcher(self.dl, self.device, select=lambda b: b[lo:hi])
        # trace hook (reference trainer.py:524-533,607: jax.profiler trace from the first step until profile_flush_step): every step up to
        # profile_flush_step is one roctx range ("train_step N", via torch.cuda.nvtx = roctx on ROCm), so `rocprofv3 --marker-trace
        # --kernel-trace -- python train.py ...` groups the kernels per step; no-op without the marker library
        def _range(push, name=''):
            try:
                import torch.cuda.nvtx as nvtx
                nvtx.range_push(name) if push else nvtx.range_pop()
            except Exception:                                    # marker library absent: tracing is optional
                pass
        first_step = self.step
        fp_kw, fp_kw_accum = {}, {}
        if focus_present_mask is not None:
            fp_shard = torch.as_tensor(focus_present_mask).reshape(-1)[lo:hi]
            fp_kw, fp_kw_accum = {'focus_present_mask': fp_shard}, {'focus_present_masks': [fp_shard] * self.accum_steps}
        while self.step < self.train_num_steps:
            shard = [next(shards) for _ in range(self.accum_steps)] if self.apply_grad_args else next(shards)
            t0 = time.time()
            traced = self.device.type == 'cuda' and self.step - first_step < max(0, int(self.profile_flush_step))
            if traced:
                _range(True, f'train_step {self.step}')
            if self.cond_path is None:
                loss = self.train_step_accum(shard, self.step, **fp_kw_accum) if self.apply_grad_args else self.train_step(shard, self.step, **fp_kw)
            elif self.apply_grad_args:                           # the prefetcher hands (video, cond) pairs on
                loss = self.train_step_accum([s[0] for s in shard], self.step, conds=[s[1] for s in shard], **fp_kw_accum)
            else:
                loss = self.train_step(shard[0], self.step, cond=shard[1], **fp_kw)
            if traced:
                _range(False)
            if self.dist_on and self.world > 1:                  # global mean loss = mean of equal-size shard means (C2)
                dist.all_reduce(loss, op=dist.ReduceOp.SUM)
                loss = loss / self.world
            current_loss = float(loss.item())                    # device -> host sync every step, as trainer.py:581
            self._scalar('step_time', time.time() - t0, self.step)
            logging.info(f'Step: {self.step}/{self.train_num_steps} | Loss: {current_loss:.4f}')
            log_fn({'loss': current_loss, 'step': self.step})
            self._scalar('loss/train', current_loss, self.step)
            self._scalar('lr/train', self.current_lr(self.step), self.step)
            if self.apply_grad_args and (self.max_grad_norm is not None or self.track_grad_norm) and self.last_grad_norm is not None:
                self._scalar('grad_norm/train', float(self.last_grad_norm.item()), self.step)      # the host's only read of the norm
            if self.step > 0 and self.step % self.checkpoint_every_steps == 0:     # cadence: before step += 1 (trainer.py:593,604)
                logging.info(f'Step: {self.step} | Saving checkpoint...')
                self._save(self.step)
            self.step += 1
        logging.info('Training completed!')
        logging.info('Saving final checkpoint...')
        self._save(self.step)                                    # final save at train_num_steps (trainer.py:619-622)
        if self._scalars:
            self._scalars.flush()
