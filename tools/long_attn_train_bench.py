"""Train-step time above 64 x 64 frames: dim 64, 16 frames x 128 x 128, B 1, bf16 operands + bf16 activation storage, through the public
surface only (Trainer.train_step over a window of steps, device events).  The bottleneck spatial attention runs over 16 x 16 = 256 tokens
there; its backward core is the three launches of csrc/attn_long_bwd.hip (attn_long_bwd_stats / dkv / dq_kernel).  A second leg installs
the library's launch hook (vdx_set_launch_hook) for a few more steps and brackets those launches and the forward core
(attention_long_core_kernel) of the same steps with device events: per-launch medians, the backward core's share of the step.
Prints one JSON line.  Needs an MI355X."""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from video_diffusion_nnx_amd import _lib as L  # noqa: E402
from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion  # noqa: E402
from video_diffusion_nnx_amd.trainer import Trainer  # noqa: E402
from video_diffusion_nnx_amd.unet3d import Unet3D  # noqa: E402

BWD = ('attn_long_bwd_stats_kernel', 'attn_long_bwd_dkv_kernel', 'attn_long_bwd_dq_kernel')
FWD = 'attention_long_core_kernel'


class Info(C.Structure):
    _fields_ = [('kernel', C.c_char_p), ('shape', C.c_char_p), ('flops', C.c_double), ('bytes', C.c_double)]


HOOK = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.POINTER(Info), C.c_void_p)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--batch', type=int, default=1)
    ap.add_argument('--steps', type=int, default=10, help='train steps per timed window')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--hook-steps', type=int, default=5, help='steps with the launch hook installed')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    dev = torch.device('cuda:0')
    Fr, S, B = a.frames, a.size, a.batch
    unet = Unet3D(dim=a.dim, rngs=0, channels=1, mode='bf16', device=dev)
    gd = GaussianDiffusion(unet, image_size=S, num_frames=Fr, channels=1, timesteps=1000)
    tmp = tempfile.mkdtemp()
    out = {'shape': f'dim {a.dim}, {Fr}f x {S}x{S}, B {B}, bf16 operands + bf16 activation storage'}
    try:
        tr = Trainer(gd, tmp, dataset_path='synthetic:8', train_batch_size=B, train_num_steps=10 ** 6, train_lr=1e-4,
                     checkpoint_every_steps=10 ** 9, results_folder=os.path.join(tmp, 'res'))
        assert tr.train_act_bf16
        batch = torch.rand(B, 1, Fr, S, S, generator=torch.Generator().manual_seed(0)).to(dev)
        count = [0]

        def steps(n):
            for _ in range(n):
                loss = tr.train_step(batch, step=count[0])
                count[0] += 1
            return loss

        steps(3)
        windows = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loss = steps(a.steps)
            e1.record()
            e1.synchronize()
            windows.append(e0.elapsed_time(e1) / a.steps)
        assert torch.isfinite(loss).all()
        step_ms = statistics.median(windows)
        out['train_step_ms'] = round(step_ms, 3)
        out['train_step_ms_all'] = [round(x, 3) for x in windows]

        records, open_ev = [], []

        def hook(user, phase, info, stream):
            name = info.contents.kernel.decode()
            if name not in BWD and name != FWD:
                return
            e = torch.cuda.Event(enable_timing=True)
            e.record(torch.cuda.ExternalStream(stream) if stream else torch.cuda.current_stream(dev))
            if phase == 0:
                open_ev.append(e)
            else:
                records.append((name, info.contents.shape.decode(), open_ev.pop(), e))

        cb = HOOK(hook)
        set_hook = L._sig('vdx_set_launch_hook', None, [HOOK, C.c_void_p])
        set_hook(cb, None)
        try:
            steps(a.hook_steps)
            torch.cuda.synchronize(dev)
        finally:
            set_hook(C.cast(None, HOOK), None)
        per = {}
        for name, shape, e0, e1 in records:
            per.setdefault(name, []).append(e0.elapsed_time(e1))
        out['core_shape'] = sorted({s for _, s, _, _ in records})
        for name, xs in per.items():
            assert len(xs) == a.hook_steps, (name, len(xs))
            out[f'{name}_ms'] = round(statistics.median(xs), 4)
        bwd_ms = sum(statistics.median(per[k]) for k in BWD)
        out['backward_core_ms'] = round(bwd_ms, 4)
        out['backward_core_share_of_step'] = round(bwd_ms / step_ms, 5)
        out['forward_core_ms'] = round(statistics.median(per[FWD]), 4)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
