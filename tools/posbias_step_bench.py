"""Cost of the temporal relative position bias (Unet3D.temporal_pos_bias) at the north-star shape (dim 64, 16f x 64 x 64, bf16 operands),
through the public surface only: the sampling step (B 64, bf16 activation storage; GaussianDiffusion.p_sample_loop timed as the difference
of a long and a short chain, so capture and first-touch costs cancel) and the train step (B 4; Trainer.train_step over a window of steps,
device events), switch off and on, alternated window by window inside one process.  --legs sample,train picks the legs; --no-on times the
switch-off legs only and uses nothing this feature added, so the same file measures an older checkout when it is copied into that tree's
tools/.  Prints one JSON line.  Needs an MI355X."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion  # noqa: E402
from video_diffusion_nnx_amd.unet3d import Unet3D  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--legs', default='sample,train')
    ap.add_argument('--no-on', action='store_true', help='switch-off legs only (older checkouts)')
    ap.add_argument('--batch', type=int, default=64, help='sampling batch')
    ap.add_argument('--train-batch', type=int, default=4)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--size', type=int, default=64)
    ap.add_argument('--short', type=int, default=4, help='steps of the short chain')
    ap.add_argument('--long', type=int, default=24, help='steps of the long chain')
    ap.add_argument('--train-steps', type=int, default=20, help='train steps per timed window')
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    dev = torch.device('cuda:0')
    variants = [False] if a.no_on else [False, True]
    legs = a.legs.split(',')
    Fr, S = a.frames, a.size
    unet = Unet3D(dim=a.dim, rngs=0, channels=1, mode='bf16', device=dev)

    def switch(on):
        if on or not a.no_on:
            unet.temporal_pos_bias = on

    def alternate(window):
        got = {v: [] for v in variants}
        for rep in range(a.reps):
            for on in (variants if rep % 2 == 0 else variants[::-1]):
                switch(on)
                got[on].append(window())
        return got

    out = {'shape': f'dim {a.dim}, {Fr}f x {S}x{S}, bf16 operands'}
    if 'sample' in legs:
        B = a.batch

        def chain(T):
            gd = GaussianDiffusion(unet, image_size=S, num_frames=Fr, channels=1, timesteps=T)
            gd.p_sample_loop((B,), key=1)                         # captures (or re-captures after a switch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gd.p_sample_loop((B,), key=2)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        got = alternate(lambda: 1e3 * (chain(a.long) - chain(a.short)) / (a.long - a.short))
        for on, v in got.items():
            out[f'sample_step_ms_{"on" if on else "off"}'] = round(statistics.median(v), 4)
            out[f'sample_step_ms_{"on" if on else "off"}_all'] = [round(x, 4) for x in v]
        out['sample_batch'] = B
    if 'train' in legs:
        from video_diffusion_nnx_amd.trainer import Trainer
        B = a.train_batch
        gd = GaussianDiffusion(unet, image_size=S, num_frames=Fr, channels=1, timesteps=1000)
        tmp = tempfile.mkdtemp()
        tr = Trainer(gd, tmp, dataset_path=f'synthetic:{S}', train_batch_size=B, train_num_steps=10 ** 6, train_lr=1e-4,
                     checkpoint_every_steps=10 ** 9, results_folder=os.path.join(tmp, 'res'))
        batch = torch.rand(B, 1, Fr, S, S, generator=torch.Generator().manual_seed(0)).to(dev)
        count = [0]

        def steps(n):
            for _ in range(n):
                tr.train_step(batch, step=count[0])
                count[0] += 1

        def window():
            steps(3)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            steps(a.train_steps)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / a.train_steps

        try:
            got = alternate(window)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        for on, v in got.items():
            out[f'train_step_ms_{"on" if on else "off"}'] = round(statistics.median(v), 4)
            out[f'train_step_ms_{"on" if on else "off"}_all'] = [round(x, 4) for x in v]
        out['train_batch'] = B
    print(json.dumps(out))


if __name__ == '__main__':
    main()
