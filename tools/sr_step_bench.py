"""Cost of the second stage of a cascade (GaussianDiffusion(lowres_cond=(ft, fs))) at the north-star shape (dim 64, 16f x 64 x 64, bf16
operands, 3 colour channels), through the public surface only.  Sampling step (B 64, bf16 activation storage; timed as the difference of
a long and a short chain, so capture, the one lowres_input launch and first-touch costs cancel): the ordinary ancestral step of a
3-channel network (p_sample_loop) | the super-resolution step of a network with channels = 6, out_dim = 3 (upsample: one lowres_pack copy
per step, and the stem conv reads 6 channels).  Train step (B 4; Trainer.train_step over a window of steps, device events): q_sample and
the 3-channel stem | lowres_down + lowres_input and the 6-channel stem with its weight gradient.  The variants of a leg alternate window
by window inside one process.  --legs sample,train picks the legs; --no-on times the ordinary variants only and uses nothing this feature
added, so the same file measures an older checkout when it is copied into that tree's tools/.  Prints one JSON line.  Needs an MI355X."""
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
    ap.add_argument('--no-on', action='store_true', help='ordinary variants only (older checkouts)')
    ap.add_argument('--batch', type=int, default=64, help='sampling batch')
    ap.add_argument('--train-batch', type=int, default=4)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--channels', type=int, default=3)
    ap.add_argument('--temporal', type=int, default=1, help='temporal factor ft of the second stage')
    ap.add_argument('--spatial', type=int, default=4, help='spatial factor fs of the second stage')
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--size', type=int, default=64)
    ap.add_argument('--short', type=int, default=4, help='steps of the short chain')
    ap.add_argument('--long', type=int, default=24, help='steps of the long chain')
    ap.add_argument('--train-steps', type=int, default=20, help='train steps per timed window')
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    dev = torch.device('cuda:0')
    legs = a.legs.split(',')
    Fr, S = a.frames, a.size
    C = a.channels
    variants = ['plain'] if a.no_on else ['plain', 'superres']
    unets = {'plain': Unet3D(dim=a.dim, rngs=0, channels=C, mode='bf16', device=dev)}
    if not a.no_on:
        unets['superres'] = Unet3D(dim=a.dim, rngs=0, channels=2 * C, out_dim=C, mode='bf16', device=dev)

    def diffusion(v, T):
        kw = dict(lowres_cond=(a.temporal, a.spatial), lowres_aug_max=T) if v == 'superres' else {}
        return GaussianDiffusion(unets[v], image_size=S, num_frames=Fr, channels=C, timesteps=T, **kw)

    def alternate(window):
        got = {v: [] for v in variants}
        for rep in range(a.reps):
            for v in (variants if rep % 2 == 0 else variants[::-1]):
                got[v].append(window(v))
        return got

    def report(out, leg, got):
        for v, xs in got.items():
            out[f'{leg}_step_ms_{v}'] = round(statistics.median(xs), 4)
            out[f'{leg}_step_ms_{v}_all'] = [round(x, 4) for x in xs]

    out = {'shape': f'dim {a.dim}, {Fr}f x {S}x{S}, {C} channels, bf16 operands, factors ({a.temporal}, {a.spatial})'}
    if 'sample' in legs:
        B = a.batch

        lo = torch.rand(B, C, Fr // a.temporal, S // a.spatial, S // a.spatial, generator=torch.Generator().manual_seed(0)).to(dev)

        def chain(T, v):
            gd = diffusion(v, T)
            run = (lambda key: gd.upsample(key, lo)) if v == 'superres' else (lambda key: gd.p_sample_loop((B,), key=key))
            run(1)                                                 # captures
            run(1)                                                 # (the graph key holds the seed: the timed call below replays)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(1)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        report(out, 'sample', alternate(lambda v: 1e3 * (chain(a.long, v) - chain(a.short, v)) / (a.long - a.short)))
        out['sample_batch'] = B
    if 'train' in legs:
        from video_diffusion_nnx_amd.trainer import Trainer
        B = a.train_batch
        tmp = tempfile.mkdtemp()
        for v in variants:
            os.makedirs(os.path.join(tmp, v))
        trs = {v: Trainer(diffusion(v, 1000), os.path.join(tmp, v), dataset_path=f'synthetic:{S}', train_batch_size=B, train_num_steps=10 ** 6,
                          train_lr=1e-4, checkpoint_every_steps=10 ** 9, results_folder=os.path.join(tmp, v, 'res')) for v in variants}
        batch = torch.rand(B, C, Fr, S, S, generator=torch.Generator().manual_seed(0)).to(dev)
        count = {v: 0 for v in variants}

        def window(v):
            def steps(n):
                for _ in range(n):
                    trs[v].train_step(batch, step=count[v])
                    count[v] += 1
            steps(3)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            steps(a.train_steps)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / a.train_steps

        try:
            report(out, 'train', alternate(window))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        out['train_batch'] = B
    print(json.dumps(out))


if __name__ == '__main__':
    main()
