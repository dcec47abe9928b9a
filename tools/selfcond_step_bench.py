"""Cost of self-conditioning (GaussianDiffusion(self_condition=True)) at the north-star shape (dim 64, 16f x 64 x 64, bf16 operands,
3 colour channels), through the public surface only.  Sampling step (B 64, bf16 activation storage; timed as the difference of a long
and a short chain, so capture and first-touch costs cancel): the self-conditioned step | the same network with channels = 6, out_dim = 3
with the state off (a super-resolution diffusion with factors (1, 1): the same lowres_pack copy and stem, no selfcond_x0 launch) | the
ordinary step of a 3-channel network (what the 6-channel stem and the pack cost together).  Train step (B 4; Trainer.train_step over a
window of steps, device events) at self_cond_prob 0 / 0.5 / 1: no first pass | one every other step on average | one in every step.  The
new kernel on its own (vdx_selfcond_x0 at the sampling batch, device events over a window of launches, against the bytes it moves).  The
variants of a leg alternate window by window inside one process.  --legs sample,train,kernel picks the legs.  Prints one JSON line.  Needs
an MI355X."""
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

from video_diffusion_nnx_amd import _lib as L  # noqa: E402
from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion  # noqa: E402
from video_diffusion_nnx_amd.unet3d import Unet3D  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--legs', default='sample,train,kernel')
    ap.add_argument('--batch', type=int, default=64, help='sampling batch')
    ap.add_argument('--train-batch', type=int, default=4)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--channels', type=int, default=3)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--size', type=int, default=64)
    ap.add_argument('--short', type=int, default=4, help='steps of the short chain')
    ap.add_argument('--long', type=int, default=24, help='steps of the long chain')
    ap.add_argument('--train-steps', type=int, default=20, help='train steps per timed window')
    ap.add_argument('--kernel-launches', type=int, default=200, help='launches per timed window of the kernel leg')
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    dev = torch.device('cuda:0')
    legs = a.legs.split(',')
    Fr, S, C = a.frames, a.size, a.channels
    wide = Unet3D(dim=a.dim, rngs=0, channels=2 * C, out_dim=C, mode='bf16', device=dev)
    narrow = Unet3D(dim=a.dim, rngs=0, channels=C, mode='bf16', device=dev)

    def diffusion(v, T):
        kw = {'on': dict(self_condition=True), 'off': dict(lowres_cond=(1, 1)), 'plain': {}}[v]
        return GaussianDiffusion(narrow if v == 'plain' else wide, image_size=S, num_frames=Fr, channels=C, timesteps=T, **kw)

    def alternate(variants, window):
        got = {v: [] for v in variants}
        for rep in range(a.reps):
            for v in (variants if rep % 2 == 0 else variants[::-1]):
                got[v].append(window(v))
        return got

    def report(out, leg, got, digits=4):
        for v, xs in got.items():
            out[f'{leg}_ms_{v}'] = round(statistics.median(xs), digits)
            out[f'{leg}_ms_{v}_all'] = [round(x, digits) for x in xs]

    out = {'shape': f'dim {a.dim}, {Fr}f x {S}x{S}, {C} channels, bf16 operands'}
    if 'sample' in legs:
        B = a.batch
        lo = torch.full((B, C, Fr, S, S), 0.5, device=dev)                 # u = up(2 * 0.5 - 1) = 0: the state-off chain of the same network

        def chain(T, v):
            gd = diffusion(v, T)
            run = {'on': lambda key: gd.p_sample_loop((B,), key=key), 'off': lambda key: gd.upsample(key, lo),
                   'plain': lambda key: gd.p_sample_loop((B,), key=key)}[v]
            run(1)                                                 # captures
            run(1)                                                 # (the graph key holds the seed: the timed call below replays)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(1)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        report(out, 'sample_step', alternate(['on', 'off', 'plain'], lambda v: 1e3 * (chain(a.long, v) - chain(a.short, v)) / (a.long - a.short)))
        out['sample_batch'] = B
    if 'train' in legs:
        from video_diffusion_nnx_amd.trainer import Trainer
        B = a.train_batch
        tmp = tempfile.mkdtemp()
        tr = Trainer(diffusion('on', 1000), tmp, dataset_path=f'synthetic:{S}', train_batch_size=B, train_num_steps=10 ** 6, train_lr=1e-4,
                     checkpoint_every_steps=10 ** 9, results_folder=os.path.join(tmp, 'res'))
        batch = torch.rand(B, C, Fr, S, S, generator=torch.Generator().manual_seed(0)).to(dev)
        count = [0]
        passes = {}

        def window(p):
            tr.self_cond_prob = float(p)

            def steps(n):
                first = 0
                for _ in range(n):
                    tr.train_step(batch, step=count[0])
                    first += int(bool(tr.last_self_cond))
                    count[0] += 1
                return first
            steps(3)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            first = steps(a.train_steps)
            e1.record()
            e1.synchronize()
            passes.setdefault(p, []).append(first)
            return e0.elapsed_time(e1) / a.train_steps

        try:
            report(out, 'train_step', alternate(['0', '0.5', '1'], window))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        out['train_batch'] = B
        out['train_first_passes_per_window'] = {p: n for p, n in passes.items()}       # (of --train-steps steps: the coin's share at 0.5)
    if 'kernel' in legs:
        B, per = a.batch, C * Fr * S * S
        gd = diffusion('on', 1000)
        g = torch.Generator().manual_seed(0)
        x = torch.randn(B, C, Fr, S, S, generator=g).to(dev)
        eps = torch.randn(B, Fr, S, S, C, generator=g).to(dev)
        t = torch.randint(0, 1000, (B,), generator=g, dtype=torch.int32).to(dev)
        xin = torch.zeros(B, 2 * C, Fr, S, S, device=dev)
        st = L.stream_ptr()

        def window(_):
            launch = lambda: L.check(L.vdx_selfcond_x0(L.ptr(x), per, L.ptr(eps), L.ptr(t), L.ptr(gd._ptab), 1000, 0, 1, L.ptr(xin), B, C, per, st))
            for _ in range(10):
                launch()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.kernel_launches):
                launch()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / a.kernel_launches

        report(out, 'kernel', alternate(['selfcond_x0'], window), digits=5)
        out['kernel_bytes'] = 12 * B * per
        out['kernel_gb_per_s'] = round(12 * B * per / (out['kernel_ms_selfcond_x0'] * 1e-3) / 1e9, 1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
