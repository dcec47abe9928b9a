"""Cost of loss-aware timestep sampling (Trainer.timestep_sampler = 'loss-second-moment') on the train step at the north-star shape (dim 64,
16f x 64 x 64, bf16 operands + bf16 storage, B 4), through the public surface only: Trainer.train_step over a window of steps between device
events, the sampler off | on (history preloaded warm, so the weighted draw, the binary search and the shifting update all run).  The two
variants alternate window by window inside one process.  --no-on times the uniform step only and uses nothing this feature added, so the
same file measures an older checkout when it is copied into that tree's tools/.  --launches adds the device time of each of the three new
launches on their own (vdx_tsampler_draw, vdx_loss_weighted, vdx_tsampler_update; events around back-to-back repeats), to say which one
carries a difference.  Prints one JSON line.  Needs an MI355X."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion  # noqa: E402
from video_diffusion_nnx_amd.trainer import Trainer  # noqa: E402
from video_diffusion_nnx_amd.unet3d import Unet3D  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--no-on', action='store_true', help='the uniform step only (older checkouts)')
    ap.add_argument('--launches', action='store_true', help='also time the three new launches on their own')
    ap.add_argument('--train-batch', type=int, default=4)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--size', type=int, default=64)
    ap.add_argument('--timesteps', type=int, default=1000)
    ap.add_argument('--train-steps', type=int, default=20, help='train steps per timed window')
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    dev = torch.device('cuda:0')
    Fr, S, B, T = a.frames, a.size, a.train_batch, a.timesteps
    variants = ['off'] if a.no_on else ['off', 'on']
    tmp = tempfile.mkdtemp()
    trs = {}
    for v in variants:
        os.makedirs(os.path.join(tmp, v))
        if v == 'on':
            Trainer.timestep_sampler = 'loss-second-moment'
        try:
            gd = GaussianDiffusion(Unet3D(dim=a.dim, rngs=0, channels=1, mode='bf16', device=dev), image_size=S, num_frames=Fr, channels=1,
                                   timesteps=T)
            trs[v] = Trainer(gd, os.path.join(tmp, v), dataset_path=f'synthetic:{S}', train_batch_size=B, train_num_steps=10 ** 6,
                             train_lr=1e-4, checkpoint_every_steps=10 ** 9, results_folder=os.path.join(tmp, v, 'res'))
        finally:
            if v == 'on':
                Trainer.timestep_sampler = 'uniform'
    if 'on' in trs:
        smp = trs['on'].sampler
        g = torch.Generator().manual_seed(1)
        smp.load_state(torch.rand(T, smp.history_per_term, generator=g, dtype=torch.float64) + 0.01,
                       torch.full((T,), smp.history_per_term, dtype=torch.int32))
        assert smp.warm
    batch = torch.rand(B, 1, Fr, S, S, generator=torch.Generator().manual_seed(0)).to(dev)
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

    out = {'shape': f'dim {a.dim}, {Fr}f x {S}x{S}, bf16 operands', 'train_batch': B, 'timesteps': T}
    try:
        got = {v: [] for v in variants}
        for rep in range(a.reps):
            for v in (variants if rep % 2 == 0 else variants[::-1]):
                got[v].append(window(v))
        for v, xs in got.items():
            out[f'train_step_ms_{v}'] = round(statistics.median(xs), 4)
            out[f'train_step_ms_{v}_all'] = [round(x, 4) for x in xs]
        if 'on' in trs:
            assert trs['on'].sampler.warm and bool(torch.isfinite(trs['on'].last_iw).all())
        if a.launches and 'on' in trs:
            from video_diffusion_nnx_amd.timestep_sampler import loss_weighted
            tr = trs['on']
            eps_hat = torch.randn(B, Fr, S, S, 1, device=dev)
            noise = torch.randn(B, 1, Fr, S, S, device=dev)
            t, iw = tr.sampler.draw(B, 1)
            entries = torch.stack([t.double(), torch.rand(B, device=dev, dtype=torch.float64)], 1).contiguous()

            def timed(fn, n=200):
                fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    fn()
                e1.record()
                e1.synchronize()
                return round(1e3 * e0.elapsed_time(e1) / n, 2)
            # the same three, inside real train steps: device events around each call site (the launch plus what it waits for on the stream)
            # (the weighted objective is GaussianDiffusion.loss_and_grad's call of timestep_sampler.loss_weighted, looked up on the module)
            from video_diffusion_nnx_amd import timestep_sampler as TSMOD
            spans = {'tsampler_draw': [], 'loss_weighted': [], 'tsampler_update': []}

            def spanned(name, fn):
                def wrapper(*args, **kw):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    r = fn(*args, **kw)
                    e1.record()
                    spans[name].append((e0, e1))
                    return r
                return wrapper
            keep = tr.sampler.draw, tr.sampler.update, TSMOD.loss_weighted
            tr.sampler.draw, tr.sampler.update = spanned('tsampler_draw', keep[0]), spanned('tsampler_update', keep[1])
            TSMOD.loss_weighted = spanned('loss_weighted', keep[2])
            try:
                for _ in range(a.train_steps):
                    tr.train_step(batch, step=count['on'])
                    count['on'] += 1
                torch.cuda.synchronize()
            finally:
                tr.sampler.draw, tr.sampler.update, TSMOD.loss_weighted = keep
            out['in_step_us'] = {k: round(1e3 * statistics.median(e0.elapsed_time(e1) for e0, e1 in v), 2) for k, v in spans.items()}
            from video_diffusion_nnx_amd import _lib as L
            from video_diffusion_nnx_amd.train_step import vdx_loss_grad, vdx_loss_sum
            lb = torch.rand(B, device=dev, dtype=torch.float64)
            t_host = torch.randint(0, T, (B,), dtype=torch.int32)

            def uniform_pair():                                    # what the sampler's pass replaces: loss_kernel + loss_grad_kernel and their glue
                acc = torch.zeros(1, dtype=torch.float64, device=dev)
                d_eps = torch.empty_like(eps_hat)
                L.check(vdx_loss_sum(L.ptr(eps_hat), L.ptr(noise), L.ptr(acc), B, 1, Fr * S * S, 0, L.stream_ptr()))
                (acc / float(noise.numel())).to(torch.float32).reshape(())
                L.check(vdx_loss_grad(L.ptr(eps_hat), L.ptr(noise), L.ptr(d_eps), B, 1, Fr * S * S, 0, L.stream_ptr()))

            def weighted_pass():
                o, _ = loss_weighted(eps_hat, noise, iw, l2=False)
                o[B].to(torch.float32).reshape(())
            out['launch_us'] = {'tsampler_draw': timed(lambda: tr.sampler.draw(B, 1)),
                                'loss_weighted': timed(lambda: loss_weighted(eps_hat, noise, iw, l2=False)),
                                'tsampler_update': timed(lambda: tr.sampler.update(entries)),
                                # with the torch glue of forward_backward around them, and the pieces of the uniform step they replace
                                'on_loss_pass_with_glue': timed(weighted_pass),
                                'on_entries_and_update': timed(lambda: tr.sampler.update(torch.stack([t.to(torch.float64), lb], 1).contiguous())),
                                'off_loss_pair_with_glue': timed(uniform_pair),
                                'off_t_upload': timed(lambda: t_host.pin_memory().to(dev, non_blocking=True))}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
