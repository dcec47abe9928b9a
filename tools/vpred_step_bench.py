"""Cost of the v-prediction objective (GaussianDiffusion(objective='pred_v')) at the north-star shape (dim 64, 16f x 64 x 64, bf16 operands),
through the public surface.  Sampling step (B 64, bf16 activation storage; GaussianDiffusion.p_sample_loop timed as the difference of a long
and a short chain, so capture and first-touch costs cancel): pred_noise, the ordinary ancestral step | pred_v (one v_to_eps_kernel launch
behind the forward).  Train step (B 4; Trainer.train_step over a window of steps, device events): pred_noise (loss_kernel +
loss_grad_kernel) | pred_v with min_snr_gamma = 5 (one v_loss_kernel pass and its final).  Kernels (leg `kernels`; device events around a
run of back-to-back launches, per launch): v_to_eps_kernel at the sampling shape, and at the train shape loss_weighted_kernel |
v_loss_kernel (both with their finals and the gradient).  The variants of a leg alternate window by window inside one process; every
figure comes with all its windows, the spread to read a difference against.  --legs sample,train,kernels picks the legs; --no-on times the
pred_noise variants only and uses nothing this feature added, so the same file measures an older checkout when it is copied into that
tree's tools/.  Prints one JSON line.  Needs an MI355X."""
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
from video_diffusion_nnx_amd import gaussian_diffusion as G  # noqa: E402
from video_diffusion_nnx_amd.unet3d import Unet3D  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--legs', default='sample,train,kernels')
    ap.add_argument('--no-on', action='store_true', help='pred_noise variants only (older checkouts)')
    ap.add_argument('--gamma', type=float, default=5.0)
    ap.add_argument('--batch', type=int, default=64, help='sampling batch')
    ap.add_argument('--train-batch', type=int, default=4)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--size', type=int, default=64)
    ap.add_argument('--short', type=int, default=4, help='steps of the short chain')
    ap.add_argument('--long', type=int, default=24, help='steps of the long chain')
    ap.add_argument('--train-steps', type=int, default=20, help='train steps per timed window')
    ap.add_argument('--launches', type=int, default=200, help='back-to-back launches per timed window of the kernels leg')
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    dev = torch.device('cuda:0')
    legs = a.legs.split(',')
    Fr, S = a.frames, a.size
    variants = ['pred_noise'] if a.no_on else ['pred_noise', 'pred_v']
    unet = Unet3D(dim=a.dim, rngs=0, channels=1, mode='bf16', device=dev)

    def diffusion(v, T):
        kw = dict(objective='pred_v', min_snr_gamma=a.gamma) if v == 'pred_v' else {}       # (gamma: the train leg's loss weights)
        return G.GaussianDiffusion(unet, image_size=S, num_frames=Fr, channels=1, timesteps=T, **kw)

    def alternate(window, names=None):
        names = names or variants
        got = {v: [] for v in names}
        for rep in range(a.reps):
            for v in (names if rep % 2 == 0 else names[::-1]):
                got[v].append(window(v))
        return got

    def report(out, leg, got, unit='step_ms'):
        for v, xs in got.items():
            out[f'{leg}_{unit}_{v}'] = round(statistics.median(xs), 4)
            out[f'{leg}_{unit}_{v}_all'] = [round(x, 4) for x in xs]

    out = {'shape': f'dim {a.dim}, {Fr}f x {S}x{S}, bf16 operands', 'gamma': a.gamma}
    if 'sample' in legs:
        B = a.batch

        def chain(T, v):
            gd = diffusion(v, T)
            gd.p_sample_loop((B,), key=1)                          # captures
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gd.p_sample_loop((B,), key=2)
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

        try:
            report(out, 'train', alternate(window))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        out['train_batch'] = B
    if 'kernels' in legs:
        from video_diffusion_nnx_amd import timestep_sampler as TS
        T, st = 1000, L.stream_ptr()
        gd = diffusion('pred_noise', T)
        sa, s1 = gd.sqrt_alphas_cumprod, gd.sqrt_one_minus_alphas_cumprod
        per = Fr * S * S

        def tensors(B):
            shape = (B, 1, Fr, S, S)
            return (torch.randn(shape, device=dev), torch.randn(shape, device=dev), torch.randn(B, Fr, S, S, 1, device=dev),
                    torch.empty(B, Fr, S, S, 1, device=dev), torch.full((B,), T // 2, dtype=torch.int32, device=dev))

        x, _, o, _, t = tensors(a.batch)
        x0, nz, net, d_out, tt = tensors(a.train_batch)
        Bt = a.train_batch
        res = torch.empty(Bt + 1, dtype=torch.float64, device=dev)
        scr = torch.empty(TS.vdx_loss_weighted_scratch_doubles(Bt), dtype=torch.float64, device=dev)
        calls = {'loss_weighted_kernel': lambda: TS.vdx_loss_weighted(L.ptr(net), L.ptr(nz), 0, L.ptr(d_out), L.ptr(scr), L.ptr(res), Bt, 1, per, 0, st)}
        if not a.no_on:
            wtab = torch.from_numpy(G.min_snr_weights(T, 'pred_v', a.gamma)).to(dev)
            calls['v_to_eps_kernel'] = lambda: L.vdx_v_to_eps(L.ptr(o), L.ptr(x), L.ptr(t), L.ptr(sa), L.ptr(s1), T, a.batch, 1, per, st)
            calls['v_loss_kernel'] = lambda: L.vdx_v_loss(L.ptr(net), L.ptr(x0), L.ptr(nz), L.ptr(tt), L.ptr(sa), L.ptr(s1), L.ptr(wtab), 0, T, 1, 2.0,
                                                          -1.0, 0, L.ptr(d_out), L.ptr(scr), L.ptr(res), Bt, 1, per, st)

        def span(name):
            for _ in range(10):
                L.check(calls[name]())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                L.check(calls[name]())
            e1.record()
            e1.synchronize()
            return 1e3 * e0.elapsed_time(e1) / a.launches           # microseconds per launch

        report(out, 'kernel', alternate(span, list(calls)), unit='us')
        out['kernel_shapes'] = dict(v_to_eps_kernel=[a.batch, 1, Fr, S, S], loss=[Bt, 1, Fr, S, S])
    print(json.dumps(out))


if __name__ == '__main__':
    main()
