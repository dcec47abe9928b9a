"""Cost of a DPM-Solver++(2M) step at the N shape (dim 64, 16f x 64 x 64, B 64, bf16 operands + bf16 activation storage): the
hipGraph-replayed step of GaussianDiffusion.dpm_sample_loop (vdx_dpm_sample_loop, order 2) against that of ddim_sample_loop
(vdx_ddim_sample_loop_dyn), alternated, plus the step kernel alone (dpm_step_kernel vs ddim_step_kernel), timed with device events.
Both chains run over the same 100-entry time sequence.  Prints one JSON line.  Needs an MI355X."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from video_diffusion_nnx_amd import _lib as L  # noqa: E402
from video_diffusion_nnx_amd.gaussian_diffusion import (GaussianDiffusion, ddim_time_sequence, vdx_ddim_sample_loop_dyn, vdx_ddim_step,  # noqa: E402
                                                        vdx_dpm_sample_loop, vdx_dpm_step)
from video_diffusion_nnx_amd.unet3d import Unet3D  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--size', type=int, default=64)
    ap.add_argument('--steps', type=int, default=20, help='replayed steps per timed window')
    ap.add_argument('--reps', type=int, default=5, help='alternating windows per variant')
    ap.add_argument('--kernel-iters', type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    B, Fr, S, T, N = a.batch, a.frames, a.size, 1000, 100
    assert 1 + a.steps <= N
    dev = torch.device('cuda:0')
    unet = Unet3D(rngs=0, mode='bf16', dim=a.dim, channels=1)
    gd = GaussianDiffusion(unet, image_size=S, num_frames=Fr, channels=1, timesteps=T)
    h = unet.handle(Fr, S)
    unet.act_bf16 = True
    unet.apply_activation_storage(h)
    ws = unet.workspace(B, Fr, S)
    shape = (B, 1, Fr, S, S)
    per = Fr * S * S
    seq_host = ddim_time_sequence(T, N)
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        img = gd.randn(shape, 1, 0)
        hist = torch.zeros_like(img)
        seq = torch.from_numpy(seq_host).to(dev)
        eps = torch.empty(B, Fr, S, S, 1, device=dev)
        t_dev = torch.full((B,), int(seq_host[0]), dtype=torch.int32, device=dev)
        step = torch.zeros(1, dtype=torch.int64, device=dev)

        def run(dpm, n):
            if dpm:
                L.check(vdx_dpm_sample_loop(h.ptr, L.ptr(unet.flat_params), L.ptr(unet.packed()), L.ptr(img), L.ptr(eps), L.ptr(hist), L.ptr(t_dev),
                                            L.ptr(step), L.ptr(gd.alphas_cumprod), L.ptr(seq), N, n, 0, 1, 2, 0, 0, 0.0, 0, L.ptr(ws), ws.numel(),
                                            B, 1, L.stream_ptr()))
            else:
                L.check(vdx_ddim_sample_loop_dyn(h.ptr, L.ptr(unet.flat_params), L.ptr(unet.packed()), L.ptr(img), L.ptr(eps), L.ptr(t_dev),
                                                 L.ptr(step), L.ptr(gd.alphas_cumprod), L.ptr(seq), N, n, 0, 1, 0, 0, 0.0, 0, L.ptr(ws), ws.numel(),
                                                 B, 1, L.stream_ptr()))

        def restart():                              # every window walks seq[0 .. 1 + steps]: the step counter never leaves the sequence
            t_dev.fill_(int(seq_host[0]))
            step.zero_()

        def timed(fn, n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            return e0.elapsed_time(e1) / n

        for dpm in (False, True):                   # capture both graphs (own slots: neither evicts the other)
            restart()
            run(dpm, 2)
        st.synchronize()
        step_ms = {False: [], True: []}
        for rep in range(a.reps):
            for dpm in ((False, True) if rep % 2 == 0 else (True, False)):
                restart()
                run(dpm, 1)                         # the window starts on a replay of the cached graph
                step_ms[dpm].append(timed(lambda: run(dpm, a.steps), a.steps))
        out = torch.empty_like(img)
        step.fill_(5)                               # a second-order step
        kern = {
            False: lambda: L.check(vdx_ddim_step(L.ptr(img), L.ptr(eps), L.ptr(out), L.ptr(gd.alphas_cumprod), L.ptr(seq), L.ptr(step), 0, 1,
                                                 B, 1, per, L.stream_ptr())),
            True: lambda: L.check(vdx_dpm_step(L.ptr(img), L.ptr(eps), L.ptr(out), L.ptr(hist), L.ptr(gd.alphas_cumprod), L.ptr(seq), L.ptr(step), 0, 1,
                                               2, B, 1, per, L.stream_ptr())),
        }
        for dpm in (False, True):
            kern[dpm]()
        kern_us = {False: [], True: []}
        for rep in range(a.reps):
            for dpm in ((False, True) if rep % 2 == 0 else (True, False)):
                kern_us[dpm].append(1e3 * timed(lambda: [kern[dpm]() for _ in range(a.kernel_iters)], a.kernel_iters))
    med = {k: statistics.median(v) for k, v in step_ms.items()}
    kmed = {k: statistics.median(v) for k, v in kern_us.items()}
    n = B * per
    print(json.dumps({
        'shape': f'dim {a.dim}, B {B}, {Fr}f x {S}x{S}, bf16 operands + bf16 storage, 100-entry sequence',
        'step_ms_ddim': round(med[False], 4), 'step_ms_dpm': round(med[True], 4),
        'step_overhead_pct': round(100 * (med[True] - med[False]) / med[False], 3),
        'step_ms_all': {'ddim': [round(v, 4) for v in step_ms[False]], 'dpm': [round(v, 4) for v in step_ms[True]]},
        'kernel_us_ddim_step': round(kmed[False], 2), 'kernel_us_dpm_step': round(kmed[True], 2),
        'kernel_tbps_ddim_step': round(12 * n / kmed[False] / 1e6, 2), 'kernel_tbps_dpm_step': round(20 * n / kmed[True] / 1e6, 2),
    }))


if __name__ == '__main__':
    main()
