"""Cost of one held-out evaluation step at the N shape (dim 64, 16f x 64 x 64, B 64, bf16 operands + bf16 activation storage): the
hipGraph-replayed step of GaussianDiffusion.calc_bpd_loop (vdx_vlb_loop: noise, forward, terms, advance) against the ancestral sampling
step (vdx_p_sample_loop: forward, p_sample, advance; the evaluation changes nothing in it), alternated windows, plus the two evaluation
kernels alone (back-to-back launches through the single-step C entries on pre-allocated buffers: per-launch time with the host's
issue in it, an upper bound of the kernel time), timed with device events.  Prints one JSON line.  Needs an MI355X."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from video_diffusion_nnx_amd import _lib as L  # noqa: E402
from video_diffusion_nnx_amd import ops  # noqa: E402
from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion, make_vlb_tables, vdx_p_sample_loop, vlb_time_sequence  # noqa: E402
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
    B, Fr, S, T = a.batch, a.frames, a.size, 1000
    assert 1 + a.steps <= T
    dev = torch.device('cuda:0')
    unet = Unet3D(rngs=0, mode='bf16', dim=a.dim, channels=1)
    gd = GaussianDiffusion(unet, image_size=S, num_frames=Fr, channels=1, timesteps=T)
    h = unet.handle(Fr, S)
    unet.act_bf16 = True
    unet.apply_activation_storage(h)
    ws = unet.workspace(B, Fr, S)
    shape = (B, 1, Fr, S, S)
    per = Fr * S * S
    seq_host = vlb_time_sequence(T)
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        img = gd.randn(shape, 1, 0)
        x = torch.rand(shape, device=dev)
        xt = torch.empty_like(x)
        tab = torch.from_numpy(make_vlb_tables(T)).to(dev)
        seq = torch.from_numpy(seq_host).to(dev)
        eps = torch.empty(B, Fr, S, S, 1, device=dev)
        t_dev = torch.full((B,), T - 1, dtype=torch.int32, device=dev)
        step = torch.zeros(1, dtype=torch.int64, device=dev)
        partial = torch.empty(L.vdx_vlb_scratch_doubles(B), dtype=torch.float64, device=dev)
        out = torch.empty(T, B, 3, dtype=torch.float64, device=dev)

        def run(vlb, n):
            if vlb:
                L.check(L.vdx_vlb_loop(h.ptr, L.ptr(unet.flat_params), L.ptr(unet.packed()), L.ptr(x), L.ptr(xt), L.ptr(eps), L.ptr(t_dev), L.ptr(step),
                                       L.ptr(tab), T, L.ptr(seq), T, n, 0, 3, 1, L.ptr(partial), L.ptr(out), L.ptr(ws), ws.numel(), B, 1, L.stream_ptr()))
            else:
                L.check(vdx_p_sample_loop(h.ptr, L.ptr(unet.flat_params), L.ptr(unet.packed()), L.ptr(img), L.ptr(eps), L.ptr(t_dev), L.ptr(step),
                                          L.ptr(gd._ptab), T, n, 0, 3, 1, L.ptr(ws), ws.numel(), B, 1, L.stream_ptr()))

        def restart():                              # every window walks the first 1 + steps levels: the step counter never leaves the sequence
            t_dev.fill_(T - 1)
            step.zero_()

        def timed(fn, n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            return e0.elapsed_time(e1) / n

        for vlb in (False, True):                   # capture both graphs (own slots: neither evicts the other)
            restart()
            run(vlb, 2)
        st.synchronize()
        step_ms = {False: [], True: []}
        for rep in range(a.reps):
            for vlb in ((False, True) if rep % 2 == 0 else (True, False)):
                restart()
                run(vlb, 1)                         # the window starts on a replay of the cached graph
                step_ms[vlb].append(timed(lambda: run(vlb, a.steps), a.steps))
        restart()
        # the single-step C entries on the buffers above: nothing is allocated between the events, each call is one ctypes call
        out3 = torch.empty(B, 3, dtype=torch.float64, device=dev)
        sp = L.stream_ptr()
        px, pxt, peps, pt, ptab, ppart, pout = (L.ptr(v) for v in (x, xt, eps, t_dev, tab, partial, out3))
        kern = {'noise': lambda: L.check(ops._vlb_noise(px, pxt, pt, ptab, T, 0, 3, 1, 0, B, per, sp)),
                'terms': lambda: L.check(ops._vlb_terms(px, peps, pt, ptab, T, 0, 3, 1, 0, 1, ppart, pout, B, 1, per, sp))}
        kern_us = {k: [] for k in kern}
        for k, fn in kern.items():
            fn()
        for rep in range(a.reps):
            for k, fn in kern.items():
                kern_us[k].append(1e3 * timed(lambda: [fn() for _ in range(a.kernel_iters)], a.kernel_iters))
    med = {k: statistics.median(v) for k, v in step_ms.items()}
    kmed = {k: statistics.median(v) for k, v in kern_us.items()}
    spread = lambda v: round(100 * (max(v) - min(v)) / statistics.median(v), 3)
    print(json.dumps({
        'shape': f'dim {a.dim}, B {B}, {Fr}f x {S}x{S}, bf16 operands + bf16 storage, T {T}',
        'step_ms_sample': round(med[False], 4), 'step_ms_vlb': round(med[True], 4),
        'step_overhead_pct': round(100 * (med[True] - med[False]) / med[False], 3),
        'spread_pct': {'sample': spread(step_ms[False]), 'vlb': spread(step_ms[True])},
        'step_ms_all': {'sample': [round(v, 4) for v in step_ms[False]], 'vlb': [round(v, 4) for v in step_ms[True]]},
        'launch_us_vlb_noise': round(kmed['noise'], 2), 'launch_us_vlb_terms_with_advance': round(kmed['terms'], 2),
        'launch_tbps_vlb_noise': round(8 * B * per / kmed['noise'] / 1e6, 2), 'launch_tbps_vlb_terms': round(8 * B * per / kmed['terms'] / 1e6, 2),
    }))


if __name__ == '__main__':
    main()
