"""Cost of frame-conditioned sampling at the N shape (dim 64, 16f x 64 x 64, B 64, bf16 operands + bf16 activation storage, half the
frames known): the hipGraph-replayed DDPM step of GaussianDiffusion.inpaint (vdx_p_sample_loop_masked, U = 1) against that of
sample() (vdx_p_sample_loop_dyn), alternated, plus the reverse-step kernel alone (p_sample_masked_kernel vs p_sample_kernel), timed
with device events.  --clean-context: the masked step with the (1, 0) mask table of inpaint(clean_context=True).  Prints one JSON
line.  Needs an MI355X."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from video_diffusion_nnx_amd import _lib as L  # noqa: E402
from video_diffusion_nnx_amd.gaussian_diffusion import (GaussianDiffusion, frame_mask, vdx_inpaint_init, vdx_p_sample_loop_dyn,  # noqa: E402
                                                        vdx_p_sample_loop_masked, vdx_p_sample_step, vdx_p_sample_step_masked)
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
    ap.add_argument('--clean-context', action='store_true', help='the known frames stay clean: the (1, 0) mask table')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    B, Fr, S, T = a.batch, a.frames, a.size, 1000
    assert 2 * (1 + a.steps) * a.reps <= T
    dev = torch.device('cuda:0')
    unet = Unet3D(rngs=0, mode='bf16', dim=a.dim, channels=1)
    gd = GaussianDiffusion(unet, image_size=S, num_frames=Fr, channels=1, timesteps=T)
    h = unet.handle(Fr, S)
    unet.act_bf16 = True
    unet.apply_activation_storage(h)
    ws = unet.workspace(B, Fr, S)
    shape = (B, 1, Fr, S, S)
    per = Fr * S * S
    mtab = gd._mtab_clean if a.clean_context else gd._mtab
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        img = gd.randn(shape, 1, 0)
        known = 2 * torch.rand(shape, device=dev) - 1
        mask = frame_mask(torch.arange(Fr, device=dev) < Fr // 2, shape)
        L.check(vdx_inpaint_init(L.ptr(img), L.ptr(known), L.ptr(mask), L.ptr(mtab), T, T - 1, img.numel(), L.stream_ptr()))
        eps = torch.empty(B, Fr, S, S, 1, device=dev)
        t_dev = torch.full((B,), T - 1, dtype=torch.int32, device=dev)
        step = torch.zeros(1, dtype=torch.int64, device=dev)
        common = lambda: (L.ptr(unet.flat_params), L.ptr(unet.packed()), L.ptr(img), L.ptr(eps), L.ptr(t_dev), L.ptr(step), L.ptr(gd._ptab), T)

        def run(masked, n):
            if masked:
                L.check(vdx_p_sample_loop_masked(h.ptr, *common(), n, 0, 1, 1, 0.0, 0, L.ptr(known), L.ptr(mask), L.ptr(mtab), 1,
                                                 L.ptr(ws), ws.numel(), B, 1, L.stream_ptr()))
            else:
                L.check(vdx_p_sample_loop_dyn(h.ptr, *common(), n, 0, 1, 1, 0.0, 0, L.ptr(ws), ws.numel(), B, 1, L.stream_ptr()))

        def timed(fn, n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            return e0.elapsed_time(e1) / n

        for masked in (False, True):              # capture both graphs (own slots: neither evicts the other)
            run(masked, 2)
        st.synchronize()
        step_ms = {False: [], True: []}
        for _ in range(a.reps):
            for masked in (False, True):
                run(masked, 1)                     # the window starts on a replay of the cached graph
                step_ms[masked].append(timed(lambda: run(masked, a.steps), a.steps))
        out = torch.empty_like(img)
        kern = {
            False: lambda: L.check(vdx_p_sample_step(L.ptr(img), L.ptr(eps), L.ptr(out), L.ptr(t_dev), L.ptr(gd._ptab), T, 0, 1, 1, 0, 0, 1,
                                                     B, 1, per, L.stream_ptr())),
            True: lambda: L.check(vdx_p_sample_step_masked(L.ptr(img), L.ptr(eps), L.ptr(out), L.ptr(t_dev), L.ptr(gd._ptab), T, L.ptr(known),
                                                           L.ptr(mask), L.ptr(mtab), 1, 1, 0, 0, 0, 1, B, 1, per, L.stream_ptr())),
        }
        for masked in (False, True):
            kern[masked]()
        kern_us = {False: [], True: []}
        for _ in range(a.reps):
            for masked in (False, True):
                kern_us[masked].append(1e3 * timed(lambda: [kern[masked]() for _ in range(a.kernel_iters)], a.kernel_iters))
    med = {k: statistics.median(v) for k, v in step_ms.items()}
    kmed = {k: statistics.median(v) for k, v in kern_us.items()}
    n = B * per
    print(json.dumps({
        'shape': f'dim {a.dim}, B {B}, {Fr}f x {S}x{S}, bf16 operands + bf16 storage, {Fr // 2} frames known', 'clean_context': bool(a.clean_context),
        'step_ms_sample': round(med[False], 4), 'step_ms_inpaint': round(med[True], 4),
        'step_overhead_pct': round(100 * (med[True] - med[False]) / med[False], 3),
        'step_ms_all': {'sample': [round(v, 4) for v in step_ms[False]], 'inpaint': [round(v, 4) for v in step_ms[True]]},
        'kernel_us_p_sample': round(kmed[False], 2), 'kernel_us_p_sample_masked': round(kmed[True], 2),
        'kernel_tbps_p_sample': round(12 * n / kmed[False] / 1e6, 2), 'kernel_tbps_p_sample_masked': round(17 * n / kmed[True] / 1e6, 2),
    }))


if __name__ == '__main__':
    main()
