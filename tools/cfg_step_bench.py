"""Cost of one guided (classifier-free guidance) ancestral step at the BASELINE.json configs[4] shape (dim 64, cond_dim 768, 16f x 64 x 64,
B 32 -> one forward over 64 samples per step, bf16 operands + bf16 activation storage), through the public surface only:
GaussianDiffusion.p_sample_loop(shape, key, cond=, cond_scale=2) timed as the difference of a long and a short chain (capture and
first-touch costs cancel, as bench.py's configs[4] leg does), repeated --reps times.  With --rescale PHI the same with
guidance_rescale=PHI next to it, alternated.  Uses nothing this commit added unless --rescale is given, so the same file measures an
older checkout (where the guided loop runs step by step from Python) when it is copied into that tree's tools/.  Prints one JSON line.
Needs an MI355X."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion  # noqa: E402
from video_diffusion_nnx_amd.unet3d import Unet3D  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--size', type=int, default=64)
    ap.add_argument('--short', type=int, default=4, help='steps of the short chain')
    ap.add_argument('--long', type=int, default=24, help='steps of the long chain')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rescale', type=float, default=None, help='also time guidance_rescale=PHI')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    B, Fr, S = a.batch, a.frames, a.size
    dev = torch.device('cuda:0')
    unet = Unet3D(dim=a.dim, rngs=0, channels=1, cond_dim=768, mode='bf16', device=dev)
    cond = torch.randn(B, 768, generator=torch.Generator().manual_seed(0)).to(dev)
    shape = (B, 1, Fr, S, S)
    gds = {T: GaussianDiffusion(unet, image_size=S, num_frames=Fr, channels=1, timesteps=T) for T in (a.short, a.long)}
    variants = {'guided': {}}
    if a.rescale is not None:
        variants['rescale'] = dict(guidance_rescale=a.rescale)

    def timed(T, kw):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = gds[T].p_sample_loop(shape, 1, cond=cond, cond_scale=2.0, **kw)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        assert torch.isfinite(out).all()
        return dt

    for kw in variants.values():                      # warm-up: packing, workspace, capture
        for T in gds:
            timed(T, kw)
    ms = {k: [] for k in variants}
    for rep in range(a.reps):
        names = list(variants) if rep % 2 == 0 else list(variants)[::-1]
        for name in names:
            ts = {T: timed(T, variants[name]) for T in gds}
            ms[name].append((ts[a.long] - ts[a.short]) / (a.long - a.short) * 1e3)
    out = {'shape': f'dim {a.dim}, cond_dim 768, B {B} (2B = {2 * B} per forward), {Fr}f x {S}x{S}, bf16 operands + bf16 storage, cond_scale 2',
           'chains': [a.short, a.long]}
    for name, v in ms.items():
        out[f'step_ms_{name}'] = round(statistics.median(v), 4)
        out[f'step_ms_{name}_all'] = [round(x, 4) for x in v]
    print(json.dumps(out))


if __name__ == '__main__':
    main()
