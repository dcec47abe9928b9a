"""CPU tests of the sampling-loop entry points' first checks: a null handle or a null required pointer is VDX_ERR_INVALID, whatever
else the call holds, and comes before the look at the handle's device state -- so these calls touch no device."""
import ctypes

from _sample_loop_sigs import SIGS, fn

INVALID, STATE = -1, -4
REQUIRED = {'p': 'h params packed img eps t_dev step_dev tables ws', 'seq': 'h params packed img eps t_dev step_dev ac seq ws'}
SCALARS = dict(timesteps=60, seq_len=12, nsteps=1, seed=3, clip=1, order=2, percentile=0.0, resample=1, cond_scale=2.0, rescale=0.0,
               ws_bytes=1 << 20, batch=2, use_graph=0, stream=0)


def _handle():
    from video_diffusion_nnx_amd.unet3d import Unet3D
    unet = Unet3D(rngs=0, mode='f32', dim=16, channels=1, dim_mults=(1, 2), cond_dim=32, device='cpu')
    return unet, unet.handle(4, 8)


def test_null_handle_and_null_pointers_are_invalid():
    import torch
    from video_diffusion_nnx_amd import _lib as L
    unet, h = _handle()
    host = (ctypes.c_double * 64)()                                    # stands in for every buffer: no row here gets as far as reading one
    buf = ctypes.addressof(host)
    for entry, sig in SIGS.items():
        names = sig.split()
        base = {n: SCALARS.get(n, buf) for n in names}
        base['h'] = h.ptr
        required = REQUIRED['p' if entry.startswith('p_') else 'seq'].split()
        required += [n for n in ('known', 'mask', 'mtab', 'scratch') if n in names] + (['cond'] if 'scratch' in names else [])
        for name in required:
            rc = fn(entry)(*[dict(base, **{name: 0})[n] for n in names])
            assert rc == INVALID, (entry, name, rc)
            assert L.vdx_last_error(), (entry, name)
        if not torch.cuda.is_available():                              # a handle created without a device: the next check, and its code
            assert fn(entry)(*[base[n] for n in names]) == STATE, entry
