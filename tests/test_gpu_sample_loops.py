"""GPU tests of the eleven sampling-loop entry points of libvdx as one family (three chains x plain / masked / guided, plus the two
shims without a dynamic threshold): what a step launches, when a captured graph is replayed and when it is captured again, and which
calls are refused before any launch.  The C functions are called directly on buffers this file owns, so the allocator plays no part;
capture and replay are told apart with tests/_launch_hook.py (a capture records two forwards: the eager step and the captured one; a
replay records nothing).  The tiny loop network of tests/test_gpu_dpm.py, with cond_dim = 32 for the guided variants."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from _launch_hook import launches
from _sample_loop_sigs import ENTRY_VARIANT, SIGS, VARIANTS, fn as _fn

DEV = 'cuda:0'
KW = dict(dim=16, channels=1, dim_mults=(1, 2))
T, S, SHAPE, B = 60, 12, (2, 1, 4, 8, 8), 2
OK, INVALID = 0, -1

class Rig:
    """One network (with or without a condition), its handle and every buffer a loop can name, all sized for 2B samples."""

    def __init__(self, cond: bool, kw=KW, frames=SHAPE[2], size=SHAPE[3]):
        from video_diffusion_nnx_amd import _lib as L
        from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion, ddim_time_sequence
        from video_diffusion_nnx_amd.unet3d import Unet3D
        self.L = L
        self.unet = Unet3D(rngs=0, mode='f32', **kw, **(dict(cond_dim=32) if cond else {}))
        self.gd = GaussianDiffusion(self.unet, image_size=size, num_frames=frames, channels=kw['channels'], timesteps=T)
        self.h = self.unet.handle(frames, size)
        self.unet.apply_activation_storage(self.h)
        self.ws = self.unet.workspace(2 * B, frames, size)
        self.st = torch.cuda.Stream(device=DEV)
        shape2 = (2 * B, kw['channels'], frames, size, size)
        g = torch.Generator().manual_seed(5)
        z = lambda *s, **k: torch.zeros(*s, device=DEV, **k)
        self.seq_host = ddim_time_sequence(T, S)
        self.t = dict(
            img=z(shape2), img2=z(shape2), eps=z(2 * B, frames, size, size, kw['channels']), hist=z(shape2), t_dev=z(2 * B, dtype=torch.int32),
            step_dev=z(1, dtype=torch.int64), thres=z(B), thres2=z(B), known=(2 * torch.rand(shape2, generator=g) - 1).to(DEV),
            mask=(torch.rand(shape2, generator=g) < 0.5).to(torch.uint8).to(DEV), seq=torch.from_numpy(self.seq_host).to(DEV),
            cond=torch.randn(B, 32, generator=g).to(DEV), scratch=z(L.vdx_cfg_scratch_doubles(B), dtype=torch.float64))
        self.x_T = torch.randn(shape2, generator=g).to(DEV)
        self.has_cond = cond
        torch.cuda.synchronize()

    def args(self, variant, **over):
        """Every named argument of the variant's entry at its default (static clip, seed 3, order 2, cond_scale 2, rescale 0, U = 2)."""
        L, t, gd = self.L, self.t, self.gd
        p = {k: L.ptr(v) for k, v in t.items()}
        a = dict(p, h=self.h.ptr, params=L.ptr(self.unet.flat_params), packed=L.ptr(self.unet.packed()), tables=L.ptr(gd._ptab), timesteps=T,
                 ac=L.ptr(gd.alphas_cumprod), seq_len=S, nsteps=1, cond=p['cond'] if self.has_cond else 0, seed=3, clip=1, order=2,
                 percentile=0.0, thres=0, mtab=L.ptr(gd._mtab), resample=2, cond_scale=2.0, rescale=0.0, ws=L.ptr(self.ws),
                 ws_bytes=self.ws.numel(), batch=B, use_graph=0, stream=self.st.cuda_stream)
        a.update(over)
        return a

    def call(self, entry, a, reset=True):
        """One call of `entry` on the rig's stream; returns (status, launches recorded).  reset: the chain starts over (x_T, t, step)."""
        seq_chain = not entry.startswith('p_')
        with torch.cuda.stream(self.st):
            if reset:
                for name in ('img', 'img2'):
                    self.t[name].copy_(self.x_T)
                self.t['t_dev'].fill_(int(self.seq_host[0]) if seq_chain else T - 1)
                self.t['step_dev'].zero_()
            with launches() as rec:
                rc = _fn(entry)(*[a[n] for n in SIGS[entry].split()])
            self.st.synchronize()
        return rc, rec


@functools.lru_cache(None)
def rig(cond: bool) -> Rig:
    return Rig(cond)


def _rig_for(variant):
    return rig(variant.endswith('_guided'))


def _forwards(rec):
    return sum(k.startswith('final_conv') for k, _ in rec)


def _after_last_forward(rec):
    last = max(i for i, (k, _) in enumerate(rec) if k.startswith('final_conv'))
    return rec[last + 1:]


# ---- 1. what one step launches ----

@pytest.mark.parametrize('variant', list(VARIANTS))
def test_step_composition(variant):
    entry, step_kernel, advance_kernel = VARIANTS[variant]
    r = _rig_for(variant)
    guided = variant.endswith('_guided')
    rows = 'B4' if guided else 'B2'
    for dyn in (False, True):
        for rescale in ((0.0, 0.5) if guided else (0.0,)):
            over = dict(rescale=rescale, **(dict(percentile=0.9, thres=r.L.ptr(r.t['thres'])) if dyn else {}))
            rc, rec = r.call(entry, r.args(variant, **over))
            assert rc == OK, (variant, r.L.vdx_last_error())
            assert _forwards(rec) == 1, rec
            tail = _after_last_forward(rec)
            expected = (['cfg_stats_partial_kernel', 'cfg_stats_final_kernel'] if rescale > 0 else []) + (['cfg_combine_kernel'] if guided else []) \
                + (['dyn_thres_kernel'] if dyn else []) + [step_kernel, advance_kernel]
            assert [k for k, _ in tail] == expected, (variant, dyn, rescale, tail)
            assert tail[-1][1] == rows, tail[-1]                           # the advance covers both halves of a guided batch
            assert tail[-2][1].startswith('B2 '), tail[-2]                 # the step kernel never does
            assert int(r.t['step_dev'].item()) == 1
            t_next = T - 1 if variant == 'p_masked' else T - 2 if variant.startswith('p') else int(r.seq_host[1])    # U = 2: t stays
            assert r.t['t_dev'].tolist() == [t_next] * (4 if guided else 2) + [T - 1 if variant.startswith('p') else int(r.seq_host[0])] * (0 if guided else 2)


# ---- 2. when the captured graph is reused ----

def _baked_scalars(variant):
    out = []
    if variant.startswith('p') or variant.endswith('_masked'):
        out.append(dict(seed=4))
    if variant.startswith('dpm'):
        out.append(dict(order=1))
    if variant.endswith('_guided'):
        out += [dict(cond_scale=3.0), dict(rescale=0.5)]
    return out


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_graph_key(variant):
    entry = VARIANTS[variant][0]
    r = rig(True)                                # the network with a condition runs all nine variants on one handle
    L = r.L
    base = r.args(variant, use_graph=1, nsteps=2)

    def run(what, captures, **over):
        rc, rec = r.call(entry, dict(base, **over))
        assert rc == OK, (variant, what, L.vdx_last_error())
        assert _forwards(rec) == (2 if captures else 0), (variant, what, rec)
        if not captures:
            assert rec == [], (variant, what, rec)

    r.call(entry, dict(base, img=L.ptr(r.t['img2'])))                    # (whatever an earlier test left in this slot goes)
    run('first call', True)
    run('same arguments, nsteps 3', False, nsteps=3)
    run('another thres_buf without a dynamic threshold', False, thres=L.ptr(r.t['thres2']))
    run('percentile without clip_denoised is no dynamic threshold', True, clip=0, percentile=0.9, thres=L.ptr(r.t['thres']))
    run('... and its thres_buf does not count either', False, clip=0, percentile=0.9, thres=L.ptr(r.t['thres2']))
    run('back', True)
    run('another img', True, img=L.ptr(r.t['img2']))
    run('back', True)
    for over in _baked_scalars(variant):
        run(f'changed {over}', True, **over)
        run(f'changed {over}, again', False, **over)
        run('back', True)
    # another variant in between leaves this one's graph alone: every (chain, variant) pair has a slot of its own
    for other in VARIANTS:
        if other != variant:
            rc, _ = r.call(VARIANTS[other][0], r.args(other, use_graph=1, nsteps=2))
            assert rc == OK, (other, L.vdx_last_error())
    run('after every other variant of this handle', False)
    # the dynamic threshold: thres_buf and percentile now count
    dyn = dict(percentile=0.9, thres=L.ptr(r.t['thres']))
    run('dynamic threshold', True, **dyn)
    run('dynamic threshold again', False, **dyn)
    run('dynamic threshold, another thres_buf', True, **dict(dyn, thres=L.ptr(r.t['thres2'])))
    run('dynamic threshold, another percentile', True, **dict(dyn, percentile=0.8))


def test_shims_without_dynamic_threshold_share_the_slot():
    """vdx_p_sample_loop / vdx_ddim_sample_loop are the _dyn entries with percentile 0: same step, same key, same graph."""
    r = rig(False)
    for shim, variant in (('p_sample_loop', 'p'), ('ddim_sample_loop', 'ddim')):
        a = r.args(variant, use_graph=1, nsteps=2)
        rc, rec = r.call(VARIANTS[variant][0], dict(a, img=r.L.ptr(r.t['img2'])))       # (whatever an earlier test left in the slot goes)
        rc, rec = r.call(VARIANTS[variant][0], a)
        assert rc == OK and _forwards(rec) == 2, rec
        rc, rec = r.call(shim, a)
        assert rc == OK and rec == [], (shim, rec)
        rc, rec = r.call(shim, dict(a, use_graph=0, nsteps=1))
        assert rc == OK and [k for k, _ in _after_last_forward(rec)] == list(VARIANTS[variant][1:]), rec


def test_captured_steps_are_the_eager_steps():
    """Three steps of every variant, captured against eager, from the same start: the same kernels on the same inputs."""
    for variant, (entry, _, _) in VARIANTS.items():
        r = _rig_for(variant)
        outs = []
        for graph in (1, 0):
            rc, _ = r.call(entry, r.args(variant, use_graph=graph, nsteps=3, percentile=0.9, thres=r.L.ptr(r.t['thres'])))
            assert rc == OK, (variant, r.L.vdx_last_error())
            outs.append((r.t['img'][:B].clone(), r.t['t_dev'].clone(), int(r.t['step_dev'].item())))
        assert torch.allclose(outs[0][0], outs[1][0], atol=1e-5), variant     # (f64 atomics of the GroupNorm statistics: last-bit jitter)
        assert torch.equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2] == 3, variant
        assert torch.isfinite(outs[0][0]).all() and not torch.equal(outs[0][0], r.x_T[:B]), variant


# ---- 3. what is refused, before any launch ----

def _rejections():
    """(entry, {argument: bad value} or a callable of the rig, why) -- one row per rule and variant the rule applies to."""
    rows = []
    every = list(SIGS)
    masked = [e for e in every if e.endswith('_masked')]
    guided = [e for e in every if e.endswith('_guided')]
    seq = [e for e in every if not e.startswith('p_')]
    dpm = [e for e in every if e.startswith('dpm_')]
    dyn_capable = [e for e in every if 'percentile' in SIGS[e].split()]
    misaligned = lambda name, by: (lambda r: {name: r.L.ptr(r.t[name]) + by})
    for e in every:
        names = SIGS[e].split()
        for must in ('h', 'params', 'packed', 'img', 'eps', 't_dev', 'step_dev', 'ws'):
            rows.append((e, {must: 0}, f'null {must}'))
        rows.append((e, {'nsteps': -1}, 'nsteps < 0'))
        if e.startswith('p_'):
            rows.append((e, {'tables': 0}, 'null tables'))
            rows.append((e, {'nsteps': 2 * T + 1 if e in masked else T + 1}, 'nsteps past the chain'))
        else:
            rows += [(e, {'ac': 0}, 'null alphas_cumprod'), (e, {'seq': 0}, 'null seq'), (e, {'seq_len': 0}, 'seq_len < 1'),
                     (e, {'nsteps': S + 1}, 'nsteps > seq_len')]
        if e in dyn_capable:
            on = {'percentile': 0.9}
            rows += [(e, lambda r, on=on: dict(on, thres=0), 'dyn without thres_buf'),
                     (e, lambda r: dict(percentile=1.5, thres=r.L.ptr(r.t['thres'])), 'percentile > 1')]
            if e in seq:
                rows.append((e, lambda r: dict(percentile=0.9, thres=r.L.ptr(r.t['thres']), tables=0), 'dyn without tables'))
                if e not in masked:                                        # (masked: timesteps >= 1 is a rule of its own, below)
                    rows.append((e, lambda r: dict(percentile=0.9, thres=r.L.ptr(r.t['thres']), timesteps=0), 'dyn with timesteps < 1'))
    for e in masked:
        rows += [(e, {'known': 0}, 'null known'), (e, {'mask': 0}, 'null mask'), (e, {'mtab': 0}, 'null mask_tables'),
                 (e, {'timesteps': 0}, 'timesteps < 1'), (e, misaligned('img', 4), 'img not 16-byte aligned'),
                 (e, misaligned('known', 4), 'known not 16-byte aligned'), (e, misaligned('mask', 1), 'mask not 4-byte aligned')]
    rows += [('p_sample_loop_masked', {'resample': 0}, 'resample_steps < 1'), ('p_sample_loop_guided', {'timesteps': 0}, 'timesteps < 1')]
    for e in dpm:
        rows += [(e, {'order': 0}, 'order 0'), (e, {'order': 3}, 'order 3'), (e, {'hist': 0}, 'order 2 without hist'),
                 (e, misaligned('img', 4), 'img not 16-byte aligned'), (e, misaligned('hist', 4), 'hist not 16-byte aligned')]
    for e in guided:
        rows += [(e, {'cond': 0}, 'null cond'), (e, {'scratch': 0}, 'null cfg_scratch'), (e, {'batch': 0}, 'batch < 1'),
                 (e, {'rescale': -0.1}, 'rescale < 0'), (e, {'rescale': 1.1}, 'rescale > 1'), (e, {'rescale': float('nan')}, 'rescale nan'),
                 (e, misaligned('img', 4), 'img not 16-byte aligned'), (e, misaligned('eps', 4), 'eps_buf not 16-byte aligned'),
                 (e, misaligned('scratch', 4), 'cfg_scratch not 8-byte aligned')]
    return rows


def test_rejections():
    rows = _rejections()
    assert {e for e, _, _ in rows} == set(SIGS)
    for entry, bad, why in rows:
        variant = ENTRY_VARIANT[entry]
        r = _rig_for(variant)
        over = bad(r) if callable(bad) else bad
        assert set(over) <= set(SIGS[entry].split()), (entry, over)
        for graph in (0, 1):
            rc, rec = r.call(entry, r.args(variant, use_graph=graph, **over), reset=False)
            assert rc == INVALID and rec == [], (entry, why, rc, rec)
            assert r.L.vdx_last_error(), (entry, why)
    # the handle must be able to run the loop at all: a network whose out_dim differs from its channels, and (guided) one without a condition
    wide = Rig(False, kw=dict(KW, out_dim=2))
    for variant in ('p', 'p_masked', 'ddim', 'ddim_masked', 'dpm', 'dpm_masked'):
        rc, rec = wide.call(VARIANTS[variant][0], wide.args(variant), reset=False)
        assert rc == INVALID and rec == [], (variant, 'out_dim != channels', rc, rec)
    plain = rig(False)
    for variant in ('p_guided', 'ddim_guided', 'dpm_guided'):
        rc, rec = plain.call(VARIANTS[variant][0], plain.args(variant, cond=plain.L.ptr(plain.t['cond'])), reset=False)
        assert rc == INVALID and rec == [], (variant, 'cond_dim == 0', rc, rec)


def test_what_is_not_asked_for():
    """The negative rows: rules that hold for some variants only must not spread to the others."""
    r = rig(False)
    # no unguided entry takes a cfg_scratch, and none asks for a condition: a network without one runs with cond = null
    for variant in ('p', 'p_masked', 'ddim', 'ddim_masked', 'dpm', 'dpm_masked'):
        entry = VARIANTS[variant][0]
        assert 'scratch' not in SIGS[entry].split()
        rc, rec = r.call(entry, r.args(variant, cond=0))
        assert rc == OK and _forwards(rec) == 1, (variant, r.L.vdx_last_error())
    # order 1 needs no history tensor; a sequence chain without a dynamic threshold needs neither tables nor timesteps
    for variant in ('dpm', 'dpm_masked'):
        rc, _ = r.call(VARIANTS[variant][0], r.args(variant, order=1, hist=0))
        assert rc == OK, (variant, r.L.vdx_last_error())
    for variant in ('ddim', 'dpm'):
        rc, _ = r.call(VARIANTS[variant][0], r.args(variant, tables=0, timesteps=0))
        assert rc == OK, (variant, r.L.vdx_last_error())
    g = rig(True)
    for variant in ('ddim_guided', 'dpm_guided'):
        rc, _ = g.call(VARIANTS[variant][0], g.args(variant, tables=0, timesteps=0))
        assert rc == OK, (variant, g.L.vdx_last_error())
    # nsteps = 0 is a valid call that launches nothing
    for variant in VARIANTS:
        rr = _rig_for(variant)
        for graph in (0, 1):
            rc, rec = rr.call(VARIANTS[variant][0], rr.args(variant, nsteps=0, use_graph=graph, img=rr.L.ptr(rr.t['hist'])))
            assert rc == OK and rec == [], (variant, rec)
    # C*F*H*W % 4 == 2 (1 x 2 x 3 x 3): only the unmasked, unguided DDIM loop takes it (its step kernel has a scalar form).  Asked with
    # nsteps = 0, so that nothing is launched at a shape the rest of the network is not tested at
    odd = Rig(False, kw=dict(dim=16, channels=1, dim_mults=(1,)), frames=2, size=3)
    odd_cond = Rig(True, kw=dict(dim=16, channels=1, dim_mults=(1,)), frames=2, size=3)
    for entry in SIGS:
        variant = ENTRY_VARIANT[entry]
        rr = odd_cond if variant.endswith('_guided') else odd
        rc, rec = rr.call(entry, rr.args(variant, nsteps=0), reset=False)
        assert rc == (OK if variant == 'ddim' else INVALID) and rec == [], (entry, rc, rr.L.vdx_last_error())
