"""GPU parity of the kernels around the UNet (csrc/diffusion.hip, csrc/optim.hip) where their loops wrap: every case of
tests/_step_cases.py through the C ABI against the fp64 references composed there, at

  WRAP      B 2, C 4, fhw 525 001 (per_sample 2 100 004): the second trip of every grid-stride loop, quads that straddle channels;
  STRADDLE  B 3, C 4, fhw 35: the option matrix of each kernel with channel boundaries inside quads;
  RAGGED    B 3, C 3, fhw 35 (per_sample 105): sample bases at 4-byte offsets for the kernels that accept them, VDX_ERR_INVALID and an
            untouched output for the others;

and the flat-buffer kernels (randn, affine, Adam, Adam behind the clip, grad_accumulate) past their grid caps.  Every output lies between
two 64-float NaN bands inside one buffer and is NaN-filled itself; every input is compared with its host copy after the calls.
tests/test_host_step_kernels.py shows on the CPU that these comparisons reject the faults the shapes were chosen for."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _step_cases as S
from _step_cases import F32, F64, INVALID, RAGGED, SHAPES, STRADDLE, WRAP

DEV = 'cuda:0'
BAND = 64
NAN = float('nan')
SMALL_CFGS = ((True, False), (False, False), (True, True))       # (clip, per-sample thres)
WRAP_CFGS = ((True, True),)


def _cfgs(sh):
    return WRAP_CFGS if sh is WRAP else SMALL_CFGS


def _L():
    from video_diffusion_nnx_amd import _lib as L
    return L


def _G():
    from video_diffusion_nnx_amd import gaussian_diffusion as G
    return G


class Dev:
    """Device copies of named host tensors; unchanged() compares every one of them with its host copy."""

    def __init__(self, **host):
        self.host = {k: v for k, v in host.items() if v is not None}
        self.dev = {k: v.to(DEV).contiguous() for k, v in self.host.items()}

    def __getitem__(self, k):
        return self.dev.get(k)

    def p(self, k):
        return _L().ptr(self.dev.get(k)) if k is not None else 0

    def unchanged(self):
        torch.cuda.synchronize()
        for k, v in self.host.items():
            assert torch.equal(self.dev[k].cpu(), v), f'input {k} was written'


def _out(n, src=None, dtype=F32):
    """A NaN-filled output of n elements between two NaN bands of one buffer; src is copied in for an in-place run."""
    buf = torch.full((n + 2 * BAND,), NAN, dtype=dtype, device=DEV)
    out = buf[BAND:BAND + n]
    if src is not None:
        out.copy_(src.reshape(-1))
    return buf, out


def _finish(buf, n, shape=None):
    torch.cuda.synchronize()
    host = buf.cpu()
    assert torch.isnan(host[:BAND]).all() and torch.isnan(host[BAND + n:]).all(), 'a value outside the output was written'
    out = host[BAND:BAND + n].clone()
    return out if shape is None else out.reshape(shape)


def _untouched(buf):
    torch.cuda.synchronize()
    assert torch.isnan(buf).all(), 'a refused call wrote its output'


def _bits(a, b, what):
    assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), f'{what}: not bit-equal'


def _tabs(T):
    return Dev(**S.device_tables(T))


def _thres(sh, on):
    return S.thres_vec(sh) if on else None


# ---- wrappers: one ABI call into a banded output -------------------------------------------------------------------------------------

def _p_sample(sh, d, tabs, clip, noise_key, seed=0, offset=0, dev_offset=None, inplace=False):
    L, n = _L(), sh.B * S.per(sh)
    buf, out = _out(n, d['x'] if inplace else None)
    rc = _G().vdx_p_sample_step(out.data_ptr() if inplace else d.p('x'), d.p('eps'), out.data_ptr(), d.p('t'), tabs.p('ptab'), S.T_P, d.p(noise_key),
                                seed, offset, L.ptr(dev_offset), d.p('thres'), int(clip), sh.B, sh.C, S.per(sh), L.stream_ptr())
    return rc, buf, n


def _p_masked(sh, d, tabs, clip, mask_key, U, step, seed, step_dev=None, inplace=False):
    L, n = _L(), sh.B * S.per(sh)
    buf, out = _out(n, d['x'] if inplace else None)
    rc = _G().vdx_p_sample_step_masked(out.data_ptr() if inplace else d.p('x'), d.p('eps'), out.data_ptr(), d.p('t'), tabs.p('ptab'), S.T_P, d.p('known'),
                                       d.p(mask_key), tabs.p('mtab'), U, seed, step, L.ptr(step_dev), d.p('thres'), int(clip), sh.B, sh.C, S.per(sh),
                                       L.stream_ptr())
    return rc, buf, n


def _ddim(sh, d, tabs, clip, step_dev, mask_key=None, seed=0, inplace=False):
    L, n = _L(), sh.B * S.per(sh)
    buf, out = _out(n, d['x'] if inplace else None)
    xp = out.data_ptr() if inplace else d.p('x')
    if mask_key is None:
        rc = _G().vdx_ddim_step(xp, d.p('eps'), out.data_ptr(), tabs.p('ac'), d.p('seq'), L.ptr(step_dev), d.p('thres'), int(clip), sh.B, sh.C, S.per(sh),
                                L.stream_ptr())
    else:
        rc = _G().vdx_ddim_step_masked(xp, d.p('eps'), out.data_ptr(), tabs.p('ac'), d.p('seq'), L.ptr(step_dev), d.p('thres'), int(clip), d.p('known'),
                                       d.p(mask_key), tabs.p('mtab'), S.T_D, seed, sh.B, sh.C, S.per(sh), L.stream_ptr())
    return rc, buf, n


def _dpm(sh, d, tabs, clip, order, step_dev, with_hist=True, mask_key=None, seed=0, inplace=False):
    """Returns (rc, out buffer, hist buffer or None, n); hist starts as the shared history draw."""
    L, n = _L(), sh.B * S.per(sh)
    buf, out = _out(n, d['x'] if inplace else None)
    hbuf, hist = _out(n, d['hist']) if with_hist else (None, None)
    xp, hp = out.data_ptr() if inplace else d.p('x'), hist.data_ptr() if with_hist else 0
    if mask_key is None:
        rc = _G().vdx_dpm_step(xp, d.p('eps'), out.data_ptr(), hp, tabs.p('ac'), d.p('seq'), L.ptr(step_dev), d.p('thres'), int(clip), order, sh.B, sh.C,
                               S.per(sh), L.stream_ptr())
    else:
        rc = _G().vdx_dpm_step_masked(xp, d.p('eps'), out.data_ptr(), hp, tabs.p('ac'), d.p('seq'), L.ptr(step_dev), d.p('thres'), int(clip), order,
                                      d.p('known'), d.p(mask_key), tabs.p('mtab'), S.T_D, seed, sh.B, sh.C, S.per(sh), L.stream_ptr())
    return rc, buf, hbuf, n


def _step_dev(k):
    return torch.full((1,), k, dtype=torch.int64, device=DEV)


def _masks_of(sh):
    return ('p04',) if sh is WRAP else ('p04', 'chan', 'lanes')


def _mask_dev(sh, kinds):
    return {f'm_{k}': S.mask(sh.name, k) for k in kinds}


# ---- randn, affine, grad_accumulate ------------------------------------------------------------------------------------------------------

def test_randn_second_sweep_with_device_offset():
    L, n, seed = _L(), S.N_RANDN, 0x1234567890ABCDEF
    dev_off = torch.full((1,), 4, dtype=torch.int64, device=DEV)
    outs = []
    for offset, dptr in ((3, dev_off), (3, dev_off), (7, None)):
        buf, out = _out(n)
        L.check(_G().vdx_randn(out.data_ptr(), n, seed, offset, L.ptr(dptr), L.stream_ptr()))
        outs.append(_finish(buf, n))
    ref = torch.from_numpy(S.philox_ref.randn(n, seed, 7))
    assert not torch.isnan(outs[0]).any()
    err = (outs[0].double() - ref.double()).abs()
    print(f'[randn n={n}] max-abs error {err.max().item():.3e} (atol {S.RANDN_ATOL:.0e}, rtol {S.RANDN_RTOL:.0e}); second sweep '
          f'{err[S.SWEEP4:].max().item():.3e}')
    np.testing.assert_allclose(outs[0].numpy(), ref.numpy(), atol=S.RANDN_ATOL, rtol=S.RANDN_RTOL)
    _bits(outs[0], outs[1], 'randn second run')
    _bits(outs[0], outs[2], 'randn offset + *dev_offset vs the explicit offset')
    assert dev_off.item() == 4


def test_affine_wraps():
    L, n = _L(), S.N_AFFINE
    g = torch.Generator().manual_seed(n)
    d = Dev(x=torch.randn(n, generator=g))
    a, b = np.float32(1.7), np.float32(-0.3)
    buf, out = _out(n)
    L.check(_G().vdx_affine(d.p('x'), out.data_ptr(), n, float(a), float(b), L.stream_ptr()))
    got = _finish(buf, n)
    ref = d.host['x'].double() * float(a) + float(b)                  # the product of two floats is exact in double: one rounding, as fmaf
    assert not torch.isnan(got).any()
    worst = ((got.double() - ref).abs() / ref.abs()).max().item()
    print(f'[affine n={n}] worst relative error {worst / S.U24:.3f} x 2^-24 (bound 1: one correctly rounded fma)')
    assert ((got.double() - ref).abs() <= S.U24 * ref.abs() * (1 + 1e-9)).all()
    buf, out = _out(n)
    L.check(_G().vdx_affine(d.p('x'), out.data_ptr(), n, float(a), float(b), L.stream_ptr()))
    _bits(got, _finish(buf, n), 'affine second run')
    d.unchanged()


@pytest.mark.parametrize('offs', [(0, 0), (1, 1), (3, 2)])           # the (acc, g) offsets of test_gpu_grad_controls.py
def test_grad_accumulate_wraps_bit_exact(offs):
    from video_diffusion_nnx_amd import ops
    n, (oa, og), PAD = S.N_ACC, offs, 8
    g = torch.Generator().manual_seed(n + 7 * oa + og)
    A, G = torch.randn(n + 2 * PAD, generator=g), torch.randn(n + 2 * PAD, generator=g)
    exp = A.clone()
    exp[oa:oa + n] = A[oa:oa + n] + G[og:og + n]
    dA, dG = A.to(DEV), G.to(DEV)
    ops.grad_accumulate(dA[oa:oa + n], dG[og:og + n])
    torch.cuda.synchronize()
    assert torch.equal(dA.cpu(), exp), 'acc + g differs, or a float outside [0, n) was written'
    assert torch.equal(dG.cpu(), G)


# ---- q_sample, inpaint_init ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['WRAP', 'STRADDLE'])
def test_q_sample_and_masked(name):
    L, G, sh = _L(), _G(), SHAPES[name]
    n, g = sh.B * S.per(sh), torch.Generator().manual_seed(42)
    x, noise, t = torch.rand(S.dims(sh), generator=g), torch.randn(S.dims(sh), generator=g), S.t_vec(sh, S.T_Q)
    kinds = _masks_of(sh) + ('zero', 'one')
    d, tabs = Dev(x=x, noise=noise, t=t.to(torch.int32), **_mask_dev(sh, kinds)), _tabs(S.T_Q)

    def run(mask_key=None):
        buf, out = _out(n)
        if mask_key is None:
            L.check(G.vdx_q_sample(d.p('x'), d.p('t'), d.p('noise'), out.data_ptr(), tabs.p('sqrt_ac'), tabs.p('sqrt_1mac'), sh.B, S.per(sh), 2.0, -1.0,
                                   L.stream_ptr()))
        else:
            L.check(G.vdx_q_sample_masked(d.p('x'), d.p('t'), d.p('noise'), d.p(mask_key), out.data_ptr(), tabs.p('sqrt_ac'), tabs.p('sqrt_1mac'), sh.B,
                                          S.per(sh), 2.0, -1.0, L.stream_ptr()))
        return _finish(buf, n, S.dims(sh))
    plain = run()
    S.check(plain, S.q_sample_ref(x, noise, t), S.Q_TOL, f'q_sample {name}')
    _bits(plain, run(), 'q_sample second run')
    norm = x * 2 - 1                                                    # == fmaf(x, 2, -1): x * 2 is exact, one rounding either way
    for k in _masks_of(sh):
        m = S.mask(name, k)
        got = run(f'm_{k}')
        S.check(got, S.q_sample_ref(x, noise, t, m), S.Q_TOL, f'q_sample_masked {name} {k}')
        assert torch.equal(got[m.bool()], norm[m.bool()]) and torch.equal(got[~m.bool()], plain[~m.bool()])
    _bits(run('m_zero'), plain, 'q_sample_masked with an all-zero mask vs q_sample')
    assert torch.equal(run('m_one'), norm)
    d.unchanged()
    tabs.unchanged()


@pytest.mark.parametrize('name', ['WRAP', 'STRADDLE'])
def test_inpaint_init(name):
    """x = mask ? sqrt_ac[t0] known + sqrt(1 - ac[t0]) x : x, in place: q_sample's expression (its bound), the rest of x keeps its bits."""
    L, sh = _L(), SHAPES[name]
    n, I, t0 = sh.B * S.per(sh), S.step_inputs(name, 5, 2.0), S.T_P - 1
    x = I['z']                                                          # x_T ~ N(0, 1)
    d, tabs = Dev(x=x, known=I['known'], **_mask_dev(sh, _masks_of(sh) + ('zero',))), _tabs(S.T_P)
    ref = S.diffusion_ref(S.T_P, F64)
    def run(k):
        buf, out = _out(n, d['x'])
        L.check(_G().vdx_inpaint_init(out.data_ptr(), d.p('known'), d.p(f'm_{k}'), tabs.p('mtab'), S.T_P, t0, n, L.stream_ptr()))
        return _finish(buf, n, S.dims(sh))
    for k in _masks_of(sh) + ('zero',):
        m = S.mask(name, k).bool()
        got = run(k)
        _bits(got, run(k), f'inpaint_init {name} {k} second run')
        exp = torch.where(m, ref.q_sample(I['known'].double(), torch.full((sh.B,), t0), x.double()), x.double())
        S.check(got, exp, S.Q_TOL, f'inpaint_init {name} {k}')
        assert torch.equal(got[~m], x[~m])
    d.unchanged()


# ---- the ancestral step ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['WRAP', 'STRADDLE', 'RAGGED'])
def test_p_sample_step_T1000(name):
    sh, I = SHAPES[name], S.step_inputs(name, 5, 2.0)
    t, tabs, seed = S.t_vec(sh, S.T_P), _tabs(S.T_P), 77
    zp = S.z_philox(sh, seed, 6) if sh is not RAGGED else None
    for clip, th in _cfgs(sh):
        thres = _thres(sh, th)
        d = Dev(x=I['x'], eps=I['eps'], z=I['z'], t=t.to(torch.int32), thres=thres)
        what = f'p_sample {name} clip={int(clip)} thres={int(th)}'

        def run(**kw):
            rc, buf, n = _p_sample(sh, d, tabs, clip, **kw)
            assert rc == 0, _L().vdx_last_error()
            return _finish(buf, n, S.dims(sh))
        got = run(noise_key='z')
        ref64, mean64 = S.p_sample_ref(I['x'], I['eps'], I['z'], t, clip, thres, F64)
        ref32, _ = S.p_sample_ref(I['x'], I['eps'], I['z'], t, clip, thres, F32)
        bound, rel, floor = S.floor_bound(S.P_TOL_NOISE, ref32, ref64)
        print(f'[{what}] CPU fp32 floor {floor:.3e}, bound {rel:.3e} x max(1, |ref|max) per sample')
        S.check(got, ref64, bound, what + ' explicit noise')
        S.check(got[0], mean64[0], S.P_TOL_T0, what + ' t = 0 is the posterior mean')
        _bits(got, run(noise_key='z'), what + ' second run')
        _bits(got, run(noise_key='z', inplace=True), what + ' x and out the same buffer')
        if sh is RAGGED:                                                # generated noise needs per_sample % 4 == 0
            rc, buf, n = _p_sample(sh, d, tabs, clip, noise_key=None, seed=seed, offset=6)
            assert rc == INVALID
            _untouched(buf)
        else:
            gp = run(noise_key=None, seed=seed, offset=6)
            r64, _ = S.p_sample_ref(I['x'], I['eps'], zp, t, clip, thres, F64)
            r32, _ = S.p_sample_ref(I['x'], I['eps'], zp, t, clip, thres, F32)
            bound, rel, floor = S.floor_bound(S.P_TOL_PHILOX, r32, r64)
            print(f'[{what} Philox] CPU fp32 floor {floor:.3e}, bound {rel:.3e} x max(1, |ref|max) per sample')
            S.check(gp, r64, bound, what + ' Philox noise')
            _bits(gp, run(noise_key=None, seed=seed, offset=2, dev_offset=_step_dev(4)), what + ' offset + *dev_offset')
            _bits(gp, run(noise_key=None, seed=seed, offset=6, inplace=True), what + ' Philox, x and out the same buffer')
        d.unchanged()
    tabs.unchanged()


@pytest.mark.parametrize('name', ['WRAP', 'STRADDLE'])
def test_p_sample_step_masked_T1000(name):
    sh, I = SHAPES[name], S.step_inputs(name, 5, 2.0)
    t, tabs, seed = S.t_vec(sh, S.T_P), _tabs(S.T_P), 91
    steps = ((3, 4), (1, 7)) if sh is WRAP else ((1, 7), (3, 4), (3, 5))      # U = 3: s = 4 re-noises (4 % 3 != 2), s = 5 does not
    for clip, th in _cfgs(sh):
        thres = _thres(sh, th)
        d = Dev(x=I['x'], eps=I['eps'], known=I['known'], t=t.to(torch.int32), thres=thres, **_mask_dev(sh, _masks_of(sh) + ('zero',)))

        def run(mask_key, U, s, **kw):
            rc, buf, n = _p_masked(sh, d, tabs, clip, mask_key, U, s, seed, **kw)
            assert rc == 0, _L().vdx_last_error()
            return _finish(buf, n, S.dims(sh))
        for k in _masks_of(sh):
            m = S.mask(name, k)
            for U, s in steps:
                what = f'p_sample_masked {name} clip={int(clip)} thres={int(th)} mask={k} U={U} s={s}'
                got = run(f'm_{k}', U, s)
                r64 = S.p_sample_masked_ref(sh, I['x'], I['eps'], I['known'], m, t, clip, thres, seed, s, U, F64)
                r32 = S.p_sample_masked_ref(sh, I['x'], I['eps'], I['known'], m, t, clip, thres, seed, s, U, F32)
                bound, rel, floor = S.floor_bound(S.P_TOL_MASKED, r32, r64)
                print(f'[{what}] CPU fp32 floor {floor:.3e}, bound {rel:.3e} x max(1, |ref|max) per sample')
                S.check(got, r64, bound, what)
                if s % U == U - 1:
                    mb = m[0].bool()
                    assert torch.equal(got[0][mb], I['known'][0][mb]), 'known elements at t = 0 are `known` exactly'
                _bits(got, run(f'm_{k}', U, s, inplace=True), what + ' x and out the same buffer')
        got = run('m_p04', 1, 7)
        _bits(got, run('m_p04', 1, 7), 'p_sample_masked second run')
        _bits(got, run('m_p04', 1, 2, step_dev=_step_dev(5)), 'p_sample_masked step + *step_dev')
        rc, buf, n = _p_sample(sh, d, tabs, clip, noise_key=None, seed=seed, offset=1 + 7)
        assert rc == 0
        _bits(run('m_zero', 1, 7), _finish(buf, n, S.dims(sh)), 'p_sample_masked with an all-zero mask vs p_sample at the same draw')
        d.unchanged()
    tabs.unchanged()


# ---- DDIM and DPM-Solver++ --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['WRAP', 'STRADDLE', 'RAGGED'])
def test_ddim_step_and_masked(name):
    sh, I = SHAPES[name], S.step_inputs(name, 3, 1.0)
    tabs, seq, seed = _tabs(S.T_D), S.time_sequence(S.T_D, S.S_DDIM), 17
    ac = tabs.host['ac']
    masked = sh is not RAGGED
    kinds = _masks_of(sh) + ('zero',) if masked else ()
    for clip, th in _cfgs(sh):
        thres = _thres(sh, th)
        d = Dev(x=I['x'], eps=I['eps'], known=I['known'], seq=torch.from_numpy(seq), thres=thres, **_mask_dev(sh, kinds))

        def run(k, **kw):
            sd = None if k is None else _step_dev(k)                      # alive until _finish has synchronised
            rc, buf, n = _ddim(sh, d, tabs, clip, sd, **kw)
            assert rc == 0, _L().vdx_last_error()
            return _finish(buf, n, S.dims(sh))
        for k in ((57,) if sh is WRAP else S.DDIM_KS):                     # first, middle, last (t_next = -1: the data itself)
            what = f'ddim {name} clip={int(clip)} thres={int(th)} k={k}'
            got = run(k)
            ref, x0 = S.ddim_ref(I['x'], I['eps'], ac, seq, k, clip, thres)
            S.check(got, ref, S.scaled(S.STEP_TOL, ref), what)
            if seq[k + 1] < 0:
                S.check(got, x0, S.STEP_TOL, what + ' into the data')
            _bits(got, run(k), what + ' second run')
            _bits(got, run(k, inplace=True), what + ' x and out the same buffer')
            if k == 0:
                _bits(got, run(None), what + ' without a step counter')
            if not masked:
                continue
            for mk in _masks_of(sh):
                m = S.mask(name, mk)
                gm = run(k, mask_key=f'm_{mk}', seed=seed)
                exp = S.known_merge(sh, ref, I['known'], m, ac, seq, k, seed)
                S.check(gm, exp, S.scaled(S.STEP_TOL, exp), what + f' masked {mk}')
                if seq[k + 1] < 0:
                    assert torch.equal(gm[m.bool()], I['known'][m.bool()])
                _bits(gm, run(k, mask_key=f'm_{mk}', seed=seed, inplace=True), what + f' masked {mk}, x and out the same buffer')
            _bits(run(k, mask_key='m_zero', seed=seed), got, what + ' all-zero mask vs ddim_step')
        if not masked:
            sd = _step_dev(0)
            rc, buf, n = _ddim(sh, d, tabs, clip, sd, mask_key='known', seed=seed)                # any pointer: refused before it is read
            assert rc == INVALID
            _untouched(buf)
        d.unchanged()
    tabs.unchanged()


@pytest.mark.parametrize('name', ['WRAP', 'STRADDLE'])
def test_dpm_step_and_masked(name):
    sh, I = SHAPES[name], S.step_inputs(name, 3, 1.0)
    tabs, seq, seed = _tabs(S.T_D), S.time_sequence(S.T_D, S.S_DPM), 17
    ac = tabs.host['ac']
    for clip, th in _cfgs(sh):
        thres = _thres(sh, th)
        d = Dev(x=I['x'], eps=I['eps'], hist=I['hist'], known=I['known'], seq=torch.from_numpy(seq), thres=thres,
                **_mask_dev(sh, _masks_of(sh) + ('zero',)))

        def run(k, order=2, **kw):
            sd = _step_dev(k)                                             # alive until _finish has synchronised
            rc, buf, hbuf, n = _dpm(sh, d, tabs, clip, order, sd, **kw)
            assert rc == 0, _L().vdx_last_error()
            return _finish(buf, n, S.dims(sh)), None if hbuf is None else _finish(hbuf, n, S.dims(sh))
        for k in ((11,) if sh is WRAP else S.DPM_KS):         # first order, the first second-order step, the middle, the step into the data
            what = f'dpm {name} clip={int(clip)} thres={int(th)} k={k}'
            got, hist = run(k)
            ref, x0 = S.dpm_ref(I['x'], I['eps'], I['hist'], ac, seq, k, 2, clip, thres)
            S.check(got, ref, S.scaled(S.STEP_TOL, ref), what + ' out')
            S.check(hist, x0, S.scaled(S.STEP_TOL, x0), what + ' hist')
            if seq[k + 1] < 0:
                assert torch.equal(got, hist) and (not clip or got.abs().max().item() <= 1.0)
            again, hagain = run(k)
            _bits(got, again, what + ' second run')
            _bits(hist, hagain, what + ' second run, hist')
            gi, hi = run(k, inplace=True)
            _bits(got, gi, what + ' x and out the same buffer')
            _bits(hist, hi, what + ' x and out the same buffer, hist')
            # order 1 is the DDIM step within the DPM bound, with and without a history tensor
            o1, h1 = run(k, order=1)
            o1n, _ = run(k, order=1, with_hist=False)
            _bits(o1, o1n, what + ' order 1 without hist')
            ref1, x01 = S.dpm_ref(I['x'], I['eps'], I['hist'], ac, seq, k, 1, clip, thres)
            S.check(o1, ref1, S.scaled(S.STEP_TOL, ref1), what + ' order 1')
            S.check(h1, x01, S.scaled(S.STEP_TOL, x01), what + ' order 1 hist')
            sd = _step_dev(k)
            rc, buf, n = _ddim(sh, d, tabs, clip, sd)
            assert rc == 0
            dd = _finish(buf, n, S.dims(sh))
            S.check(o1, dd.double(), S.scaled(S.STEP_TOL, dd.double()), what + ' order 1 vs vdx_ddim_step')
            for mk in _masks_of(sh):
                m = S.mask(name, mk)
                gm, hm = run(k, mask_key=f'm_{mk}', seed=seed)
                exp = S.known_merge(sh, ref, I['known'], m, ac, seq, k, seed)
                S.check(gm, exp, S.scaled(S.STEP_TOL, exp), what + f' masked {mk}')
                _bits(hm, hist, what + f' masked {mk}: hist holds the network\'s x0 everywhere')
                if seq[k + 1] < 0:
                    assert torch.equal(gm[m.bool()], I['known'][m.bool()])
                gmi, hmi = run(k, mask_key=f'm_{mk}', seed=seed, inplace=True)
                _bits(gm, gmi, what + f' masked {mk}, x and out the same buffer')
                _bits(hm, hmi, what + f' masked {mk}, x and out the same buffer, hist')
            gz, hz = run(k, mask_key='m_zero', seed=seed)
            _bits(gz, got, what + ' all-zero mask vs dpm_step')
            _bits(hz, hist, what + ' all-zero mask vs dpm_step, hist')
        d.unchanged()
    tabs.unchanged()


# ---- dynamic threshold ---------------------------------------------------------------------------------------------------------------------------

def _dyn(x_dev, eps_dev, t_dev, tab_dev, q, B, C, per_sample):
    L = _L()
    buf, out = _out(B)
    L.check(_G().vdx_dynamic_threshold(L.ptr(x_dev), L.ptr(eps_dev), L.ptr(t_dev), L.ptr(tab_dev), S.T_DYN, q, out.data_ptr(), B, C, per_sample,
                                       L.stream_ptr()))
    return _finish(buf, B)


@pytest.mark.parametrize('per_sample,C', S.DYN_GAUSS)
def test_dynamic_threshold_gaussian(per_sample, C):
    Gs = S.dyn_gauss(per_sample, C)
    d = Dev(x=Gs['x'], eps=Gs['eps'], t=Gs['t'], tab=S.dyn_tables())
    for q in S.DYN_QS:
        got = _dyn(d['x'], d['eps'], d['t'], d['tab'], q, S.DYN_B, C, per_sample)
        ref = Gs['ref'][q]
        assert not torch.isnan(got).any()
        worst = (np.abs(got.double().numpy() - ref) / ref).max()
        print(f'[dyn_thres per={per_sample} C={C} q={q}] worst relative error {worst:.3e} (rtol = atol = {S.DYN_RTOL:.0e}); quantiles {ref}')
        assert (ref >= S.DYN_MARGIN).all()
        np.testing.assert_allclose(got.double().numpy(), ref, rtol=S.DYN_RTOL, atol=S.DYN_ATOL)
        _bits(got, _dyn(d['x'], d['eps'], d['t'], d['tab'], q, S.DYN_B, C, per_sample), 'dyn_thres second run')
    d.unchanged()


@pytest.mark.parametrize('q', S.EXACT_QS)
@pytest.mark.parametrize('per_sample', S.EXACT_PERS)
def test_dynamic_threshold_exact_order_statistic(per_sample, q):
    """eps = 0 and frac = 0: the result is one order statistic of fl(kr x), bit for bit, whatever the ties around the wanted rank."""
    E = S.dyn_exact(per_sample, q)
    B = len(S.EXACT_PATTERNS)
    d = Dev(x=E['x'], eps=torch.zeros(B, 1, 1, per_sample, 1), t=E['t'], tab=S.dyn_tables())
    got = _dyn(d['x'], d['eps'], d['t'], d['tab'], q, B, 1, per_sample).numpy()
    for b, pattern in enumerate(S.EXACT_PATTERNS):
        print(f'[dyn_thres exact per={per_sample} q={q} {pattern}] got {got[b]!r} want {E["want"][b]!r} (rank {E["k"]}; below {E["below"][b]!r}, '
              f'above {E["above"][b]!r})')
    assert np.array_equal(got.view(np.uint32), E['want'].view(np.uint32))
    d.unchanged()


# ---- losses and their gradients ------------------------------------------------------------------------------------------------------------------

def _loss_masked(sh, d, mask_key, l2, fill):
    """vdx_loss_sum_masked: (sum, count) followed by the kernels' scratch, all inside one banded buffer."""
    L, G = _L(), _G()
    n = 2 + G.vdx_loss_masked_scratch_doubles()
    buf, acc = _out(n, dtype=F64)
    acc.fill_(fill)
    rc = G.vdx_loss_sum_masked(d.p('eps'), d.p('noise'), d.p(mask_key), acc.data_ptr() + 16, acc.data_ptr(), sh.B, sh.C, sh.fhw, int(l2), L.stream_ptr())
    return rc, buf, acc, n


@pytest.mark.parametrize('l2', [0, 1])
@pytest.mark.parametrize('name', ['WRAP', 'STRADDLE', 'RAGGED'])
def test_loss_sum_and_masked(name, l2):
    L, G, sh, I = _L(), _G(), SHAPES[name], S.loss_inputs(name)
    masked = sh is not RAGGED
    kinds = _masks_of(sh) + ('one',) if masked else ()
    d = Dev(eps=I['eps'], noise=I['noise'], **_mask_dev(sh, kinds))
    n = sh.B * S.per(sh)
    buf, acc = _out(1, dtype=F64)
    acc.zero_()
    L.check(G.vdx_loss_sum(d.p('eps'), d.p('noise'), acc.data_ptr(), sh.B, sh.C, sh.fhw, l2, L.stream_ptr()))
    got, ref = _finish(buf, 1).item() / n, S.loss_mean_ref(I['eps'], I['noise'], l2)
    print(f'[loss_sum {name} l2={l2}] mean {got!r} vs fp64 {ref!r}: error {abs(got - ref):.3e} (bound {S.LOSS_TOL:.0e})')
    assert abs(got - ref) < S.LOSS_TOL
    for k in _masks_of(sh) if masked else ():
        m = S.mask(name, k).bool()
        exp_sum, exp_n = S.FR.loss_sum_count(S.cf(I['eps']).double(), I['noise'].double(), m, l2)
        outs = []
        for fill in (NAN, 0.0):                                            # the kernels own the scratch: nothing in it is read first
            rc, mbuf, macc, mn = _loss_masked(sh, d, f'm_{k}', l2, fill)
            assert rc == 0
            outs.append(_finish(mbuf, mn)[:2])
        got_sum, got_n = outs[0][0].item(), outs[0][1].item()
        rel = abs(got_sum - exp_sum.item()) / abs(exp_sum.item())
        print(f'[loss_sum_masked {name} l2={l2} {k}] sum {got_sum!r} vs fp64 {exp_sum.item()!r}: relative error {rel:.3e} (bound '
              f'{S.LOSS_MASKED_RTOL:.0e}); count {got_n} vs {exp_n}')
        assert got_n == exp_n and rel <= S.LOSS_MASKED_RTOL
        assert torch.equal(outs[0].view(torch.int64), outs[1].view(torch.int64)), 'two runs: equal bits'
    if masked:
        rc, mbuf, macc, mn = _loss_masked(sh, d, 'm_one', l2, NAN)
        full = _finish(mbuf, mn)
        assert rc == 0 and full[0].item() == 0.0 and full[1].item() == 0.0
    else:
        rc, mbuf, macc, mn = _loss_masked(sh, d, 'noise', l2, NAN)         # channels * fhw % 4 != 0: refused before anything is read
        assert rc == INVALID
        _untouched(mbuf)
    d.unchanged()


@pytest.mark.parametrize('l2', [0, 1])
@pytest.mark.parametrize('name', ['WRAP', 'STRADDLE', 'RAGGED'])
def test_loss_grad_and_masked(name, l2):
    from video_diffusion_nnx_amd.train_step import vdx_loss_grad, vdx_loss_grad_masked
    L, sh, I = _L(), SHAPES[name], S.loss_inputs(name)
    masked = sh is not RAGGED
    kinds = _masks_of(sh) + ('zero', 'one') if masked else ()
    d = Dev(eps=I['eps'], noise=I['noise'], **_mask_dev(sh, kinds))
    n = sh.B * S.per(sh)

    def plain():
        buf, out = _out(n)
        L.check(vdx_loss_grad(d.p('eps'), d.p('noise'), out.data_ptr(), sh.B, sh.C, sh.fhw, l2, L.stream_ptr()))
        return _finish(buf, n, S.eps_dims(sh))
    got = plain()
    assert not torch.isnan(got).any()
    ref, ref32 = S.loss_grad_ref(I['eps'], I['noise'], l2, F64), S.loss_grad_ref(I['eps'], I['noise'], l2, F32)
    bd, rr = S.small_bound(ref32, ref), S.rel_l2(got, ref)
    print(f'[loss_grad {name} l2={l2}] rel {rr:.3e} (bound {bd:.3e}); {int(I["tie"].sum())} exact ties')
    assert rr < bd
    if sh is WRAP:                                                          # the elements of the later sweeps on their own
        lo = S.EW_BLOCKS * S.THREADS
        gs, rs, r32s = (v.reshape(-1)[lo:] for v in (got, ref, ref32))
        bd2, rr2 = S.small_bound(r32s, rs), S.rel_l2(gs, rs)
        print(f'[loss_grad {name} l2={l2}] sweeps 2 to 9: rel {rr2:.3e} (bound {bd2:.3e})')
        assert rr2 < bd2
    assert (got[I['tie']] == 0).all(), 'gradient at eps_hat == noise must be 0'
    _bits(got, plain(), 'loss_grad second run')
    if not masked:
        buf, out = _out(n)
        assert vdx_loss_grad_masked(d.p('eps'), d.p('noise'), d.p('noise'), d.p('noise'), out.data_ptr(), sh.B, sh.C, sh.fhw, l2, L.stream_ptr()) == INVALID
        _untouched(buf)
        d.unchanged()
        return

    def run(mask_key):
        rc, mbuf, macc, mn = _loss_masked(sh, d, mask_key, l2, 0.0)
        assert rc == 0
        buf, out = _out(n)
        L.check(vdx_loss_grad_masked(d.p('eps'), d.p('noise'), d.p(mask_key), macc.data_ptr() + 8, out.data_ptr(), sh.B, sh.C, sh.fhw, l2, L.stream_ptr()))
        return _finish(buf, n, S.eps_dims(sh))
    for k in _masks_of(sh):
        m = S.mask(name, k)
        gm = run(f'm_{k}')
        exp, bound = S.loss_grad_masked_ref(I['eps'], I['noise'], m, l2)
        S.check(S.cf(gm), exp, bound * (1 + 1e-12) + 1e-300, f'loss_grad_masked {name} l2={l2} {k}')
        assert (S.cf(gm)[m.bool()] == 0.0).all()
        _bits(gm, run(f'm_{k}'), f'loss_grad_masked {name} l2={l2} {k} second run')
    _bits(run('m_zero'), got, 'loss_grad_masked with an all-zero mask vs loss_grad')
    assert (run('m_one') == 0.0).all()
    d.unchanged()


# ---- classifier-free guidance ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['WRAP', 'STRADDLE'])
def test_cfg_combine(name):
    L, sh = _L(), SHAPES[name]
    B, per_sample, s = sh.B, S.per(sh), 7.5
    eps2 = S.cfg_inputs(name)
    d = Dev(eps2=eps2)
    n = B * per_sample

    def run(phi, inplace):
        scratch = torch.full((L.vdx_cfg_scratch_doubles(B),), NAN, dtype=F64, device=DEV) if phi else None
        buf, out = _out(2 * n if inplace else n, d['eps2'] if inplace else None)
        rc = L.vdx_cfg_combine(out.data_ptr() if inplace else d.p('eps2'), out.data_ptr(), s, phi, L.ptr(scratch), B, per_sample, L.stream_ptr())
        assert rc == 0, L.vdx_last_error()
        return _finish(buf, 2 * n if inplace else n).reshape(-1, per_sample)
    g, exp, factor = S.cfg_ref(eps2, B, s, 0.7)
    got = run(0.0, False)
    assert not torch.isnan(got).any()
    _bits(got, g, f'cfg_combine {name} vs torch\'s expression')
    print(f'[cfg_combine {name}] bit-equal to n + (c - n) * s over {n} elements')
    _bits(got, run(0.0, False), 'cfg_combine second run')
    work = run(0.0, True)
    _bits(work[:B], g, 'cfg_combine in place')
    _bits(work[B:], eps2[B:], 'cfg_combine in place: the null rows keep their bits')
    gr = run(0.7, False)
    err = np.abs(gr.numpy().astype(np.float64) - exp)
    worst = (err / np.maximum(np.abs(exp), 1e-300)).max()
    print(f'[cfg_combine {name} rescale 0.7] factors {factor}, worst relative error {worst / S.U24:.3f} x 2^-24 (bound 3)')
    assert not torch.isnan(gr).any() and (err <= 3 * S.U24 * np.abs(exp)).all()
    _bits(gr, run(0.7, False), 'cfg_combine rescale second run')
    wr = run(0.7, True)
    _bits(wr[:B], gr, 'cfg_combine rescale in place')
    _bits(wr[B:], eps2[B:], 'cfg_combine rescale in place: the null rows keep their bits')
    d.unchanged()


# ---- Adam ----------------------------------------------------------------------------------------------------------------------------------------------

def _adam_run(clip_norm=None):
    """One step on fresh banded copies of the shared inputs; clip_norm None: vdx_adam_ema_step, else vdx_adam_ema_step_clip."""
    from video_diffusion_nnx_amd import ops
    I, n = S.adam_inputs(), S.N_ADAM
    bufs = {k: _out(n, I[k].to(DEV)) for k in ('p', 'g', 'm', 'v', 'ema')}
    t = {k: bufs[k][1] for k in bufs}
    norm = None
    if clip_norm is None:
        ops.adam_ema_step(t['p'], t['g'], t['m'], t['v'], t['ema'], **S.ADAM_HYP)
    else:
        sqnorm = ops.grad_sqnorm(t['g'])                                    # alive until _finish has synchronised
        norm = ops.adam_ema_step_clip(t['p'], t['g'], t['m'], t['v'], t['ema'], sqnorm, clip_norm, **S.ADAM_HYP)
    got = {k: _finish(bufs[k][0], n) for k in bufs}
    assert torch.equal(got['g'], I['g']), 'the gradient buffer is read-only'
    got['dp'] = got['p'].double() - I['p'].double()
    if norm is not None:
        got['norm'] = norm.cpu()
    return got


def _adam_compare(got, ref, ref32, bound, what):
    """Per tensor rel-L2 against fp64 within bound(fp32-on-CPU result, fp64 result), over the whole buffer and over the part
    past the first sweep of the 4096 x 256 x 4 grid (2800 elements as quads, then the 3-element scalar tail)."""
    fails = []
    for k in ('p', 'dp', 'm', 'v', 'ema'):
        for part, sl in (('all', slice(None)), ('second sweep + tail', slice(S.ADAM_SWEEP, None))):
            bd = bound(ref32[k][sl], ref[k][sl])
            rr = S.rel_l2(got[k][sl], ref[k][sl])
            print(f'[{what}] {k} ({part}): rel {rr:.3e} (bound {bd:.3e})')
            if not rr < bd:
                fails.append((k, part, rr, bd))
    assert not fails, fails


def test_adam_ema_step_wraps():
    got = _adam_run()
    _adam_compare(got, S.adam_ref(F64), S.adam_ref(F32), S.small_bound, f'adam n={S.N_ADAM}')          # test_adam_ema_six_steps' rule
    again = _adam_run()
    for k in ('p', 'm', 'v', 'ema'):
        _bits(got[k], again[k], f'adam second run, {k}')


def test_adam_ema_step_clip_wraps():
    plain, noclip = _adam_run(), _adam_run(1e30)
    for k in ('p', 'm', 'v', 'ema'):
        _bits(plain[k], noclip[k], f'adam clip == 1 must leave the bits of vdx_adam_ema_step, {k}')
    got = _adam_run(S.ADAM_MAX_NORM)
    ref, ref32, unclipped = S.adam_ref(F64, S.ADAM_MAX_NORM), S.adam_ref(F32, S.ADAM_MAX_NORM), S.adam_ref(F64)
    assert ref['norm'].item() > 10 * S.ADAM_MAX_NORM                                          # the clip is active
    _adam_compare(got, ref, ref32, S.clip_bound, f'adam clip n={S.N_ADAM}')                   # test_adam_clip_kernel_matches_fp64_restatement's rule
    e32, e = S.rel_l2(ref32['norm'], ref['norm']), S.rel_l2(got['norm'], ref['norm'])
    print(f'[adam clip norm] fp32-on-CPU rel {e32:.3e}  bound {8 * e32:.3e}  kernel rel {e:.3e}')
    assert e <= 8 * e32
    for k in ('m', 'v'):
        assert S.rel_l2(unclipped[k], ref[k]) > S.clip_bound(ref32[k], ref[k]), f'{k}: the bound does not tell a missing clip apart'


# ---- RAGGED: the float4 kernels refuse per_sample % 4 != 0 and leave the output alone ----------------------------------------------------------------

def test_ragged_is_refused_untouched():
    L, G, sh = _L(), _G(), RAGGED
    I, n, per_sample = S.step_inputs('RAGGED', 5, 2.0), RAGGED.B * S.per(RAGGED), S.per(RAGGED)
    tp, td, tq = _tabs(S.T_P), _tabs(S.T_D), _tabs(S.T_Q)
    d = Dev(x=I['x'], eps=I['eps'], z=I['z'], hist=I['hist'], known=I['known'], t=S.t_vec(sh, S.T_Q).to(torch.int32), m=S.mask('RAGGED', 'p04'),
            seq=torch.from_numpy(S.time_sequence(S.T_D, S.S_DPM)), eps2=S.cfg_inputs('RAGGED'))
    st = L.stream_ptr()
    calls = {
        'q_sample': lambda o: G.vdx_q_sample(d.p('x'), d.p('t'), d.p('z'), o, tq.p('sqrt_ac'), tq.p('sqrt_1mac'), sh.B, per_sample, 2.0, -1.0, st),
        'q_sample_masked': lambda o: G.vdx_q_sample_masked(d.p('x'), d.p('t'), d.p('z'), d.p('m'), o, tq.p('sqrt_ac'), tq.p('sqrt_1mac'), sh.B, per_sample,
                                                           2.0, -1.0, st),
        'p_sample_masked': lambda o: G.vdx_p_sample_step_masked(d.p('x'), d.p('eps'), o, d.p('t'), tp.p('ptab'), S.T_P, d.p('known'), d.p('m'), tp.p('mtab'),
                                                                1, 91, 7, 0, 0, 1, sh.B, sh.C, per_sample, st),
        'ddim_masked': lambda o: G.vdx_ddim_step_masked(d.p('x'), d.p('eps'), o, td.p('ac'), d.p('seq'), 0, 0, 1, d.p('known'), d.p('m'), td.p('mtab'),
                                                        S.T_D, 17, sh.B, sh.C, per_sample, st),
        'dpm': lambda o: G.vdx_dpm_step(d.p('x'), d.p('eps'), o, d.p('hist'), td.p('ac'), d.p('seq'), 0, 0, 1, 2, sh.B, sh.C, per_sample, st),
        'dpm_masked': lambda o: G.vdx_dpm_step_masked(d.p('x'), d.p('eps'), o, d.p('hist'), td.p('ac'), d.p('seq'), 0, 0, 1, 2, d.p('known'), d.p('m'),
                                                      td.p('mtab'), S.T_D, 17, sh.B, sh.C, per_sample, st),
        'cfg_combine': lambda o: L.vdx_cfg_combine(d.p('eps2'), o, 7.5, 0.0, 0, sh.B, per_sample, st),
    }
    for what, call in calls.items():
        buf, out = _out(n)
        assert call(out.data_ptr()) == INVALID, what
        _untouched(buf)
    buf, out = _out(n, d['z'])                                             # in place: x must keep its bits
    assert G.vdx_inpaint_init(out.data_ptr(), d.p('known'), d.p('m'), tp.p('mtab'), S.T_P, S.T_P - 1, n, st) == INVALID
    assert torch.equal(_finish(buf, n), I['z'].reshape(-1))
    d.unchanged()
