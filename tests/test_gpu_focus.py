"""GPU tests of the focus-present mask (Unet3D(focus_present=True)): the FOCUS instantiations of the generic attention
kernels and attention_present_kernel at block level, the focus forms of the backward cores, and the network with the switch on -- forward,
gradients, sampling graphs, one train step -- against the fp64 references of tests/_focus_ref.py.  Every case asserts through
tests/_launch_hook.py which kernel served it.  Bounds are the ones tests/test_gpu_posbias.py states for the same kernels."""
import contextlib
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _focus_ref as FR
import _launch_hook as LH
import _parity as P
import _posbias_ref as PB
from oracle import philox_ref, train_ref, unet3d_ref as R
from oracle.diffusion_ref import DiffusionRef

DEV = 'cuda'
F64 = torch.float64
EMB = 'time_rel_pos_bias.relative_attention_bias.embedding'
TOL = {'f32': 2e-5, 'bf16': 1.5e-2, 'bf16io': 4e-2}          # tests/test_gpu_posbias.py / test_gpu_blocks.py, on the attention branch
MODE_ID = {'f32': 0, 'bf16': 1, 'f16': 2, 'bf16io': 1}
ALL = ('f32', 'bf16', 'f16', 'bf16io')


def _rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _mha(C, heads, g):
    HD = heads * 32
    return (torch.randn(C, 3 * HD, generator=g) / C ** 0.5, torch.randn(3 * HD, generator=g) * 0.2,
            torch.randn(HD, C, generator=g) / HD ** 0.5, torch.randn(C, generator=g) * 0.2)


def _pack(w, mode):
    from video_diffusion_nnx_amd import ops
    wqkv, bqkv, wo, bo = w
    return (ops.pack_conv_weights(wqkv.to(DEV).contiguous(), mode), bqkv.to(DEV), ops.pack_conv_weights(wo.to(DEV).contiguous(), mode), bo.to(DEV))


def _seq_view(t):
    """[B, F, H, W, C] -> one group per temporal sequence"""
    B, Fr, H, W, C = t.shape
    return [t.permute(0, 2, 3, 1, 4).reshape(B * H * W, Fr * C)]


def _inputs(shape, mode):
    B, Fr, H, W, C, heads = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, Fr, H, W, C, generator=g)
    w = _mha(C, heads, g)
    bias = PB.bias_table(torch.randn(32, heads, generator=g), Fr)
    if mode == 'bf16io':
        x = x.bfloat16()
    elif mode == 'f16':
        x = P.f16r(x)                                                    # (the f16 kernels stage x exactly when it is fp16-representable)
    return x, w, bias


# ---- 1. masked block forward -----------------------------------------------------------------------------------------------------------
FWD_CASES = [
    # (B, F, H, W, C, heads), modes, mask, kernel, shape-string parts: workgroups straddle samples with different flags
    ((3, 16, 3, 2, 64, 8), ALL, [1, 0, 1], 'attention_reg_kernel', '{m}, 4, {f}> C64 L16 nseq18'),     # 4 sequences per workgroup, 6 per sample
    ((2, 10, 3, 3, 32, 8), ALL, [0, 1], 'attention_reg_kernel', '{m}, 4, {f}> C32 L10 nseq18'),        # masked keys plus focus
    ((2, 3, 2, 2, 128, 8), ALL, [1, 0], 'attention_reg_kernel', '{m}, 8, {f}> C128 L3 nseq8'),
    ((2, 16, 2, 2, 512, 8), ALL, [0, 1], 'attention_reg_kernel', '{m}, 32, {f}> C512 L16 nseq8'),
    ((2, 16, 2, 2, 528, 8), ('f32',), [0, 1], 'attention_kernel', '{m}, 16, 16, {f}> C528 L16 nseq8'),  # f32, C > 512: the staged kernel at LP 16
    ((3, 20, 3, 3, 16, 4), ALL, [1, 0, 1], 'attention_kernel', '{m}, 32, 1, {f}> C16 L20 nseq27'),     # LP 32: 2 sequences per workgroup, 9 per sample
    ((2, 40, 2, 2, 64, 8), ALL, [1, 0], 'attention_kernel', '{m}, 64, 1, {f}> C64 L40 nseq8'),         # LP 64
]


@pytest.mark.parametrize('biased', [False, True], ids=['nobias', 'bias'])
@pytest.mark.parametrize('case', [(c, m) for c in FWD_CASES for m in c[1]], ids=lambda cm: f'{cm[0][0]}-{cm[1]}')
def test_block_forward(case, biased):
    from video_diffusion_nnx_amd import ops
    (shape, _, mask, kernel, parts), mode = case
    B, Fr, H, W, C, heads = shape
    x, w, bias = _inputs(shape, mode)
    io16 = mode == 'bf16io'
    op = 'bf16' if io16 else mode
    packed = _pack(w, op)
    xd = x.to(DEV)
    focus = torch.tensor(mask)
    bd = bias.to(DEV) if biased else None
    with LH.launches() as rec, LH.nan_outputs():
        y = ops.attention_forward_focus(xd, packed, focus, heads, True, op, bias=bd)
        torch.cuda.synchronize()
    LH.assert_launches(rec, [(kernel, [parts.format(m=f'<{MODE_ID[mode]}', f='bias+focus' if biased else 'focus'), f'io16 {int(io16)}'])], f'{shape} {mode}')
    assert torch.isfinite(y).all()
    # unmasked samples: bit-equal to the same kernel family launched without a mask (a zero table where there is no bias)
    y_plain = ops.attention_forward_bias(xd, packed, bd if biased else torch.zeros_like(bias).to(DEV), heads, True, op)
    y_pres = ops.attention_present_forward(xd, packed, heads, True, op)
    x64 = x.double()
    args = [t.double() for t in w]
    ref_branch, _ = FR.attention_block_focus(x64, *args, focus, bias=bias.double() if biased else None, heads=heads)
    got = y.double().cpu() - x64
    plain = y_plain.double().cpu() - x64
    pres = y_pres.double().cpu() - x64
    if mode == 'f16':
        emu, _ = FR.attention_block_focus(x64, *args, focus, bias=bias.double() if biased else None, heads=heads, emulate=True, operand='f16')
        bound = P.view_bound(emu, ref_branch, _seq_view)
    else:
        bound = TOL[mode]
    for b in range(B):
        if not mask[b]:
            assert torch.equal(y[b], y_plain[b]), (shape, mode, b)
            continue
        sl = slice(b, b + 1)
        if mode == 'f16':
            worst = P.assert_views(got[sl], ref_branch[sl], _seq_view, bound, f'masked attention f16 {shape} sample {b}')
            P.assert_views(got[sl], pres[sl] , _seq_view, bound, f'masked attention f16 {shape} sample {b} vs the present kernel')
            moved = float(P.view_rels(plain[sl], ref_branch[sl], _seq_view).min())
        else:
            worst, vs_pres = _rel(got[sl], ref_branch[sl]), _rel(got[sl], pres[sl])
            print(f'masked attention {shape} {mode} sample {b}: branch rel {worst:.3e}, vs the present kernel {vs_pres:.3e} (bound {bound:.1e})')
            assert worst < bound and vs_pres < bound, (shape, mode, b, worst, vs_pres)
            moved = _rel(plain[sl], ref_branch[sl])
        # the case proves something only if the mask moves the sample's branch by far more than the bound
        print(f'   the mask moves the branch of sample {b} by {moved:.3e}')
        assert moved > 10 * bound, (shape, mode, b, moved, bound)
    y2 = ops.attention_forward_focus(xd, packed, focus, heads, True, op, bias=bd)
    assert torch.equal(y, y2)


# ---- 2. the present kernel -------------------------------------------------------------------------------------------------------------
PRESENT_CASES = [
    ((1, 5, 3, 3, 64, 8), ALL, 1),        # 45 rows: one ragged tile
    ((2, 16, 2, 2, 512, 8), ALL, 8),
    ((1, 10, 3, 3, 32, 8), ALL, 1),
    ((1, 3, 2, 2, 128, 8), ALL, 2),
    ((1, 16, 2, 2, 1024, 8), ALL, 16),
    ((1, 16, 2, 2, 528, 8), ('f32',), 16),
    ((1, 20, 3, 3, 16, 4), ALL, 1),
]


def _tile_view(t):
    """[B, F, H, W, C] -> one group per 64 consecutive token rows of the launch (row = token r % L of sequence r / L: what one workgroup
    of attention_present_kernel owns), the ragged last tile a group of its own"""
    B, Fr, H, W, C = t.shape
    return P.pixel_tile_view(64)(t.permute(0, 2, 3, 1, 4).reshape(1, B * H * W * Fr, C))


@pytest.mark.parametrize('case', [(c, m) for c in PRESENT_CASES for m in c[1]], ids=lambda cm: f'{cm[0][0]}-{cm[1]}')
def test_present_kernel(case):
    """Against fp64 x + bo + Wo (Wv x + bv) at TOL, and per 64-row tile at 3 x the emulation that rounds v once to the operand type
    (P.view_bound); f32 has no rounding point, so its per-tile bound is the exact-products kind (P.f32_group_bounds: max(2e-6, 8 x the
    same formula in fp32 on the CPU))."""
    from video_diffusion_nnx_amd import ops
    (shape, _, tmo), mode = case
    B, Fr, H, W, C, heads = shape
    x, w, _ = _inputs(shape, mode)
    io16 = mode == 'bf16io'
    op = 'bf16' if io16 else mode
    packed = _pack(w, op)
    xd = x.to(DEV)
    with LH.launches() as rec, LH.nan_outputs():
        y = ops.attention_present_forward(xd, packed, heads, True, op)
        torch.cuda.synchronize()
    LH.assert_launches(rec, [('attention_present_kernel', [f'<{MODE_ID[mode]}, {tmo}> C{C} rows{B * Fr * H * W} ', f'io16 {int(io16)}'])], f'{shape} {mode}')
    assert torch.isfinite(y).all()
    x64 = x.double()
    args = [t.double() for t in w]
    ref, _ = FR.present_block(x64, *args, heads=heads)
    got = y.double().cpu() - x64
    if mode == 'f16':
        emu, _ = FR.present_block(x64, *args, heads=heads, emulate=True, operand='f16')
        P.assert_views(got, ref, _seq_view, P.view_bound(emu, ref, _seq_view), f'present f16 {shape}')
    else:
        r = _rel(got, ref)
        print(f'present kernel {shape} {mode}: branch rel {r:.3e} (bound {TOL[mode]:.1e})')
        assert r < TOL[mode]
    if mode == 'f32':
        e32, _ = FR.present_block(x, *w, heads=heads, dtype=torch.float32)
        tb = P.f32_group_bounds(e32.double(), ref, _tile_view)
    else:
        eb, ey = FR.present_block(x64, *args, heads=heads, emulate=True, operand=op, round_out=io16)
        tb = P.view_bound((ey - x64) if io16 else eb, ref, _tile_view)      # bf16 tensors: the branch as read off the rounded y
    P.assert_views(got, ref, _tile_view, tb, f'present {mode} {shape} per 64-row tile')
    assert torch.equal(y, ops.attention_present_forward(xd, packed, heads, True, op))


# ---- 3. masked backward cores ----------------------------------------------------------------------------------------------------------
BWD_CASES = [
    # B, F, H, W, bf16_operands, io_bf16, kernel, mask: the geometries of test_gpu_posbias.py::BWD_CASES with B >= 2 and a mixed mask
    (2, 16, 3, 3, True, False, 'attn_core_bwd16_focus_kernel', [1, 0]),
    (2, 16, 3, 3, True, True, 'attn_core_bwd16_focus_kernel', [0, 1]),
    (2, 10, 2, 2, True, False, 'attn_core_bwd16_focus_kernel', [1, 0]),
    (2, 10, 2, 2, True, True, 'attn_core_bwd16_focus_kernel', [1, 0]),
    (3, 20, 2, 2, False, False, 'attn_core_bwd_focus_kernel', [1, 0, 1]),
    (2, 10, 2, 2, False, False, 'attn_core_bwd_focus_kernel', [0, 1]),
    (2, 20, 2, 2, True, False, 'attn_core_bwd_focus_kernel', [1, 0]),
]


@pytest.mark.parametrize('biased', [False, True], ids=['nobias', 'bias'])
@pytest.mark.parametrize('case', BWD_CASES, ids=str)
def test_block_backward(case, biased):
    from video_diffusion_nnx_amd import ops
    B, Fr, H, W, bf16_ops, io16, kernel, mask = case
    heads, HD, HW = 8, 256, H * W
    npix = B * Fr * HW
    g = torch.Generator().manual_seed(B + Fr + H + 17)
    qkv = torch.randn(npix, 3 * HD, generator=g)
    d_o = torch.randn(npix, HD, generator=g)
    bias = PB.bias_table(torch.randn(32, heads, generator=g), Fr) if biased else None
    mfma = bf16_ops and Fr <= 16
    dt = torch.bfloat16 if io16 else torch.float32
    o_ref, g_ref, db_ref = FR.attn_core_focus(qkv, d_o, mask, B, Fr, HW, heads, bias=bias)
    tol_o, tol_g = (1.5e-2, 1.5e-2) if mfma else (1e-5, 2e-5)
    runs = []
    for _ in range(2):
        with LH.launches() as rec, LH.nan_outputs():
            o, dqkv, dbias = ops.attention_core_backward_focus(qkv.to(DEV, dt), d_o.to(DEV, dt), mask, B, Fr, H, W, heads, True,
                                                               bf16_operands=bf16_ops, bias=None if bias is None else bias.to(DEV))
            torch.cuda.synchronize()
        want = [(kernel, [f'bias {int(biased)}> L{Fr} nseq{B * HW} heads8'])] + ([('attn_dbias_sum_kernel', [f'heads8 L{Fr}'])] if biased else [])
        LH.assert_launches(rec, want, str(case))
        runs.append((o, dqkv) + ((dbias,) if biased else ()))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    o, dqkv = runs[0][0].double().cpu(), runs[0][1].double().cpu()
    ro, rg = _rel(o, o_ref), _rel(dqkv, g_ref)
    print(f'[focus bwd] {case} bias {biased}: o {ro:.3e} (bound {tol_o:.1e}), dqkv {rg:.3e} ({tol_g:.1e})')
    assert ro < tol_o and rg < tol_g
    for nm, a, b in (('dq', 0, HD), ('dk', HD, 2 * HD), ('dv', 2 * HD, 3 * HD)):
        assert _rel(dqkv[:, a:b], g_ref[:, a:b]) < tol_g, (case, nm)
    # masked samples, exactly: dq == dk == 0, dv == dO and O == v after the tensor's storage rounding
    rows = torch.arange(npix).reshape(B, Fr * HW)
    st = (lambda t: P.bf16r(t.double())) if (io16 or mfma) else (lambda t: t.double())
    for b in range(B):
        if not mask[b]:
            continue
        r = rows[b]
        assert (dqkv[r, :2 * HD] == 0).all(), (case, b)
        src_do = d_o.to(dt).double() if io16 else d_o.double()
        src_v = qkv.to(dt).double()[:, 2 * HD:] if io16 else qkv.double()[:, 2 * HD:]
        assert torch.equal(dqkv[r, 2 * HD:], st(src_do[r])), (case, b, 'dv == dO')
        assert torch.equal(o[r], st(src_v[r])), (case, b, 'O == v')
    if biased:
        # dBias within the bounds of test_gpu_posbias.py, of the reference computed on the UNMASKED samples alone
        keep = torch.cat([rows[b] for b in range(B) if not mask[b]])
        nb = len(keep) // (Fr * HW)
        _, _, db_un = PB.attn_core_bias(qkv[keep], d_o[keep], bias, nb, Fr, HW, heads, True)
        if mfma:
            _, _, db_emu = PB.attn_core_bias(qkv[keep], d_o[keep], bias, nb, Fr, HW, heads, True, emulate=True, round_out=io16)
            db_bound = 3.0 * _rel(db_emu, db_un)
        else:
            _, _, db32 = PB.attn_core_bias(qkv[keep], d_o[keep], bias, nb, Fr, HW, heads, True, dtype=torch.float32)
            db_bound = max(2e-5, 8.0 * _rel(db32.double(), db_un))
            assert db_bound < P.EXACT_CEILING
        rb = _rel(runs[0][2].double().cpu(), db_un)
        print(f'   dBias {rb:.3e} (bound {db_bound:.3e})')
        assert rb < db_bound, (case, rb, db_bound)
        assert _rel(db_ref, db_un) < 1e-12


# ---- network ---------------------------------------------------------------------------------------------------------------------------
KW = dict(dim=16, channels=1)
NINE = [f'downs.{i}.3' for i in range(4)] + ['mid_temporal_attn'] + [f'ups.{i}.3' for i in range(4)]
FWD_TOL = {'f32': 2e-5, 'bf16': 2e-2, 'f16': 4e-3, 'bf16+act16': 3e-2}      # tests/test_gpu_posbias.py::test_network_forward
BWD_TOL = {'f32': 2e-4, 'bf16': 6e-2, 'bf16+act16': 7e-2}                   # tests/test_gpu_posbias.py::test_network_gradients
MASK3 = [1, 0, 1]


@functools.lru_cache(maxsize=None)
def _net_inputs(frames):
    cfg = R.UnetConfig(**KW)
    p64 = R.random_params(cfg, seed=7, dtype=F64)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 1, frames, 16, 16, generator=g)
    t = torch.randint(0, 1000, (3,), generator=g)
    d_out = torch.randn(3, frames, 16, 16, 1, generator=g)
    return cfg, p64, x, t, d_out


@functools.lru_cache(maxsize=None)
def _net_ref(frames, focus, pos, want_grads=False):
    """Shared fp64 reference at B = 3: the patched forward under the mask `focus` (a tuple, or None) and, on request, all gradients."""
    cfg, p64, x, t, d_out = _net_inputs(frames)
    fm = None if focus is None else torch.tensor(focus)
    if not want_grads:
        with torch.no_grad(), (FR.patched(fm, pos) if (fm is not None or pos) else contextlib.nullcontext()):
            return R.unet_forward(p64, cfg, x.double(), t), None
    leaves = {k: v.clone().requires_grad_(True) for k, v in p64.items()}
    with FR.patched(fm, pos):
        out = R.unet_forward(leaves, cfg, x.double(), t)
    gr = torch.autograd.grad(out, list(leaves.values()), d_out.double(), allow_unused=True)
    return out.detach(), {k: (torch.zeros_like(v) if q is None else q) for (k, v), q in zip(leaves.items(), gr)}


def _model(mode, p64=None, on=True, pos=False, rngs=0, **kw):
    from video_diffusion_nnx_amd.unet3d import Unet3D
    m = Unet3D(rngs=rngs, mode=mode.split('+')[0], focus_present=on, temporal_pos_bias=pos, **{**KW, **kw})
    if p64 is not None:
        m.load_state_dict({k: v.float() for k, v in p64.items()})
    return m


def _attn_launches(rec):
    return [(k, s) for k, s in rec if k.startswith('attention') or k.startswith('attn_') or k.startswith('pos_bias')]


@pytest.mark.parametrize('mode,frames', [('f32', 5), ('bf16', 5), ('f16', 5), ('bf16+act16', 5), ('bf16', 10)])
def test_network_forward(mode, frames):
    cfg, p64, x, t, _ = _net_inputs(frames)
    tol = FWD_TOL[mode]
    m = _model(mode, p64)
    m.act_bf16 = mode.endswith('+act16')
    plain = _net_ref(frames, None, False)[0]
    with LH.launches() as rec_off:
        y_off = m(x, t).clone()                                          # switch on, no mask, p = 0: nothing is masked
    assert _rel(y_off.cpu().double(), plain) < tol
    init_launch = _attn_launches(rec_off)[0]
    # a mixed batch
    ref = _net_ref(frames, tuple(MASK3), False)[0]
    with LH.launches() as rec:
        y = m(x, t, focus_present_mask=torch.tensor(MASK3)).clone()
        torch.cuda.synchronize()
    r = _rel(y.cpu().double(), ref)
    print(f'network forward, mask {MASK3}, {mode}, {frames} frames: rel {r:.3e} (bound {tol:.1e})')
    assert r < tol
    assert _rel(y.cpu().double(), plain) > 3 * tol                       # a forward that ignored the mask would miss the bound
    att = _attn_launches(rec)
    assert att[0] == init_launch, att                                    # init_temporal_attn: what it runs without the feature
    masked = [(k, s) for k, s in att if 'focus>' in s]
    assert len(masked) == 9 and all(k == 'attention_reg_kernel' and ', focus>' in s and f'L{frames} ' in s for k, s in masked), att
    assert len(att) == 11
    # ... with the position bias on
    m.temporal_pos_bias = True
    ref_pos = _net_ref(frames, tuple(MASK3), True)[0]
    with LH.launches() as rec:
        y_pos = m(x, t, focus_present_mask=torch.tensor(MASK3)).clone()
    r = _rel(y_pos.cpu().double(), ref_pos)
    print(f'   with the position bias: rel {r:.3e}')
    assert r < tol
    att = _attn_launches(rec)
    assert att[0][0] == 'pos_bias_table_kernel' and 'bias>' in att[1][1] and 'focus' not in att[1][1]
    assert len([s for _, s in att if 'bias+focus>' in s]) == 9
    m.temporal_pos_bias = False
    # ... and all-present: nine launches of the present kernel, the init block as before
    ref_all = _net_ref(frames, (1,), False)[0]
    with LH.launches() as rec:
        y_all = m(x, t, prob_focus_present=1.0).clone()
    r = _rel(y_all.cpu().double(), ref_all)
    print(f'   all-present: rel {r:.3e}')
    assert r < tol
    att = _attn_launches(rec)
    assert att[0] == init_launch and [k for k, _ in att].count('attention_present_kernel') == 9 and len(att) == 11, att
    # an all-ones per-sample mask is the same network on the masked generic route
    y_ones = m(x, t, focus_present_mask=torch.ones(3))
    assert _rel(y_ones.cpu().double(), ref_all) < tol


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_off_means_off(mode):
    import test_gpu_posbias as TP
    cfg = R.UnetConfig(**KW)
    p64 = R.random_params(cfg, seed=7, dtype=F64)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 1, 5, 16, 16, generator=g)
    t = torch.randint(0, 1000, (2,), generator=g)
    parent = [tuple(e) for e in TP.PARENT_ATTN[mode]]
    m = _model(mode, p64, on=False)
    y0 = m(x, t).clone()
    with LH.launches() as rec:
        y1 = m(x, t, focus_present_mask=torch.tensor([1, 0]), prob_focus_present=1.0).clone()      # switch off: accepted and ignored
    assert torch.equal(y0, y1) and _attn_launches(rec) == parent
    m.focus_present = True
    with LH.launches() as rec:
        y2 = m(x, t).clone()                                             # switch on, no mask, p = 0
    assert torch.equal(y0, y2) and _attn_launches(rec) == parent
    y3 = m(x, t, focus_present_mask=torch.tensor([1, 0])).clone()
    assert not torch.equal(y0[0], y3[0])
    with LH.launches() as rec:
        y4 = m(x, t).clone()                                             # ... and back
    assert torch.equal(y0, y4) and _attn_launches(rec) == parent


def _backward(m, d_out, staged):
    grads = torch.full_like(m.flat_params, 3.0)
    ns = m.num_stages
    if staged:
        m.backward(d_out, grads, ns - 1, ns - 1)
        m.backward(d_out, grads, ns - 2, 2)
        m.backward(d_out, grads, 1, 0)
    else:
        m.backward(d_out, grads)
    torch.cuda.synchronize()
    return grads


def _grad_dict(m, grads):
    return {n: grads[o:o + int(np.prod(s))].cpu().double().reshape(s) for n, s, o in m.param_table}


@pytest.mark.parametrize('mode', ['f32', 'bf16', 'bf16+act16'])
def test_network_gradients(mode):
    cfg, p64, x, t, d_out = _net_inputs(5)
    tol = BWD_TOL[mode]
    core = 'attn_core_bwd_focus_kernel' if mode == 'f32' else 'attn_core_bwd16_focus_kernel'
    m = _model(mode, p64)
    m.act_bf16 = 2 if mode.endswith('+act16') else False
    # a mixed batch against autograd through the patched oracle
    _, ref_grads = _net_ref(5, tuple(MASK3), False, True)
    m(x, t, focus_present_mask=torch.tensor(MASK3))
    with LH.launches() as rec:
        grads = _backward(m, d_out.to(DEV), staged=True)
    names = [k for k, _ in rec]
    assert names.count(core) == 9 and 'attn_dbias_sum_kernel' not in names, names
    got = _grad_dict(m, grads)
    total_ref = torch.cat([ref_grads[n].reshape(-1) for n, _, _ in m.param_table])
    total_got = torch.cat([got[n].reshape(-1) for n, _, _ in m.param_table])
    scale = total_ref.norm().item()
    bad = [(n, _rel(got[n], ref_grads[n])) for n, _, _ in m.param_table if ref_grads[n].norm() > 1e-6 * scale and _rel(got[n], ref_grads[n]) > 5 * tol]
    assert not bad, sorted(bad, key=lambda z: -z[1])[:6]
    rt = _rel(total_got, total_ref)
    print(f'network gradients, mask {MASK3}, {mode}: all {rt:.3e} (bound {tol:.1e})')
    assert rt < tol
    g2 = _backward(m, d_out.to(DEV), staged=False)
    assert torch.equal(grads, g2)
    # all-present, with the position bias: q / k of the nine blocks get exactly nothing, the init block trains, and the embedding's
    # gradient is the init block's contribution alone (what the patched oracle gives: its masked blocks add exactly 0)
    _, ref_all = _net_ref(5, (1,), True, True)
    m.temporal_pos_bias = True
    m(x, t, prob_focus_present=1.0)
    with LH.launches() as rec:
        grads = _backward(m, d_out.to(DEV), staged=False)
    names = [k for k, _ in rec]
    assert names.count(core) == 9 and names.count('attn_dbias_sum_kernel') == 10
    got = _grad_dict(m, grads)
    for blk in NINE:
        for part in ('q', 'k'):
            for leaf in ('kernel', 'bias'):
                n = f'{blk}.fn.fn.fn.{part}.{leaf}'
                assert (got[n] == 0).all() and (ref_all[n] == 0).all(), n
        assert got[f'{blk}.fn.fn.fn.v.kernel'].abs().max() > 0
    for part in ('q', 'k'):
        assert got[f'init_temporal_attn.fn.fn.fn.{part}.kernel'].abs().max() > 0
    re = _rel(got[EMB], ref_all[EMB])
    ra = _rel(torch.cat([got[n].reshape(-1) for n, _, _ in m.param_table]), torch.cat([ref_all[n].reshape(-1) for n, _, _ in m.param_table]))
    print(f'   all-present with the position bias, {mode}: all {ra:.3e}, embedding {re:.3e} (bound {tol:.1e})')
    assert ref_all[EMB].norm().item() > 0 and re < tol and ra < tol


def test_c_abi_state_errors():
    """Handle state under the C ABI: a forward whose batch is no multiple of the stored mask's length is VDX_ERR_INVALID, fp8 attention
    on a handle with focus on is VDX_ERR_STATE (and the other way round), and nothing is launched by a refused call."""
    from video_diffusion_nnx_amd import _lib as L, unet3d as U
    cfg, p64, x, t, _ = _net_inputs(5)
    m = _model('bf16', p64)
    h = m.handle(5, 16)
    m(x, t, focus_present_mask=torch.tensor(MASK3))
    assert U.vdx_get_focus_present(h.ptr) == 2
    assert U.vdx_set_attention_fp8(h.ptr, 1) == -4
    real = m.resolve_focus
    m.resolve_focus = lambda batch, *a, **k: torch.tensor([1, 0], dtype=torch.uint8)      # (past the Python check: B = 3, n = 2)
    try:
        with LH.launches() as rec, pytest.raises(L.VdxError, match='status -1'):
            m(x, t)
    finally:
        m.resolve_focus = real
    assert not _attn_launches(rec)
    m(x, t)                                                              # no mask: mode 0 again
    assert U.vdx_get_focus_present(h.ptr) == 0
    assert U.vdx_set_attention_fp8(h.ptr, 1) == 0
    buf = torch.ones(3, dtype=torch.uint8, device=DEV)
    assert U.vdx_set_focus_present(h.ptr, 2, buf.data_ptr(), 3) == -4
    assert U.vdx_set_focus_present(h.ptr, 1, None, 0) == -4
    assert U.vdx_set_attention_fp8(h.ptr, 0) == 0
    assert U.vdx_set_focus_present(h.ptr, 1, None, 0) == 0 and U.vdx_get_focus_present(h.ptr) == 1
    assert U.vdx_set_focus_present(h.ptr, 0, None, 0) == 0


# ---- 7. samplers and graphs ------------------------------------------------------------------------------------------------------------
def test_samplers_and_graphs():
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    cfg, p64, _, _, _ = _net_inputs(5)
    m = _model('bf16', p64)
    never = _model('bf16', p64, on=False)
    gd = GaussianDiffusion(m, image_size=16, num_frames=5, channels=1, timesteps=4)
    gd0 = GaussianDiffusion(never, image_size=16, num_frames=5, channels=1, timesteps=4)
    mask = torch.tensor([1, 0])
    loops = {'ddpm': lambda g, **kw: g.p_sample_loop((2,), key=5, **kw), 'ddim': lambda g, **kw: g.ddim_sample_loop((2,), key=5, steps=2, **kw),
             'dpm': lambda g, **kw: g.dpm_sample_loop((2,), key=5, steps=2, **kw)}
    for name, run in loops.items():
        base = run(gd0).clone()
        off = run(gd).clone()
        assert torch.equal(off, base), name
        for fp in (mask, True):
            cap = run(gd, focus_present=fp).clone()
            eager = run(gd, focus_present=fp, use_graph=False).clone()
            assert torch.equal(cap, eager), (name, fp)                   # captured == eager, bit for bit
            assert not torch.equal(cap, base), (name, fp)
        assert torch.equal(run(gd).clone(), base), name                  # toggled on and off again: a handle that never had it
    a = loops['ddpm'](gd, focus_present=torch.tensor([1, 0])).clone()
    b = loops['ddpm'](gd, focus_present=torch.tensor([0, 1])).clone()
    assert not torch.equal(a, b)
    assert torch.equal(b, loops['ddpm'](gd, focus_present=torch.tensor([0, 1]), use_graph=False))
    with pytest.raises(ValueError):
        loops['ddpm'](gd0, focus_present=True)                           # needs the switch
    with pytest.raises(ValueError):
        loops['ddpm'](gd, focus_present=torch.tensor([1, 0, 1]))         # wrong length
    # guided: 2B rows through a [B] mask
    cm = _model('bf16', None, rngs=3, cond_dim=8)
    gdc = GaussianDiffusion(cm, image_size=16, num_frames=5, channels=1, timesteps=4)
    cond = torch.randn(2, 8, generator=torch.Generator().manual_seed(1))
    plain = gdc.p_sample_loop((2,), key=5, cond=cond, cond_scale=2.0).clone()
    cap = gdc.p_sample_loop((2,), key=5, cond=cond, cond_scale=2.0, focus_present=mask).clone()
    eager = gdc.p_sample_loop((2,), key=5, cond=cond, cond_scale=2.0, focus_present=mask, use_graph=False).clone()
    torch.cuda.synchronize()
    assert torch.equal(cap, eager) and not torch.equal(cap, plain)
    s = gdc.sample(5, cond=cond, cond_scale=2.0, focus_present=mask)
    assert torch.equal(s, cap)
    # fp8 attention and the switch exclude each other
    m.attn_fp8 = True
    with pytest.raises(ValueError):
        m(torch.zeros(1, 1, 5, 16, 16), torch.zeros(1, dtype=torch.long))
    m.attn_fp8 = False


def test_mask_contents_change_without_a_new_capture():
    """The handle stores the caller's mask POINTER: new contents in the same buffer reach the next replay of the captured loop, which
    launches through no launcher (nothing is recorded); switching the feature off drops the graph.  On the fixed buffers of
    tests/test_gpu_sample_loops.py's rig (the graph key holds every buffer's address)."""
    import test_gpu_sample_loops as SL
    r = SL.Rig(False)
    u = r.unet
    u.focus_present = True
    entry = SL.VARIANTS['p'][0]

    def go(mask, use_graph):
        u._focus = u.resolve_focus(SL.B, mask)
        u.apply_activation_storage(r.h)
        u._focus = None
        rc, rec = r.call(entry, r.args('p', use_graph=use_graph, nsteps=2))
        assert rc == SL.OK, r.L.vdx_last_error()
        return r.t['img'][:SL.B].clone(), rec
    a, rec = go(torch.tensor([1, 0]), 1)
    assert SL._forwards(rec) == 2 and sum('focus>' in s for _, s in rec) == 2 * (2 + 2 * len(SL.KW['dim_mults']) - 1), rec
    b, rec = go(torch.tensor([0, 1]), 1)
    assert rec == [], rec                                               # a replay: no new capture
    assert not torch.equal(a, b)
    c, _ = go(torch.tensor([0, 1]), 0)
    assert torch.equal(b, c)                                            # ... of the NEW mask: what the eager steps give
    off, rec = go(None, 1)
    assert SL._forwards(rec) == 2 and not any('focus' in s for _, s in rec)      # the setter dropped the graph
    assert not torch.equal(off, b)


# ---- 8. one train step -----------------------------------------------------------------------------------------------------------------
TRAIN_FWD_TOL, TRAIN_GRAD_TOL = 3e-2, 7e-2       # tests/test_gpu_posbias.py::test_one_train_step


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_one_train_step(tmp_path, mode):
    """tests/test_gpu_posbias.py::test_one_train_step with an explicit focus-present mask, against train_ref on the patched forward, at
    that test's bounds (f32: loss 2e-5, update and EMA 2e-2; bf16: PB.l2_loss_bound / PB.adam_first_step_bound at 3e-2 / 7e-2)."""
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.trainer import Trainer
    from video_diffusion_nnx_amd.unet3d import Unet3D
    ukw = dict(dim=16, channels=1, dim_mults=(1, 2))
    cfg = R.UnetConfig(**ukw)
    g = torch.Generator().manual_seed(0)
    batch = torch.rand(2, 1, 4, 8, 8, generator=g)
    mask = torch.tensor([1, 0], dtype=torch.uint8)
    unet = Unet3D(rngs=1, mode=mode, focus_present=True, **ukw)
    gd = GaussianDiffusion(unet, image_size=8, num_frames=4, channels=1, timesteps=50, loss_type='l2')
    tr = Trainer(gd, str(tmp_path / 'r'), dataset_path='synthetic:8', train_batch_size=2, train_num_steps=2, train_lr=1e-3,
                 checkpoint_every_steps=10, results_folder=str(tmp_path / 'res'), step_start_ema=0, update_ema_every=1, ema_decay=0.9)
    p0 = {k: v.detach().cpu().double().clone() for k, v in unet.state_dict().items()}
    loss_dev = tr.train_step(batch, step=0, focus_present_mask=mask)
    torch.cuda.synchronize()
    assert torch.equal(torch.as_tensor(tr.last_focus_mask), mask)
    t = tr.last_t.cpu().long()
    noise = torch.from_numpy(philox_ref.randn(batch.numel(), tr.last_noise_key, 0)).double().reshape(batch.shape)
    preds = []

    def loss_fn(params):
        def fwd(a, b):
            preds.append(FR.unet_forward_focus(params, cfg, a, b, mask))
            return preds[-1]
        ref = DiffusionRef(fwd, image_size=8, num_frames=4, channels=1, timesteps=50, loss_type='l2', dtype=F64)
        return ref.loss(batch.double(), t, noise)
    ref_loss, grads = train_ref.loss_and_grads(p0, loss_fn)
    zeros = {k: torch.zeros_like(v) for k, v in p0.items()}
    p1, _, _ = train_ref.adam_update(p0, grads, zeros, zeros, count=0, lr=train_ref.lr_schedule(0, 1e-3))
    ema1 = train_ref.ema_update(p0, p1, step=0, step_start_ema=0, update_ema_every=1, decay=0.9)
    if mode == 'f32':
        loss_tol = 2e-5 * max(1.0, abs(ref_loss.item()))
        upd_tol = 2e-2
    else:
        loss_tol = PB.l2_loss_bound(ref_loss.item(), preds[-1].detach(), TRAIN_FWD_TOL)
        upd_tol = PB.adam_first_step_bound(grads, TRAIN_GRAD_TOL)
    got = {k: v.detach().cpu().double() for k, v in unet.state_dict().items()}
    ema_got = {n: tr.ema[o:o + int(np.prod(s))].cpu().double().reshape(s) for n, s, o in unet.param_table}

    def dist(a, b, names):
        num = sum(((a[k] - p0[k]) - (b[k] - p0[k])).pow(2).sum() for k in names)
        den = sum((b[k] - p0[k]).pow(2).sum() for k in names)
        return (num / den).sqrt().item()
    d_loss = abs(loss_dev.item() - ref_loss.item())
    d_upd, d_ema = dist(got, p1, list(p0)), dist(ema_got, ema1, list(p0))
    print(f'train step with a focus-present mask, {mode}: loss {d_loss:.3e} (bound {loss_tol:.3e}), update {d_upd:.3e} and EMA {d_ema:.3e} (bound {upd_tol:.3e})')
    assert d_loss < loss_tol
    assert d_upd < upd_tol and d_ema < upd_tol
    # the mask reached the step: the unmasked oracle's loss is elsewhere
    plain = DiffusionRef(lambda a, b: R.unet_forward(p0, cfg, a, b), image_size=8, num_frames=4, channels=1, timesteps=50, loss_type='l2', dtype=F64)
    if mode == 'f32':
        assert abs(plain.loss(batch.double(), t, noise).item() - ref_loss.item()) > 3 * loss_tol


def test_trainer_draws_the_mask_under_its_key(tmp_path):
    from video_diffusion_nnx_amd import train_step as TS
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.trainer import Trainer
    from video_diffusion_nnx_amd.unet3d import Unet3D
    unet = Unet3D(rngs=1, mode='bf16', focus_present=True, dim=16, channels=1, dim_mults=(1, 2))
    gd = GaussianDiffusion(unet, image_size=8, num_frames=4, channels=1, timesteps=50, loss_type='l2')
    tr = Trainer(gd, str(tmp_path / 'r'), dataset_path='synthetic:8', train_batch_size=4, train_num_steps=2, train_lr=1e-3, rng_seed=11,
                 checkpoint_every_steps=10, results_folder=str(tmp_path / 'res'))
    assert tr.prob_focus_present == 0.0 and tr.last_focus_mask is None
    tr.train(prob_focus_present=0.5)
    want = TS.focus_present_draw(4, 0.5, torch.Generator().manual_seed(TS.focus_present_key(11, 0, 1, 0) & 0x7FFFFFFFFFFFFFFF))
    assert torch.equal(torch.as_tensor(tr.last_focus_mask).cpu(), want)
    assert tr.prob_focus_present == 0.5 and tr.step == 2
