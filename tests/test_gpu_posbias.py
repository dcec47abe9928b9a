"""GPU tests of the temporal relative position bias (Unet3D(temporal_pos_bias=True)): the BIAS instantiations of the
generic attention kernels at block level, the bias forms of the backward cores with their deterministic dBias, and the network with the
switch on -- forward, gradients (the embedding's among them), sampling graphs, one train step -- against the fp64 references of
tests/_posbias_ref.py.  Every case asserts through tests/_launch_hook.py which kernel served it."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _launch_hook as LH
import _parity as P
import _posbias_ref as PB
from oracle import philox_ref, train_ref, unet3d_ref as R
from oracle.diffusion_ref import DiffusionRef

DEV = 'cuda'
F64 = torch.float64
EMB = 'time_rel_pos_bias.relative_attention_bias.embedding'


def _rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# ---- block forward -------------------------------------------------------------------------------------------------------------------------
# tolerances of the unbiased block: tests/test_gpu_blocks.py::test_attention TOL (f32, bf16, on the attention branch alone) and the bf16-tensor
# figure of test_attention_bf16_tensors (branch 4e-2); f16: 3 x the emulation of the fp16 rounding points, per sequence (test_gpu_f16_forms.py)
TOL = {'f32': 2e-5, 'bf16': 1.5e-2, 'bf16io': 4e-2}

FWD_CASES = [
    # (B, F, H, W, C, heads), modes, kernel, shape-string parts per mode index
    ((1, 16, 3, 2, 64, 8), ('f32', 'bf16', 'f16', 'bf16io'), 'attention_reg_kernel', '{m}, 4, bias> C64 L16 nseq6'),     # 6 sequences: ragged last workgroup
    ((2, 10, 3, 3, 32, 8), ('f32', 'bf16', 'f16', 'bf16io'), 'attention_reg_kernel', '{m}, 4, bias> C32 L10 nseq18'),    # masked keys
    ((1, 3, 2, 2, 128, 8), ('f32', 'bf16', 'f16', 'bf16io'), 'attention_reg_kernel', '{m}, 8, bias> C128 L3 nseq4'),
    ((1, 16, 2, 2, 512, 8), ('f32', 'bf16', 'f16', 'bf16io'), 'attention_reg_kernel', '{m}, 32, bias> C512 L16 nseq4'),  # f32: C = 512 is still the register kernel
    ((1, 16, 2, 2, 528, 8), ('f32',), 'attention_kernel', '{m}, 16, 16, bias> C528 L16 nseq4'),                          # f32, C > 512: the staged kernel at LP 16
    ((1, 20, 3, 3, 16, 4), ('f32', 'bf16', 'f16', 'bf16io'), 'attention_kernel', '{m}, 32, 1, bias> C16 L20 nseq9'),     # LP 32
    ((1, 40, 2, 2, 64, 8), ('f32', 'bf16', 'f16', 'bf16io'), 'attention_kernel', '{m}, 64, 1, bias> C64 L40 nseq4'),     # LP 64
]
MODE_ID = {'f32': 0, 'bf16': 1, 'f16': 2, 'bf16io': 1}


def _mha(C, heads, g):
    HD = heads * 32
    wqkv = torch.randn(C, 3 * HD, generator=g) / C ** 0.5      # unit-variance q, k, v: content scores of unit variance, like the bias
    bqkv = torch.randn(3 * HD, generator=g) * 0.2
    wo = torch.randn(HD, C, generator=g) / HD ** 0.5
    bo = torch.randn(C, generator=g) * 0.2
    return wqkv, bqkv, wo, bo


def _pack(w, heads, mode):
    from video_diffusion_nnx_amd import ops
    wqkv, bqkv, wo, bo = w
    return (ops.pack_conv_weights(wqkv.to(DEV).contiguous(), mode), bqkv.to(DEV), ops.pack_conv_weights(wo.to(DEV).contiguous(), mode), bo.to(DEV))


def _seq_view(t):
    """[B, F, H, W, C] -> one group per temporal sequence"""
    B, Fr, H, W, C = t.shape
    return [t.permute(0, 2, 3, 1, 4).reshape(B * H * W, Fr * C)]


@pytest.mark.parametrize('case', [(c, m) for c in FWD_CASES for m in c[1]], ids=lambda cm: f'{cm[0][0]}-{cm[1]}')
def test_block_forward(case):
    from video_diffusion_nnx_amd import ops
    (shape, _, kernel, parts), mode = case
    B, Fr, H, W, C, heads = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, Fr, H, W, C, generator=g)
    w = _mha(C, heads, g)
    bias = PB.bias_table(torch.randn(32, heads, generator=g), Fr)       # N(0, 1) per (bucket, head): bias[h, i, j] != bias[h, j, i]
    io16 = mode == 'bf16io'
    op = 'bf16' if io16 else mode
    if io16:
        x = x.bfloat16()
    elif mode == 'f16':
        x = P.f16r(x)                                                    # (the f16 kernels stage x exactly when it is fp16-representable)
    packed = _pack(w, heads, op)
    xd = x.to(DEV)
    with LH.launches() as rec, LH.nan_outputs():
        y = ops.attention_forward_bias(xd, packed, bias.to(DEV), heads, True, op)
        torch.cuda.synchronize()
    LH.assert_launches(rec, [(kernel, [parts.format(m=f'<{MODE_ID[mode]}'), f'io16 {int(io16)}'])], f'{shape} {mode}')
    x64 = x.double()
    args = [t.double() for t in w]
    ref_branch, _ = PB.attention_block_bias(x64, *args, bias.double(), heads, True)
    got_branch = y.double().cpu() - x64
    assert torch.isfinite(got_branch).all()
    if mode == 'f16':
        emu, _ = PB.attention_block_bias(x64, *args, bias.double(), heads, True, emulate=True, operand='f16')
        bound = P.view_bound(emu, ref_branch, _seq_view)
        worst = P.assert_views(got_branch, ref_branch, _seq_view, bound, f'biased attention f16 {shape}')
    else:
        bound = TOL[mode]
        worst = _rel(got_branch, ref_branch)
        print(f'biased attention {shape} {mode}: branch rel {worst:.3e} (bound {bound:.1e})')
        assert worst < bound, (shape, mode, worst)
    # the case proves something only if the bias moves the result by far more than the bound: against the UNBIASED kernel's output
    y0 = ops.attention_forward_bf16(xd, packed, heads, True) if io16 else ops.attention_forward(xd, packed, heads, True, op)
    moved = _rel(y.double().cpu() - y0.double().cpu(), ref_branch) if mode != 'f16' else \
        float(P.view_rels(y.double().cpu() - y0.double().cpu() + ref_branch, ref_branch, _seq_view).min())
    print(f'   the bias moves the branch by {moved:.3e}')
    assert moved > 10 * bound, (shape, mode, moved, bound)
    y2 = ops.attention_forward_bias(xd, packed, bias.to(DEV), heads, True, op)
    assert torch.equal(y, y2)


# ---- block backward ------------------------------------------------------------------------------------------------------------------------
# O, dq|dk|dv: the bounds of the unbiased tests of the same kernels (test_gpu_conv_backward.py::test_attention_core_backward: 1e-5 / 2e-5 for
# the fp32 core, 1.5e-2 for the bf16 MFMA core; test_gpu_backward_forms.py's _io form states the same 1.5e-2 on bf16 tensors).
# dBias: bf16 core: 3 x the distance of the operand-rounded emulation (PB.attn_core_bias(emulate=True)) from fp64 -- the margin of
# _parity.group_bound.  fp32 core: no rounding point, so the emulation IS the reference; the bound is the exact-products kind of
# _parity.f32_group_bounds: max(2e-5 -- what the same kernel's dq|dk|dv are held to --, 8 x the closed form evaluated in fp32 on the CPU).
# Measured (MI355X): see DESIGN.md 8.
BWD_CASES = [
    # B, F, H, W, bf16_operands, io_bf16, kernel
    (1, 16, 3, 3, True, False, 'attn_core_bwd16_bias_kernel'),      # nine sequences: three dead waves in the last group of four
    (1, 16, 3, 3, True, True, 'attn_core_bwd16_bias_kernel'),
    (2, 10, 2, 2, True, False, 'attn_core_bwd16_bias_kernel'),      # masked keys, zero rows
    (2, 10, 2, 2, True, True, 'attn_core_bwd16_bias_kernel'),
    (1, 20, 2, 2, False, False, 'attn_core_bwd_bias_kernel'),       # the generic fp32 core
    (2, 10, 2, 2, False, False, 'attn_core_bwd_bias_kernel'),
    (1, 20, 2, 2, True, False, 'attn_core_bwd_bias_kernel'),        # bf16 mode beyond 16 tokens runs the fp32 core too
]


@pytest.mark.parametrize('case', BWD_CASES, ids=str)
def test_block_backward(case):
    from video_diffusion_nnx_amd import ops
    B, Fr, H, W, bf16_ops, io16, kernel = case
    heads, HD, HW = 8, 256, H * W
    npix = B * Fr * HW
    g = torch.Generator().manual_seed(B + Fr + H + 17)
    qkv = torch.randn(npix, 3 * HD, generator=g)
    d_o = torch.randn(npix, HD, generator=g)
    bias = PB.bias_table(torch.randn(32, heads, generator=g), Fr)
    mfma = bf16_ops and Fr <= 16
    dt = torch.bfloat16 if io16 else torch.float32
    o_ref, g_ref, db_ref = PB.attn_core_bias(qkv, d_o, bias, B, Fr, HW, heads, True)
    if mfma:
        _, _, db_emu = PB.attn_core_bias(qkv, d_o, bias, B, Fr, HW, heads, True, emulate=True, round_out=io16)
        tol_o = tol_g = 1.5e-2
        db_bound = 3.0 * _rel(db_emu, db_ref)
    else:
        _, _, db32 = PB.attn_core_bias(qkv, d_o, bias, B, Fr, HW, heads, True, dtype=torch.float32)
        tol_o, tol_g = 1e-5, 2e-5
        db_bound = max(2e-5, 8.0 * _rel(db32.double(), db_ref))
        assert db_bound < P.EXACT_CEILING
    runs = []
    for _ in range(2):
        with LH.launches() as rec, LH.nan_outputs():
            o, dqkv, dbias = ops.attention_core_backward_bias(qkv.to(DEV, dt), d_o.to(DEV, dt), bias.to(DEV), B, Fr, H, W, heads, True, bf16_operands=bf16_ops)
            torch.cuda.synchronize()
        LH.assert_launches(rec, [(kernel, [f'L{Fr} nseq{B * HW} heads8']), ('attn_dbias_sum_kernel', [f'heads8 L{Fr}'])], str(case))
        runs.append((o, dqkv, dbias))
    o, dqkv, dbias = [t.double().cpu() for t in runs[0]]
    ro, rg, rb = _rel(o, o_ref), _rel(dqkv, g_ref), _rel(dbias, db_ref)
    print(f'[posbias bwd] {case}: o {ro:.3e} (bound {tol_o:.1e}), dqkv {rg:.3e} ({tol_g:.1e}), dBias {rb:.3e} (bound {db_bound:.3e})')
    assert ro < tol_o and rg < tol_g
    for nm, a, b in (('dq', 0, HD), ('dk', HD, 2 * HD), ('dv', 2 * HD, 3 * HD)):
        assert _rel(dqkv[:, a:b], g_ref[:, a:b]) < tol_g, (case, nm)
    assert rb < db_bound, (case, rb, db_bound)
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)                                         # slots + ordered sum: bit-equal run to run
    # the bias reaches the backward: the unbiased core's output is far away
    o0, dq0 = ops.attention_core_backward_io(qkv.to(DEV, dt), d_o.to(DEV, dt), B, Fr, H, W, heads, True, bf16_operands=bf16_ops)
    assert _rel(dq0.double().cpu(), g_ref) > 10 * tol_g and _rel(o0.double().cpu(), o_ref) > 10 * tol_o


# ---- network -------------------------------------------------------------------------------------------------------------------------------
KW = dict(dim=16, channels=1)
TEMPORAL = ['init_temporal_attn'] + [f'downs.{i}.3' for i in range(4)] + ['mid_temporal_attn'] + [f'ups.{i}.3' for i in range(4)]
FWD_TOL = {'f32': 2e-5, 'bf16': 2e-2, 'f16': 4e-3, 'bf16+act16': 3e-2}      # tests/test_gpu_unet.py TOL / TOL_ACT16; f16: test_gpu_configs.py's stated 4e-3
BWD_TOL = {'f32': 2e-4, 'bf16': 6e-2, 'bf16+act16': 7e-2}                   # tests/test_gpu_backward.py


@functools.lru_cache(maxsize=None)
def _net_ref(frames):
    """Shared fp64 reference at B = 2, `frames` frames of 16 x 16: inputs, the patched forward, and (5 frames) all gradients."""
    cfg = R.UnetConfig(**KW)
    p64 = R.random_params(cfg, seed=7, dtype=F64)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 1, frames, 16, 16, generator=g)
    t = torch.randint(0, 1000, (2,), generator=g)
    d_out = torch.randn(2, frames, 16, 16, 1, generator=g)
    leaves = {k: v.clone().requires_grad_(True) for k, v in p64.items()}
    out = PB.unet_forward_pos(leaves, cfg, x.double(), t)
    grads = None
    if frames == 5:
        gr = torch.autograd.grad(out, list(leaves.values()), d_out.double(), allow_unused=True)
        grads = {k: (torch.zeros_like(v) if q is None else q) for (k, v), q in zip(leaves.items(), gr)}
    return cfg, p64, x, t, d_out, out.detach(), grads


def _model(mode, p64=None, on=True, rngs=0):
    from video_diffusion_nnx_amd.unet3d import Unet3D
    m = Unet3D(rngs=rngs, mode=mode.split('+')[0], temporal_pos_bias=on, **KW)
    if p64 is not None:
        m.load_state_dict({k: v.float() for k, v in p64.items()})
    return m


def _attn_launches(rec):
    return [(k, s) for k, s in rec if k.startswith('attention') or k.startswith('attn_') or k.startswith('pos_bias')]


@pytest.mark.parametrize('mode,frames', [('f32', 5), ('bf16', 5), ('f16', 5), ('bf16+act16', 5), ('bf16', 10)])
def test_network_forward(mode, frames):
    cfg, p64, x, t, _, ref, _ = _net_ref(frames)
    m = _model(mode, p64)
    m.act_bf16 = mode.endswith('+act16')
    with LH.launches() as rec:
        y = m(x, t)
        torch.cuda.synchronize()
    r = _rel(y.cpu().double(), ref)
    print(f'network forward with the position bias, {mode}, {frames} frames: rel {r:.3e} (bound {FWD_TOL[mode]:.1e})')
    assert r < FWD_TOL[mode]
    # the unbiased network is elsewhere: a forward that ignored the bias would miss the bound (random_params' embedding, std 1 / sqrt(8))
    assert _rel(y.cpu().double(), R.unet_forward(p64, cfg, x.double(), t)) > 3 * FWD_TOL[mode]
    att = _attn_launches(rec)
    assert att[0][0] == 'pos_bias_table_kernel' and f'heads8 n{frames}' in att[0][1]
    biased = [(k, s) for k, s in att[1:] if 'bias' in s]
    assert len(biased) == 10 and all(k == 'attention_reg_kernel' and f'L{frames} ' in s for k, s in biased), att
    plain = [(k, s) for k, s in att[1:] if 'bias' not in s]
    assert len(plain) == 1 and 'L4 ' in plain[0][1], att                   # the mid spatial block (2 x 2 pixels): no bias
    m.temporal_pos_bias = False
    with LH.launches() as rec0:
        m(x, t)
    assert _attn_launches(rec0)[5] == plain[0]                             # ... and it reports what it reports with the switch off


# the attention launches of Unet3D(dim=16, channels=1) at B = 2, 5 frames of 16 x 16 with the switch off, recorded on the parent commit
PARENT_ATTN = {
    'f32': [
        ('attention_reg_kernel', '<0, 4, fp8 0> C16 L5 nseq512 io16 0'),
        ('attention_reg_kernel', '<0, 4, fp8 0> C16 L5 nseq512 io16 0'),
        ('attention_reg_kernel', '<0, 4, fp8 0> C32 L5 nseq128 io16 0'),
        ('attention_h8_kernel', '<0, 2, 1, 2, 0, 0, 0> C64 L5 nseq32'),
        ('attention_reg_kernel', '<0, 8, fp8 0> C128 L5 nseq8 io16 0'),
        ('attention_reg_kernel', '<0, 8, fp8 0> C128 L4 nseq10 io16 0'),
        ('attention_reg_kernel', '<0, 8, fp8 0> C128 L5 nseq8 io16 0'),
        ('attention_h8_kernel', '<0, 2, 1, 2, 0, 0, 0> C64 L5 nseq8'),
        ('attention_reg_kernel', '<0, 4, fp8 0> C32 L5 nseq32 io16 0'),
        ('attention_reg_kernel', '<0, 4, fp8 0> C16 L5 nseq128 io16 0'),
        ('attention_reg_kernel', '<0, 4, fp8 0> C16 L5 nseq512 io16 0'),
    ],
    'bf16': [
        ('attention_reg_kernel', '<1, 4, fp8 0> C16 L5 nseq512 io16 0'),
        ('attention_reg_kernel', '<1, 4, fp8 0> C16 L5 nseq512 io16 0'),
        ('attention_reg_kernel', '<1, 4, fp8 0> C32 L5 nseq128 io16 0'),
        ('attention_h8_kernel', '<1, 1, 1, 2, 0, 0, 0> C64 L5 nseq32'),
        ('attention_h8_kernel', '<1, 2, 1, 4, 0, 0, 0> C128 L5 nseq8'),
        ('attention_reg_kernel', '<1, 8, fp8 0> C128 L4 nseq10 io16 0'),
        ('attention_h8_kernel', '<1, 2, 1, 4, 0, 0, 0> C128 L5 nseq8'),
        ('attention_h8_kernel', '<1, 1, 1, 2, 0, 0, 0> C64 L5 nseq8'),
        ('attention_reg_kernel', '<1, 4, fp8 0> C32 L5 nseq32 io16 0'),
        ('attention_reg_kernel', '<1, 4, fp8 0> C16 L5 nseq128 io16 0'),
        ('attention_reg_kernel', '<1, 4, fp8 0> C16 L5 nseq512 io16 0'),
    ],
}


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_switch_off_launches_what_the_parent_launched(mode):
    cfg, p64, x, t, _, _, _ = _net_ref(5)
    m = _model(mode, p64, on=False)
    with LH.launches() as rec:
        y = m(x, t)
        torch.cuda.synchronize()
    att = _attn_launches(rec)
    assert att == [tuple(e) for e in PARENT_ATTN[mode]], att
    assert not any('bias' in s for _, s in att)
    assert _rel(y.cpu().double(), R.unet_forward(p64, cfg, x.double(), t)) < FWD_TOL[mode]


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


@pytest.mark.parametrize('mode', ['f32', 'bf16', 'bf16+act16'])
def test_network_gradients(mode):
    cfg, p64, x, t, d_out, _, ref_grads = _net_ref(5)
    tol = BWD_TOL[mode]
    m = _model(mode, p64)
    m.act_bf16 = 2 if mode.endswith('+act16') else False
    m(x, t)
    with LH.launches() as rec:
        grads = _backward(m, d_out.to(DEV), staged=True)
    names = [k for k, _ in rec]
    core = 'attn_core_bwd_bias_kernel' if mode == 'f32' else 'attn_core_bwd16_bias_kernel'
    assert names.count(core) == 10 and names.count('attn_dbias_sum_kernel') == 10 and names.count('pos_bias_scatter_kernel') == 1
    assert 'attn_bwd16x_kernel' not in names
    got = {n: grads[o:o + int(np.prod(s))].cpu().double().reshape(s) for n, s, o in m.param_table}
    total_ref = torch.cat([ref_grads[n].reshape(-1) for n, _, _ in m.param_table])
    total_got = torch.cat([got[n].reshape(-1) for n, _, _ in m.param_table])
    scale = total_ref.norm().item()
    bad = [(n, _rel(got[n], ref_grads[n])) for n, _, _ in m.param_table if ref_grads[n].norm() > 1e-6 * scale and _rel(got[n], ref_grads[n]) > 5 * tol]
    assert not bad, sorted(bad, key=lambda z: -z[1])[:6]
    rt = _rel(total_got, total_ref)
    re = _rel(got[EMB], ref_grads[EMB])
    print(f'network gradients with the position bias, {mode}: all {rt:.3e}, embedding {re:.3e} (|ref| {ref_grads[EMB].norm().item():.3e}; bound {tol:.1e})')
    assert rt < tol
    assert ref_grads[EMB].norm().item() > 1e-6 * scale and got[EMB].norm().item() > 0         # today's exact zero is gone
    assert re < tol, re
    # bit-equal over two runs, staged == unstaged
    g2 = _backward(m, d_out.to(DEV), staged=False)
    g3 = _backward(m, d_out.to(DEV), staged=False)
    assert torch.equal(grads, g2) and torch.equal(g2, g3)


def test_zero_embedding_is_the_unbiased_network_and_order_matters():
    cfg, p64, x, t, _, _, _ = _net_ref(5)
    tol = FWD_TOL['f32']
    perm = torch.tensor([3, 0, 4, 1, 2])
    m = _model('f32', p64)
    # switch off: equivariant under a permutation of the frames (within the f32 tolerance); switch on: not
    m.temporal_pos_bias = False
    y_off = m(x, t).clone()
    assert _rel(m(x[:, :, perm].contiguous(), t), y_off[:, perm]) < tol
    m.temporal_pos_bias = True
    y_on = m(x, t).clone()
    broken = _rel(m(x[:, :, perm].contiguous(), t), y_on[:, perm])
    print(f'frame permutation with the position bias on the GPU: {broken:.3e}')
    assert broken > 1e-3
    # a zero embedding: the biased kernels compute the unbiased network (other kernels: within tolerance, not bit-equal)
    z = dict(p64)
    z[EMB] = torch.zeros_like(p64[EMB])
    m.load_state_dict({k: v.float() for k, v in z.items()})
    y_zero = m(x, t).clone()
    m.temporal_pos_bias = False
    assert _rel(y_zero, m(x, t)) < tol


def test_toggling_graphs_and_samplers():
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.unet3d import Unet3D
    cfg, p64, x, t, _, _, _ = _net_ref(5)
    m = _model('bf16', p64, on=False)
    a = m(x, t).clone()
    m.temporal_pos_bias = True
    b = m(x, t).clone()
    m.temporal_pos_bias = False
    c = m(x, t).clone()
    assert torch.equal(a, c) and not torch.equal(a, b)
    gd = GaussianDiffusion(m, image_size=16, num_frames=5, channels=1, timesteps=4)
    s_off = gd.p_sample_loop((2,), key=5).clone()
    m.temporal_pos_bias = True
    s_on = gd.p_sample_loop((2,), key=5).clone()
    s_eager = gd.p_sample_loop((2,), key=5, use_graph=False).clone()
    m.temporal_pos_bias = False
    s_off2 = gd.p_sample_loop((2,), key=5).clone()
    torch.cuda.synchronize()
    assert torch.equal(s_off, s_off2) and not torch.equal(s_off, s_on)       # the graph cache sees the switch
    assert torch.equal(s_on, s_eager)                                         # graph == eager with the switch on
    m.temporal_pos_bias = True
    assert torch.isfinite(gd.ddim_sample_loop((2,), key=5, steps=1)).all()
    assert torch.isfinite(gd.dpm_sample_loop((2,), key=5, steps=1)).all()
    # fp8 attention and the switch exclude each other
    with pytest.raises(ValueError):
        Unet3D(rngs=0, mode='bf16', attn_fp8=True, temporal_pos_bias=True, **KW)
    m.attn_fp8 = True
    with pytest.raises(ValueError):
        m(x, t)
    m.attn_fp8 = False


# One train step against oracle/train_ref.py on the patched forward.  f32: the bounds of tests/test_gpu_train.py (loss 2e-5, update and EMA 2e-2).
# bf16 (operands + the training forward's bf16 storage): that file states no bf16 figure and its f32 ones are below bf16's resolution, so the
# bounds follow from the tolerances the suite already holds this mode to -- forward 3e-2 (test_gpu_unet.TOL_ACT16), all gradients 7e-2
# (test_gpu_backward, 'bf16+act16') -- through PB.l2_loss_bound and PB.adam_first_step_bound (the sign flips to expect of a gradient that just meets
# its tolerance; computed from the fp64 reference alone), for all parameters and for the embedding on its own.  Measured figures: DESIGN.md 8.
TRAIN_FWD_TOL, TRAIN_GRAD_TOL = 3e-2, 7e-2


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_one_train_step(tmp_path, mode):
    """tests/test_gpu_train.py::test_one_train_step_matches_oracle with the switch on, against train_ref on the patched forward."""
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.trainer import Trainer
    from video_diffusion_nnx_amd.unet3d import Unet3D
    ukw = dict(dim=16, channels=1, dim_mults=(1, 2))
    cfg = R.UnetConfig(**ukw)
    g = torch.Generator().manual_seed(0)
    batch = torch.rand(2, 1, 4, 8, 8, generator=g)
    ends = []
    for run in range(2):
        unet = Unet3D(rngs=1, mode=mode, temporal_pos_bias=True, **ukw)
        gd = GaussianDiffusion(unet, image_size=8, num_frames=4, channels=1, timesteps=50, loss_type='l2')
        tr = Trainer(gd, str(tmp_path / f'r{run}'), dataset_path='synthetic:8', train_batch_size=2, train_num_steps=3, train_lr=1e-3,
                     checkpoint_every_steps=2, results_folder=str(tmp_path / f'res{run}'), step_start_ema=0, update_ema_every=1, ema_decay=0.9)
        p0 = {k: v.detach().cpu().double().clone() for k, v in unet.state_dict().items()}
        loss_dev = tr.train_step(batch, step=0)
        torch.cuda.synchronize()
        ends.append((loss_dev.item(), unet.flat_params.clone(), tr.ema.clone()))
    assert ends[0][0] == ends[1][0] and torch.equal(ends[0][1], ends[1][1]) and torch.equal(ends[0][2], ends[1][2])
    t = tr.last_t.cpu().long()
    noise = torch.from_numpy(philox_ref.randn(batch.numel(), tr.last_noise_key, 0)).double().reshape(batch.shape)
    preds = []

    def loss_fn(params):
        def fwd(a, b):
            preds.append(PB.unet_forward_pos(params, cfg, a, b))
            return preds[-1]
        ref = DiffusionRef(fwd, image_size=8, num_frames=4, channels=1, timesteps=50, loss_type='l2', dtype=F64)
        return ref.loss(batch.double(), t, noise)
    ref_loss, grads = train_ref.loss_and_grads(p0, loss_fn)
    assert grads[EMB].abs().max() > 0
    zeros = {k: torch.zeros_like(v) for k, v in p0.items()}
    p1, _, _ = train_ref.adam_update(p0, grads, zeros, zeros, count=0, lr=train_ref.lr_schedule(0, 1e-3))
    ema1 = train_ref.ema_update(p0, p1, step=0, step_start_ema=0, update_ema_every=1, decay=0.9)
    if mode == 'f32':
        loss_tol = 2e-5 * max(1.0, abs(ref_loss.item()))
        upd_tol = emb_tol = 2e-2
    else:
        loss_tol = PB.l2_loss_bound(ref_loss.item(), preds[-1].detach(), TRAIN_FWD_TOL)
        upd_tol = PB.adam_first_step_bound(grads, TRAIN_GRAD_TOL)
        emb_tol = PB.adam_first_step_bound({EMB: grads[EMB]}, TRAIN_GRAD_TOL)
    got = {k: v.detach().cpu().double() for k, v in unet.state_dict().items()}
    ema_got = {n: tr.ema[o:o + int(np.prod(s))].cpu().double().reshape(s) for n, s, o in unet.param_table}

    def dist(a, b, names):                                                    # (test_gpu_train.py: the UPDATE, tolerating sign flips of ~zero gradients)
        num = sum(((a[k] - p0[k]) - (b[k] - p0[k])).pow(2).sum() for k in names)
        den = sum((b[k] - p0[k]).pow(2).sum() for k in names)
        return (num / den).sqrt().item()
    d_loss = abs(loss_dev.item() - ref_loss.item())
    d_upd, d_ema, d_emb = dist(got, p1, list(p0)), dist(ema_got, ema1, list(p0)), dist(got, p1, [EMB])
    print(f'train step with the position bias, {mode}: loss {d_loss:.3e} (bound {loss_tol:.3e}), update {d_upd:.3e} and EMA {d_ema:.3e} '
          f'(bound {upd_tol:.3e}), the embedding\'s update {d_emb:.3e} (bound {emb_tol:.3e})')
    assert d_loss < loss_tol
    assert d_upd < upd_tol and d_ema < upd_tol
    assert d_emb < emb_tol
    assert tr.opt_count == 1
    moved = (unet.get_param(EMB).cpu().double() - p0[EMB]).abs().max().item()
    assert moved > 0                                                          # the embedding trains
