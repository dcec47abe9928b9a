"""Block-level parity of the forward forms that only vdx_unet_forward reaches: the per-head attention / SLA kernels of the wide levels
with their 1x1 out-projection, the long attention core between two 1x1 convs, the tails on bf16 tensors (all-bf16, mixed, with the
head inside), the final conv on bf16 input, the MFMA init conv and bf16 init-conv output, the scale/shift pass -- through the
test-facing entry points of include/vdx.h ("Forward forms of the network").

Every input is made bf16-representable on the host where the kernel's contract says so, so input rounding is not part of any error.
References are fp64 through oracle/unet3d_ref.py (the per-head kernels: the fp64 closed forms of tests/_parity.py, which
tests/test_host_parity_helpers.py pins to the oracle).  Cases, references and bounds are built in tests/_forward_cases.py from the
reference side alone; every bound is printed next to the measured value (run with -s).  Outputs are NaN-filled before each call (an
unwritten row shows), every case runs twice and the two runs must be bit-identical.  tests/test_host_parity_helpers.py shows on the
CPU that a neighbouring head's output, unmasked padding keys, an unwritten pixel pass, a consumer reading slot 0 only and a
scale/shift row of the wrong sample are rejected at these bounds."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _forward_cases as FC
import _parity as P
import _parity_routes as PR
from _launch_hook import assert_launches, launches
from oracle import unet3d_ref as R

DEV = 'cuda:0'
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16


def _dev(t, dtype=F32):
    return None if t is None else t.detach().to(dtype).to(DEV).contiguous()


def _twice(fn):
    """Run fn twice (fresh NaN-filled outputs each time); the two runs must be bit-identical.  -> outputs of the first run, on the CPU"""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    a = [t.cpu() for t in (a if isinstance(a, (tuple, list)) else (a,))]
    b = [t.cpu() for t in (b if isinstance(b, (tuple, list)) else (b,))]
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.uint8), v.view(torch.uint8)), 'two runs are not bit-identical'
    return a


def _finite(t, what):
    assert torch.isfinite(t.float()).all(), f'{what}: non-finite output (a row the kernel did not write?)'


# ---- attention heads --------------------------------------------------------------------------------------------------------------------

_HEADS = ([(s, True, io16, False) for s in FC.ATTN_HEADS_TEMPORAL for io16 in (False, True)] +
          [(FC.ATTN_HEADS_TEMPORAL[0], True, io16, True) for io16 in (False, True)] +
          [(s, False, io16, False) for s in FC.ATTN_HEADS_SPATIAL for io16 in (False, True)] +
          # the fp8 flag on 64 tokens, as the fp8 network sets it on mid_spatial_attn: launch_attention_head reports "fp8 1, lt 4" and runs
          # the bf16 core (sequences of more than 16 tokens ignore the flag) -- the output must be that of the unflagged call, bit for bit
          [(FC.ATTN_HEADS_SPATIAL[0], False, True, True)])


def _run_heads(c, temporal, io16, fp8):
    from video_diffusion_nnx_amd import ops
    wqkv, bqkv, wo, bo = c['w']
    packed = (ops.pack_conv_weights(_dev(wqkv), 'bf16'), _dev(bqkv), ops.pack_conv_weights(_dev(wo), 'bf16'), _dev(bo))
    x = _dev(c['x'], BF if io16 else F32)
    return _twice(lambda: ops.attention_heads_forward(x, packed, temporal, fp8_core=fp8))


@pytest.mark.parametrize('shape,temporal,io16,fp8', _HEADS)
def test_attention_heads(shape, temporal, io16, fp8):
    """attention_head_kernel<IO16, 4, F8, LT = 1 | 4> + the 1x1 out-projection with residual (model.hip attention_block_forward)."""
    core8 = fp8 and (shape[1] if temporal else shape[2] * shape[3]) <= 16       # the e4m3 core exists for sequences of at most 16 tokens
    c = FC.attn_heads_case(shape, temporal, io16, core8)
    with PR.bound(PR.cid('heads', shape, temporal, io16, fp8)):
        y, o = _run_heads(c, temporal, io16, fp8)
    what = f'attention heads {shape} temporal={int(temporal)} io16={int(io16)} fp8={int(fp8)}'
    _finite(o, what + ' o'); _finite(y, what + ' y')
    assert y.dtype == (BF if io16 else F32) and o.dtype == BF
    P.assert_groups(c['og'](o.double()), c['og'](c['o64']), (c['nseq'], 8), c['bound_o'], what + ' o per (sequence, head)')
    P.assert_groups(FC.seq_groups(y.double(), temporal), FC.seq_groups(c['y64'], temporal), (c['nseq'],), c['bound_y'], what + ' y per sequence')
    if fp8 and not core8:
        y0, o0 = _run_heads(c, temporal, io16, False)
        assert torch.equal(o.view(torch.uint8), o0.view(torch.uint8)) and torch.equal(y.view(torch.uint8), y0.view(torch.uint8)), f'{what}: the flag changed the output'
    if core8:
        # the fp8 core must actually run: its error sits well above the bf16 operands' (the check the fp8 tests of test_gpu_blocks.py use)
        c16 = FC.attn_heads_case(shape, temporal, io16, False)
        _, o16 = _run_heads(c16, temporal, io16, False)
        r8, r16 = P.rel(o, c['o64']), P.rel(o16, c['o64'])
        print(f'[{what}] o rel {r8:.3e} against {r16:.3e} with bf16 operands')
        assert r8 > 1.5 * r16
        # and the project's stated figure for the fp8 core on the attention branch as a whole (tests/test_gpu_blocks.py)
        xd = c['x'].double()
        rb = P.rel(y.double() - xd, c['y64'] - xd)
        print(f'[{what}] attention branch rel {rb:.3e} (stated 1e-1)')
        assert rb < 1e-1


def test_attention_heads_rejects_what_the_network_routes_elsewhere():
    from video_diffusion_nnx_amd import ops
    from video_diffusion_nnx_amd._lib import VdxError
    g = torch.Generator().manual_seed(1)
    for shape, temporal in (((1, 4, 2, 2, 128), True), ((1, 17, 2, 2, 256), True), ((1, 1, 9, 9, 256), False), ((1, 4, 2, 2, 320), True)):
        C = shape[-1]
        wqkv, bqkv, wo, bo = FC.mha_weights(C, g)
        packed = (ops.pack_conv_weights(_dev(wqkv), 'bf16'), _dev(bqkv), ops.pack_conv_weights(_dev(wo), 'bf16'), _dev(bo))
        with pytest.raises(VdxError):
            ops.attention_heads_forward(torch.zeros(shape, device=DEV), packed, temporal)


# ---- long attention core ------------------------------------------------------------------------------------------------------------------

LONG_MODES = [('f32', False), ('bf16', False), ('bf16', True), ('f16', False)]


@pytest.mark.parametrize('mode,io16', LONG_MODES)
@pytest.mark.parametrize('shape', FC.ATTN_LONG)
def test_attention_long(shape, mode, io16):
    """1x1 q|k|v conv -> attention_long_core_kernel -> 1x1 out-projection + residual (more than 64 tokens).  Each stage is judged on
    the input the stage before it produced (the REFERENCE of the core is the fp64 softmax of the kernel's qkv, that of the out-projection
    the fp64 product of the kernel's o: producer and consumer are judged separately), while every BOUND comes from the reference chain
    of tests/_forward_cases.py: the convs under the exact-products contract, the fp32 core at 8 x the same softmax evaluated in fp32."""
    from video_diffusion_nnx_amd import ops
    c = FC.attn_long_case(shape)
    wqkv, bqkv, wo, bo = c['w']
    packed = (ops.pack_conv_weights(_dev(wqkv), mode), _dev(bqkv), ops.pack_conv_weights(_dev(wo), mode), _dev(bo))
    x = _dev(c['x'], BF if io16 else F32)
    what = f'long attention {shape} {mode} io16={int(io16)}'
    with launches() as rec:                     # (ops.attention_long_forward NaN-fills y and the scratch itself)
        y, qkv, o = _twice(lambda: ops.attention_long_forward(x, packed, 8, mode))
    PR.assert_first(PR.cid('long', shape, mode, io16), rec)
    if mode == 'f16':           # both projections on the fp16 form of the generic conv (x and the weights here are fp16 numbers as well)
        assert_launches(rec[:3], [('conv_igemm_kernel', ['<2, 128, 2, 8, 0>', 'conv1x1 128->768']), ('attention_long_core_kernel', [f"L{c['L']}"]),
                                  ('conv_igemm_kernel', ['<2, 128, 2, 8, 0>', 'conv1x1 256->128', '+res'])], what)
        assert rec[3:] == rec[:3]
    for t, n in ((qkv, 'qkv'), (o, 'o'), (y, 'y')):
        _finite(t, f'{what} {n}')
    P.assert_exact_products(qkv, c['qkv64'], c['b_qkv'], c['seq_sl'], c['sb_qkv'], None, what + ' qkv')
    # the core, per (sequence, head): reference = the same softmax in fp64 of the qkv the kernel read; bound from the reference's qkv
    nseq, L, hg = c['nseq'], c['L'], c['hg']
    P.assert_groups(hg(o), hg(FC.long_core(qkv, nseq, L, F64)), (nseq * 8,), c['b_core'], what + ' o per (sequence, head)')
    # the out-projection: reference = the o it read (bf16 mode: rounded to bf16 at staging) . Wo + bias + residual in fp64
    oin = P.bf16r(o) if mode == 'bf16' else P.f16r(o) if mode == 'f16' else o
    y64 = (oin.double() @ wo.double() + bo.double()).reshape(c['x'].shape) + c['x'].double()
    b_y, sb_y = c['b_out'][mode]
    if io16:
        P.assert_bf16_store(y, y64, P.FWD_STATED, what + ' y')
    else:
        P.assert_exact_products(y, y64, b_y, c['y_sl'], sb_y, None, what + ' y')
    # and the chain as a whole against the oracle's block, at the figures tests/test_gpu_blocks.py states for the short kernels
    branch = P.rel(y.double() - c['x'].double(), c['y64'] - c['x'].double())
    tol = 2e-5 if mode == 'f32' else (4e-2 if io16 else 1.5e-2)
    print(f'[{what}] attention branch against the oracle: rel {branch:.3e} (stated {tol:.1e})')
    assert branch < tol


def test_attention_long_rejects_short_sequences():
    from video_diffusion_nnx_amd import ops
    from video_diffusion_nnx_amd._lib import VdxError
    wqkv, bqkv, wo, bo = FC.mha_weights(128, torch.Generator().manual_seed(2))
    packed = (ops.pack_conv_weights(_dev(wqkv), 'f32'), _dev(bqkv), ops.pack_conv_weights(_dev(wo), 'f32'), _dev(bo))
    with pytest.raises(VdxError):
        ops.attention_long_forward(torch.zeros(1, 2, 8, 8, 128, device=DEV), packed, 8, 'f32')


# ---- SLA heads ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('io16', [False, True])
@pytest.mark.parametrize('shape', FC.SLA_HEADS)
def test_sla_heads(shape, io16):
    """sla_head_kernel<IO16, 4 | 1> + the 1x1 to_out with residual (model.hip sla_block_forward)."""
    from video_diffusion_nnx_amd import ops
    c = FC.sla_heads_case(shape, io16)
    x = _dev(c['x'], BF if io16 else F32)
    w = [_dev(t.reshape(1, *t.shape)) for t in c['w']]
    with PR.bound(PR.cid('sla heads', shape, io16)):
        y, o = _twice(lambda: ops.sla_heads_forward(x, *w))
    what = f'sla heads {shape} io16={int(io16)}'
    _finite(o, what + ' o'); _finite(y, what + ' y')
    P.assert_groups(c['og'](o.double()), c['og'](c['o64']), (c['NF'], 8), c['bound_o'], what + ' o per (frame, head)')
    P.assert_groups(y.double().reshape(c['NF'], -1), c['y64'].reshape(c['NF'], -1), (c['NF'],), c['bound_y'], what + ' y per frame')


def test_sla_heads_rejects_what_the_network_routes_elsewhere():
    from video_diffusion_nnx_amd import ops
    from video_diffusion_nnx_amd._lib import VdxError
    for shape in ((1, 2, 4, 4, 128), (1, 2, 3, 5, 256)):              # narrow level; N % 16 != 0
        C = shape[-1]
        w = [torch.zeros(1, C, 256, device=DEV)] * 3 + [torch.zeros(1, 256, C, device=DEV)]
        with pytest.raises(VdxError):
            ops.sla_heads_forward(torch.zeros(shape, device=DEV), *w)


# ---- tails -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C,B,shape', FC.TAIL16)
def test_resblock_tail_all_bf16(C, B, shape):
    """resblock_tail16_kernel<1 | 2>: y2, r and out bf16, r read from memory; statistics spread over several slots."""
    from video_diffusion_nnx_amd import ops
    c = FC.tail_case(C, B, shape, True)
    args = [_dev(c['y2'], BF), _dev(c['r'], BF), c['slab'].reshape(-1).to(DEV)] + [_dev(t) for t in c['par']]
    (out,) = _twice(lambda: ops.resblock_tail_ex(*args, out_bf16=True))
    assert out.dtype == BF
    P.assert_bf16_store(out, c['ref64'], c['store_floor'], f'tail16 C{C} B{B} {shape}')


@pytest.mark.parametrize('C,B,shape', FC.TAIL_MIXED)
def test_resblock_tail_bf16_y2_fp32_r_out(C, B, shape):
    """resblock_tail_kernel with y2_bf16 and fp32 r / out: the training forward of a bf16-mode handle."""
    from video_diffusion_nnx_amd import ops
    c = FC.tail_case(C, B, shape, False)
    args = [_dev(c['y2'], BF), _dev(c['r']), c['slab'].reshape(-1).to(DEV)] + [_dev(t) for t in c['par']]
    (out,) = _twice(lambda: ops.resblock_tail_ex(*args, out_bf16=False))
    assert out.dtype == F32
    P.assert_exact_products(out, c['ref64'], c['bound'], c['sl'], c['sb'], None, f'tail y2 bf16 / fp32 C{C} B{B} {shape}')


@pytest.mark.parametrize('c0,c1,C,B,shape', FC.TAIL_HEAD)
def test_resblock_tail_with_head(c0, c1, C, B, shape):
    """The FIN form of resblock_tail_rc16_kernel: res_conv, tail and the one-channel final conv in one kernel, fp32 output."""
    from video_diffusion_nnx_amd import ops
    c = FC.tail_head_case(c0, c1, C, B, shape)
    args = [_dev(c['y2'], BF), _dev(c['x0'], BF), _dev(c['x1'], BF), _dev(c['w']), _dev(c['rb']), c['slab'].reshape(-1).to(DEV)] + \
           [_dev(t) for t in c['par']] + [_dev(c['fw']), _dev(c['fb'])]
    (out,) = _twice(lambda: ops.resblock_tail_rc_head_bf16(*args))
    P.assert_exact_products(out, c['ref64'], c['bound'], c['sl'], c['sb'], None, f'tail with head {c0}+{c1}->{C} B{B} {shape}')


# ---- final conv on bf16 input, init conv -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('D,Cout,npix', FC.FINAL16)
def test_final_conv_bf16_input(D, Cout, npix):
    """final_conv16_kernel<Cout> (D in {16, 32, 64, 128}) and final_conv_kernel with bf16 input (D = 24)."""
    from video_diffusion_nnx_amd import ops
    c = FC.final_case(D, Cout, npix)
    x, k, b = _dev(c['x'], BF), _dev(c['kern']), _dev(c['bias'])
    (y,) = _twice(lambda: ops.final_conv_ex(x, k, b))
    P.assert_exact_products(y, c['ref64'], c['bound'], c['sl'], c['sb'], None, f'final conv bf16 x D{D}->{Cout} px{npix}')


# (init_conv_kernel with fp32 y is what vdx_init_conv runs: tests/test_gpu_blocks.py::test_init_conv)
@pytest.mark.parametrize('Cin,K,Cout,y16', [(*c, y16) for c in FC.INIT for y16 in (False, True) if c[0] == 1 or y16])
def test_init_conv_bf16_mode(Cin, K, Cout, y16):
    """init_conv_mfma_kernel (bf16 mode, one input channel) with fp32 and bf16 y; init_conv_kernel (three channels) with bf16 y."""
    from video_diffusion_nnx_amd import ops
    c = FC.init_case(Cin, K, Cout)
    x, k, b = _dev(c['x']), _dev(c['kern']), _dev(c['bias'])
    (y,) = _twice(lambda: ops.init_conv_ex(x, k, b, 'bf16', y_bf16=y16))
    what = f'init conv bf16 mode {Cin}->{Cout} k{K} y16={int(y16)}'
    if y16:
        assert y.dtype == BF
        P.assert_bf16_store(y, c['ref64'], P.FWD_STATED, what)
    else:
        P.assert_exact_products(y, c['ref64'], c['bound'], c['sl'], c['sb'], None, what)


# ---- scale / shift ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('B', [1, 8, 9, 19])
@pytest.mark.parametrize('temb_dim', [96, 1024])
def test_resblock_scale_shift(temb_dim, B):
    """resblock_ss_lin_kernel + resblock_ss_norm_kernel: layers of 64, 128 and 2048 columns in one table, second and third groups of 8
    samples, the last one ragged.  Both the Linear (what the backward reads) and its LayerNorm, per (layer, sample)."""
    from video_diffusion_nnx_amd import ops
    c = FC.ss_case(temb_dim, B)
    params, temb = _dev(c['params']), _dev(c['temb'])
    ss, lin = _twice(lambda: ops.resblock_scale_shift(params, temb, c['layers']))
    for i, l in enumerate(c['layers']):
        for name, flat, ref, (bound, sb, _) in (('lin', lin, c['lin64'][i], c['b_lin'][i]), ('ss', ss, c['ss64'][i], c['b_ss'][i])):
            got = FC.ss_rows(flat, c['layers'], B)[i]
            P.assert_exact_products(got, ref, bound, c['sl'], sb, None, f'scale/shift temb{temb_dim} B{B} n{l["n"]} {name}')
