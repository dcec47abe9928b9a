"""Per-group parity of the kernel instantiations that only fp16 operand mode (mode='f16', VDX_MODE_F16) reaches.

The one-wave-per-head and persistent kernels hard-code the bf16 / f32 register formats, so fp16 mode runs attention_reg_kernel<2, TMA, false>
for every sequence of at most 16 tokens, attention_kernel<2, LP, TMO> for 17..64 tokens, the generic sla_ctx_kernel<2> -> sla_combine_kernel<2>
-> sla_out_kernel<2, TMO> for every channel count, and conv_igemm_kernel<2, .., 0> for every conv, forward and data gradient.  The shapes
that the other modes share are f16 entries of tests/test_gpu_attention_groups.py (ATTN32, SLA32), tests/test_gpu_forward_forms.py (long
attention) and tests/test_gpu_backward_forms.py (row-sliced data gradient); this file holds what fp16 mode alone needs.

Attention / SLA: inputs fp16-representable, the fp64 reference of the branch y - x, per-group bounds 3 x the worst group of the fp64
emulation of the fp16 rounding points, AND closeness to that emulation within a small multiple of its own fp32-vs-fp64 distance -- the
check that can see a rounding of the wrong type (tests/_attention_cases.py, tests/_parity.py; tests/test_host_parity_helpers.py proves
both on the CPU).  Convs: the exact-products contract per (frame, 16 x 16 tile), no global figure.  Every case runs twice on NaN-filled
outputs (0xFF-filled workspaces), bit-identical, and asserts the kernel and shape string the launch hook reports."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _attention_cases as AC
import _forward_cases as FC
import _parity as P
from _launch_hook import assert_launches, launches, nan_outputs
from oracle import unet3d_ref as R
from test_gpu_attention_groups import _check, _dev, _nan_like, _run_attention, _run_sla, _sla32
import _parity_routes as PR
from test_gpu_conv import CASES as FWD_CASES, _conv_chain, _conv_form
from test_gpu_conv_backward import CASES as BWD_CASES

DEV = 'cuda:0'
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
IGEMM = 'conv_igemm_kernel'


# ---- attention (vdx_attention_forward_ex, mode f16) ---------------------------------------------------------------------------------------
# attention_reg "<MODE, TMA, fp8>": TMA = 4 / 8 / 16 / 32 / 64 output-channel tiles for C <= 64 / 128 / 256 / 512 / 1024, 4 sequences per
# workgroup.  attention_kernel "<MODE, LP, TMO>": 64 / LP sequences per workgroup, TMO = 1 / 2 / 4 / 8 / 16 by C.
ATTN_F16 = [
    # shape (B, F, H, W, C), temporal, iso, kernel, parts of the shape string
    ((1, 16, 8, 8, 64), True, True, 'attention_reg_kernel', ['<2, 4, fp8 0>', 'C64 L16 nseq64']),          # per (sequence, head): head-isolating Wo
    ((1, 16, 1, 2, 512), True, False, 'attention_reg_kernel', ['<2, 32, fp8 0>', 'C512 L16 nseq2']),       # the widths of BASELINE configs[3] at 16 frames;
    ((1, 16, 1, 2, 1024), True, False, 'attention_reg_kernel', ['<2, 64, fp8 0>', 'C1024 L16 nseq2']),     # 2 of a workgroup's 4 sequences exist
    ((1, 32, 1, 3, 256), True, False, 'attention_kernel', ['<2, 32, 4>', 'C256 L32 nseq3']),               # configs[3]: 32 frames, the last workgroup half empty
    ((1, 32, 1, 3, 256), True, True, 'attention_kernel', ['<2, 32, 4>', 'C256 L32 nseq3']),                # ... per (sequence, head)
    ((1, 32, 1, 3, 512), True, False, 'attention_kernel', ['<2, 32, 8>', 'C512 L32 nseq3']),
    ((1, 32, 1, 3, 1024), True, False, 'attention_kernel', ['<2, 32, 16>', 'C1024 L32 nseq3']),
    ((1, 20, 1, 3, 256), True, False, 'attention_kernel', ['<2, 32, 4>', 'C256 L20 nseq3']),               # keys 20..31 masked
]


@pytest.mark.parametrize('shape,temporal,iso,kernel,parts', ATTN_F16)
def test_attention_f16_per_group(shape, temporal, iso, kernel, parts):
    c = AC.attn_case(shape, temporal, False, 'f16', False, iso, True)
    what = f'attention f16 {shape} temporal={int(temporal)} iso={int(iso)}'
    y, rec = _run_attention(c, 'f16', False, False, what)
    assert_launches(rec, [(kernel, parts)], what)
    PR.assert_first(PR.cid('attention f16', shape, temporal, iso), rec)
    assert y.dtype == F32
    _check(c, y, what)


# ---- SLA (vdx_sla_forward, mode f16) ------------------------------------------------------------------------------------------------------
SLA_F16 = [
    # shape, iso, chunks
    ((1, 2, 16, 16, 64), False, 1),        # C = 64 and 128 on the generic kernels: fp16 mode alone does that (the other modes: one wave per head)
    ((2, 3, 8, 8, 128), True, 1),          # ... per (frame, head)
    ((1, 1, 16, 16, 512), False, 1),       # sla_out_kernel TMO 8
    ((1, 1, 16, 16, 1024), False, 1),      # ... TMO 16: the bottleneck width of dim 128
]


@pytest.mark.parametrize('shape,iso,nchunk', SLA_F16)
def test_sla_f16_per_group(shape, iso, nchunk):
    B, Fr, H, W, C = shape
    c = AC.sla_case(shape, False, 'f16', iso)
    what = f'SLA f16 {shape} iso={int(iso)}'
    y, rec = _run_sla(c, 'f16', False, what)
    assert_launches(rec, _sla32('f16', C, H * W, B * Fr, nchunk), what)
    PR.assert_first(PR.cid('sla f16', shape, iso), rec)
    _check(c, y, what)


# ---- convs (ops.conv_forward, mode f16) ----------------------------------------------------------------------------------------------------
# conv_igemm_kernel "<MODE, BC, 2, waves, INF>": BC = 64 output channels per workgroup up to Cout 64, else 128; 8 waves except the 64-channel
# stride-2 form (4); INF 0 = fp32 tensors staged through M::store4 (conv_igemm.hip:284-293) -- the only input form fp16 mode has.


def _igemm_parts(cout, stride):
    bc = 64 if cout <= 64 else 128
    return [f'<2, {bc}, 2, {4 if bc == 64 and stride == 2 else 8}, 0>']


def _fwd(x, kern, bias, k, stride, kind):
    if kind == 1:
        return R.conv_transpose_144(x, kern, bias)
    if k == 1:
        return R.conv_pointwise(x, kern[0], bias)
    return R.conv_1kk(x, kern, bias, stride=stride)


def _conv_twice(fn, what):
    """fn() -> tensor(s), twice under the launch hook on NaN-filled outputs (nan_outputs: ops.conv_forward allocates with torch.empty),
    bit-identical.  -> (outputs of one run on the CPU, launches of one run)"""
    with launches() as rec, nan_outputs():
        a, b = fn(), fn()
        torch.cuda.synchronize()
    a, b = [t if isinstance(t, (tuple, list)) else (t,) for t in (a, b)]
    for u, v in zip(a, b):                                                    # (the fp64 statistics slab is summed with atomics: not compared)
        assert u.dtype != F32 or torch.equal(u.view(torch.uint8), v.view(torch.uint8)), f'{what}: two runs are not bit-identical'
    n = len(rec) // 2
    assert rec[:n] == rec[n:], f'{what}: the two runs launched differently: {rec}'
    print(f'[{what}] launched: ' + '; '.join(f'{k} {s}' for k, s in rec[:n]))
    return [t.cpu() for t in a], rec[:n]


def _assert_tiles_exact(got, ref32, ref64, what):
    """Exact-products bound per (frame, 16 x 16 tile) and globally, from the reference side (P.exact_products_bounds, stated 2e-6)."""
    sl = P.tile_slices(ref64.shape)
    bound, sb, floor = P.exact_products_bounds(ref32, ref64, sl, None, P.FWD_STATED)
    P.assert_exact_products(got, ref64, bound, sl, sb, None, f'{what} (CPU floor {floor:.1e})')


@pytest.mark.parametrize('case', FWD_CASES)
def test_conv_f16_per_tile(case):
    """The shapes of test_conv_parity with fp16-representable operands, bias and the statistics epilogue."""
    from video_diffusion_nnx_amd import ops
    B, Fr, H, W, Cin, Cout, k, stride, kind = case
    g = torch.Generator().manual_seed(sum(case) + 16)
    x = P.f16r(torch.randn(B, Fr, H, W, Cin, generator=g))
    kern = P.f16r(torch.randn(1, k, k, Cin, Cout, generator=g) / (k * k * Cin) ** 0.5)
    bias = torch.randn(Cout, generator=g)
    ref64, ref32 = _fwd(x.double(), kern.double(), bias.double(), k, stride, kind), _fwd(x, kern, bias, k, stride, kind)
    pw = ops.pack_conv_weights(_dev(kern), 'f16')
    xd, bd = _dev(x), _dev(bias)
    what = f'conv f16 {case}'

    def go():
        stats = ops.gn_stats_zeros(B, 8, DEV) if Cout % 8 == 0 else None
        y = ops.conv_forward(xd, pw, Cout, mode='f16', bias=bd, kind=kind, k=k, stride=stride, out_stats=stats, out_groups=8)
        return (y, stats) if stats is not None else (y,)
    out, rec = _conv_twice(go, what)
    assert_launches(rec, [(IGEMM, _igemm_parts(Cout, stride))], what)
    PR.assert_first(PR.cid('conv f16', case), rec)
    _assert_tiles_exact(out[0], ref32, ref64, what)
    if len(out) > 1:
        tiles = -(-ref64[0].numel() // Cout // 256)
        P.assert_gn_stats(ops.gn_stats_reduce(out[1], B, 8), ref64, ref32, tiles, what=what)


def test_conv_f16_concat_and_prologue():
    """Two-pointer concat input, then the fused GroupNorm / SiLU / scale-shift prologue consuming it: per (frame, tile) at
    max(2e-6, 4 x the flip floor of the activation ROUNDED TO FP16), producer slab and hand-made slab, with and without scale / shift."""
    from video_diffusion_nnx_amd import ops
    g = torch.Generator().manual_seed(7)
    B, Fr, H, W, C0, C1, Cout = 2, 4, 8, 8, 32, 16, 32
    xa, xb = P.f16r(torch.randn(B, Fr, H, W, C0, generator=g)), P.f16r(torch.randn(B, Fr, H, W, C1, generator=g))
    kern = P.f16r(torch.randn(1, 3, 3, C0 + C1, Cout, generator=g) / (9 * (C0 + C1)) ** 0.5)
    bias = torch.randn(Cout, generator=g)
    pw = ops.pack_conv_weights(_dev(kern), 'f16')
    cat = torch.cat((xa, xb), -1)
    ref64, ref32 = R.conv_1kk(cat.double(), kern.double(), bias.double()), R.conv_1kk(cat, kern, bias)

    def first():
        stats = ops.gn_stats_zeros(B, 8, DEV)
        return ops.conv_forward(_dev(xa), pw, Cout, mode='f16', bias=_dev(bias), x1=_dev(xb), out_stats=stats), stats
    (y1, stats1), rec = _conv_twice(first, 'conv f16 concat')
    assert_launches(rec, [(IGEMM, _igemm_parts(Cout, 1) + ['concat'])], 'conv f16 concat')
    PR.assert_first(PR.cid('conv f16 concat'), rec)
    _assert_tiles_exact(y1, ref32, ref64, 'conv f16 concat')
    P.assert_gn_stats(ops.gn_stats_reduce(stats1, B, 8), ref64, ref32, 1, what='conv f16 concat')
    gamma, beta = 1 + 0.1 * torch.randn(Cout, generator=g), 0.1 * torch.randn(Cout, generator=g)
    ss = torch.randn(B, 2 * Cout, generator=g) * 0.3
    kern2 = P.f16r(torch.randn(1, 3, 3, Cout, Cout, generator=g) / (9 * Cout) ** 0.5)
    pw2 = ops.pack_conv_weights(_dev(kern2), 'f16')
    y1d, y1f = _dev(y1), y1.double()
    hand = P.spread_slots(P.gn_stats_slab(y1f), seed=Cout).reshape(-1)
    for use_ss in (True, False):
        def act(dt):
            h = R.group_norm(y1f.to(dt), gamma.to(dt), beta.to(dt), 8)
            if use_ss:
                h = h * (ss.to(dt)[:, None, None, None, :Cout] + 1) + ss.to(dt)[:, None, None, None, Cout:]
            return P.f16r(R.silu(h)).double()
        out_of = lambda a: R.conv_1kk(a, kern2.double(), None)
        bound, floor = P.tile_bound(act(F32), act(F64), out_of, operand='f16')
        print(f'[conv f16 prologue use_ss={use_ss}] flip floor {floor:.3e} -> per-tile bound {bound:.3e}')
        assert bound < 5e-3 / 8, 'a derived bound above an eighth of the bf16 form\'s 5e-3 would be a finding (fp16 has 3 more bits)'
        ref2 = out_of(act(F64))
        for label, slab in (('producer slab', stats1), ('hand-made slab', hand)):
            what = f'conv f16 prologue use_ss={use_ss}, {label}'
            sd = slab.to(DEV)
            (y2,), rec = _conv_twice(lambda: ops.conv_forward(y1d, pw2, Cout, mode='f16', in_stats=sd, gamma=_dev(gamma), beta=_dev(beta),
                                                              scale_shift=_dev(ss) if use_ss else None), what)
            assert_launches(rec, [(IGEMM, _igemm_parts(Cout, 1) + ['+prologue'])], what)
            PR.assert_first(PR.cid('conv f16 prologue', use_ss), rec)
            P.assert_tiles(y2, ref2, bound, what=what)


F16_CHAINS = [
    # mode, bf16 tensors, B, F, H, W, C0, C1, Cout   (tests/test_gpu_conv.py GENERIC_CHAINS: what the dim-128 network at fp16 operands launches)
    ('f16', False, 2, 3, 16, 16, 24, 16, 72),        # <2, 128, 2, 8, 0> conv3x3 concat, then <2, 128, 2, 8, 0> conv3x3 +prologue (128-channel workgroup tile)
]
F16_FORMS = [
    # mode, bf16 tensors, B, F, H, W, C0, C1, Cout, k, stride, kind, res   (tests/test_gpu_conv.py GENERIC_FORMS)
    ('f16', False, 1, 3, 6, 10, 24, 16, 40, 1, 1, 0, None),        # <2, 64, 2, 8, 0> conv1x1 concat
    ('f16', False, 1, 3, 6, 10, 24, 24, 72, 1, 1, 0, None),        # <2, 128, 2, 8, 0> conv1x1 concat
    ('f16', False, 1, 3, 12, 20, 40, 0, 72, 4, 2, 0, None),        # <2, 128, 2, 8, 0> conv4x4 s2
]


@pytest.mark.parametrize('mode,t16,B,Fr,H,W,C0,C1,Cout', F16_CHAINS)
def test_conv_f16_chain(mode, t16, B, Fr, H, W, C0, C1, Cout):
    """The 128-channel workgroup tile of the fp16 generic conv on a concat input, then its fused-prologue form: per (frame, tile), the
    prologue at max(2e-6, 4 x the flip floor of the activation rounded to fp16), below an eighth of the bf16 form's 5e-3."""
    _conv_chain(mode, t16, B, Fr, H, W, C0, C1, Cout, 'f16 chain', 5e-3 / 8)


@pytest.mark.parametrize('mode,t16,B,Fr,H,W,C0,C1,Cout,k,stride,kind,res', F16_FORMS)
def test_conv_f16_form(mode, t16, B, Fr, H, W, C0, C1, Cout, k, stride, kind, res):
    """Pointwise convs on a concat input (the res_conv of the up blocks) and the Downsample with more than 64 output channels."""
    _conv_form(mode, t16, B, Fr, H, W, C0, C1, Cout, k, stride, kind, res, 'f16 form')


PW_F16 = [((1, 2, 9, 9), 256, 128), ((1, 3, 5, 7), 40, 48)]


@pytest.mark.parametrize('shape,cin,cout', PW_F16)
def test_pointwise_conv_f16_bias_and_residual(shape, cin, cout):
    """The out-projection of the long attention: 1x1, bias, fp32 residual; 40 -> 48: ragged channels on both sides."""
    from video_diffusion_nnx_amd import ops
    g = torch.Generator().manual_seed(cin + cout)
    x = P.f16r(torch.randn(*shape, cin, generator=g))
    kern = P.f16r(torch.randn(1, cin, cout, generator=g) / cin ** 0.5)
    bias, res = torch.randn(cout, generator=g), torch.randn(*shape, cout, generator=g)
    ref = lambda dt: x.to(dt) @ kern[0].to(dt) + bias.to(dt) + res.to(dt)
    pw = ops.pack_conv_weights(_dev(kern), 'f16')
    what = f'1x1 conv f16 {shape} {cin}->{cout} + bias + res'
    (y,), rec = _conv_twice(lambda: ops.conv_forward(_dev(x), pw, cout, mode='f16', bias=_dev(bias), k=1, res=_dev(res)), what)
    assert_launches(rec, [(IGEMM, _igemm_parts(cout, 1) + ['+res'])], what)
    PR.assert_first(PR.cid('pw f16', shape, cin, cout), rec)
    _assert_tiles_exact(y, ref(F32), ref(F64), what)


@pytest.mark.parametrize('case', BWD_CASES)
def test_conv_dgrad_f16_per_tile(case):
    """Data gradient = the forward kernel on pack_weights_t_kernel<MODE_F16>'s transposed / flipped packing (Down <-> Up swapped)."""
    from video_diffusion_nnx_amd import ops
    B, Fr, H, W, Cin, Cout, k, stride, kind = case
    g = torch.Generator().manual_seed(sum(case) + 16)
    kern = P.f16r(torch.randn(1, k, k, Cin, Cout, generator=g) / (k * k * Cin) ** 0.5)
    yshape = _fwd(torch.zeros(B, Fr, H, W, Cin), kern, None, k, stride, kind).shape
    dy = P.f16r(torch.randn(yshape, generator=g))

    def gx_of(dt):
        x = torch.zeros(B, Fr, H, W, Cin, dtype=dt, requires_grad=True)
        (gx,) = torch.autograd.grad(_fwd(x, kern.to(dt), None, k, stride, kind), x, dy.to(dt))
        return gx
    ref64, ref32 = gx_of(F64), gx_of(F32)
    pwt = ops.pack_conv_weights_t(_dev(kern), 'f16')
    dyd = _dev(dy)
    kw = dict(k=4, stride=2) if kind == 1 else dict(kind=1) if stride == 2 else dict(k=k)
    what = f'dgrad f16 {case}'
    (dx,), rec = _conv_twice(lambda: ops.conv_forward(dyd, pwt, Cin, mode='f16', **kw), what)
    assert_launches(rec, [(IGEMM, _igemm_parts(Cin, 2 if kind == 1 else 1))], what)
    _assert_tiles_exact(dx, ref32, ref64, what)


def test_conv_f16_subnormal_operands():
    """x scaled by 2^-12: a fifth of the operands are below 2^-14, fp16 subnormals once staged.  The result must be the exact-products
    conv of EITHER the IEEE-rounded operands (gradual underflow, P.f16r) or the flushed ones (P.f16r_ftz); which one is printed (and
    recorded in DESIGN.md section 8).  The two references are 6e-2 apart (printed); matching neither is a kernel fault."""
    from video_diffusion_nnx_amd import ops
    g = torch.Generator().manual_seed(14)
    B, Fr, H, W, Cin, Cout = 1, 4, 16, 16, 32, 64
    x = torch.randn(B, Fr, H, W, Cin, generator=g) * 2.0 ** -12
    kern = P.f16r(torch.randn(1, 3, 3, Cin, Cout, generator=g) / (9 * Cin) ** 0.5)
    share = (P.f16r(x).abs() < 2.0 ** -14).double().mean().item()
    pw = ops.pack_conv_weights(_dev(kern), 'f16')
    what = 'conv f16 subnormal operands'
    (y,), rec = _conv_twice(lambda: ops.conv_forward(_dev(x), pw, Cout, mode='f16'), what)
    assert_launches(rec, [(IGEMM, _igemm_parts(Cout, 1))], what)
    PR.assert_first(PR.cid('conv f16 subnormal'), rec)
    assert torch.isfinite(y).all()
    sl = P.tile_slices(y.shape)
    verdict, refs = {}, []
    for name, rd in (('IEEE (gradual underflow)', P.f16r), ('flush to zero', P.f16r_ftz)):
        xr, kr = rd(x), rd(kern)
        ref64, ref32 = R.conv_1kk(xr.double(), kr.double(), None), R.conv_1kk(xr, kr, None)
        bound, sb, _ = P.exact_products_bounds(ref32, ref64, sl, None, P.FWD_STATED)
        worst = max(r / sb[lab] for lab, r in P.slice_rels(y, ref64, sl))
        verdict[name] = (P.rel(y, ref64), bound, worst)
        print(f'[{what}] against {name}: rel {verdict[name][0]:.3e} (bound {bound:.3e}), worst tile at {worst:.3g} x its bound')
        refs = refs + [ref64]
    print(f'[{what}] the two references are {P.rel(refs[1], refs[0]):.2e} apart')
    ok = [n for n, (r, b, w) in verdict.items() if r < b and w < 1.0]
    print(f'[{what}] {share:.1%} of the staged operands are fp16 subnormals; the kernel matches: {ok}')
    assert len(ok) == 1, f'{what}: matches {ok or "neither reference"}: {verdict}'


# ---- rejections ----------------------------------------------------------------------------------------------------------------------------


def test_f16_mode_rejects_bf16_tensors_and_the_fp8_core():
    """bf16 tensors and the fp8 core exist in bf16 mode only: each call returns VDX_ERR_INVALID (-1) and launches nothing."""
    from video_diffusion_nnx_amd import _lib as L, ops
    from video_diffusion_nnx_amd import unet3d as U
    g = torch.Generator().manual_seed(3)
    z = lambda *s, dtype=F32: torch.zeros(*s, dtype=dtype, device=DEV)
    w = FC.mha_weights(128, g, operand='f16')
    packed = (ops.pack_conv_weights(_dev(w[0]), 'f16'), _dev(w[1]), ops.pack_conv_weights(_dev(w[2]), 'f16'), _dev(w[3]))
    pw = ops.pack_conv_weights(z(1, 3, 3, 64, 64), 'f16')
    unet = U.Unet3D(rngs=0, mode='f16', dim=16, channels=1)
    h = unet.handle(4, 16)
    torch.cuda.synchronize()
    with launches() as rec:
        with pytest.raises(L.VdxError, match='status -1'):                                    # a bf16 input tensor in an f16 conv
            ops.conv_forward(z(1, 2, 8, 8, 64, dtype=BF), pw, 64, mode='f16')
        with pytest.raises(L.VdxError, match='status -1'):                                    # ... a bf16 output
            ops.conv_forward(z(1, 2, 8, 8, 64), pw, 64, mode='f16', y_bf16=True)
        with pytest.raises(L.VdxError, match='status -1'):                                    # ... a bf16 residual
            ops.conv_forward(z(1, 2, 8, 8, 64), pw, 64, mode='f16', res=z(1, 2, 8, 8, 64, dtype=BF))
        x = z(1, 16, 2, 2, 128)
        y = _nan_like(x)
        assert L.vdx_attention_forward_ex(ops._mode('f16'), L.ptr(x), L.ptr(y), *[L.ptr(t) for t in packed], 1, 16, 2, 2, 128, 8, 1, 1, L.stream_ptr()) == -1
        with pytest.raises(L.VdxError, match='status -1'):                                    # bf16 tensors through the long attention
            ops.attention_long_forward(z(1, 1, 9, 9, 128, dtype=BF), packed, 8, 'f16')
        assert U.vdx_set_attention_fp8(h.ptr, 1) == -1
        assert U.vdx_set_activation_storage(h.ptr, 1) == -1 and U.vdx_set_activation_storage(h.ptr, 2) == -1
        torch.cuda.synchronize()
    assert rec == [], f'a rejected call launched {rec}'
    assert torch.isnan(y).all()
    assert U.vdx_get_activation_storage(h.ptr) == 0
