"""GPU parity: conv_igemm (through the C ABI) vs oracle/unet3d_ref.py conv restatements."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _parity as P
import _parity_routes as PR
from oracle import unet3d_ref as R

# Every kernel call under test runs inside PR.bound(case id): the first launch it reports is compared with the row of
# tests/golden/parity_routes.json that tests/_parity_routes.py recorded for the same call on the CPU (one comparison, no second run).


def _bf16r(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _check_stats(stats, B, ref64, ref32, what):
    """The statistics epilogue against the fp64 conv, per (sample, group), at 8 x the conv and its sums evaluated in fp32 on the CPU
    (tests/_parity.py assert_gn_stats); one tile = 256 output pixels, the unit a workgroup flushes."""
    from video_diffusion_nnx_amd import ops
    tiles = -(-ref64[0].numel() // ref64.shape[-1] // 256)
    P.assert_gn_stats(ops.gn_stats_reduce(stats, B, 8).cpu(), ref64, ref32, tiles, what=what)


def _check_prologue_conv(run, y1f, gamma, beta, ss, kern2, ref2, stats, bf16_out, what):
    """A fused-prologue conv, per (frame, 16 x 16 tile), against the reference whose activation is rounded to bf16 where the kernel
    rounds it; bound = max(2e-6, 4 x the rounding-boundary flip floor) (+ 2^-9 for a bf16 output), tests/_parity.py tile_bound.
    run(slab) launches the conv with that statistics slab: the producer's own, then a hand-made one of y1 spread over the slots, so
    that producer and consumer are judged separately.  y1f: the tensor the conv reads, fp64; ref2: the test's own fp64 reference of the
    conv (activation rounded to bf16).  The flip floor is taken on the first two frames of every sample: the activation is elementwise
    and a tile's output depends on its own frame alone, so more frames only repeat the CPU convs."""
    C = y1f.shape[-1]
    def act(dt):
        h = R.group_norm(y1f.to(dt), gamma.to(dt), beta.to(dt), 8)
        if ss is not None:
            h = h * (ss.to(dt)[:, None, None, None, :C] + 1) + ss.to(dt)[:, None, None, None, C:]
        return P.bf16r(R.silu(h)).double()
    k2 = P.bf16r(kern2).double()
    out_of = lambda a: R.conv_1kk(a[:, :2], k2, None)
    bound, floor = P.tile_bound(act(torch.float32), act(torch.float64), out_of, bf16_out=bf16_out)
    print(f'[prologue {what}] flip floor {floor:.3e} -> per-tile bound {bound:.3e}')
    assert bound < 5e-3, 'a derived bound above the 5e-3 this test states would be a finding'
    hand = P.spread_slots(P.gn_stats_slab(y1f), seed=C).reshape(-1).to(stats.device)
    for label, slab in (('producer slab', stats), ('hand-made slab', hand)):
        y2 = run(slab)
        torch.cuda.synchronize()
        P.assert_tiles(y2.float().cpu(), ref2, bound, what=f'{what}, {label}')


CASES = [
    # B, F, H, W, Cin, Cout, k, stride, kind
    (1, 4, 16, 16, 16, 32, 3, 1, 0),
    (2, 4, 16, 16, 64, 64, 3, 1, 0),
    (1, 2, 32, 32, 64, 128, 3, 1, 0),
    (1, 3, 6, 10, 8, 24, 3, 1, 0),        # ragged: odd frames, non-pow2 image, masked tiles
    (1, 4, 2, 2, 128, 128, 3, 1, 0),      # 2x2 images (tiny-config bottleneck)
    (1, 4, 16, 16, 32, 32, 4, 2, 0),      # Downsample
    (2, 2, 8, 8, 64, 64, 4, 2, 0),
    (1, 4, 8, 8, 32, 32, 4, 1, 1),        # Upsample (ConvTranspose)
    (1, 2, 4, 4, 128, 128, 4, 1, 1),
    (1, 4, 8, 8, 48, 40, 1, 1, 0),        # pointwise
    (1, 16, 64, 64, 64, 64, 3, 1, 0),     # north-star level-0 shape
]


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
@pytest.mark.parametrize('case', CASES)
def test_conv_parity(mode, case):
    from video_diffusion_nnx_amd import ops
    B, Fr, H, W, Cin, Cout, k, stride, kind = case
    g = torch.Generator().manual_seed(hash(case) % 1000)
    x = torch.randn(B, Fr, H, W, Cin, generator=g)
    kern = torch.randn(1, k, k, Cin, Cout, generator=g) / (k * k * Cin) ** 0.5
    bias = torch.randn(Cout, generator=g)
    dev = torch.device('cuda:0')
    pw = ops.pack_conv_weights(kern.to(dev), mode)
    stats = ops.gn_stats_zeros(B, 8, dev) if Cout % 8 == 0 else None
    with PR.bound(PR.cid('conv', mode, case)):
        y = ops.conv_forward(x.to(dev), pw, Cout, mode=mode, bias=bias.to(dev), kind=kind, k=k, stride=stride,
                             out_stats=stats, out_groups=8)
    torch.cuda.synchronize()
    xr, kr = (x, kern) if mode == 'f32' else (_bf16r(x), _bf16r(kern))
    if kind == 1:
        ref = R.conv_transpose_144(xr.double(), kr.double(), bias.double())
    elif k == 1:
        ref = R.conv_pointwise(xr.double(), kr.double()[0], bias.double())
    else:
        ref = R.conv_1kk(xr.double(), kr.double(), bias.double(), stride=stride)
    assert y.shape == ref.shape
    rel = _rel(y.cpu().double(), ref)
    assert rel < 2e-6, f'{mode} {case}: rel {rel}'           # exact products, fp32 accumulate
    if mode == 'bf16':                                      # and against the un-rounded fp32 reference
        full = (R.conv_transpose_144(x.double(), kern.double(), bias.double()) if kind == 1 else
                R.conv_pointwise(x.double(), kern.double()[0], bias.double()) if k == 1 else
                R.conv_1kk(x.double(), kern.double(), bias.double(), stride=stride))
        assert _rel(y.cpu().double(), full) < 8e-3
    if stats is not None:
        s = ops.gn_stats_reduce(stats, B, 8).cpu()
        yg = ref.reshape(B, -1, 8, Cout // 8)
        np.testing.assert_allclose(s[..., 0], yg.sum(dim=(1, 3)), rtol=1e-4, atol=1e-2)
        np.testing.assert_allclose(s[..., 1], (yg * yg).sum(dim=(1, 3)), rtol=1e-4, atol=1e-2)


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_conv_concat_and_prologue(mode):
    """Two-pointer concat input; GroupNorm-apply * (scale+1) + shift -> SiLU prologue (Block, modules.py:171-179)."""
    from video_diffusion_nnx_amd import ops
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(7)
    B, Fr, H, W, C0, C1, Cout = 2, 4, 8, 8, 32, 16, 32
    xa, xb = torch.randn(B, Fr, H, W, C0, generator=g), torch.randn(B, Fr, H, W, C1, generator=g)
    kern = torch.randn(1, 3, 3, C0 + C1, Cout, generator=g) / (9 * (C0 + C1)) ** 0.5
    bias = torch.randn(Cout, generator=g)
    pw = ops.pack_conv_weights(kern.to(dev), mode)
    stats1 = ops.gn_stats_zeros(B, 8, dev)
    with PR.bound(PR.cid('conv concat', mode)):
        y1 = ops.conv_forward(xa.to(dev), pw, Cout, mode=mode, bias=bias.to(dev), x1=xb.to(dev), out_stats=stats1)
    cat = torch.cat((xa, xb), -1)
    cr, kr = (cat, kern) if mode == 'f32' else (_bf16r(cat), _bf16r(kern))
    ref1 = R.conv_1kk(cr.double(), kr.double(), bias.double())
    assert _rel(y1.cpu().double(), ref1) < 2e-6
    # second conv consumes y1 through the fused prologue
    gamma, beta = 1 + 0.1 * torch.randn(Cout, generator=g), 0.1 * torch.randn(Cout, generator=g)
    ss = torch.randn(B, 2 * Cout, generator=g) * 0.3
    kern2 = torch.randn(1, 3, 3, Cout, Cout, generator=g) / (9 * Cout) ** 0.5
    pw2 = ops.pack_conv_weights(kern2.to(dev), mode)
    for use_ss in (True, False):
        with PR.bound(PR.cid('conv prologue', mode, use_ss)):
            y2 = ops.conv_forward(y1, pw2, Cout, mode=mode, in_stats=stats1, gamma=gamma.to(dev), beta=beta.to(dev),
                                  scale_shift=ss.to(dev) if use_ss else None)
        h = R.group_norm(y1.cpu().double(), gamma.double(), beta.double(), 8)
        if use_ss:
            h = h * (ss[:, None, None, None, :Cout].double() + 1) + ss[:, None, None, None, Cout:].double()
        h = R.silu(h)
        if mode == 'bf16':
            h, k2 = _bf16r(h.float()).double(), _bf16r(kern2).double()
        else:
            k2 = kern2.double()
        ref2 = R.conv_1kk(h, k2, None)
        tol = 2e-5 if mode == 'f32' else 3e-3     # bf16: rounding boundary flips of the fused activation
        assert _rel(y2.cpu().double(), ref2) < tol, (mode, use_ss, _rel(y2.cpu().double(), ref2))


C64_CASES = [(False, 2, 32), (True, 2, 32), (True, 3, 22)]      # act_bf16, B, F


@pytest.mark.parametrize('act_bf16,B,Fr', C64_CASES)
def test_persistent_c64_conv(act_bf16, B, Fr):
    """The persistent level-0 specialisations (3x3, 64 -> 64 channels, bf16 mode, >= 1024 tiles of 16x16 pixels; fp32 tensors:
    conv64p_kernel, weights resident in LDS; bf16 tensors: conv64r_kernel for the plain form, weights in registers + a three-deep
    LDS-DMA tile ring, and conv64q_kernel<64, true> for the prologue form, the prologue applied in place one tile ahead): plain form
    with statistics, then the fused-prologue form consuming it, several samples
    so that the per-sample flush of the register-resident statistics and the coefficient switch are exercised.  (3, 22): 1056 tiles = 5
    per workgroup, so workgroups 70 and 140 walk ACROSS a sample boundary (tiles 352, 704)."""
    from video_diffusion_nnx_amd import ops
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(11)
    H, W, C = 64, 64, 64                                   # (2, 32): 64 frames x 16 tiles = 1024 tiles
    x = torch.randn(B, Fr, H, W, C, generator=g)
    x[1] *= 1.7                                            # different statistics per sample
    if B > 2:
        x[2] = x[2] * 0.6 + 0.4
    kern = torch.randn(1, 3, 3, C, C, generator=g) / (9 * C) ** 0.5
    bias = torch.randn(C, generator=g)
    pw = ops.pack_conv_weights(kern.to(dev), 'bf16')
    stats1 = ops.gn_stats_zeros(B, 8, dev)
    xin = x.to(dev).to(torch.bfloat16) if act_bf16 else x.to(dev)
    with PR.bound(PR.cid('c64', act_bf16, B, Fr, 'plain')):
        y1 = ops.conv_forward(xin, pw, C, mode='bf16', bias=bias.to(dev), out_stats=stats1, y_bf16=act_bf16)
    torch.cuda.synchronize()
    ref1 = R.conv_1kk(_bf16r(x).double(), _bf16r(kern).double(), bias.double())
    y1f = y1.float().cpu().double()
    assert _rel(y1f, ref1) < (4e-3 if act_bf16 else 2e-6)    # bf16 output: one rounding of the result
    if act_bf16:
        P.assert_bf16_store(y1.cpu(), ref1, P.FWD_STATED, f'conv64r B{B} F{Fr}')
    s = ops.gn_stats_reduce(stats1, B, 8).cpu()
    yg = ref1.reshape(B, -1, 8, C // 8)
    np.testing.assert_allclose(s[..., 0], yg.sum(dim=(1, 3)), rtol=2e-3, atol=5.0)       # statistics are taken before the output rounding
    np.testing.assert_allclose(s[..., 1], (yg * yg).sum(dim=(1, 3)), rtol=2e-3)
    _check_stats(stats1, B, ref1, R.conv_1kk(_bf16r(x), _bf16r(kern), bias), f'c64 conv act_bf16={act_bf16} B{B} F{Fr}')
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    ss = torch.randn(B, 2 * C, generator=g) * 0.3
    kern2 = torch.randn(1, 3, 3, C, C, generator=g) / (9 * C) ** 0.5
    pw2 = ops.pack_conv_weights(kern2.to(dev), 'bf16')
    with PR.bound(PR.cid('c64', act_bf16, B, Fr, 'prologue')):
        y2 = ops.conv_forward(y1, pw2, C, mode='bf16', in_stats=stats1, gamma=gamma.to(dev), beta=beta.to(dev), scale_shift=ss.to(dev),
                              y_bf16=act_bf16)
    h = R.group_norm(y1f, gamma.double(), beta.double(), 8)
    h = R.silu(h * (ss[:, None, None, None, :C].double() + 1) + ss[:, None, None, None, C:].double())
    ref2 = R.conv_1kk(_bf16r(h.float()).double(), _bf16r(kern2).double(), None)
    assert _rel(y2.float().cpu().double(), ref2) < 5e-3
    _check_prologue_conv(lambda slab: ops.conv_forward(y1, pw2, C, mode='bf16', in_stats=slab, gamma=gamma.to(dev), beta=beta.to(dev),
                                                       scale_shift=ss.to(dev), y_bf16=act_bf16),
                         y1f, gamma, beta, ss, kern2, ref2, stats1, act_bf16, f'c64 conv act_bf16={act_bf16} B{B} F{Fr}')


@pytest.mark.parametrize('concat', [True, False])
def test_persistent_c128_to_64_conv(concat):
    """conv64q_kernel<128, ...>: 3x3, 128 -> 64 channels (two-pointer concat of 64 + 64, or one 128-channel tensor), bf16 tensors,
    >= 1024 tiles, two 64-channel plane passes per tile; statistics of two samples."""
    from video_diffusion_nnx_amd import ops
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(13)
    B, Fr, H, W = 2, 32, 64, 64
    xa = torch.randn(B, Fr, H, W, 64, generator=g)
    xb = torch.randn(B, Fr, H, W, 64, generator=g)
    xb[1] *= 0.5
    kern = torch.randn(1, 3, 3, 128, 64, generator=g) / (9 * 128) ** 0.5
    bias = torch.randn(64, generator=g)
    pw = ops.pack_conv_weights(kern.to(dev), 'bf16')
    stats = ops.gn_stats_zeros(B, 8, dev)
    with PR.bound(PR.cid('c128->64', concat)):
        if concat:
            y = ops.conv_forward(xa.to(dev).to(torch.bfloat16), pw, 64, mode='bf16', bias=bias.to(dev), x1=xb.to(dev).to(torch.bfloat16),
                                 out_stats=stats, y_bf16=True)
        else:
            y = ops.conv_forward(torch.cat((xa, xb), -1).to(dev).to(torch.bfloat16), pw, 64, mode='bf16', bias=bias.to(dev), out_stats=stats, y_bf16=True)
    torch.cuda.synchronize()
    ref = R.conv_1kk(_bf16r(torch.cat((xa, xb), -1)).double(), _bf16r(kern).double(), bias.double())
    assert _rel(y.float().cpu().double(), ref) < 4e-3
    P.assert_bf16_store(y.cpu(), ref, P.FWD_STATED, f'conv64q<128> concat={concat}')
    s = ops.gn_stats_reduce(stats, B, 8).cpu()
    yg = ref.reshape(B, -1, 8, 8)
    np.testing.assert_allclose(s[..., 0], yg.sum(dim=(1, 3)), rtol=2e-3, atol=5.0)
    np.testing.assert_allclose(s[..., 1], (yg * yg).sum(dim=(1, 3)), rtol=2e-3)
    _check_stats(stats, B, ref, R.conv_1kk(_bf16r(torch.cat((xa, xb), -1)), _bf16r(kern), bias), f'conv64q<128> concat={concat}')


CONCAT32_CASES = [(32, 2, 32, 64), (64, 16, 16, 32)]            # c, B, F, S


@pytest.mark.parametrize('c,B,Fr,S', CONCAT32_CASES)
def test_persistent_concat_conv_32_outputs(c, B, Fr, S):
    """conv64q_kernel<64 | 128, ..., COUT 32>: the 3x3 convs on a concat input (c + c channels) with 32 output channels of dim-32 networks
    (configs/config_v2_2.yaml as written: ups.3 block1 at 64 x 64, ups.2 block1 at 32 x 32), bf16 tensors, >= 1024 tiles; statistics of
    samples of different scale."""
    from video_diffusion_nnx_amd import ops
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(17 + c)
    xa = torch.randn(B, Fr, S, S, c, generator=g)
    xb = torch.randn(B, Fr, S, S, c, generator=g)
    xb[1] *= 0.5
    kern = torch.randn(1, 3, 3, 2 * c, 32, generator=g) / (9 * 2 * c) ** 0.5
    bias = torch.randn(32, generator=g)
    pw = ops.pack_conv_weights(kern.to(dev), 'bf16')
    stats = ops.gn_stats_zeros(B, 8, dev)
    with PR.bound(PR.cid('concat->32', c, B, Fr, S)):
        y = ops.conv_forward(xa.to(dev).to(torch.bfloat16), pw, 32, mode='bf16', bias=bias.to(dev), x1=xb.to(dev).to(torch.bfloat16),
                             out_stats=stats, y_bf16=True)
    torch.cuda.synchronize()
    ref = R.conv_1kk(_bf16r(torch.cat((xa, xb), -1)).double(), _bf16r(kern).double(), bias.double())
    assert _rel(y.float().cpu().double(), ref) < 4e-3
    P.assert_bf16_store(y.cpu(), ref, P.FWD_STATED, f'conv64q<{2 * c}, 32 outputs>')
    s = ops.gn_stats_reduce(stats, B, 8).cpu()
    yg = ref.reshape(B, -1, 8, 4)
    np.testing.assert_allclose(s[..., 0], yg.sum(dim=(1, 3)), rtol=2e-3, atol=5.0)
    np.testing.assert_allclose(s[..., 1], (yg * yg).sum(dim=(1, 3)), rtol=2e-3)
    _check_stats(stats, B, ref, R.conv_1kk(_bf16r(torch.cat((xa, xb), -1)), _bf16r(kern), bias), f'conv64q<{2 * c}, 32 outputs>')


IGEMM, WS3 = 'conv_igemm_kernel', 'conv3x3_ws_kernel'

WS_CASES = [
    # B, F, S, C0, C1, Cout            (3x3, stride 1, bf16 tensors, Cout % 128 == 0; conv3x3_ws_kernel needs >= 128 work items = tiles x
    #                                   128-wide output-channel tiles, a tile being 16 x 16 pixels, one 16 x 16 frame or four 8 x 8 frames)
    (2, 16, 32, 128, 0, 128),          # level-1 shape: 16 x 16 tiles of a 32 x 32 frame, one output-channel tile
    (5, 16, 32, 64, 0, 128),           # 320 tiles over 256 ranges: ragged ranges, one K chunk
    (4, 16, 16, 128, 128, 256),        # level-2 shape with a two-pointer concat input, two output-channel tiles per range
    (8, 16, 8, 512, 0, 512),           # level-3 / mid shape: four whole 8 x 8 frames per tile, four output-channel tiles, ring of 3
    (8, 8, 8, 256, 0, 128),            # F = 8: 16 tiles x 1 channel tile < 128 work items -> both convs run the GENERIC kernel
    (16, 16, 8, 512, 512, 256),        # ups.0 block1: 1024 -> 256 on a concat input, two output-channel tiles, 16 K chunks
    (22, 10, 8, 256, 0, 256),          # F = 10 (config_v2_2 as written) at 8 x 8: per-sample tiles of 4, 4 and 2 frames (the last one partly filled)
    (6, 6, 16, 128, 0, 256),           # 36 tiles x 2 channel tiles < 128 work items -> both convs run the GENERIC kernel
    (4, 16, 16, 128, 0, 256),          # 16 x 16, one tensor: <16, false>, and 64 tiles x 2 channel tiles for the prologue form <16, true>
    (11, 6, 16, 128, 0, 256),          # F = 6 at 16 x 16: one frame per tile, 66 tiles x 2 = 132 work items over 128 ranges (ragged), both forms
    (16, 16, 8, 128, 0, 256),          # 8 x 8: 64 tiles x 2 channel tiles: <8, false> and the prologue form <8, true>
    (2, 16, 32, 64, 64, 128),          # 32 x 32 with a two-pointer concat input: <0, false> concat
]
# Output channels of the second (fused-prologue) conv: 128 = one output-channel tile unless stated.  With one tile the 16 x 16 and 8 x 8
# rows of the table above stay below 128 work items and their second conv runs the generic kernel (the kernels each row reaches:
# WS_KERNELS, asserted against the CPU routing by tests/test_host_parity_routes.py).
WS_SECOND = {(4, 16, 16, 128, 0, 256): 256, (11, 6, 16, 128, 0, 256): 256, (16, 16, 8, 128, 0, 256): 256}
WS_KERNELS = {     # (plain form, prologue form) where not conv3x3_ws_kernel twice
    (4, 16, 16, 128, 128, 256): (WS3, IGEMM), (8, 16, 8, 512, 0, 512): (WS3, IGEMM), (8, 8, 8, 256, 0, 128): (IGEMM, IGEMM),
    (16, 16, 8, 512, 512, 256): (WS3, IGEMM), (22, 10, 8, 256, 0, 256): (WS3, IGEMM), (6, 6, 16, 128, 0, 256): (IGEMM, IGEMM),
}


@pytest.mark.parametrize('case', WS_CASES)
@pytest.mark.parametrize('y_bf16', [True, False])
def test_weight_streaming_conv(case, y_bf16):
    """conv3x3_ws_kernel (conv_ws.hip): persistent weight-streaming 3x3 conv of the wide levels.  Plain form (bias + statistics
    epilogue, samples of different scale so the per-sample statistics flush is visible), then the fused-prologue form
    (GroupNorm-apply * (scale + 1) + shift -> SiLU, per-sample coefficients) consuming its output.  Which rows reach the kernel and in
    which instantiation (<0 | 16 | 8, prologue>: 16 x 16 tiles of larger frames, whole 16 x 16 frames, four 8 x 8 frames) is WS_KERNELS
    and tests/golden/parity_routes.json; the rows below the threshold of 128 work items run conv_igemm_kernel on bf16 tensors, held to the
    same bounds."""
    from video_diffusion_nnx_amd import ops
    dev = torch.device('cuda:0')
    B, Fr, S, C0, C1, Cout = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, Fr, S, S, C0 + C1, generator=g)
    x *= (1.0 + 0.25 * torch.arange(B).float()).view(B, 1, 1, 1, 1)
    kern = torch.randn(1, 3, 3, C0 + C1, Cout, generator=g) / (9 * (C0 + C1)) ** 0.5
    bias = torch.randn(Cout, generator=g)
    pw = ops.pack_conv_weights(kern.to(dev), 'bf16')
    stats1 = ops.gn_stats_zeros(B, 8, dev)
    xd = x.to(dev).to(torch.bfloat16)
    x0, x1 = (xd[..., :C0].contiguous(), xd[..., C0:].contiguous()) if C1 else (xd, None)
    with PR.bound(PR.cid('ws', case, y_bf16, 'plain')):
        y1 = ops.conv_forward(x0, pw, Cout, mode='bf16', bias=bias.to(dev), x1=x1, out_stats=stats1, y_bf16=y_bf16)
    torch.cuda.synchronize()
    ref1 = R.conv_1kk(_bf16r(x).double(), _bf16r(kern).double(), bias.double())
    y1f = y1.float().cpu().double()
    r1 = _rel(y1f, ref1)
    assert r1 < (4e-3 if y_bf16 else 2e-6), r1               # exact bf16 products, fp32 accumulate (+ one output rounding)
    if y_bf16:
        P.assert_bf16_store(y1.cpu(), ref1, P.FWD_STATED, f'conv3x3_ws {case}')
    s = ops.gn_stats_reduce(stats1, B, 8).cpu()
    yg = ref1.reshape(B, -1, 8, Cout // 8)
    np.testing.assert_allclose(s[..., 0], yg.sum(dim=(1, 3)), rtol=2e-3, atol=5.0)     # statistics are taken before the output rounding
    np.testing.assert_allclose(s[..., 1], (yg * yg).sum(dim=(1, 3)), rtol=2e-3)
    _check_stats(stats1, B, ref1, R.conv_1kk(_bf16r(x), _bf16r(kern), bias), f'conv3x3_ws {case} y_bf16={y_bf16}')
    if not y_bf16:
        return                                               # the prologue form needs bf16 input tensors
    gamma, beta = 1 + 0.1 * torch.randn(Cout, generator=g), 0.1 * torch.randn(Cout, generator=g)
    ss = torch.randn(B, 2 * Cout, generator=g) * 0.3
    Cout2 = WS_SECOND.get(case, 128)
    kern2 = torch.randn(1, 3, 3, Cout, Cout2, generator=g) / (9 * Cout) ** 0.5
    pw2 = ops.pack_conv_weights(kern2.to(dev), 'bf16')
    for use_ss in (True, False):
        stats2 = ops.gn_stats_zeros(B, 8, dev)
        with PR.bound(PR.cid('ws', case, 'prologue', use_ss)):
            y2 = ops.conv_forward(y1, pw2, Cout2, mode='bf16', in_stats=stats1, gamma=gamma.to(dev), beta=beta.to(dev),
                                  scale_shift=ss.to(dev) if use_ss else None, out_stats=stats2, y_bf16=True)
        h = R.group_norm(y1f, gamma.double(), beta.double(), 8)
        if use_ss:
            h = h * (ss[:, None, None, None, :Cout].double() + 1) + ss[:, None, None, None, Cout:].double()
        ref2 = R.conv_1kk(_bf16r(R.silu(h).float()).double(), _bf16r(kern2).double(), None)
        r2 = _rel(y2.float().cpu().double(), ref2)
        assert r2 < 5e-3, (use_ss, r2)
        _check_prologue_conv(lambda slab: ops.conv_forward(y1, pw2, Cout2, mode='bf16', in_stats=slab, gamma=gamma.to(dev), beta=beta.to(dev),
                                                           scale_shift=ss.to(dev) if use_ss else None, out_stats=ops.gn_stats_zeros(B, 8, dev), y_bf16=True),
                             y1f, gamma, beta, ss if use_ss else None, kern2, ref2, stats1, True, f'conv3x3_ws {case} use_ss={use_ss}')


@pytest.mark.parametrize('res_bf16', [False, True])
def test_persistent_conv64_with_residual(res_bf16):
    """conv64d_kernel<false, true>: the level-0 3x3 64->64 conv with an fp32 residual added in the epilogue (in training: the data
    gradient of a ResnetBlock's first conv + the gradient of the skip path), 1024 tiles = the persistent form's threshold; the plain
    form it is compared with is conv64r_kernel.  (A bf16 residual takes the generic kernel: same check.)"""
    from video_diffusion_nnx_amd import ops
    dev = torch.device('cuda:0')
    B, Fr, S, C = 4, 16, 64, 64
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, Fr, S, S, C, generator=g).to(torch.bfloat16)
    kern = torch.randn(1, 3, 3, C, C, generator=g) / (9 * C) ** 0.5
    bias = torch.randn(C, generator=g)
    res = torch.randn(B, Fr, S, S, C, generator=g)
    if res_bf16:
        res = res.to(torch.bfloat16)
    pw = ops.pack_conv_weights(kern.to(dev), 'bf16')
    with PR.bound(PR.cid('c64 res', res_bf16)):
        y = ops.conv_forward(x.to(dev), pw, C, mode='bf16', bias=bias.to(dev), res=res.to(dev), y_bf16=False)
    with PR.bound(PR.cid('c64 res', 'plain')):
        y0 = ops.conv_forward(x.to(dev), pw, C, mode='bf16', bias=bias.to(dev), y_bf16=False)
    torch.cuda.synchronize()
    # the plain persistent form is checked against the oracle elsewhere in this file; here: residual form == plain form + res
    np.testing.assert_allclose((y - y0).cpu().numpy(), res.float().numpy(), atol=2e-5 * float(y0.abs().max()))
    ref = R.conv_1kk(x[:1].float().double(), _bf16r(kern).double(), bias.double()) + res[:1].double()
    assert _rel(y[:1].cpu().double(), ref) < 2e-6


PW_CASES = [
    # B, F, S, C0, C1, Cout, res      (1x1, bf16 tensors, Cin % 128 == 0, Cout % 64 == 0 and >= 128, >= 8192 pixels)
    (8, 16, 8, 256, 0, 512, False),    # downs.3.0 res_conv: 128-row tiles, 2 K blocks
    (8, 16, 8, 512, 512, 256, False),  # ups.0.0 res_conv on a concat: 64-row tiles (Cin = 1024), two-pointer K blocks
    (2, 16, 16, 256, 256, 128, False), # ups.1.0 res_conv: Cin = 512, one 128-row tile
    (2, 16, 16, 256, 0, 256, True),    # level-2 attention / SLA to_out: + residual
    (9, 16, 8, 256, 0, 512, True),     # level-3 to_out, 9216 pixels: ragged pixel ranges
    (4, 8, 16, 128, 0, 192, True),     # one K block, three 64-row tiles
    (2, 16, 32, 64, 0, 256, False),    # Cin = 64 (one 2-step K block per pixel group): the q / k / v projections the SLA backward recomputes at level 0
    (1, 9, 32, 64, 0, 192, False),     # Cin = 64, 64-row tiles, 288 pixel groups (ragged ranges)
    (1, 16, 32, 64, 0, 768, True),     # Cin = 64, six 128-row tiles, + residual
]

PW32_CASES = [
    # B, F, S, Cin, Cout, res      (1x1, bf16 x, fp32 y and res: the dx projections of the attention / SLA backward)
    (1, 16, 32, 768, 64, True),        # level 0: dq|dk|dv . [Wq;Wk;Wv]^T + g, one 64-row tile
    (2, 16, 16, 768, 256, True),       # level 2: two 128-row tiles
    (4, 16, 8, 768, 512, True),        # level 3 at 4096 pixels: below the kernel's 8192 -> the GENERIC kernel with bf16 input and fp32 output
    (2, 8, 32, 256, 128, False),       # no residual
]


PW32_KERNELS = {(4, 16, 8, 768, 512, True): IGEMM}        # where not conv1x1_pw_kernel


@pytest.mark.parametrize('case', PW_CASES)
def test_pointwise_conv_bf16(case):
    """conv1x1_pw_kernel (conv_pw.hip): the 1x1 convs of the wide levels on bf16 tensors -- weight rows resident in LDS, x rows straight
    from global memory into MFMA fragments, permuted output rows, optional residual.  Reference: fp64 matmul of the bf16-rounded
    operands; one output rounding to bf16."""
    from video_diffusion_nnx_amd import ops
    dev = torch.device('cuda:0')
    B, Fr, S, C0, C1, Cout, with_res = case
    g = torch.Generator().manual_seed(sum(case[:6]))
    bf = torch.bfloat16
    x = torch.randn(B, Fr, S, S, C0 + C1, generator=g).to(bf)
    kern = torch.randn(1, C0 + C1, Cout, generator=g) / (C0 + C1) ** 0.5
    bias = torch.randn(Cout, generator=g)
    res = torch.randn(B, Fr, S, S, Cout, generator=g).to(bf) if with_res else None
    pw = ops.pack_conv_weights(kern.to(dev), 'bf16')
    xd = x.to(dev)
    kw = dict(mode='bf16', bias=bias.to(dev), k=1, y_bf16=True, res=None if res is None else res.to(dev))
    with PR.bound(PR.cid('pw', case)):
        if C1:
            y = ops.conv_forward(xd[..., :C0].contiguous(), pw, Cout, x1=xd[..., C0:].contiguous(), **kw)
        else:
            y = ops.conv_forward(xd, pw, Cout, **kw)
    torch.cuda.synchronize()
    ref = x.double() @ _bf16r(kern[0]).double() + bias.double()
    if with_res:
        ref = ref + res.double()
    assert y.dtype == bf
    assert _rel(y.float().cpu().double(), ref) < 4e-3
    assert (y.float().cpu().double() - ref).abs().max() < 2e-2 * ref.abs().max()
    P.assert_bf16_store(y.cpu(), ref, P.FWD_STATED, f'conv1x1_pw {case}')


@pytest.mark.parametrize('case', PW32_CASES)
def test_pointwise_conv_bf16_in_fp32_out(case):
    """conv1x1_pw_kernel<ROWS, 4, OUT32>: bf16 input rows, fp32 output (+ fp32 residual) -- how the backward's dx projections run."""
    from video_diffusion_nnx_amd import ops
    dev = torch.device('cuda:0')
    B, Fr, S, Cin, Cout, with_res = case
    g = torch.Generator().manual_seed(sum(case[:5]))
    x = torch.randn(B, Fr, S, S, Cin, generator=g).to(torch.bfloat16)
    kern = torch.randn(1, Cin, Cout, generator=g) / Cin ** 0.5
    bias = torch.randn(Cout, generator=g)
    res = torch.randn(B, Fr, S, S, Cout, generator=g) if with_res else None
    pw = ops.pack_conv_weights(kern.to(dev), 'bf16')
    with PR.bound(PR.cid('pw32', case)):
        y = ops.conv_forward(x.to(dev), pw, Cout, mode='bf16', bias=bias.to(dev), k=1, y_bf16=False, res=None if res is None else res.to(dev))
    torch.cuda.synchronize()
    ref = x.double() @ _bf16r(kern[0]).double() + bias.double()
    if with_res:
        ref = ref + res.double()
    assert y.dtype == torch.float32
    assert _rel(y.cpu().double(), ref) < 3e-6                       # fp32 accumulation of exact bf16 products, no output rounding


WS4_CASES = [
    # kind (0 = Downsample 4x4 / stride 2, 1 = Upsample ConvTranspose), B, F, S_in, C, Cout   (bf16 tensors; >= 128 work items)
    (0, 8, 16, 32, 128, 128),          # level-1 Downsample: 32 -> 16, whole 16 x 16 output frames, 2 K chunks per parity plane
    (0, 16, 16, 16, 256, 256),         # level-2 Downsample: 16 -> 8, four 8 x 8 output frames per tile, two output-channel tiles
    (0, 52, 10, 16, 64, 128),          # one K chunk per plane, F = 10: 130 tiles over 128 ranges (ragged)
    (1, 8, 16, 8, 256, 256),           # level-3 -> 2 Upsample: 8 -> 16, four input frames per tile x 4 phases
    (1, 4, 16, 16, 128, 128),          # level-2 -> 1 Upsample: 16 -> 32
    (1, 11, 12, 8, 64, 128),           # 33 input tiles x 4 phases over 128 ranges (ragged, ranges of whole phase groups)
    (0, 4, 16, 64, 64, 64),            # level-0 Downsample: 64 -> 32, bands of 8 x 32 output pixels, 64-channel output tile
    (1, 2, 16, 32, 64, 64),            # level-1 -> 0 Upsample: 32 -> 64, bands of 8 x 32 input pixels x 4 phases
    (0, 3, 12, 64, 128, 128),          # bands with a 128-channel output tile, 2 K chunks per plane, 144 tiles (ragged)
    (1, 8, 16, 16, 128, 64),           # whole 16 x 16 frames with a 64-channel output tile
    (0, 3, 10, 64, 32, 32),            # resample32_kernel (dim-32 networks, level 0): Downsample 64 -> 32, everything in registers
    (1, 3, 10, 32, 32, 32),            # resample32_kernel: Upsample 32 -> 64 (four output phases from the 3 x 3 neighbourhood)
    (0, 1, 3, 32, 32, 32),             # ragged: 48 tiles over 48 waves
    (1, 1, 3, 16, 32, 32),
    (0, 8, 16, 32, 64, 64),            # level-1 Downsample of dim-32 networks: 32 -> 16, whole 16 x 16 output frames with a 64-channel output tile
    (1, 2, 16, 32, 128, 128),          # Upsample 32 -> 64 at 128 channels (the dim-128 configuration): bands of 8 x 32 input pixels, 128-channel output tile
]


def ws4_kernel(case, y_bf16):
    """The kernel a row of WS4_CASES reaches: resample32_kernel writes bf16 only, so the 32-channel rows with an fp32 output run the
    generic kernel (on bf16 input)."""
    return ('resample32_kernel' if y_bf16 else IGEMM) if case[4] == 32 else 'conv4x4_ws_kernel'


@pytest.mark.parametrize('case', WS4_CASES)
@pytest.mark.parametrize('y_bf16', [True, False])
def test_weight_streaming_resampling_conv(case, y_bf16):
    """conv4x4_ws_kernel (conv_ws.hip): Downsample / Upsample of the wide levels on the weight-streaming machinery (parity planes /
    output phases of 2 x 2 taps), and resample32_kernel (conv_rs.hip) for the 32-channel rows (ws4_kernel); reference utils.py:103-125 through the oracle's conv_1kk(stride 2) / conv_transpose_144."""
    from video_diffusion_nnx_amd import ops
    dev = torch.device('cuda:0')
    kind, B, Fr, S, C, Cout = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, Fr, S, S, C, generator=g)
    kern = torch.randn(1, 4, 4, C, Cout, generator=g) / (8 * C) ** 0.5
    bias = torch.randn(Cout, generator=g)
    pw = ops.pack_conv_weights(kern.to(dev), 'bf16')
    xd = x.to(dev).to(torch.bfloat16)
    if kind == 1:
        with PR.bound(PR.cid('ws4', case, y_bf16)):
            y = ops.conv_forward(xd, pw, Cout, mode='bf16', bias=bias.to(dev), kind=1, k=4, y_bf16=y_bf16)
        ref = R.conv_transpose_144(_bf16r(x).double(), _bf16r(kern).double(), bias.double())
    else:
        with PR.bound(PR.cid('ws4', case, y_bf16)):
            y = ops.conv_forward(xd, pw, Cout, mode='bf16', bias=bias.to(dev), k=4, stride=2, y_bf16=y_bf16)
        ref = R.conv_1kk(_bf16r(x).double(), _bf16r(kern).double(), bias.double(), stride=2)
    torch.cuda.synchronize()
    assert tuple(y.shape) == tuple(ref.shape)
    r = _rel(y.float().cpu().double(), ref)
    assert r < (4e-3 if y_bf16 else 2e-6), r
    if y_bf16:
        P.assert_bf16_store(y.cpu(), ref, P.FWD_STATED, f'conv4x4_ws {case}')


C32_CASES = [(32, 2, 32, 64), (32, 3, 22, 64)]                  # c, B, F, S


@pytest.mark.parametrize('c,B,Fr,S', C32_CASES)
def test_persistent_c32_conv(c, B, Fr, S):
    """conv64p_kernel<.., C 32>: the 3x3 32 -> 32 convs of level 0 of dim-32 networks on bf16 tensors (weights resident in LDS, >= 1024
    tiles of 16 x 16 pixels): plain form with statistics, then the fused-prologue form consuming it, with and without scale / shift,
    producer slab and hand-made slab.  (2, 32): 1024 tiles, the threshold.  (3, 22): 1056 tiles -- the plain form walks 3 per workgroup
    (512 workgroup slots), the prologue form 5 (256 slots), so workgroups 117 (plain) and 70 (prologue) walk ACROSS the sample boundary
    at tile 352: the per-sample flush of the register-resident statistics and the coefficient switch inside one workgroup's walk."""
    from video_diffusion_nnx_amd import ops
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(19 + B)
    x = torch.randn(B, Fr, S, S, c, generator=g)
    x[1] *= 1.7                                            # different statistics per sample
    if B > 2:
        x[2] = x[2] * 0.6 + 0.4
    kern = torch.randn(1, 3, 3, c, c, generator=g) / (9 * c) ** 0.5
    bias = torch.randn(c, generator=g)
    pw = ops.pack_conv_weights(kern.to(dev), 'bf16')
    stats1 = ops.gn_stats_zeros(B, 8, dev)
    sh = (B, Fr, S, S, c)
    with PR.bound(PR.cid('c32', *sh, 'plain')):
        y1 = ops.conv_forward(x.to(dev).to(torch.bfloat16), pw, c, mode='bf16', bias=bias.to(dev), out_stats=stats1, y_bf16=True)
    torch.cuda.synchronize()
    ref1 = R.conv_1kk(_bf16r(x).double(), _bf16r(kern).double(), bias.double())
    y1f = y1.float().cpu().double()
    P.assert_bf16_store(y1.cpu(), ref1, P.FWD_STATED, f'conv64p C32 B{B} F{Fr}')
    _check_stats(stats1, B, ref1, R.conv_1kk(_bf16r(x), _bf16r(kern), bias), f'conv64p C32 B{B} F{Fr}')
    gamma, beta = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    ss = torch.randn(B, 2 * c, generator=g) * 0.3
    kern2 = torch.randn(1, 3, 3, c, c, generator=g) / (9 * c) ** 0.5
    pw2 = ops.pack_conv_weights(kern2.to(dev), 'bf16')
    for use_ss in (True, False):
        run = lambda slab: ops.conv_forward(y1, pw2, c, mode='bf16', in_stats=slab, gamma=gamma.to(dev), beta=beta.to(dev),
                                            scale_shift=ss.to(dev) if use_ss else None, y_bf16=True)
        with PR.bound(PR.cid('c32', *sh, 'prologue', use_ss)):
            run(stats1)
        h = R.group_norm(y1f, gamma.double(), beta.double(), 8)
        if use_ss:
            h = h * (ss[:, None, None, None, :c].double() + 1) + ss[:, None, None, None, c:].double()
        ref2 = R.conv_1kk(_bf16r(R.silu(h).float()).double(), _bf16r(kern2).double(), None)
        _check_prologue_conv(run, y1f, gamma, beta, ss if use_ss else None, kern2, ref2, stats1, True, f'conv64p C32 B{B} F{Fr} use_ss={use_ss}')


# ---- the generic kernel in the forms the networks reach it in ----------------------------------------------------------------------------
# conv_igemm_kernel "<MODE, BC, 2, waves, INF>": MODE 0 f32 / 1 bf16 / 2 f16 operands, BC = 64 output channels per workgroup up to
# Cout 64, else 128, INF 0 = fp32 input tensors, 2 = bf16 input tensors.  The training forward at B = 4 and every level below the
# thresholds of the persistent kernels run it with a concat input, the fused prologue, stride 2, the ConvTranspose phases and a
# residual; the rows here are the smallest shapes tests/_parity_routes.py routes to each of those forms (odd frame counts, frames that
# are no multiple of the 16 x 16 tile, channel counts that are no multiple of the K tile), and no shape a dedicated kernel takes.
# Inputs are representable in the operand type, so the references are fp64 on the same numbers.

def _rd(mode):
    return (lambda t: t) if mode == 'f32' else P.operand_rounding(mode)


def _check_conv_output(y, ref32, ref64, y16, what):
    """fp32 output: the exact-products contract per (frame, 16 x 16 tile) and globally (stated 2e-6); bf16 output: one rounding of it."""
    if y16:
        P.assert_bf16_store(y.cpu(), ref64, P.FWD_STATED, what)
    else:
        sl = P.tile_slices(ref64.shape)
        bound, sb, floor = P.exact_products_bounds(ref32, ref64, sl, None, P.FWD_STATED)
        P.assert_exact_products(y.cpu(), ref64, bound, sl, sb, None, f'{what} (CPU floor {floor:.1e})')


GENERIC_CHAINS = [
    # mode, bf16 tensors, B, F, H, W, C0, C1, Cout      (3x3 with bias and statistics, then the fused-prologue 3x3 Cout -> Cout on its output.
    #   Whole 16 x 16 frames, several of them: the per-tile bound of the prologue form is 4 x the worst tile of the CPU's own fp32 flips,
    #   and a tile of a few thousand activations holds too few flips for that figure to be stable; ragged frames are in GENERIC_FORMS)
    ('bf16', True, 2, 3, 16, 16, 40, 0, 64),        # <1, 64, 2, 8, 2> conv3x3, then ... +prologue: the N shape's training forward at level 0
    ('bf16', True, 2, 3, 16, 16, 40, 24, 64),       # <1, 64, 2, 8, 2> conv3x3 concat (ups.2.0.conv1 of the N shape when sampling)
    ('bf16', True, 2, 3, 16, 16, 40, 32, 72),       # <1, 128, 2, 8, 2> conv3x3 concat
    ('bf16', False, 2, 3, 16, 16, 24, 16, 72),       # <1, 128, 2, 8, 0> conv3x3 concat: fp32 tensors in bf16 mode
    ('f32', False, 2, 3, 16, 16, 24, 0, 72),        # <0, 128, 2, 8, 0> ... +prologue
]


def _conv_chain(mode, t16, B, Fr, H, W, C0, C1, Cout, table, prologue_ceiling):
    from video_diffusion_nnx_amd import ops
    dev = torch.device('cuda:0')
    case = (B, Fr, H, W, C0, C1, Cout)
    what = f'{table} {mode} bf16 tensors={int(t16)} {case}'
    rd, st = _rd(mode), (lambda t: t.to(dev).to(torch.bfloat16) if t16 else t.to(dev))
    g = torch.Generator().manual_seed(sum(case) + len(mode))
    x = torch.randn(B, Fr, H, W, C0 + C1, generator=g)
    x *= (1.0 + 0.25 * torch.arange(B).float()).view(B, 1, 1, 1, 1)          # samples of different scale
    x = P.bf16r(x) if t16 else rd(x)
    kern = rd(torch.randn(1, 3, 3, C0 + C1, Cout, generator=g) / (9 * (C0 + C1)) ** 0.5)
    bias = torch.randn(Cout, generator=g)
    pw = ops.pack_conv_weights(kern.to(dev), mode)
    stats1 = ops.gn_stats_zeros(B, 8, dev)
    with PR.bound(PR.cid(table, mode, t16, case, 'plain')):
        y1 = ops.conv_forward(st(x[..., :C0].contiguous()), pw, Cout, mode=mode, bias=bias.to(dev), x1=st(x[..., C0:].contiguous()) if C1 else None,
                              out_stats=stats1, y_bf16=t16)
    torch.cuda.synchronize()
    ref1, ref1_32 = R.conv_1kk(x.double(), kern.double(), bias.double()), R.conv_1kk(x, kern, bias)
    _check_conv_output(y1, ref1_32, ref1, t16, what)
    P.assert_gn_stats(ops.gn_stats_reduce(stats1, B, 8).cpu(), ref1, ref1_32, -(-H * W // 256) * Fr, what=what)
    y1f = y1.float().cpu().double()
    gamma, beta = 1 + 0.1 * torch.randn(Cout, generator=g), 0.1 * torch.randn(Cout, generator=g)
    ss = torch.randn(B, 2 * Cout, generator=g) * 0.3
    kern2 = rd(torch.randn(1, 3, 3, Cout, Cout, generator=g) / (9 * Cout) ** 0.5)
    pw2 = ops.pack_conv_weights(kern2.to(dev), mode)
    hand = P.spread_slots(P.gn_stats_slab(y1f), seed=Cout).reshape(-1).to(dev)
    for use_ss in (True, False):
        def act(dt):
            h = R.group_norm(y1f.to(dt), gamma.to(dt), beta.to(dt), 8)
            if use_ss:
                h = h * (ss.to(dt)[:, None, None, None, :Cout] + 1) + ss.to(dt)[:, None, None, None, Cout:]
            return rd(R.silu(h)).double()
        out_of = lambda a: R.conv_1kk(a, kern2.double(), None)
        if mode == 'f32':                     # no rounding of the activation: the norm chain and the conv in fp32 against fp64, per tile
            ref2, ref2_32 = out_of(act(torch.float64)), R.conv_1kk(act(torch.float32).float(), kern2, None)
        else:
            bound, floor = P.tile_bound(act(torch.float32), act(torch.float64), out_of, bf16_out=t16, operand='f16' if mode == 'f16' else 'bf16')
            print(f'[prologue {what} use_ss={use_ss}] flip floor {floor:.3e} -> per-tile bound {bound:.3e}')
            assert bound < prologue_ceiling, f'a derived bound above {prologue_ceiling:.1e} would be a finding'
            ref2 = out_of(act(torch.float64))
        for label, slab in (('producer slab', stats1), ('hand-made slab', hand)):
            with PR.bound(PR.cid(table, mode, t16, case, 'prologue', use_ss)):
                y2 = ops.conv_forward(y1, pw2, Cout, mode=mode, in_stats=slab, gamma=gamma.to(dev), beta=beta.to(dev),
                                      scale_shift=ss.to(dev) if use_ss else None, out_stats=ops.gn_stats_zeros(B, 8, dev), y_bf16=t16)
            torch.cuda.synchronize()
            if mode == 'f32':
                _check_conv_output(y2, ref2_32, ref2, False, f'{what} prologue use_ss={use_ss}, {label}')
            else:
                P.assert_tiles(y2.float().cpu(), ref2, bound, what=f'{what} prologue use_ss={use_ss}, {label}')


@pytest.mark.parametrize('mode,t16,B,Fr,H,W,C0,C1,Cout', GENERIC_CHAINS)
def test_generic_conv_chain(mode, t16, B, Fr, H, W, C0, C1, Cout):
    """conv_igemm_kernel, plain form with a (concat) input and the statistics epilogue, then the fused-prologue form consuming it: the
    bounds of test_weight_streaming_conv (bf16 store / exact products, assert_gn_stats, tile_bound with producer and hand-made slab;
    f32 mode rounds nothing, so its prologue form is held to the exact-products rule against the same chain in fp64)."""
    _conv_chain(mode, t16, B, Fr, H, W, C0, C1, Cout, 'generic chain', 5e-3)


GENERIC_FORMS = [
    # mode, bf16 tensors, B, F, H, W, C0, C1, Cout, k, stride, kind, res (None | 'f32' | 'bf16')
    ('f32', False, 1, 3, 6, 10, 24, 16, 40, 1, 1, 0, None),        # <0, 64, 2, 8, 0> conv1x1 concat: a res_conv on the skip concat
    ('bf16', False, 1, 3, 6, 10, 24, 16, 40, 1, 1, 0, None),       # <1, 64, 2, 8, 0> conv1x1 concat
    ('bf16', False, 1, 3, 6, 10, 24, 24, 72, 1, 1, 0, None),       # <1, 128, 2, 8, 0> conv1x1 concat
    ('bf16', False, 1, 3, 6, 10, 48, 0, 72, 1, 1, 0, 'f32'),       # <1, 128, 2, 8, 0> conv1x1 +res: the out-projection of the long attention
    ('bf16', False, 1, 3, 12, 20, 40, 0, 72, 4, 2, 0, None),       # <1, 128, 2, 8, 0> conv4x4 s2
    ('bf16', True, 1, 3, 6, 10, 40, 0, 64, 1, 1, 0, None),         # <1, 64, 2, 8, 2> conv1x1
    ('bf16', True, 1, 3, 6, 10, 40, 24, 64, 1, 1, 0, None),        # <1, 64, 2, 8, 2> conv1x1 concat
    ('bf16', True, 1, 3, 6, 10, 40, 32, 72, 1, 1, 0, None),        # <1, 128, 2, 8, 2> conv1x1 concat
    ('bf16', True, 1, 3, 12, 20, 72, 0, 72, 4, 2, 0, None),        # <1, 128, 2, 8, 2> conv4x4 s2
    ('bf16', True, 1, 3, 6, 10, 72, 0, 72, 4, 1, 1, None),         # <1, 128, 2, 8, 2> convT4x4
]


def _conv_form(mode, t16, B, Fr, H, W, C0, C1, Cout, k, stride, kind, res, table):
    from video_diffusion_nnx_amd import ops
    dev = torch.device('cuda:0')
    case = (B, Fr, H, W, C0, C1, Cout, k, stride, kind, res)
    what = f'{table} {mode} bf16 tensors={int(t16)} {case}'
    rd, st = _rd(mode), (lambda t: t.to(dev).to(torch.bfloat16) if t16 else t.to(dev))
    g = torch.Generator().manual_seed(sum(case[:10]) + len(mode))
    x = torch.randn(B, Fr, H, W, C0 + C1, generator=g)
    x = P.bf16r(x) if t16 else rd(x)
    kern = rd(torch.randn(1, k, k, C0 + C1, Cout, generator=g) / (k * k * (C0 + C1)) ** 0.5)
    bias = torch.randn(Cout, generator=g)

    def fwd(dt):
        xx, kk, bb = x.to(dt), kern.to(dt), bias.to(dt)
        return R.conv_transpose_144(xx, kk, bb) if kind == 1 else R.conv_pointwise(xx, kk[0], bb) if k == 1 else R.conv_1kk(xx, kk, bb, stride=stride)
    ref64, ref32 = fwd(torch.float64), fwd(torch.float32)
    r = None
    if res:
        r = torch.randn(ref64.shape, generator=g)
        r = P.bf16r(r) if res == 'bf16' else r
        ref64, ref32 = ref64 + r.double(), ref32 + r
        r = r.to(dev).to(torch.bfloat16) if res == 'bf16' else r.to(dev)
    pw = ops.pack_conv_weights(kern.to(dev), mode)
    with PR.bound(PR.cid(table, mode, t16, case)):
        y = ops.conv_forward(st(x[..., :C0].contiguous()), pw, Cout, mode=mode, bias=bias.to(dev), x1=st(x[..., C0:].contiguous()) if C1 else None,
                             kind=kind, k=k, stride=stride, y_bf16=t16, res=r)
    torch.cuda.synchronize()
    assert tuple(y.shape) == tuple(ref64.shape)
    _check_conv_output(y, ref32, ref64, t16, what)


@pytest.mark.parametrize('mode,t16,B,Fr,H,W,C0,C1,Cout,k,stride,kind,res', GENERIC_FORMS)
def test_generic_conv_form(mode, t16, B, Fr, H, W, C0, C1, Cout, k, stride, kind, res):
    """conv_igemm_kernel: pointwise on a concat input, pointwise with a residual, Downsample and Upsample, on fp32 and on bf16 tensors."""
    _conv_form(mode, t16, B, Fr, H, W, C0, C1, Cout, k, stride, kind, res, 'generic form')
