"""GPU parity of conv3x3_ws_kernel (conv_ws.hip) at the boundaries of its operand pipeline: the smallest shapes that still pass
conv3x3_ws_plan (tiles x Cout / 128 >= 128) and cross the weight ring's wrap, a tile epilogue inside a workgroup's range, a partly
filled last tile, a slab count per tile that is no multiple of the ring depth, and the tiled (halo) geometry on a concat input.

Driven through ops.conv_forward like tests/test_gpu_conv.py::test_weight_streaming_conv, against the same reference (oracle conv_1kk in
fp64 on bf16-rounded operands) and the same bounds; the helpers are that module's.  The plain forms of two cases are also compared BIT FOR
BIT with the recorded output of an earlier build (tests/golden/ws_pipeline_*.npz: sha256 + one checksum per pixel row, written by
tools/ws_pipeline_golden.py from the commit before the tap loop was last changed):
the MFMA order of every accumulator (K chunk, tap, K step 0, K step 1) is part of the kernel's contract."""
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _parity as P
from _launch_hook import launches
from oracle import unet3d_ref as R

WS3 = 'conv3x3_ws_kernel'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# name -> (B, F, S, C0, C1, Cout)
CASES = {
    'w8_one_tile': (128, 4, 8, 128, 0, 128),       # 8 x 8: 128 tiles of 4 frames, one tile per workgroup (18 slabs: the ring wraps inside the tile)
    'w8_256': (256, 4, 8, 128, 0, 128),            # 256 tiles: as many as the chip has compute units (one tile per workgroup there, two on a smaller part)
    'w8_two_tiles': (260, 4, 8, 128, 0, 128),      # 260 tiles > 256 compute units: ranges of TWO tiles, the ring wraps across a tile epilogue (AFTER_EPI waits)
    'w8_f10': (64, 10, 8, 128, 0, 256),            # F = 10: tiles of 4, 4 and 2 frames (a partly filled last tile), two output-channel tiles
    'w16_k3': (8, 16, 16, 192, 0, 128),            # 16 x 16: three K chunks = 27 slabs per tile, no multiple of a ring depth of 4 or 5
    'tiled_concat': (2, 16, 32, 64, 64, 128),      # 32 x 32: 16 x 16 tiles with a halo, two-pointer concat input, 128 tiles (plain form only: the plan's rule)
}
GEO = {8: 8, 16: 16, 32: 0}
BITWISE = ('w8_f10', 'w16_k3')                      # the cases whose plain output is pinned bit for bit (tests/golden/ws_pipeline_<name>.npz)


def inputs(name):
    """-> x [B, F, S, S, C0 + C1] fp32 (samples of different scale), kernel [1, 3, 3, Cin, Cout], bias [Cout]; CPU, seeded by the case"""
    B, Fr, S, C0, C1, Cout = CASES[name]
    g = torch.Generator().manual_seed(sum(CASES[name]))
    x = torch.randn(B, Fr, S, S, C0 + C1, generator=g)
    x *= (1.0 + 0.25 * (torch.arange(B) % 8).float()).view(B, 1, 1, 1, 1)
    kern = torch.randn(1, 3, 3, C0 + C1, Cout, generator=g) / (9 * (C0 + C1)) ** 0.5
    bias = torch.randn(Cout, generator=g)
    return x, kern, bias


def run_plain(name, y_bf16, dev):
    """the plain form with bias and output statistics -> (y, statistics slab, recorded launches)"""
    from video_diffusion_nnx_amd import ops
    B, Fr, S, C0, C1, Cout = CASES[name]
    x, kern, bias = inputs(name)
    pw = ops.pack_conv_weights(kern.to(dev), 'bf16')
    stats = ops.gn_stats_zeros(B, 8, dev)
    xd = x.to(dev).to(torch.bfloat16)
    x0, x1 = (xd[..., :C0].contiguous(), xd[..., C0:].contiguous()) if C1 else (xd, None)
    with launches() as rec:
        y = ops.conv_forward(x0, pw, Cout, mode='bf16', bias=bias.to(dev), x1=x1, out_stats=stats, y_bf16=y_bf16)
    torch.cuda.synchronize()
    return y, stats, rec


def digest(y):
    """-> (sha256 of the tensor's bytes, one uint32 checksum per pixel row: position-weighted sum of the elements' bit patterns)"""
    y = y.detach().cpu().contiguous()
    bits = y.view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32).reshape(-1, y.shape[-1]).to(torch.int64)
    bits &= 0xFFFF if y.dtype == torch.bfloat16 else 0xFFFFFFFF
    w = torch.arange(1, y.shape[-1] + 1, dtype=torch.int64)
    rows = ((bits * w).sum(dim=1) & 0xFFFFFFFF).numpy().astype(np.uint32)
    return hashlib.sha256(bits.numpy().astype(np.uint16 if y.dtype == torch.bfloat16 else np.uint32).tobytes()).hexdigest(), rows


_REF = {}


def _ref(name):
    """the fp64 reference of the plain conv and its fp32 evaluation, computed once per case and left unchanged"""
    if name not in _REF:
        x, kern, bias = inputs(name)
        _REF[name] = (R.conv_1kk(P.bf16r(x).double(), P.bf16r(kern).double(), bias.double()), R.conv_1kk(P.bf16r(x), P.bf16r(kern), bias))
    return _REF[name]


def _assert_route(rec, name, pro):
    assert len(rec) >= 1 and rec[0][0] == WS3, rec
    label = f'<{GEO[CASES[name][2]]}, {"true" if pro else "false"}>'
    assert rec[0][1].startswith(label), (rec[0], label)


@pytest.mark.parametrize('y_bf16', [True, False])
@pytest.mark.parametrize('name', list(CASES))
def test_ws_pipeline_plain(name, y_bf16):
    """plain form: y against the fp64 reference (exact bf16 products, fp32 accumulation, + one output rounding for bf16 y), the
    statistics epilogue, and for the BITWISE cases equality with the recorded output of the earlier build"""
    import test_gpu_conv as T
    from video_diffusion_nnx_amd import ops
    dev = torch.device('cuda:0')
    B, Fr, S, C0, C1, Cout = CASES[name]
    y, stats, rec = run_plain(name, y_bf16, dev)
    _assert_route(rec, name, False)
    ref64, ref32 = _ref(name)
    r1 = T._rel(y.float().cpu().double(), ref64)
    print(f'[ws pipeline] {name} y_bf16={y_bf16}: rel-L2 {r1:.3e}')
    assert r1 < (4e-3 if y_bf16 else 2e-6), r1
    if y_bf16:
        P.assert_bf16_store(y.cpu(), ref64, P.FWD_STATED, f'conv3x3_ws {name}')
    s = ops.gn_stats_reduce(stats, B, 8).cpu()
    yg = ref64.reshape(B, -1, 8, Cout // 8)
    np.testing.assert_allclose(s[..., 0], yg.sum(dim=(1, 3)), rtol=2e-3, atol=5.0)
    np.testing.assert_allclose(s[..., 1], (yg * yg).sum(dim=(1, 3)), rtol=2e-3)
    T._check_stats(stats, B, ref64, ref32, f'conv3x3_ws {name} y_bf16={y_bf16}')
    if name in BITWISE:
        gold = np.load(os.path.join(GOLDEN, f'ws_pipeline_{name}.npz'))
        key = 'bf16' if y_bf16 else 'f32'
        sha, rows = digest(y)
        bad = np.nonzero(rows != gold[f'rows_{key}'])[0]
        assert bad.size == 0, f'{name} {key}: {bad.size} pixel rows differ from the recorded output, first {bad[:8]}'
        assert sha == str(gold[f'sha_{key}']), f'{name} {key}: the output differs from the recorded one (sha256)'


@pytest.mark.parametrize('name', [n for n in CASES if CASES[n][4] == 0])
def test_ws_pipeline_prologue(name):
    """fused-prologue form (GroupNorm-apply * (scale + 1) + shift -> SiLU on the input, per-sample coefficients) on the SAME shape, bf16
    y, output statistics on: the input is the case's bf16 tensor, its statistics slab is made by hand (everything in slot 0, then spread
    over the slots by _check_prologue_conv)"""
    import test_gpu_conv as T
    from video_diffusion_nnx_amd import ops
    dev = torch.device('cuda:0')
    B, Fr, S, C0, C1, Cout = CASES[name]
    x, kern, _ = inputs(name)
    g = torch.Generator().manual_seed(1 + sum(CASES[name]))
    gamma, beta = 1 + 0.1 * torch.randn(C0, generator=g), 0.1 * torch.randn(C0, generator=g)
    ss = torch.randn(B, 2 * C0, generator=g) * 0.3
    xb = x.to(torch.bfloat16)
    xf = xb.float().double()
    xd = xb.to(dev)
    pw = ops.pack_conv_weights(kern.to(dev), 'bf16')
    slab = P.gn_stats_slab(xf).reshape(-1).to(dev)
    h = R.group_norm(xf, gamma.double(), beta.double(), 8)
    h = h * (ss[:, None, None, None, :C0].double() + 1) + ss[:, None, None, None, C0:].double()
    ref2 = R.conv_1kk(P.bf16r(R.silu(h).float()).double(), P.bf16r(kern).double(), None)

    def run(in_stats, out_stats):
        return ops.conv_forward(xd, pw, Cout, mode='bf16', in_stats=in_stats, gamma=gamma.to(dev), beta=beta.to(dev), scale_shift=ss.to(dev),
                                out_stats=out_stats, y_bf16=True)

    stats2 = ops.gn_stats_zeros(B, 8, dev)
    with launches() as rec:
        y2 = run(slab, stats2)
    torch.cuda.synchronize()
    _assert_route(rec, name, True)
    r2 = T._rel(y2.float().cpu().double(), ref2)
    print(f'[ws pipeline] {name} prologue: rel-L2 {r2:.3e}')
    assert r2 < 5e-3, r2
    s = ops.gn_stats_reduce(stats2, B, 8).cpu()
    yg = ref2.reshape(B, -1, 8, Cout // 8)
    np.testing.assert_allclose(s[..., 0], yg.sum(dim=(1, 3)), rtol=2e-3, atol=5.0)
    np.testing.assert_allclose(s[..., 1], (yg * yg).sum(dim=(1, 3)), rtol=2e-3)
    T._check_prologue_conv(lambda sl: run(sl, ops.gn_stats_zeros(B, 8, dev)), xf, gamma, beta, ss, kern, ref2, slab, True,
                           f'conv3x3_ws pipeline {name}')
