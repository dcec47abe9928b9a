"""GPU parity of the non-conv UNet blocks (through the C ABI) vs oracle/unet3d_ref.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _parity as P
import _parity_routes as PR
from oracle import unet3d_ref as R

DEV = 'cuda:0'


def _rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


TOL = {'f32': 2e-5, 'bf16': 1.5e-2}


@pytest.mark.parametrize('C,B,shape', [(16, 1, (4, 6, 6)), (64, 2, (4, 16, 16)), (128, 1, (2, 8, 8)), (256, 1, (2, 4, 4)),
                                        (512, 2, (4, 2, 2)), (1024, 1, (2, 2, 2)), (24, 1, (3, 5, 5))])
def test_resblock_tail(C, B, shape):
    from video_diffusion_nnx_amd import ops
    g = torch.Generator().manual_seed(C)
    y2 = torch.randn(B, *shape, C, generator=g) * 2 + 0.5
    r = torch.randn(B, *shape, C, generator=g)
    gg, gb = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    lg, lb = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    # statistics slab as the conv epilogue would leave it: everything in slot 0
    yg = y2.double().reshape(B, -1, 8, C // 8)
    stats = torch.zeros(B, 32, 8, 2, dtype=torch.float64)
    stats[:, 0, :, 0] = yg.sum(dim=(1, 3)); stats[:, 0, :, 1] = (yg * yg).sum(dim=(1, 3))
    out = ops.resblock_tail(y2.to(DEV), r.to(DEV), stats.reshape(-1).to(DEV), gg.to(DEV), gb.to(DEV), lg.to(DEV), lb.to(DEV))
    ref = R.silu(R.group_norm(y2.double(), gg.double(), gb.double(), 8)) + R.layer_norm(r.double(), lg.double(), lb.double())
    assert _rel(out.cpu().double(), ref) < 2e-6


@pytest.mark.parametrize('C,B,shape,ss', [(256, 2, (4, 8, 8), True), (512, 1, (16, 8, 8), True), (256, 3, (5, 16, 16), False), (64, 1, (3, 7, 5), True),
                                         (1024, 1, (2, 4, 4), False), (24, 2, (1, 3, 3), True)])
def test_block_prologue_pass_bf16(C, B, shape, ss):
    """gn_silu_apply16_kernel (the sampling forward's pre-pass of the wide second convs) vs the oracle's GroupNorm / scale-shift / SiLU."""
    from video_diffusion_nnx_amd import ops
    g = torch.Generator().manual_seed(7 * C + B)
    y = _bf(torch.randn(B, *shape, C, generator=g) * 1.5 + 0.3)
    gg, gb = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    sc = 0.2 * torch.randn(B, 2 * C, generator=g) if ss else None
    yg = y.double().reshape(B, -1, 8, C // 8)
    stats = torch.zeros(B, 32, 8, 2, dtype=torch.float64)
    stats[:, 0, :, 0] = yg.sum(dim=(1, 3)); stats[:, 0, :, 1] = (yg * yg).sum(dim=(1, 3))
    out = ops.gn_silu_apply_bf16(y.to(DEV).to(torch.bfloat16).contiguous(), stats.reshape(-1).to(DEV), gg.to(DEV), gb.to(DEV),
                                 None if sc is None else sc.to(DEV))
    h = R.group_norm(y.double(), gg.double(), gb.double(), 8)
    if ss:
        bc = (B,) + (1,) * len(shape) + (C,)
        h = h * (sc[:, :C].double().reshape(bc) + 1) + sc[:, C:].double().reshape(bc)
    ref = R.silu(h)
    assert _rel(out.float().cpu().double(), ref) < 4e-3          # one bf16 rounding of the result
    # every element bf16(ref) or its neighbour, and only where the fp32 arithmetic can cross a rounding boundary: the floor is 8 x the
    # same formula evaluated in fp32 on the CPU (tests/_parity.py)
    h32 = R.group_norm(y, gg, gb, 8)
    if ss:
        h32 = h32 * (sc[:, :C].reshape(bc) + 1) + sc[:, C:].reshape(bc)
    P.assert_bf16_store(out.cpu(), ref, 8.0 * P.rel(R.silu(h32), ref), f'gn_silu_apply16 C{C} B{B} {shape} ss={ss}')


@pytest.mark.parametrize('c0,c1,C,B,shape', [(64, 64, 64, 2, (4, 16, 16)), (64, 0, 128, 1, (3, 8, 8)), (128, 128, 64, 2, (2, 8, 8)),
                                             (128, 0, 256, 1, (5, 4, 4)), (256, 0, 64, 1, (4, 32, 32)), (64, 64, 64, 3, (16, 64, 64)),
                                             (32, 32, 32, 2, (10, 16, 16)), (32, 0, 64, 1, (10, 8, 8)), (64, 64, 32, 1, (3, 8, 8))])   # dim-32 networks (config_v2_2 as written)
def test_resblock_tail_with_res_conv_bf16(c0, c1, C, B, shape):
    """resblock_tail_rc16_kernel (bf16 activation storage): the block's 1x1 res_conv computed inside the tail from the (concat) block
    input.  Reference = the oracle ops in fp64 on the SAME bf16-rounded tensors and bf16-rounded res_conv weights; the kernel
    accumulates in fp32 and rounds only its output to bf16 (2^-9 relative per element)."""
    from video_diffusion_nnx_amd import ops
    g = torch.Generator().manual_seed(c0 + C)
    bf = torch.bfloat16
    y2 = (torch.randn(B, *shape, C, generator=g) * 2 + 0.5).to(bf)
    x0 = torch.randn(B, *shape, c0, generator=g).to(bf)
    x1 = torch.randn(B, *shape, c1, generator=g).to(bf) if c1 else None
    w = torch.randn(c0 + c1, C, generator=g) / (c0 + c1) ** 0.5
    rb = 0.3 * torch.randn(C, generator=g)
    gg, gb = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    lg, lb = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    yg = y2.double().reshape(B, -1, 8, C // 8)
    stats = torch.zeros(B, 32, 8, 2, dtype=torch.float64)
    stats[:, 3, :, 0] = yg.sum(dim=(1, 3)); stats[:, 3, :, 1] = (yg * yg).sum(dim=(1, 3))
    out = ops.resblock_tail_rc_bf16(y2.to(DEV), x0.to(DEV), None if x1 is None else x1.to(DEV), w.to(DEV), rb.to(DEV),
                                    stats.reshape(-1).to(DEV), gg.to(DEV), gb.to(DEV), lg.to(DEV), lb.to(DEV))
    x = x0.double() if x1 is None else torch.cat([x0.double(), x1.double()], dim=-1)
    r = x @ w.to(bf).double() + rb.double()
    ref = R.silu(R.group_norm(y2.double(), gg.double(), gb.double(), 8)) + R.layer_norm(r, lg.double(), lb.double())
    assert out.dtype == bf
    assert _rel(out.cpu().double(), ref) < 3e-3                         # bf16 output rounding: 2^-9 / sqrt(3) ~ 1.1e-3 rms
    assert (out.cpu().double() - ref).abs().max() < 2e-2 * ref.abs().max()
    r32 = x.float() @ w.to(bf).float() + rb
    ref32 = R.silu(R.group_norm(y2.float(), gg, gb, 8)) + R.layer_norm(r32, lg, lb)
    P.assert_bf16_store(out.cpu(), ref, 8.0 * P.rel(ref32, ref), f'tail_rc16 {c0}+{c1}->{C} B{B} {shape}')


def test_resblock_tail_with_res_conv_rejects_unserved_shapes():
    from video_diffusion_nnx_amd import ops
    from video_diffusion_nnx_amd._lib import VdxError
    bf = torch.bfloat16
    y2 = torch.zeros(1, 2, 4, 4, 96, dtype=bf, device=DEV)
    x0 = torch.zeros(1, 2, 4, 4, 64, dtype=bf, device=DEV)
    z = torch.zeros(96, device=DEV)
    with pytest.raises(VdxError):
        ops.resblock_tail_rc_bf16(y2, x0, None, torch.zeros(64, 96, device=DEV), z, torch.zeros(32 * 8 * 2, dtype=torch.float64, device=DEV),
                                  z, z, z, z)


@pytest.mark.parametrize('Cin,D,k', [(1, 64, 7), (3, 16, 7), (3, 40, 3)])
def test_init_conv(Cin, D, k):
    from video_diffusion_nnx_amd import ops
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, Cin, 3, 20, 12, generator=g)
    kern = torch.randn(1, k, k, Cin, D, generator=g) / k
    bias = torch.randn(D, generator=g)
    y = ops.init_conv(x.to(DEV), kern.to(DEV), bias.to(DEV))
    ref = R.conv_1kk(x.double().permute(0, 2, 3, 4, 1), kern.double(), bias.double())
    assert _rel(y.cpu().double(), ref) < 2e-6


@pytest.mark.parametrize('D,Cout', [(64, 1), (16, 3), (32, 2)])
def test_final_conv(D, Cout):
    from video_diffusion_nnx_amd import ops
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 3, 7, 5, D, generator=g)
    kern = torch.randn(1, D, Cout, generator=g)
    bias = torch.randn(Cout, generator=g)
    y = ops.final_conv(x.to(DEV), kern.to(DEV), bias.to(DEV))
    assert _rel(y.cpu().double(), R.conv_pointwise(x.double(), kern.double(), bias.double())) < 2e-6


@pytest.mark.parametrize('dim,cond_dim', [(64, 0), (16, 32), (32, 768)])
def test_time_mlp(dim, cond_dim):
    from video_diffusion_nnx_amd import ops
    g = torch.Generator().manual_seed(3)
    B = 5
    t = torch.tensor([0, 1, 437, 998, 999])
    w1, b1 = torch.randn(dim, 4 * dim, generator=g) / dim ** 0.5, torch.randn(4 * dim, generator=g) * 0.1
    w2, b2 = torch.randn(4 * dim, 4 * dim, generator=g) / (4 * dim) ** 0.5, torch.randn(4 * dim, generator=g) * 0.1
    cond = torch.randn(B, cond_dim, generator=g) if cond_dim else None
    null = torch.randn(1, cond_dim, generator=g) if cond_dim else None
    mask = torch.tensor([0, 1, 0, 1, 1], dtype=torch.bool) if cond_dim else None
    temb = ops.time_mlp(t.to(DEV), w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV),
                        cond=None if cond is None else cond.to(DEV), null_cond_emb=None if null is None else null.to(DEV),
                        cond_mask=None if mask is None else mask.to(DEV))
    e = R.sinusoidal_pos_emb(t, dim, torch.float64)
    ref = R.gelu_tanh(e @ w1.double() + b1.double()) @ w2.double() + b2.double()
    if cond_dim:
        ref = torch.cat((ref, torch.where(mask[:, None], null.double(), cond.double())), -1)
    # fp32 sin/cos of arguments up to ~1e3 rad: absolute error ~6e-5 in the embedding
    assert _rel(temb.cpu().double(), ref) < 2e-4


def _mha_params(C, heads, g):
    p = {}
    for n in ('q', 'k', 'v'):
        p[f'a.{n}.kernel'] = torch.randn(C, heads, 32, generator=g) / C ** 0.5 * 2
        p[f'a.{n}.bias'] = torch.randn(heads, 32, generator=g) * 0.2
    p['a.out.kernel'] = torch.randn(heads, 32, C, generator=g) / (heads * 32) ** 0.5
    p['a.out.bias'] = torch.randn(C, generator=g) * 0.2
    return p


ATTN_CASES = [
    # B, F, H, W, C, heads, temporal
    (1, 16, 8, 8, 64, 8, True),
    (2, 10, 4, 6, 32, 8, True),       # F = 10 (YAML config): padded keys are masked
    (1, 4, 2, 2, 128, 8, True),
    (1, 16, 2, 2, 512, 8, True),
    (1, 32, 3, 3, 16, 4, True),
    (1, 3, 8, 8, 512, 8, False),      # bottleneck spatial attention: 64 tokens
    (2, 4, 2, 2, 128, 8, False),      # 4 tokens
    (1, 2, 4, 4, 256, 8, False),
    (1, 2, 5, 5, 64, 8, False),       # 25 tokens -> LP 32
    (1, 16, 192, 192, 64, 8, True),   # 36864 sequences: workgroups walk 9 sub-tiles (more than 8, last workgroup ragged)
]


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
@pytest.mark.parametrize('case', ATTN_CASES)
def test_attention(mode, case):
    from video_diffusion_nnx_amd import ops
    B, Fr, H, W, C, heads, temporal = case
    g = torch.Generator().manual_seed(sum(case[:5]))
    x = torch.randn(B, Fr, H, W, C, generator=g)
    p = _mha_params(C, heads, g)
    packed = ops.pack_mha(*[(p[f'a.{n}.kernel'].to(DEV), p[f'a.{n}.bias'].to(DEV)) for n in ('q', 'k', 'v', 'out')], mode)
    with PR.bound(PR.cid('blocks attention', mode, case)):       # (the first launch against tests/golden/parity_routes.json)
        y = ops.attention_forward(x.to(DEV), packed, heads, temporal, mode)
    pd = {k: v.double() for k, v in p.items()}
    xd = x.double()
    if temporal:
        xt = xd.permute(0, 2, 3, 1, 4).reshape(B, H * W, Fr, C)
        o = R.multihead_attention(pd, 'a', xt, 32).reshape(B, H, W, Fr, C).permute(0, 3, 1, 2, 4)
    else:
        o = R.multihead_attention(pd, 'a', xd.reshape(B, Fr, H * W, C), 32).reshape(B, Fr, H, W, C)
    ref = o + xd
    rel = _rel((y.cpu().double() - xd), o)          # error of the attention branch itself, not hidden by the residual
    assert rel < TOL[mode], (mode, case, rel)
    assert _rel(y.cpu().double(), ref) < TOL[mode]


# The same block on bf16 TENSORS (bf16 activation storage), through vdx_attention_forward_bf16.  C = 64 with 16 frames and >= 256
# sequences is attention_w_kernel (one wave per group of 4 sequences, all heads in the wave: the level-0 kernel of the N shape): 1, 2
# and 3 groups per wave, a ragged last workgroup (waves without a group), groups on both sides of a sample boundary; the other cases
# keep the one-wave-per-head kernels covered at block level.  The oracle sees the bf16-rounded input; the output is rounded to bf16
# once more (2^-9 of |x + branch| against a branch of ~0.3 |x|), hence the wider stated tolerance on the branch alone.
ATTN16_CASES = [
    # B, F, H, W, C
    (1, 16, 16, 16, 64),       # 64 groups: one per wave, 8 workgroups
    (2, 16, 48, 47, 64),       # 1128 groups over two samples
    (1, 16, 96, 93, 64),       # 2232 groups: 2 per wave, last workgroup has 8 groups for 8 waves x 2
    (3, 16, 64, 48, 64),       # 2304 groups, 3 samples
    (1, 16, 8, 8, 64),         # 64 sequences: below the threshold -> attention_h8_kernel FULL form
    (1, 12, 16, 16, 64),       # 12 frames: the masked form of attention_w_kernel (keys >= L masked, rows of tokens >= L not touched)
    (1, 16, 16, 16, 32),       # C = 32 (level 0 of dim-32 networks): one K chunk, one pair of output tiles
    (2, 10, 24, 22, 32),       # the YAML-literal config_v2_2's temporal attention: C = 32, 10 frames, 264 groups over two samples
    (1, 10, 8, 8, 32),         # below the threshold: attention_h8_kernel C = 32 form
    (1, 16, 8, 8, 128),
]


ATTN16_FP8 = (ATTN16_CASES[0], ATTN16_CASES[7])     # the cases that run the fp8 (e4m3) core as well
ATTN16_KERNEL = {c: 'attention_w_kernel' if c[2] * c[3] >= 256 and c[4] in (32, 64) else 'attention_h8_kernel' for c in ATTN16_CASES}    # what the comments of the table say


@pytest.mark.parametrize('case', ATTN16_CASES)
def test_attention_bf16_tensors(case):
    from video_diffusion_nnx_amd import ops
    B, Fr, H, W, C = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, Fr, H, W, C, generator=g).bfloat16()
    p = _mha_params(C, 8, g)
    packed = ops.pack_mha(*[(p[f'a.{n}.kernel'].to(DEV), p[f'a.{n}.bias'].to(DEV)) for n in ('q', 'k', 'v', 'out')], 'bf16')
    with PR.bound(PR.cid('blocks attention16', case)):
        y = ops.attention_forward_bf16(x.to(DEV), packed, 8, True)
    xd = x.double()
    xt = xd.permute(0, 2, 3, 1, 4).reshape(B, H * W, Fr, C)
    o = R.multihead_attention({k: v.double() for k, v in p.items()}, 'a', xt, 32).reshape(B, H, W, Fr, C).permute(0, 3, 1, 2, 4)
    yd = y.cpu().double()
    assert torch.isfinite(yd).all()
    rel_branch, rel = _rel(yd - xd, o), _rel(yd, o + xd)
    print(f'attention on bf16 tensors {case}: branch {rel_branch:.3e}, block {rel:.3e}')
    assert rel_branch < 4e-2 and rel < 1e-2, (case, rel_branch, rel)
    y2 = ops.attention_forward_bf16(x.to(DEV), packed, 8, True)
    assert torch.equal(y, y2)                      # no order-dependent sums: bit-reproducible
    if case in ATTN16_FP8:  # the fp8 (e4m3) QK^T / PV core of the same kernels (parity unpinned; stated 1e-1 as above)
        with PR.bound(PR.cid('blocks attention16', case, 'fp8')):
            y8 = ops.attention_forward_bf16(x.to(DEV), packed, 8, True, fp8_core=True).cpu().double()
        r8 = _rel(y8 - xd, o)
        print(f'   fp8 core: branch {r8:.3e}')
        assert rel_branch * 1.5 < r8 < 1e-1, (case, r8, rel_branch)


# fp8 attention core (vdx_set_attention_fp8 / BASELINE.json configs[4]): q, k, v and the softmax probabilities of the <= 16-token
# blocks are rounded to e4m3 (3 mantissa bits: 2^-4 relative per element) before QK^T / PV.  No reference counterpart (parity
# unpinned): checked against the fp64 oracle of the block.  Measured (r02): attention branch 4-7e-2 against 0.4-0.8e-2 with bf16
# operands (the test weights give scores of several units, where an e4m3 rounding of q and k moves a logit by ~0.1); stated 1e-1.  The kernels covered: attention_h8 (C = 64 / 128, 8 heads), attention_head + 1x1 (C >= 256 through the
# network test below), attention_reg (other head counts / widths).  Sequences of more than 16 tokens ignore the flag.
FP8_CASES = [c for c in ATTN_CASES if (c[1] if c[6] else c[2] * c[3]) <= 16 and c[2] < 100]


@pytest.mark.parametrize('case', FP8_CASES)
def test_attention_fp8_core(case):
    from video_diffusion_nnx_amd import ops
    B, Fr, H, W, C, heads, temporal = case
    g = torch.Generator().manual_seed(sum(case[:5]))
    x = torch.randn(B, Fr, H, W, C, generator=g)
    p = _mha_params(C, heads, g)
    packed = ops.pack_mha(*[(p[f'a.{n}.kernel'].to(DEV), p[f'a.{n}.bias'].to(DEV)) for n in ('q', 'k', 'v', 'out')], 'bf16')
    with PR.bound(PR.cid('blocks fp8', case, False)):
        y16 = ops.attention_forward(x.to(DEV), packed, heads, temporal, 'bf16')
    with PR.bound(PR.cid('blocks fp8', case, True)):
        y8 = ops.attention_forward(x.to(DEV), packed, heads, temporal, 'bf16', fp8_core=True)
    pd = {k: v.double() for k, v in p.items()}
    xd = x.double()
    if temporal:
        xt = xd.permute(0, 2, 3, 1, 4).reshape(B, H * W, Fr, C)
        o = R.multihead_attention(pd, 'a', xt, 32).reshape(B, H, W, Fr, C).permute(0, 3, 1, 2, 4)
    else:
        o = R.multihead_attention(pd, 'a', xd.reshape(B, Fr, H * W, C), 32).reshape(B, Fr, H, W, C)
    r16, r8 = _rel(y16.cpu().double() - xd, o), _rel(y8.cpu().double() - xd, o)
    print(f'fp8 core {case}: attention branch rel {r8:.3e} (bf16 operands {r16:.3e})')
    assert r8 < 1e-1, (case, r8)
    assert r8 > 1.5 * r16, 'the fp8 path must actually run (its error sits well above the bf16 operands\')'


SLA_CASES = [
    # B, F, H, W, C
    (1, 2, 16, 16, 64),
    (1, 2, 64, 64, 64),       # N = 4096: 8 chunks of 8 sub-tiles, online softmax rescale path
    (2, 3, 8, 8, 128),
    (1, 4, 2, 2, 512),        # N = 4 (single ragged tile)
    (1, 2, 5, 7, 16),         # N = 35 ragged
    (1, 1, 24, 24, 256),      # N = 576: 9 tiles -> 2 chunks, second ragged
]


# The SLA block on bf16 tensors (vdx_sla_forward_bf16).  C = 64 with >= 128 frames of >= 2048 pixels: the second half on sla_out_w_kernel
# (one wave per 64 pixels); fewer frames / smaller frames / other widths keep sla_out8_kernel covered at block level.  Stated tolerance as for the attention block on bf16 tensors.
SLA16_CASES = [
    # B, F, H, W, C
    (8, 16, 64, 64, 64),       # 128 frames of 64 groups: sla_out_w_kernel, one frame per workgroup
    (22, 12, 64, 32, 64),      # 264 frames of 32 groups over 256 workgroups: 2 frames per workgroup, the last range ragged
    (13, 10, 32, 32, 64),      # frames of 1024 pixels: below the kernel's pixel threshold -> sla_out8_kernel
    (8, 16, 16, 16, 64),
    (1, 16, 32, 32, 64),       # 16 frames: sla_out8_kernel
    (2, 10, 16, 16, 32),
    (1, 4, 16, 16, 128),
]


@pytest.mark.parametrize('case', SLA16_CASES)
def test_sla_bf16_tensors(case):
    from video_diffusion_nnx_amd import ops
    B, Fr, H, W, C = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, Fr, H, W, C, generator=g)
    x[:, :, H // 2, W // 2] *= 6                                  # (a spike in the k logits: the online-softmax rescale of the first half)
    x = x.bfloat16()
    p = {f'a.{n}.kernel': torch.randn(1, C, 256, generator=g) / C ** 0.5 * 3 for n in ('q', 'k', 'v')}
    p['a.to_out.kernel'] = torch.randn(1, 256, C, generator=g) / 16
    with PR.bound(PR.cid('blocks sla16', case)):
        y = ops.sla_forward_bf16(x.to(DEV), *[p[f'a.{n}.kernel'].to(DEV) for n in ('q', 'k', 'v', 'to_out')])
    xd = x.double()
    o = R.spatial_linear_attention({k: v.bfloat16().double() for k, v in p.items()}, 'a', xd, 8)
    yd = y.cpu().double()
    assert torch.isfinite(yd).all()
    rel_branch, rel = _rel(yd - xd, o), _rel(yd, o + xd)
    print(f'SLA on bf16 tensors {case}: branch {rel_branch:.3e}, block {rel:.3e}')
    assert rel_branch < 4e-2 and rel < 1e-2, (case, rel_branch, rel)
    y2 = ops.sla_forward_bf16(x.to(DEV), *[p[f'a.{n}.kernel'].to(DEV) for n in ('q', 'k', 'v', 'to_out')])
    assert torch.equal(y, y2)


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
@pytest.mark.parametrize('case', SLA_CASES)
def test_sla(mode, case):
    from video_diffusion_nnx_amd import ops
    B, Fr, H, W, C = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, Fr, H, W, C, generator=g)
    p = {f'a.{n}.kernel': torch.randn(1, C, 256, generator=g) / C ** 0.5 * 3 for n in ('q', 'k', 'v')}
    p['a.to_out.kernel'] = torch.randn(1, 256, C, generator=g) / 16
    # spike some k logits so the running max jumps between sub-tiles (forces the rescale branch)
    x[:, :, H // 2, W // 2] *= 6
    with PR.bound(PR.cid('blocks sla', mode, case)):
        y = ops.sla_forward(x.to(DEV), p['a.q.kernel'].to(DEV), p['a.k.kernel'].to(DEV), p['a.v.kernel'].to(DEV),
                            p['a.to_out.kernel'].to(DEV), 8, mode)
    o = R.spatial_linear_attention({k: v.double() for k, v in p.items()}, 'a', x.double(), 8)
    rel = _rel(y.cpu().double() - x.double(), o)
    assert rel < TOL[mode], (mode, case, rel)
