"""The comparison helpers of tests/_parity.py bite: CPU tensors only.

Each test builds an fp64 reference and the clean fp32 CPU evaluation of the same operation, derives the bound exactly as
tests/test_gpu_backward_forms.py does (from the reference side), checks that the clean evaluation passes, and then hands the helper
a "kernel output" with one subtle, localized fault -- the class of fault the whole-network gradient tests (rel-L2 2.5e-2 .. 7e-2,
five times that per tensor) cannot see.  The helper must reject every one of them."""
import pytest
import torch

import _parity as P
from oracle import unet3d_ref as R


def _wgrad(x, dy, k=3):
    """Weight gradient of a (1,k,k) SAME conv through the oracle, in the dtype of x."""
    kern = torch.zeros(1, k, k, x.shape[-1], dy.shape[-1], dtype=x.dtype, requires_grad=True)
    y = R.conv_1kk(x, kern, None)
    (g,) = torch.autograd.grad(y, kern, dy)
    return g


@pytest.fixture(scope='module')
def nshape_wgrad():
    """conv2 of a level-0 block at the north-star shape: 64 -> 64, 16 frames of 64 x 64, B = 2; bf16-representable operands."""
    g = torch.Generator().manual_seed(11)
    x = P.bf16r(torch.randn(2, 16, 64, 64, 64, generator=g))
    dy = P.bf16r(torch.randn(2, 16, 64, 64, 64, generator=g))
    ref64 = _wgrad(x.double(), dy.double())
    ref32 = _wgrad(x, dy)
    return x, dy, ref64, ref32


def test_dropped_boundary_row_of_one_patch_is_rejected(nshape_wgrad):
    x, dy, ref64, ref32 = nshape_wgrad
    sl = P.wgrad_slices(ref64.shape)
    bound, sb, floor = P.exact_products_bounds(ref32, ref64, sl, P._view3)
    print(f'N-shape wgrad: CPU fp32 floor {floor:.3e}, bound {bound:.3e}')
    P.assert_exact_products(ref32, ref64, bound, sl, sb, P._view3, 'clean fp32 evaluation')
    # an 8 x 16 patch of frame 5 of sample 1 (rows 24..31, columns 32..47) loses the halo row below it: the three taps that look one
    # row down (ky = 2) miss the contribution of the patch's last row -- 16 of the 131072 positions of each weight element
    b, f, y, x0 = 1, 5, 31, 32
    got = ref32.clone()
    for kx in range(3):
        xs = x[b, f, y + 1, x0 + kx - 1:x0 + kx - 1 + 16, :]           # input pixels under tap (2, kx) of output row y
        got[0, 2, kx] -= xs.t() @ dy[b, f, y, x0:x0 + 16, :]
    whole = P.rel(got, ref64)
    assert whole < 2.5e-2, 'the fault must be one the whole-network bound cannot see'
    with pytest.raises(AssertionError):
        P.assert_exact_products(got, ref64, bound, sl, sb, P._view3, 'dropped boundary row')
    # and a single slice (tap 8) is enough to trip the per-slice check even where a generous global bound would not
    with pytest.raises(AssertionError, match='slice'):
        P.assert_exact_products(got, ref64, 1.0, sl, sb, P._view3, 'dropped boundary row, per-slice only')


def test_omitted_last_slot_and_swapped_split_blocks_are_rejected():
    # the q|k|v weight gradient (64 -> 768, split 256) as 40 per-workgroup slots added in a fixed order
    g = torch.Generator().manual_seed(12)
    rows, nslots = 40 * 64, 40
    x = P.bf16r(torch.randn(rows, 64, generator=g))
    dy = P.bf16r(torch.randn(rows, 768, generator=g))
    ref64 = x.double().t() @ dy.double()
    slots = torch.stack([x[k * 64:(k + 1) * 64].t() @ dy[k * 64:(k + 1) * 64] for k in range(nslots)])      # fp32 partial tiles
    clean = torch.zeros(64, 768)
    for k in range(nslots):
        clean += slots[k]
    sl = P.wgrad_slices(ref64.shape)
    bound, sb, floor = P.exact_products_bounds(x.t() @ dy, ref64, sl, P._view3)
    P.assert_exact_products(clean, ref64, bound, sl, sb, P._view3, 'clean slot sum')
    with pytest.raises(AssertionError):
        P.assert_exact_products(clean - slots[-1], ref64, bound, sl, sb, P._view3, 'last of 40 slots omitted')
    # the exact-integer form the GPU test of the slot pass uses
    part, exp = P.slot_pattern(40, 1000, 1003)
    s = part.reshape(40, 1003)[:, :1000].double()
    assert torch.equal(s.sum(0), exp)
    assert not torch.equal(s[:-1].sum(0), exp)                              # dropped slot
    assert not torch.equal(torch.cat((s.sum(0)[:-1], s.sum(0)[:1])), exp)  # ragged tail: last element wrong
    # split epilogue that misplaces a column block of 4 channels: columns 4..7 and 8..11 of dWk swapped
    blocks = P.split_columns(clean.reshape(-1), 768, 256)
    refb = P.split_columns(ref64.reshape(-1), 768, 256)
    bad = blocks[1].clone()
    bad[:, 4:8], bad[:, 8:12] = blocks[1][:, 8:12], blocks[1][:, 4:8]
    slb = P.wgrad_slices(refb[1].shape)
    P.assert_exact_products(blocks[1], refb[1], bound, slb, None, P._view3, 'clean dWk')
    assert P.rel(torch.cat([blocks[0], bad, blocks[2]], 1), ref64) < 0.35, 'the fault must be one the per-tensor whole-network bound cannot see'
    with pytest.raises(AssertionError):
        P.assert_exact_products(bad, refb[1], bound, slb, None, P._view3, 'swapped 4-channel column blocks')


def test_truncation_instead_of_rounding_is_rejected():
    # dL/dy of the block prologue act = SiLU(GroupNorm(y) * (1 + s) + sh), stored as bf16
    g = torch.Generator().manual_seed(13)
    C, B = 64, 2
    y = P.bf16r(torch.randn(B, 4, 16, 16, C, generator=g) * 1.5 + 0.3)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    ss = 0.3 * torch.randn(B, 2 * C, generator=g)
    dact = torch.randn(y.shape, generator=g)

    def dy_of(dt):
        yy = y.to(dt).requires_grad_(True)
        h = R.group_norm(yy, gamma.to(dt), beta.to(dt), 8) * (ss.to(dt)[:, None, None, None, :C] + 1) + ss.to(dt)[:, None, None, None, C:]
        (gy,) = torch.autograd.grad(R.silu(h), yy, dact.to(dt))
        return gy

    ref64, ref32 = dy_of(torch.float64), dy_of(torch.float32)
    floor = 3e-5          # what tests/test_gpu_backward_forms.py passes: the bound the fp32-tensor twin of the kernel is held to
    P.assert_bf16_store(ref32.to(torch.bfloat16), ref64, floor, 'clean fp32 evaluation, rounded once')
    trunc = P.bf16_trunc(ref32).to(torch.bfloat16)
    # truncation stays within one ulp (+ floor) of bf16(ref) everywhere: the per-element check runs first and passes, only the cap sees it
    with pytest.raises(AssertionError, match='differ'):
        P.assert_bf16_store(trunc, ref64, floor, 'truncated')
    # rounding twice (through fp16-like 11 bits, then 8): also within one ulp, also over the cap
    m, e = torch.frexp(ref32.double())
    twice = torch.ldexp(torch.round(m * 2 ** 9) / 2 ** 9, e).float().to(torch.bfloat16)
    with pytest.raises(AssertionError):
        P.assert_bf16_store(twice, ref64, floor, 'rounded twice')
    # an element two ulps off is rejected however few there are
    off = ref32.to(torch.bfloat16).clone()
    off.view(-1)[7] = (off.view(-1)[7].double() + 2.5 * P.bf16_ulp(off.view(-1)[7].double())).to(torch.bfloat16)
    with pytest.raises(AssertionError, match='ulp'):
        P.assert_bf16_store(off, ref64, floor, 'one element 2.5 ulp off')


def test_one_zeroed_attention_sequence_of_4096_is_rejected():
    # temporal attention at level 0 of the north-star shape: 64 x 64 sequences of 16 frames, 8 heads
    g = torch.Generator().manual_seed(14)
    B, Fr, HW, heads = 1, 16, 4096, 8
    qkv = P.bf16r(torch.randn(B * Fr * HW, 3 * heads * 32, generator=g))
    d_o = P.bf16r(torch.randn(B * Fr * HW, heads * 32, generator=g))
    o64, g64 = P.attn_core(qkv, d_o, B, Fr, HW, heads, True)
    oe, ge = P.attn_core(qkv, d_o, B, Fr, HW, heads, True, emulate=True, round_out=True)
    seqs = lambda t: t.reshape(B, Fr, HW, -1).permute(0, 2, 1, 3)
    bound = P.group_bound(seqs(ge), seqs(g64), (B, HW))
    print(f'per-sequence bound {bound:.3e}')
    assert bound < 2e-2, 'the emulated bf16 roundings should cost well under the global 1.5e-2 per sequence'
    _, clean = P.attn_core(qkv, d_o, B, Fr, HW, heads, True, emulate=True, round_out=True, dtype=torch.float32)
    assert P.rel(clean, g64) < 1.5e-2
    P.assert_groups(seqs(clean), seqs(g64), (B, HW), bound, 'clean fp32 evaluation')
    bad = clean.clone().reshape(B, Fr, HW, -1)
    bad[:, :, 1234, :] = 0                                                  # one sequence never written
    bad = bad.reshape(clean.shape)
    assert P.rel(bad, g64) < 2.5e-2, 'the fault must be one the whole-network bound cannot see'
    with pytest.raises(AssertionError, match='group'):
        P.assert_groups(seqs(bad), seqs(g64), (B, HW), bound, 'one sequence zeroed')


def test_closed_forms_match_autograd():
    """The fp64 closed forms that serve as references for the attention cores are autodiff of the oracle's forward."""
    g = torch.Generator().manual_seed(15)
    D = torch.float64
    for B, Fr, H, W, heads, temporal in [(2, 5, 2, 3, 8, True), (1, 2, 3, 3, 4, False)]:
        HD, npix = heads * 32, B * Fr * H * W
        qkv = torch.randn(npix, 3 * HD, generator=g, dtype=D).requires_grad_(True)
        d_o = torch.randn(npix, HD, generator=g, dtype=D)
        x = qkv.reshape(B, Fr, H * W, 3, heads, 32)
        seq = x.permute(0, 2, 1, 3, 4, 5) if temporal else x
        q, k, v = seq[..., 0, :, :] / 32 ** 0.5, seq[..., 1, :, :], seq[..., 2, :, :]
        o = torch.einsum('...hij,...jhd->...ihd', torch.softmax(torch.einsum('...ihd,...jhd->...hij', q, k), -1), v)
        o_rows = (o.permute(0, 2, 1, 3, 4) if temporal else o).reshape(npix, HD)
        (gq,) = torch.autograd.grad(o_rows, qkv, d_o)
        o2, g2 = P.attn_core(qkv.detach(), d_o, B, Fr, H * W, heads, temporal)
        assert P.rel(o2, o_rows.detach()) < 1e-12 and P.rel(g2, gq) < 1e-12
    NF, N = 2, 35
    q, k, v = [(2 * torch.randn(NF * N, 256, generator=g, dtype=D)).requires_grad_(True) for _ in range(3)]
    d_out = torch.randn(NF * N, 256, generator=g, dtype=D)
    hs = lambda t: t.reshape(NF, N, 8, 32).permute(0, 2, 3, 1)
    ctx = torch.einsum('bhdn,bhen->bhde', torch.softmax(hs(k), -1), hs(v))
    out = torch.einsum('bhde,bhdn->bhen', ctx, torch.softmax(hs(q), -2)).permute(0, 3, 1, 2).reshape(NF * N, 256)
    gq, gk, gv = torch.autograd.grad(out, (q, k, v), d_out)
    o2, g2 = P.sla_core(q.detach(), k.detach(), v.detach(), d_out, NF, N)
    assert P.rel(o2, out.detach()) < 1e-12 and P.rel(g2, torch.cat((gq, gk, gv), -1)) < 1e-12
    # fused temporal attention block
    B, Fr, HW = 1, 5, 6
    x = torch.randn(B, Fr, HW, 64, generator=g, dtype=D).requires_grad_(True)
    dy = torch.randn(B, Fr, HW, 64, generator=g, dtype=D)
    wqkv, bqkv, wo = torch.randn(64, 768, generator=g, dtype=D) * 0.15, torch.randn(768, generator=g, dtype=D) * 0.1, torch.randn(256, 64, generator=g, dtype=D) * 0.1
    s = (x.reshape(-1, 64) @ wqkv + bqkv).reshape(B, Fr, HW, 3, 8, 32).permute(0, 2, 1, 3, 4, 5)
    q, k, v = s[..., 0, :, :] / 32 ** 0.5, s[..., 1, :, :], s[..., 2, :, :]
    o = torch.einsum('...hij,...jhd->...ihd', torch.softmax(torch.einsum('...ihd,...jhd->...hij', q, k), -1), v).permute(0, 2, 1, 3, 4).reshape(-1, 256)
    y = (o @ wo).reshape(x.shape) + x
    (gx,) = torch.autograd.grad(y, x, dy)
    dx, o2, _ = P.fused_attention(x.detach(), dy, wqkv, bqkv, wo, B, Fr, HW)
    assert P.rel(dx, gx.reshape(-1, 64)) < 1e-12 and P.rel(o2, o.detach()) < 1e-12


def test_helper_primitives():
    t = torch.tensor([1.0, 1.00390625, 3.0, -0.75, 0.0], dtype=torch.float64)
    assert torch.equal(P.bf16_ulp(t), torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 0.0], dtype=torch.float64))
    assert torch.equal(P.bf16r(torch.tensor([1.00390625])), torch.tensor([1.0]))            # tie to even
    assert torch.equal(P.bf16_trunc(torch.tensor([1.0078124])), torch.tensor([1.0]))
    w, i, allr = P.per_group_rel(torch.tensor([[1.0, 1.0], [2.0, 0.0]]), torch.tensor([[1.0, 1.0], [2.0, 2.0]]), (2,))
    assert i == 1 and abs(w - 0.5 ** 0.5) < 1e-12 and allr.shape == (2,)
    with pytest.raises(AssertionError):
        P.exact_products_bounds(torch.tensor([1.0, 1.001]), torch.tensor([1.0, 1.0], dtype=torch.float64))      # floor too high to mean anything


# ---- forward forms: the bounds of tests/test_gpu_forward_forms.py, tests/test_gpu_conv.py and tests/test_gpu_blocks.py bite ------------------
# Data from the reference at the GPU tests' own shapes (tests/_forward_cases.py builds cases and bounds for both sides); one fault at a
# time; the clean CPU evaluation passes, the fault is rejected at exactly the bound the GPU test uses.

import _forward_cases as FC


@pytest.fixture(scope='module')
def c64_conv():
    """test_persistent_c64_conv's plain form: (2, 32, 64, 64, 64), 3x3, 64 -> 64, bf16-rounded operands; fp64 and fp32 evaluations."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 32, 64, 64, 64, generator=g)
    x[1] *= 1.7
    kern = torch.randn(1, 3, 3, 64, 64, generator=g) / (9 * 64) ** 0.5
    bias = torch.randn(64, generator=g)
    ref64 = R.conv_1kk(P.bf16r(x).double(), P.bf16r(kern).double(), bias.double())
    ref32 = R.conv_1kk(P.bf16r(x), P.bf16r(kern), bias)
    return ref64, ref32


def test_truncating_store_and_scaled_tile_row_are_rejected(c64_conv):
    ref64, ref32 = c64_conv
    clean = ref32.to(torch.bfloat16)
    P.assert_bf16_store(clean, ref64, P.FWD_STATED, 'clean fp32 evaluation, rounded once')
    trunc = P.bf16_trunc(ref32).to(torch.bfloat16)
    assert P.rel(trunc, ref64) < 4e-3, 'the fault must be one the global rel-L2 of the test cannot see'
    with pytest.raises(AssertionError, match='differ'):
        P.assert_bf16_store(trunc, ref64, P.FWD_STATED, 'truncated')
    # one 16-pixel row of one 16 x 16 tile scaled by 0.9: what a wrong halo row does
    bad = ref32.clone()
    bad[1, 7, 16 + 5, 32:48, :] *= 0.9
    bad = bad.to(torch.bfloat16)
    assert P.rel(bad, ref64) < 4e-3
    with pytest.raises(AssertionError, match='ulp'):
        P.assert_bf16_store(bad, ref64, P.FWD_STATED, 'one tile row scaled')


def test_scaled_tile_row_behind_a_prologue_is_rejected(c64_conv):
    """The prologue form of test_persistent_c64_conv: per-(frame, tile) rel-L2 at max(2e-6, 4 x the flip floor)."""
    ref64, _ = c64_conv
    g = torch.Generator().manual_seed(12)
    y1 = P.bf16r(ref64[:, :4].float())                                 # 4 frames are enough for the CPU proof
    C = 64
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    ss = torch.randn(2, 2 * C, generator=g) * 0.3
    kern2 = P.bf16r(torch.randn(1, 3, 3, C, C, generator=g) / (9 * C) ** 0.5)
    act = lambda dt: P.bf16r(R.silu(R.group_norm(y1.to(dt), gamma.to(dt), beta.to(dt), 8) * (ss.to(dt)[:, None, None, None, :C] + 1) + ss.to(dt)[:, None, None, None, C:]))
    out_of = lambda a: R.conv_1kk(a.double(), kern2.double(), None)
    a64, a32 = act(torch.float64), act(torch.float32).double()
    bound, floor = P.tile_bound(a32, a64, out_of)
    print(f'prologue tile bound {bound:.3e} (flip floor {floor:.3e})')
    assert bound < 5e-3, 'a derived bound above what the test states would be a finding'
    ref2 = out_of(a64)
    clean = R.conv_1kk(a32.float(), kern2, None)
    P.assert_tiles(clean, ref2, bound, what='clean fp32 evaluation')
    bad = clean.clone()
    bad[1, 2, 16 + 5, 32:48, :] *= 0.9
    assert P.rel(bad, ref2) < 5e-3
    with pytest.raises(AssertionError, match='tile'):
        P.assert_tiles(bad, ref2, bound, what='one tile row scaled')
    # the same form with a bf16 output: one rounding of the result is within the 2^-9 the bound gains, the scaled row is not
    bound16, _ = P.tile_bound(a32, a64, out_of, bf16_out=True)
    assert abs(bound16 - bound - P.BF16_ROUNDING) < 1e-12
    worst = P.assert_tiles(clean.to(torch.bfloat16), ref2, bound16, what='clean fp32 evaluation, bf16 output')
    assert worst > bound, 'a bf16 output does not fit the fp32-output bound: the 2^-9 term is needed'
    with pytest.raises(AssertionError, match='tile'):
        P.assert_tiles(bad.to(torch.bfloat16), ref2, bound16, what='one tile row scaled, bf16 output')


def test_tile_statistics_credited_to_the_neighbouring_sample_are_rejected(c64_conv):
    ref64, ref32 = c64_conv
    B, tiles = 2, 32 * 16                                               # 16 tiles of 16 x 16 per frame
    s1, _, s2 = P.gn_sums(ref32, 8, torch.float32)
    clean = torch.stack((s1, s2), -1).double()
    P.assert_gn_stats(clean, ref64, ref32, tiles, what='clean fp32 evaluation')
    # the last tile of sample 0 flushed into sample 1's sums (the per-sample flush of register-resident sums at a sample boundary)
    t1, _, t2 = P.gn_sums(ref64[0:1, 31:, 48:, 48:], 8)
    bad = clean.clone()
    bad[1, :, 0] += t1[0]; bad[1, :, 1] += t2[0]
    bad[0, :, 0] -= t1[0]; bad[0, :, 1] -= t2[0]
    r2 = (ref64.reshape(2, -1, 8, 8) ** 2).sum(dim=(1, 3))
    worst = ((bad[..., 1] - r2).abs() / r2).max().item()
    print(f'one tile in the wrong sample moves sum y^2 by {worst:.2e}')
    assert worst < 2.2e-3, 'the fault must be one rtol = 2e-3 misses or barely sees'
    with pytest.raises(AssertionError, match='sum'):
        P.assert_gn_stats(bad, ref64, ref32, tiles, what='one tile credited to the wrong sample')
    # a bound that could not see one tile is refused
    with pytest.raises(AssertionError, match='share'):
        P.assert_gn_stats(clean, ref64, ref32, 10 ** 6, what='too many tiles for the bound')


def test_consumer_reading_slot_0_only_and_unwritten_pixel_pass_are_rejected():
    C, B, shape = FC.TAIL16[4]                                          # the multi-pass case: 35 pixel groups over 32 workgroups
    c = FC.tail_case(C, B, shape, True)
    slab = c['slab']
    assert (slab[:, 1:].abs().sum() > 0) and torch.allclose(slab.sum(1), P.gn_stats_slab(c['y2'])[:, 0], rtol=1e-12)
    clean = c['ref32'].to(torch.bfloat16)
    P.assert_bf16_store(clean, c['ref64'], c['store_floor'], 'clean fp32 evaluation')
    # statistics from slot 0 alone
    n = c['y2'][0].numel() // 8
    s0 = slab[:, 0]
    mean = s0[..., 0] / n
    rstd = torch.rsqrt((s0[..., 1] / n - mean * mean).clamp_min(0) + R.NORM_EPS)
    bad = FC.tail_formula(c['y2'], c['r'], *c['par'], torch.float32, (mean, rstd)).to(torch.bfloat16)
    with pytest.raises(AssertionError, match='ulp'):
        P.assert_bf16_store(bad, c['ref64'], c['store_floor'], 'slot 0 only')
    # the second pixel pass (pixels 1024..1099 of every sample) never written: NaN-filled output, or stale zeros
    for fill, why in ((float('nan'), 'non-finite'), (0.0, 'ulp')):
        bad = clean.clone().reshape(B, -1, C)
        bad[:, 32 * 32:] = fill
        with pytest.raises(AssertionError, match=why):
            P.assert_bf16_store(bad.reshape(clean.shape), c['ref64'], c['store_floor'], 'second pass unwritten')
    # the fp32-output form at its bound
    m = FC.tail_case(*FC.TAIL_MIXED[0], False)
    P.assert_exact_products(m['ref32'], m['ref64'], m['bound'], m['sl'], m['sb'], None, 'clean mixed tail')
    s0 = m['slab'][:, 0]
    n = m['y2'][0].numel() // 8
    mean = s0[..., 0] / n
    rstd = torch.rsqrt((s0[..., 1] / n - mean * mean).clamp_min(0) + R.NORM_EPS)
    with pytest.raises(AssertionError, match='rel-L2'):
        P.assert_exact_products(FC.tail_formula(m['y2'], m['r'], *m['par'], torch.float32, (mean, rstd)), m['ref64'], m['bound'], m['sl'], m['sb'], None, 'slot 0 only')


def test_neighbouring_head_and_unmasked_keys_are_rejected():
    shape = FC.ATTN_HEADS_TEMPORAL[1]                                   # (2, 10, 5, 7, 512): 10 of 16 key slots are real
    B, Fr, H, W, C = shape
    c = FC.attn_heads_case(shape, True, True, False)
    og, nseq = c['og'], c['nseq']
    P.assert_groups(og(c['oe']), og(c['o64']), (nseq, 8), c['bound_o'], 'clean emulation')
    P.assert_groups(FC.seq_groups(c['ye'], True), FC.seq_groups(c['y64'], True), (nseq,), c['bound_y'], 'clean emulation, y')
    # one (sequence, head) of o taken from the neighbouring head
    bad = og(c['oe']).clone()
    bad[37, 3] = bad[37, 4]
    assert P.rel(bad, og(c['o64'])) < 8e-2, 'one of 560 groups: the tensor as a whole barely moves'
    with pytest.raises(AssertionError, match='group'):
        P.assert_groups(bad, og(c['o64']), (nseq, 8), c['bound_o'], 'neighbouring head')
    # keys past L left unmasked: the 6 padding slots of the 16-token tile take part with k = v = bias
    ob, yb = P.attention_block_fwd(c['x'], *c['w'], B, Fr, H, W, True, emulate=True, round_out=True, unmasked_pad=6)
    with pytest.raises(AssertionError, match='group'):
        P.assert_groups(og(ob), og(c['o64']), (nseq, 8), c['bound_o'], 'unmasked padding keys')
    with pytest.raises(AssertionError, match='group'):
        P.assert_groups(FC.seq_groups(yb, True), FC.seq_groups(c['y64'], True), (nseq,), c['bound_y'], 'unmasked padding keys, y')
    # SLA: one (frame, head) from the neighbouring head
    s = FC.sla_heads_case(FC.SLA_HEADS[1], True)
    P.assert_groups(s['og'](s['oe']), s['og'](s['o64']), (s['NF'], 8), s['bound_o'], 'clean SLA emulation')
    bad = s['og'](s['oe']).clone()
    bad[40, 2] = bad[40, 1]
    with pytest.raises(AssertionError, match='group'):
        P.assert_groups(bad, s['og'](s['o64']), (s['NF'], 8), s['bound_o'], 'SLA neighbouring head')


def test_scale_shift_row_of_the_wrong_sample_is_rejected():
    c = FC.ss_case(96, 9)                                               # sample 8 opens the second group of 8
    for i in range(len(c['layers'])):
        bound, sb, _ = c['b_ss'][i]
        clean = R.layer_norm(R.silu(c['temb']) @ c['layers'][i]['W'] + c['layers'][i]['b'], c['layers'][i]['g'], c['layers'][i]['be'])
        P.assert_exact_products(clean, c['ss64'][i], bound, c['sl'], sb, None, f'clean layer {i}')
        bad = clean.clone()
        bad[8] = clean[0]
        with pytest.raises(AssertionError, match='rel-L2'):
            P.assert_exact_products(bad, c['ss64'][i], bound, c['sl'], sb, None, f'layer {i}: row 8 = row 0')
        # ... and by the per-sample check alone, where a generous global bound would not see one row of nine
        with pytest.raises(AssertionError, match=r'slice\(s\) over their bound, first sample8'):
            P.assert_exact_products(bad, c['ss64'][i], 10.0, c['sl'], sb, None, f'layer {i}: row 8 = row 0, per sample only')


def test_forward_closed_forms_match_the_oracle():
    """attention_block_fwd / sla_block_fwd with emulate=False are the oracle's MultiheadAttention / SpatialLinearAttention + residual."""
    g = torch.Generator().manual_seed(21)
    for (B, Fr, H, W, C), temporal in (((2, 5, 2, 3, 64), True), ((1, 2, 3, 3, 32), False)):
        x = torch.randn(B, Fr, H, W, C, generator=g, dtype=torch.float64)
        w = [t.double() for t in FC.mha_weights(C, g)]
        o, y = P.attention_block_fwd(x, *w, B, Fr, H, W, temporal)
        p = FC.mha_oracle_params(*w)
        if temporal:
            xt = x.permute(0, 2, 3, 1, 4).reshape(B, H * W, Fr, C)
            ref = R.multihead_attention(p, 'a', xt, 32).reshape(B, H, W, Fr, C).permute(0, 3, 1, 2, 4) + x
        else:
            ref = R.multihead_attention(p, 'a', x.reshape(B, Fr, H * W, C), 32).reshape(x.shape) + x
        assert P.rel(y, ref) < 1e-12
        assert P.seq_head_groups(o, B, Fr, H * W, temporal).shape == (B * (H * W if temporal else Fr), 8, (Fr if temporal else H * W) * 32)
    B, Fr, H, W, C = 2, 2, 3, 5, 48
    x = torch.randn(B, Fr, H, W, C, generator=g, dtype=torch.float64)
    wq, wk, wv = [torch.randn(C, 256, generator=g, dtype=torch.float64) for _ in range(3)]
    wo = torch.randn(256, C, generator=g, dtype=torch.float64) / 16
    _, y = P.sla_block_fwd(x, wq, wk, wv, wo, B, Fr, H, W)
    p = {'a.q.kernel': wq[None], 'a.k.kernel': wk[None], 'a.v.kernel': wv[None], 'a.to_out.kernel': wo[None]}
    assert P.rel(y, R.spatial_linear_attention(p, 'a', x, 8) + x) < 1e-12
    if P.have_e4m3():
        assert torch.equal(P.e4m3r(torch.tensor([0.3, 17.0, 500.0])), torch.tensor([0.3125, 16.0, 448.0]))


# ---- per-group bounds of the level-0 attention / SLA kernels (tests/test_gpu_attention_groups.py) ----------------------------------------
# Each fault below is injected into the emulated output of a case of that file.  First it PASSES what tests/test_gpu_blocks.py asserts of
# the same kernels (branch < 4e-2 and block < 1e-2 against the oracle on un-rounded weights), then the per-group assertion rejects it.
# Two faults replace a whole group and cannot pass the 1e-2 at any case of the list (a tile on the neighbouring frame's context, a sequence
# not written): of those the first half asserts that the old check catches them only marginally (_old_assertions_marginal).

import _attention_cases as AC


def _old_figures(branch, x, y_old, what):
    """The global figures of test_attention_bf16_tensors / test_sla_bf16_tensors.  -> (branch rel, block rel)"""
    xd = x.double()
    rb, r = P.rel(branch, y_old - xd), P.rel(branch + xd, y_old)
    print(f'[old assertions] {what}: branch {rb:.3e} (asserted 4e-2), block {r:.3e} (asserted 1e-2)')
    return rb, r


def _old_assertions_pass(rb, r, what):
    assert rb < 4e-2 and r < 1e-2, f'{what}: the global figures do see this fault ({rb:.3e}, {r:.3e}): use a larger case'


def _old_assertions_marginal(rb, r, n, what):
    """A fault that replaces ONE WHOLE group of n by something unrelated has an error of up to sqrt(2) x the group's own size, sqrt(2 / n) of
    the branch; no case of the list has enough groups to take that below the 1e-2 on the block (at 16384 tiles the swapped context still
    reads 1.2e-2, and 8928 sequences are the most an attention case has).  What is true of such a fault is asserted instead: the branch
    assertion passes, and the block assertion catches it by less than sqrt(2 / n) + the clean figure (< 1e-2) -- a margin below 3 where
    the per-group bound has one of 30 and more."""
    assert rb < 4e-2 and 1e-2 <= r < (2 / n) ** 0.5 + 1e-2 <= 3.3e-2, f'{what}: expected the old block assertion to catch this marginally ({rb:.3e}, {r:.3e})'


def _rejected(c, branch, names, what):
    for n in names:
        with pytest.raises(AssertionError, match='over their bound'):
            P.assert_views(branch, c['ref'], c['views'][n], c['bounds'][n], f'{what} per {n}', c['chunk'])


def _clean_passes(c, what):
    for n, v in c['views'].items():
        P.assert_views(c['cmp'], c['ref'], v, c['bounds'][n], f'clean emulation, {what} per {n}', c['chunk'])


def _fp32_attention_passes(c, io16, q_scaled, fp8=False):
    """The rounding points evaluated in fp32 instead of fp64 -- the arithmetic of a correct kernel up to summation order -- inside every bound."""
    y32 = P.attention_block_fwd(c['x'], *c['w'], *c['shape'][:4], c['temporal'], emulate=True, fp8=fp8, round_out=io16, q_scaled=q_scaled, dtype=torch.float32)[1]
    for n, v in c['views'].items():
        P.assert_views(y32.double() - c['x'].double(), c['ref'], v, c['bounds'][n], f"fp32 emulation, attention {c['shape']} fp8={int(fp8)} per {n}")


def _fp32_sla_passes(c, io16):
    b32 = AC.sla_eval(c['x'], c['w'], c['chunk'] or AC.SLA_CHUNK, emulate=True, round_out=io16, dtype=torch.float32)
    for n, v in c['views'].items():
        P.assert_views(b32, c['ref'], v, c['bounds'][n], f"fp32 emulation, SLA {c['shape']} per {n}", c['chunk'])


def test_attention_faults_of_one_group_pass_the_global_figures_and_are_rejected_per_sequence():
    # padding keys unmasked in the last group of 4 sequences: (2, 12, 16, 16, 64), 512 sequences, 4 of 16 key slots are padding
    shape = (2, 12, 16, 16, 64)
    B, Fr, H, W, C = shape
    for iso in (False, True):
        c = AC.attn_case(shape, True, True, 'bf16', False, iso)
        _clean_passes(c, f'attention {shape} iso={int(iso)}')
        _fp32_attention_passes(c, True, False)
        y_old = AC.attn_old_oracle(c)
        yb = P.attention_block_fwd(c['x'], *c['w'], B, Fr, H, W, True, emulate=True, round_out=True, unmasked_pad=4)[1] - c['x'].double()
        bad = c['cmp'].clone()
        bad[1, :, 15, 12:16] = yb[1, :, 15, 12:16]
        _old_assertions_pass(*_old_figures(bad, c['x'], y_old, f'unmasked padding keys in one group of 4, iso={int(iso)}'), 'unmasked padding keys')
        _rejected(c, bad, c['views'], 'unmasked padding keys in one group of 4')
    # (1, 16, 96, 93, 64), 8928 sequences: one head replaced by its neighbour in ONE sequence
    shape = (1, 16, 96, 93, 64)
    B, Fr, H, W, C = shape
    c = AC.attn_case(shape, True, True, 'bf16')
    _clean_passes(c, f'attention {shape}')
    y_old = AC.attn_old_oracle(c)
    wqkv, bqkv, wo, bo = c['w']
    o = P.attention_block_fwd(c['x'], *c['w'], B, Fr, H, W, True, emulate=True, round_out=True)[0]
    pix = 95 * 93 + 90                                                      # a sequence of the last, half-empty workgroup
    rows = torch.arange(Fr) * (H * W) + pix
    o[rows, 7 * 32:8 * 32] = o[rows, 6 * 32:7 * 32]
    bad = P.block_tail(o, c['x'], wo, bo, True) - c['x'].double()
    assert torch.equal(bad.reshape(Fr, H * W, C)[:, :pix], c['cmp'].reshape(Fr, H * W, C)[:, :pix])     # (every other sequence untouched)
    _old_assertions_pass(*_old_figures(bad, c['x'], y_old, 'head 7 := head 6 in one sequence'), 'head 7 := head 6')
    _rejected(c, bad, ['sequence'], 'head 7 := head 6 in one sequence')
    # one sequence of 8928 not written (y = x): sqrt(1 / 8928) = 1.06e-2 of the branch, at the largest attention case of the list: the old
    # block assertion catches it, by a hair
    bad = c['cmp'].clone()
    bad.reshape(Fr, H * W, C)[:, pix] = 0.0
    _old_assertions_marginal(*_old_figures(bad, c['x'], y_old, 'one sequence not written'), H * W, 'one sequence not written')
    _rejected(c, bad, ['sequence'], 'one sequence not written')


def test_sla_faults_of_one_frame_or_tile_pass_the_global_figures_and_are_rejected_per_group():
    shape = (8, 16, 64, 32, 64)                                             # 128 frames of 2048 pixels = 4 chunks of 8 tiles
    f, h = 77, 5
    for iso in (False, True):
        c = AC.sla_case(shape, True, 'bf16', iso)
        _clean_passes(c, f'SLA {shape} iso={int(iso)}')
        _fp32_sla_passes(c, True)
        y_old = AC.sla_old_oracle(c)
        x, w = c['x'], c['w']
        kw = dict(emulate=True, round_out=True)
        # the last chunk's partial of one (frame, head) never reaches the context
        bad = c['cmp'].clone()
        bad[f] = AC.sla_eval(x[f:f + 1], w, fault=('drop_ctx', 0, h, 1536), **kw)[0]
        _old_assertions_pass(*_old_figures(bad, x, y_old, f'a dropped chunk partial of one (frame, head), iso={int(iso)}'), 'a dropped chunk partial')
        _rejected(c, bad, c['views'], 'a dropped chunk partial of one (frame, head)')
        if iso:
            continue
        # one 64-pixel tile computed with the neighbouring frame's context: a whole group of 128 x 32 replaced
        bad = c['cmp'].clone()
        bad[f] = AC.sla_eval(x[f:f + 2], w, fault=('swap_ctx', 0, 31 * 64, 32 * 64, 1), **kw)[0]
        assert torch.equal(bad[f, :31 * 64], c['cmp'][f, :31 * 64])
        _old_assertions_marginal(*_old_figures(bad, x, y_old, 'one tile on the neighbouring frame\'s context'), 128 * 32, 'tile on the neighbouring context')
        _rejected(c, bad, ['(frame, 64-pixel tile)'], 'one tile on the neighbouring frame\'s context')


def test_sla_tile_not_written_passes_the_global_figures_at_512_frames_and_is_rejected_per_tile():
    """One 64-pixel tile left as y = x moves the block figure by sqrt(1 / tiles) of the branch's share: 1.6e-2 at the 4096 tiles of the
    128-frame case, which the 1e-2 sees; at the 16384 tiles of the 512-frame case a typical tile passes.  The tile is the one of median
    branch norm (tiles differ: one of the heaviest, tile 5 of frame 333 at 1.3 x the median, still reads 1.07e-2).  The case is walked
    in chunks of frames."""
    shape = (32, 16, 64, 32, 64)
    c = AC.sla_case(shape, True, 'bf16', old=True)
    step, faulty = c['chunk'], {}
    norms = c['ref'].reshape(c['NF'], c['N'] // 64, -1).norm(dim=2).flatten()
    f, t = divmod(int(norms.argsort()[norms.numel() // 2]), c['N'] // 64)
    tile = slice(t * 64, (t + 1) * 64)
    print(f'[tile not written] frame {f} tile {t}: branch norm {norms[f * (c["N"] // 64) + t]:.3e}, rms over the tiles {norms.square().mean().sqrt():.3e}, max {norms.max():.3e}')

    def unwritten(i0, e):
        if i0 <= f < i0 + step:
            faulty['clean'], faulty['i0'] = e.clone(), i0
            e[f - i0, tile] = 0.0
            faulty['bad'] = e

    rb, r = AC.sla_old_figures(c, unwritten, [f])
    print(f'[old assertions] one tile of 16384 not written: branch {rb:.3e} (asserted 4e-2), block {r:.3e} (asserted 1e-2)')
    _old_assertions_pass(rb, r, 'one tile of 16384 not written')
    i0 = faulty['i0']
    ref = c['ref'][i0:i0 + step]
    for n, v in c['views'].items():
        P.assert_views(faulty['clean'], ref, v, c['bounds'][n], f'clean emulation, frames {i0}.., per {n}')
    with pytest.raises(AssertionError, match='1 group\\(s\\) over their bound'):
        P.assert_views(faulty['bad'], ref, c['views']['(frame, 64-pixel tile)'], c['bounds']['(frame, 64-pixel tile)'], 'one tile not written')


def test_fp32_evaluation_of_the_emulations_passes_every_group_bound():
    """The rounding points evaluated in fp32 instead of fp64 -- the arithmetic of a correct kernel up to summation order -- stay inside
    3 x the fp64 emulation in every group of every view (the masked C = 64 attention_w case and the 128-frame sla_out_w case: in the
    fault tests above, where they are built anyway); and the f32-mode bounds are finite, per group and below the ceiling."""
    for shape, temporal, io16, iso, qs in (((1, 16, 16, 16, 64), True, True, True, False), ((2, 10, 12, 12, 32), True, True, False, False),
                                           ((1, 10, 6, 6, 128), True, True, False, False), ((1, 16, 2, 2, 256), True, False, False, True),
                                           ((1, 2, 5, 5, 64), False, False, False, True)):
        _fp32_attention_passes(AC.attn_case(shape, temporal, io16, 'bf16', False, iso, qs), io16, qs)
        f = AC.attn_case(shape, temporal, False, 'f32', False, iso)
        assert all(b.numel() == P.view_rels(f['ref'], f['ref'], f['views'][n]).numel() and P.FWD_STATED <= b.min() and b.max() < P.EXACT_CEILING
                   for n, b in f['bounds'].items())
    if P.have_e4m3():                                                       # the bounds of the fp8 core, on both kernels that have one
        for shape in ((1, 16, 16, 16, 64), (1, 16, 8, 8, 64)):
            _fp32_attention_passes(AC.attn_case(shape, True, True, 'bf16', True), True, False, fp8=True)
    for shape, io16, iso in (((1, 16, 32, 32, 64), True, True), ((2, 10, 16, 16, 32), True, False), ((1, 1, 24, 24, 256), False, True),
                             ((1, 2, 5, 7, 16), False, False)):
        _fp32_sla_passes(AC.sla_case(shape, io16, 'bf16', iso), io16)
    assert len(P.pixel_tile_view(64)(torch.zeros(2, 35, 16))) == 1 and P.pixel_tile_view(64)(torch.zeros(2, 600, 8))[1].shape == (2, 24 * 8)


def test_head_isolating_out_projection_and_q_scaling_flag():
    g = torch.Generator().manual_seed(5)
    for C in (32, 64, 128):
        wo = P.isolate_heads(torch.randn(256, C, generator=g, dtype=torch.float64))
        o = torch.randn(7, 256, generator=g, dtype=torch.float64)
        o2 = o.clone()
        o2[:, 3 * 32:4 * 32] += 1.0                                          # head 3 moves ...
        d = ((o2 - o) @ wo).abs().sum(0)
        assert (d[torch.arange(C) % 8 == 3] > 0).all() and (d[torch.arange(C) % 8 != 3] == 0).all()     # ... channels c % 8 == 3 alone
    # q_scaled changes where q is rounded, not the function: identical without emulation, different (slightly) with it
    shape = (1, 16, 2, 2, 64)
    x = P.bf16r(torch.randn(*shape, generator=g))
    w = FC.mha_weights(64, g)
    a = P.attention_block_fwd(x, *w, *shape[:4], True)[1]
    b = P.attention_block_fwd(x, *w, *shape[:4], True, q_scaled=True)[1]
    assert P.rel(b, a) < 1e-14
    ae = P.attention_block_fwd(x, *w, *shape[:4], True, emulate=True)[1]
    be = P.attention_block_fwd(x, *w, *shape[:4], True, emulate=True, q_scaled=True)[1]
    assert 0 < P.rel(be, ae) < 1e-2


# ---- fp16 operand mode (tests/test_gpu_f16_forms.py and the f16 entries of tests/test_gpu_attention_groups.py) --------------------------------
# fp16 rounding is 8 x finer than bf16: ONE bf16 rounding left in an fp16 kernel stays inside 3 x the fp16 emulation's own distance from the
# reference (and far inside the whole-network 4e-3).  What sees it is the distance to the EMULATION, measured in multiples of the distance
# between the emulation's own fp32 and fp64 evaluations (P.assert_close_to_emulation).

import test_gpu_attention_groups as G
import test_gpu_f16_forms as G16


def _f16_attention_cases():
    return [(s, t, iso) for s, t, iso, e in G.ATTN32 if 'f16' in e] + [(s, t, iso) for s, t, iso, _, _ in G16.ATTN_F16]


def _f16_sla_cases():
    return [(s, iso) for s, iso, _ in G.SLA32] + [(s, iso) for s, iso, _ in G16.SLA_F16]


def test_f16_rounding_known_answers():
    t = lambda *v: torch.tensor(v, dtype=torch.float64)
    x = t(1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65504.0, 65520.0, 2.0 ** -24, 2.0 ** -25, -(2.0 ** -14), -(2.0 ** -14) * (1 - 2.0 ** -10))
    assert torch.equal(P.f16r(x), t(1.0, 1 + 2.0 ** -9, 65504.0, float('inf'), 2.0 ** -24, 0.0, -(2.0 ** -14), -(2.0 ** -14) * (1 - 2.0 ** -10)))
    assert torch.equal(P.f16r_ftz(x), t(1.0, 1 + 2.0 ** -9, 65504.0, float('inf'), 0.0, 0.0, -(2.0 ** -14), 0.0))       # the smallest normal stays
    assert P.f16r(x.float()).dtype == torch.float32 and P.f16r(x).dtype == torch.float64
    assert torch.equal(P.f16_ulp(t(1.0, 1.5, 3.0, 2.0 ** -14, 2.0 ** -20, 0.0)), t(2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -24, 2.0 ** -24, 0.0))
    assert P.operand_rounding('bf16') is P.bf16r and P.operand_rounding('f16') is P.f16r
    # the running maximum of the generic SLA context kernel: per chunk of nsub tiles, up to and including the pixel's own tile
    K = torch.tensor([1.0, 0.0, 5.0, 2.0, 3.0, 9.0, 0.0]).reshape(1, 1, 7, 1)
    assert P.running_max(K, 2, 1).flatten().tolist() == [1.0, 1.0, 5.0, 5.0, 9.0, 9.0, 0.0]          # chunks of one tile: the tile's own maximum
    assert P.running_max(K, 2, 4).flatten().tolist() == [1.0, 1.0, 5.0, 5.0, 9.0, 9.0, 9.0]          # one chunk: the ragged last tile keeps the 9
    K = torch.tensor([5.0, 0.0, 1.0, 0.0, 2.0, 0.0, 1.0]).reshape(1, 1, 7, 1)
    assert P.running_max(K, 2, 2).flatten().tolist() == [5.0, 5.0, 5.0, 5.0, 2.0, 2.0, 2.0]          # the second chunk starts afresh
    # the default operand leaves the bf16 emulations as they were
    g = torch.Generator().manual_seed(6)
    x = P.bf16r(torch.randn(1, 4, 3, 3, 64, generator=g))
    w = FC.mha_weights(64, g)
    assert torch.equal(P.attention_block_fwd(x, *w, 1, 4, 3, 3, True, emulate=True)[1], P.attention_block_fwd(x, *w, 1, 4, 3, 3, True, emulate=True, operand='bf16')[1])
    with pytest.raises(AssertionError):
        P.block_tail(torch.zeros(36, 256), x, w[2], None, True, operand='f16')                   # no bf16 output in f16 mode


def test_fp32_evaluation_of_the_f16_emulations_passes_and_underflow_does_not_decide():
    """Every f16 case of the GPU tests: the emulation evaluated in fp32 -- a correct kernel up to summation order -- passes the case's
    3 x bounds and (trivially, at ratio 1) the closeness check; the derived bounds sit in [5e-4, 5e-3]; and the emulation with fp16
    subnormals flushed to zero differs from the IEEE one by less than a third of each bound, so that these tests do not depend on what the
    hardware does with subnormals (tests/test_gpu_f16_forms.py test_conv_f16_subnormal_operands asks that question itself)."""
    for shape, temporal, iso in _f16_attention_cases():
        c = AC.attn_case(shape, temporal, False, 'f16', False, iso, True)
        ftz = P.attention_block_fwd(c['x'], *c['w'], *shape[:4], temporal, emulate=True, q_scaled=True, operand='f16_ftz')[1] - c['x'].double()
        _f16_case_checks(c, ftz, f'attention {shape} iso={int(iso)}')
    for shape, iso in _f16_sla_cases():
        c = AC.sla_case(shape, False, 'f16', iso)
        ftz = AC.sla_eval(c['x'], c['w'], **dict(AC.sla_f16_kw(c['N']), operand='f16_ftz'))
        _f16_case_checks(c, ftz, f'SLA {shape} iso={int(iso)}')


def _f16_case_checks(c, ftz, what):
    for n, v in c['views'].items():
        b = c['bounds'][n]
        assert 5e-4 < b < AC.F16_BOUND_CEILING
        P.assert_views(c['emu32'], c['ref'], v, b, f'fp32 emulation, {what} per {n}')
        P.assert_close_to_emulation(c['emu32'], c['cmp'], c['emu32'], v, AC.close_margin(c), f'fp32 emulation, {what} per {n}')
        d = P.view_rels(ftz, c['cmp'], v).max().item()
        print(f'[underflow] {what} per {n}: flushed subnormals move the emulation by {d:.3e} (bound {b:.3e})')
        assert d < b / 3


def _stray_figures(c, evaluate, points, what):
    """One bf16 rounding at a time in the fp32 evaluation of the f16 emulation.  -> {point: (passes the reference bounds, smallest over
    the views of distance to the emulation / flip floor, rel-L2 of y)}"""
    out = {}
    x = c['x'].double()
    for pt in points:
        bad = evaluate(pt)
        passes = all(bool((P.view_rels(bad, c['ref'], v) < c['bounds'][n]).all()) for n, v in c['views'].items())
        for n, v in c['views'].items():
            print(f'[stray bf16 rounding] {what}, at {pt}, per {n}: worst group {P.view_rels(bad, c["ref"], v).max().item():.2e} from the reference '
                  f'(bound {c["bounds"][n]:.2e})')
        ratio = min(P.view_rels(bad, c['cmp'], v).max().item() / P.view_rels(c['emu32'], c['cmp'], v).max().item() for v in c['views'].values())
        out[pt] = (passes, ratio, P.rel(bad + x, c['ref'] + x))
        print(f'[stray bf16 rounding] {what}, at {pt}: {"inside" if passes else "REJECTED by"} the 3 x reference bounds; {ratio:.1f} x the flip floor from the '
              f'emulation; y rel-L2 {out[pt][2]:.2e}')
    return out


def test_one_stray_bf16_rounding_in_an_f16_kernel_is_seen_by_the_closeness_check_only():
    margin = AC.F16_CLOSE_MARGIN
    smallest = {'attention': float('inf'), 'sla': float('inf')}
    for shape, temporal in (((1, 16, 8, 8, 64), True), ((1, 32, 1, 3, 256), True)):           # attention_reg_kernel, attention_kernel
        c = AC.attn_case(shape, temporal, False, 'f16', False, False, True)
        ev = lambda pt: P.attention_block_fwd(c['x'], *c['w'], *shape[:4], temporal, emulate=True, q_scaled=True, operand='f16', stray=pt,
                                              dtype=torch.float32)[1].double() - c['x'].double()
        f = _stray_figures(c, ev, ('qkv', 'P', 'o'), f'attention {shape}')
        assert [pt for pt, r in f.items() if not r[0]] == ['qkv'], 'the reference bound sees a bf16 rounding of q | k | v only'
        assert all(r[1] >= 2 * margin['attention'] and r[2] < 4e-3 for r in f.values())
        smallest['attention'] = min(smallest['attention'], *[r[1] for r in f.values()])
    for shape in ((1, 1, 24, 24, 256), (1, 2, 64, 64, 64)):                                    # two chunks (ragged), eight chunks
        c = AC.sla_case(shape, False, 'f16')
        ev = lambda pt: AC.sla_eval(c['x'], c['w'], dtype=torch.float32, **dict(AC.sla_f16_kw(c['N']), stray=pt))
        f = _stray_figures(c, ev, ('ek', 'v', 'ctx', 'qs', 'o'), f'SLA {shape}')
        # SLA's emulation sits 3.5e-4 from the reference, half of attention's: its 3 x bound (1.1e-3) does reject one bf16 rounding anywhere
        # but at exp(k), whose error the softmax denominator largely divides out -- 3.8e-4, inside every bound and a few flip floors from the
        # emulation: the one rounding point neither check can see
        assert [pt for pt, r in f.items() if r[0]] == ['ek']
        assert all(r[1] >= 2 * margin['sla'] for pt, r in f.items() if pt != 'ek') and f['ek'][1] < 2 * margin['sla']
        assert all(r[2] < 4e-3 for r in f.values()), 'the whole-network style figure lets every one of them pass'
        smallest['sla'] = min(smallest['sla'], *[r[1] for pt, r in f.items() if pt != 'ek'])
    print(f'[stray bf16 rounding] smallest ratios: {smallest}; margins in use {margin}, {AC.F16_CLOSE_MARGIN_OF_CASE}')
    assert all(margin[k] <= smallest[k] / 2 for k in margin), 'a closeness margin above half the smallest single-stray ratio no longer sees it'
    for (kind, shape, iso), m in AC.F16_CLOSE_MARGIN_OF_CASE.items():              # a case with a margin of its own: against its OWN stray ratios
        assert kind == 'sla' and m <= smallest[kind] / 2
        c = AC.sla_case(shape, False, 'f16', iso)
        ev = lambda pt: AC.sla_eval(c['x'], c['w'], dtype=torch.float32, **dict(AC.sla_f16_kw(c['N']), stray=pt))
        f = _stray_figures(c, ev, ('v', 'ctx', 'qs', 'o'), f'SLA {shape}')
        assert all(r[1] >= 2 * m for r in f.values()), f'SLA {shape}: margin {m} no longer sees one stray rounding'
    # and the check itself rejects
    c = AC.attn_case((1, 16, 8, 8, 64), True, False, 'f16', False, False, True)
    bad = P.attention_block_fwd(c['x'], *c['w'], 1, 16, 8, 8, True, emulate=True, q_scaled=True, operand='f16', stray='P', dtype=torch.float32)[1].double() - c['x'].double()
    v = c['views']['sequence']
    P.assert_views(bad, c['ref'], v, c['bounds']['sequence'], 'stray P against the reference')
    with pytest.raises(AssertionError, match='from the emulation'):
        P.assert_close_to_emulation(bad, c['cmp'], c['emu32'], v, margin['attention'], 'stray P')
    nan = c['emu32'].clone()
    nan[0, 3, 2, 1] = float('nan')
    with pytest.raises(AssertionError, match='from the emulation'):
        P.assert_close_to_emulation(nan, c['cmp'], c['emu32'], v, margin['attention'], 'one NaN')


def test_f16_prologue_tile_bound_and_rounding_against_the_final_maximum():
    """tile_bound on an fp16-rounded activation: the flip floor is an eighth of the bf16 one; and the SLA emulation that rounds exp(k)
    against the final maximum (right for bf16, where rounding is relative at every magnitude) is further from the running-maximum
    emulation than the flip floor: in fp16 mode the kernel's order matters."""
    g = torch.Generator().manual_seed(12)
    C = 32
    y1 = torch.randn(2, 2, 16, 16, C, generator=g)
    kern2 = P.f16r(torch.randn(1, 3, 3, C, C, generator=g) / (9 * C) ** 0.5)
    out_of = lambda a: R.conv_1kk(a.double(), kern2.double(), None)
    b = {}
    for op in ('bf16', 'f16'):
        act = lambda dt: P.operand_rounding(op)(R.silu(y1.to(dt))).double()
        b[op] = P.tile_bound(act(torch.float32), act(torch.float64), out_of, operand=op)
    print(f'prologue tile bounds (bound, floor): {b}')
    assert b['f16'][1] < b['bf16'][1] / 4 and b['f16'][0] < 5e-3 / 8
    c = AC.sla_case((1, 2, 64, 64, 64), False, 'f16')
    final = AC.sla_eval(c['x'], c['w'], emulate=True, operand='f16')
    for n, v in c['views'].items():
        d, floor = P.view_rels(final, c['cmp'], v).max().item(), P.view_rels(c['emu32'], c['cmp'], v).max().item()
        print(f'[final-maximum emulation] per {n}: {d:.3e} from the running-maximum emulation, flip floor {floor:.3e}')
    assert P.view_rels(final, c['cmp'], P.frame_view).max().item() > P.view_rels(c['emu32'], c['cmp'], P.frame_view).max().item()


# ---- ResnetBlock time-MLP backward (tests/test_gpu_ss_backward.py) -----------------------------------------------------------------------
# The only other check of resblock_ss_bwd_kernel / resblock_ss_bwd_w_kernel is the whole-network gradient test: 5 x tol per tensor, 1e-3 on
# an f32 network and 0.3 on a bf16 one.  kernel_steps restates the two kernels' steps in fp64; one fault at a time goes in, and each proof
# states what the per-tensor figures of the faulted layer and the per-(layer, sample) bound on d(lin) make of it.

import _ss_backward_cases as SC

NET_F32, NET_BF16 = 1e-3, 0.3          # 5 x tol of tests/test_gpu_backward.py


def _ss_figures(c, out):
    """-> (worst rel of a dW / db / d gamma / d beta tensor, worst d(lin) group as (rel / bound, rel, bound, layer, sample))"""
    tens = max(P.rel(out[k][i], c['ref'][k][i]) for k in ('dW', 'db', 'dg', 'dbe') for i in range(len(c['layers'])))
    groups = [(r / c['b_dlin'][i][1][lab], r, c['b_dlin'][i][1][lab], i, lab) for i in range(len(c['layers']))
              for lab, r in P.slice_rels(out['dlin'][i], c['ref']['dlin'][i], c['sl'])]
    return tens, max(groups)


@pytest.mark.parametrize('name', ['corner', 't96_b9', 'ragged_kb8', 'offset'])
def test_ss_backward_kernel_steps_are_the_autograd_reference(name):
    c = SC.case(name)
    out = SC.kernel_steps(c['temb'], c['tensors'], c['lin_r'], c['dss_rows'])
    tens, (ratio, r, bound, i, lab) = _ss_figures(c, out)
    assert tens < 1e-11 and r < 1e-11 and P.rel(out['dtemb'], c['ref']['dtemb']) < 1e-11
    # ... and evaluated in fp32 they pass every bound (the bounds leave room for a correct fp32 evaluation in another order)
    out32 = SC.kernel_steps(c['temb'], c['tensors'], c['lin_r'], c['dss_rows'], dt=torch.float32)
    for i in range(len(c['layers'])):
        bound, sb = c['b_dlin'][i]
        P.assert_exact_products(out32['dlin'][i], c['ref']['dlin'][i], bound, c['sl'], sb, None, f'{name} fp32 steps d(lin) layer {i}')
        for k in ('dW', 'db', 'dg', 'dbe'):
            P.assert_exact_products(out32[k][i], c['ref'][k][i], c['b_par'][k][i], what=f'{name} fp32 steps {k} layer {i}')
    P.assert_exact_products(out32['dtemb'], c['ref']['dtemb'], c['b_dtemb'][0], c['sl'], c['b_dtemb'][1], None, f'{name} fp32 steps d(temb)')


def test_ss_backward_norm_eps_ten_times_too_small():
    """NORM_EPS = 1e-7 instead of 1e-6.  At the widths and embeddings of the table (var(lin) ~ 0.4) the fault moves rstd by 1e-6 of
    itself: the *.mlp.* tensors move by under 1e-6 -- three orders below the whole-network 1e-3 -- and d(lin) by 1.2e-6 of a (layer,
    sample), which the 2e-6 bound does NOT reject either: fp32 cannot tell the two epsilons apart there.  The `small_var` case exists for
    this fault: var(lin) ~ 1e-4, where the per-(layer, sample) bound rejects it by three orders (and where a per-tensor 1e-3 would see
    it too, had the parity networks such a layer)."""
    c = SC.case('t96_b19')
    bad = SC.kernel_steps(c['temb'], c['tensors'], c['lin_r'], c['dss_rows'], eps=R.NORM_EPS / 10)
    tens, (ratio, r, bound, i, lab) = _ss_figures(c, bad)
    print(f'[eps / 10, t96_b19] worst *.mlp.* tensor rel {tens:.3e} (whole-network bound {NET_F32:.0e}); worst d(lin) layer {i} {lab} rel {r:.3e} = '
          f'{ratio:.2f} x its bound {bound:.2e}')
    assert tens < NET_F32 / 100
    assert ratio < 1.0, 'the table shapes were not expected to tell 1e-7 from 1e-6'
    c = SC.case('small_var')
    var = min(v.double().var(1, unbiased=False).min().item() for v in c['lin_r'])
    bad = SC.kernel_steps(c['temb'], c['tensors'], c['lin_r'], c['dss_rows'], eps=R.NORM_EPS / 10)
    tens, (ratio, r, bound, i, lab) = _ss_figures(c, bad)
    print(f'[eps / 10, small_var: var(lin) >= {var:.1e}] worst tensor rel {tens:.3e}; worst d(lin) layer {i} {lab} rel {r:.3e} = {ratio:.0f} x its bound {bound:.2e}')
    assert ratio > 100
    for i in range(len(c['layers'])):
        with pytest.raises(AssertionError, match='slice'):
            P.assert_exact_products(bad['dlin'][i], c['ref']['dlin'][i], 10.0, c['sl'], c['b_dlin'][i][1], None, f'eps / 10, layer {i}, per sample only')


def test_ss_backward_m2_of_the_previous_sample():
    """Sample 11 of the 2048-column layer at B = 19 takes m2 from sample 10 (a stale red[] between two rounds of the `for b` loop).
    d(lin) of that (layer, sample) is off by 3e-2: four orders above its bound.  The layer's tensors: d gamma and d beta do not depend on
    m2; db moves by 4e-3 and dW by 7e-3 -- ABOVE 1e-3, so an f32 whole-network test does see this one (at B = 2, where one sample is half
    the sum, by 7e-2); the bf16 networks (0.3) do not, and the N-shape table runs in bf16 only."""
    c = SC.case('t96_b19')
    bad = SC.kernel_steps(c['temb'], c['tensors'], c['lin_r'], c['dss_rows'], stale_m2=(2, 11))
    per = {k: P.rel(bad[k][2], c['ref'][k][2]) for k in ('dW', 'db', 'dg', 'dbe')}
    tens, (ratio, r, bound, i, lab) = _ss_figures(c, bad)
    print(f'[stale m2, t96_b19 layer 2 sample 11] tensors {", ".join(f"{k} {v:.3e}" for k, v in per.items())} (whole-network bounds {NET_F32:.0e} f32, '
          f'{NET_BF16} bf16); d(lin) layer {i} {lab} rel {r:.3e} = {ratio:.0f} x its bound {bound:.2e}; d(temb) rel {P.rel(bad["dtemb"], c["ref"]["dtemb"]):.3e}')
    assert (i, lab) == (2, 'sample11') and ratio > 1000
    assert per['dg'] == 0 and per['dbe'] == 0 and NET_F32 < per['db'] < per['dW'] < NET_BF16 / 10      # visible at 1e-3 after all, not at 0.3
    for j in (0, 1):           # the other layers are untouched
        P.assert_exact_products(bad['dlin'][j], c['ref']['dlin'][j], c['b_dlin'][j][0], c['sl'], c['b_dlin'][j][1], None, f'stale m2: layer {j}')
    with pytest.raises(AssertionError, match=r'slice\(s\) over their bound, first sample11'):
        P.assert_exact_products(bad['dlin'][2], c['ref']['dlin'][2], 10.0, c['sl'], c['b_dlin'][2][1], None, 'stale m2, per sample only')
    # the network's own corner (B = 2): one sample is half of every sum
    c = SC.case('corner')
    bad = SC.kernel_steps(c['temb'], c['tensors'], c['lin_r'], c['dss_rows'], stale_m2=(1, 1))
    tens, (ratio, r, bound, i, lab) = _ss_figures(c, bad)
    print(f'[stale m2, corner layer 1 sample 1] worst tensor rel {tens:.3e}; d(lin) layer {i} {lab} rel {r:.3e} = {ratio:.0f} x its bound {bound:.2e}')
    assert NET_F32 < tens < NET_BF16 and ratio > 1000


# ---- the 8 x 8-patch weight-gradient cases (W < 16 with the prologue, and over a two-pointer concat) --------------------------------

import test_gpu_backward_forms as BF_


@pytest.mark.parametrize('name', ['l3_128_pro', 'ragged_7x9_pro', 'l3_concat_128_64', 'ragged_7x9_concat'])
def test_8x8_patch_cases_reject_a_dropped_patch_row_and_x1_read_through_x0(name):
    """The case's own bounds (built by _wg_case from the reference side, within their caps) pass the clean CPU evaluation and reject
    (a) one row of one 8 x 8 patch left out of the sum, and, for the concat cases, (b) the x1 channel block read through the x0 pointer."""
    c = BF_._wg_case(name)
    B, Fr, H, W, c0, c1, cout, k, stride, kind, pro, split = BF_.WG_CASES[name]
    dy = c['dy'].double()
    if pro:
        stats, gamma, beta, ss = c['pro']
        xin = P.bf16r(BF_._prologue(c['x0'], gamma, beta, ss, torch.float32)).double()      # the fp32-then-rounded activation: the bound's own floor
    else:
        xin = torch.cat((c['x0'], c['x1']), -1).double()
    ev = lambda x, d: BF_._conv_wgrad_ref(x, d, k, stride, kind)
    clean = ev(xin.float().double(), dy) if pro else ev(xin.float(), dy.float())
    P.assert_exact_products(clean, c['ref'], c['bound'], c['sl'], c['sb'], P._view3, f'{name}: clean CPU evaluation')
    dropped = dy.clone()
    dropped[B - 1, Fr - 1, H - 1, :8] = 0                        # the last row of the first 8 x 8 patch of the last frame
    with pytest.raises(AssertionError):
        P.assert_exact_products(ev(xin, dropped), c['ref'], c['bound'], c['sl'], c['sb'], P._view3, f'{name}: dropped patch row')
    if c1:
        swapped = torch.cat((c['x0'], c['x0'][..., :c1]), -1).double()
        with pytest.raises(AssertionError):
            P.assert_exact_products(ev(swapped, dy), c['ref'], c['bound'], c['sl'], c['sb'], P._view3, f'{name}: x1 read through the x0 pointer')
