"""Comparison helpers shared by the block-level parity tests of the backward and forward forms (tests/test_gpu_backward_forms.py,
tests/test_gpu_forward_forms.py, the bf16-store checks of tests/test_gpu_conv.py and tests/test_gpu_blocks.py) and by the CPU-only
sensitivity tests that prove they bite (tests/test_host_parity_helpers.py).  A plain module: nothing here is
collected, nothing here touches the GPU.

Where the numbers come from.  No bound in this file is derived from a kernel's output:

* exact-products forms (bf16-representable operands, fp32 accumulate, fp32 result): the project states 5e-6 for the weight
  gradient and 2e-6 for the forward under this contract (tests/test_gpu_conv_backward.py, tests/test_gpu_conv.py), measured at
  tensors of the size of one slice here.  `exact_products_bounds` keeps that figure where the arithmetic allows it and, for long
  reductions, replaces it by 8 x the error of the same contraction evaluated in fp32 on the CPU against fp64 (a CPU GEMM sums in a
  more favourable order than a chunked GPU sum; 8 x covers the difference).  A bound of 1e-4 or more is refused: one bf16 rounding
  is 2^-9 = 2e-3, and a test looser than two orders below that no longer separates a kernel fault from arithmetic.
* bf16 stores: the kernel rounds an fp32 value once, so an element is bf16(ref) or, when the fp32 error moved the value across a
  rounding boundary, its neighbour -- never further.  `assert_bf16_store` checks that per element and caps the share of elements
  that differ from bf16(ref) at all by 4 x the share of reference elements close enough to a rounding boundary to flip.
* attention / SLA cores round probabilities and score gradients to bf16 inside: `attn_core`, `sla_core` and `fused_attention` with
  emulate=True restate the kernels' rounding points in fp64; the per-group bound is 3 x the worst group of that
  emulation against the plain fp64 reference (the emulation cannot reproduce the MFMA summation order, hence the margin).
* fp16 operand mode (operand='f16' of the emulations, `f16r`): the same 3 x bound, and -- because one stray bf16 rounding in an fp16
  kernel stays inside it -- the distance to the emulation itself, in multiples of the distance between the emulation's fp32 and fp64
  evaluations on the CPU (`assert_close_to_emulation`); the margins and how they were fixed are in tests/_attention_cases.py.
"""
import math

import torch

BF16_ROUNDING = 2.0 ** -9          # half an ulp of bf16 relative to the binade's lower end
EXACT_CEILING = 1e-4               # an exact-products bound must stay below this (see above)
WGRAD_STATED = 5e-6                # the project's stated bound for the exact-products weight gradient
FWD_STATED = 2e-6                  # ... and for the exact-products forward / data gradient


def bf16r(t: torch.Tensor) -> torch.Tensor:
    """Round-trip through bf16 (round to nearest even), keeping the dtype."""
    return t.float().to(torch.bfloat16).to(t.dtype)


def f16r(t: torch.Tensor) -> torch.Tensor:
    """Round-trip through IEEE half (round to nearest even, gradual underflow below 2^-14, overflow to inf past 65504 + half an ulp),
    keeping the dtype: what v_cvt_f16_f32 / the (_Float16) casts of Mma<MODE_F16> do with subnormals enabled."""
    return t.float().to(torch.float16).to(t.dtype)


def f16r_ftz(t: torch.Tensor) -> torch.Tensor:
    """f16r with results below 2^-14 in magnitude (the fp16 subnormals) set to zero: hardware that flushes them."""
    r = f16r(t)
    return torch.where(r.abs() < 2.0 ** -14, torch.zeros_like(r), r)


ROUNDINGS = {'bf16': bf16r, 'f16': f16r, 'f16_ftz': f16r_ftz}


def operand_rounding(operand):
    """The rounding of an arithmetic mode's MFMA operand type: 'bf16' (the default everywhere), 'f16', or 'f16_ftz' (f16 with flushed
    subnormals, for the underflow proofs)."""
    return ROUNDINGS[operand]


def bf16_trunc(t: torch.Tensor) -> torch.Tensor:
    """bf16 by TRUNCATION of the fp32 bit pattern (what a kernel that drops the low 16 bits would store); keeps the dtype."""
    bits = t.float().contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).to(t.dtype)


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    """rel-L2 of a against the reference b."""
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-300)).item()


def bf16_ulp(t: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 numbers in the binade of each element (fp64; 0 for 0)."""
    t = t.double().abs()
    _, e = torch.frexp(t)                                   # t = m 2^e, m in [0.5, 1)
    ulp = torch.ldexp(torch.ones_like(t), e - 8)            # 8 significant bits
    return torch.where(t > 0, ulp, torch.zeros_like(t))


def f16_ulp(t: torch.Tensor) -> torch.Tensor:
    """Spacing of fp16 numbers in the binade of each element (fp64; 0 for 0): 11 significant bits, 2^-24 in the subnormal range."""
    t = t.double().abs()
    _, e = torch.frexp(t)
    ulp = torch.ldexp(torch.ones_like(t), (e - 11).clamp_min(-24))
    return torch.where(t > 0, ulp, torch.zeros_like(t))


# ---- slices -------------------------------------------------------------------------------------------------------------


def wgrad_slices(shape, tile=64):
    """Slices of a Flax weight gradient [..taps.., Cin, Cout]: one per (tap, 64-input-channel tile, 64-output-channel tile) -- the unit a
    weight-gradient workgroup owns.  -> list of (label, index tuple) on the tensor viewed as [taps, Cin, Cout]."""
    cin, cout = shape[-2], shape[-1]
    taps = 1
    for s in shape[:-2]:
        taps *= s
    out = []
    for t in range(taps):
        for ci in range(0, cin, tile):
            for co in range(0, cout, tile):
                out.append((f'tap{t}/ci{ci}/co{co}', (t, slice(ci, min(ci + tile, cin)), slice(co, min(co + tile, cout)))))
    return out


def sample_slices(shape):
    """One slice per sample (leading axis) of an activation tensor."""
    return [(f'sample{b}', (b,)) for b in range(shape[0])]


def _view3(t):
    return t.reshape(-1, t.shape[-2], t.shape[-1])


def slice_rels(got, ref64, slices, view=None):
    """rel-L2 per slice -> list of (label, rel)."""
    v = view or (lambda t: t)
    g, r = v(got.double()), v(ref64.double())
    return [(lab, rel(g[idx], r[idx])) for lab, idx in slices]


# ---- exact products ---------------------------------------------------------------------------------------------------------


def exact_products_bounds(ref32, ref64, slices=None, view=None, stated=WGRAD_STATED):
    """Bounds for a kernel under the exact-products contract, from the reference side alone: ref32 = the same contraction
    evaluated in fp32 on the CPU, ref64 in fp64, both on the same bf16-representable operands.
    -> (global bound, {slice label: bound}, global floor): bound = max(stated, 8 x floor), refused when >= 1e-4."""
    floor = rel(ref32, ref64)
    bound = max(stated, 8.0 * floor)
    assert bound < EXACT_CEILING, f'exact-products bound {bound:.2e} (floor {floor:.2e}) does not separate a kernel fault from arithmetic'
    sb = {}
    if slices:
        for lab, f in slice_rels(ref32, ref64, slices, view):
            sb[lab] = max(stated, 8.0 * f)
            assert sb[lab] < EXACT_CEILING, f'slice {lab}: bound {sb[lab]:.2e} too loose'
    return bound, sb, floor


def assert_exact_products(got, ref64, floor, slices=None, slice_floors=None, view=None, what=''):
    """rel-L2 of `got` against the fp64 reference (computed on the same bf16-representable operands) below `floor` (the bound from
    exact_products_bounds or a stated figure), and below `slice_floors[label]` (default: `floor`) on every slice, so that one bad tile
    cannot hide in the global norm.  Prints measured value and bound.  -> (global rel, worst slice label, worst slice rel)"""
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), f'{what}: non-finite output'
    r = rel(got, ref64)
    worst = ('-', 0.0, floor)
    bad = []
    for lab, sr in (slice_rels(got, ref64, slices, view) if slices else []):
        b = (slice_floors or {}).get(lab, floor)
        if sr / b > worst[1] / worst[2]:
            worst = (lab, sr, b)
        if not sr < b:
            bad.append((lab, sr, b))
    print(f'[exact] {what}: rel {r:.3e} (bound {floor:.3e}); worst slice {worst[0]} {worst[1]:.3e} (bound {worst[2]:.3e})')
    assert r < floor, f'{what}: rel-L2 {r:.3e} >= {floor:.3e}'
    assert not bad, f'{what}: {len(bad)} slice(s) over their bound, first {bad[0][0]}: {bad[0][1]:.3e} >= {bad[0][2]:.3e}'
    return r, worst[0], worst[1]


# ---- bf16 stores -----------------------------------------------------------------------------------------------------------


def bf16_flip_cap(ref64, fp32_floor):
    """Share of reference elements closer to a bf16 rounding boundary (the midpoint of two neighbouring bf16 numbers) than
    fp32_floor * |ref|, times 4: only those elements can legitimately be stored as the neighbour of bf16(ref)."""
    r = ref64.double()
    rb = bf16r(r)
    dist = (bf16_ulp(r) * 0.5 - (r - rb).abs()).abs()       # distance of ref to the nearer boundary of its rounding interval
    near = (dist < fp32_floor * r.abs()) & (r != 0)
    return 4.0 * near.double().mean().item()


def assert_bf16_store(got_bf16, ref64, fp32_floor, what=''):
    """For a kernel that rounds an fp32 result to bf16 once.  Every element within one bf16 ulp of bf16(ref) plus
    fp32_floor * rms(ref) (the absolute term is for elements that are small through cancellation) -- no element is exempt; and the
    share of elements that differ from bf16(ref) at all at most bf16_flip_cap(ref, fp32_floor).  A kernel that truncates, or rounds
    twice, differs on a large share and fails the cap although every element is within one ulp.  -> (share, cap, worst excess)"""
    assert got_bf16.shape == ref64.shape, (what, got_bf16.shape, ref64.shape)
    g = got_bf16.double()
    assert torch.isfinite(g).all(), f'{what}: non-finite output'
    r = ref64.double()
    rb = bf16r(r)
    rms = r.pow(2).mean().sqrt().item()
    tol = torch.maximum(bf16_ulp(rb), bf16_ulp(g)) + fp32_floor * rms
    excess = ((g - rb).abs() / tol).max().item()
    share = (g != rb).double().mean().item()
    cap = bf16_flip_cap(r, fp32_floor)
    print(f'[bf16 store] {what}: differing share {share:.3e} (cap {cap:.3e}); worst |got - bf16(ref)| = {excess:.3f} x (1 ulp + {fp32_floor:.1e} rms)')
    assert excess <= 1.0, f'{what}: an element is {excess:.2f} x (one ulp + floor) away from bf16(ref)'
    assert share <= cap, f'{what}: {share:.3e} of the elements differ from bf16(ref), cap {cap:.3e} (truncation or a second rounding?)'
    return share, cap, excess


# ---- groups ----------------------------------------------------------------------------------------------------------------


def per_group_rel(got, ref, group_shape):
    """rel-L2 per group: both tensors are viewed as [*group_shape, -1] (the caller permutes so that the group axes lead: attention
    sequences, (frame, head) pairs).  -> (worst rel, index of the worst group, tensor of all)"""
    n = 1
    for s in group_shape:
        n *= s
    g, r = got.double().reshape(n, -1), ref.double().reshape(n, -1)
    rels = (g - r).norm(dim=1) / (r.norm(dim=1) + 1e-300)
    i = int(rels.argmax())
    return rels[i].item(), i, rels.reshape(*group_shape)


def assert_groups(got, ref, group_shape, bound, what=''):
    w, i, _ = per_group_rel(got, ref, group_shape)
    print(f'[groups] {what}: worst group {i} rel {w:.3e} (bound {bound:.3e})')
    assert w < bound, f'{what}: group {i} rel-L2 {w:.3e} >= {bound:.3e}'
    return w


# ---- fp64 references and emulations of the attention cores --------------------------------------------------------------------


def _seq_view(rows, B, Fr, HW, heads, temporal, parts):
    """[rows][parts*heads*32] -> [nseq..., L, parts, heads, 32] with the token axis third from... (b, hw, f, ..) or (b, f, hw, ..)."""
    x = rows.reshape(B, Fr, HW, parts, heads, 32)
    return x.permute(0, 2, 1, 3, 4, 5) if temporal else x


def _seq_unview(t, temporal):
    """inverse of _seq_view for [b, s, L, heads, 32]-shaped results -> [rows][heads*32]"""
    t = t.permute(0, 2, 1, 3, 4) if temporal else t
    return t.reshape(-1, t.shape[-2] * 32)


def attn_core(qkv, d_o, B, Fr, HW, heads, temporal, emulate=False, round_out=False, dtype=torch.float64):
    """Attention core backward in `dtype` (fp64 = the reference), closed form (autodiff of softmax(q k^T / sqrt 32) v per sequence and head).
    emulate: probabilities P and score gradients dS are rounded to bf16 before the second products, as attn_core_bwd16_kernel
    does (q, k, v, d_o are expected bf16-representable already); round_out: o, dq, dk, dv rounded to bf16 (the io_bf16 store).
    -> o [rows][HD], dqkv [rows][3 HD]"""
    s = _seq_view(qkv.to(dtype), B, Fr, HW, heads, temporal, 3)
    q, k, v = s[..., 0, :, :], s[..., 1, :, :], s[..., 2, :, :]                     # [b, s, L, h, d]
    do = _seq_view(d_o.to(dtype), B, Fr, HW, heads, temporal, 1)[..., 0, :, :]
    sc = 1.0 / math.sqrt(32.0)
    S = torch.einsum('bsihd,bsjhd->bshij', q, k) * sc
    P = torch.softmax(S, -1)
    dP = torch.einsum('bsihd,bsjhd->bshij', do, v)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    if emulate:
        P, dS = bf16r(P), bf16r(dS)
    o = torch.einsum('bshij,bsjhd->bsihd', P, v)
    dv = torch.einsum('bshij,bsihd->bsjhd', P, do)
    dq = torch.einsum('bshij,bsjhd->bsihd', dS, k) * sc
    dk = torch.einsum('bshij,bsihd->bsjhd', dS, q) * sc
    outs = [_seq_unview(t, temporal) for t in (o, dq, dk, dv)]
    if round_out:
        outs = [bf16r(t) for t in outs]
    return outs[0], torch.cat(outs[1:], -1)


def sla_core(q, k, v, d_out, NF, N, emulate=False, round_out=False, dtype=torch.float64):
    """SpatialLinearAttention core backward in fp64, closed form, 8 heads x 32 (autodiff of out = ctx^T softmax_d(q),
    ctx = softmax_n(k)^T v per (frame, head)).  emulate: the rounding points of sla_bwd_a16_kernel / sla_bwd_b16_kernel:
    exp(k - max), softmax_d(q) rounded to bf16 for the two reductions; ctx, dctx, softmax_d(q), softmax_n(k) rounded to bf16 for the
    four per-pixel products (the elementwise factors stay unrounded).  -> o [rows][256], dqkv [rows][768]"""
    hs = lambda t: t.to(dtype).reshape(NF, N, 8, 32).permute(0, 2, 1, 3)            # [f, h, n, d]
    Q, K, V, D = hs(q), hs(k), hs(v), hs(d_out)
    rd = bf16r if emulate else (lambda t: t)
    qs = torch.softmax(Q, -1)
    ek = torch.exp(K - K.max(dim=2, keepdim=True).values)
    ksum = ek.sum(2, keepdim=True)
    ks = ek / ksum
    ctx = torch.einsum('fhnd,fhne->fhde', rd(ek), V) / ksum.transpose(2, 3)
    dctx = torch.einsum('fhnd,fhne->fhde', rd(qs), D)
    T = (ctx * dctx).sum(-1)                                                       # [f, h, d]
    o = torch.einsum('fhde,fhnd->fhne', rd(ctx), rd(qs))
    dqs = torch.einsum('fhde,fhne->fhnd', rd(ctx), D)
    dq = qs * (dqs - (qs * dqs).sum(-1, keepdim=True))
    dv = torch.einsum('fhde,fhnd->fhne', rd(dctx), rd(ks))
    dks = torch.einsum('fhde,fhne->fhnd', rd(dctx), V)
    dk = ks * (dks - T[:, :, None, :])
    back = lambda t: t.permute(0, 2, 1, 3).reshape(NF * N, 256)
    outs = [back(t) for t in (o, dq, dk, dv)]
    if round_out:
        outs = [bf16r(t) for t in outs]
    return outs[0], torch.cat(outs[1:], -1)


def fused_attention(x, dy, wqkv, bqkv, wo, B, Fr, HW, emulate=False, dtype=torch.float64):
    """Backward of y = MHA(x) + x over the frames of every pixel (8 heads x 32, C = 64) in fp64, closed form.  emulate: the rounding
    points of attn_bwd16x_kernel: q|k|v = bf16(x W + b), dO = bf16(dy Wo^T), the core as attn_core(emulate), o and dq|dk|dv stored
    as bf16 and read back as such for dx = dy + dqkv W^T (x, dy, W, Wo are expected bf16-representable already).
    -> dx [rows][64], o [rows][256], dqkv [rows][768]"""
    X, G = x.to(dtype).reshape(-1, 64), dy.to(dtype).reshape(-1, 64)
    W, Wo = wqkv.to(dtype), wo.to(dtype)
    rd = bf16r if emulate else (lambda t: t)
    qkv = rd(X @ W + bqkv.to(dtype))
    dO = rd(G @ Wo.t())
    o, dqkv = attn_core(qkv, dO, B, Fr, HW, 8, True, emulate=emulate, round_out=emulate, dtype=dtype)
    dx = G + dqkv @ W.t()
    return dx, o, dqkv


def group_bound(emulated, ref64, group_shape, margin=3.0):
    """Per-group bound for a kernel with bf16 rounding inside: margin x the worst group of the fp64 emulation of its rounding points
    against the plain fp64 reference."""
    return margin * per_group_rel(emulated, ref64, group_shape)[0]


# ---- small closed forms --------------------------------------------------------------------------------------------------------


def gn_stats_slab(y, groups=8):
    """GroupNorm statistics slab [B][32 slots][groups][2] (sum, sum of squares; slot 0 holds everything) of a channel-last tensor, fp64."""
    B, C = y.shape[0], y.shape[-1]
    yg = y.double().reshape(B, -1, groups, C // groups)
    stats = torch.zeros(B, 32, groups, 2, dtype=torch.float64)
    stats[:, 0, :, 0] = yg.sum(dim=(1, 3))
    stats[:, 0, :, 1] = (yg * yg).sum(dim=(1, 3))
    return stats


def slot_pattern(nslots, e_count, slot_stride):
    """Hand-made slots for the fixed-order pass: slot k holds (k + 1) + 3 (e % 11) in element e, the last element carries 1000 more
    and the last slot 7 more, the padding between slots -1e6 (never to be read).  Every sum is an integer below 2^24, so the
    expected result is exact in fp32 whatever the order: a dropped slot or a ragged tail is an exact integer mismatch.
    -> (part [nslots * slot_stride] fp32, expected sums [e_count] fp64)"""
    k = torch.arange(nslots, dtype=torch.float64)[:, None]
    e = torch.arange(e_count, dtype=torch.float64)[None, :]
    val = (k + 1) + 3 * (e % 11) + 1000 * (e == e_count - 1) + 7 * (k == nslots - 1)
    part = torch.full((nslots, slot_stride), -1e6, dtype=torch.float64)
    part[:, :e_count] = val
    exp = val.sum(0)
    assert exp.max() < 2 ** 24
    return part.reshape(-1).float(), exp


def split_columns(flat, cout, split):
    """[rows * cout] laid out [rows][cout] -> list of [rows][split] column blocks (the q|k|v split epilogue's targets)."""
    m = flat.reshape(-1, cout)
    return [m[:, i * split:(i + 1) * split].contiguous() for i in range(cout // split)]


# ---- forward forms -------------------------------------------------------------------------------------------------------------------


def e4m3r(t: torch.Tensor) -> torch.Tensor:
    """Round-trip through OCP e4m3 (round to nearest even, saturating at +-448: what v_cvt_pk_fp8_f32 does on gfx950), keeping the dtype."""
    return t.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float().to(t.dtype)


def have_e4m3() -> bool:
    try:
        return bool(torch.equal(e4m3r(torch.tensor([1.0, 1.06, 300.0, -0.3])), torch.tensor([1.0, 1.0, 288.0, -0.3125])))
    except Exception:
        return False


def attention_block_fwd(x, wqkv, bqkv, wo, bo, B, Fr, H, W, temporal, emulate=False, fp8=False, round_out=False, unmasked_pad=0,
                        q_scaled=False, dtype=torch.float64, operand='bf16', stray=None):
    """y = MHA(x) + x (8 heads x 32) over the frames of every pixel (temporal) or the pixels of every frame, in `dtype` (fp64 = the
    reference; fp32 = the floor of the f32-mode bounds), closed form.
    x [B, Fr, H, W, C]; wqkv [C, 768] = q | k | v column blocks, bqkv [768], wo [256, C], bo [C].
    emulate: the rounding points of attention_head_kernel (attention.hip): q, k, v = bf16(x W + b) -- the projections' fp32 accumulators
    become MFMA operands through pack_bf16x2 in Mma::mma16 (vdx_common.h:87-91; core_mma16 calls at attention.hip:1158-1159, 1181);
    the scores stay fp32 and are scaled inside the exponential (:1171); the probabilities are rounded to bf16 as the operand of the PV
    product (:1176 -> :1181); o is stored as bf16 (:1182-1183).  fp8: e4m3 instead of bf16 for q, k, v and P (mma16_fp8,
    vdx_common.h:95-99; o is still stored as bf16).  round_out: y rounded to bf16 (the io_bf16 store of the 1x1 out-projection).
    unmasked_pad > 0 (a FAULT, for the CPU proofs): that many padding keys with k = v = their bias take part in the softmax.

    The level-0 and narrow-level kernels of attention.hip in bf16 mode (tests/test_gpu_attention_groups.py) round at the same points:
    * attention_w_kernel: q, k = bias + W x in fp32 accumulators (:894-925) become operands of the score product through core_mma16
      (:930-931 -> Mma::mma16 / mma16_fp8, vdx_common.h:87-99); the mask and the softmax run in fp32 with 1 / sqrt(32) inside the exponent
      (:933-979); P and v are rounded as the operands of the PV product (:988); o is packed to bf16 -- also with the fp8 core -- as the B
      fragment of the out-projection (:994 -> :998), whose fp32 accumulators start from bo (:878-880); y = bf16(acc + x) (:1009-1012).
    * attention_h8_kernel: the same core (:578-579 scores, :584-606 softmax, :613 PV); o goes to LDS as bf16 (:617-618, or store4 :621) for
      the out-projection (:637-641); y = acc + x in fp32 (:666), or bf16(acc + x) on bf16 tensors (:660-663): round_out.  An fp32 x is
      rounded to bf16 at staging (:489): the tests feed bf16-representable x.
    * attention_reg_kernel: q = (acc + bias) * scale in fp32 BEFORE the operand rounding (:352-353 -> :359-360): q_scaled; P and v rounded
      at :376, o rounded as the operand of the out-projection's mma16 (:380); y fp32 (:394-396).
    * attention_kernel: q = bf16((acc + bias) * scale) (:140-141): q_scaled; k, v stored as bf16 (:143, :147-148), P stored as bf16
      (:186), o stored as bf16 (:199); y fp32 (:231-233).
    In f32 mode every one of them keeps fp32 throughout (Mma<MODE_F32>: f32 MFMA operands, 4-byte LDS elements): no rounding point, the
    bound is the exact-products kind (f32_group_bounds).
    q_scaled: q is multiplied by 1 / sqrt(32) before it is rounded (the scores are then not scaled again).

    operand='f16' (mode 'f16', Mma<MODE_F16>): fp16 mode reaches attention_reg_kernel (L <= 16) and attention_kernel (17..64 tokens) alone
    (launch_attn_m skips every attention_h8 / attention_w form, attention.hip:1267), and both round at the points listed above, every one
    through the mode's type:
    * attention_reg_kernel<2, TMA, false>: x staged with M::store4 (:288; exact for fp16-representable x); q = (acc + bias) * scale in fp32
      (:352-353), q, k rounded by pack_f16x2 inside M::mma16 (:359-360 -> vdx_common.h:135-139): q_scaled; P and v rounded as the operands
      of the PV product (:376, the same mma16); o rounded as the B operand of the out-projection's M::mma16 (:380), whose A operand is read
      back exactly by M::load_w4 (:379); y = acc + bo + x in fp32 (:394-396).
    * attention_kernel<2, LP, TMO>: x staged with M::store4 (:79); q = f16((acc + bias) * scale) (:140-141): q_scaled; k (:143) and v
      (M::store1, :147-148) stored as fp16; P = s * inv stored with M::store4 (:186); o stored with M::store4 (:199); every product is
      M::mma = v_mfma_f32_16x16x32_f16; y fp32 (:231-233).
    No rounding point of either instantiation is hard-coded bf16; the only bf16 conversions in their text (load4_f32_or_bf16 /
    store4_f32_or_bf16 with io_bf16) are unreachable: vdx_attention_forward_ex takes fp32 tensors, and the model refuses bf16 activation
    storage on an f16 handle.  y stays fp32: round_out does not exist in this mode.
    stray (a FAULT, for the CPU proofs): one of 'qkv', 'P', 'o' -- that rounding point alone rounds to bf16 instead of the operand type.
    -> (o [rows][256], y [B, Fr, H, W, C])"""
    dt = dtype
    C_ = x.shape[-1]
    X = x.to(dt).reshape(-1, C_)
    qkv = X @ wqkv.to(dt) + bqkv.to(dt)
    assert stray in (None, 'qkv', 'P', 'o') and not (fp8 and operand != 'bf16')
    rd_op = operand_rounding(operand)
    at = lambda point: (lambda t: t) if not emulate else e4m3r if fp8 and point != 'o' else bf16r if stray == point else rd_op
    rd = at('qkv')
    if q_scaled:
        qkv = torch.cat((qkv[:, :256] / math.sqrt(32.0), qkv[:, 256:]), 1)
    s = _seq_view(rd(qkv), B, Fr, H * W, 8, temporal, 3)
    q, k, v = s[..., 0, :, :], s[..., 1, :, :], s[..., 2, :, :]                     # [b, s, L, h, d]
    if unmasked_pad:
        pad = rd(bqkv.to(dt)).reshape(3, 8, 32)
        ext = lambda t, i: torch.cat((t, pad[i].expand(*t.shape[:2], unmasked_pad, 8, 32)), 2)
        k, v = ext(k, 1), ext(v, 2)
    S = torch.einsum('bsihd,bsjhd->bshij', q, k)
    if not q_scaled:
        S = S / math.sqrt(32.0)
    P = at('P')(torch.softmax(S, -1))
    o = at('o')(_seq_unview(torch.einsum('bshij,bsjhd->bsihd', P, v), temporal))
    return o, block_tail(o, x, wo, bo, round_out, dt, operand)


def block_tail(o, x, wo, bo=None, round_out=False, dtype=torch.float64, operand='bf16'):
    """y = o Wo (+ bo) + x of an attention / SLA block from the per-head output o [rows][256]; round_out: y rounded to bf16 (bf16 tensors
    exist in bf16 mode only: in f16 mode y is fp32 and there is no output rounding)."""
    assert not (round_out and operand != 'bf16'), 'f16 mode has no bf16 tensors: y is fp32'
    y = o.to(dtype) @ wo.to(dtype)
    if bo is not None:
        y = y + bo.to(dtype)
    y = y.reshape(x.shape) + x.to(dtype)
    return bf16r(y) if round_out else y


def running_max(K, tile, nsub):
    """K [f, h, n, d] -> the maximum the generic SLA context kernel holds when it rounds the exponentials of each pixel: over the
    `tile`-pixel sub-tiles of the pixel's chunk (nsub sub-tiles) up to and including its own (sla_ctx_kernel, sla.hip:138-144)."""
    f, h, n, d = K.shape
    nt = -(-n // tile)
    pad = torch.full((f, h, nt * tile - n, d), -float('inf'), dtype=K.dtype)
    tm = torch.cat((K, pad), 2).reshape(f, h, nt, tile, d).max(dim=3).values               # [f, h, nt, d]
    run = torch.cat([tm[:, :, c:c + nsub].cummax(dim=2).values for c in range(0, nt, nsub)], 2)
    return run.repeat_interleave(tile, dim=2)[:, :, :n]


def sla_block_fwd(x, wq, wk, wv, wo, B, Fr, H, W, emulate=False, round_out=False, dtype=torch.float64, fault=None, operand='bf16',
                  stray=None, running=None):
    """y = SpatialLinearAttention(x) + x (8 heads x 32) in `dtype` (fp64 = the reference; fp32 = the floor of the f32-mode bounds), closed
    form: ctx = softmax_n(k)^T v, out = ctx^T softmax_d(q) per
    (frame, head).  wq / wk / wv [C, 256], wo [256, C].  emulate: the rounding points of sla_head_kernel (sla.hip): exp(k - max) and v
    are rounded to bf16 as the operands of the context product (Mma::mma16 at :1023) while the softmax denominator sums the unrounded
    exponentials (:1006-1007) and divides the fp32 context (:1026-1033); ctx and softmax_d(q) are rounded to bf16 as the operands of
    the output product (:1070-1071); o is stored as bf16 (:1072-1073).  (The kernel rounds exp(k - running max); rounding is relative,
    so the final maximum gives the same relative error.)

    The narrow-level kernels in bf16 mode (tests/test_gpu_attention_groups.py) round at the same points:
    * sla_ctx8_kernel: exp2 of the k logits against the running maximum in fp32 (ctx8_softmax_step, :436), the denominator sums the
      unrounded exponentials (:439-441); e and v become bf16 as the operands of the context product (Mma::mma16 at :516); the fp32 context
      is divided by the denominator and stored ONCE in the storage type of ctxT, bf16 -- by the kernel itself when a frame is one chunk
      (:527-531), else by sla_combine_kernel from fp32 partials (:212-221) -- and read back as such: the rd(ctx) below, no second rounding.
    * sla_out8_kernel: ctx^T fragments read from ctxT as bf16 (:584); softmax_d(q) in fp32 (:634-651), rounded as the operand of
      Mma::mma16 (:660); o stored to LDS as bf16 (:661) for to_out (:674-681); y = acc + x in fp32 (:721-722) or bf16(acc + x) on bf16
      tensors (:705-708): round_out.
    * sla_out_w_kernel: ctx^T from the LDS image of ctxT, bf16 (:849); softmax_d(q) rounded at :883; o packed to bf16 as the B fragment
      of to_out (:887 -> :892); y = bf16(acc + x) (:903-906).
    * sla_ctx_kernel: e stored as bf16 (:156-157) while the sum takes the unrounded e (:158), v stored as bf16 (:171), context product
      :181-183, fp32 partials (:189) -> sla_combine_kernel as above.  sla_out_kernel: softmax_d(q) stored as bf16 (:309), ctxT read as
      bf16 (:320), o stored as bf16 (:329), y fp32 (:360-364).
    In f32 mode all of them keep fp32 throughout (ctxT included: M::store1 of Mma<MODE_F32>): the bound is f32_group_bounds.
    operand='f16' (mode 'f16', Mma<MODE_F16>): fp16 mode runs the generic kernels for EVERY channel count (launch_sla_m skips the
    one-wave-per-head forms, sla.hip:1218), and they round at the points above, every one through the mode's type:
    * sla_ctx_kernel<2>: x staged with M::store4 (:88; exact for fp16-representable x); e = exp(k - running max) stored with M::store1
      (:156-157) while the sum takes the unrounded e (:158); v stored with M::store1 (:171); context product M::mma (:181-183), rescaled
      by alpha in fp32 (:178); fp32 partials (:189-190).
    * sla_combine_kernel<2>: partials merged and divided by the denominator in fp32 (:212-219), ctx stored ONCE with M::store1 (:221).
    * sla_out_kernel<2, TMO>: x staged with M::store4 (:265); softmax_d(q) stored with M::store4 (:309); ctxT read as fp16 (:320); o
      stored with M::store4 (:329); to_out M::mma (:349); y = acc + x in fp32 (:360-364).
    No rounding point of the three is hard-coded bf16 (the io_bf16 loads / stores are unreachable: vdx_sla_forward takes fp32 tensors).
    Unlike bf16, fp16 rounding is relative only down to 2^-14: below, the spacing is 2^-24 absolute.  exp(k - max) of most pixels of a
    frame IS that small, so in this mode it matters which maximum the kernel subtracts before it rounds: `running`.
    running = (tile, nsub): the exponentials are rounded against the running maximum of sla_ctx_kernel (running_max) and rescaled to the
    final maximum unrounded, as the kernel's alpha (:142, :178) and the combine's exp(m_chunk - m) (:217) do in fp32.
    stray (a FAULT, for the CPU proofs): one of 'ek', 'v', 'ctx', 'qs', 'o' -- that rounding point alone rounds to bf16.
    fault (for the CPU proofs): ('drop_ctx', f, h, n0) -- pixels n0.. of frame f are missing from head h's context, numerator and
    denominator (a chunk partial the combine never adds); ('swap_ctx', f, n0, n1, f2) -- pixels n0..n1 of frame f take frame f2's context.
    -> (o [rows][256], y [B, Fr, H, W, C])"""
    dt = dtype
    C_, NF, N = x.shape[-1], B * Fr, H * W
    X = x.to(dt).reshape(-1, C_)
    hs = lambda t: t.reshape(NF, N, 8, 32).permute(0, 2, 1, 3)                      # [f, h, n, d]
    Q, K, V = hs(X @ wq.to(dt)), hs(X @ wk.to(dt)), hs(X @ wv.to(dt))
    assert stray in (None, 'ek', 'v', 'ctx', 'qs', 'o')
    rd_op = operand_rounding(operand)
    at = lambda point: (lambda t: t) if not emulate else bf16r if stray == point else rd_op
    rd = rd_op if emulate else (lambda t: t)
    qs = torch.softmax(Q, -1)
    kmax = K.max(dim=2, keepdim=True).values
    ek = torch.exp(K - kmax)
    if fault and fault[0] == 'drop_ctx':
        ek = ek.clone()
        ek[fault[1], fault[2], fault[3]:] = 0.0
    if running and emulate:
        assert not fault
        run = running_max(K, *running)
        ekr = at('ek')(torch.exp(K - run)) * torch.exp(run - kmax)
    else:
        ekr = at('ek')(ek)
    ctx = torch.einsum('fhnd,fhne->fhde', ekr, at('v')(V)) / ek.sum(2, keepdim=True).transpose(2, 3)
    o = torch.einsum('fhde,fhnd->fhne', at('ctx')(ctx), at('qs')(qs))
    if fault and fault[0] == 'swap_ctx':
        _, f, n0, n1, f2 = fault
        o[f, :, n0:n1] = torch.einsum('hde,hnd->hne', rd(ctx[f2]), rd(qs[f, :, n0:n1]))
    o = at('o')(o.permute(0, 2, 1, 3).reshape(NF * N, 256))
    return o, block_tail(o, x, wo, None, round_out, dt, operand)


def seq_head_groups(o, B, Fr, HW, temporal):
    """o [rows][256] -> [sequences, heads, L * 32]: the groups of a per-head attention output."""
    s = _seq_view(o, B, Fr, HW, 8, temporal, 1)[..., 0, :, :]                        # [b, s, L, h, d]
    return s.permute(0, 1, 3, 2, 4).reshape(s.shape[0] * s.shape[1], 8, -1)


def frame_head_groups(o, NF, N):
    """o [rows][256] -> [frames, heads, N * 32]."""
    return o.reshape(NF, N, 8, 32).permute(0, 2, 1, 3).reshape(NF, 8, -1)


# ---- group views of a block's branch y - x (tests/test_gpu_attention_groups.py) ---------------------------------------------------------
# A view maps a tensor to a LIST of 2-D tensors [groups, elements]: one row per group; a ragged last tile is a piece of its own (as the
# slices of slice_rels), so that it is a group like any other.  Every SLA view leads with the frame axis of a [NF, N, C] tensor and no
# group crosses a frame: the comparison may then walk the frames in chunks (`chunk`), which bounds the host memory of the largest case.


def isolate_heads(wo):
    """Head-isolating out-projection: Wo[h * 32 + d, c] = 0 unless c % 8 == h.  Channels c % 8 == h of the branch then depend on head h
    alone (8 / 4 / 16 channels per head at C = 64 / 32 / 128), which localises a fault to a (sequence, head) through the block's own ABI."""
    rows = torch.arange(wo.shape[0])[:, None] // 32
    cols = torch.arange(wo.shape[1])[None, :] % 8
    return wo * (rows == cols).to(wo.dtype)


def seq_head_view(temporal):
    """[B, F, H, W, C] -> one group per (sequence, head): the channels c % 8 == h of a sequence (isolate_heads)"""
    def view(t):
        B, Fr, H, W, C = t.shape
        s = t.reshape(B, Fr, H * W, C // 8, 8)
        s = s.permute(0, 2, 4, 1, 3) if temporal else s.permute(0, 1, 4, 2, 3)       # [b, sequence, head, token, C / 8]
        return [s.reshape(s.shape[0] * s.shape[1] * 8, -1)]
    return view


def frame_view(t):
    """[NF, N, C] -> one group per frame"""
    return [t.reshape(t.shape[0], -1)]


def frame_head_view(t):
    """[NF, N, C] -> one group per (frame, head): the channels c % 8 == h of a frame (isolate_heads)"""
    NF, N, C = t.shape
    return [t.reshape(NF, N, C // 8, 8).permute(0, 3, 1, 2).reshape(NF * 8, -1)]


def pixel_tile_view(tile=64):
    """[NF, N, C] -> one group per (frame, `tile` consecutive pixels): what one wave of sla_out_w_kernel / one pass of sla_out8_kernel
    owns; the ragged last tile of a frame is a group of its own (second piece)."""
    def view(t):
        NF, N, C = t.shape
        full = N // tile
        out = [t[:, :full * tile].reshape(NF * full, tile * C)] if full else []
        if N % tile:
            out.append(t[:, full * tile:].reshape(NF, -1))
        return out
    return view


def view_rels(got, ref, view, chunk=None):
    """rel-L2 of every group of `view` -> 1-D tensor (piece after piece; with `chunk`: per chunk of the leading axis, piece after piece)"""
    if chunk:
        return torch.cat([view_rels(got[i:i + chunk], ref[i:i + chunk], view) for i in range(0, ref.shape[0], chunk)])
    return torch.cat([per_group_rel(g, r, (r.shape[0],))[2] for g, r in zip(view(got.double()), view(ref.double()))])


def view_bound(emulated, ref64, view, chunk=None, margin=3.0):
    """group_bound over every piece of a view: margin x the worst emulated group."""
    if chunk:
        return max(view_bound(emulated[i:i + chunk], ref64[i:i + chunk], view, None, margin) for i in range(0, ref64.shape[0], chunk))
    return max(group_bound(e, r, (r.shape[0],), margin) for e, r in zip(view(emulated.double()), view(ref64.double())))


def f32_group_bounds(eval32, ref64, view, chunk=None, stated=FWD_STATED):
    """Per-group bounds of an f32-mode block: max(stated, 8 x the same formula evaluated in fp32 on the CPU against fp64), one figure per
    group, in the order of view_rels; refused at EXACT_CEILING."""
    b = (8.0 * view_rels(eval32, ref64, view, chunk)).clamp_min(stated)
    assert b.max().item() < EXACT_CEILING, f'f32 group bound {b.max().item():.2e} does not separate a kernel fault from arithmetic'
    return b


def assert_views(got, ref, view, bound, what='', chunk=None):
    """Every group of `view` below `bound` (one figure, or one per group in the order of view_rels); none is exempt, a non-finite group
    fails.  Prints the bound next to the worst group.  -> worst rel"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    r = view_rels(got, ref, view, chunk)
    b = bound if torch.is_tensor(bound) else torch.full_like(r, float(bound))
    assert b.shape == r.shape, (what, b.shape, r.shape)
    ratio = torch.where(torch.isfinite(r), r / b, torch.full_like(r, float('inf')))
    i = int(ratio.argmax())
    print(f'[groups] {what}: {r.numel()} groups, worst group {i} rel {r[i].item():.3e} (bound {b[i].item():.3e}; bounds {b.min().item():.3e} .. {b.max().item():.3e})')
    nbad = int((~(ratio < 1.0)).sum())
    assert nbad == 0, f'{what}: {nbad} group(s) over their bound, worst group {i} rel-L2 {r[i].item():.3e} >= {b[i].item():.3e}'
    return r[i].item()


def assert_close_to_emulation(got, emu64, emu32, view, margin, what='', chunk=None):
    """A kernel's output against the EMULATION of its rounding points, not against the plain reference: what can see a rounding of the
    wrong type (one stray bf16 rounding in an fp16 kernel stays inside 3 x the emulation's own distance from the reference, but sits far
    from the emulation).  emu64, emu32: the same emulation evaluated on the CPU in fp64 and in fp32 -- their distance is the floor a
    correct kernel has too: values computed in fp32 land on the other side of a rounding boundary for a few elements.  Every group of
    `view`: rel(got, emu64) <= max(FWD_STATED, margin x the worst group of rel(emu32, emu64)).  -> (worst rel, floor): worst / floor is the
    figure to report."""
    assert got.shape == emu64.shape == emu32.shape, (what, got.shape, emu64.shape, emu32.shape)
    floor = view_rels(emu32, emu64, view, chunk).max().item()
    bound = max(FWD_STATED, margin * floor)
    r = view_rels(got, emu64, view, chunk)
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float('inf')))
    i = int(r.argmax())
    print(f'[closeness] {what}: {r.numel()} groups, worst group {i} rel {r[i].item():.3e} to the emulation = {r[i].item() / floor:.2f} x the flip floor '
          f'{floor:.3e} (bound {margin:g} x = {bound:.3e})')
    nbad = int((~(r <= bound)).sum())
    assert nbad == 0, f'{what}: {nbad} group(s) further than {bound:.3e} from the emulation, worst group {i} at {r[i].item():.3e}'
    return r[i].item(), floor


def norm_bound(ref32, ref64, slices=None, stated=FWD_STATED):
    """Bound for an fp32 output of norm arithmetic (GroupNorm / LayerNorm / SiLU chains): max(stated, 8 x the same formula evaluated in
    fp32 on the CPU against fp64), globally and per slice; refused at 1e-4 or more.  -> (bound, {label: bound}, floor)"""
    return exact_products_bounds(ref32, ref64, slices, None, stated)


def spread_slots(slab, seed=0):
    """Sum-preserving split of a GroupNorm statistics slab [B][32][G][2] (everything in slot 0) over several of the 32 slots, as a
    producing conv's workgroups leave it: slot k gets an uneven share w_k (some slots stay empty), slot 31 the remainder."""
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(32, generator=g, dtype=torch.float64)
    w[torch.rand(32, generator=g) < 0.4] = 0.0
    w[0] = max(w[0].item(), 0.1)
    w = w / w.sum()
    tot = slab[:, 0]
    out = tot[:, None] * w[None, :, None, None]
    out[:, 31] += tot - out.sum(1)
    return out


def tile_slices(shape, tile=16):
    """One slice per (frame, tile x tile block) of a channel-last [B, F, H, W, C] tensor: the unit a conv workgroup owns."""
    B, Fr, H, W = shape[:4]
    return [(f'b{b}/f{f}/y{y}/x{x}', (b, f, slice(y, min(y + tile, H)), slice(x, min(x + tile, W))))
            for b in range(B) for f in range(Fr) for y in range(0, H, tile) for x in range(0, W, tile)]


def tile_rels(got, ref, tile=16):
    """rel-L2 per (frame, tile x tile block) of channel-last [B, F, H, W, C] tensors (H, W multiples of tile) -> [B, F, H/t, W/t]."""
    B, Fr, H, W, C_ = ref.shape
    v = lambda t: t.double().reshape(B, Fr, H // tile, tile, W // tile, tile, C_).permute(0, 1, 2, 4, 3, 5, 6).reshape(B, Fr, H // tile, W // tile, -1)
    g, r = v(got), v(ref)
    return (g - r).norm(dim=-1) / (r.norm(dim=-1) + 1e-300)


def tile_bound(act32_rounded, act64_rounded, out_of, tile=16, stated=FWD_STATED, bf16_out=False, operand='bf16'):
    """Per-tile bound of a fused-prologue conv: the kernel rounds the activation it recomputes to bf16; computed in fp32 it lands on the
    other side of a rounding boundary for a few elements.  floor = the worst tile of out_of(activation computed in fp32, rounded)
    against out_of(activation computed in fp64, rounded), not below the effect of ONE flipped element of rms size on a tile's output,
    bf16_ulp(rms) / ||activation of one tile||; bound = max(stated, 4 x floor).  bf16_out: the output is stored as bf16 -- one rounding
    moves an element by at most 2^-9 of itself, hence a tile's rel-L2 by at most 2^-9, which is added (a figure of the number format;
    a tile row scaled by 0.9 is 0.1 / sqrt(16) = 2.5e-2, an order above it).  operand='f16': the activation is rounded to fp16 (the caller
    rounds it so), one flipped element moves by an fp16 ulp; there are no bf16 outputs in that mode.  -> (bound, floor)"""
    assert not (bf16_out and operand != 'bf16')
    ulp = bf16_ulp if operand == 'bf16' else f16_ulp
    ref, alt = out_of(act64_rounded), out_of(act32_rounded)
    t = min(tile, ref.shape[2], ref.shape[3])
    floor = tile_rels(alt, ref, t).max().item()
    a = act64_rounded.double()
    one_flip = (ulp(a.pow(2).mean().sqrt()) / (a.pow(2).mean().sqrt() * math.sqrt(t * t * a.shape[-1]))).item()
    floor = max(floor, one_flip)
    return max(stated, 4.0 * floor) + (BF16_ROUNDING if bf16_out else 0.0), floor


def assert_tiles(got, ref, bound, tile=16, what=''):
    t = min(tile, ref.shape[2], ref.shape[3])
    r = tile_rels(got, ref, t)
    i = int(r.argmax())
    print(f'[tiles] {what}: worst (frame, {t}x{t} tile) #{i} rel {r.max().item():.3e} (bound {bound:.3e})')
    assert r.max().item() < bound, f'{what}: tile {i} rel-L2 {r.max().item():.3e} >= {bound:.3e}'
    return r.max().item()


def gn_sums(y, groups=8, dtype=torch.float64):
    """[B, ..., C] -> (sum y, sum |y|, sum y^2), each [B, groups], accumulated in `dtype`."""
    B, C_ = y.shape[0], y.shape[-1]
    yg = y.to(dtype).reshape(B, -1, groups, C_ // groups)
    return yg.sum(dim=(1, 3)), yg.abs().sum(dim=(1, 3)), (yg * yg).sum(dim=(1, 3))


def gn_stats_errors(s1, s2, ref64, groups=8):
    """|d sum y| / sum |y| and |d sum y^2| / sum y^2 per (sample, group) of sums s1, s2 [B, groups] against the fp64 tensor."""
    r1, ra, r2 = gn_sums(ref64, groups)
    return (s1.double() - r1).abs() / ra, (s2.double() - r2).abs() / r2


def assert_gn_stats(stats, ref64, ref32, tiles_per_sample, groups=8, what=''):
    """GroupNorm statistics epilogue of a conv: stats [B, groups, 2] (sum, sum of squares) against the fp64 conv output ref64, per
    (sample, group).  Bound = 8 x the worst (sample, group) of the same two figures for ref32, the conv AND its sums evaluated in fp32
    on the CPU.  Refused unless the bound is at most a quarter of the share one tile has in a sample's sums, 1 / tiles_per_sample: a
    tile credited to the wrong sample changes sum y^2 by about that share.  -> (worst e1, worst e2, bound 1, bound 2)"""
    f1, _, f2 = gn_sums(ref32.float(), groups, torch.float32)
    fe1, fe2 = gn_stats_errors(f1, f2, ref64, groups)
    b1, b2 = 8.0 * fe1.max().item(), 8.0 * fe2.max().item()
    share = 1.0 / tiles_per_sample
    assert max(b1, b2) <= 0.25 * share, f'{what}: statistics bound {max(b1, b2):.2e} is not below a quarter of one tile\'s share {share:.2e}'
    e1, e2 = gn_stats_errors(stats[..., 0], stats[..., 1], ref64, groups)
    assert torch.isfinite(stats).all(), f'{what}: non-finite statistics'
    print(f'[gn stats] {what}: sum {e1.max().item():.3e} (bound {b1:.3e}), sum of squares {e2.max().item():.3e} (bound {b2:.3e}); one tile = {share:.1e}')
    assert e1.max().item() <= b1, f'{what}: sum y off by {e1.max().item():.3e} of sum |y| at (sample, group) {divmod(int(e1.argmax()), groups)}, bound {b1:.3e}'
    assert e2.max().item() <= b2, f'{what}: sum y^2 off by {e2.max().item():.3e} at (sample, group) {divmod(int(e2.argmax()), groups)}, bound {b2:.3e}'
    return e1.max().item(), e2.max().item(), b1, b2
