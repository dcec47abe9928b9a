"""Case data of the forward-form parity tests: inputs (bf16-representable where the kernel contract says so), fp64 references through
oracle/unet3d_ref.py and the bounds derived from the reference side, built on the CPU and cached.  A plain module: nothing here is
collected, nothing here touches the GPU.  tests/test_gpu_forward_forms.py runs the kernels against these cases;
tests/test_host_parity_helpers.py injects faults into the same cases and shows that the same bounds reject them."""
import functools
import math

import torch

import _parity as P
from oracle import unet3d_ref as R

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * (i + 1) for i, k in enumerate(key)) % (2 ** 31))


def _bc(v, nd):
    """[B, n] -> [B, 1 x (nd - 2), n]"""
    return v.reshape(v.shape[0], *([1] * (nd - 2)), v.shape[-1])


# ---- attention heads --------------------------------------------------------------------------------------------------------------------

ATTN_HEADS_TEMPORAL = [
    # B, F, H, W, C
    (1, 16, 6, 6, 256),        # 36 sequences: chunks of 32 + 4, waves without a group
    (2, 10, 5, 7, 512),        # L = 10 masked; 35 sequences per sample: a group of 4 straddles the sample boundary, last group ragged (2)
    (1, 16, 17, 16, 256),      # 272 sequences = 9 chunks: the second round of the XCD-aware chunk decode
]
ATTN_HEADS_SPATIAL = [
    (1, 10, 8, 8, 512),        # LT = 4, 64 tokens, 10 sequences in chunks of 8 + 2
    (1, 3, 6, 6, 256),         # 36 tokens: the third key tile partly masked, the fourth empty
    (3, 5, 4, 4, 256),         # 16 tokens: LT = 1 on the spatial layout
]


def mha_weights(C, g, raw=False, operand='bf16'):
    """wqkv [C, 768] (q | k | v), bqkv [768], wo [256, C], bo [C]; the kernels bf16-representable (the packing rounds them), the biases fp32.
    raw: -> (those, the same with the kernels as drawn, before the rounding); operand='f16': rounded as pack_weights_kernel<MODE_F16> does"""
    rd = P.operand_rounding(operand)
    wqkv = torch.randn(C, 768, generator=g) / C ** 0.5 * 2
    bqkv = torch.randn(768, generator=g) * 0.2
    wo = torch.randn(256, C, generator=g) / 16
    bo = torch.randn(C, generator=g) * 0.2
    w = rd(wqkv), bqkv, rd(wo), bo
    return (w, (wqkv, bqkv, wo, bo)) if raw else w


def mha_oracle_params(wqkv, bqkv, wo, bo):
    C = wqkv.shape[0]
    p = {}
    for i, n in enumerate('qkv'):
        p[f'a.{n}.kernel'] = wqkv[:, i * 256:(i + 1) * 256].reshape(C, 8, 32).double()
        p[f'a.{n}.bias'] = bqkv[i * 256:(i + 1) * 256].reshape(8, 32).double()
    p['a.out.kernel'] = wo.reshape(8, 32, C).double()
    p['a.out.bias'] = bo.double()
    return p


def seq_groups(y, temporal):
    """y [B, F, H, W, C] -> [sequences, L * C]"""
    B, Fr, H, W, C = y.shape
    return y.permute(0, 2, 3, 1, 4).reshape(B * H * W, Fr * C) if temporal else y.reshape(B * Fr, H * W * C)


@functools.lru_cache(maxsize=4)
def attn_heads_case(shape, temporal, io16, fp8):
    B, Fr, H, W, C = shape
    g = _gen(*shape, temporal)
    x = P.bf16r(torch.randn(B, Fr, H, W, C, generator=g))
    w = mha_weights(C, g)
    o64, y64 = P.attention_block_fwd(x, *w, B, Fr, H, W, temporal)
    emu = not fp8 or P.have_e4m3()
    oe, ye = P.attention_block_fwd(x, *w, B, Fr, H, W, temporal, emulate=emu, fp8=fp8 and emu, round_out=io16 and emu)
    og = lambda t: P.seq_head_groups(t, B, Fr, H * W, temporal)
    nseq = og(o64).shape[0]
    bound_o = P.group_bound(og(oe), og(o64), (nseq, 8))
    bound_y = P.group_bound(seq_groups(ye, temporal), seq_groups(y64, temporal), (nseq,))
    if fp8 and not P.have_e4m3():                   # (no e4m3 casts on this CPU: oe / ye above are the plain reference; the project's stated figure)
        bound_o = bound_y = 1e-1
    print(f'[attention heads {shape} temporal={int(temporal)} io16={int(io16)} fp8={int(fp8)}] emulated rounding points -> bound per (sequence, head) '
          f'{bound_o:.3e}, per sequence of y {bound_y:.3e}')
    return dict(x=x, w=w, o64=o64, y64=y64, oe=oe, ye=ye, og=og, nseq=nseq, bound_o=bound_o, bound_y=bound_y)


# ---- long attention --------------------------------------------------------------------------------------------------------------------

ATTN_LONG = [
    # B, F, H, W (C = 128)
    (1, 2, 9, 9),              # 81 tokens: just past the limit of the register / LDS kernels
    (1, 1, 16, 16),            # 256 tokens: one row per thread
    (1, 2, 18, 18),            # 324 tokens: rows 256..323 run the second pass of `row += 256`
]


def long_core(qkv, nseq, L, dtype):
    """softmax(q k^T / sqrt 32) v per (sequence, head) from token-major qkv [rows][768] -> o [rows][256]"""
    s = qkv.to(dtype).reshape(nseq, L, 3, 8, 32)
    q, k, v = s[:, :, 0], s[:, :, 1], s[:, :, 2]
    S = torch.einsum('sihd,sjhd->shij', q, k) / math.sqrt(32.0)
    return torch.einsum('shij,sjhd->sihd', torch.softmax(S, -1), v).reshape(nseq * L, 256)


@functools.lru_cache(maxsize=4)
def attn_long_case(shape):
    B, Fr, H, W = shape
    C = 128
    g = _gen(*shape, 128)
    x = P.bf16r(torch.randn(B, Fr, H, W, C, generator=g))
    w = mha_weights(C, g)
    wqkv, bqkv, wo, bo = w
    nseq, L = B * Fr, H * W
    X = x.reshape(-1, C)
    qkv64 = X.double() @ wqkv.double() + bqkv.double()
    qkv32 = X @ wqkv + bqkv
    seq_sl = [(f'seq{s}', (slice(s * L, (s + 1) * L),)) for s in range(nseq)]
    b_qkv, sb_qkv, _ = P.exact_products_bounds(qkv32, qkv64, seq_sl, None, P.FWD_STATED)
    y64 = R.multihead_attention(mha_oracle_params(*w), 'a', x.double().reshape(B, Fr, L, C), 32).reshape(x.shape) + x.double()
    # bounds of the later stages, from the reference's own qkv and o (the test feeds each stage's REFERENCE the tensor the kernel read,
    # but takes no bound from a kernel output): the core per (sequence, head) at 8 x the same softmax in fp32; the out-projection
    # under the exact-products contract, on o as the mode stages it (bf16 mode rounds it to bf16)
    hg = lambda t: t.reshape(nseq, L, 8, 32).permute(0, 2, 1, 3).reshape(nseq * 8, -1)
    q32 = qkv64.float()                              # (the core reads fp32: the input's rounding to fp32 is not part of its error)
    o64 = long_core(q32, nseq, L, F64)
    core_floor = P.per_group_rel(hg(long_core(q32, nseq, L, F32)), hg(o64), (nseq * 8,))[0]
    b_core = max(P.FWD_STATED, 8.0 * core_floor)
    assert b_core < P.EXACT_CEILING, f'long attention {shape}: core bound {b_core:.2e} does not separate a kernel fault from arithmetic'
    y_sl = [(f'seq{s}', (s // Fr, s % Fr)) for s in range(nseq)]
    b_out = {}
    for mode in ('f32', 'bf16', 'f16'):
        oin = P.bf16r(o64.float()) if mode == 'bf16' else P.f16r(o64.float()) if mode == 'f16' else o64.float()
        yo64 = (oin.double() @ wo.double() + bo.double()).reshape(x.shape) + x.double()
        yo32 = (oin @ wo + bo).reshape(x.shape) + x
        b_out[mode] = P.exact_products_bounds(yo32, yo64, y_sl, None, P.FWD_STATED)[:2]
    return dict(x=x, w=w, nseq=nseq, L=L, qkv64=qkv64, seq_sl=seq_sl, b_qkv=b_qkv, sb_qkv=sb_qkv, y64=y64, hg=hg, b_core=b_core, y_sl=y_sl,
                b_out=b_out)


# ---- SLA heads -------------------------------------------------------------------------------------------------------------------------

SLA_HEADS = [
    # B, F, H, W, C
    (1, 10, 16, 16, 256),      # N = 256, TT = 4, frames in chunks of 8 + 2
    (9, 8, 8, 8, 256),         # 72 frames = 9 chunks
    (3, 3, 4, 4, 512),         # N = 16, TT = 1
    (1, 3, 4, 12, 256),        # N = 48: three 16-pixel tiles, TT = 1
]


@functools.lru_cache(maxsize=4)
def sla_weights(C, g, raw=False, operand='bf16'):
    """wq, wk, wv [C, 256] at 3 / sqrt C, wo [256, C] / 16, bf16-representable (operand='f16': fp16-representable).
    raw: -> (those, the same as drawn, before the rounding)"""
    drawn = tuple([torch.randn(C, 256, generator=g) / C ** 0.5 * 3 for _ in range(3)] + [torch.randn(256, C, generator=g) / 16])
    w = tuple(P.operand_rounding(operand)(t) for t in drawn)
    return (w, drawn) if raw else w


def sla_input(shape, g, operand='bf16'):
    """x [B, F, H, W, C], bf16-representable (operand='f16': fp16-representable), with a spike in the k logits of one pixel: the
    online-softmax rescale"""
    B, Fr, H, W, C = shape
    x = torch.randn(B, Fr, H, W, C, generator=g)
    x[:, :, H // 2, W // 2] *= 6
    return P.operand_rounding(operand)(x)


def sla_heads_case(shape, io16):
    B, Fr, H, W, C = shape
    g = _gen(*shape, 7)
    x = sla_input(shape, g)
    wq, wk, wv, wo = sla_weights(C, g)
    o64, y64 = P.sla_block_fwd(x, wq, wk, wv, wo, B, Fr, H, W)
    oe, ye = P.sla_block_fwd(x, wq, wk, wv, wo, B, Fr, H, W, emulate=True, round_out=io16)
    NF, N = B * Fr, H * W
    og = lambda t: P.frame_head_groups(t, NF, N)
    bound_o = P.group_bound(og(oe), og(o64), (NF, 8))
    bound_y = P.group_bound(ye.reshape(NF, -1), y64.reshape(NF, -1), (NF,))
    print(f'[sla heads {shape} io16={int(io16)}] emulated rounding points -> bound per (frame, head) {bound_o:.3e}, per frame of y {bound_y:.3e}')
    return dict(x=x, w=(wq, wk, wv, wo), o64=o64, y64=y64, oe=oe, ye=ye, og=og, NF=NF, N=N, bound_o=bound_o, bound_y=bound_y)


# ---- tails -----------------------------------------------------------------------------------------------------------------------------

TAIL16 = [
    # C, B, pixel shape
    (64, 2, (3, 5, 7)), (24, 2, (3, 5, 7)), (512, 2, (3, 5, 7)), (1024, 2, (3, 5, 7)),
    (64, 64, (1, 25, 44)),     # 1100 pixels per sample: 35 pixel groups over 32 workgroups, a ragged second pass
]
TAIL_MIXED = [(64, 2, (3, 5, 7)), (40, 2, (3, 5, 7))]
TAIL_HEAD = [(64, 64, 64, 2, (1, 12, 20)), (32, 32, 32, 2, (1, 12, 20))]        # c0, c1, C, B, pixel shape (240 pixels per sample)


def tail_formula(y2, r, gg, gb, lg, lb, dt, mean_rstd=None):
    """SiLU(GroupNorm(y2)) + LayerNorm_C(r) in dt; mean_rstd: per (sample, group) statistics to use instead of the tensor's own."""
    if mean_rstd is None:
        h = R.group_norm(y2.to(dt), gg.to(dt), gb.to(dt), 8)
    else:
        B, C = y2.shape[0], y2.shape[-1]
        mean, rstd = mean_rstd
        yg = y2.to(dt).reshape(B, -1, 8, C // 8)
        h = ((yg - mean.to(dt)[:, None, :, None]) * rstd.to(dt)[:, None, :, None]).reshape(y2.shape) * gg.to(dt) + gb.to(dt)
    return R.silu(h) + R.layer_norm(r.to(dt), lg.to(dt), lb.to(dt))


def norm_params(C, g):
    return (1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g), 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g))


@functools.lru_cache(maxsize=4)
def tail_case(C, B, shape, r16):
    """y2 bf16; r bf16 (r16) or fp32.  The slab is spread over several slots (a sum-preserving split)."""
    g = _gen(C, B, *shape, r16)
    y2 = P.bf16r(torch.randn(B, *shape, C, generator=g) * 2 + 0.5)
    y2[B - 1] = P.bf16r(y2[B - 1] * 1.7)                              # samples of different scale
    r = torch.randn(B, *shape, C, generator=g)
    if r16:
        r = P.bf16r(r)
    par = norm_params(C, g)
    slab = P.spread_slots(P.gn_stats_slab(y2), seed=C + B)
    ref64 = tail_formula(y2, r, *par, F64)
    ref32 = tail_formula(y2, r, *par, F32)
    sl = P.sample_slices(ref64.shape)
    bound, sb, floor = P.norm_bound(ref32, ref64, sl)
    return dict(y2=y2, r=r, par=par, slab=slab, ref64=ref64, ref32=ref32, sl=sl, bound=bound, sb=sb, store_floor=8.0 * floor)


@functools.lru_cache(maxsize=2)
def tail_head_case(c0, c1, C, B, shape):
    g = _gen(c0, c1, C, B, *shape)
    y2 = torch.randn(B, *shape, C, generator=g) * 2 + 0.5
    x0, x1 = torch.randn(B, *shape, c0, generator=g), torch.randn(B, *shape, c1, generator=g)
    y2[B - 1] *= 3.0                                                  # samples of different scale
    x0[B - 1] *= 0.4
    y2, x0, x1 = P.bf16r(y2), P.bf16r(x0), P.bf16r(x1)
    w = P.bf16r(torch.randn(c0 + c1, C, generator=g) / (c0 + c1) ** 0.5)
    rb = 0.3 * torch.randn(C, generator=g)
    par = norm_params(C, g)
    fw, fb = torch.randn(1, C, 1, generator=g) / C ** 0.5, torch.randn(1, generator=g)
    slab = P.spread_slots(P.gn_stats_slab(y2), seed=c0 + C)

    def head(dt):
        # resblock_tail_rc16_kernel<.., FIN>: the dot product takes the fp32 values of `out` (elementwise.hip: `o[]` goes into
        # `dot = fmaf(o[k], w, dot)` as computed; pack_bf16x2 is in the other branch) -- no bf16 rounding of out before the head
        r = torch.cat((x0, x1), -1).to(dt) @ w.to(dt) + rb.to(dt)
        out = tail_formula(y2, r, *par, dt)
        return out @ fw[0].to(dt) + fb.to(dt)

    ref64, ref32 = head(F64), head(F32)
    sl = P.sample_slices(ref64.shape)
    bound, sb, floor = P.norm_bound(ref32, ref64, sl)
    return dict(y2=y2, x0=x0, x1=x1, w=w, rb=rb, par=par, fw=fw, fb=fb, slab=slab, ref64=ref64, ref32=ref32, sl=sl, bound=bound, sb=sb)


# ---- final conv on bf16 input, init conv ------------------------------------------------------------------------------------------------

FINAL16 = ([(D, co, 1000) for D in (16, 32, 64, 128) for co in (1, 2, 3, 4)] +      # final_conv16_kernel<Cout>, every lane width; ragged
           [(24, 3, 1000),                    # final_conv_kernel: 8 channels per lane
            (64, 1, 4096 * 128 + 77)])        # the 4096-block cap: more than one pass, ragged


def row_slices(n, block):
    return [(f'rows{i}', (slice(i, min(i + block, n)),)) for i in range(0, n, block)]


@functools.lru_cache(maxsize=2)
def final_case(D, Cout, npix):
    g = _gen(D, Cout, npix)
    x = P.bf16r(torch.randn(npix, D, generator=g))
    kern = P.bf16r(torch.randn(1, D, Cout, generator=g))
    bias = torch.randn(Cout, generator=g)
    ref64 = R.conv_pointwise(x.double(), kern.double(), bias.double())
    ref32 = R.conv_pointwise(x, kern, bias)
    sl = row_slices(npix, 256 if npix < 10 ** 4 else 8192)
    bound, sb, _ = P.exact_products_bounds(ref32, ref64, sl, None, P.FWD_STATED)
    return dict(x=x, kern=kern, bias=bias, ref64=ref64, sl=sl, bound=bound, sb=sb)


INIT = [(1, 7, 64), (1, 3, 32), (1, 5, 12), (3, 7, 16)]           # Cin, K, Cout; Cin = 3: init_conv_kernel (bf16 y only)


@functools.lru_cache(maxsize=4)
def init_case(Cin, K, Cout):
    g = _gen(Cin, K, Cout)
    x = P.bf16r(torch.randn(2, Cin, 3, 20, 12, generator=g))      # partial 16 x 16 tiles on both axes
    kern = P.bf16r(torch.randn(1, K, K, Cin, Cout, generator=g) / K)
    bias = torch.randn(Cout, generator=g)
    xl = x.permute(0, 2, 3, 4, 1)
    ref64 = R.conv_1kk(xl.double(), kern.double(), bias.double())
    ref32 = R.conv_1kk(xl.contiguous(), kern, bias)
    sl = P.sample_slices(ref64.shape)
    bound, sb, _ = P.exact_products_bounds(ref32, ref64, sl, None, P.FWD_STATED)
    return dict(x=x, kern=kern, bias=bias, ref64=ref64, sl=sl, bound=bound, sb=sb)


# ---- scale / shift ----------------------------------------------------------------------------------------------------------------------

SS_WIDTHS = (64, 128, 2048)


@functools.lru_cache(maxsize=2)
def ss_case(temb_dim, B):
    """Layers of n = 64, 128 and 2048 in one table over one flat parameter buffer.  -> params, temb, layers, fp64 / fp32 references
    [layer][B, n] of the Linear (lin) and of its LayerNorm (ss), bounds per (layer, sample)."""
    g = _gen(temb_dim, B)
    temb = torch.randn(B, temb_dim, generator=g)
    temb *= (1.0 + 0.2 * torch.arange(B).float())[:, None]            # no two samples alike
    chunks, layers, off, out_off = [], [], 0, 0
    for n in SS_WIDTHS:
        W = torch.randn(temb_dim, n, generator=g) / temb_dim ** 0.5
        b, ga, be = 0.1 * torch.randn(n, generator=g), 1 + 0.1 * torch.randn(n, generator=g), 0.1 * torch.randn(n, generator=g)
        l = dict(n=n, out_off=out_off, W=W, b=b, g=ga, be=be)
        for key, t in (('w_off', W), ('b_off', b), ('g_off', ga), ('be_off', be)):
            l[key] = off
            chunks.append(t.reshape(-1))
            off += t.numel()
        out_off += n
        layers.append(l)
    params = torch.cat(chunks)

    def ref(dt):
        lin = [R.silu(temb.to(dt)) @ l['W'].to(dt) + l['b'].to(dt) for l in layers]
        return lin, [R.layer_norm(v, l['g'].to(dt), l['be'].to(dt)) for v, l in zip(lin, layers)]

    lin64, ss64 = ref(F64)
    lin32, ss32 = ref(F32)
    sl = P.sample_slices((B,))
    b_lin = [P.norm_bound(a, b, sl) for a, b in zip(lin32, lin64)]
    b_ss = [P.norm_bound(a, b, sl) for a, b in zip(ss32, ss64)]
    return dict(params=params, temb=temb, layers=layers, lin64=lin64, ss64=ss64, b_lin=b_lin, b_ss=b_ss, sl=sl)


def ss_rows(flat, layers, B):
    """flat ss / lin buffer -> [layer][B, n]"""
    return [flat[l['out_off'] * B:(l['out_off'] + l['n']) * B].reshape(B, l['n']) for l in layers]
