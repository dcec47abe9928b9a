"""Thin operator wrappers over the C ABI (used by the per-block parity tests and by debugging tools).
The network-level entry points live in unet3d.py / gaussian_diffusion.py."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L


def _mode(mode) -> int:
    return L.MODES[mode] if isinstance(mode, str) else int(mode)


def _is16(t) -> int:
    assert t.dtype in (torch.float32, torch.bfloat16)
    return int(t.dtype == torch.bfloat16)


def pack_conv_weights(kernel: torch.Tensor, mode) -> torch.Tensor:
    """kernel: Flax layout (..., kh, kw, Cin, Cout) / (1, Cin, Cout) / (Cin, Cout) -> packed byte tensor."""
    m = _mode(mode)
    cin, cout = kernel.shape[-2], kernel.shape[-1]
    taps = kernel.numel() // (cin * cout)
    k = kernel.contiguous().float()
    n = L.vdx_packed_conv_bytes(m, taps, cin, cout)
    out = torch.empty(n, dtype=torch.uint8, device=k.device)
    L.check(L.vdx_pack_conv_weights(m, L.ptr(k), L.ptr(out), taps, cin, cout, L.stream_ptr()))
    return out


def gn_stats_zeros(batch: int, groups: int, device) -> torch.Tensor:
    return torch.zeros(batch * L.GN_SLOTS * groups * 2, dtype=torch.float64, device=device)


def gn_stats_reduce(stats: torch.Tensor, batch: int, groups: int) -> torch.Tensor:
    """-> [batch, groups, 2] (sum, sumsq)."""
    return stats.view(batch, L.GN_SLOTS, groups, 2).sum(1)


def conv_forward(x0, packed_w, cout, *, mode, bias=None, x1=None, kind=0, k=3, stride=1,
                 in_stats=None, gamma=None, beta=None, groups=8, scale_shift=None,
                 out_stats=None, out_groups=8, y_bf16=False, res=None) -> torch.Tensor:
    """x0: [B,F,H,W,C0] channel-last fp32 -- or bf16 (bf16 mode: bf16 activation storage) -- (x1 likewise, concatenated on
    channels); y_bf16 selects a bf16 output tensor; res: optional residual [B,F,H,W,cout] (fp32 or bf16) added to the output."""
    B, Fr, H, W, c0 = x0.shape
    c1 = 0 if x1 is None else x1.shape[-1]
    if kind == 1:
        Ho, Wo = 2 * H, 2 * W
    else:
        Ho, Wo = -(-H // stride), -(-W // stride)
    x_bf16 = x0.dtype == torch.bfloat16
    assert x0.dtype in (torch.float32, torch.bfloat16) and (x1 is None or x1.dtype == x0.dtype)
    y = torch.empty(B, Fr, Ho, Wo, cout, dtype=torch.bfloat16 if y_bf16 else torch.float32, device=x0.device)
    d = L.ConvDesc()
    d.x_bf16, d.y_bf16 = int(x_bf16), int(bool(y_bf16))
    d.x0, d.x1, d.c0, d.c1 = L.ptr(x0), L.ptr(x1), c0, c1
    d.packed_w, d.bias, d.y, d.cout = L.ptr(packed_w), L.ptr(bias), L.ptr(y), cout
    d.batch, d.frames, d.h, d.w = B, Fr, H, W
    d.kind, d.kh, d.kw, d.stride = kind, k, k, stride
    d.in_stats, d.gamma, d.beta, d.groups = L.ptr(in_stats), L.ptr(gamma), L.ptr(beta), groups
    d.scale_shift = L.ptr(scale_shift)
    d.scale_shift_stride = 0 if scale_shift is None else scale_shift.shape[-1]
    d.out_stats, d.out_groups = L.ptr(out_stats), out_groups
    d.res, d.res_bf16 = L.ptr(res), int(res is not None and res.dtype == torch.bfloat16)
    L.check(L.vdx_conv_forward(_mode(mode), C.byref(d), L.stream_ptr()))
    return y


def resblock_tail(y2, r, stats, gn_gamma, gn_beta, ln_gamma, ln_beta, groups=8):
    B, C = y2.shape[0], y2.shape[-1]
    pix = y2.numel() // (B * C)
    out = torch.empty_like(y2)
    L.check(L.vdx_resblock_tail(L.ptr(y2), L.ptr(r), L.ptr(out), L.ptr(stats), L.ptr(gn_gamma), L.ptr(gn_beta), groups,
                                L.ptr(ln_gamma), L.ptr(ln_beta), C, B, pix, L.stream_ptr()))
    return out


def _pack_rc(rc_kernel):
    cin = rc_kernel.shape[0]
    wp = rc_kernel.t().contiguous().to(torch.bfloat16)           # [C][Cin], K-contiguous: the packed operand layout
    if cin % 64:                                                 # (rows padded to 64 input channels, as vdx_pack_conv_weights lays them out)
        wp = torch.nn.functional.pad(wp, (0, 64 - cin % 64)).contiguous()
    return wp


def resblock_tail_rc_bf16(y2, x0, x1, rc_kernel, rc_bias, stats, gn_gamma, gn_beta, ln_gamma, ln_beta, groups=8):
    """Tail with the 1x1 res_conv inside (bf16 tensors): y2 [B,...,C], x0 [B,...,C0], x1 [B,...,C1] or None (all torch.bfloat16),
    rc_kernel Flax [C0+C1, C] fp32 -> out bf16."""
    B, C = y2.shape[0], y2.shape[-1]
    pix = y2.numel() // (B * C)
    c0, c1 = x0.shape[-1], (0 if x1 is None else x1.shape[-1])
    wp = _pack_rc(rc_kernel)
    out = torch.empty_like(y2)
    L.check(L.vdx_resblock_tail_rc_bf16(L.ptr(y2), L.ptr(x0), None if x1 is None else L.ptr(x1), c0, c1, L.ptr(wp), L.ptr(rc_bias),
                                        L.ptr(out), L.ptr(stats), L.ptr(gn_gamma), L.ptr(gn_beta), groups, L.ptr(ln_gamma),
                                        L.ptr(ln_beta), C, B, pix, L.stream_ptr()))
    return out


def gn_silu_apply_bf16(y, stats, gn_gamma, gn_beta, scale_shift=None, groups=8):
    """Block prologue in place on a bf16 tensor y [B,...,C]: SiLU(GroupNorm(y) * (scale + 1) + shift); scale_shift fp32 [B, 2C] or None."""
    assert y.dtype == torch.bfloat16 and y.is_contiguous()
    B, C = y.shape[0], y.shape[-1]
    pix = y.numel() // (B * C)
    L.check(L.vdx_gn_silu_apply_bf16(L.ptr(y), L.ptr(stats), L.ptr(gn_gamma), L.ptr(gn_beta), None if scale_shift is None else L.ptr(scale_shift),
                                     0 if scale_shift is None else scale_shift.shape[-1], groups, C, B, pix, L.stream_ptr()))
    return y


def init_conv(x, kernel, bias):
    """x [B,C,F,H,W] (external layout); kernel Flax (1,k,k,C,D) -> [B,F,H,W,D]."""
    B, Cin, Fr, H, W = x.shape
    k, cout = kernel.shape[1], kernel.shape[-1]
    y = torch.empty(B, Fr, H, W, cout, dtype=torch.float32, device=x.device)
    L.check(L.vdx_init_conv(L.ptr(x), L.ptr(kernel.contiguous()), L.ptr(bias), L.ptr(y), B, Cin, Fr, H, W, cout, k, L.stream_ptr()))
    return y


def final_conv(x, kernel, bias):
    d, cout = kernel.shape[-2], kernel.shape[-1]
    npix = x.numel() // d
    y = torch.empty(*x.shape[:-1], cout, dtype=torch.float32, device=x.device)
    L.check(L.vdx_final_conv(L.ptr(x), L.ptr(kernel.contiguous()), L.ptr(bias), L.ptr(y), npix, d, cout, L.stream_ptr()))
    return y


def time_mlp(time, w1, b1, w2, b2, cond=None, null_cond_emb=None, cond_mask=None, null_all=False):
    B, dim = time.shape[0], w1.shape[0]
    cond_dim = 0 if cond is None else cond.shape[-1]
    temb = torch.empty(B, 4 * dim + cond_dim, dtype=torch.float32, device=w1.device)
    t32 = time.to(torch.int32).contiguous()
    cm = None if cond_mask is None else cond_mask.to(torch.uint8).contiguous()
    L.check(L.vdx_time_mlp(L.ptr(t32), L.ptr(w1), L.ptr(b1), L.ptr(w2), L.ptr(b2), dim, L.ptr(cond), L.ptr(null_cond_emb),
                           L.ptr(cm), int(null_all), cond_dim, L.ptr(temb), B, L.stream_ptr()))
    return temb


def pack_mha(pq, pk, pv, po, mode):
    """pq/pk/pv: (kernel (C,H,D), bias (H,D)); po: (kernel (H,D,C), bias (C))."""
    C_ = pq[0].shape[0]
    wqkv = torch.cat([p[0].reshape(C_, -1) for p in (pq, pk, pv)], dim=1).contiguous()
    bqkv = torch.cat([p[1].reshape(-1) for p in (pq, pk, pv)]).contiguous()
    wo = po[0].reshape(-1, C_).contiguous()
    return pack_conv_weights(wqkv, mode), bqkv, pack_conv_weights(wo, mode), po[1].contiguous()


def attention_forward(x, packed, heads, temporal, mode, fp8_core=False):
    B, Fr, H, W, C_ = x.shape
    y = torch.empty_like(x)
    wqkv, bqkv, wo, bo = packed
    L.check(L.vdx_attention_forward_ex(_mode(mode), L.ptr(x), L.ptr(y), L.ptr(wqkv), L.ptr(bqkv), L.ptr(wo), L.ptr(bo),
                                       B, Fr, H, W, C_, heads, int(temporal), int(bool(fp8_core)), L.stream_ptr()))
    return y


def attention_forward_bf16(x, packed, heads, temporal, fp8_core=False):
    """x: bf16 channel-last [B, F, H, W, C]; packed = pack_mha(..., 'bf16')."""
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    B, Fr, H, W, C_ = x.shape
    y = torch.empty_like(x)
    wqkv, bqkv, wo, bo = packed
    L.check(L.vdx_attention_forward_bf16(L.ptr(x), L.ptr(y), L.ptr(wqkv), L.ptr(bqkv), L.ptr(wo), L.ptr(bo),
                                         B, Fr, H, W, C_, heads, int(temporal), int(bool(fp8_core)), L.stream_ptr()))
    return y


_attn_fwd_bias = L._sig('vdx_attention_forward_bias', C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int] * 7 + [C.c_void_p])


def attention_forward_bias(x, packed, bias, heads, temporal, mode):
    """The attention block with a pre-softmax bias [heads, L, L] fp32 (the temporal blocks under Unet3D(temporal_pos_bias=True)).
    x: fp32 or bfloat16 (mode 'bf16') channel-last [B, F, H, W, C]; y has x's dtype."""
    B, Fr, H, W, C_ = x.shape
    Ltok = Fr if temporal else H * W
    bias = bias.to(x.device, torch.float32).contiguous()
    assert x.is_contiguous() and tuple(bias.shape) == (heads, Ltok, Ltok)
    y = torch.empty_like(x)
    wqkv, bqkv, wo, bo = packed
    L.check(_attn_fwd_bias(_mode(mode), L.ptr(x), L.ptr(y), _is16(x), L.ptr(wqkv), L.ptr(bqkv), L.ptr(wo), L.ptr(bo), L.ptr(bias),
                           B, Fr, H, W, C_, heads, int(temporal), L.stream_ptr()))
    return y


_attn_fwd_focus = L._sig('vdx_attention_forward_focus', C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int] * 8 + [C.c_void_p])
_attn_present = L._sig('vdx_attention_present_forward', C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 7 + [C.c_void_p])


def attention_forward_focus(x, packed, focus, heads, temporal, mode, bias=None):
    """The attention block with the per-sample focus-present mask (Unet3D(focus_present=True), a mixed batch): focus [n] bool / uint8
    with B % n == 0, sample b reads focus[b % n]; a flagged sample's tokens attend to themselves only.  bias: optional pre-softmax
    [heads, L, L] fp32 as attention_forward_bias.  x fp32 or bfloat16 (mode 'bf16') channel-last [B, F, H, W, C]; y has x's dtype."""
    B, Fr, H, W, C_ = x.shape
    Ltok = Fr if temporal else H * W
    if bias is not None:
        bias = bias.to(x.device, torch.float32).contiguous()
        assert tuple(bias.shape) == (heads, Ltok, Ltok)
    focus = (torch.as_tensor(focus) != 0).to(x.device, torch.uint8).contiguous()
    assert x.is_contiguous() and focus.dim() == 1 and B % focus.numel() == 0
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    wqkv, bqkv, wo, bo = packed
    L.check(_attn_fwd_focus(_mode(mode), L.ptr(x), L.ptr(y), _is16(x), L.ptr(wqkv), L.ptr(bqkv), L.ptr(wo), L.ptr(bo), L.ptr(bias),
                            L.ptr(focus), focus.numel(), B, Fr, H, W, C_, heads, int(temporal), L.stream_ptr()))
    return y


def attention_present_forward(x, packed, heads, temporal, mode, out=None):
    """The block of an all-focus-present batch in one launch: y = x + bo + Wo . rd(Wv x + bv) (attention_present_kernel).  x fp32 or
    bfloat16 (mode 'bf16') channel-last [B, F, H, W, C]; y (or `out`) has x's dtype."""
    B, Fr, H, W, C_ = x.shape
    assert x.is_contiguous()
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device) if out is None else out
    wqkv, bqkv, wo, bo = packed
    L.check(_attn_present(_mode(mode), L.ptr(x), L.ptr(y), _is16(x), L.ptr(wqkv), L.ptr(bqkv), L.ptr(wo), L.ptr(bo),
                          B, Fr, H, W, C_, heads, int(temporal), L.stream_ptr()))
    return y


def sla_forward(x, wq, wk, wv, wo, heads, mode):
    """wq/wk/wv: Flax (1, C, 256); wo: (1, 256, C)."""
    B, Fr, H, W, C_ = x.shape
    m = _mode(mode)
    y = torch.empty_like(x)
    ws = torch.empty(L.vdx_sla_workspace_bytes(m, B * Fr, H * W, heads), dtype=torch.uint8, device=x.device)
    pk = [pack_conv_weights(t, mode) for t in (wq, wk, wv, wo)]
    L.check(L.vdx_sla_forward(m, L.ptr(x), L.ptr(y), L.ptr(pk[0]), L.ptr(pk[1]), L.ptr(pk[2]), L.ptr(pk[3]), L.ptr(ws),
                              B, Fr, H, W, C_, heads, L.stream_ptr()))
    return y


def sla_forward_bf16(x, wq, wk, wv, wo, heads=8):
    """x: bf16 channel-last [B, F, H, W, C]; wq/wk/wv: Flax (1, C, 256); wo: (1, 256, C)."""
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    B, Fr, H, W, C_ = x.shape
    m = _mode('bf16')
    y = torch.empty_like(x)
    ws = torch.empty(L.vdx_sla_workspace_bytes(m, B * Fr, H * W, heads), dtype=torch.uint8, device=x.device)
    pk = [pack_conv_weights(t, 'bf16') for t in (wq, wk, wv, wo)]
    L.check(L.vdx_sla_forward_bf16(L.ptr(x), L.ptr(y), L.ptr(pk[0]), L.ptr(pk[1]), L.ptr(pk[2]), L.ptr(pk[3]), L.ptr(ws),
                                   B, Fr, H, W, C_, heads, L.stream_ptr()))
    return y


# ---- forward forms of the network (vdx.h: "Forward forms of the network"): the compositions and flags model.hip sets ----------------
# Outputs and scratch are NaN-filled before the call: a row the kernels do not write shows.


def _nan(shape, dtype, device):
    return torch.full(shape, float('nan'), dtype=dtype, device=device)


def attention_heads_forward(x, packed, temporal, fp8_core=False):
    """The wide-level attention block of a bf16-mode network (attention_head_kernel + 1x1 out-projection with residual).  x fp32 or
    bfloat16 [B, F, H, W, C]; packed = pack_mha(..., 'bf16').  -> (y like x, o [rows, 256] bfloat16: the core's output per head)"""
    B, Fr, H, W, C_ = x.shape
    assert x.is_contiguous()
    y = _nan(x.shape, x.dtype, x.device)
    o = _nan((B * Fr * H * W, 256), torch.bfloat16, x.device)
    assert o.numel() * 2 == L.vdx_attention_heads_scratch_bytes(B, Fr, H, W)
    wqkv, bqkv, wo, bo = packed
    L.check(L.vdx_attention_heads_forward(L.ptr(x), L.ptr(y), _is16(x), L.ptr(wqkv), L.ptr(bqkv), L.ptr(wo), L.ptr(bo), L.ptr(o), o.numel() * 2,
                                          B, Fr, H, W, C_, int(bool(temporal)), int(bool(fp8_core)), L.stream_ptr()))
    return y, o


def attention_long_forward(x, packed, heads, mode):
    """Spatial attention over more than 64 tokens (1x1 q|k|v conv, fp32 core, 1x1 out-projection with residual).
    -> (y like x, qkv [rows, 3 * heads * 32] fp32, o [rows, heads * 32] fp32: the scratch as the chain leaves it)"""
    B, Fr, H, W, C_ = x.shape
    assert x.is_contiguous()
    rows, HD = B * Fr * H * W, heads * 32
    y = _nan(x.shape, x.dtype, x.device)
    scr = _nan((rows * 4 * HD,), torch.float32, x.device)
    assert scr.numel() * 4 == L.vdx_attention_long_scratch_bytes(B, Fr, H, W, heads)
    wqkv, bqkv, wo, bo = packed
    L.check(L.vdx_attention_long_forward(_mode(mode), L.ptr(x), L.ptr(y), _is16(x), L.ptr(wqkv), L.ptr(bqkv), L.ptr(wo), L.ptr(bo), L.ptr(scr),
                                         scr.numel() * 4, B, Fr, H, W, C_, heads, L.stream_ptr()))
    return y, scr[:rows * 3 * HD].view(rows, 3 * HD), scr[rows * 3 * HD:].view(rows, HD)


def sla_heads_forward(x, wq, wk, wv, wo):
    """The wide-level SpatialLinearAttention block of a bf16-mode network (sla_head_kernel + 1x1 to_out with residual).  x fp32 or
    bfloat16 [B, F, H, W, C]; wq/wk/wv: Flax (1, C, 256); wo: (1, 256, C).  -> (y like x, o [rows, 256] bfloat16)"""
    B, Fr, H, W, C_ = x.shape
    assert x.is_contiguous()
    y = _nan(x.shape, x.dtype, x.device)
    o = _nan((B * Fr * H * W, 256), torch.bfloat16, x.device)
    pk = [pack_conv_weights(t, 'bf16') for t in (wq, wk, wv, wo)]
    L.check(L.vdx_sla_heads_forward(L.ptr(x), L.ptr(y), _is16(x), L.ptr(pk[0]), L.ptr(pk[1]), L.ptr(pk[2]), L.ptr(pk[3]), L.ptr(o), o.numel() * 2,
                                    B, Fr, H, W, C_, L.stream_ptr()))
    return y, o


def resblock_tail_ex(y2, r, stats, gn_gamma, gn_beta, ln_gamma, ln_beta, out_bf16=False, groups=8):
    """resblock_tail with a storage type per tensor: y2 / r fp32 or bfloat16 (their dtypes), out bfloat16 when out_bf16."""
    B, C_ = y2.shape[0], y2.shape[-1]
    pix = y2.numel() // (B * C_)
    out = _nan(y2.shape, torch.bfloat16 if out_bf16 else torch.float32, y2.device)
    L.check(L.vdx_resblock_tail_ex(L.ptr(y2), _is16(y2), L.ptr(r), _is16(r), L.ptr(out), int(bool(out_bf16)), L.ptr(stats), L.ptr(gn_gamma),
                                   L.ptr(gn_beta), groups, L.ptr(ln_gamma), L.ptr(ln_beta), C_, B, pix, L.stream_ptr()))
    return out


def resblock_tail_rc_head_bf16(y2, x0, x1, rc_kernel, rc_bias, stats, gn_gamma, gn_beta, ln_gamma, ln_beta, fin_kernel, fin_bias, groups=8):
    """resblock_tail_rc_bf16 with the one-channel final conv inside (fin_kernel Flax (1, C, 1)): -> [B, ..., 1] fp32."""
    B, C_ = y2.shape[0], y2.shape[-1]
    pix = y2.numel() // (B * C_)
    wp = _pack_rc(rc_kernel)
    fw = fin_kernel.reshape(-1).contiguous().float()
    assert fw.numel() == C_
    out = _nan((*y2.shape[:-1], 1), torch.float32, y2.device)
    L.check(L.vdx_resblock_tail_rc_head_bf16(L.ptr(y2), L.ptr(x0), L.ptr(x1), x0.shape[-1], x1.shape[-1], L.ptr(wp), L.ptr(rc_bias), L.ptr(stats),
                                             L.ptr(gn_gamma), L.ptr(gn_beta), groups, L.ptr(ln_gamma), L.ptr(ln_beta), C_, L.ptr(fw), L.ptr(fin_bias),
                                             L.ptr(out), B, pix, L.stream_ptr()))
    return out


def final_conv_ex(x, kernel, bias):
    """final_conv on x fp32 or bfloat16 [.., D]."""
    d, cout = kernel.shape[-2], kernel.shape[-1]
    npix = x.numel() // d
    y = _nan((*x.shape[:-1], cout), torch.float32, x.device)
    L.check(L.vdx_final_conv_ex(L.ptr(x), _is16(x), L.ptr(kernel.contiguous()), L.ptr(bias), L.ptr(y), npix, d, cout, L.stream_ptr()))
    return y


def init_conv_ex(x, kernel, bias, mode, y_bf16=False):
    """init_conv as the network launches it: mode 'bf16' with one input channel runs the MFMA kernel; y_bf16: bfloat16 output."""
    B, Cin, Fr, H, W = x.shape
    k, cout = kernel.shape[1], kernel.shape[-1]
    y = _nan((B, Fr, H, W, cout), torch.bfloat16 if y_bf16 else torch.float32, x.device)
    L.check(L.vdx_init_conv_ex(_mode(mode), L.ptr(x), L.ptr(kernel.contiguous()), L.ptr(bias), L.ptr(y), int(bool(y_bf16)), B, Cin, Fr, H, W, cout, k,
                               L.stream_ptr()))
    return y


def _ss_table(layers, device):
    """list of dicts (w_off, b_off, g_off, be_off, out_off, n) -> the vdx_ss_layer table as a uint8 device tensor"""
    tab = (L.SsLayer * len(layers))()
    for t, l in zip(tab, layers):
        t.w_off, t.b_off, t.g_off, t.be_off, t.out_off, t.n = l['w_off'], l['b_off'], l['g_off'], l['be_off'], l['out_off'], l['n']
    # (an empty table is still a valid pointer: the library refuses nlayers = 0 itself)
    return torch.frombuffer(bytearray(bytes(tab)) or bytearray(C.sizeof(L.SsLayer)), dtype=torch.uint8).to(device)


def resblock_scale_shift(params, temb, layers):
    """Every ResnetBlock's (scale, shift) rows in one launch pair.  params: flat fp32 buffer; temb [B, temb_dim]; layers: list of dicts
    (w_off, b_off, g_off, be_off, out_off, n), offsets in floats (out_off per sample).  -> (ss, lin): flat fp32 buffers, layer l /
    sample b at [out_off * B + b * n, + n)."""
    B, temb_dim = temb.shape
    raw = _ss_table(layers, params.device)
    total = max(l['out_off'] + l['n'] for l in layers) * B
    ss, lin = _nan((total,), torch.float32, params.device), _nan((total,), torch.float32, params.device)
    L.check(L.vdx_resblock_scale_shift(L.ptr(params), L.ptr(temb), L.ptr(raw), len(layers), L.ptr(ss), L.ptr(lin), temb_dim, B,
                                       max(l['n'] for l in layers), L.stream_ptr()))
    return ss, lin


# ---- backward building blocks ---------------------------------------------------------------------------


class WgradDesc(C.Structure):
    _fields_ = [('x0', C.c_void_p), ('x1', C.c_void_p), ('c0', C.c_int), ('c1', C.c_int), ('dy', C.c_void_p), ('cout', C.c_int),
                ('dw', C.c_void_p), ('batch', C.c_int), ('frames', C.c_int), ('h', C.c_int), ('w', C.c_int),
                ('kind', C.c_int), ('kh', C.c_int), ('kw', C.c_int), ('stride', C.c_int),
                ('in_stats', C.c_void_p), ('gamma', C.c_void_p), ('beta', C.c_void_p), ('groups', C.c_int),
                ('scale_shift', C.c_void_p), ('scale_shift_stride', C.c_int), ('bf16_operands', C.c_int)]


_pack_t = L._sig('vdx_pack_conv_weights_t', C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p])
_wgrad = L._sig('vdx_conv_backward_weights', C.c_int, [C.POINTER(WgradDesc), C.c_void_p])
_colsum = L._sig('vdx_colsum', C.c_int, [C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p])


def pack_conv_weights_t(kernel: torch.Tensor, mode) -> torch.Tensor:
    m = _mode(mode)
    cin, cout = kernel.shape[-2], kernel.shape[-1]
    taps = kernel.numel() // (cin * cout)
    k = kernel.contiguous().float()
    out = torch.empty(L.vdx_packed_conv_bytes(m, taps, cout, cin), dtype=torch.uint8, device=k.device)
    L.check(_pack_t(m, L.ptr(k), L.ptr(out), taps, cin, cout, L.stream_ptr()))
    return out


def conv_backward_weights(x0, dy, kshape, *, x1=None, kind=0, k=3, stride=1, in_stats=None, gamma=None, beta=None, groups=8,
                          scale_shift=None, dw=None, bf16_operands=False) -> torch.Tensor:
    B, Fr, H, W, c0 = x0.shape
    c1 = 0 if x1 is None else x1.shape[-1]
    cout = dy.shape[-1]
    if dw is None:
        dw = torch.zeros(kshape, dtype=torch.float32, device=x0.device)
    d = WgradDesc()
    d.x0, d.x1, d.c0, d.c1, d.dy, d.cout, d.dw = L.ptr(x0), L.ptr(x1), c0, c1, L.ptr(dy), cout, L.ptr(dw)
    d.batch, d.frames, d.h, d.w = B, Fr, H, W
    d.kind, d.kh, d.kw, d.stride = kind, k, k, stride
    d.in_stats, d.gamma, d.beta, d.groups = L.ptr(in_stats), L.ptr(gamma), L.ptr(beta), groups
    d.scale_shift = L.ptr(scale_shift)
    d.scale_shift_stride = 0 if scale_shift is None else scale_shift.shape[-1]
    d.bf16_operands = int(bool(bf16_operands))
    L.check(_wgrad(C.byref(d), L.stream_ptr()))
    return dw


def colsum(x: torch.Tensor) -> torch.Tensor:
    c = x.shape[-1]
    out = torch.zeros(c, dtype=torch.float32, device=x.device)
    L.check(_colsum(L.ptr(x), L.ptr(out), x.numel() // c, c, L.stream_ptr()))
    return out


_norm_bwd = L._sig('vdx_norm_act_backward', C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 9 + [C.c_int, C.c_int, C.c_long, C.c_void_p])


_norm_bwd_scr = L._sig('vdx_norm_act_backward_scratch_floats', C.c_size_t, [C.c_int, C.c_int, C.c_long])


def norm_act_backward(dact, y, stats, gamma, beta, groups=8, scale_shift=None, r=None, ln_gamma=None):
    """-> dict(dy, d_gamma, d_beta, dss, dr, d_ln_gamma, d_ln_beta)"""
    B, Cc = y.shape[0], y.shape[-1]
    pix = y.numel() // (B * Cc)
    dev = y.device
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    out = dict(dy=torch.empty_like(y), d_gamma=z(Cc), d_beta=z(Cc), dss=z(B, 2 * Cc) if scale_shift is not None else None,
               dr=torch.empty_like(y) if r is not None else None, d_ln_gamma=z(Cc) if r is not None else None,
               d_ln_beta=z(Cc) if r is not None else None)
    scratch = torch.empty(_norm_bwd_scr(Cc, B, pix), dtype=torch.float32, device=dev)       # uninitialised on purpose: nothing accumulates into it
    L.check(_norm_bwd(L.ptr(dact), L.ptr(y), L.ptr(out['dy']), L.ptr(stats), L.ptr(gamma), L.ptr(beta), groups, L.ptr(scale_shift),
                      0 if scale_shift is None else scale_shift.shape[-1], L.ptr(out['d_gamma']), L.ptr(out['d_beta']), L.ptr(out['dss']),
                      L.ptr(r), L.ptr(ln_gamma), L.ptr(out['dr']), L.ptr(out['d_ln_gamma']), L.ptr(out['d_ln_beta']), L.ptr(scratch),
                      Cc, B, pix, L.stream_ptr()))
    return out


_attn_core_bwd = L._sig('vdx_attention_core_backward_ex', C.c_int, [C.c_void_p] * 6 + [C.c_int] * 7 + [C.c_void_p])
_sla_scr = L._sig('vdx_sla_backward_scratch_floats', C.c_size_t, [C.c_int, C.c_int])
_sla_core_bwd = L._sig('vdx_sla_core_backward_ex', C.c_int, [C.c_void_p] * 9 + [C.c_int] * 4 + [C.c_void_p])


def attention_core_backward(qkv, d_o, B, Fr, H, W, heads, temporal, bf16_operands=False):
    """Attention core backward: qkv [rows][3*heads*32] (biased, q unscaled), d_o [rows][heads*32], fp32 -> o, dq, dk, dv.
    Up to 64 tokens per sequence, spatial or temporal; spatial sequences (temporal=False) also at every multiple of 64 up to 640 tokens
    (the tiled exact-fp32 core, three launches).  Any other length raises VdxError; bf16_operands only matters up to 16 tokens."""
    outs = [torch.empty_like(d_o) for _ in range(4)]
    L.check(_attn_core_bwd(L.ptr(qkv), L.ptr(d_o), *[L.ptr(t) for t in outs], B, Fr, H, W, heads, int(temporal), int(bool(bf16_operands)),
                           L.stream_ptr()))
    return outs      # o, dq, dk, dv


_attn_bwd_fused = L._sig('vdx_temporal_attention_backward_fused', C.c_int, [C.c_void_p] * 8 + [C.c_int] * 4 + [C.c_void_p])


def temporal_attention_backward_fused(x, dy, wqkv, bqkv, wo):
    """x, dy: fp32 (B, F, H, W, 64); wqkv (64, 768) = [Wq | Wk | Wv], bqkv (768,), wo (256, 64) Flax kernels.
    Returns dx (fp32), o (rows, 256) and dqkv (rows, 768) as bfloat16 (the bf16-mode backward of the widest level's temporal attention)."""
    B, Fr, H, W, C_ = x.shape
    assert C_ == 64 and wqkv.shape == (64, 768) and wo.shape == (256, 64)
    pw = pack_conv_weights(wqkv, 'bf16')
    pwo_t = pack_conv_weights_t(wo, 'bf16')
    rows = B * Fr * H * W
    o = torch.empty(rows, 256, dtype=torch.bfloat16, device=x.device)
    dqkv = torch.empty(rows, 768, dtype=torch.bfloat16, device=x.device)
    dx = torch.empty_like(x)
    bq = bqkv.contiguous().float()
    L.check(_attn_bwd_fused(L.ptr(x), L.ptr(dy), L.ptr(pw), L.ptr(bq), L.ptr(pwo_t), L.ptr(o), L.ptr(dqkv), L.ptr(dx), B, Fr, H, W, L.stream_ptr()))
    return dx, o, dqkv


def sla_core_backward(q, k, v, d_out, nframes, npix, heads=8, bf16_operands=False):
    outs = [torch.empty_like(q) for _ in range(4)]
    scr = torch.empty(_sla_scr(nframes, heads), dtype=torch.float32, device=q.device)
    L.check(_sla_core_bwd(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(d_out), *[L.ptr(t) for t in outs], L.ptr(scr), nframes, npix, heads,
                          int(bool(bf16_operands)), L.stream_ptr()))
    return outs      # o, dq, dk, dv


# ---- backward forms of the network (vdx.h: "Backward forms of the network"): the flag combinations model_bwd.hip sets ---------------



class WgradExDesc(C.Structure):
    _fields_ = [('x0', C.c_void_p), ('x1', C.c_void_p), ('c0', C.c_int), ('c1', C.c_int), ('x_bf16', C.c_int),
                ('dy', C.c_void_p), ('cout', C.c_int), ('dy_bf16', C.c_int),
                ('dw', C.c_void_p), ('dw1', C.c_void_p), ('dw2', C.c_void_p), ('split', C.c_int),
                ('db', C.c_void_p), ('db1', C.c_void_p), ('db2', C.c_void_p),
                ('batch', C.c_int), ('frames', C.c_int), ('h', C.c_int), ('w', C.c_int),
                ('kind', C.c_int), ('kh', C.c_int), ('kw', C.c_int), ('stride', C.c_int),
                ('in_stats', C.c_void_p), ('gamma', C.c_void_p), ('beta', C.c_void_p), ('groups', C.c_int),
                ('scale_shift', C.c_void_p), ('scale_shift_stride', C.c_int), ('bf16_operands', C.c_int),
                ('scratch', C.c_void_p), ('scratch_floats', C.c_size_t)]


WG_PART_FLOATS = L._sig('vdx_wgrad_scratch_floats', C.c_size_t, [])()          # the slot scratch model_bwd.hip hands every weight gradient
_wgrad_ex = L._sig('vdx_conv_backward_weights_ex', C.c_int, [C.POINTER(WgradExDesc), C.c_void_p])
_slot_sum = L._sig('vdx_slot_sum', C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
_norm_bwd_ex = L._sig('vdx_norm_act_backward_ex', C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6 +
                      [C.c_int, C.c_int, C.c_long, C.c_void_p])
_attn_core_bwd_io = L._sig('vdx_attention_core_backward_io', C.c_int, [C.c_void_p] * 4 + [C.c_int] * 9 + [C.c_void_p])
_attn_bwd_fused_ex = L._sig('vdx_temporal_attention_backward_fused_ex', C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.c_int] * 4 + [C.c_void_p])
_sla_core_bwd_io = L._sig('vdx_sla_core_backward_io', C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p])
_conv_rows = L._sig('vdx_conv_forward_rows', C.c_int, [C.c_int, C.POINTER(L.ConvDesc), C.c_int, C.c_int, C.c_void_p])
_final_bwd = L._sig('vdx_final_conv_backward', C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p])
_init_wgrad = L._sig('vdx_init_conv_backward_weights', C.c_int, [C.c_void_p] * 4 + [C.c_int] * 7 + [C.c_void_p, C.c_size_t, C.c_void_p])
_time_mlp_bwd = L._sig('vdx_time_mlp_backward', C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p])


def conv_backward_weights_ex(x0, dy, kshape, *, x1=None, kind=0, k=3, stride=1, in_stats=None, gamma=None, beta=None, groups=8,
                             scale_shift=None, bf16_operands=True, split=0, bias=False, scratch=None):
    """Weight gradient as the network launches it.  x0 / x1 / dy: fp32 or bfloat16 tensors (x_bf16 / dy_bf16 follow the dtypes);
    split > 0: returns one dW (and db) per column block of dy; bias: also the fused bias sums; scratch: float32 tensor for the
    per-workgroup slots (fixed-order sums) or None (float atomics).  -> (list of dW, list of db or None)"""
    B, Fr, H, W, c0 = x0.shape
    c1 = 0 if x1 is None else x1.shape[-1]
    cout = dy.shape[-1]
    assert x1 is None or x1.dtype == x0.dtype
    nb = cout // split if split else 1
    shp = list(kshape)
    if split:
        shp[-1] = split
    dws = [torch.zeros(shp, dtype=torch.float32, device=x0.device) for _ in range(nb)]
    dbs = [torch.zeros(shp[-1], dtype=torch.float32, device=x0.device) for _ in range(nb)] if bias else None
    d = WgradExDesc()
    d.x0, d.x1, d.c0, d.c1, d.x_bf16 = L.ptr(x0), L.ptr(x1), c0, c1, _is16(x0)
    d.dy, d.cout, d.dy_bf16 = L.ptr(dy), cout, _is16(dy)
    d.dw, d.dw1, d.dw2 = [L.ptr(dws[i]) if i < nb else 0 for i in range(3)]
    d.db, d.db1, d.db2 = [L.ptr(dbs[i]) if bias and i < nb else 0 for i in range(3)]
    d.split = split
    d.batch, d.frames, d.h, d.w = B, Fr, H, W
    d.kind, d.kh, d.kw, d.stride = kind, k, k, stride
    d.in_stats, d.gamma, d.beta, d.groups = L.ptr(in_stats), L.ptr(gamma), L.ptr(beta), groups
    d.scale_shift = L.ptr(scale_shift)
    d.scale_shift_stride = 0 if scale_shift is None else scale_shift.shape[-1]
    d.bf16_operands = int(bool(bf16_operands))
    d.scratch, d.scratch_floats = L.ptr(scratch), 0 if scratch is None else scratch.numel()
    L.check(_wgrad_ex(C.byref(d), L.stream_ptr()))
    return dws, dbs


def slot_sum(part, nslots, slot_stride, e_count, dsts, cout=0, split=0):
    """dsts[co // split][...] += sum over the slots in order (dsts: 1..3 float32 tensors, accumulated in place)."""
    p = [L.ptr(t) for t in dsts] + [0, 0]
    L.check(_slot_sum(L.ptr(part), nslots, slot_stride, e_count, cout, split, p[0], p[1], p[2], L.stream_ptr()))
    return dsts


def norm_act_backward_ex(dact, y, stats, gamma, beta, groups=8, scale_shift=None, r=None, ln_gamma=None, dy_bf16=False, deterministic=False):
    """norm_act_backward on the network's tensor types: y / r fp32 or bfloat16, dy written as bfloat16 when dy_bf16; deterministic:
    parameter gradients through the per-sample rows (dgp) instead of float atomics.  -> dict as norm_act_backward."""
    B, Cc = y.shape[0], y.shape[-1]
    pix = y.numel() // (B * Cc)
    dev = y.device
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    out = dict(dy=torch.empty(y.shape, dtype=torch.bfloat16 if dy_bf16 else torch.float32, device=dev), d_gamma=z(Cc), d_beta=z(Cc),
               dss=z(B, 2 * Cc) if scale_shift is not None else None,
               dr=torch.empty(y.shape, dtype=torch.float32, device=dev) if r is not None else None,
               d_ln_gamma=z(Cc) if r is not None else None, d_ln_beta=z(Cc) if r is not None else None)
    # both scratches uninitialised on purpose (NaN-filled: anything read before it is written shows)
    scratch = torch.full((_norm_bwd_scr(Cc, B, pix),), float('nan'), dtype=torch.float32, device=dev)
    dgp = torch.full((B, 4, Cc), float('nan'), dtype=torch.float32, device=dev) if deterministic else None
    L.check(_norm_bwd_ex(L.ptr(dact), L.ptr(y), _is16(y), L.ptr(out['dy']), int(bool(dy_bf16)), L.ptr(stats), L.ptr(gamma), L.ptr(beta), groups,
                         L.ptr(scale_shift), 0 if scale_shift is None else scale_shift.shape[-1], L.ptr(out['d_gamma']), L.ptr(out['d_beta']),
                         L.ptr(out['dss']), L.ptr(r), 0 if r is None else _is16(r), L.ptr(ln_gamma), L.ptr(out['dr']), L.ptr(out['d_ln_gamma']),
                         L.ptr(out['d_ln_beta']), L.ptr(scratch), L.ptr(dgp), Cc, B, pix, L.stream_ptr()))
    return out


def attention_core_backward_io(qkv, d_o, B, Fr, H, W, heads, temporal, bf16_operands=True, sentinel=None, pad_cols=0):
    """Interleaved form: qkv / d_o fp32 or bfloat16 (same dtype) -> o [rows][heads*32], dqkv [rows][3*heads*32 + pad_cols] of that dtype
    (the network's buffer has pad_cols = 0).  sentinel: value dqkv is pre-filled with; the pad columns must keep it.
    Lengths as attention_core_backward: above 64 tokens only spatial sequences of a multiple of 64 up to 640 tokens, fp32 tensors."""
    assert qkv.dtype == d_o.dtype
    HD = heads * 32
    o = torch.empty_like(d_o)
    dqkv = torch.empty(d_o.shape[0], 3 * HD + pad_cols, dtype=d_o.dtype, device=d_o.device)
    if sentinel is not None:
        dqkv.fill_(sentinel)
    L.check(_attn_core_bwd_io(L.ptr(qkv), L.ptr(d_o), L.ptr(o), L.ptr(dqkv), 3 * HD + pad_cols, _is16(qkv), B, Fr, H, W, heads, int(temporal),
                              int(bool(bf16_operands)), L.stream_ptr()))
    return o, dqkv


_attn_bias_scr = L._sig('vdx_attention_bias_backward_scratch_floats', C.c_size_t, [C.c_int, C.c_int])
_attn_core_bwd_bias = L._sig('vdx_attention_core_backward_bias', C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t] +
                             [C.c_int] * 7 + [C.c_void_p])


def attention_core_backward_bias(qkv, d_o, bias, B, Fr, H, W, heads, temporal, bf16_operands=True):
    """attention_core_backward_io with the pre-softmax bias [heads, L, L] fp32 -> o, dqkv (dtype of qkv), dbias [heads, L, L] fp32
    (the sum of dS over the sequences; deterministic: per-workgroup slots + an ordered second pass).  At most 64 tokens per sequence."""
    assert qkv.dtype == d_o.dtype
    HD = heads * 32
    Ltok = Fr if temporal else H * W
    bias = bias.to(qkv.device, torch.float32).contiguous()
    assert tuple(bias.shape) == (heads, Ltok, Ltok)
    o = torch.empty_like(d_o)
    dqkv = torch.empty(d_o.shape[0], 3 * HD, dtype=d_o.dtype, device=d_o.device)
    dbias = torch.zeros_like(bias)
    scratch = torch.empty(_attn_bias_scr(heads, Ltok), dtype=torch.float32, device=qkv.device)
    L.check(_attn_core_bwd_bias(L.ptr(qkv), L.ptr(d_o), L.ptr(o), L.ptr(dqkv), 3 * HD, _is16(qkv), L.ptr(bias), L.ptr(dbias), L.ptr(scratch),
                                scratch.numel(), B, Fr, H, W, heads, int(temporal), int(bool(bf16_operands)), L.stream_ptr()))
    return o, dqkv, dbias


_attn_core_bwd_focus = L._sig('vdx_attention_core_backward_focus', C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t] +
                              [C.c_void_p, C.c_int] + [C.c_int] * 7 + [C.c_void_p])


def attention_core_backward_focus(qkv, d_o, focus, B, Fr, H, W, heads, temporal, bf16_operands=True, bias=None):
    """attention_core_backward_bias with the per-sample focus-present mask focus [n] (B % n == 0) -> o, dqkv, dbias (None without bias).
    For a flagged sample exactly: dq == dk == 0, dv == dO, o == v, and nothing added to dbias.  At most 64 tokens per sequence."""
    assert qkv.dtype == d_o.dtype
    HD = heads * 32
    Ltok = Fr if temporal else H * W
    focus = (torch.as_tensor(focus) != 0).to(qkv.device, torch.uint8).contiguous()
    assert focus.dim() == 1 and B % focus.numel() == 0
    o = torch.empty(d_o.shape, dtype=d_o.dtype, device=d_o.device)
    dqkv = torch.empty(d_o.shape[0], 3 * HD, dtype=d_o.dtype, device=d_o.device)
    dbias = scratch = None
    if bias is not None:
        bias = bias.to(qkv.device, torch.float32).contiguous()
        assert tuple(bias.shape) == (heads, Ltok, Ltok)
        dbias = torch.zeros_like(bias)
        scratch = torch.empty(_attn_bias_scr(heads, Ltok), dtype=torch.float32, device=qkv.device)
    L.check(_attn_core_bwd_focus(L.ptr(qkv), L.ptr(d_o), L.ptr(o), L.ptr(dqkv), 3 * HD, _is16(qkv), L.ptr(bias), L.ptr(dbias), L.ptr(scratch),
                                 0 if scratch is None else scratch.numel(), L.ptr(focus), focus.numel(), B, Fr, H, W, heads, int(temporal),
                                 int(bool(bf16_operands)), L.stream_ptr()))
    return o, dqkv, dbias


def temporal_attention_backward_fused_ex(x, dy, wqkv, bqkv, wo):
    """temporal_attention_backward_fused with x fp32 or bfloat16 (bf16 activation storage)."""
    B, Fr, H, W, C_ = x.shape
    assert C_ == 64 and wqkv.shape == (64, 768) and wo.shape == (256, 64) and dy.dtype == torch.float32
    pw = pack_conv_weights(wqkv, 'bf16')
    pwo_t = pack_conv_weights_t(wo, 'bf16')
    rows = B * Fr * H * W
    o = torch.empty(rows, 256, dtype=torch.bfloat16, device=x.device)
    dqkv = torch.empty(rows, 768, dtype=torch.bfloat16, device=x.device)
    dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    bq = bqkv.contiguous().float()
    L.check(_attn_bwd_fused_ex(L.ptr(x), _is16(x), L.ptr(dy), L.ptr(pw), L.ptr(bq), L.ptr(pwo_t), L.ptr(o), L.ptr(dqkv), L.ptr(dx), B, Fr, H, W,
                               L.stream_ptr()))
    return dx, o, dqkv


def sla_core_backward_io(q, k, v, d_out, nframes, npix, heads=8, bf16_operands=True, sentinel=None, pad_cols=0):
    """Interleaved form: q, k, v, d_out fp32 or bfloat16 -> o [rows][256], dqkv [rows][768 + pad_cols] of that dtype."""
    o = torch.empty_like(q)
    dqkv = torch.empty(q.shape[0], 768 + pad_cols, dtype=q.dtype, device=q.device)
    if sentinel is not None:
        dqkv.fill_(sentinel)
    scr = torch.empty(_sla_scr(nframes, heads), dtype=torch.float32, device=q.device)
    L.check(_sla_core_bwd_io(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(d_out), L.ptr(o), L.ptr(dqkv), 768 + pad_cols, _is16(q), L.ptr(scr), nframes, npix, heads,
                             int(bool(bf16_operands)), L.stream_ptr()))
    return o, dqkv


def conv_dgrad_rows(dy, packed_wt, w_rows, w_row0, nrows, *, mode, k=3, res=None):
    """Data gradient of a stride-1 conv towards input channels [w_row0, w_row0 + nrows) of its w_rows input channels: packed_wt =
    pack_conv_weights_t of the whole kernel; dy fp32 or bfloat16; res (fp32) is added.  -> fp32 [B,F,H,W,nrows]"""
    B, Fr, H, W, cdy = dy.shape
    y = torch.empty(B, Fr, H, W, nrows, dtype=torch.float32, device=dy.device)
    d = L.ConvDesc()
    d.x_bf16, d.y_bf16 = _is16(dy), 0
    d.x0, d.x1, d.c0, d.c1 = L.ptr(dy), 0, cdy, 0
    d.packed_w, d.bias, d.y, d.cout = L.ptr(packed_wt), 0, L.ptr(y), nrows
    d.batch, d.frames, d.h, d.w = B, Fr, H, W
    d.kind, d.kh, d.kw, d.stride = 0, k, k, 1
    d.res, d.res_bf16 = L.ptr(res), 0
    L.check(_conv_rows(_mode(mode), C.byref(d), w_rows, w_row0, L.stream_ptr()))
    return y


def final_conv_backward(x, d_out, kernel, scratch=None):
    """x [.., D] fp32 or bfloat16, d_out [.., Cout], kernel Flax (1, D, Cout) -> dx [.., D], dw (D, Cout), db (Cout)."""
    D_, cout = kernel.shape[-2], kernel.shape[-1]
    npix = x.numel() // D_
    dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    dw = torch.zeros(D_, cout, dtype=torch.float32, device=x.device)
    db = torch.zeros(cout, dtype=torch.float32, device=x.device)
    L.check(_final_bwd(L.ptr(x), _is16(x), L.ptr(d_out), L.ptr(kernel.contiguous()), L.ptr(dx), L.ptr(dw), L.ptr(db), npix, D_, cout,
                       L.ptr(scratch), 0 if scratch is None else scratch.numel(), L.stream_ptr()))
    return dx, dw, db


def init_conv_backward_weights(x, dy, k, scratch=None):
    """x [B,C,F,H,W] (external layout), dy [B,F,H,W,D] -> dw (1,k,k,C,D), db (D)."""
    B, Cin, Fr, H, W = x.shape
    cout = dy.shape[-1]
    dw = torch.zeros(1, k, k, Cin, cout, dtype=torch.float32, device=x.device)
    db = torch.zeros(cout, dtype=torch.float32, device=x.device)
    L.check(_init_wgrad(L.ptr(x), L.ptr(dy), L.ptr(dw), L.ptr(db), B, Cin, Fr, H, W, cout, k, L.ptr(scratch),
                        0 if scratch is None else scratch.numel(), L.stream_ptr()))
    return dw, db


def time_mlp_backward(time, w1, b1, w2, b2, dtemb, cond_dim=0, cond_mask=None, null_all=False):
    """-> dw1, db1, dw2, db2, dnull (None without conditioning)."""
    B, dim = time.shape[0], w1.shape[0]
    t32 = time.to(torch.int32).contiguous()
    cm = None if cond_mask is None else cond_mask.to(torch.uint8).contiguous()
    outs = [torch.zeros_like(t) for t in (w1, b1, w2, b2)]
    dnull = torch.zeros(cond_dim, dtype=torch.float32, device=w1.device) if cond_dim else None
    L.check(_time_mlp_bwd(L.ptr(t32), L.ptr(w1), L.ptr(b1), L.ptr(w2), L.ptr(b2), dim, L.ptr(cm), int(null_all), cond_dim, L.ptr(dtemb),
                          *[L.ptr(t) for t in outs], L.ptr(dnull), B, L.stream_ptr()))
    return (*outs, dnull)


_ss_bwd = L._sig('vdx_resblock_scale_shift_backward', C.c_int, [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                                                   C.c_void_p])


def resblock_scale_shift_backward(params, grads, temb, layers, lin, dss, dtemb, scratch=None, scratch_floats=None):
    """Backward of resblock_scale_shift over `layers` (the forward's table, or any part of it), in place: dss (d(scale|shift), laid out
    like the forward's ss) becomes d(lin); grads (flat, laid out like params) and dtemb [B, temb_dim] are accumulated into.  scratch:
    float32 tensor for the per-layer d(temb) slots (fixed-order sum) or None (float atomics); scratch_floats: the capacity reported
    instead of scratch.numel()."""
    B, temb_dim = temb.shape
    raw = _ss_table(layers, params.device)
    cap = scratch_floats if scratch_floats is not None else (0 if scratch is None else scratch.numel())
    L.check(_ss_bwd(L.ptr(params), L.ptr(grads), L.ptr(temb), L.ptr(raw), len(layers), L.ptr(lin), L.ptr(dss), L.ptr(dtemb), temb_dim, B,
                    L.ptr(scratch), cap, L.stream_ptr()))


_loss_grad = L._sig('vdx_loss_grad', C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_long, C.c_int, C.c_void_p])
_adam_ema = L._sig('vdx_adam_ema_step', C.c_int, [C.c_void_p] * 5 + [C.c_long] + [C.c_float] * 4 + [C.c_long, C.c_float, C.c_int, C.c_float, C.c_void_p])


def loss_grad(eps_hat, noise, l2):
    """eps_hat channel-last [B,F,H,W,C], noise external [B,C,F,H,W] -> d(mean loss)/d(eps_hat), channel-last."""
    B, Cc = noise.shape[0], noise.shape[1]
    fhw = noise.numel() // (B * Cc)
    out = torch.empty_like(eps_hat)
    L.check(_loss_grad(L.ptr(eps_hat), L.ptr(noise), L.ptr(out), B, Cc, fhw, int(bool(l2)), L.stream_ptr()))
    return out


def adam_ema_step(p, g, m, v, ema, *, lr, b1, b2, eps, step_count, grad_scale=1.0, do_ema=True, ema_decay=0.995):
    """In place on p, m, v (and ema when do_ema)."""
    L.check(_adam_ema(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(ema), p.numel(), lr, b1, b2, eps, step_count, grad_scale, int(bool(do_ema)),
                      ema_decay, L.stream_ptr()))


_grad_accumulate = L._sig('vdx_grad_accumulate', C.c_int, [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p])
_grad_sqnorm_scratch = L._sig('vdx_grad_sqnorm_scratch_doubles', C.c_size_t, [])
_grad_sqnorm = L._sig('vdx_grad_sqnorm', C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p])
_adam_ema_clip = L._sig('vdx_adam_ema_step_clip', C.c_int, [C.c_void_p] * 5 + [C.c_long] + [C.c_float] * 4 + [C.c_long, C.c_float, C.c_int, C.c_float,
                                                            C.c_void_p, C.c_float, C.c_void_p, C.c_void_p])


def grad_accumulate(acc, g):
    """acc += g in place; flat fp32 tensors (or contiguous slices of them, at any 4-byte offset) of equal length."""
    assert acc.numel() == g.numel() and acc.dtype == g.dtype == torch.float32
    L.check(_grad_accumulate(L.ptr(acc), L.ptr(g), acc.numel(), L.stream_ptr()))


def grad_sqnorm(g, out=None):
    """sum of g^2 in double -> device tensor [1] (float64); g flat fp32 at any 4-byte offset."""
    assert g.dtype == torch.float32
    scratch = torch.empty(_grad_sqnorm_scratch(), dtype=torch.float64, device=g.device)
    out = torch.empty(1, dtype=torch.float64, device=g.device) if out is None else out
    L.check(_grad_sqnorm(L.ptr(g), g.numel(), L.ptr(scratch), L.ptr(out), L.stream_ptr()))
    return out


def adam_ema_step_clip(p, g, m, v, ema, sqnorm, max_grad_norm, *, lr, b1, b2, eps, step_count, grad_scale=1.0, do_ema=True, ema_decay=0.995):
    """adam_ema_step on g clipped to max_grad_norm by its global norm (sqnorm = grad_sqnorm(g), device); in place on p, m, v (and ema);
    returns the device float [1] of the pre-clip norm of grad_scale * g."""
    norm = torch.empty(1, dtype=torch.float32, device=p.device)
    L.check(_adam_ema_clip(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(ema), p.numel(), lr, b1, b2, eps, step_count, grad_scale, int(bool(do_ema)),
                           ema_decay, L.ptr(sqnorm), max_grad_norm, L.ptr(norm), L.stream_ptr()))
    return norm


# held-out evaluation (vdx.h: "Held-out evaluation"): tables = GaussianDiffusion's make_vlb_tables(T) as a [VLB_ROWS, T] float64 device tensor
_u64 = C.c_uint64
VLB_ROWS = L.VLB_ROWS
_vlb_scratch = L._sig('vdx_vlb_scratch_doubles', C.c_size_t, [C.c_int])
_vlb_noise = L._sig('vdx_vlb_noise', C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_void_p, _u64, _u64, C.c_void_p, C.c_int, C.c_long, C.c_void_p])
_vlb_terms = L._sig('vdx_vlb_terms', C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_void_p, _u64, _u64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                C.c_long, C.c_void_p])
_vlb_prior = L._sig('vdx_vlb_prior', C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_void_p])


def _vlb_check(x, tables):
    assert x.dtype == torch.float32 and x.dim() == 5 and tables.dtype == torch.float64 and tables.shape[0] == VLB_ROWS
    return x.shape[0], x.numel() // x.shape[0], tables.shape[1]


def vlb_noise(x, t, tables, *, noise=None, seed=0, draw=0, step_dev=None):
    """x [B,C,F,H,W] in [0, 1], t int32 [B] -> x_t = sqrt_ac[t] (2 x - 1) + sqrt(1 - ac[t]) eps with eps = `noise` or the Philox draw
    `draw` (+ *step_dev) of `seed`."""
    B, per, T = _vlb_check(x, tables)
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    L.check(_vlb_noise(L.ptr(x), L.ptr(out), L.ptr(t), L.ptr(tables), T, L.ptr(noise), int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw), L.ptr(step_dev),
                       B, per, L.stream_ptr()))
    return out


def vlb_terms(x, eps_hat, t, tables, *, noise=None, seed=0, draw=0, step_dev=None, clip=True):
    """x [B,C,F,H,W] in [0, 1], eps_hat channel-last [B,F,H,W,C], t int32 [B] -> float64 [B, 3] = (vb, mse, xstart_mse) per sample in
    bits/dim (vb) and per element (the two MSEs), with the noise of vlb_noise."""
    B, per, T = _vlb_check(x, tables)
    partial = torch.empty(_vlb_scratch(B), dtype=torch.float64, device=x.device)
    out = torch.empty(B, 3, dtype=torch.float64, device=x.device)
    L.check(_vlb_terms(L.ptr(x), L.ptr(eps_hat), L.ptr(t), L.ptr(tables), T, L.ptr(noise), int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw), L.ptr(step_dev),
                       int(bool(clip)), L.ptr(partial), L.ptr(out), B, x.shape[1], per, L.stream_ptr()))
    return out


def vlb_prior(x, tables):
    """x [B,C,F,H,W] in [0, 1] -> float64 [B]: KL(q(x_{T-1} | x0) || N(0, 1)) in bits/dim."""
    B, per, T = _vlb_check(x, tables)
    partial = torch.empty(_vlb_scratch(B), dtype=torch.float64, device=x.device)
    out = torch.empty(B, dtype=torch.float64, device=x.device)
    L.check(_vlb_prior(L.ptr(x), L.ptr(tables), T, L.ptr(partial), L.ptr(out), B, per, L.stream_ptr()))
    return out


# ---- learned variances (vdx.h: "Learned variances"): out2 = the network's channel-last output [B,F,H,W,2C], eps_hat | v ----

def p_sample_step_lv(x, out2, tables, *, level=None, step=0, step_dev=None, noise=None, seed=0, offset=0, dev_offset=None, clip=True,
                     post=(1.0, 0.0), out=None):
    """One reverse step with the model's variance.  x [B,C,F,H,W], tables float32 [6, S] (make_lv_tables(...)['step']); the level is
    `level` (int32 [B] on the device) or S - 1 - (step + *step_dev).  z = `noise` or Philox(seed, offset + *dev_offset).  out may be x."""
    assert x.dtype == torch.float32 and x.dim() == 5 and tables.dtype == torch.float32 and tables.shape[0] == 6
    B, per = x.shape[0], x.numel() // x.shape[0]
    out = torch.empty_like(x) if out is None else out
    L.check(L.vdx_p_sample_step_lv(L.ptr(x), L.ptr(out2), L.ptr(out), L.ptr(level), L.ptr(tables), tables.shape[1], int(step), L.ptr(step_dev),
                                   L.ptr(noise), int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset), L.ptr(dev_offset), int(bool(clip)), float(post[0]),
                                   float(post[1]), B, x.shape[1], per, L.stream_ptr()))
    return out


def hybrid_loss(x, noise, out2, t, tables64, *, pre=(1.0, 0.0), l2=False, vlb_weight=1.0, want_grad=True, weighted=False, iw=None):
    """mean |eps_hat - eps|^p + vlb_weight * mean vb (bits per element, eps_hat detached) -> (out float64 [2B + 3] = per-sample means
    (mse, vb) then the batch's (mse, vb, total), d_out float32 like out2 or None).  x [B,C,F,H,W] (x0 = x pre[0] + pre[1]), t int32 [B],
    tables64 float64 [LV_ROWS, T] (make_lv_tables(T)['tab64']).  weighted: through vdx_hybrid_loss_w with the importance weights iw
    (float64 [B], or None: its null form)."""
    assert x.dtype == torch.float32 and x.dim() == 5 and tables64.dtype == torch.float64 and tables64.shape[0] == L.LV_ROWS
    B, per = x.shape[0], x.numel() // x.shape[0]
    scratch = torch.empty(L.vdx_hybrid_scratch_doubles(B), dtype=torch.float64, device=x.device)
    out = torch.empty(2 * B + 3, dtype=torch.float64, device=x.device)
    d_out = torch.empty_like(out2) if want_grad else None
    if weighted or iw is not None:
        L.check(L.vdx_hybrid_loss_w(L.ptr(x), L.ptr(noise), L.ptr(out2), L.ptr(t), L.ptr(tables64), tables64.shape[1], float(pre[0]), float(pre[1]),
                                    int(bool(l2)), float(vlb_weight), int(bool(want_grad)), L.ptr(d_out), L.ptr(scratch), L.ptr(out), B, x.shape[1],
                                    per, L.ptr(iw), L.stream_ptr()))
        return out, d_out
    L.check(L.vdx_hybrid_loss(L.ptr(x), L.ptr(noise), L.ptr(out2), L.ptr(t), L.ptr(tables64), tables64.shape[1], float(pre[0]), float(pre[1]),
                              int(bool(l2)), float(vlb_weight), int(bool(want_grad)), L.ptr(d_out), L.ptr(scratch), L.ptr(out), B, x.shape[1], per,
                              L.stream_ptr()))
    return out, d_out


def vlb_terms_lv(x, out2, t, tables64, *, noise=None, seed=0, draw=0, step_dev=None, clip=True):
    """vlb_terms with the model's variance: out2 [B,F,H,W,2C], tables64 float64 [LV_ROWS, T] -> float64 [B, 3] = (vb, mse, xstart_mse)."""
    assert x.dtype == torch.float32 and x.dim() == 5 and tables64.dtype == torch.float64 and tables64.shape[0] == L.LV_ROWS
    B, per = x.shape[0], x.numel() // x.shape[0]
    partial = torch.empty(_vlb_scratch(B), dtype=torch.float64, device=x.device)
    out = torch.empty(B, 3, dtype=torch.float64, device=x.device)
    L.check(L.vdx_vlb_terms_lv(L.ptr(x), L.ptr(out2), L.ptr(t), L.ptr(tables64), tables64.shape[1], L.ptr(noise), int(seed) & 0xFFFFFFFFFFFFFFFF,
                               int(draw), L.ptr(step_dev), int(bool(clip)), L.ptr(partial), L.ptr(out), B, x.shape[1], per, L.stream_ptr()))
    return out


def final_conv_backward_wide(x, d_out, kernel, scratch=None):
    """final_conv_backward for up to 6 output channels (the eps | v head of a learned-variance network)."""
    D_, cout = kernel.shape[-2], kernel.shape[-1]
    npix = x.numel() // D_
    dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    dw = torch.zeros(D_, cout, dtype=torch.float32, device=x.device)
    db = torch.zeros(cout, dtype=torch.float32, device=x.device)
    L.check(L.vdx_final_conv_backward_wide(L.ptr(x), _is16(x), L.ptr(d_out), L.ptr(kernel.contiguous()), L.ptr(dx), L.ptr(dw), L.ptr(db), npix, D_, cout,
                                           L.ptr(scratch), 0 if scratch is None else scratch.numel(), L.stream_ptr()))
    return dx, dw, db


# ---- cascaded super-resolution (vdx.h: "Cascaded super-resolution"): xin [B,2C,F,S,S] = [ x_t | aug(up(2 lo - 1)) ] ----

def lowres_down(x, ft: int, fs: int):
    """The box mean of x [B,C,F,S,S] over ft x fs x fs blocks -> [B,C,F/ft,S/fs,S/fs] (fp32 sums in a fixed order; (1, 1): x's bits)."""
    assert x.dtype == torch.float32 and x.dim() == 5 and x.shape[3] == x.shape[4]
    B, Cc, Fr, S, _ = x.shape
    ft, fs = int(ft), int(fs)
    lo = torch.empty(B, Cc, Fr // max(ft, 1), S // max(fs, 1), S // max(fs, 1), dtype=torch.float32, device=x.device)
    L.check(L.vdx_lowres_down(L.ptr(x.contiguous()), L.ptr(lo), B, Cc, Fr, S, ft, fs, L.stream_ptr()))
    return lo


def lowres_input(lo, ft: int, fs: int, *, x0=None, t=None, noise=None, tables=None, aug_levels=None, seed=0, draw=0, pre=(1.0, 0.0), out=None):
    """One launch that builds the super-resolution network input xin [B,2C,F,S,S] from lo [B,C,F/ft,S/fs,S/fs] in [0, 1]: planes [C, 2C)
    = aug(up(2 lo - 1)); with x0 [B,C,F,S,S] (and t int32 [B], noise like x0) planes [0, C) = vdx_q_sample's x_t on x0 pre[0] + pre[1],
    without x0 they are left as they are (zeros in a fresh tensor).  tables = (sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod),
    float32 [T] on the device: needed with x0 or aug_levels.  aug_levels int32 [B] on the device (-1 = none for that sample): the noise is
    Philox(seed, draw) in randn's layout.  out: an xin to write into."""
    assert lo.dtype == torch.float32 and lo.dim() == 5 and lo.shape[3] == lo.shape[4]
    B, Cc, f, s, _ = lo.shape
    ft, fs = int(ft), int(fs)
    Fr, S = f * ft, s * fs
    if out is None:
        out = (torch.empty if x0 is not None else torch.zeros)(B, 2 * Cc, Fr, S, S, dtype=torch.float32, device=lo.device)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, 2 * Cc, Fr, S, S)
    if x0 is not None:
        assert tuple(x0.shape) == (B, Cc, Fr, S, S) and tuple(noise.shape) == tuple(x0.shape) and t.dtype == torch.int32
    if aug_levels is not None:
        assert aug_levels.dtype == torch.int32 and tuple(aug_levels.shape) == (B,)
    sa, sm = (None, None) if tables is None else tables
    L.check(L.vdx_lowres_input(L.ptr(x0), L.ptr(t), L.ptr(noise), L.ptr(lo), L.ptr(aug_levels), L.ptr(out), L.ptr(sa), L.ptr(sm),
                               0 if sa is None else sa.numel(), int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFFFFFFFFFF, float(pre[0]),
                               float(pre[1]), B, Cc, Fr, S, ft, fs, L.stream_ptr()))
    return out


def lowres_pack(img, xin):
    """xin[:, :C] = img for img [B,C,F,S,S] and xin [B,2C,F,S,S] (the first launch of a super-resolution sampling step); xin[:, C:] is
    not touched.  Returns xin."""
    B, per = img.shape[0], img.numel() // img.shape[0]
    assert img.dtype == torch.float32 and xin.dtype == torch.float32 and xin.numel() == 2 * img.numel() and xin.shape[0] == B
    L.check(L.vdx_lowres_pack(L.ptr(img), L.ptr(xin), B, per, L.stream_ptr()))
    return xin
