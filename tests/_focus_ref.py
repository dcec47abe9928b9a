"""fp64 references for the focus-present mask (Unet3D(focus_present=True)): the attention block and its core backward with
the per-sample mask applied BEFORE the softmax (scores with key != query at -1e30, after the position bias), emulations of the kernels'
rounding points, and the oracle network with the temporal attention of its nine downs / mid / ups blocks patched to the masked form
(init_temporal_attn stays unmasked).  A plain module: nothing here is collected.  The oracle file itself is not edited.

The rounding points are those of tests/_posbias_ref.py; for a masked sample the probabilities are exactly one-hot, so the block's branch
is out(rd(v)) and the core's backward is dq = dk = 0, dv = dO, o = v.
"""
import math
from unittest import mock

import torch

import _parity as P
import _posbias_ref as PB
from oracle import unet3d_ref as R

NEG = -1e30


def _sample_mask(focus, B, fault=None):
    """bool [B]: flag of every sample (focus [n], sample b reads focus[b % n]); fault 'next_sample': sample b gets the flag of b + 1."""
    f = (torch.as_tensor(focus) != 0).reshape(-1)
    idx = torch.arange(B) + (1 if fault == 'next_sample' else 0)
    return f[idx % f.numel()]


def attention_block_focus(x, wqkv, bqkv, wo, bo, focus, bias=None, heads=8, emulate=False, operand='bf16', round_out=False, fault=None,
                          dtype=torch.float64):
    """y = MHA(x) + x over the frames of every pixel (x [B, Fr, H, W, C]) with the scores of the samples flagged in focus [n] masked to
    -1e30 off the diagonal before the softmax (after the optional bias [heads, L, L]).  Arguments as PB.attention_block_bias.
    fault (for the CPU proofs): 'next_sample' applies the flag of sample b + 1 to sample b.  -> (branch y - x, y)"""
    B, Fr, H, W, C_ = x.shape
    HD = heads * 32
    rd = P.operand_rounding(operand) if emulate else (lambda t: t)
    qkv = x.to(dtype).reshape(-1, C_) @ wqkv.to(dtype) + bqkv.to(dtype)
    qkv = torch.cat((qkv[:, :HD] / math.sqrt(32.0), qkv[:, HD:]), 1)
    s = PB._seq(rd(qkv), B, Fr, H * W, heads, True, 3)
    q, k, v = s[..., 0, :, :], s[..., 1, :, :], s[..., 2, :, :]                     # [b, s, L, h, d]
    S = torch.einsum('bsihd,bsjhd->bshij', q, k)
    if bias is not None:
        S = S + bias.to(dtype)
    fm = _sample_mask(focus, B, fault).reshape(B, 1, 1, 1, 1)
    off = ~torch.eye(Fr, dtype=torch.bool)
    S = torch.where(fm & off, torch.full_like(S, NEG), S)
    Pm = torch.softmax(S, -1)
    o = rd(PB._unseq(torch.einsum('bshij,bsjhd->bsihd', rd(Pm), v), True))
    branch = (o @ wo.to(dtype) + bo.to(dtype)).reshape(x.shape)
    y = branch + x.to(dtype)
    return branch, (P.bf16r(y) if round_out else y)


def present_block(x, wqkv, bqkv, wo, bo, heads=8, emulate=False, operand='bf16', round_out=False, dtype=torch.float64):
    """The all-present block: y = x + bo + Wo rd(Wv x + bv) -> (branch, y)."""
    HD = heads * 32
    rd = P.operand_rounding(operand) if emulate else (lambda t: t)
    v = rd(x.to(dtype).reshape(-1, x.shape[-1]) @ wqkv.to(dtype)[:, 2 * HD:] + bqkv.to(dtype)[2 * HD:])
    branch = (v @ wo.to(dtype) + bo.to(dtype)).reshape(x.shape)
    y = branch + x.to(dtype)
    return branch, (P.bf16r(y) if round_out else y)


def attn_core_focus(qkv, d_o, focus, B, Fr, HW, heads, bias=None, emulate=False, round_out=False, dtype=torch.float64):
    """PB.attn_core_bias (temporal) with the focus mask on the scores: -> o, dqkv, dbias (the sum of dS over ALL sequences: masked samples
    add exactly 0; zeros without a bias)."""
    rd = P.bf16r if emulate else (lambda t: t)
    s = PB._seq(rd(qkv.to(dtype)), B, Fr, HW, heads, True, 3)
    q, k, v = s[..., 0, :, :], s[..., 1, :, :], s[..., 2, :, :]
    do = PB._seq(rd(d_o.to(dtype)), B, Fr, HW, heads, True, 1)[..., 0, :, :]
    sc = 1.0 / math.sqrt(32.0)
    S = torch.einsum('bsihd,bsjhd->bshij', q, k) * sc
    if bias is not None:
        S = S + bias.to(dtype)
    fm = _sample_mask(focus, B).reshape(B, 1, 1, 1, 1)
    S = torch.where(fm & ~torch.eye(Fr, dtype=torch.bool), torch.full_like(S, NEG), S)
    Pm = torch.softmax(S, -1)
    dP = torch.einsum('bsihd,bsjhd->bshij', do, v)
    dS = Pm * (dP - (Pm * dP).sum(-1, keepdim=True))
    dbias = dS.sum((0, 1))
    Pm, dS = rd(Pm), rd(dS)
    o = torch.einsum('bshij,bsjhd->bsihd', Pm, v)
    dv = torch.einsum('bshij,bsihd->bsjhd', Pm, do)
    dq = torch.einsum('bshij,bsjhd->bsihd', dS, k) * sc
    dk = torch.einsum('bshij,bsihd->bsjhd', dS, q) * sc
    outs = [PB._unseq(t, True) for t in (o, dq, dk, dv)]
    if round_out:
        outs = [P.bf16r(t) for t in outs]
    return outs[0], torch.cat(outs[1:], -1), dbias


def temporal_attention_focus(focus, pos=False, fault=None):
    """R.temporal_attention's replacement: the nine blocks of downs / mid / ups masked by focus [n] (None: no mask), init_temporal_attn
    unmasked (dispatch on `prefix`; fault 'init_too' masks it as well); pos: the pre-softmax relative position bias on all ten."""
    def fn(p, prefix, x, dim_head):
        B, Fr, H, W, C = x.shape
        pre = f'{prefix}.fn.fn.fn'
        heads = p[f'{pre}.q.bias'].shape[0]
        xt = x.permute(0, 2, 3, 1, 4).reshape(B, H * W, Fr, C)
        lin = lambda n: torch.einsum('...c,chd->...hd', xt, p[f'{pre}.{n}.kernel']) + p[f'{pre}.{n}.bias']
        q, k, v = lin('q') / dim_head ** 0.5, lin('k'), lin('v')
        sim = torch.einsum('...ihd,...jhd->...hij', q, k)
        if pos:
            sim = sim + R.relative_position_bias(p, Fr, heads).to(x.dtype)
        if focus is not None and (not prefix.startswith('init_temporal_attn') or fault == 'init_too'):
            fm = _sample_mask(focus, B).reshape(B, 1, 1, 1, 1)
            sim = torch.where(fm & ~torch.eye(Fr, dtype=torch.bool), torch.full_like(sim, NEG), sim)
        a = torch.einsum('...hij,...jhd->...ihd', torch.softmax(sim, dim=-1), v)
        o = torch.einsum('...hd,hdc->...c', a, p[f'{pre}.out.kernel']) + p[f'{pre}.out.bias']
        return o.reshape(B, H, W, Fr, C).permute(0, 3, 1, 2, 4) + x
    return fn


def patched(focus, pos=False, fault=None):
    """Context manager: the oracle's temporal attention is the masked form inside (R.unet_forward, oracle.train_ref, ...)."""
    return mock.patch.object(R, 'temporal_attention', temporal_attention_focus(focus, pos, fault))


def unet_forward_focus(p, cfg, x, time, focus, pos=False, **kw):
    with patched(focus, pos):
        return R.unet_forward(p, cfg, x, time, **kw)
