"""fp64 references for the temporal relative position bias (Unet3D(temporal_pos_bias=True)): the attention block and its core
backward with a PRE-softmax bias, emulations of the kernels' rounding points, and the oracle network with its temporal attention patched
to the biased form.  A plain module: nothing here is collected.  The oracle file itself is not edited -- `unet_forward_pos` swaps
`oracle.unet3d_ref.temporal_attention` for the duration of one call (unittest.mock.patch.object).

The rounding points follow tests/_parity.py (attention_block_fwd, attn_core); the bias is added to the fp32 scores and is never rounded:
* attention_reg_kernel / attention_kernel, BIAS instantiations: q = rd((x Wq + bq) / sqrt(32)), k, v = rd(x W + b); S = q k^T + bias in fp32;
  P = rd(softmax(S)); o = rd(P v); y = o Wo + bo + x in fp32 (rounded to bf16 once more on bf16 tensors).
* attn_core_bwd16_kernel, bias form: q, k, v, dO rounded to bf16 at staging (q UNSCALED: the scale multiplies the fp32 scores);
  P and dS rounded to bf16 for the second products; dBias = the sum of the UNROUNDED fp32 dS over the sequences.
"""
import math
from unittest import mock

import torch

import _parity as P
from oracle import unet3d_ref as R


def buckets_ref(n: int) -> torch.Tensor:
    """The oracle's bucket map [n, n] (int64), read off R.relative_position_bias with an embedding that names its own row."""
    emb = torch.arange(32, dtype=torch.float64)[:, None]
    return R.relative_position_bias({'time_rel_pos_bias.relative_attention_bias.embedding': emb}, n, 1)[0].to(torch.int64)


def bias_table(emb: torch.Tensor, n: int) -> torch.Tensor:
    """[heads, n, n] from an embedding [32, heads], through the oracle."""
    return R.relative_position_bias({'time_rel_pos_bias.relative_attention_bias.embedding': emb}, n, emb.shape[1])


def _seq(rows, B, Fr, HW, heads, temporal, parts):
    x = rows.reshape(B, Fr, HW, parts, heads, 32)
    return x.permute(0, 2, 1, 3, 4, 5) if temporal else x


def _unseq(t, temporal):
    t = t.permute(0, 2, 1, 3, 4) if temporal else t
    return t.reshape(-1, t.shape[-2] * 32)


def attention_block_bias(x, wqkv, bqkv, wo, bo, bias, heads, temporal, emulate=False, operand='bf16', round_out=False, fault=None,
                         dtype=torch.float64):
    """y = MHA_bias(x) + x: softmax_j(q_i . k_j / sqrt(32) + bias[h, i, j]) v_j, heads x 32, over the frames of every pixel (temporal) or
    the pixels of every frame.  x [B, Fr, H, W, C]; wqkv [C, 3 HD] = q | k | v column blocks, bqkv [3 HD], wo [HD, C], bo [C];
    bias [heads, L, L] or None (the unbiased block).  emulate: q, k, v, P, o rounded to the operand type ('bf16' / 'f16'; see the module
    docstring); round_out: y rounded to bf16 (bf16 tensors).  fault (for the CPU proofs): 'transpose' uses bias[h, j, i];
    'post_softmax' adds the bias to the probabilities (the reference's dead code) instead of the scores.
    -> (branch y - x [B, Fr, H, W, C], y)"""
    B, Fr, H, W, C_ = x.shape
    HD = heads * 32
    rd = P.operand_rounding(operand) if emulate else (lambda t: t)
    qkv = x.to(dtype).reshape(-1, C_) @ wqkv.to(dtype) + bqkv.to(dtype)
    qkv = torch.cat((qkv[:, :HD] / math.sqrt(32.0), qkv[:, HD:]), 1)
    s = _seq(rd(qkv), B, Fr, H * W, heads, temporal, 3)
    q, k, v = s[..., 0, :, :], s[..., 1, :, :], s[..., 2, :, :]                     # [b, s, L, h, d]
    S = torch.einsum('bsihd,bsjhd->bshij', q, k)
    bb = None if bias is None else (bias.to(dtype).transpose(-1, -2) if fault == 'transpose' else bias.to(dtype))
    if bb is not None and fault != 'post_softmax':
        S = S + bb
    Pm = torch.softmax(S, -1)
    if bb is not None and fault == 'post_softmax':
        Pm = Pm + bb
    o = rd(_unseq(torch.einsum('bshij,bsjhd->bsihd', rd(Pm), v), temporal))
    branch = (o @ wo.to(dtype) + bo.to(dtype)).reshape(x.shape)
    y = branch + x.to(dtype)
    return branch, (P.bf16r(y) if round_out else y)


def attn_core_bias(qkv, d_o, bias, B, Fr, HW, heads, temporal, emulate=False, round_out=False, dtype=torch.float64):
    """Attention core backward with the pre-softmax bias, closed form in `dtype`: qkv [rows][3 HD] (biased, q unscaled), d_o [rows][HD],
    bias [heads, L, L] -> o [rows][HD], dqkv [rows][3 HD], dbias [heads, L, L] = sum over the sequences of dS.
    emulate: q, k, v, d_o rounded to bf16 (the staging of attn_core_bwd16_kernel), P and dS rounded to bf16 for the second products;
    dbias sums the unrounded dS.  round_out: o, dq, dk, dv rounded to bf16 (bf16 tensors)."""
    rd = P.bf16r if emulate else (lambda t: t)
    s = _seq(rd(qkv.to(dtype)), B, Fr, HW, heads, temporal, 3)
    q, k, v = s[..., 0, :, :], s[..., 1, :, :], s[..., 2, :, :]
    do = _seq(rd(d_o.to(dtype)), B, Fr, HW, heads, temporal, 1)[..., 0, :, :]
    sc = 1.0 / math.sqrt(32.0)
    S = torch.einsum('bsihd,bsjhd->bshij', q, k) * sc + bias.to(dtype)
    Pm = torch.softmax(S, -1)
    dP = torch.einsum('bsihd,bsjhd->bshij', do, v)
    dS = Pm * (dP - (Pm * dP).sum(-1, keepdim=True))
    dbias = dS.sum((0, 1))
    Pm, dS = rd(Pm), rd(dS)
    o = torch.einsum('bshij,bsjhd->bsihd', Pm, v)
    dv = torch.einsum('bshij,bsihd->bsjhd', Pm, do)
    dq = torch.einsum('bshij,bsjhd->bsihd', dS, k) * sc
    dk = torch.einsum('bshij,bsihd->bsjhd', dS, q) * sc
    outs = [_unseq(t, temporal) for t in (o, dq, dk, dv)]
    if round_out:
        outs = [P.bf16r(t) for t in outs]
    return outs[0], torch.cat(outs[1:], -1), dbias


def temporal_attention_pos(p, prefix, x, dim_head):
    """R.temporal_attention with the relative position bias added to the scores before the softmax (T5 / Video Diffusion Models form)."""
    B, Fr, H, W, C = x.shape
    pre = f'{prefix}.fn.fn.fn'
    heads = p[f'{pre}.q.bias'].shape[0]
    bias = R.relative_position_bias(p, Fr, heads).to(x.dtype)
    xt = x.permute(0, 2, 3, 1, 4).reshape(B, H * W, Fr, C)
    lin = lambda n: torch.einsum('...c,chd->...hd', xt, p[f'{pre}.{n}.kernel']) + p[f'{pre}.{n}.bias']
    q, k, v = lin('q') / dim_head ** 0.5, lin('k'), lin('v')
    sim = torch.einsum('...ihd,...jhd->...hij', q, k) + bias
    a = torch.einsum('...hij,...jhd->...ihd', torch.softmax(sim, dim=-1), v)
    o = torch.einsum('...hd,hdc->...c', a, p[f'{pre}.out.kernel']) + p[f'{pre}.out.bias']
    return o.reshape(B, H, W, Fr, C).permute(0, 3, 1, 2, 4) + x


def patched():
    """Context manager: the oracle's temporal attention is the biased form inside (R.unet_forward, oracle.train_ref, ...)."""
    return mock.patch.object(R, 'temporal_attention', temporal_attention_pos)


def unet_forward_pos(p, cfg, x, time, **kw):
    """R.unet_forward with every temporal attention block biased (the mid spatial attention keeps none)."""
    with patched():
        return R.unet_forward(p, cfg, x, time, **kw)


def adam_first_step_bound(grads, eps_g):
    """Relative L2 distance to expect, at most, between Adam's first update on `grads` (the fp64 reference, name -> tensor) and on a
    gradient that just meets the relative tolerance eps_g in every tensor.  The first step is lr g / (|g| + 1e-8) = lr sign(g), so the
    two updates differ only where the error flips a sign, by 2 lr there, out of lr per element that moves at all.  Model: in a tensor of
    n elements the error is spread evenly, Gaussian with sigma = eps_g |g| / sqrt(n) per element and independent of g, so element i
    flips with probability Phi(-|g_i| / sigma).  With E the expected number of flips and a three-sigma allowance for its (Poisson)
    spread -- which matters for a tensor as small as the embedding, where one flip is a visible step -- the bound is
    2 sqrt((E + 3 sqrt(E)) / #{g_i != 0}).  Elements whose reference gradient is exactly zero (unused buckets) do not move and do not
    count.  Computed from the reference alone."""
    flips, moving = 0.0, 0
    for v in grads.values():
        g = v.reshape(-1).double().abs()
        g = g[g > 0]
        if g.numel() == 0:
            continue
        sigma = eps_g * g.norm() / math.sqrt(v.numel())
        flips += (0.5 * torch.erfc(g / (sigma * math.sqrt(2.0)))).sum().item()
        moving += g.numel()
    return 2.0 * math.sqrt((flips + 3.0 * math.sqrt(flips)) / max(1, moving))


def l2_loss_bound(ref_loss, pred, eps_f):
    """Bound on |mean((noise - pred')^2) - mean((noise - pred)^2)| for a prediction within relative L2 distance eps_f of `pred`:
    (2 |r| |d| + |d|^2) / n with the residual norm |r| = sqrt(n loss) and |d| = eps_f |pred| (Cauchy-Schwarz)."""
    n = pred.numel()
    d = eps_f * pred.double().norm().item()
    return (2.0 * math.sqrt(n * float(ref_loss)) * d + d * d) / n
