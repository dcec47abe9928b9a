"""The algebra of the tiled attention-core backward for more than 64 tokens (csrc/attn_long_bwd.hip), restated in fp64 on the CPU:
64-token tiles, an online softmax over the key tiles (-> O, the row maximum m, 1 / sum exp(s - m), delta = sum_d dO . O), then the
recompute of P = exp(S - m) / sum and dS = P o (dP - delta) tile by tile for dV, dK (per key tile) and dQ (per query tile).  It must
be the closed form of tests/_parity.py (attn_core, which tests/test_host_parity_helpers.py pins to autograd) to round-off, independent
of any device; and a key tile dropped from the first pass of ONE (sequence, head) must stand far above the per-sequence bound the GPU
test states, so that bound can see such a fault."""
import math

import pytest
import torch

import _parity as P

F64 = torch.float64
T = 64
SEQ_BOUND = 2e-5          # tests/test_gpu_long_attention_backward.py: dq|dk|dv per sequence (and o at half of it)


def tiled_core(qkv, d_o, B, Fr, HW, heads, skip=None):
    """-> o [rows][HD], dqkv [rows][3 HD] in fp64, spatial sequences.  skip = (sequence, head, key tile): that tile is left out of the
    first pass (the online softmax) of that (sequence, head) -- the fault of the sensitivity test."""
    assert HW % T == 0 and HW > T
    nt, nseq, sc = HW // T, B * Fr, 1.0 / math.sqrt(32.0)
    s = qkv.to(F64).reshape(nseq, HW, 3, heads, 32)
    do = d_o.to(F64).reshape(nseq, HW, heads, 32)
    o, dq, dk, dv = (torch.zeros(nseq, HW, heads, 32, dtype=F64) for _ in range(4))
    for n in range(nseq):
        for h in range(heads):
            q, k, v, g = s[n, :, 0, h] * sc, s[n, :, 1, h], s[n, :, 2, h], do[n, :, h]
            m, inv, delta = torch.empty(HW, dtype=F64), torch.empty(HW, dtype=F64), torch.empty(HW, dtype=F64)
            for i in range(nt):                                   # stats pass: one query tile, all key tiles
                qi = slice(i * T, (i + 1) * T)
                mi, li, acc = torch.full((T,), -3.0e38, dtype=F64), torch.zeros(T, dtype=F64), torch.zeros(T, 32, dtype=F64)
                for j in range(nt):
                    if skip == (n, h, j):
                        continue
                    kj = slice(j * T, (j + 1) * T)
                    S = q[qi] @ k[kj].T
                    mn = torch.maximum(mi, S.max(dim=1).values)
                    corr, p = torch.exp(mi - mn), torch.exp(S - mn[:, None])
                    li = li * corr + p.sum(dim=1)
                    acc = acc * corr[:, None] + p @ v[kj]
                    mi = mn
                o[n, qi, h] = acc / li[:, None]
                m[qi], inv[qi] = mi, 1.0 / li
                delta[qi] = (g[qi] * o[n, qi, h]).sum(dim=1)
            for j in range(nt):                                   # dkv pass: one key tile, all query tiles
                kj = slice(j * T, (j + 1) * T)
                for i in range(nt):
                    qi = slice(i * T, (i + 1) * T)
                    Pt = torch.exp(k[kj] @ q[qi].T - m[qi][None, :]) * inv[qi][None, :]
                    dSt = Pt * (v[kj] @ g[qi].T - delta[qi][None, :])
                    dv[n, kj, h] += Pt @ g[qi]
                    dk[n, kj, h] += dSt @ q[qi]
            for i in range(nt):                                   # dq pass: one query tile, all key tiles
                qi = slice(i * T, (i + 1) * T)
                for j in range(nt):
                    kj = slice(j * T, (j + 1) * T)
                    Pm = torch.exp(q[qi] @ k[kj].T - m[qi][:, None]) * inv[qi][:, None]
                    dS = Pm * (g[qi] @ v[kj].T - delta[qi][:, None])
                    dq[n, qi, h] += dS @ k[kj] * sc
    HD = heads * 32
    return o.reshape(-1, HD), torch.cat([t.reshape(-1, HD) for t in (dq, dk, dv)], dim=1)


def _inputs(B, Fr, H, W, heads):
    g = torch.Generator().manual_seed(B + Fr + H)
    npix, HD = B * Fr * H * W, heads * 32
    return P.bf16r(torch.randn(npix, 3 * HD, generator=g)), P.bf16r(torch.randn(npix, HD, generator=g))


@pytest.mark.parametrize('B,Fr,H,W,heads', [(1, 2, 8, 16, 8), (1, 2, 24, 24, 2)])
def test_tiled_restatement_is_the_closed_form(B, Fr, H, W, heads):
    qkv, d_o = _inputs(B, Fr, H, W, heads)
    o_ref, g_ref = P.attn_core(qkv, d_o, B, Fr, H * W, heads, False)
    o, g = tiled_core(qkv, d_o, B, Fr, H * W, heads)
    ro, rg = P.rel(o, o_ref), P.rel(g, g_ref)
    print(f'tiled restatement, {H * W} tokens: o {ro:.3e}, dq|dk|dv {rg:.3e}')
    assert ro < 1e-12 and rg < 1e-12
    HD = heads * 32
    for a in range(3):
        assert P.rel(g[:, a * HD:(a + 1) * HD], g_ref[:, a * HD:(a + 1) * HD]) < 1e-12


@pytest.mark.parametrize('B,Fr,H,W,heads,skip', [(1, 2, 8, 16, 8, (1, 3, 1)), (1, 2, 24, 24, 2, (0, 1, 4))])
def test_a_dropped_key_tile_stands_far_above_the_bound(B, Fr, H, W, heads, skip):
    qkv, d_o = _inputs(B, Fr, H, W, heads)
    o_ref, g_ref = P.attn_core(qkv, d_o, B, Fr, H * W, heads, False)
    o, g = tiled_core(qkv, d_o, B, Fr, H * W, heads, skip=skip)
    seq = lambda t: t.reshape(B * Fr, -1)
    wo, io, _ = P.per_group_rel(seq(o), seq(o_ref), (B * Fr,))
    wg, ig, _ = P.per_group_rel(seq(g), seq(g_ref), (B * Fr,))
    print(f'key tile {skip[2]} dropped for (sequence {skip[0]}, head {skip[1]}): o {wo:.3e} (sequence {io}), dq|dk|dv {wg:.3e} (sequence {ig})')
    assert io == skip[0] and ig == skip[0]
    assert wo > 100 * SEQ_BOUND and wg > 100 * SEQ_BOUND
