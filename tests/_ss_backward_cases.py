"""Case data of the ResnetBlock time-MLP backward parity tests (resblock_ss_bwd_kernel + resblock_ss_bwd_w_kernel + the slot pass, through
vdx_resblock_scale_shift_backward): layer tables, inputs, fp64 references and the bounds derived from the reference side, built on the
CPU and cached.  A plain module: nothing here is collected, nothing here touches the GPU.  tests/test_gpu_ss_backward.py runs the
kernels against these cases; tests/test_host_parity_helpers.py injects faults into a restatement of the kernels' steps (`kernel_steps`)
and shows what the bounds reject.

Reference: fp64 autograd of sum over the layers of LayerNorm_n(SiLU(temb) W + b) * dss through oracle/unet3d_ref.py (R.silu, R.layer_norm
with the oracle's NORM_EPS), with respect to temb and the four parameters of every layer.  The kernel reads `lin` (the forward's
pre-LayerNorm values) from memory: it gets the fp32 rounding of the fp64 lin, and the reference differentiates the LayerNorm at that
same tensor, so the rounding of lin is not part of any error.
Bound: the rule of the forward twin (P.norm_bound): max(2e-6, 8 x the same formulas in fp32 on the CPU against fp64) per group -- d(lin)
per (layer, sample), dW / db / d gamma / d beta per layer, d(temb) per sample.  Nothing in a bound comes from a kernel's output; a bound
above 2e-5 is refused here (the CPU floor is 1.5e-7 .. 5e-7, under the cancellation of the `offset` case 1.8e-6)."""
import functools

import torch

import _parity as P
from oracle import unet3d_ref as R

F32, F64 = torch.float32, torch.float64
SENTINEL = -768.0
BOUND_CEILING = 2e-5
PARAM_GAP, OUT_GAP = 7, 3          # floats between two tensors of the parameter buffer / columns (per sample) between two layers' rows
FORWARD_WIDTHS = (64, 128, 2048)   # the table of the forward test (tests/_forward_cases.py SS_WIDTHS)

# name: temb_dim, B, widths and what the case reaches.  Which form runs follows from launch_resblock_ss_bwd's dispatch (the launcher does
# not report to the launch hook): fewer than 8 layers -> one row of the Linear per workgroup (kb = 1, grid nlayers x temb_dim), 8 or more
# -> 8 rows (kb = 8, grid nlayers x ceil(temb_dim / 8)); the slot pass runs slot_sum_kernel below 32 layers, slot_sum16_kernel from 32 on.
CASES = {
    'corner': dict(temb_dim=64, B=2, widths=(32, 64)),                      # the network's own corner: kb = 1, 2 slots
    't96_b1': dict(temb_dim=96, B=1, widths=FORWARD_WIDTHS),                # 2048 columns = 8 strides of 256 threads; kb = 1
    't96_b8': dict(temb_dim=96, B=8, widths=FORWARD_WIDTHS),
    't96_b9': dict(temb_dim=96, B=9, widths=FORWARD_WIDTHS),
    't96_b19': dict(temb_dim=96, B=19, widths=FORWARD_WIDTHS),
    't1024_b9': dict(temb_dim=1024, B=9, widths=FORWARD_WIDTHS),            # long n-reductions of d(temb); kb = 1, 1024 row workgroups per layer
    'ragged_kb8': dict(temb_dim=100, B=5, widths=(32, 48) * 5),             # kb = 8, the last row block holds rows 96..99; n = 48: a partly filled wave
    'n_table': dict(temb_dim=256, B=4, widths=(128,) * 4 + (256,) * 4 + (512,) * 4 + (1024,) * 6),   # the N shape's table: kb = 8, 18 slots
    'slots34': dict(temb_dim=64, B=3, widths=(32,) * 34),                   # 34 slots: slot_sum16_kernel
    'offset': dict(temb_dim=96, B=9, widths=FORWARD_WIDTHS, offset=3.0),    # biases + 3 rms: ss / N - mean^2 under cancellation
    'stages6': dict(temb_dim=64, B=2, widths=(32, 64) * 3),                 # three stages of two layers, as model_backward issues them
    'small_var': dict(temb_dim=96, B=2, widths=(64, 128), temb_scale=0.02, bias_scale=0.01),   # var(lin) ~ 1e-4: NORM_EPS = 1e-6 is 1 % of it
    # B x temb_dim floats = 192 KB: more than a workgroup's LDS, which the LayerNorm half once reserved (and never used)
    'b48_t1024': dict(temb_dim=1024, B=48, widths=(64, 64)),
}


def _gen(name):
    return torch.Generator().manual_seed(sum(ord(c) * (i + 1) for i, c in enumerate(name)) % (2 ** 31))


def layout(widths, temb_dim):
    """Layer table over one flat parameter buffer and one flat row buffer, neither contiguous: PARAM_GAP floats before every tensor,
    OUT_GAP columns before every layer's rows, and the LAST layer of the table placed first in both buffers (a table out of address
    order).  -> (layers: list of dicts n, w_off, b_off, g_off, be_off, out_off; parameter floats; row columns per sample)"""
    order = [len(widths) - 1] + list(range(len(widths) - 1))
    layers = [dict(n=n) for n in widths]
    off = out = 0
    for i in order:
        l = layers[i]
        for key, cnt in (('w_off', temb_dim * l['n']), ('b_off', l['n']), ('g_off', l['n']), ('be_off', l['n'])):
            off += PARAM_GAP
            l[key] = off
            off += cnt
        out += OUT_GAP
        l['out_off'] = out
        out += l['n']
    return layers, off + PARAM_GAP, out + OUT_GAP


def pack_params(layers, tensors, total, fill=SENTINEL):
    """tensors[i] = (W, b, gamma, beta) of layer i -> the flat fp32 buffer, `fill` in the gaps"""
    flat = torch.full((total,), fill, dtype=F32)
    for l, ts in zip(layers, tensors):
        for key, t in zip(('w_off', 'b_off', 'g_off', 'be_off'), ts):
            flat[l[key]:l[key] + t.numel()] = t.reshape(-1).float()
    return flat


def unpack_params(flat, layers, temb_dim):
    """flat buffer -> [layer] (W [temb_dim, n], b, gamma, beta)"""
    return [(flat[l['w_off']:l['w_off'] + temb_dim * l['n']].reshape(temb_dim, l['n']), flat[l['b_off']:l['b_off'] + l['n']],
             flat[l['g_off']:l['g_off'] + l['n']], flat[l['be_off']:l['be_off'] + l['n']]) for l in layers]


def gap_mask(layers, temb_dim, total):
    """True where the parameter buffer belongs to no layer"""
    m = torch.ones(total, dtype=torch.bool)
    for l in layers:
        for key, cnt in (('w_off', temb_dim * l['n']), ('b_off', l['n']), ('g_off', l['n']), ('be_off', l['n'])):
            m[l[key]:l[key] + cnt] = False
    return m


def pack_rows(layers, rows, cols, B, fill=SENTINEL):
    """rows[i] [B, n] of layer i -> the flat fp32 buffer of the forward's ss / lin layout, `fill` in the gaps"""
    flat = torch.full((cols * B,), fill, dtype=F32)
    for l, r in zip(layers, rows):
        flat[l['out_off'] * B:(l['out_off'] + l['n']) * B] = r.reshape(-1).float()
    return flat


def unpack_rows(flat, layers, B):
    return [flat[l['out_off'] * B:(l['out_off'] + l['n']) * B].reshape(B, l['n']) for l in layers]


def row_mask(layers, cols, B, which):
    """True on the rows of the layers `which` (indices)"""
    m = torch.zeros(cols * B, dtype=torch.bool)
    for i in which:
        l = layers[i]
        m[l['out_off'] * B:(l['out_off'] + l['n']) * B] = True
    return m


def reference(temb, tensors, lin_r, dss, dt):
    """Autograd in `dt`.  -> dict(dlin=[layer][B, n], dW, db, dg, dbe = [layer], dtemb [B, temb_dim])"""
    t = temb.to(dt).requires_grad_(True)
    out = dict(dlin=[], dW=[], db=[], dg=[], dbe=[], dtemb=torch.zeros_like(t))
    for (W, b, g, be), lr, d in zip(tensors, lin_r, dss):
        W, b, g, be = (p.to(dt).requires_grad_(True) for p in (W, b, g, be))
        lin_at = lr.to(dt).requires_grad_(True)                          # the tensor the kernel reads
        dlin, dg, dbe = torch.autograd.grad(R.layer_norm(lin_at, g, be), (lin_at, g, be), d.to(dt))
        dtemb, dW, db = torch.autograd.grad(R.silu(t) @ W + b, (t, W, b), dlin)
        for k, v in (('dlin', dlin), ('dW', dW), ('db', db), ('dg', dg), ('dbe', dbe)):
            out[k].append(v)
        out['dtemb'] = out['dtemb'] + dtemb
    return out


def kernel_steps(temb, tensors, lin_r, dss, eps=R.NORM_EPS, stale_m2=None, dt=F64):
    """The steps of the two kernels restated in `dt`, sample by sample (csrc/small_bwd.hip): mean and the one-pass variance ss / N - mean^2,
    rstd = rsqrt(max(var, 0) + eps), xh, m1 = mean(g d), m2 = mean(g d xh), dlin = rstd (g d - m1 - xh m2); d gamma = sum_b d xh,
    d beta = sum_b d, db = sum_b dlin; dW = SiLU(temb)^T dlin, dtemb = SiLU'(temb) (dlin W^T).  Faults, for the CPU proofs: eps (another
    NORM_EPS); stale_m2 = (layer, sample): that sample's m2 is the previous sample's (a stale red[] between two rounds of the `for b` loop).
    -> dict as reference()"""
    t = temb.to(dt)
    sg = torch.sigmoid(t)
    act, dact = t * sg, sg * (1 + t * (1 - sg))
    out = dict(dlin=[], dW=[], db=[], dg=[], dbe=[], dtemb=torch.zeros_like(t))
    for i, ((W, b, g, be), lr, d) in enumerate(zip(tensors, lin_r, dss)):
        W, g, x, d = W.to(dt), g.to(dt), lr.to(dt), d.to(dt)
        N = x.shape[1]
        mean = x.sum(1, keepdim=True) / N
        rstd = torch.rsqrt(((x * x).sum(1, keepdim=True) / N - mean * mean).clamp_min(0.0) + eps)
        xh, gd = (x - mean) * rstd, g * d
        m1, m2 = gd.sum(1, keepdim=True) / N, (gd * xh).sum(1, keepdim=True) / N
        if stale_m2 is not None and stale_m2[0] == i:
            m2 = m2.clone()
            m2[stale_m2[1]] = m2[stale_m2[1] - 1]
        dlin = rstd * (gd - m1 - xh * m2)
        for k, v in (('dlin', dlin), ('dW', act.t() @ dlin), ('db', dlin.sum(0)), ('dg', (d * xh).sum(0)), ('dbe', d.sum(0))):
            out[k].append(v)
        out['dtemb'] = out['dtemb'] + dact * (dlin @ W.t())
    return out


def _bound(name, what, ref32, ref64, slices=None):
    bound, sb, floor = P.norm_bound(ref32, ref64, slices)
    worst = max([bound] + list(sb.values()))
    print(f'[ss bwd {name}] {what}: CPU fp32 floor {floor:.2e} -> bound {bound:.2e}' + (f', worst group bound {worst:.2e}' if slices else ''))
    assert worst <= BOUND_CEILING, f'{name} {what}: derived bound {worst:.2e} above {BOUND_CEILING:.0e}: a finding, not a setting'
    return bound, sb


@functools.lru_cache(maxsize=2)
def case(name):
    """-> dict: layers, total / cols (buffer sizes), params / lin / dss (flat fp32 buffers, sentinel gaps), temb, tensors, lin_r, dss_rows,
    ref (fp64, as reference()), bounds: b_dlin [layer] (bound, {sample: bound}), b_par {dW, db, dg, dbe: [layer] bound}, b_dtemb
    (bound, {sample: bound}), sl (sample slices)"""
    c = CASES[name]
    temb_dim, B, widths = c['temb_dim'], c['B'], c['widths']
    g = _gen(name)
    temb = torch.randn(B, temb_dim, generator=g) * c.get('temb_scale', 1.0)
    temb *= (1.0 + 0.2 * torch.arange(B).float())[:, None]               # no two samples alike
    layers, total, cols = layout(widths, temb_dim)
    tensors, dss_rows = [], []
    for n in widths:
        W = torch.randn(temb_dim, n, generator=g) / temb_dim ** 0.5
        b = 0.1 * c.get('bias_scale', 1.0) * torch.randn(n, generator=g)
        ga, be = 1 + 0.1 * torch.randn(n, generator=g), 0.1 * torch.randn(n, generator=g)
        if c.get('offset'):
            # (the rms of the sample with the smallest one: mean / std is `offset` there and below it in every other sample)
            b = b + c['offset'] * (R.silu(temb.double()) @ W.double()).pow(2).mean(1).sqrt().min().float()
        tensors.append((W, b, ga, be))
        dss_rows.append(torch.randn(B, n, generator=g))
    lin_r = [(R.silu(temb.double()) @ W.double() + b.double()).float() for W, b, _, _ in tensors]
    ref, ref32 = reference(temb, tensors, lin_r, dss_rows, F64), reference(temb, tensors, lin_r, dss_rows, F32)
    sl = P.sample_slices((B,))
    b_dlin = [_bound(name, f'd(lin) layer {i} n{n}', a, r, sl) for i, (n, a, r) in enumerate(zip(widths, ref32['dlin'], ref['dlin']))]
    b_par = {k: [_bound(name, f'{k} layer {i} n{n}', a, r)[0] for i, (n, a, r) in enumerate(zip(widths, ref32[k], ref[k]))]
             for k in ('dW', 'db', 'dg', 'dbe')}
    b_dtemb = _bound(name, 'd(temb)', ref32['dtemb'], ref['dtemb'], sl)
    return dict(name=name, temb_dim=temb_dim, B=B, widths=widths, layers=layers, total=total, cols=cols, temb=temb, tensors=tensors,
                lin_r=lin_r, dss_rows=dss_rows, params=pack_params(layers, tensors, total), lin=pack_rows(layers, lin_r, cols, B),
                dss=pack_rows(layers, dss_rows, cols, B), ref=ref, b_dlin=b_dlin, b_par=b_par, b_dtemb=b_dtemb, sl=sl)


def stages(nlayers):
    """Contiguous groups of the table in reverse order, as the stages of model_backward issue them: pairs (three of them for six layers),
    the first group of the table takes what is left.  -> list of lists of layer indices, in call order"""
    per = max(2, -(-nlayers // 3)) if nlayers >= 2 else 1
    groups = [list(range(i, min(i + per, nlayers))) for i in range(0, nlayers, per)]
    return groups[::-1]
