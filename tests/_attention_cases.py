"""Case data of the per-group parity tests of the level-0 / narrow-level attention and SLA kernels: inputs (bf16-representable on both
sides: x, and the weights rounded as the packing rounds them; mode 'f16': fp16-representable), the fp64 reference of the block's BRANCH
y - x, the fp64 emulation of the kernels' rounding points (bf16 and f16 modes) or the fp32 evaluation of the same formula (f32 mode), and
the per-group bounds derived from them.  Mode 'f16' keeps the fp32 evaluation of its emulation as well (c['emu32']): the floor of the
closeness-to-emulation check (P.assert_close_to_emulation).
Built on the CPU and cached.  A plain module: nothing here is collected, nothing here touches the GPU.
tests/test_gpu_attention_groups.py runs the kernels against these cases; tests/test_host_parity_helpers.py injects faults into the
same cases and shows that the global figures of tests/test_gpu_blocks.py let them pass while these bounds reject them."""
import functools

import torch

import _forward_cases as FC
import _parity as P

F32, F64 = torch.float32, torch.float64

SLA_CHUNK = 32                 # frames per evaluation / comparison chunk of the large SLA cases (fp64 q, k, v of 32 x 2048 pixels: 400 MB)
KEEP_EMULATED = 20 * 2 ** 20   # elements up to which a case keeps its emulated branch (the CPU proofs start from it)


# ---- weights ---------------------------------------------------------------------------------------------------------------------------


def _iso(pair, iso, at):
    """(rounded, raw) weight tuples with the head-isolating out-projection (P.isolate_heads) in place of wo = t[at] of both, when asked for."""
    if not iso:
        return pair
    return tuple(t[:at] + (P.isolate_heads(t[at]),) + t[at + 1:] for t in pair)


# ---- attention -------------------------------------------------------------------------------------------------------------------------


FP8_STATED = 1e-1    # the fp8 core's branch figure as tests/test_gpu_blocks.py (test_attention_fp8_core) and DESIGN.md section 8 state it


def seq_view(temporal):
    """[B, F, H, W, C] -> one group per attention sequence (FC.seq_groups, as a view: a list of 2-D pieces)"""
    return lambda t: [FC.seq_groups(t, temporal)]


# Closeness of an f16-mode kernel to the emulation of its rounding points, in multiples of the flip floor (P.assert_close_to_emulation).
# 4 is the margin P.tile_bound gives the same kind of floor.  A margin may be raised to 1.5 x the worst ratio measured on the GPU, never
# above half the smallest ratio a single stray bf16 rounding produces (tests/test_host_parity_helpers.py finds 12.9 for attention: cap 6.4;
# 19 for SLA without exp(k): cap 9.6).  DESIGN.md section 8 holds the measured ratios.
# Attention: measured 0.46 .. 1.58 on an MI355X, SLA 0.38 .. 1.54: both stay 4.  One case has a margin of its own: SLA (1,2,5,7,16),
# 35 pixels per frame, measured 4.79.  At that size single flipped roundings ARE the figure: compared pixel by pixel with the emulation,
# the kernel's frame 1 shares six flips with the CPU's fp32 evaluation (the same 5.8e-5 .. 8.2e-4 on the same pixels) and has two of its
# own, on pixels 11 and 23 (6.0e-3 and 3.3e-3: one fp16 ulp of an o element near 16, the spiked pixel's v, through Wo), where the CPU
# has one small one (pixel 28, 1.8e-4); every other pixel is within 6e-6.  The larger of the two alone is 4.2 floors of 6.8e-6.  No
# rounding point is missing from the emulation, so that case takes 1.5 x 4.79; with a head-isolating Wo the same shape would read 8.7,
# which is why the isolated-head SLA cases are larger ones.
F16_CLOSE_MARGIN = {'attention': 4.0, 'sla': 4.0}
F16_CLOSE_MARGIN_OF_CASE = {('sla', (1, 2, 5, 7, 16), False): 7.2}


def close_margin(c):
    """The closeness margin of an f16 case (F16_CLOSE_MARGIN, or the case's own)."""
    return F16_CLOSE_MARGIN_OF_CASE.get((c['kind'], c['shape'], c['iso']), F16_CLOSE_MARGIN[c['kind']])
F16_BOUND_CEILING = 5e-3   # 3 x the fp16 emulation sits near 2e-3 (attention) / 1e-3 (SLA): a derived bound above this is itself a finding


def _bounds(mode, cmp, ref, views, chunk, fixed=None):
    """{view name: bound}: bf16 and f16 modes 3 x the worst emulated group (P.view_bound); f32 mode one figure per group (P.f32_group_bounds)."""
    if fixed is not None:
        return {n: fixed for n in views}
    if mode == 'f32':
        return {n: P.f32_group_bounds(cmp, ref, v, chunk) for n, v in views.items()}
    b = {n: P.view_bound(cmp, ref, v, chunk) for n, v in views.items()}
    if mode == 'f16':
        assert max(b.values()) < F16_BOUND_CEILING, f'f16 bounds {b}: 3 x the emulation above {F16_BOUND_CEILING:.0e} -- the emulation or the case is off'
    return b


def _show(what, bounds):
    txt = ', '.join(f'per {n} {b.max().item() if torch.is_tensor(b) else b:.3e}' for n, b in bounds.items())
    print(f'[{what}] bounds from the reference side: {txt}')


@functools.lru_cache(maxsize=2)
def attn_case(shape, temporal, io16, mode, fp8=False, iso=False, q_scaled=False):
    """mode 'bf16': cmp = the fp64 emulation of the rounding points (round_out with io16, e4m3 operands with fp8, q_scaled for the
    kernels that scale q before rounding it); mode 'f32': cmp = the formula in fp32; mode 'f16': inputs and weights fp16-representable,
    cmp = the fp64 emulation with fp16 rounding points (always q_scaled: both kernels the mode reaches scale q first), emu32 = the same in
    fp32.  Tensors are branches y - x, [B, F, H, W, C]."""
    B, Fr, H, W, C = shape
    g = FC._gen(*shape, temporal, 16)
    operand = 'f16' if mode == 'f16' else 'bf16'
    x = P.operand_rounding(operand)(torch.randn(B, Fr, H, W, C, generator=g))
    w, raw = _iso(FC.mha_weights(C, g, raw=True, operand=operand), iso, 2)       # raw: the un-rounded kernels, what the oracle of tests/test_gpu_blocks.py sees
    xd = x.double()
    ref = P.attention_block_fwd(x, *w, B, Fr, H, W, temporal)[1] - xd
    fixed, emu32 = None, None
    if mode == 'f16':
        assert q_scaled and not io16 and not fp8
        kw = dict(emulate=True, q_scaled=True, operand='f16')
        cmp = P.attention_block_fwd(x, *w, B, Fr, H, W, temporal, **kw)[1] - xd
        emu32 = P.attention_block_fwd(x, *w, B, Fr, H, W, temporal, dtype=F32, **kw)[1].double() - xd
    elif mode == 'f32':
        cmp = P.attention_block_fwd(x, *w, B, Fr, H, W, temporal, dtype=F32)[1].double() - xd
    elif fp8 and not P.have_e4m3():                 # (no e4m3 casts in this torch: nothing to emulate the fp8 core with)
        cmp, fixed = ref, FP8_STATED
        print(f'[attention {shape} fp8] FALLBACK: torch has no e4m3 casts, so the bound below is the stated {FP8_STATED:.0e} per group, not 3 x an emulation')
    else:
        cmp = P.attention_block_fwd(x, *w, B, Fr, H, W, temporal, emulate=True, fp8=fp8, round_out=io16, q_scaled=q_scaled)[1] - xd
    views = {'sequence': seq_view(temporal)}
    if iso:
        views['(sequence, head)'] = P.seq_head_view(temporal)
    bounds = _bounds(mode, cmp, ref, views, None, fixed)
    _show(f'attention {shape} temporal={int(temporal)} io16={int(io16)} {mode} fp8={int(fp8)} iso={int(iso)}', bounds)
    return dict(x=x, w=w, raw=raw, ref=ref, cmp=cmp, emu32=emu32, views=views, bounds=bounds, chunk=None, shape=shape, temporal=temporal, kind='attention', iso=iso)


def attn_old_oracle(c):
    """The block as tests/test_gpu_blocks.py judges it: fp64 on the UN-rounded weights.  -> y"""
    B, Fr, H, W, _ = c['shape']
    return P.attention_block_fwd(c['x'], *c['raw'], B, Fr, H, W, c['temporal'])[1]


# ---- SLA -------------------------------------------------------------------------------------------------------------------------------


def sla_eval(x3, w, chunk=None, **kw):
    """Branch y - x of P.sla_block_fwd over x3 [NF, N, C], `chunk` frames at a time (frames are independent).  -> [NF, N, C] fp64"""
    NF, N, _ = x3.shape
    step = chunk or NF
    out = []
    for i in range(0, NF, step):
        xs = x3[i:i + step]
        out.append(P.sla_block_fwd(xs, *w, xs.shape[0], 1, N, 1, **kw)[1].double() - xs.double())
    return torch.cat(out)


@functools.lru_cache(maxsize=2)
def sla_case(shape, io16, mode, iso=False, old=False):
    """As attn_case; tensors are branches [NF, N, C].  Large cases are evaluated and compared SLA_CHUNK frames at a time and keep the
    reference only (c['cmp'] is None).  old: keep, per chunk, the sums of sla_old_figures for the clean emulation (c['old_sums']).
    mode 'f16': the emulation rounds the exponentials against the running maximum of sla_ctx_kernel (P.running_max over sla_plan's
    chunks of min(tiles, 8) sub-tiles of 64 pixels; the cases here are below the 1024 workgroups at which launch_sla_m lengthens them)."""
    B, Fr, H, W, C = shape
    NF, N = B * Fr, H * W
    g = FC._gen(*shape, 7, 16)
    operand = 'f16' if mode == 'f16' else 'bf16'
    x = FC.sla_input(shape, g, operand).reshape(NF, N, C)
    w, raw = _iso(FC.sla_weights(C, g, raw=True, operand=operand), iso, 3)
    views = {'frame': P.frame_view, '(frame, 64-pixel tile)': P.pixel_tile_view(64)}
    if iso:
        views['(frame, head)'] = P.frame_head_view
    chunk = SLA_CHUNK if NF > SLA_CHUNK and NF * N >= 2 ** 17 else None
    kw = dict(dtype=F32) if mode == 'f32' else dict(emulate=True, round_out=io16)
    if mode == 'f16':
        assert not io16 and NF * -(-N // 64) < 1024
        kw = sla_f16_kw(N)
    keep = x.numel() <= KEEP_EMULATED
    assert keep or mode != 'f16'
    ref, cmps, parts, sums, e32 = torch.empty(NF, N, C, dtype=F64), [], [], {}, []
    for i in range(0, NF, chunk or NF):                           # (reference and emulation of one chunk side by side: bounded host memory)
        xs = x[i:i + (chunk or NF)]
        r, e = sla_eval(xs, w), sla_eval(xs, w, **kw)
        ref[i:i + xs.shape[0]] = r
        if keep:
            cmps.append(e)
        if mode == 'f16':
            e32.append(sla_eval(xs, w, dtype=F32, **kw))
        parts.append(_bounds(mode, e, r, views, None))
        if old:
            sums[i] = _old_sums(e, sla_eval(xs, raw), xs)
    if mode == 'f32':
        bounds = {n: torch.cat([p[n] for p in parts]) for n in views}
    else:
        bounds = {n: max(p[n] for p in parts) for n in views}
    _show(f'SLA {shape} io16={int(io16)} {mode} iso={int(iso)}', bounds)
    return dict(x=x, w=w, raw=raw, ref=ref, cmp=torch.cat(cmps) if keep else None, emu32=torch.cat(e32) if e32 else None, views=views, bounds=bounds,
                chunk=chunk, shape=shape, NF=NF, N=N, old_sums=sums, kind='sla', iso=iso)


def sla_f16_kw(N):
    """The arguments of P.sla_block_fwd that make it the emulation of the f16-mode kernels at N pixels per frame."""
    return dict(emulate=True, operand='f16', running=(64, min(-(-N // 64), 8)))


def sla_old_oracle(c):
    """The block as tests/test_gpu_blocks.py judges it: fp64 on the UN-rounded weights.  -> y [NF, N, C]"""
    return sla_eval(c['x'], c['raw'], c['chunk']) + c['x'].double()


def _old_sums(e, old, xs):
    return (e - old).square().sum().item(), old.square().sum().item(), (old + xs.double()).square().sum().item()


def sla_old_figures(c, fault=None, frames=()):
    """The global figures of tests/test_gpu_blocks.py (rel-L2 of the branch and of the block against the oracle on un-rounded weights) of
    the emulated output of a case, walked in chunks of frames so that the largest case needs no full-size emulation.
    fault(i0, e): edits the emulated branch e of the chunk that starts at frame i0, in place; frames: the frames it touches -- the other
    chunks take the sums that sla_case(old=True) kept.  -> (branch rel, block rel)"""
    x, step = c['x'], c['chunk'] or c['NF']
    tot = [0.0, 0.0, 0.0]
    for i in range(0, c['NF'], step):
        if i in c['old_sums'] and not any(i <= f < i + step for f in frames):
            part = c['old_sums'][i]
        else:
            xs = x[i:i + step]
            e = sla_eval(xs, c['w'], emulate=True, round_out=True)
            if fault is not None:
                fault(i, e)
            part = _old_sums(e, sla_eval(xs, c['raw']), xs)
        tot = [a + b for a, b in zip(tot, part)]
    return (tot[0] / tot[1]) ** 0.5, (tot[0] / tot[2]) ** 0.5
