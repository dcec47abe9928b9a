"""Per-group parity of the fused attention and SLA kernels of the narrow levels -- attention_w_kernel, attention_h8_kernel,
attention_reg_kernel, attention_kernel; sla_ctx8_kernel -> sla_combine_kernel -> sla_out8_kernel / sla_out_w_kernel; sla_ctx_kernel ->
sla_out_kernel -- through vdx_attention_forward_bf16, vdx_attention_forward_ex, vdx_sla_forward_bf16 and vdx_sla_forward.

tests/test_gpu_blocks.py holds these kernels to global rel-L2 figures over whole tensors; a fault confined to one wave's work (padding
keys unmasked in one group of 4 sequences, a chunk partial the combine drops for one head of one frame, one 64-pixel tile on the wrong
frame's context) moves those figures by a tenth of their bound.  Here the BRANCH y - x (the residual hides the attention output) is
compared per sequence, per frame and per (frame, 64-pixel tile); a second variant of selected cases runs with a head-isolating
out-projection (P.isolate_heads), which makes channels c % 8 == h depend on head h alone: groups (sequence, head) and (frame, head).

Inputs are bf16-representable on both sides (x, and the weights as the packing rounds them), the reference is the fp64 closed form of
tests/_parity.py, and every bound comes from the reference side (tests/_attention_cases.py): bf16 mode 3 x the worst group of the fp64
emulation of the kernels' rounding points, f32 mode max(2e-6, 8 x the formula in fp32 on the CPU) per group.  Every group is asserted,
bound and worst group are printed (run with -s).  Outputs are NaN-filled before each call, every case runs twice and the runs must be
bit-identical, and each case asserts the kernels the launch hook reports (tests/_launch_hook.py): which form a shape reaches depends
on thresholds and on the number of compute units (256 on an MI355X; the arithmetic is in each case's comment).
tests/test_host_parity_helpers.py shows on the CPU that the faults above pass the global figures and are rejected here."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _attention_cases as AC
import _parity as P
import _parity_routes as PR
from _launch_hook import assert_launches, launches

# (tests/test_gpu_f16_forms.py runs the shapes that only fp16 mode needs through _run_attention / _run_sla / _check of this module)
DEV = 'cuda:0'
F32, BF = torch.float32, torch.bfloat16


def _dev(t, dtype=F32):
    return t.detach().to(dtype).to(DEV).contiguous()


def _nan_like(x):
    return torch.full(x.shape, float('nan'), dtype=x.dtype, device=x.device)


def _twice(fn, what):
    """fn() -> y on fresh NaN-filled output, twice under the launch hook; bit-identical runs.  -> (y on the CPU, launches of ONE run)"""
    with launches() as rec:
        a, b = fn(), fn()
        torch.cuda.synchronize()
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f'{what}: two runs are not bit-identical'
    n = len(rec) // 2
    assert rec[:n] == rec[n:], f'{what}: the two runs launched differently: {rec}'
    print(f'[{what}] launched: ' + '; '.join(f'{k} {s}' for k, s in rec[:n]))
    return a.cpu(), rec[:n]


def _check(c, y, what):
    """The branch y - x against the fp64 reference in every view of the case, each group below its bound."""
    x, ref = c['x'], c['ref']
    y = y.reshape(x.shape)
    branch = torch.empty_like(ref)
    step = c['chunk'] or x.shape[0]
    for i in range(0, x.shape[0], step):                                # (chunked: the largest case stays below 2 GB of host memory)
        branch[i:i + step] = y[i:i + step].double() - x[i:i + step].double()
        assert torch.isfinite(branch[i:i + step]).all(), f'{what}: non-finite output (a row the kernel did not write?)'
    for name, view in c['views'].items():
        P.assert_views(branch, ref, view, c['bounds'][name], f'{what} per {name}', c['chunk'])
    if c.get('emu32') is not None:                                      # mode f16: close to the emulation of its rounding points as well
        for name, view in c['views'].items():
            P.assert_close_to_emulation(branch, c['cmp'], c['emu32'], view, AC.close_margin(c), f'{what} per {name}', c['chunk'])


def _run_attention(c, mode, io16, fp8, what):
    from video_diffusion_nnx_amd import _lib as L, ops
    B, Fr, H, W, C = c['shape']
    wqkv, bqkv, wo, bo = c['w']
    packed = (ops.pack_conv_weights(_dev(wqkv), mode), _dev(bqkv), ops.pack_conv_weights(_dev(wo), mode), _dev(bo))
    x = _dev(c['x'], BF if io16 else F32)

    def go():
        y = _nan_like(x)
        if io16:
            L.check(L.vdx_attention_forward_bf16(L.ptr(x), L.ptr(y), *[L.ptr(t) for t in packed], B, Fr, H, W, C, 8, int(c['temporal']), int(fp8), L.stream_ptr()))
        else:
            L.check(L.vdx_attention_forward_ex(ops._mode(mode), L.ptr(x), L.ptr(y), *[L.ptr(t) for t in packed], B, Fr, H, W, C, 8, int(c['temporal']),
                                               int(fp8), L.stream_ptr()))
        return y
    return _twice(go, what)


def _run_sla(c, mode, io16, what):
    from video_diffusion_nnx_amd import _lib as L, ops
    B, Fr, H, W, C = c['shape']
    m = ops._mode(mode)
    pk = [ops.pack_conv_weights(_dev(t.reshape(1, *t.shape)), mode) for t in c['w']]
    x = _dev(c['x'].reshape(B, Fr, H, W, C), BF if io16 else F32)
    nbytes = L.vdx_sla_workspace_bytes(m, B * Fr, H * W, 8)

    def go():
        y = _nan_like(x)
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)      # (0xFF bytes: NaN as fp32 and as bf16 -- an unwritten partial or context shows)
        fn = L.vdx_sla_forward_bf16 if io16 else L.vdx_sla_forward
        args = ([] if io16 else [m]) + [L.ptr(x), L.ptr(y)] + [L.ptr(t) for t in pk] + [L.ptr(ws), B, Fr, H, W, C, 8, L.stream_ptr()]
        L.check(fn(*args))
        return y
    return _twice(go, what)


# ---- attention on bf16 tensors (vdx_attention_forward_bf16, temporal) ------------------------------------------------------------------------
# attention_w_kernel needs >= 256 sequences in multiples of 4 and H W % 4 == 0 (attn_w_eligible); it walks groups of 4 sequences, one
# wave per group, persistent_split(groups, 256 CUs x 8 waves = 2048 wave slots).  Below 256 sequences: attention_h8_kernel, one workgroup
# per 4 sequences (nsub = max(1, sub-tiles / 1024) = 1 here).  Shape strings: attention_w "<fp8 F8> C L nseq", attention_h8
# "<MODE, NKT, TMO, TNO, IO16, F8, FULL> C L nseq" (MODE 1 = bf16).
ATTN16 = [
    # shape (B, F, H, W, C), fp8, iso, kernel, parts of the shape string
    ((1, 16, 16, 16, 64), False, False, 'attention_w_kernel', ['<fp8 0>', 'C64 L16 nseq256']),     # 64 groups <= 2048 slots: 1 per wave, 8 workgroups; <.., 64, FULL>
    ((1, 16, 16, 16, 64), True, False, 'attention_w_kernel', ['<fp8 1>', 'C64 L16 nseq256']),      # ... with the e4m3 core
    ((1, 16, 16, 16, 64), False, True, 'attention_w_kernel', ['<fp8 0>', 'C64 L16 nseq256']),      # ... head-isolating Wo
    ((1, 16, 96, 93, 64), False, False, 'attention_w_kernel', ['<fp8 0>', 'C64 L16 nseq8928']),    # 2232 groups > 2048 slots: ceil(2232 / 2048) = 2 per wave, 1116 waves = 139.5 workgroups: the last one half empty
    ((2, 12, 16, 16, 64), False, False, 'attention_w_kernel', ['<fp8 0>', 'C64 L12 nseq512']),     # masked form (keys >= 12), two samples, 128 groups
    ((2, 12, 16, 16, 64), False, True, 'attention_w_kernel', ['<fp8 0>', 'C64 L12 nseq512']),      # ... head-isolating Wo
    ((1, 16, 16, 16, 32), False, False, 'attention_w_kernel', ['<fp8 0>', 'C32 L16 nseq256']),     # C = 32, full
    ((2, 10, 12, 12, 32), False, False, 'attention_w_kernel', ['<fp8 0>', 'C32 L10 nseq288']),     # C = 32, masked, 288 sequences = 72 groups over two samples
    ((1, 16, 8, 8, 64), False, False, 'attention_h8_kernel', ['<1, 1, 1, 2, 1, 0, 1>', 'C64 L16 nseq64']),     # 64 < 256 sequences: IO16 FULL
    ((1, 16, 8, 8, 64), True, False, 'attention_h8_kernel', ['<1, 1, 1, 2, 1, 1, 0>', 'C64 L16 nseq64']),      # ... with the e4m3 core (no FULL form of it)
    ((1, 16, 8, 8, 64), False, True, 'attention_h8_kernel', ['<1, 1, 1, 2, 1, 0, 1>', 'C64 L16 nseq64']),      # ... head-isolating Wo
    ((1, 10, 8, 8, 64), False, False, 'attention_h8_kernel', ['<1, 1, 1, 2, 1, 0, 0>', 'C64 L10 nseq64']),     # masked
    ((1, 16, 8, 8, 128), False, False, 'attention_h8_kernel', ['<1, 2, 1, 4, 1, 0, 1>', 'C128 L16 nseq64']),   # C = 128 (attention_w serves 64 / 32 only), full
    ((1, 10, 6, 6, 128), False, False, 'attention_h8_kernel', ['<1, 2, 1, 4, 1, 0, 0>', 'C128 L10 nseq36']),   # C = 128 masked, 9 workgroups
    ((1, 10, 8, 8, 32), False, False, 'attention_h8_kernel', ['<1, 1, 1, 1, 1, 0, 0>', 'C32 L10 nseq64']),     # C = 32 below the threshold
    ((1, 10, 6, 6, 128), True, False, 'attention_h8_kernel', ['<1, 2, 1, 4, 1, 1, 0>', 'C128 L10 nseq36']),    # C = 128 masked with the e4m3 core: level 1 of the N shape's fp8 sampling
]


@pytest.mark.parametrize('shape,fp8,iso,kernel,parts', ATTN16)
def test_attention_bf16_tensors_per_group(shape, fp8, iso, kernel, parts):
    c = AC.attn_case(shape, True, True, 'bf16', fp8, iso)
    what = f'attention bf16 tensors {shape} fp8={int(fp8)} iso={int(iso)}'
    y, rec = _run_attention(c, 'bf16', True, fp8, what)
    assert_launches(rec, [(kernel, parts)], what)
    PR.assert_first(PR.cid('attention16', shape, fp8, iso), rec)
    assert y.dtype == BF
    _check(c, y, what)


# What vdx_attention_forward_bf16 runs where neither attention_w nor attention_h8 has a form: attention_kernel <1, LP, TMO> for 17..64 tokens
# (the dim-128 configuration on bf16 tensors: 32 frames, every width of its levels) and attention_reg_kernel <1, TMA, fp8> for channel
# counts / sequence counts attention_h8 does not take (the dim-16 model).  Both scale q before they round it; "io16 1" in the shape string.
ATTN16_GENERIC = [
    # shape (B, F, H, W, C), temporal, kernel, parts of the shape string
    ((1, 32, 1, 3, 128), True, 'attention_kernel', ['<1, 32, 2>', 'C128 L32 nseq3', 'io16 1']),            # 3 sequences, 2 per workgroup: the last one half empty
    ((1, 32, 1, 3, 256), True, 'attention_kernel', ['<1, 32, 4>', 'C256 L32 nseq3', 'io16 1']),
    ((1, 20, 1, 3, 512), True, 'attention_kernel', ['<1, 32, 8>', 'C512 L20 nseq3', 'io16 1']),            # keys 20..31 masked
    ((1, 32, 1, 2, 1024), True, 'attention_kernel', ['<1, 32, 16>', 'C1024 L32 nseq2', 'io16 1']),
    ((2, 4, 3, 3, 16), True, 'attention_reg_kernel', ['<1, 4, fp8 0>', 'C16 L4 nseq18', 'io16 1']),        # 18 sequences: 5 workgroups of 4, the last one half empty
    ((1, 2, 2, 2, 128), False, 'attention_reg_kernel', ['<1, 8, fp8 0>', 'C128 L4 nseq2', 'io16 1']),      # 4 tokens of a 2 x 2 bottleneck, 2 sequences
]


@pytest.mark.parametrize('shape,temporal,kernel,parts', ATTN16_GENERIC)
def test_attention_bf16_tensors_generic_kernels_per_group(shape, temporal, kernel, parts):
    c = AC.attn_case(shape, temporal, True, 'bf16', False, False, True)
    what = f'attention bf16 tensors, generic kernels {shape} temporal={int(temporal)}'
    y, rec = _run_attention(c, 'bf16', True, False, what)
    assert_launches(rec, [(kernel, parts)], what)
    PR.assert_first(PR.cid('attention16 generic', shape, temporal), rec)
    assert y.dtype == BF
    _check(c, y, what)


# ---- attention on fp32 tensors (vdx_attention_forward_ex, modes f32 and bf16) ----------------------------------------------------------------
# f32 packs rows in K tiles of 32 channels, bf16 of 64: nkt = CPad / KT.  attention_h8 takes C = 64 (nkt 1 or 2) and C = 128 with nkt = 2,
# so C = 128 in f32 mode (nkt = 4) goes to attention_reg_kernel, like every C it has no form for; more than 16 tokens: attention_kernel
# <MODE, LP, TMO>.  attention_reg_kernel and attention_kernel scale q before they round it (q_scaled).  attention_reg "<MODE, TMA, fp8>".
# Mode f16 (MODE 2) has no attention_h8 / attention_w form at all: attention_reg_kernel up to 16 tokens, attention_kernel beyond; its cases
# are held to the closeness-to-emulation check as well (_check).  The shapes only fp16 mode needs are in tests/test_gpu_f16_forms.py.
ATTN32 = [
    # shape, temporal, iso, {mode: (kernel, parts, q_scaled)}
    ((1, 16, 8, 8, 64), True, False, {'f32': ('attention_h8_kernel', ['<0, 2, 1, 2, 0, 0, 0>', 'C64 L16 nseq64'], False),       # the nkt = 2 f32 form
                                      'bf16': ('attention_h8_kernel', ['<1, 1, 1, 2, 0, 0, 0>', 'C64 L16 nseq64'], False),
                                      'f16': ('attention_reg_kernel', ['<2, 4, fp8 0>', 'C64 L16 nseq64'], True)}),               # the shape the other modes serve with attention_h8
    ((1, 10, 6, 6, 128), True, False, {'f32': ('attention_reg_kernel', ['<0, 8, fp8 0>', 'C128 L10 nseq36'], False),            # 128 / 32 = 4 K tiles: no h8 form
                                       'bf16': ('attention_h8_kernel', ['<1, 2, 1, 4, 0, 0, 0>', 'C128 L10 nseq36'], False),
                                       'f16': ('attention_reg_kernel', ['<2, 8, fp8 0>', 'C128 L10 nseq36'], True)}),             # keys 10..15 masked
    ((1, 16, 2, 2, 256), True, False, {'f32': ('attention_reg_kernel', ['<0, 16, fp8 0>', 'C256 L16 nseq4'], False),
                                       'bf16': ('attention_reg_kernel', ['<1, 16, fp8 0>', 'C256 L16 nseq4'], True),
                                       'f16': ('attention_reg_kernel', ['<2, 16, fp8 0>', 'C256 L16 nseq4'], True)}),
    ((1, 2, 5, 5, 64), False, False, {'f32': ('attention_kernel', ['<0, 32, 1>', 'C64 L25 nseq2'], False),                       # 25 tokens -> LP 32, keys 25..31 masked
                                      'bf16': ('attention_kernel', ['<1, 32, 1>', 'C64 L25 nseq2'], True),
                                      'f16': ('attention_kernel', ['<2, 32, 1>', 'C64 L25 nseq2'], True)}),
    ((1, 3, 8, 8, 128), False, False, {'f32': ('attention_kernel', ['<0, 64, 2>', 'C128 L64 nseq3'], False),
                                       'bf16': ('attention_kernel', ['<1, 64, 2>', 'C128 L64 nseq3'], True),
                                       'f16': ('attention_kernel', ['<2, 64, 2>', 'C128 L64 nseq3'], True)}),
    # 9 sequences (inner = 9 is no multiple of 4: no h8 form in any mode): 3 workgroups of 4, the last one with a single sequence
    ((1, 10, 3, 3, 64), True, False, {'f32': ('attention_reg_kernel', ['<0, 4, fp8 0>', 'C64 L10 nseq9'], False),
                                      'bf16': ('attention_reg_kernel', ['<1, 4, fp8 0>', 'C64 L10 nseq9'], True),
                                      'f16': ('attention_reg_kernel', ['<2, 4, fp8 0>', 'C64 L10 nseq9'], True)}),
    # 32 frames (the temporal attention of BASELINE configs[3]): LP 32, workgroups of 2 sequences, 3 sequences: the last one half empty
    ((1, 32, 1, 3, 128), True, False, {'f32': ('attention_kernel', ['<0, 32, 2>', 'C128 L32 nseq3'], False),
                                       'bf16': ('attention_kernel', ['<1, 32, 2>', 'C128 L32 nseq3'], True),
                                       'f16': ('attention_kernel', ['<2, 32, 2>', 'C128 L32 nseq3'], True)}),
]


@pytest.mark.parametrize('mode', ['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('shape,temporal,iso,expect', ATTN32)
def test_attention_fp32_tensors_per_group(shape, temporal, iso, expect, mode):
    kernel, parts, q_scaled = expect[mode]
    c = AC.attn_case(shape, temporal, False, mode, False, iso, q_scaled)
    what = f'attention fp32 tensors {shape} temporal={int(temporal)} {mode}'
    y, rec = _run_attention(c, mode, False, False, what)
    assert_launches(rec, [(kernel, parts)], what)
    PR.assert_first(PR.cid('attention32', shape, temporal, iso, mode), rec)
    _check(c, y, what)


# ---- SLA on bf16 tensors (vdx_sla_forward_bf16) ------------------------------------------------------------------------------------------
# sla_plan: tiles = N / 64, nsub = min(tiles, 8) sub-tiles per chunk; launch_sla_m doubles nsub while NF x chunks stays >= 1024 workgroups.
# sla_ctx8_kernel writes ctxT itself when a frame is one chunk, else partials + sla_combine_kernel.  Second half: sla_out_w_kernel for
# C = 64, N >= 2048, NF >= 128 (persistent_split(NF, 256 CUs) frames per workgroup), else sla_out8_kernel <MODE, NKT, TMO, TNO, IO16>.
def _sla16(C, N, NF, nchunk, out):
    nkt = 2 if C == 128 else 1
    seq = [('sla_ctx8_kernel', [f'<1, {nkt}, 1>', f'C{C} N{N} NF{NF} nchunk{nchunk}'])]
    if nchunk > 1:
        seq.append(('sla_combine_kernel', [f'NF{NF} nchunk{nchunk}']))
    if out == 'w':
        seq.append(('sla_out_w_kernel', [f'C{C} N{N} NF{NF}']))
    else:
        seq.append(('sla_out8_kernel', [f'<1, {nkt}, 1, {out}, 1>', f'C{C} N{N} NF{NF}']))
    return seq


SLA16 = [
    # shape, iso, launches
    ((8, 16, 64, 32, 64), False, _sla16(64, 2048, 128, 4, 'w')),       # 32 tiles: nsub 8, 4 chunks (128 x 2 < 1024: not doubled); 128 frames <= 256 CUs: one per workgroup
    ((8, 16, 64, 32, 64), True, _sla16(64, 2048, 128, 4, 'w')),        # ... head-isolating to_out
    ((7, 37, 64, 32, 64), False, _sla16(64, 2048, 259, 4, 'w')),       # 259 frames > 256 CUs: ceil(259 / 256) = 2 per workgroup, 130 workgroups, the last one has 1 frame
    ((13, 10, 32, 32, 64), False, _sla16(64, 1024, 130, 2, 2)),        # N < 2048: sla_out8, 16 tiles = 2 chunks + combine
    ((1, 16, 32, 32, 64), False, _sla16(64, 1024, 16, 2, 2)),          # few frames
    ((1, 16, 32, 32, 64), True, _sla16(64, 1024, 16, 2, 2)),           # ... head-isolating to_out
    ((8, 16, 16, 16, 64), False, _sla16(64, 256, 128, 1, 2)),          # 4 tiles = one chunk per frame: sla_ctx8 writes ctxT itself, no combine
    ((2, 10, 16, 16, 32), False, _sla16(32, 256, 20, 1, 1)),           # C = 32 form
    ((1, 4, 16, 16, 128), False, _sla16(128, 256, 4, 1, 4)),           # C = 128 form
    ((32, 16, 64, 32, 64), False, _sla16(64, 2048, 512, 2, 'w')),      # 512 frames: 512 x (32 / 16) = 1024 workgroups -> nsub doubled to 16, 2 chunks: the many-frames plan of the benchmark
    # widths without a one-wave-per-head form (16 of the dim-16 model, 1024 of the dim-128 bottleneck): the generic kernels on bf16 tensors
    ((1, 2, 8, 8, 16), False, [('sla_ctx_kernel', ['<1>', 'C16 N64 NF2 nchunk1', 'io16 1']), ('sla_combine_kernel', ['<1>', 'NF2 nchunk1']),
                               ('sla_out_kernel', ['<1, 1>', 'C16 N64 NF2', 'io16 1'])]),
]


@pytest.mark.parametrize('shape,iso,expect', SLA16)
def test_sla_bf16_tensors_per_group(shape, iso, expect):
    c = AC.sla_case(shape, True, 'bf16', iso)
    what = f'SLA bf16 tensors {shape} iso={int(iso)}'
    y, rec = _run_sla(c, 'bf16', True, what)
    assert_launches(rec, expect, what)
    PR.assert_first(PR.cid('sla16', shape, iso), rec)
    assert y.dtype == BF
    _check(c, y, what)


# ---- SLA on fp32 tensors (vdx_sla_forward, modes f32 and bf16) ---------------------------------------------------------------------------
# one wave per head (sla_ctx8 / sla_out8) for C = 64 with nkt 1 or 2 and C = 128 with nkt = 2; everything else -- C = 128 in f32 mode (4 K
# tiles), C = 256, C = 16 -- runs the generic sla_ctx_kernel -> sla_combine_kernel -> sla_out_kernel <MODE, TMO>.
def _sla32(mode, C, N, NF, nchunk):
    m = {'f32': 0, 'bf16': 1, 'f16': 2}[mode]
    nkt = -(-C // (32 if mode == 'f32' else 64))
    if mode != 'f16' and ((C == 64 and nkt <= 2) or (C == 128 and nkt == 2)):      # (f16 has no one-wave-per-head form: always generic)
        seq = [('sla_ctx8_kernel', [f'<{m}, {nkt}, 0>', f'C{C} N{N} NF{NF} nchunk{nchunk}'])]
        if nchunk > 1:
            seq.append(('sla_combine_kernel', [f'<{m}>', f'NF{NF} nchunk{nchunk}']))
        return seq + [('sla_out8_kernel', [f'<{m}, {nkt}, 1, {2 if C == 64 else 4}, 0>', f'C{C} N{N} NF{NF}'])]
    tmo = 1 if C <= 64 else 2 if C <= 128 else 4 if C <= 256 else 8 if C <= 512 else 16
    return [('sla_ctx_kernel', [f'<{m}>', f'C{C} N{N} NF{NF} nchunk{nchunk}']), ('sla_combine_kernel', [f'<{m}>', f'NF{NF} nchunk{nchunk}']),
            ('sla_out_kernel', [f'<{m}, {tmo}>', f'C{C} N{N} NF{NF}'])]


SLA32 = [
    # shape, iso, chunks
    ((1, 2, 64, 64, 64), False, 8),        # N = 4096: 64 tiles = 8 chunks of 8, the online-softmax rescale across chunks
    ((2, 3, 8, 8, 128), False, 1),         # N = 64: one tile; f32: the generic kernels, bf16: one wave per head
    ((1, 1, 24, 24, 256), False, 2),       # generic kernels, 9 tiles = 8 + 1: ragged second chunk
    ((1, 1, 24, 24, 256), True, 2),        # ... head-isolating to_out
    ((1, 2, 5, 7, 16), False, 1),          # N = 35: one ragged tile
]


@pytest.mark.parametrize('mode', ['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('shape,iso,nchunk', SLA32)
def test_sla_fp32_tensors_per_group(shape, iso, nchunk, mode):
    B, Fr, H, W, C = shape
    c = AC.sla_case(shape, False, mode, iso)
    what = f'SLA fp32 tensors {shape} {mode} iso={int(iso)}'
    y, rec = _run_sla(c, mode, False, what)
    assert_launches(rec, _sla32(mode, C, H * W, B * Fr, nchunk), what)
    PR.assert_first(PR.cid('sla32', shape, iso, mode), rec)
    _check(c, y, what)
