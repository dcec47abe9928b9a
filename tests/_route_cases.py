"""Which kernel form a forward call of libvdx reaches (the host routing of launch_conv, launch_attention, launch_sla and of the block
compositions of model.hip), shared by tests/test_host_routes.py and the recorder at the bottom.  A plain module: nothing here is collected.

Every launcher reports its launch to the hook (vdx_set_launch_hook) BEFORE its first runtime call, so without a device a call that passes
validation returns VDX_ERR_HIP having reported the first launch of its route, and a refused call returns VDX_ERR_INVALID having reported
none.  Pointers are the stand-in host array of tests/_api_cases.py: nothing is read or written, so the shapes are the workload's own
(640 frames of 64 x 64) and the thresholds are met at their real values.  Two groups of cases:

  * the network: every conv, attention and SLA block of model_build's level table with the flags model.hip sets, for the N shape (dim 64,
    10 frames, 64 x 64) at B = 64 (sampling: bf16 storage) and B = 4 (training forward: fp32 and bf16 storage), the Y shape (dim 32), the
    dim-128 configuration (32 frames, 128 x 128, fp16 operands) and a dim-16 tiny model in the three modes;
  * the edges: one case on each side of every condition of every predicate.

    VDX_LIB=/path/to/libvdx.so python tests/_route_cases.py > table.json

records {case id: [status, [[kernel, label], ...]]}; tests/golden/kernel_routes.json is that table."""
import ctypes as C
import json
import os
import sys

import _api_cases as A
from _launch_hook import launches

F32, BF16, F16 = 0, 1, 2
BUF = A.BUF
G = 8                                                       # resnet_groups
W_MIN_N = 2048                                              # VDX_SLA_W_MIN_N (sla.hip)
PREPASS_MIN_C = 256                                         # VDX_PREPASS_MIN_C (model.hip)


class ConvDesc(C.Structure):                                # vdx_conv_desc (include/vdx.h)
    _fields_ = [('x0', C.c_void_p), ('x1', C.c_void_p), ('c0', C.c_int), ('c1', C.c_int), ('packed_w', C.c_void_p), ('bias', C.c_void_p),
                ('y', C.c_void_p), ('cout', C.c_int), ('batch', C.c_int), ('frames', C.c_int), ('h', C.c_int), ('w', C.c_int),
                ('kind', C.c_int), ('kh', C.c_int), ('kw', C.c_int), ('stride', C.c_int),
                ('in_stats', C.c_void_p), ('gamma', C.c_void_p), ('beta', C.c_void_p), ('groups', C.c_int),
                ('scale_shift', C.c_void_p), ('scale_shift_stride', C.c_int), ('out_stats', C.c_void_p), ('out_groups', C.c_int),
                ('x_bf16', C.c_int), ('y_bf16', C.c_int), ('res', C.c_void_p), ('res_bf16', C.c_int)]


# ---- one call = (entry, values); conv() and the attention / SLA helpers below build the values the way model.hip fills its arguments -----
def conv(mode, c0, cout, batch, frames, s, k=3, c1=0, stride=1, kind=0, pro=0, stats=0, x16=0, y16=0, res=None, w=None, rows=None, groups=G, out_groups=G):
    """res: None or the residual's res_bf16; rows: None or (w_rows, w_row0) of vdx_conv_forward_rows"""
    d = dict(x0=BUF, x1=BUF if c1 else 0, c0=c0, c1=c1, packed_w=BUF, bias=BUF, y=BUF, cout=cout, batch=batch, frames=frames, h=s, w=w or s,
             kind=kind, kh=k, kw=k, stride=stride, x_bf16=x16, y_bf16=y16)
    if pro:
        d.update(in_stats=BUF, gamma=BUF, beta=BUF, groups=groups, scale_shift=BUF, scale_shift_stride=2 * c0)
    if stats:
        d.update(out_stats=BUF, out_groups=out_groups)
    if res is not None:
        d.update(res=BUF, res_bf16=res)
    return ('conv_forward_rows', dict(mode=mode, desc=d, w_rows=rows[0], w_row0=rows[1])) if rows else ('conv_forward', dict(mode=mode, desc=d))


def _geo(batch, frames, h, w, c, **more):
    return dict(batch=batch, frames=frames, h=h, w=w, c=c, **more)


def _head_lds(c):                                           # the per-head weight image of the wide-level kernels fits the 160 KB of LDS
    return 96 * (c * 2 + 32) <= 160 * 1024


def attention(mode, a16, batch, frames, h, w, c, temporal, heads=8, fp8=0, bias=0, focus=0, present=0):
    """the entry that stands for run_attn with these switches (model.hip: attention_block_forward decides heads / long / present / fused)"""
    L = frames if temporal else h * w
    g = _geo(batch, frames, h, w, c)
    if present:
        return 'attention_present_forward', dict(g, mode=mode, io_bf16=a16, heads=heads, temporal=temporal)
    if focus:
        return 'attention_forward_focus', dict(g, mode=mode, io_bf16=a16, heads=heads, temporal=temporal, bias=BUF if bias else 0, focus_n=batch)
    if bias:
        return 'attention_forward_bias', dict(g, mode=mode, io_bf16=a16, heads=heads, temporal=temporal)
    if L > 64:
        return 'attention_long_forward', dict(g, mode=mode, io_bf16=a16, heads=heads, scratch_bytes=('size', 'attention_long_scratch_bytes', 'batch frames h w heads'))
    if mode == BF16 and heads == 8 and c >= 256 and c % 128 == 0 and _head_lds(c) and L <= (16 if temporal else 64):
        return 'attention_heads_forward', dict(g, io_bf16=a16, temporal=temporal, fp8=fp8, scratch_bytes=('size', 'attention_heads_scratch_bytes', 'batch frames h w'))
    if a16:
        return 'attention_forward_bf16', dict(g, heads=heads, temporal=temporal, fp8=fp8)
    return 'attention_forward_ex', dict(g, mode=mode, heads=heads, temporal=temporal, fp8=fp8)


def sla(mode, a16, batch, frames, s, c, w=None):
    g = _geo(batch, frames, s, w or s, c)
    if mode == BF16 and c >= 256 and c % 128 == 0 and _head_lds(c) and (s * (w or s)) % 16 == 0:
        return 'sla_heads_forward', dict(g, io_bf16=a16, scratch_bytes=('size', 'attention_heads_scratch_bytes', 'batch frames h w'))
    if a16:
        return 'sla_forward_bf16', dict(g, heads=8)
    return 'sla_forward', dict(g, mode=mode, heads=8)


# ---- the network: model_build's level table and the flags of run_res / run_attn / run_sla / run_resample (model.hip) ------------------
def _tail_rc16(cin, c0, cout, pix):                         # elementwise.hip: tail_rc16_supported
    shape = (cin, cout) in ((128, 64), (64, 128), (256, 64), (128, 256), (64, 32), (32, 64), (128, 32))
    return shape and c0 in (cin, cin // 2) and pix % 16 == 0 and pix * max(cin, cout) * 2 < 1 << 31


def network(dim, batch, frames, size, mode, act16, fp8=0, mults=(1, 2, 4, 8)):
    """[(block name, entry, values)]; act16: 0 fp32 storage, 1 bf16 storage of the sampling forward, 2 of the training forward"""
    a16 = 1 if act16 and mode == BF16 else 0
    half = 1 if mode == BF16 else 0
    out = []

    def res(name, c0, c1, cout, lvl):
        s = size >> lvl
        out.append((f'{name}.conv1', *conv(mode, c0, cout, batch, frames, s, c1=c1, stats=1, x16=a16, y16=half)))
        prepass = half and act16 == 1 and cout >= PREPASS_MIN_C
        out.append((f'{name}.conv2', *conv(mode, cout, cout, batch, frames, s, pro=0 if prepass else 1, stats=1, x16=half, y16=half)))
        if c0 + c1 != cout and not (a16 and act16 == 1 and _tail_rc16(c0 + c1, c0, cout, frames * s * s)):
            out.append((f'{name}.res_conv', *conv(mode, c0, cout, batch, frames, s, k=1, c1=c1, x16=a16, y16=a16)))

    def attn(name, c, lvl, temporal):
        s = size >> lvl
        entry, v = attention(mode, a16, batch, frames, s, s, c, temporal, fp8=fp8)
        out.append((name, entry, v))
        HD = 256
        if entry == 'attention_heads_forward':              # its out-projection: a 1x1 conv on the bf16 per-head output, + bias + residual
            out.append((f'{name}.to_out', *conv(mode, HD, c, batch, frames, s, k=1, x16=1, y16=a16, res=a16)))
        if entry == 'attention_long_forward':               # q|k|v projection and out-projection around the fp32 core
            out.append((f'{name}.to_qkv', *conv(mode, c, 3 * HD, batch, frames, s, k=1, x16=a16)))
            out.append((f'{name}.to_out', *conv(mode, HD, c, batch, frames, s, k=1, y16=a16, res=a16)))

    def level(name, c0, c1, cout, lvl, resample):
        s = size >> lvl
        res(f'{name}.0', c0, c1, cout, lvl)
        res(f'{name}.1', cout, 0, cout, lvl)
        entry, v = sla(mode, a16, batch, frames, s, cout)
        out.append((f'{name}.2', entry, v))
        if entry == 'sla_heads_forward':
            out.append((f'{name}.2.to_out', *conv(mode, 256, cout, batch, frames, s, k=1, x16=1, y16=a16, res=a16)))
        attn(f'{name}.3', cout, lvl, 1)
        if resample == 'down':
            out.append((f'{name}.4', *conv(mode, cout, cout, batch, frames, s, k=4, stride=2, x16=a16, y16=a16)))
        if resample == 'up':
            out.append((f'{name}.4', *conv(mode, cout, cout, batch, frames, s, k=4, kind=1, x16=a16, y16=a16)))

    dims = [dim] + [dim * m for m in mults]
    nl = len(mults)
    attn('init_temporal_attn', dim, 0, 1)
    for i in range(nl):
        level(f'downs.{i}', dims[i], 0, dims[i + 1], i, 'down' if i < nl - 1 else None)
    res('mid_block1', dims[nl], 0, dims[nl], nl - 1)
    attn('mid_spatial_attn', dims[nl], nl - 1, 0)
    attn('mid_temporal_attn', dims[nl], nl - 1, 1)
    res('mid_block2', dims[nl], 0, dims[nl], nl - 1)
    cur = dims[nl]
    for i in range(nl):
        din, dout = dims[nl - 1 - i], dims[nl - i]
        level(f'ups.{i}', cur, dout, din, nl - 1 - i, 'up' if i < nl - 1 else None)
        cur = din
    res('final_conv.0', dim, dim, dim, 0)
    return out


NETWORKS = [
    ('N sampling B64', dict(dim=64, batch=64, frames=10, size=64, mode=BF16, act16=1)),
    ('N sampling B64 fp8', dict(dim=64, batch=64, frames=10, size=64, mode=BF16, act16=1, fp8=1)),
    ('N training B4 fp32 storage', dict(dim=64, batch=4, frames=10, size=64, mode=BF16, act16=0)),
    ('N training B4 bf16 storage', dict(dim=64, batch=4, frames=10, size=64, mode=BF16, act16=2)),
    ('Y sampling B64', dict(dim=32, batch=64, frames=10, size=64, mode=BF16, act16=1)),
    ('Y training B4 bf16 storage', dict(dim=32, batch=4, frames=10, size=64, mode=BF16, act16=2)),
    ('dim128 B1 fp16', dict(dim=128, batch=1, frames=32, size=128, mode=F16, act16=0)),
    ('dim128 B1 bf16 storage', dict(dim=128, batch=1, frames=32, size=128, mode=BF16, act16=1)),
    ('tiny f32', dict(dim=16, batch=2, frames=4, size=16, mode=F32, act16=0)),
    ('tiny bf16', dict(dim=16, batch=2, frames=4, size=16, mode=BF16, act16=1)),
    ('tiny f16', dict(dim=16, batch=2, frames=4, size=16, mode=F16, act16=0)),
]


# ---- the edges: each side of every condition of every predicate -------------------------------------------------------------------------
def edges():
    e = []

    def add(label, call):
        e.append((label, *call))

    b16 = dict(x16=1, y16=1)
    # the level-0 persistent forms (conv_igemm.hip): at least 1024 whole 16 x 16 tiles, by input format, prologue and residual
    for nf in (1023, 1024):
        add(f'conv64r tiles {nf}', conv(BF16, 64, 64, nf, 1, 16, **b16))
        add(f'conv64q pro tiles {nf}', conv(BF16, 64, 64, nf, 1, 16, pro=1, **b16))
        add(f'conv64d tiles {nf}', conv(BF16, 64, 64, nf, 1, 16, x16=1, y16=0, res=0))
        add(f'conv64p tiles {nf}', conv(BF16, 64, 64, nf, 1, 16, pro=1, y16=1))
        add(f'conv64p c32 tiles {nf}', conv(BF16, 32, 32, nf, 1, 16, pro=1, **b16))
        add(f'conv64q cout32 tiles {nf}', conv(BF16, 32, 32, nf, 1, 16, c1=32, **b16))
        add(f'conv64q cin128 tiles {nf}', conv(BF16, 64, 64, nf, 1, 16, c1=64, **b16))
    for h, w in ((16, 24), (24, 16), (32, 48)):
        add(f'conv64r {h}x{w}', conv(BF16, 64, 64, 2048, 1, h, w=w, **b16))
        add(f'conv3x3_ws 128 {h}x{w}', conv(BF16, 128, 128, 2048, 1, h, w=w, **b16))
    for y16 in (0, 1):
        for pro in (0, 1):
            add(f'conv64 x16 pro {pro} y16 {y16}', conv(BF16, 64, 64, 64, 10, 64, pro=pro, stats=1, x16=1, y16=y16))
            add(f'conv64 x32 pro {pro} y16 {y16}', conv(BF16, 64, 64, 64, 10, 64, pro=pro, stats=1, x16=0, y16=y16))
        add(f'conv64 128 in y16 {y16}', conv(BF16, 128, 64, 64, 10, 64, stats=1, x16=1, y16=y16))
    add('conv64 res bf16', conv(BF16, 64, 64, 64, 10, 64, x16=1, y16=1, res=1))
    add('conv64 res pro', conv(BF16, 64, 64, 64, 10, 64, x16=1, pro=1, res=0))
    add('conv64 res x32', conv(BF16, 64, 64, 64, 10, 64, res=0))
    add('conv64 f32 mode', conv(F32, 64, 64, 64, 10, 64))
    add('conv64 f16 mode', conv(F16, 64, 64, 64, 10, 64))
    add('conv64 stride 2', conv(BF16, 64, 64, 64, 10, 64, k=4, stride=2, **b16))
    add('conv64 1x1', conv(BF16, 64, 64, 64, 10, 64, k=1, **b16))
    for og in (1, 2, 4, 32, 64):                             # statistics groups the epilogues do not serve go to the generic kernel
        add(f'conv64r out_groups {og}', conv(BF16, 64, 64, 64, 10, 64, stats=1, out_groups=og, **b16))
        add(f'conv64q cin128 out_groups {og}', conv(BF16, 64, 64, 64, 10, 64, c1=64, stats=1, out_groups=og, **b16))
        if og <= 32:
            add(f'conv64q cout32 out_groups {og}', conv(BF16, 32, 32, 64, 10, 64, c1=32, stats=1, out_groups=og, **b16))
            add(f'conv64p c32 out_groups {og}', conv(BF16, 32, 32, 64, 10, 64, stats=1, out_groups=og, **b16))
    for g in (1, 4, 32, 64):
        add(f'conv64q pro groups {g}', conv(BF16, 64, 64, 64, 10, 64, pro=1, groups=g, **b16))
    add('conv64q cout32 128 in', conv(BF16, 64, 32, 64, 10, 32, c1=64, **b16))
    add('conv64q cout32 y32', conv(BF16, 32, 32, 64, 10, 64, c1=32, x16=1, y16=0))
    add('conv64q cout32 pro', conv(BF16, 64, 32, 64, 10, 64, pro=1, **b16))
    add('conv64p c32 y32', conv(BF16, 32, 32, 64, 10, 64, x16=1, y16=0))
    add('conv64p c32 x32', conv(BF16, 32, 32, 64, 10, 64, x16=0, y16=1))
    # weight-row slices (the data gradients of the backward run as forward convs on a slice of a wider packing)
    for rows in ((64, 0), (128, 0), (128, 64), (192, 128)):
        add(f'conv64r rows {rows}', conv(BF16, 64, 64, 64, 10, 64, rows=rows, **b16))
        add(f'conv64q cin128 rows {rows}', conv(BF16, 64, 64, 64, 10, 64, c1=64, rows=rows, **b16))
    add('conv3x3_ws rows (256, 128)', conv(BF16, 128, 128, 64, 10, 32, rows=(256, 128), **b16))
    add('conv3x3_ws rows (128, 0)', conv(BF16, 128, 128, 64, 10, 32, rows=(128, 0), **b16))
    add('conv1x1 rows (768, 256)', conv(BF16, 128, 256, 64, 10, 32, k=1, rows=(768, 256), **b16))
    # 32-bit limits: a 4 GiB fp32 output of the 64 -> 64 forms, 256-byte input pixels of the 128 -> 64 form, a 4 GiB input of launch_conv itself
    for nf in (4095, 4096):
        add(f'conv64r y32 frames {nf}', conv(BF16, 64, 64, nf, 1, 64, x16=1, y16=0))
        add(f'conv64q cin128 concat frames {nf}', conv(BF16, 64, 64, nf, 1, 64, c1=64, **b16))
        add(f'conv 128 in frames {nf}', conv(BF16, 128, 64, nf, 1, 64, **b16))
    for nf, fr in ((65534, 2), (65535, 5)):                  # 128 input channels x 2 bytes x pixels at the 0xFFFF0000 limit of the weight-streaming kernels
        add(f'conv3x3_ws 128 frames {nf}', conv(BF16, 128, 128, nf // fr, fr, 16, **b16))
        add(f'conv1x1_pw 128 frames {nf}', conv(BF16, 128, 128, nf // fr, fr, 16, k=1, **b16))
    # the wide levels (conv_ws.hip, conv_pw.hip): tiles x output-channel tiles 127 / 128, frame geometries, channel steps
    for nf in (508, 512):
        add(f'conv3x3_ws 128->128 8x8 frames {nf}', conv(BF16, 128, 128, nf // 4, 4, 8, **b16))
    for nf in (252, 256):
        add(f'conv3x3_ws 256->256 8x8 frames {nf}', conv(BF16, 256, 256, nf // 4, 4, 8, pro=1, stats=1, **b16))
    for nf in (127, 128):
        add(f'conv3x3_ws 128->128 16x16 frames {nf}', conv(BF16, 128, 128, 1, nf, 16, **b16))
        add(f'conv4x4_ws down 128 32x32 frames {nf}', conv(BF16, 128, 128, 1, nf, 32, k=4, stride=2, **b16))
        add(f'conv4x4_ws up 128 16x16 frames {nf // 4}', conv(BF16, 128, 128, 1, nf // 4, 16, k=4, kind=1, **b16))
    for s in (8, 16, 32, 64, 12):
        add(f'conv3x3_ws 256 {s}x{s}', conv(BF16, 256, 256, 64, 10, s, **b16))
        add(f'conv3x3_ws 256 pro {s}x{s}', conv(BF16, 256, 256, 64, 10, s, pro=1, stats=1, **b16))
        add(f'conv4x4_ws down 256 {2 * s}x{2 * s}', conv(BF16, 256, 256, 64, 10, 2 * s, k=4, stride=2, **b16))
        add(f'conv4x4_ws up 256 {s}x{s}', conv(BF16, 256, 256, 64, 10, s, k=4, kind=1, **b16))
    add('conv4x4_ws down 64 32x32', conv(BF16, 64, 64, 64, 10, 32, k=4, stride=2, **b16))
    add('conv4x4_ws up 64 16x16', conv(BF16, 64, 64, 64, 10, 16, k=4, kind=1, **b16))
    add('conv4x4_ws down 8x8 frames 642', conv(BF16, 256, 256, 321, 2, 16, k=4, stride=2, **b16))
    add('conv4x4_ws x32', conv(BF16, 256, 256, 64, 10, 32, k=4, stride=2))
    for cout in (128, 256, 384, 512, 640, 1024):
        add(f'conv3x3_ws 128->{cout}', conv(BF16, 128, cout, 64, 10, 16, stats=1, **b16))
    add('conv3x3_ws concat 256+256->256', conv(BF16, 256, 256, 64, 10, 16, c1=256, stats=1, **b16))
    add('conv3x3_ws 96->128', conv(BF16, 96, 128, 64, 10, 16, **b16))
    add('conv3x3_ws 128->192', conv(BF16, 128, 192, 64, 10, 16, **b16))
    add('conv3x3_ws out_groups 32', conv(BF16, 128, 128, 64, 10, 16, stats=1, out_groups=32, **b16))
    add('conv3x3_ws x32', conv(BF16, 128, 128, 64, 10, 16, y16=1))
    add('conv3x3_ws res', conv(BF16, 128, 128, 64, 10, 16, res=1, **b16))
    for cin, cout in ((64, 64), (64, 128), (128, 64), (128, 128), (256, 512), (512, 256), (1024, 1024), (1152, 128), (192, 128), (256, 192)):
        add(f'conv1x1_pw {cin}->{cout}', conv(BF16, cin, cout, 64, 10, 16, k=1, **b16))
        add(f'conv1x1_pw {cin}->{cout} y32', conv(BF16, cin, cout, 64, 10, 16, k=1, x16=1, y16=0))
    add('conv1x1_pw concat 128+128->128', conv(BF16, 128, 128, 64, 10, 16, k=1, c1=128, **b16))
    add('conv1x1_pw concat 64+64->128', conv(BF16, 64, 128, 64, 10, 16, k=1, c1=64, **b16))
    add('conv1x1_pw res y32 res32', conv(BF16, 256, 128, 64, 10, 16, k=1, x16=1, y16=0, res=0))
    add('conv1x1_pw res y16 res32', conv(BF16, 256, 128, 64, 10, 16, k=1, x16=1, y16=1, res=0))
    add('conv1x1_pw res y16 res16', conv(BF16, 256, 128, 64, 10, 16, k=1, x16=1, y16=1, res=1))
    for nf in (31, 32):                                      # 32 x 256 pixels
        add(f'conv1x1_pw pixels {nf * 256}', conv(BF16, 128, 128, 1, nf, 16, k=1, **b16))
    add('conv1x1_pw pixels % 32', conv(BF16, 128, 128, 1, 1000, 3, k=1, **b16))
    # 32-channel resampling (conv_rs.hip)
    for s in (64, 48, 32, 16, 8):
        add(f'resample32 down {s}x{s}', conv(BF16, 32, 32, 64, 10, s, k=4, stride=2, **b16))
        add(f'resample32 up {s}x{s}', conv(BF16, 32, 32, 64, 10, s, k=4, kind=1, **b16))
    add('resample32 x32', conv(BF16, 32, 32, 64, 10, 64, k=4, stride=2))
    # the generic kernel: channel tile, stride, input format, mode
    for mode in (F32, BF16, F16):
        for cout in (64, 68, 128):
            add(f'conv_igemm mode {mode} 36->{cout}', conv(mode, 36, cout, 2, 4, 16))
            add(f'conv_igemm mode {mode} 36->{cout} stride 2', conv(mode, 36, cout, 2, 4, 16, k=4, stride=2))
        add(f'conv_igemm mode {mode} up', conv(mode, 36, 36, 2, 4, 16, k=4, kind=1))
        add(f'conv_igemm mode {mode} 1x1 concat pro-less', conv(mode, 36, 36, 2, 4, 16, k=1, c1=28))
        add(f'conv_igemm mode {mode} pro', conv(mode, 64, 64, 2, 4, 16, pro=1, stats=1))
    add('conv_igemm bf16 one tensor 72', conv(BF16, 72, 64, 2, 4, 16, **b16))
    add('conv_igemm bf16 concat 40+24', conv(BF16, 40, 64, 2, 4, 16, c1=24, **b16))
    add('conv_igemm 1x1 2x2 frames', conv(F32, 64, 64, 2, 4, 2, k=1))
    add('conv_igemm 1x1 1x1 frames', conv(F32, 64, 64, 2, 4, 1, k=1))
    add('conv_igemm pro 1024', conv(F32, 1024, 64, 1, 4, 16, pro=1))

    # attention (attention.hip): sequence length, channel ladder, heads, sequences % 4, storage, fp8, bias, focus, present
    for mode in (F32, BF16, F16):
        for L in (16, 17, 32, 33, 64, 65):
            add(f'attention mode {mode} temporal L {L}', attention(mode, 0, 1, L, 4, 4, 64, 1))
            add(f'attention mode {mode} spatial L {L}', attention(mode, 0, 2, 2, 1, L, 64, 0))
            add(f'attention mode {mode} bias L {L}', attention(mode, 0, 1, L, 4, 4, 64, 1, bias=1))
            add(f'attention mode {mode} focus L {L}', attention(mode, 0, 2, L, 4, 4, 64, 1, focus=1))
            add(f'attention mode {mode} bias+focus L {L}', attention(mode, 0, 2, L, 4, 4, 64, 1, bias=1, focus=1))
        for c in (32, 64, 68, 128, 132, 256, 260, 512, 516, 1024):
            add(f'attention mode {mode} C {c} L 10', attention(mode, 0, 1, 10, 4, 4, c, 1, heads=4))
            add(f'attention mode {mode} C {c} L 10 8 heads', attention(mode, 0, 1, 10, 4, 4, c, 1))
            add(f'attention mode {mode} C {c} L 10 bias', attention(mode, 0, 1, 10, 4, 4, c, 1, bias=1))
            add(f'attention mode {mode} C {c} L 24', attention(mode, 0, 1, 24, 4, 4, c, 1))
            add(f'attention mode {mode} C {c} L 48 focus', attention(mode, 0, 1, 48, 4, 4, c, 1, focus=1))
            add(f'attention mode {mode} C {c} present', attention(mode, 0, 1, 10, 4, 4, c, 1, present=1))
        add(f'attention mode {mode} nseq 3', attention(mode, 0, 1, 10, 1, 3, 64, 1))
        add(f'attention mode {mode} nseq 6', attention(mode, 0, 1, 10, 2, 3, 64, 1))
        add(f'attention mode {mode} spatial nseq 6', attention(mode, 0, 2, 3, 4, 4, 64, 0))
        add(f'attention mode {mode} long 256 tokens', attention(mode, 0, 1, 2, 16, 16, 128, 0))
        add(f'attention mode {mode} long temporal', attention(mode, 0, 1, 65, 16, 16, 128, 1))
    for c in (32, 64, 128, 256):
        for L in (10, 16):
            for fp8 in (0, 1):
                add(f'attention bf16 storage C {c} L {L} fp8 {fp8}', attention(BF16, 1, 64, L, 64, 64, c, 1, fp8=fp8))
                add(f'attention bf16 storage small C {c} L {L} fp8 {fp8}', attention(BF16, 1, 1, L, 8, 8, c, 1, fp8=fp8))
                add(f'attention bf16 fp32 storage C {c} L {L} fp8 {fp8}', attention(BF16, 0, 4, L, 64, 64, c, 1, fp8=fp8))
    for nseq_hw in ((15, 17), (16, 16)):                     # attention_w: whole groups of 4 sequences, at least 256 of them
        add(f'attention_w nseq {nseq_hw[0] * nseq_hw[1]}', attention(BF16, 1, 1, 10, *nseq_hw, 64, 1))
    add('attention_w nseq 252', attention(BF16, 1, 1, 10, 14, 18, 64, 1))
    add('attention_w spatial', attention(BF16, 1, 64, 4, 4, 4, 64, 0))
    add('attention bias bf16 storage', attention(BF16, 1, 64, 10, 64, 64, 64, 1, bias=1))
    add('attention focus bf16 storage', attention(BF16, 1, 64, 10, 64, 64, 64, 1, focus=1))
    for c in (256, 384, 512, 1024):
        for L, temporal in ((10, 1), (16, 1), (17, 1), (64, 0), (16, 0)):
            fr, h = (L, 8) if temporal else (2, {64: 8, 16: 4}[L])
            add(f'attention heads C {c} L {L} temporal {temporal}', attention(BF16, 1, 4, fr, h, h, c, temporal))
        add(f'attention heads C {c} fp8', attention(BF16, 1, 4, 10, 8, 8, c, 1, fp8=1))
        add(f'attention heads C {c} fp32 storage', attention(BF16, 0, 4, 10, 8, 8, c, 1))
        add(f'attention heads C {c} bias', attention(BF16, 1, 4, 10, 8, 8, c, 1, bias=1))
    add('attention heads 4 heads', attention(BF16, 1, 4, 10, 8, 8, 256, 1, heads=4))
    add('attention heads scratch short', ('attention_heads_forward', dict(_geo(4, 10, 8, 8, 256), io_bf16=1, temporal=1, fp8=0, scratch_bytes=1024)))

    # SLA (sla.hip): the one-wave-per-head forms by width and storage, the chunk plan, sla_out_w's frames and pixels (the first launch of
    # the chain is sla_ctx8_kernel on both sides), the generic form's channel ladder
    for mode in (F32, BF16, F16):
        for c in (32, 64, 68, 128, 132, 192, 256, 260, 512, 516, 1024):
            add(f'sla mode {mode} C {c}', sla(mode, 0, 2, 4, 16, c))
        for s in (4, 8, 24, 32, 64):
            add(f'sla mode {mode} C 64 {s}x{s}', sla(mode, 0, 2, 4, s, 64))
    for c in (32, 64, 128, 256, 512):
        add(f'sla bf16 storage C {c}', sla(BF16, 1, 64, 10, 32, c))
        add(f'sla bf16 storage C {c} N 15x15', sla(BF16, 1, 4, 10, 15, c))
    for nf in (127, 128):
        for s, w in ((32, 32), (32, 64), (64, 64)):          # N = 1024, 2048 (VDX_SLA_W_MIN_N), 4096
            add(f'sla_out_w NF {nf} N {s * w}', sla(BF16, 1, 1, nf, s, 64, w=w))
    assert 32 * 64 == W_MIN_N
    for nf in (15, 16, 255, 256, 1023, 1024):                # the chunk plan doubles while VDX_SLA_MIN_WGS workgroups remain
        add(f'sla chunks NF {nf} N 4096', sla(BF16, 1, 1, nf, 64, 64))
    return e


def all_cases():
    """[(case id, entry, values)]"""
    out = [(f'{net}: {name}', entry, v) for net, kw in NETWORKS for name, entry, v in network(**kw)]
    out += [(f'edge: {label}', entry, v) for label, entry, v in edges()]
    ids = [c[0] for c in out]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return out


def call(entry, vals):
    """[status, [[kernel, label], ...]] of one call: what the hook saw"""
    lib = A._lib()
    with launches() as rec:
        if entry.startswith('conv_forward'):
            fn = getattr(lib, 'vdx_' + entry)
            fn.restype = C.c_int
            desc = ConvDesc(**vals['desc'])
            if entry == 'conv_forward':
                fn.argtypes = [C.c_int, C.POINTER(ConvDesc), C.c_void_p]
                rc = fn(vals['mode'], C.byref(desc), None)
            else:
                fn.argtypes = [C.c_int, C.POINTER(ConvDesc), C.c_int, C.c_int, C.c_void_p]
                rc = fn(vals['mode'], C.byref(desc), vals['w_rows'], vals['w_row0'], None)
        else:
            rc = A.call(entry, dict(A.base(entry), **vals))[0]
    return [rc, [list(r) for r in rec]]


def record():
    return {cid: call(entry, vals) for cid, entry, vals in all_cases()}


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print('{\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v)}' for k, v in record().items()) + '\n}')
