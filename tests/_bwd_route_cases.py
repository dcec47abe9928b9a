"""Which kernel form a call of the reverse pass or the train step reaches (the host routing of launch_conv_wgrad, launch_norm_bwd, the
attention and SLA core backward, the small launchers of small_bwd.hip and optim.hip), shared by tests/test_host_bwd_routes.py and the
recorder at the bottom.  A plain module: nothing here is collected.  Built like tests/_route_cases.py: every launcher reports to the hook
before its first runtime call, pointers are the stand-in host array of tests/_api_cases.py, shapes are the workload's own.  Two groups:

  * the network: the reverse walk of model_backward (model_bwd.hip) for the training rows of _route_cases.NETWORKS and a dim-16 two-level
    32 x 32 model (256-token bottleneck: the long core), block by block with the flags model_bwd.hip fills;
  * the edges: one case on each side of every condition, and the sizes of the scratch queries ('size: ...', recorded as [value, []]).

    VDX_LIB=/path/to/libvdx.so python tests/_bwd_route_cases.py > table.json

records {case id: [status, [[kernel, label], ...]]}; tests/golden/backward_routes.json is that table."""
import ctypes as C
import json
import os
import sys

import _api_cases as A
import _route_cases as F

F32, BF16, F16 = F.F32, F.BF16, F.F16
BUF, HD, G = A.BUF, A.HD, F.G
WG_PART = 12 << 20                                          # WG_PART_FLOATS (vdx_internal.h): the slot scratch of one stream
_KIND = dict(A._KIND, f=C.c_float)

# ---- entry points tests/_api_cases.py does not hold ('name:f' a float) -------------------------------------------------------------------
_ADAM = 'params grads m v ema n:l lr:f b1:f b2:f eps:f step_count:l grad_scale:f do_ema:i ema_decay:f'
SIGS = {
    'final_conv_backward': 'x x_bf16:i d_out kernel dx dw db npix:l d:i cout:i scratch scratch_floats:z stream',
    'init_conv_backward_weights': 'x dy dw db batch:i cin:i frames:i h:i w:i cout:i k:i scratch scratch_floats:z stream',
    'time_mlp_backward': 'time w1 b1 w2 b2 dim:i cond_mask null_all:i cond_dim:i dtemb dw1 db1 dw2 db2 dnull batch:i stream',
    'resblock_scale_shift_backward': 'params grads temb layers nlayers:i lin dss dtemb temb_dim:i batch:i slots slots_cap:z stream',
    'slot_sum': 'part nslots:i slot_stride:z e:l cout:i split:i d0 d1 d2 stream',
    'colsum': 'x out rows:l c:i stream',
    'loss_grad': 'eps_hat noise d_eps batch:i channels:i fhw:l l2:i stream',
    'loss_grad_masked': 'eps_hat noise mask count d_eps batch:i channels:i fhw:l l2:i stream',
    'adam_ema_step': f'{_ADAM} stream',
    'adam_ema_step_clip': f'{_ADAM} sqnorm max_grad_norm:f norm_out stream',
    'grad_accumulate': 'acc g n:l stream',
    'grad_sqnorm': 'g n:l scratch out stream',
}
_SCALARS = dict(lr=1e-4, b1=0.9, b2=0.99, eps=1e-8, step_count=0, grad_scale=1.0, do_ema=1, ema_decay=0.995, max_grad_norm=1.0, l2=1, null_all=0, cond_dim=0,
                split=0, x_bf16=0, k=7, scratch_floats=WG_PART, slots_cap=WG_PART)
SIZES = {
    'norm_act_backward_scratch_floats': [C.c_int, C.c_int, C.c_long],
    'sla_backward_scratch_floats': [C.c_int, C.c_int],
    'attention_bias_backward_scratch_floats': [C.c_int, C.c_int],
    'grad_sqnorm_scratch_doubles': [],
    'wgrad_scratch_floats': [],
}


def own(entry, **vals):
    """an entry of SIGS above: pointers default to BUF, `stream` to 0, scalars to _SCALARS"""
    v = {}
    for tok in SIGS[entry].split():
        n, k = (tok.split(':') + ['p'])[:2]
        v[n] = vals[n] if n in vals else ((0 if n == 'stream' else BUF) if k == 'p' else _SCALARS[n])
    assert set(vals) <= set(v), (entry, set(vals) - set(v))
    return entry, v


# ---- one call = (entry, values), filled the way model_bwd.hip fills the launchers' arguments ---------------------------------------------
def wgrad(bf16, c0, cout, batch, frames, s, k=3, c1=0, stride=1, kind=0, pro=0, x16=0, dy16=0, db=1, split=0, w=None, scratch=WG_PART, groups=G):
    """model_bwd.hip: wgrad / wgrad1x1 / wgrad1x1_qkv.  scratch: floats of slot scratch, 0 = none (float atomics)"""
    d = dict(x0=BUF, x1=BUF if c1 else 0, c0=c0, c1=c1, x_bf16=x16, dy=BUF, cout=cout, dy_bf16=dy16, dw=BUF, split=split, db=BUF if db else 0,
             batch=batch, frames=frames, h=s, w=w or s, kind=kind, kh=k, kw=k, stride=stride, bf16_operands=bf16,
             scratch=BUF if scratch else 0, scratch_floats=scratch)
    if split:
        nb = cout // split
        d.update(dw1=BUF if nb > 1 else 0, dw2=BUF if nb > 2 else 0, db1=BUF if db and nb > 1 else 0, db2=BUF if db and nb > 2 else 0)
    if pro:
        d.update(in_stats=BUF, gamma=BUF, beta=BUF, groups=groups, scale_shift=BUF, scale_shift_stride=2 * c0)
    return 'conv_backward_weights_ex', d


def norm(c, batch, pix, ln=0, ss=0, dss=0, dgp=1, y16=0, dy16=0, r16=0, groups=G):
    """model_bwd.hip res_bwd: the tail (ln) and the prologue (ss, dss) of a ResnetBlock"""
    v = dict(A.base('norm_act_backward_ex'), y_bf16=y16, dy_bf16=dy16, r_bf16=r16 if ln else 0, groups=groups, ss=BUF if ss else 0, ss_stride=2 * c,
             dss=BUF if dss else 0, dgp=BUF if dgp else 0, c=c, batch=batch, pix=pix)
    if not ln:
        v.update(r=0, ln_gamma=0, dr=0, d_ln_gamma=0, d_ln_beta=0)
    return 'norm_act_backward_ex', v


def core(bf16, io16, batch, frames, h, w, temporal, heads=8, bias=0, focus=0):
    g = dict(batch=batch, frames=frames, h=h, w=w, heads=heads, temporal=temporal, bf16_operands=bf16, io_bf16=io16, dstride=3 * heads * 32)
    if focus:
        nb = dict(bias=BUF, dbias=BUF, scratch=BUF, scratch_floats=WG_PART) if bias else dict(bias=0, dbias=0, scratch=0, scratch_floats=0)
        return 'attention_core_backward_focus', dict(g, focus_n=batch, **nb)
    if bias:
        return 'attention_core_backward_bias', dict(g, scratch_floats=WG_PART)
    return 'attention_core_backward_io', g


def fused(x16, batch, frames, h, w):
    return 'temporal_attention_backward_fused_ex', dict(x_bf16=x16, batch=batch, frames=frames, h=h, w=w)


def sla_core(bf16, io16, nframes, npix, heads=8):
    return 'sla_core_backward_io', dict(nframes=nframes, npix=npix, heads=heads, bf16_operands=bf16, io_bf16=io16, dstride=3 * heads * 32)


def dgrad(mode, cdy, rows_total, row0, nrows, batch, frames, s, k, dy16, res):
    entry, v = F.conv(mode, cdy, nrows, batch, frames, s, k=k, x16=dy16, res=0 if res else None, rows=(rows_total, row0))
    v['desc'].update(bias=0)                                # model_bwd.hip dgrad: no bias
    return entry, v


# ---- the network: the reverse walk of model_backward ---------------------------------------------------------------------------------------
def network(dim, batch, frames, size, mode, act16, mults=(1, 2, 4, 8), channels=1, **_):
    """[(block name, entry, values)] in forward order of the blocks; act16 as in _route_cases.network (2: bf16 storage of the training forward)"""
    bf = 1 if mode == BF16 else 0
    a16 = 1 if act16 == 2 and bf else 0
    d16 = bf                                                # dL/d(y2), dL/d(y1) are bf16 tensors in bf16 mode
    out = []

    def add(name, call):
        out.append((name, *call))

    def res(name, c0, c1, cout, lvl):
        s = size >> lvl
        pix, cin = frames * s * s, c0 + c1
        add(f'{name}.tail', norm(cout, batch, pix, ln=1, y16=bf, dy16=d16, r16=a16))
        add(f'{name}.conv2.dw', wgrad(bf, cout, cout, batch, frames, s, pro=1, x16=bf, dy16=d16))
        if cin != cout:
            add(f'{name}.res_conv.dw', wgrad(bf, c0, cout, batch, frames, s, k=1, c1=c1, x16=a16))
        add(f'{name}.conv2.dx', dgrad(mode, cout, cout, 0, cout, batch, frames, s, 3, d16, 0))
        add(f'{name}.prologue', norm(cout, batch, pix, ss=1, dss=1, y16=bf, dy16=d16))
        add(f'{name}.conv1.dw', wgrad(bf, c0, cout, batch, frames, s, c1=c1, x16=a16, dy16=d16))
        for tag, row0, n in (('x0', 0, c0), ('x1', c0, c1)):
            if n:
                if cin != cout:
                    add(f'{name}.res_conv.d{tag}', dgrad(mode, cout, cin, row0, n, batch, frames, s, 1, 0, 0))
                add(f'{name}.conv1.d{tag}', dgrad(mode, cout, cin, row0, n, batch, frames, s, 3, d16, 1))

    def attn(name, c, lvl, temporal):
        s = size >> lvl
        L = frames if temporal else s * s
        io16 = 1 if bf and L <= 16 else 0
        if bf and temporal and c == 64 and frames <= 16:
            add(name, fused(a16, batch, frames, s, s))
            io16 = 1
        else:
            add(name, core(bf, io16, batch, frames, s, s, temporal))
        add(f'{name}.to_out.dw', wgrad(bf, HD, c, batch, frames, s, k=1, x16=io16))
        add(f'{name}.to_qkv.dw', wgrad(bf, c, 3 * HD, batch, frames, s, k=1, x16=a16, dy16=io16, split=HD))

    def level(name, c0, c1, cout, lvl, resample):
        s = size >> lvl
        res(f'{name}.0', c0, c1, cout, lvl)
        res(f'{name}.1', cout, 0, cout, lvl)
        add(f'{name}.2', sla_core(bf, bf, batch * frames, s * s))
        add(f'{name}.2.to_out.dw', wgrad(bf, HD, cout, batch, frames, s, k=1, x16=bf, db=0))
        add(f'{name}.2.to_qkv.dw', wgrad(bf, cout, 3 * HD, batch, frames, s, k=1, x16=a16, dy16=bf, split=HD, db=0))
        attn(f'{name}.3', cout, lvl, 1)
        if resample == 'down':
            add(f'{name}.4.dw', wgrad(bf, cout, cout, batch, frames, s, k=4, stride=2, x16=a16))
        if resample == 'up':
            add(f'{name}.4.dw', wgrad(bf, cout, cout, batch, frames, s, k=4, kind=1, x16=a16))

    dims = [dim] + [dim * m for m in mults]
    nl = len(mults)
    pix0 = batch * frames * size * size
    add('init_conv.dw', own('init_conv_backward_weights', batch=batch, cin=channels, frames=frames, h=size, w=size, cout=dim))
    add('time_mlp', own('time_mlp_backward', dim=dim, batch=batch, cond_mask=0, dnull=0))
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
    add('final_conv.1', own('final_conv_backward', x_bf16=a16, npix=pix0, d=dim, cout=channels))
    for n in (2, 4 * nl + 3):                               # one stage's two blocks, and every ResnetBlock of the network
        add(f'scale_shift {n} layers', own('resblock_scale_shift_backward', nlayers=n, temb_dim=4 * dim, batch=batch))
    return out


NETWORKS = [(n, kw) for n, kw in F.NETWORKS if 'training' in n or n.startswith('tiny')] + [
    ('long f32', dict(dim=16, batch=2, frames=2, size=32, mode=F32, act16=0, mults=(1, 2))),
    ('long bf16 storage', dict(dim=16, batch=2, frames=2, size=32, mode=BF16, act16=2, mults=(1, 2))),
]


# ---- the edges ---------------------------------------------------------------------------------------------------------------------------------
def edges():
    e = []

    def add(label, call):
        e.append((label, *call))

    # weight gradient (wgrad.hip): taps, the 8 x 16 patch, the wide GEMM tile, tensor formats, the prologue, resampling, slot capacity, split
    for bf in (0, 1):
        for k, kw in ((1, {}), (3, {}), (4, dict(stride=2)), (4, dict(kind=1))):
            add(f'wgrad operands {bf} taps {k * k}{" up" if kw.get("kind") else ""}', wgrad(bf, 64, 64, 4, 10, 32, k=k, **kw))
        for w in (15, 16):
            add(f'wgrad operands {bf} 3x3 W {w}', wgrad(bf, 64, 64, 4, 10, 16, w=w))
            add(f'wgrad operands {bf} 1x1 W {w}', wgrad(bf, 64, 64, 4, 10, 16, k=1, w=w))
        for cout in (192, 256, 320):
            add(f'wgrad operands {bf} 1x1 cout {cout}', wgrad(bf, 128, cout, 4, 10, 16, k=1))
        for x16 in (0, 1):
            for dy16 in (0, 1):
                add(f'wgrad operands {bf} 3x3 x16 {x16} dy16 {dy16}', wgrad(bf, 64, 64, 4, 10, 32, x16=x16, dy16=dy16))
                add(f'wgrad operands {bf} 1x1 x16 {x16} dy16 {dy16}', wgrad(bf, 64, 64, 4, 10, 32, k=1, x16=x16, dy16=dy16))
                add(f'wgrad operands {bf} 1x1 cout 256 x16 {x16} dy16 {dy16}', wgrad(bf, 64, 256, 4, 10, 32, k=1, x16=x16, dy16=dy16))
        add(f'wgrad operands {bf} prologue 3x3', wgrad(bf, 64, 64, 4, 10, 32, pro=1, x16=bf))
        add(f'wgrad operands {bf} prologue 1x1', ('conv_backward_weights', dict(A.base('conv_backward_weights'), kh=1, kw=1, bf16_operands=bf)))
        add(f'wgrad operands {bf} 1x1 stride 2', ('conv_backward_weights', dict(A.base('conv_backward_weights'), in_stats=0, kh=1, kw=1, stride=2, bf16_operands=bf)))
        add(f'wgrad operands {bf} concat', wgrad(bf, 64, 64, 4, 10, 32, c1=64))
        add(f'wgrad operands {bf} no db', wgrad(bf, 64, 64, 4, 10, 32, db=0))
        add(f'wgrad operands {bf} no scratch', wgrad(bf, 64, 64, 4, 10, 32, scratch=0))
        add(f'wgrad operands {bf} 1x1 no scratch', wgrad(bf, 64, 64, 4, 10, 32, k=1, scratch=0))
        for nb in (2, 3):
            add(f'wgrad operands {bf} split 256 blocks {nb}', wgrad(bf, 64, nb * 256, 4, 10, 32, k=1, split=256))
        add(f'wgrad operands {bf} split 64 blocks 3', wgrad(bf, 64, 192, 4, 10, 32, k=1, split=64))
    # slots of a launch: chunks x (taps x Cin x Cout + Cout) floats.  3x3 64 -> 64 on 40 frames of 32 x 32: 256 / 1 = 256 chunks in bf16
    # operands (8 x 16 patches), 1024 / 9 -> 256 / 1 in f32; the 1x1 GEMM form: 1024 / 1 slots of 64 x 64 + 64
    need3, need1 = 256 * (9 * 64 * 64 + 64), 640 * (64 * 64 + 64)
    for bf in (0, 1):
        for short in (0, 1):
            add(f'wgrad operands {bf} 3x3 scratch {"one short" if short else "exact"}', wgrad(bf, 64, 64, 4, 10, 32, scratch=need3 - short))
    for short in (0, 1):
        add(f'wgrad 1x1 GEMM scratch {"one short" if short else "exact"}', wgrad(1, 64, 64, 4, 10, 32, k=1, scratch=need1 - short))
    # norm backward (norm_bwd.hip): values per lane 1 / 2 / 4 by channel count, the branches, the reduce pass's workgroups per sample
    for c in (256, 260, 512, 516, 768, 1024):
        g = 4 if c % 8 else 8
        add(f'norm C {c} tail', norm(c, 4, 2560, ln=1, groups=g))
        add(f'norm C {c} prologue', norm(c, 4, 2560, ss=1, dss=1, groups=g))
        add(f'norm C {c} plain no dgp', norm(c, 4, 2560, dgp=0, groups=g))
    for pix in (1, 64, 40960, 1 << 20):
        add(f'norm C 64 pix {pix}', norm(64, 4, pix, ln=1))
        add(f'norm C 1024 pix {pix}', norm(1024, 4, pix, ss=1))
    add('norm ss without dss', norm(64, 4, 2560, ss=1))
    add('norm bf16 tensors', norm(64, 4, 2560, ln=1, y16=1, dy16=1, r16=1))
    for g in (1, 32):
        add(f'norm C 64 groups {g}', norm(64, 4, 2560, groups=g))
    add('norm C 1024 groups 1', norm(1024, 4, 2560, groups=1))
    add('norm C 4 groups 1', norm(4, 4, 2560, groups=1))
    # attention core backward (attn_bwd.hip, attn_long_bwd.hip)
    for L in (16, 17):
        for bf in (0, 1):
            add(f'core L {L} operands {bf}', core(bf, 0, 2, L, 4, 4, 1))
            add(f'core L {L} operands {bf} bias', core(bf, 0, 2, L, 4, 4, 1, bias=1))
            add(f'core L {L} operands {bf} focus', core(bf, 0, 2, L, 4, 4, 1, focus=1))
            add(f'core L {L} operands {bf} bias+focus', core(bf, 0, 2, L, 4, 4, 1, bias=1, focus=1))
        add(f'core L {L} io16', core(1, 1, 2, L, 4, 4, 1))
        add(f'core L {L} io16 bias', core(1, 1, 2, L, 4, 4, 1, bias=1))
        add(f'core L {L} io16 focus', core(1, 1, 2, L, 4, 4, 1, focus=1))
    for h, w in ((8, 8), (8, 16), (20, 32), (22, 32)):       # 64, 128, 640, 704 tokens
        add(f'core spatial L {h * w}', core(0, 0, 1, 2, h, w, 0))
        add(f'core spatial L {h * w} operands', core(1, 0, 1, 2, h, w, 0))
    add('core nseq 3 operands', core(1, 0, 1, 10, 1, 3, 1))
    for fr in (16, 17):
        for x16 in (0, 1):
            add(f'fused frames {fr} x16 {x16}', fused(x16, 4, fr, 8, 8))
    # SLA core backward: the three forms, one and two pixel tiles per frame
    for bf, io16 in ((0, 0), (1, 0), (1, 1)):
        for npix in (256, 257):
            add(f'sla core operands {bf} io16 {io16} N {npix}', sla_core(bf, io16, 40, npix))
    # the small launchers
    for n in (31, 32):
        add(f'slot_sum slots {n}', own('slot_sum', nslots=n, slot_stride=4096, e=4096, cout=64))
        add(f'slot_sum slots {n} split', own('slot_sum', nslots=n, slot_stride=768 * 64, e=768 * 64, cout=768, split=256))
    for over in (0, 1):                                     # slot_sum16's grid: 16 elements per workgroup
        add(f'slot_sum16 grid limit + {over}', own('slot_sum', nslots=32, slot_stride=16 * 65535 * 16 + over, e=16 * 65535 * 16 + over, cout=1))
    for rows, c in ((2560, 64), (1, 64), (1 << 20, 1024), (100, 2048)):
        add(f'colsum rows {rows} C {c}', own('colsum', rows=rows, c=c))
    for d, cout in ((256, 4), (260, 4), (256, 5), (64, 1)):
        add(f'final_conv_backward D {d} cout {cout}', own('final_conv_backward', npix=40960, d=d, cout=cout))
    add('final_conv_backward no scratch', own('final_conv_backward', npix=40960, d=64, cout=1, scratch=0, scratch_floats=0))
    for short in (0, 1):                                    # 512 workgroups x (D + 1) x Cout floats
        add(f'final_conv_backward scratch {"one short" if short else "exact"}', own('final_conv_backward', npix=40960, d=64, cout=1, scratch_floats=512 * 65 - short))
    for short in (0, 1):                                    # 16 tiles x 40 frames slots of 49 x 64 + 64 floats
        add(f'init_conv scratch {"one short" if short else "exact"}',
            own('init_conv_backward_weights', batch=4, cin=1, frames=10, h=64, w=64, cout=64, scratch_floats=640 * (49 * 64 + 64) - short))
    add('init_conv 3 channels k 3', own('init_conv_backward_weights', batch=4, cin=3, frames=10, h=64, w=64, cout=64, k=3))
    for cin in (24, 25):                                    # (cin x 22 x 22 + 256 x 17) x 4 bytes against 64 KB
        add(f'init_conv LDS limit cin {cin}', own('init_conv_backward_weights', batch=4, cin=cin, frames=10, h=64, w=64, cout=64))
    for b in (60, 61):                                      # dim 64: B (64 + 512 + 64) x 4 bytes against 150 KB
        add(f'time_mlp_backward dim 64 B {b}', own('time_mlp_backward', dim=64, batch=b, cond_mask=0, dnull=0))
    add('time_mlp_backward cond', own('time_mlp_backward', dim=64, batch=4, cond_dim=768))
    for n in (7, 8):
        add(f'scale_shift {n} layers', own('resblock_scale_shift_backward', nlayers=n, temb_dim=256, batch=4))
    for short in (0, 1):
        add(f'scale_shift scratch {"one short" if short else "exact"}', own('resblock_scale_shift_backward', nlayers=2, temb_dim=256, batch=4, slots_cap=2 * 4 * 256 - short))
    add('scale_shift no slots', own('resblock_scale_shift_backward', nlayers=2, temb_dim=256, batch=4, slots=0, slots_cap=0))
    # the train step (optim.hip)
    for l2 in (0, 1):
        add(f'loss_grad l2 {l2}', own('loss_grad', batch=4, channels=1, fhw=40960, l2=l2))
        add(f'loss_grad_masked l2 {l2}', own('loss_grad_masked', batch=4, channels=1, fhw=40960, l2=l2))
    for ema in (0, 1):
        add(f'adam_ema_step ema {ema}', own('adam_ema_step', n=1000003, do_ema=ema))
        add(f'adam_ema_step_clip ema {ema}', own('adam_ema_step_clip', n=1000003, do_ema=ema))
    add('grad_accumulate', own('grad_accumulate', n=1000003))
    add('grad_accumulate offset 4 bytes', own('grad_accumulate', acc=BUF + 4, n=1000003))
    add('grad_sqnorm', own('grad_sqnorm', n=1000003))
    return e


def sizes():
    s = [('norm_act_backward_scratch_floats', (c, 4, pix)) for c in (64, 260, 1024) for pix in (1, 64, 40960, 1 << 20)]
    s += [('sla_backward_scratch_floats', (40, 8)), ('attention_bias_backward_scratch_floats', (8, 10)), ('attention_bias_backward_scratch_floats', (8, 17)),
          ('grad_sqnorm_scratch_doubles', ()), ('wgrad_scratch_floats', ())]
    return [(f'{q}{list(args)}', 'size', dict(query=q, args=args)) for q, args in s]


def all_cases():
    """[(case id, entry, values)]"""
    out = [(f'{net}: {name}', entry, v) for net, kw in NETWORKS for name, entry, v in network(**kw)]
    out += [(f'edge: {label}', entry, v) for label, entry, v in edges()]
    out += [(f'size: {label}', entry, v) for label, entry, v in sizes()]
    ids = [c[0] for c in out]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return out


def call(entry, vals):
    """[status, [[kernel, label], ...]] of one call: what the hook saw ([value, []] of a size query)"""
    lib = A._lib()
    if entry == 'size':
        q = getattr(lib, 'vdx_' + vals['query'])
        q.restype, q.argtypes = C.c_size_t, SIZES[vals['query']]
        return [q(*vals['args']), []]
    if entry == 'conv_forward_rows':
        return F.call(entry, vals)
    with F.launches() as rec:
        if entry in SIGS:
            fn = getattr(lib, 'vdx_' + entry)
            toks = [(t.split(':') + ['p'])[:2] for t in SIGS[entry].split()]
            fn.restype, fn.argtypes = C.c_int, [_KIND[k] for _, k in toks]
            rc = fn(*[vals[n] for n, _ in toks])
        else:
            rc = A.call(entry, dict(A.base(entry), **vals))[0]
    return [rc, [list(r) for r in rec]]


def record():
    return {cid: call(entry, vals) for cid, entry, vals in all_cases()}


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print('{\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v)}' for k, v in record().items()) + '\n}')
