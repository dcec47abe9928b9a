"""Accept/reject cases of libvdx's block-level entry points (include/vdx.h), shared by tests/test_host_api_validation.py and the recorder
at the bottom.  A plain module: nothing here is collected.

Every entry has one base call at a tiny valid geometry (batch 1, 2 frames, 4 x 4, C 64, 8 heads, 8 groups) whose pointers are the address
of one small host array, and a list of single perturbations of it: every pointer nulled in turn, every scalar at the edges its rules name,
and the flag combinations the rules forbid.  Without a device a rejected call returns VDX_ERR_INVALID with its message and a call that
passes validation returns VDX_ERR_HIP from the launcher's first runtime call, so the whole accept/reject boundary shows on a CPU.

    VDX_LIB=/path/to/libvdx.so python tests/_api_cases.py > table.json

records {case id: [status, message without its " (file:line)"]} from any build of the library; tests/golden/api_validation.json is that
table of the library as committed."""
import ctypes as C
import json
import os
import re
import sys

_KIND = {'p': C.c_void_p, 'i': C.c_int, 'l': C.c_long, 'z': C.c_size_t}
_host = (C.c_double * 80)()                                # stands in for every buffer: no case here gets as far as reading one
BUF = (C.addressof(_host) + 15) & ~15                      # 16-byte aligned
HD = 8 * 32


class WgradDesc(C.Structure):
    _fields_ = [('x0', C.c_void_p), ('x1', C.c_void_p), ('c0', C.c_int), ('c1', C.c_int), ('dy', C.c_void_p), ('cout', C.c_int),
                ('dw', C.c_void_p), ('batch', C.c_int), ('frames', C.c_int), ('h', C.c_int), ('w', C.c_int),
                ('kind', C.c_int), ('kh', C.c_int), ('kw', C.c_int), ('stride', C.c_int),
                ('in_stats', C.c_void_p), ('gamma', C.c_void_p), ('beta', C.c_void_p), ('groups', C.c_int),
                ('scale_shift', C.c_void_p), ('scale_shift_stride', C.c_int), ('bf16_operands', C.c_int)]


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


# ---- the positional signatures of include/vdx.h: `name` is a pointer, `name:i|l|z` an int / long / size_t ------------------------------
_GEO = 'batch:i frames:i h:i w:i'
_ATT_W = 'wqkv bqkv wo bo'
_SLA_W = 'wq wk wv wo'
_GN = 'stats gn_gamma gn_beta groups:i ln_gamma ln_beta'
_TAIL_END = 'c:i batch:i pix:l stream'
_NB_OUT = 'd_gamma d_beta dss'
_NB_LN = 'ln_gamma dr d_ln_gamma d_ln_beta'
_CORE_IO = 'qkv d_o o dqkv dstride:i io_bf16:i'
_CORE_END = f'{_GEO} heads:i temporal:i bf16_operands:i stream'
_FUSED = 'dy wqkv bqkv wo_t o dqkv dx'
SIGS = {
    'attention_forward': f'mode:i x y {_ATT_W} {_GEO} c:i heads:i temporal:i stream',
    'attention_forward_ex': f'mode:i x y {_ATT_W} {_GEO} c:i heads:i temporal:i fp8:i stream',
    'attention_forward_bf16': f'x y {_ATT_W} {_GEO} c:i heads:i temporal:i fp8:i stream',
    'attention_forward_bias': f'mode:i x y io_bf16:i {_ATT_W} bias {_GEO} c:i heads:i temporal:i stream',
    'attention_forward_focus': f'mode:i x y io_bf16:i {_ATT_W} bias focus focus_n:i {_GEO} c:i heads:i temporal:i stream',
    'attention_present_forward': f'mode:i x y io_bf16:i {_ATT_W} {_GEO} c:i heads:i temporal:i stream',
    'attention_heads_forward': f'x y io_bf16:i {_ATT_W} scratch scratch_bytes:z {_GEO} c:i temporal:i fp8:i stream',
    'attention_long_forward': f'mode:i x y io_bf16:i {_ATT_W} scratch scratch_bytes:z {_GEO} c:i heads:i stream',
    'sla_forward': f'mode:i x y {_SLA_W} ws {_GEO} c:i heads:i stream',
    'sla_forward_bf16': f'x y {_SLA_W} ws {_GEO} c:i heads:i stream',
    'sla_heads_forward': f'x y io_bf16:i {_SLA_W} scratch scratch_bytes:z {_GEO} c:i stream',
    'resblock_tail': f'y2 r out {_GN} {_TAIL_END}',
    'resblock_tail_ex': f'y2 y2_bf16:i r r_bf16:i out out_bf16:i {_GN} {_TAIL_END}',
    'resblock_tail_rc_bf16': f'y2 x0 x1 c0:i c1:i rc_w rc_b out {_GN} {_TAIL_END}',
    'resblock_tail_rc_head_bf16': f'y2 x0 x1 c0:i c1:i rc_w rc_b {_GN} c:i fin_w fin_b fin_out batch:i pix:l stream',
    'norm_act_backward': f'dact y dy stats gamma beta groups:i ss ss_stride:i {_NB_OUT} r {_NB_LN} scratch {_TAIL_END}',
    'norm_act_backward_ex': f'dact y y_bf16:i dy dy_bf16:i stats gamma beta groups:i ss ss_stride:i {_NB_OUT} r r_bf16:i {_NB_LN} scratch dgp {_TAIL_END}',
    'attention_core_backward': f'qkv d_o o dq dk dv {_GEO} heads:i temporal:i stream',
    'attention_core_backward_ex': f'qkv d_o o dq dk dv {_CORE_END}',
    'attention_core_backward_io': f'{_CORE_IO} {_CORE_END}',
    'attention_core_backward_bias': f'{_CORE_IO} bias dbias scratch scratch_floats:z {_CORE_END}',
    'attention_core_backward_focus': f'{_CORE_IO} bias dbias scratch scratch_floats:z focus focus_n:i {_CORE_END}',
    'temporal_attention_backward_fused': f'x {_FUSED} {_GEO} stream',
    'temporal_attention_backward_fused_ex': f'x x_bf16:i {_FUSED} {_GEO} stream',
    'sla_core_backward': 'q k v d_out o dq dk dv scratch nframes:i npix:i heads:i stream',
    'sla_core_backward_ex': 'q k v d_out o dq dk dv scratch nframes:i npix:i heads:i bf16_operands:i stream',
    'sla_core_backward_io': 'q k v d_out o dqkv dstride:i io_bf16:i scratch nframes:i npix:i heads:i bf16_operands:i stream',
    'pack_conv_weights': 'mode:i kernel packed taps:i cin:i cout:i stream',
    'pack_conv_weights_t': 'mode:i kernel packed taps:i cin:i cout:i stream',
    'conv_backward_weights': WgradDesc,
    'conv_backward_weights_ex': WgradExDesc,
}

# ---- base calls: what every scalar is unless the entry says otherwise; pointers are BUF, `stream` is 0 -----------------------------------
_SCALARS = dict(mode=0, batch=1, frames=2, h=4, w=4, c=64, heads=8, temporal=0, fp8=0, io_bf16=0, focus_n=1, groups=8, pix=32,
                y2_bf16=0, r_bf16=0, out_bf16=0, y_bf16=0, dy_bf16=0, x_bf16=0, ss_stride=128, c0=64, c1=64, dstride=3 * HD, bf16_operands=0,
                scratch_floats=1 << 24, scratch_bytes=1 << 24, nframes=2, npix=16, taps=9, cin=64, cout=64,
                kind=0, kh=3, kw=3, stride=1, split=0, scale_shift_stride=128)
_BASE = {
    'attention_heads_forward': dict(c=256, scratch_bytes=('size', 'attention_heads_scratch_bytes', 'batch frames h w')),
    'attention_long_forward': dict(h=16, w=16, scratch_bytes=('size', 'attention_long_scratch_bytes', 'batch frames h w heads')),
    'sla_heads_forward': dict(c=256, scratch_bytes=('size', 'attention_heads_scratch_bytes', 'batch frames h w')),
    # the plain weight gradient: a 3x3 conv with the prologue, no concat; _ex: no prologue either (its forms exclude each other)
    'conv_backward_weights': dict(x1=0, c1=0),
    'conv_backward_weights_ex': dict(x1=0, c1=0, dw1=0, dw2=0, db1=0, db2=0, in_stats=0, gamma=0, beta=0, scale_shift=0, scratch_floats=1 << 20),
}
_BIAS_SCRATCH = ('size', 'attention_bias_backward_scratch_floats', 'heads L')

# ---- perturbations: (label, overrides), applied to an entry when every name exists in its signature --------------------------------------
_S64, _S65 = dict(h=8, w=8), dict(h=5, w=13)
_COMMON = [(f'{n}={v}', {n: v}) for n in ('batch', 'frames', 'h', 'w', 'nframes', 'npix', 'pix', 'heads', 'c', 'focus_n', 'cout', 'cin', 'taps') for v in (0, -1)]
_COMMON += [
    ('mode=3', dict(mode=3)), ('mode=2', dict(mode=2)), ('mode=1', dict(mode=1)),
    ('c=1024', dict(c=1024)), ('c=1028', dict(c=1028)), ('c=66', dict(c=66)), ('c=68', dict(c=68)), ('c=2', dict(c=2)),
    ('groups=0', dict(groups=0)), ('groups=33', dict(groups=33)), ('groups=7', dict(groups=7)), ('groups=32', dict(groups=32)),
    ('heads=4', dict(heads=4)), ('heads=1', dict(heads=1)),
    ('spatial L=64', _S64), ('spatial L=65', _S65),
    ('temporal L=2', dict(temporal=1)), ('temporal L=64', dict(temporal=1, frames=64)), ('temporal L=65', dict(temporal=1, frames=65)),
    ('frames=16', dict(frames=16)), ('frames=17', dict(frames=17)),
    ('fp8 f32', dict(fp8=1, mode=0)), ('fp8 bf16', dict(fp8=1, mode=1)), ('fp8', dict(fp8=1)),
    ('io_bf16 f32', dict(io_bf16=1, mode=0)), ('io_bf16 f16', dict(io_bf16=1, mode=2)), ('io_bf16 bf16', dict(io_bf16=1, mode=1)),
    ('io_bf16 bf16 c=68', dict(io_bf16=1, mode=1, c=68)), ('io_bf16 c=68', dict(io_bf16=1, c=68)), ('io_bf16', dict(io_bf16=1)),
    ('y2_bf16 c=68', dict(y2_bf16=1, c=68)), ('r_bf16 c=68', dict(r_bf16=1, c=68)), ('out_bf16 c=68', dict(out_bf16=1, c=68)),
    ('pix=8', dict(pix=8)), ('c1=-4', dict(c1=-4)), ('c1=0 x1=0', dict(c1=0, x1=0, c0=128)), ('c0=32 c1=96', dict(c0=32, c1=96)),
    ('c=128', dict(c=128)), ('c0=c1=32 c=32', dict(c0=32, c1=32, c=32)),
    # the tail and norm entries check the groups first: channel counts the 8 groups (or 2, 4) divide reach the channel rules themselves
    ('c=1032', dict(c=1032)), ('c=66 groups=2', dict(c=66, groups=2)), ('c=1024 ss_stride=2048', dict(c=1024, ss_stride=2048)), ('c=1024 ss=0', dict(c=1024, ss=0)),
    ('y2_bf16 c=68 groups=4', dict(y2_bf16=1, c=68, groups=4)), ('r_bf16 c=68 groups=4', dict(r_bf16=1, c=68, groups=4)),
    ('out_bf16 c=68 groups=4', dict(out_bf16=1, c=68, groups=4)), ('c=68 groups=4', dict(c=68, groups=4)), ('y2_bf16 c=72', dict(y2_bf16=1, c=72)),
    ('ss_stride=127', dict(ss_stride=127)), ('ss_stride=127 ss=0', dict(ss_stride=127, ss=0)),
    ('r=0 ln=0', dict(r=0, ln_gamma=0, dr=0, d_ln_gamma=0, d_ln_beta=0)), ('r=0 r_bf16', dict(r=0, r_bf16=1)),
    # core backward: above 64 tokens only the spatial multiples of 64 up to 640
    ('core L=128', dict(h=8, w=16)), ('core L=144', dict(h=12, w=12)), ('core L=640', dict(h=20, w=32)), ('core L=704', dict(h=22, w=32)),
    ('core temporal L=128', dict(temporal=1, frames=128)),
    ('dstride=760', dict(dstride=3 * HD - 8)), ('dstride=772', dict(dstride=3 * HD + 4)), ('dstride=776', dict(dstride=3 * HD + 8)),
    ('io_bf16 no operands', dict(io_bf16=1, bf16_operands=0)), ('io_bf16 operands', dict(io_bf16=1, bf16_operands=1)),
    ('io_bf16 operands L=17', dict(io_bf16=1, bf16_operands=1, h=1, w=17)), ('io_bf16 operands L=16', dict(io_bf16=1, bf16_operands=1, h=1, w=16)),
    ('operands', dict(bf16_operands=1)),
    ('bias=0 dbias=0', dict(bias=0, dbias=0)), ('bias=0 dbias=0 scratch=0', dict(bias=0, dbias=0, scratch=0, scratch_floats=0)),
    ('scratch_floats=0', dict(scratch_floats=0)),
    ('scratch_floats exact', dict(dbias=BUF, scratch_floats=_BIAS_SCRATCH)), ('scratch_floats short', dict(dbias=BUF, scratch_floats=_BIAS_SCRATCH + (-1,))),
    ('scratch_bytes=0', dict(scratch_bytes=0)),
]
_WGRAD = [(f'{n}={v}', {n: v}) for n in ('c0', 'cout') for v in (0, -4, 66)] + [
    ('c1=64 x1=0', dict(c1=64)), ('c1=64', dict(c1=64, x1=BUF)), ('c1=66', dict(c1=66, x1=BUF)), ('c1=-4 x1', dict(c1=-4, x1=BUF)), ('c1=-4 x1 no prologue', dict(c1=-4, x1=BUF, in_stats=0)), ('c1=64 no prologue', dict(c1=64, x1=BUF, in_stats=0)),
    ('kind=1', dict(kind=1)), ('kind=2', dict(kind=2)), ('kh=5', dict(kh=5, kw=5)), ('kh=3 kw=1', dict(kw=1)), ('kh=0', dict(kh=0, kw=0)),
    ('kh=2', dict(kh=2, kw=2)), ('stride=3', dict(stride=3)), ('stride=2', dict(stride=2)), ('4x4 stride=2', dict(kh=4, kw=4, stride=2)),
    ('4x4 stride=2 h=5', dict(kh=4, kw=4, stride=2, h=5)), ('1x1', dict(kh=1, kw=1)), ('bf16_operands', dict(bf16_operands=1)),
]
_PRO = dict(in_stats=BUF, gamma=BUF, beta=BUF, scale_shift=BUF)
_WGRAD_PRO = [('groups=0', dict(groups=0)), ('groups=33', dict(groups=33)), ('groups=7', dict(groups=7)), ('gamma=0', dict(gamma=0)), ('beta=0', dict(beta=0)),
              ('scale_shift=0', dict(scale_shift=0)), ('ss_stride=127', dict(scale_shift_stride=127)), ('ss_stride=127 ss=0', dict(scale_shift_stride=127, scale_shift=0)),
              ('c1=64', dict(c1=64, x1=BUF)), ('in_stats=0', dict(in_stats=0))]
_QKV = dict(kh=1, kw=1, cout=3 * HD, split=HD, dw1=BUF, dw2=BUF, db=BUF, db1=BUF, db2=BUF)
_WGRAD_EX = [('pro', _PRO)] + [(f'pro {k}', dict(_PRO, **v)) for k, v in _WGRAD_PRO] + [
    ('pro 1x1', dict(_PRO, kh=1, kw=1)), ('pro split', dict(_PRO, split=64)), ('pro kind=1', dict(_PRO, kind=1)),
    ('qkv', _QKV), ('qkv split=32', dict(_QKV, split=32, cout=96)), ('qkv split=64', dict(_QKV, split=64, cout=192)), ('qkv split=-64', dict(_QKV, split=-64)),
    ('qkv 4 blocks', dict(_QKV, split=64, cout=256)), ('qkv split=256 cout=640', dict(_QKV, cout=640)), ('qkv 3x3', dict(_QKV, kh=3, kw=3)),
    ('qkv dw1=0', dict(_QKV, dw1=0)), ('qkv dw2=0', dict(_QKV, dw2=0)), ('qkv db1=0', dict(_QKV, db1=0)), ('qkv db2=0', dict(_QKV, db2=0)),
    ('qkv db=0', dict(_QKV, db=0)), ('qkv db=db1=db2=0', dict(_QKV, db=0, db1=0, db2=0)), ('qkv 2 blocks dw2=0', dict(_QKV, cout=2 * HD, dw2=0, db2=0)),
    ('dw1 no split', dict(dw1=BUF)), ('db1 no split', dict(db=BUF, db1=BUF)), ('db', dict(db=BUF)),
    ('x_bf16', dict(x_bf16=1)), ('x_bf16 operands', dict(x_bf16=1, bf16_operands=1)), ('x_bf16 operands c0=68', dict(x_bf16=1, bf16_operands=1, c0=68)),
    ('dy_bf16 operands', dict(dy_bf16=1, bf16_operands=1)), ('dy_bf16 operands cout=68', dict(dy_bf16=1, bf16_operands=1, cout=68)), ('dy_bf16', dict(dy_bf16=1)),
    ('scratch=0', dict(scratch=0)), ('scratch_floats=0', dict(scratch_floats=0)), ('scratch=0 scratch_floats=0', dict(scratch=0, scratch_floats=0)),
]
# perturbations of a sequence length go to the entries whose rules name one
_ONLY = {'core ': 'attention_core_backward', 'frames=1': 'temporal_attention', 'spatial L': 'attention', 'temporal L': 'attention'}
_EXTRA = {
    'conv_backward_weights': _WGRAD + _WGRAD_PRO,
    'conv_backward_weights_ex': _WGRAD + _WGRAD_EX,
}


def _names(entry):
    sig = SIGS[entry]
    if isinstance(sig, str):
        return [(t.split(':') + ['p'])[:2] for t in sig.split()]
    kinds = {C.c_void_p: 'p', C.c_int: 'i', C.c_size_t: 'z'}
    return [[n, kinds[t]] for n, t in sig._fields_]


def base(entry):
    """name -> value of the entry's base call (size queries still symbolic: resolve())"""
    b = {n: (0 if n == 'stream' else BUF) if k == 'p' else _SCALARS[n] for n, k in _names(entry)}
    b.update(_BASE.get(entry, {}))
    return b


def cases(entry):
    """[(label, name -> value)]: the base call, every pointer nulled, every perturbation whose names the entry has"""
    b = base(entry)
    out = [('base', b)]
    out += [(f'{n}=0', dict(b, **{n: 0})) for n, k in _names(entry) if k == 'p' and b[n]]
    for label, over in _COMMON + _EXTRA.get(entry, []):
        only = [e for pre, e in _ONLY.items() if label.startswith(pre)]
        if all(n in b for n in over) and any(b[n] != v for n, v in over.items()) and all(entry.startswith(e) for e in only):
            out.append((label, dict(b, **over)))
    if isinstance(b.get('scratch_bytes'), tuple):              # one byte less than the entry's own query answers
        out.append(('scratch_bytes short', dict(b, scratch_bytes=b['scratch_bytes'] + (-1,))))
    uniq = {}
    for label, vals in out:                                    # the same perturbation may come from two lists; a label never names two
        assert uniq.setdefault(label, vals) == vals, (entry, label)
    return list(uniq.items())


def all_cases():
    return [(f'{entry}: {label}', entry, vals) for entry in SIGS for label, vals in cases(entry)]


_own = []


def _lib():
    """a CDLL object of our own on the package's library: the argtypes set here stay off the functions the package has bound"""
    if not _own:
        from video_diffusion_nnx_amd import _lib as L
        _own.append(C.CDLL(L.LIB_PATH))
    return _own[0]


def resolve(vals):
    """the symbolic sizes: ('size', query, argument names[, delta]) = what the library's query function answers for this call's geometry"""
    lib = _lib()
    out = dict(vals)
    for n, v in vals.items():
        if isinstance(v, tuple) and v[0] == 'size':
            g = dict(vals, L=vals['frames'] if vals.get('temporal') else vals['h'] * vals['w'])
            q = getattr(lib, 'vdx_' + v[1])
            q.restype, q.argtypes = C.c_size_t, [C.c_int] * len(v[2].split())
            out[n] = q(*[g[a] for a in v[2].split()]) + (v[3] if len(v) > 3 else 0)
    return out


_LOC = re.compile(r' \([^()]*:\d+\)$')


def call(entry, vals):
    """(status, message without the trailing " (file:line)") of one call"""
    lib = _lib()
    fn = getattr(lib, 'vdx_' + entry)
    fn.restype = C.c_int
    v = resolve(vals)
    sig = SIGS[entry]
    if isinstance(sig, str):
        names = _names(entry)
        fn.argtypes = [_KIND[k] for _, k in names]
        rc = fn(*[v[n] for n, _ in names])
    else:
        fn.argtypes = [C.POINTER(sig), C.c_void_p]
        rc = fn(C.byref(sig(**v)), None)
    lib.vdx_last_error.restype = C.c_char_p
    return rc, _LOC.sub('', lib.vdx_last_error().decode()) if rc else ''


def _call_forked(entry, vals):
    """call() in a child process: a build whose launcher divides by a zero geometry on the host is recorded, not fatal"""
    r, w = os.pipe()
    pid = os.fork()
    if pid == 0:
        try:
            os.write(w, json.dumps(call(entry, vals)).encode())
        finally:
            os._exit(0)
    os.close(w)
    data = os.read(r, 1 << 16)
    os.close(r)
    st = os.waitpid(pid, 0)[1]
    return json.loads(data) if data else ['signal %d' % (st & 127), '']


def record():
    _lib()
    return {cid: list(_call_forked(entry, vals)) for cid, entry, vals in all_cases()}


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print('{\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v)}' for k, v in record().items()) + '\n}')
