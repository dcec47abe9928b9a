"""Which kernel form every kernel-level forward parity case reaches, and whether every form the network routes to has such a case: shared
by tests/test_host_parity_routes.py (CPU), the GPU parity files (which assert their first launch against the table) and the recorder at
the bottom.  A plain module: nothing here is collected, nothing here touches the GPU.

A FORM is (kernel, template string, flag words): the kernel name the launcher reports, the "<...>" at the head of its label, and the
label's remaining words with the size words taken out.  Size words are  AxBxC  (frames x height x width),  a->b  (channels),  C<n>,  L<n>,
N<n>,  NF<n>,  nseq<n>  and  nchunk<n>;  everything else ("conv3x3", "+prologue", "+res", "concat", "s2", "io16 0", ...) is a flag
word.  Two launches of one form run the same instantiation of the same kernel with the same optional paths; they differ in sizes only.

network_forms() are the forms of the non-edge rows of tests/golden/kernel_routes.json (tests/_route_cases.py: every conv, attention and
SLA block of the N, Y, dim-128 and tiny networks).  parity_calls() restates every call of the kernel-level forward parity tests in the
vocabulary of tests/_route_cases.py, at the test's own shape and flags and with the fields the wrappers of video_diffusion_nnx_amd/ops.py
fill; the tables are the tests' own objects (imported).  A case id is cid(table, *key); the GPU test builds the same id from the same key
and asserts the first launch it records against the row of tests/golden/parity_routes.json (bound / assert_first below).  The few
tests that state their one shape inline (the concat / prologue pair, the 64-channel persistent convs, the fp16 subnormal conv) are restated
here by hand; the label in their row carries channels and frame sizes, so a test whose shape moves away from its row fails its binding.

    VDX_LIB=/path/to/libvdx.so python tests/_parity_routes.py > tests/golden/parity_routes.json

records {case id: [status, [[kernel, label], ...]]} without a device, like the other two tables.  The backward (backward_routes.json)
has its own pair network_forms / parity_calls over tests/_bwd_route_cases.py in tests/_bwd_parity_routes.py, which reuses the word
splitting, cid and form_str of this file."""
import contextlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _route_cases as R

F32, BF16, F16 = R.F32, R.BF16, R.F16
MODE = {'f32': F32, 'bf16': BF16, 'f16': F16}

_SIZE_WORD = re.compile(r'^(\d+x\d+x\d+|\d+->\d+|C\d+|L\d+|N\d+|NF\d+|nseq\d+|nchunk\d+)$')
_LABEL = re.compile(r'^(<[^>]*>)?\s*(.*)$')


def form(kernel, label):
    """-> (kernel, '<...>' or '', flag words joined by one blank)"""
    tpl, rest = _LABEL.match(label).groups()
    return (kernel, tpl or '', ' '.join(w for w in rest.split() if not _SIZE_WORD.match(w)))


def form_str(f):
    return ' '.join(p for p in f if p)


def _golden(name):
    with open(os.path.join(HERE, 'golden', name)) as f:
        return json.load(f)


def network_forms(table=None):
    """{form: [case ids]} of the network rows (not 'edge: ') of kernel_routes.json; a row's form is that of its first launch"""
    out = {}
    for cid, (status, recs) in (table or _golden('kernel_routes.json')).items():
        if not cid.startswith('edge: '):
            out.setdefault(form(*recs[0]), []).append(cid)
    return out


def cid(table, *key):
    return f'{table}: ' + ' '.join(str(k) for k in key)


# ---- one call, as the wrappers of ops.py fill it ---------------------------------------------------------------------------------------
def conv(mode, shape, cout, *, c1=0, k=3, stride=1, kind=0, x16=False, y16=False, pro=False, use_ss=True, stats=False, res=None):
    """ops.conv_forward: shape = x0's [B, F, H, W, C0]; x_bf16 from the dtype, groups = out_groups = 8 whether used or not, scale_shift
    and its stride absent when use_ss is false, out_stats only when the test passes it, res: None or the residual's bf16-ness."""
    B, Fr, H, W, c0 = shape
    entry, v = R.conv(MODE[mode], c0, cout, B, Fr, H, k=k, c1=c1, stride=stride, kind=kind, pro=int(pro), stats=int(stats), x16=int(x16), y16=int(y16),
                      res=None if res is None else int(res), w=W)
    v['desc'].update(groups=8, out_groups=8)
    if pro and not use_ss:
        v['desc'].update(scale_shift=0, scale_shift_stride=0)
    return entry, v


def attention_ex(mode, shape, heads, temporal, fp8=False):
    """ops.attention_forward / vdx_attention_forward_ex on fp32 tensors"""
    return 'attention_forward_ex', dict(R._geo(*shape), mode=MODE[mode], heads=heads, temporal=int(temporal), fp8=int(fp8))


def attention_bf16(shape, temporal=True, fp8=False):
    return 'attention_forward_bf16', dict(R._geo(*shape), heads=8, temporal=int(temporal), fp8=int(fp8))


def attention_heads(shape, temporal, io16, fp8):
    return 'attention_heads_forward', dict(R._geo(*shape), io_bf16=int(io16), temporal=int(temporal), fp8=int(fp8),
                                           scratch_bytes=('size', 'attention_heads_scratch_bytes', 'batch frames h w'))


def attention_long(mode, shape, io16):
    return 'attention_long_forward', dict(R._geo(*shape, 128), mode=MODE[mode], io_bf16=int(io16), heads=8,
                                          scratch_bytes=('size', 'attention_long_scratch_bytes', 'batch frames h w heads'))


def sla(mode, shape, io16=False):
    if io16:
        return 'sla_forward_bf16', dict(R._geo(*shape), heads=8)
    return 'sla_forward', dict(R._geo(*shape), mode=MODE[mode], heads=8)


def sla_heads(shape, io16):
    return 'sla_heads_forward', dict(R._geo(*shape), io_bf16=int(io16), scratch_bytes=('size', 'attention_heads_scratch_bytes', 'batch frames h w'))


# ---- the parity cases -----------------------------------------------------------------------------------------------------------------
IGEMM, WS3, WS4, PW = 'conv_igemm_kernel', 'conv3x3_ws_kernel', 'conv4x4_ws_kernel', 'conv1x1_pw_kernel'


def _chain_cases(table, rows):
    """test_gpu_conv._conv_chain: plain (concat) conv with statistics, then the prologue conv Cout -> Cout, with and without scale / shift"""
    out = []
    for mode, t16, B, Fr, H, W, C0, C1, Cout in rows:
        case = (B, Fr, H, W, C0, C1, Cout)
        out.append((cid(table, mode, t16, case, 'plain'), *conv(mode, (B, Fr, H, W, C0), Cout, c1=C1, x16=t16, y16=t16, stats=True), IGEMM))
        for ss in (True, False):
            out.append((cid(table, mode, t16, case, 'prologue', ss), *conv(mode, (B, Fr, H, W, Cout), Cout, x16=t16, y16=t16, pro=True, use_ss=ss, stats=True), IGEMM))
    return out


def _form_cases(table, rows):
    """test_gpu_conv._conv_form: one conv"""
    out = []
    for mode, t16, B, Fr, H, W, C0, C1, Cout, k, stride, kind, res in rows:
        case = (B, Fr, H, W, C0, C1, Cout, k, stride, kind, res)
        out.append((cid(table, mode, t16, case), *conv(mode, (B, Fr, H, W, C0), Cout, c1=C1, k=k, stride=stride, kind=kind, x16=t16, y16=t16,
                                                        res=None if res is None else res == 'bf16'), IGEMM))
    return out


def _conv_cases():
    import test_gpu_conv as T
    out = []
    for mode in ('f32', 'bf16'):
        for case in T.CASES:
            B, Fr, H, W, Cin, Cout, k, stride, kind = case
            out.append((cid('conv', mode, case), *conv(mode, (B, Fr, H, W, Cin), Cout, k=k, stride=stride, kind=kind, stats=Cout % 8 == 0), IGEMM))
        out.append((cid('conv concat', mode), *conv(mode, (2, 4, 8, 8, 32), 32, c1=16, stats=True), IGEMM))
        for ss in (True, False):
            out.append((cid('conv prologue', mode, ss), *conv(mode, (2, 4, 8, 8, 32), 32, pro=True, use_ss=ss), IGEMM))
    for act, B, Fr in T.C64_CASES:
        sh = (B, Fr, 64, 64, 64)
        out.append((cid('c64', act, B, Fr, 'plain'), *conv('bf16', sh, 64, x16=act, y16=act, stats=True), 'conv64r_kernel' if act else 'conv64p_kernel'))
        out.append((cid('c64', act, B, Fr, 'prologue'), *conv('bf16', sh, 64, x16=act, y16=act, pro=True), 'conv64q_kernel' if act else 'conv64p_kernel'))
    for c, B, Fr, S in T.C32_CASES:
        sh = (B, Fr, S, S, c)
        out.append((cid('c32', *sh, 'plain'), *conv('bf16', sh, c, x16=True, y16=True, stats=True), 'conv64p_kernel'))
        for ss in (True, False):
            out.append((cid('c32', *sh, 'prologue', ss), *conv('bf16', sh, c, x16=True, y16=True, pro=True, use_ss=ss), 'conv64p_kernel'))
    for concat in (True, False):
        sh = (2, 32, 64, 64, 64 if concat else 128)
        out.append((cid('c128->64', concat), *conv('bf16', sh, 64, c1=64 if concat else 0, x16=True, y16=True, stats=True), 'conv64q_kernel'))
    for c, B, Fr, S in T.CONCAT32_CASES:
        out.append((cid('concat->32', c, B, Fr, S), *conv('bf16', (B, Fr, S, S, c), 32, c1=c, x16=True, y16=True, stats=True), 'conv64q_kernel'))
    for case in T.WS_CASES:
        B, Fr, S, C0, C1, Cout = case
        (k1, k2), Cout2 = T.WS_KERNELS.get(case, (WS3, WS3)), T.WS_SECOND.get(case, 128)
        for y16 in (True, False):
            out.append((cid('ws', case, y16, 'plain'), *conv('bf16', (B, Fr, S, S, C0), Cout, c1=C1, x16=True, y16=y16, stats=True), k1))
        for ss in (True, False):
            out.append((cid('ws', case, 'prologue', ss), *conv('bf16', (B, Fr, S, S, Cout), Cout2, x16=True, y16=True, pro=True, use_ss=ss, stats=True), k2))
    for rb in (False, True):
        out.append((cid('c64 res', rb), *conv('bf16', (4, 16, 64, 64, 64), 64, x16=True, res=rb), IGEMM if rb else 'conv64d_kernel'))
    out.append((cid('c64 res', 'plain'), *conv('bf16', (4, 16, 64, 64, 64), 64, x16=True), 'conv64r_kernel'))
    for case in T.PW_CASES:
        B, Fr, S, C0, C1, Cout, res = case
        out.append((cid('pw', case), *conv('bf16', (B, Fr, S, S, C0), Cout, c1=C1, k=1, x16=True, y16=True, res=True if res else None), PW))
    for case in T.PW32_CASES:
        B, Fr, S, Cin, Cout, res = case
        out.append((cid('pw32', case), *conv('bf16', (B, Fr, S, S, Cin), Cout, k=1, x16=True, res=False if res else None), T.PW32_KERNELS.get(case, PW)))
    for case in T.WS4_CASES:
        kind, B, Fr, S, C, Cout = case
        for y16 in (True, False):
            kw = dict(kind=1, k=4) if kind else dict(k=4, stride=2)
            out.append((cid('ws4', case, y16), *conv('bf16', (B, Fr, S, S, C), Cout, x16=True, y16=y16, **kw), T.ws4_kernel(case, y16)))
    out += _chain_cases('generic chain', T.GENERIC_CHAINS) + _form_cases('generic form', T.GENERIC_FORMS)
    return out


def _blocks_cases():
    import test_gpu_blocks as T
    out = []
    for mode in ('f32', 'bf16'):
        for case in T.ATTN_CASES:
            out.append((cid('blocks attention', mode, case), *attention_ex(mode, case[:5], case[5], case[6]), None))
        for case in T.SLA_CASES:
            out.append((cid('blocks sla', mode, case), *sla(mode, case), None))
    for case in T.ATTN16_CASES:
        out.append((cid('blocks attention16', case), *attention_bf16(case), T.ATTN16_KERNEL.get(case)))
        if case in T.ATTN16_FP8:
            out.append((cid('blocks attention16', case, 'fp8'), *attention_bf16(case, fp8=True), T.ATTN16_KERNEL.get(case)))
    for case in T.FP8_CASES:
        for fp8 in (False, True):
            out.append((cid('blocks fp8', case, fp8), *attention_ex('bf16', case[:5], case[5], case[6], fp8), None))
    for case in T.SLA16_CASES:
        out.append((cid('blocks sla16', case), *sla('bf16', case, True), 'sla_ctx8_kernel'))
    return out


def _forward_forms_cases():
    import _forward_cases as FC
    import test_gpu_forward_forms as T
    out = []
    for shape, temporal, io16, fp8 in T._HEADS:
        out.append((cid('heads', shape, temporal, io16, fp8), *attention_heads(shape, temporal, io16, fp8), 'attention_head_kernel'))
    for shape in FC.ATTN_LONG:
        for mode, io16 in T.LONG_MODES:
            out.append((cid('long', shape, mode, io16), *attention_long(mode, shape, io16), None))       # (first launch: the q|k|v projection)
    for shape in FC.SLA_HEADS:
        for io16 in (False, True):
            out.append((cid('sla heads', shape, io16), *sla_heads(shape, io16), 'sla_head_kernel'))
    return out


def _f16_cases():
    import test_gpu_f16_forms as T
    out = []
    for shape, temporal, iso, kernel, parts in T.ATTN_F16:
        out.append((cid('attention f16', shape, temporal, iso), *attention_ex('f16', shape, 8, temporal), kernel))
    for shape, iso, nchunk in T.SLA_F16:
        out.append((cid('sla f16', shape, iso), *sla('f16', shape), 'sla_ctx_kernel'))
    for case in T.FWD_CASES:
        B, Fr, H, W, Cin, Cout, k, stride, kind = case
        out.append((cid('conv f16', case), *conv('f16', (B, Fr, H, W, Cin), Cout, k=k, stride=stride, kind=kind, stats=Cout % 8 == 0), IGEMM))
    out.append((cid('conv f16 concat'), *conv('f16', (2, 4, 8, 8, 32), 32, c1=16, stats=True), IGEMM))
    for ss in (True, False):
        out.append((cid('conv f16 prologue', ss), *conv('f16', (2, 4, 8, 8, 32), 32, pro=True, use_ss=ss), IGEMM))
    for shape, cin, cout in T.PW_F16:
        out.append((cid('pw f16', shape, cin, cout), *conv('f16', (*shape, cin), cout, k=1, res=False), IGEMM))
    out.append((cid('conv f16 subnormal'), *conv('f16', (1, 4, 16, 16, 32), 64), IGEMM))
    out += _chain_cases('f16 chain', T.F16_CHAINS) + _form_cases('f16 form', T.F16_FORMS)
    return out


def _groups_cases():
    import test_gpu_attention_groups as T
    out = []
    for shape, fp8, iso, kernel, parts in T.ATTN16:
        out.append((cid('attention16', shape, fp8, iso), *attention_bf16(shape, fp8=fp8), kernel))
    for shape, temporal, kernel, parts in T.ATTN16_GENERIC:
        out.append((cid('attention16 generic', shape, temporal), *attention_bf16(shape, temporal), kernel))
    for shape, temporal, iso, expect in T.ATTN32:
        for mode in ('f32', 'bf16', 'f16'):
            out.append((cid('attention32', shape, temporal, iso, mode), *attention_ex(mode, shape, 8, temporal), expect[mode][0]))
    for shape, iso, expect in T.SLA16:
        out.append((cid('sla16', shape, iso), *sla('bf16', shape, True), expect[0][0]))
    for shape, iso, nchunk in T.SLA32:
        for mode in ('f32', 'bf16', 'f16'):
            out.append((cid('sla32', shape, iso, mode), *sla(mode, shape), T._sla32(mode, shape[4], shape[2] * shape[3], shape[0] * shape[1], nchunk)[0][0]))
    return out


def parity_calls():
    """[(case id, entry, values, expected kernel or None)]"""
    out = _conv_cases() + _blocks_cases() + _forward_forms_cases() + _f16_cases() + _groups_cases()
    ids = [c[0] for c in out]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return out


def record():
    return {c: R.call(entry, vals) for c, entry, vals, _ in parity_calls()}


# ---- closure ---------------------------------------------------------------------------------------------------------------------------
def covered(table, skip=()):
    """{form: [case ids]} of the first launches of a parity table"""
    out = {}
    for c, (status, recs) in table.items():
        if recs and c not in skip:
            out.setdefault(form(*recs[0]), []).append(c)
    return out


def closure(table, exempt=(), skip=(), net=None):
    """The network forms that are neither the first launch of a parity case of `table` (less the cases of `skip`) nor exempt, sorted"""
    have = covered(table, skip)
    return sorted(f for f in (net if net is not None else network_forms()) if f not in have and f not in exempt)


# ---- binding on the GPU ----------------------------------------------------------------------------------------------------------------
_TABLE = None


def golden_row(case_id):
    global _TABLE
    if _TABLE is None:
        _TABLE = _golden('parity_routes.json')
    return _TABLE[case_id]


def assert_first(case_id, rec):
    """rec: what _launch_hook.launches() recorded around the call under test; its first launch is the golden row's"""
    assert rec, f'{case_id}: no launch on record'
    want = golden_row(case_id)[1][0]
    assert list(rec[0]) == want, f'{case_id}: the device route {list(rec[0])} differs from the route recorded on the CPU {want}'


@contextlib.contextmanager
def bound(case_id):
    """with bound(id): the call under test -- records its launches and asserts the first against the golden row"""
    from _launch_hook import launches
    with launches() as rec:
        yield rec
    assert_first(case_id, rec)


if __name__ == '__main__':
    print('{\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v)}' for k, v in record().items()) + '\n}')
