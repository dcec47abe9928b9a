"""Which kernel form every kernel-level BACKWARD parity case reaches, and whether every form the reverse pass of the networks routes to
has such a case: the second pair network_forms / parity_calls that tests/_parity_routes.py announces, over tests/_bwd_route_cases.py.
Shared by tests/test_host_bwd_parity_routes.py (CPU), the GPU parity files (which assert their launches against the table) and the
recorder at the bottom.  A plain module: nothing here is collected, nothing here touches the GPU.  form_str, closure's shape, cid and
the word splitting are those of tests/_parity_routes.py; only the size-word list is longer.

FORM RULE.  A word of a label is a size word -- and is taken out of a form -- only if no launcher picks a kernel, an instantiation or a
branch from it.  Size words: the forward list (AxBxC, a->b, C<n>, L<n>, N<n>, NF<n>, nseq<n>, nchunk<n>) and  batch<n> pix<n> npix<n>
nwg<n> rows<n> slots<n> chunks<n> dim<n> time_dim<n> temb<n> B<n> D<n> E<n> layers<n> heads<n>.  Kept: `patch 8x8|8x16|4x8`, `det 0|1`,
split<n>, +db, +prologue, concat, s2, up, `ln|ss|dss|dgp 0|1`, Cout<n>, cond<n>, kb<n> and every template string.  Read in wgrad.hip,
norm_bwd.hip, small_bwd.hip and attn_bwd.hip: chunks / slots / layers do choose between slot_sum_kernel and slot_sum16_kernel (32 and
up), but that is a launch BEHIND the first one and is restated in tail_forms() below from the very numbers; C chooses the <vpl>
instantiation of the norm backward, which the template string already shows; L above 64 chooses another kernel name.

TAILS.  Without a device a chain is seen up to its first launch only.  tail_forms(kernel, label) restates what follows a given first
launch -- kernel names and template strings only, the slot-sum kernel from slots / chunks / layers and `det` -- so the kernels behind a
first launch (norm_bwd_finalize / apply, sla_bwd_b / b16, final_conv_dw, resblock_ss_bwd_w, the attn_long passes, the two slot sums)
enter the closure as forms (kernel, template, '').  THIS RULE CAN ONLY BE CONFIRMED ON THE GPU: every bound GPU case compares the chain
it records behind its first launch with tail_forms of that first launch (bound() below), and tests/test_host_bwd_parity_routes.py
feeds it the literal first labels of the chains tests/test_gpu_backward_routes.py pins.  Three first labels do not carry what their
tail depends on (final_conv_dx_kernel: x16 and det; resblock_ss_bwd_kernel: det; wgrad1x1_kernel: whether bias sums follow, it has no
+db word); the caller hands these over (hints() from a call's values, keywords of bound() in a GPU test).

network_forms(): first forms and their tails of the network rows (neither 'edge: ' nor 'size: ') of tests/golden/backward_routes.json.
parity_calls(): every call of tests/test_gpu_backward_forms.py, test_gpu_conv_backward.py, test_gpu_ss_backward.py and the core tests
of test_gpu_long_attention_backward.py, each parametrisation and each inner loop, with the fields the wrappers of
video_diffusion_nnx_amd/ops.py fill; the tables are the tests' own objects (imported).  Left out: calls a test expects to be REJECTED
(they launch nothing), the optimizer / loss kernels of test_gpu_backward_forms.py (train step: no network row of backward_routes.json)
and the whole-network tests of the long-attention file (not kernel level).  A data-gradient form also counts as covered when
tests/golden/parity_routes.json reaches the identical form: same kernel, instantiation and flags, only the host packing differs, and
that packing is what test_dgrad_row_slice_with_res and test_conv_dgrad_wgrad_bias hold.

    VDX_LIB=/path/to/libvdx.so python tests/_bwd_parity_routes.py > tests/golden/bwd_parity_routes.json

records {case id: [status, [[kernel, label], ...]]} without a device."""
import contextlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _bwd_route_cases as B
import _parity_routes as PR
from _parity_routes import cid, form_str                     # noqa: F401  (re-exported)

BUF, WG_PART = B.BUF, B.WG_PART
TINY = 1024                                                  # the scratch 'too small for any launch' of the weight-gradient test
_BWD_SIZE_WORD = re.compile(r'^((batch|pix|npix|nwg|rows|slots|chunks|dim|time_dim|temb|B|D|E|layers|heads)\d+)$')


def form(kernel, label):
    """-> (kernel, '<...>' or '', flag words joined by one blank): PR.form with the backward's size words taken out as well"""
    tpl, rest = PR._LABEL.match(label).groups()
    return (kernel, tpl or '', ' '.join(w for w in rest.split() if not PR._SIZE_WORD.match(w) and not _BWD_SIZE_WORD.match(w)))


# ---- what follows a first launch -------------------------------------------------------------------------------------------------------
def _num(label, word):
    m = re.search(rf'(?:^|\s){word}(\d+)(?:\s|$)', label)
    return int(m.group(1)) if m else None


def _slot_sum(nslots, E):
    """launch_slot_sum (wgrad.hip)"""
    return ('slot_sum16_kernel' if nslots >= 32 and (E + 15) // 16 <= 65535 * 16 else 'slot_sum_kernel', '', '')


def tail_forms(kernel, label, x16=None, det=None, db=None):
    """[(kernel, template, '')] of the launches behind the first launch (kernel, label), in launch order.  x16 / det: what the labels
    of final_conv_dx_kernel and resblock_ss_bwd_kernel do not carry, db: whether a wgrad1x1_kernel call has bias sums (its label has no
    +db) -- hints()."""
    tpl = PR._LABEL.match(label).group(1) or ''
    if kernel in ('conv_wgrad_kernel', 'conv_wgrad16_kernel', 'wgrad1x1_kernel', 'init_conv_wgrad_kernel'):
        if ' det 1' not in label:
            return []
        k, cin, cout = map(int, re.search(r'conv(\d+)x\d+ (\d+)->(\d+)', label).groups())
        n = _num(label, 'slots') if _num(label, 'slots') is not None else _num(label, 'chunks')
        bias = '+db' in label.split() or kernel == 'init_conv_wgrad_kernel'                      # (the stem conv always has its bias sums)
        if kernel == 'wgrad1x1_kernel':
            bias = bool(db)
        return [_slot_sum(n, k * k * cin * cout)] + ([_slot_sum(n, cout)] if bias else [])
    if kernel == 'norm_bwd_reduce_kernel':
        return [('norm_bwd_finalize_kernel', '', ''), ('norm_bwd_apply_kernel', tpl, '')]
    if kernel == 'sla_bwd_a_kernel':
        return [('sla_bwd_b_kernel', '', '')]
    if kernel == 'sla_bwd_a16_kernel':
        return [('sla_bwd_b16_kernel', tpl, '')]
    if kernel == 'attn_long_bwd_stats_kernel':
        return [('attn_long_bwd_dkv_kernel', '', ''), ('attn_long_bwd_dq_kernel', '', '')]
    if kernel == 'final_conv_dx_kernel':
        D, cout, npix = _num(label, 'D'), _num(label, 'Cout'), _num(label, 'npix')
        n = max(1, min(-(-npix // (256 // D)), 512))
        return [('final_conv_dw_kernel', f'<x16 {int(x16)}>', '')] + ([_slot_sum(n, D * cout), _slot_sum(n, cout)] if det else [])
    if kernel == 'resblock_ss_bwd_kernel':
        return [('resblock_ss_bwd_w_kernel', '', '')] + ([_slot_sum(_num(label, 'layers'), _num(label, 'B') * _num(label, 'temb'))] if det else [])
    if kernel == 'colsum_kernel':
        return [_slot_sum(_num(label, 'slots'), _num(label, 'C'))] if ' det 1' in label else []
    return []


def hints(entry, vals):
    """the keyword arguments of tail_forms that a call's first label does not carry"""
    if entry == 'final_conv_backward':
        n = max(1, min(-(-vals['npix'] // (256 // vals['d'])), 512))
        return dict(x16=vals['x_bf16'], det=bool(vals['scratch']) and n * (vals['d'] + 1) * vals['cout'] <= vals['scratch_floats'])
    if entry == 'resblock_scale_shift_backward':
        return dict(det=bool(vals['slots']) and vals['nlayers'] * vals['batch'] * vals['temb_dim'] <= vals['slots_cap'])
    if entry == 'conv_backward_weights_ex':
        return dict(db=bool(vals.get('db')))
    return {}


def forms_of(entry, vals, recs):
    """first form + tail forms of one recorded call"""
    return [form(*recs[0])] + tail_forms(*recs[0], **hints(entry, vals))


def _golden(name):
    return PR._golden(name)


def network_forms(table=None):
    """{form: [case ids]} of the network rows of backward_routes.json, tails included"""
    table = table or _golden('backward_routes.json')
    out = {}
    for c, entry, vals in B.all_cases():
        if not c.startswith(('edge: ', 'size: ')):
            for f in forms_of(entry, vals, table[c][1]):
                out.setdefault(f, []).append(c)
    return out


# ---- one call, as the wrappers of ops.py fill it ---------------------------------------------------------------------------------------
def _scr(label):
    return {'atomics': 0, 'slots': WG_PART, 'slots too small': TINY}[label]


def wgrad_ex(bf, case, x16, dy16, scratch, bias):
    """ops.conv_backward_weights_ex over a row (B, F, H, W, c0, c1, cout, k, stride, kind, prologue, split) of WG_CASES"""
    Bn, Fr, H, W, c0, c1, cout, k, stride, kind, pro, split = case
    return B.wgrad(bf, c0, cout, Bn, Fr, H, k=k, c1=c1, stride=stride, kind=kind, pro=int(pro), x16=int(x16), dy16=int(dy16), db=int(bias), split=split, w=W,
                   scratch=scratch)


def wgrad_plain(bf, shape, cout, *, c1=0, k=3, stride=1, kind=0, pro=False):
    """ops.conv_backward_weights: no scratch, no bias sums, fp32 tensors; groups = 8 whether used or not"""
    Bn, Fr, H, W, c0 = shape
    p = BUF if pro else 0
    return 'conv_backward_weights', dict(x0=BUF, x1=BUF if c1 else 0, c0=c0, c1=c1, dy=BUF, cout=cout, dw=BUF, batch=Bn, frames=Fr, h=H, w=W, kind=kind, kh=k, kw=k,
                                         stride=stride, in_stats=p, gamma=p, beta=p, groups=8, scale_shift=p, scale_shift_stride=2 * c0 if pro else 0, bf16_operands=int(bf))


def norm_ex(C, Bn, shape, use_ss, tail, det, dy16, y16=1):
    """ops.norm_act_backward_ex: dss with the scale / shift, ss_stride 0 without it, dgp only when deterministic, r_bf16 from r's dtype"""
    entry, v = B.norm(C, Bn, shape[0] * shape[1] * shape[2], ln=int(tail), ss=int(use_ss), dss=int(use_ss), dgp=int(det), y16=y16, dy16=int(dy16), r16=y16)
    v.update(ss_stride=2 * C if use_ss else 0)
    return entry, v


def norm_plain(C, Bn, shape, use_ss, tail):
    """ops.norm_act_backward (fp32 tensors, float atomics)"""
    t, s = (BUF if tail else 0), (BUF if use_ss else 0)
    return 'norm_act_backward', dict(groups=8, ss=s, ss_stride=2 * C if use_ss else 0, dss=s, r=t, ln_gamma=t, dr=t, d_ln_gamma=t, d_ln_beta=t, c=C, batch=Bn,
                                     pix=shape[0] * shape[1] * shape[2])


def core_io(case, io16, pad=0, bf=1):
    Bn, Fr, H, W, heads, temporal = case
    entry, v = B.core(bf, int(io16), Bn, Fr, H, W, int(temporal), heads=heads)
    v.update(dstride=3 * heads * 32 + pad)
    return entry, v


def core_ex(case, bf):
    Bn, Fr, H, W, heads, temporal = case
    return 'attention_core_backward_ex', dict(batch=Bn, frames=Fr, h=H, w=W, heads=heads, temporal=int(temporal), bf16_operands=int(bf))


def sla_io(NF, N, io16, pad=0):
    entry, v = B.sla_core(1, int(io16), NF, N)
    v.update(dstride=768 + pad)
    return entry, v


def dgrad_rows(mode, dy16, k, shape, cin, cout, row0, nrows):
    """ops.conv_dgrad_rows: dy [B, F, H, W, cout] through rows [row0, row0 + nrows) of the transposed packing; fp32 residual, no bias"""
    Bn, Fr, H, W = shape
    entry, v = B.F.conv(PR.MODE[mode], cout, nrows, Bn, Fr, H, k=k, x16=int(dy16), res=0, w=W, rows=(cin, row0))
    v['desc'].update(bias=0)
    return entry, v


def dgrad_fwd(mode, case):
    """test_conv_dgrad_wgrad_bias: the data gradient as a forward conv over dy with the transposed packing, Down <-> Up swapped"""
    Bn, Fr, H, W, Cin, Cout, k, stride, kind = case
    Ho, Wo = (2 * H, 2 * W) if kind else (H // stride, W // stride)
    kw = dict(k=4, stride=2) if kind == 1 else dict(k=4, kind=1) if stride == 2 else dict(k=k)
    entry, v = PR.conv(mode, (Bn, Fr, Ho, Wo, Cout), Cin, **kw)
    v['desc'].update(bias=0)
    return entry, v


def final_conv(D, cout, npix, x16, scratch):
    return B.own('final_conv_backward', x_bf16=int(x16), npix=npix, d=D, cout=cout, scratch=BUF if scratch else 0, scratch_floats=scratch)


def ss_bwd(nlayers, temb_dim, Bn, label):
    """ops.resblock_scale_shift_backward: the network's slots, none, or slots reported one float short"""
    need = nlayers * Bn * temb_dim
    cap = {'slots': WG_PART, 'atomics': 0, 'short': need - 1}[label]
    return B.own('resblock_scale_shift_backward', nlayers=nlayers, temb_dim=temb_dim, batch=Bn, slots=BUF if label != 'atomics' else 0, slots_cap=cap)


# ---- the parity cases -------------------------------------------------------------------------------------------------------------------
WG16, WG32, WG1X1 = 'conv_wgrad16_kernel', 'conv_wgrad_kernel', 'wgrad1x1_kernel'
MODES16 = [(False, False), (True, False), (False, True), (True, True)]
SCRATCH = ('atomics', 'slots', 'slots too small')


def _backward_forms_cases():
    import test_gpu_backward_forms as T
    out = []
    for name, case in T.WG_CASES.items():
        k, kind, pro = case[7], case[9], case[10]
        want = WG1X1 if k == 1 and not kind else WG16
        for x16, dy16 in MODES16:
            for label in SCRATCH:
                out.append((cid('wg16', name, x16, dy16, label), *wgrad_ex(1, case, x16, dy16, _scr(label), True), want))
    for name in T.WG32_NAMES:
        for bias in (True, False):
            for label in (SCRATCH[:2] if bias else SCRATCH[1:2]):
                out.append((cid('wg32', name, bias, label), *wgrad_ex(0, T.WG_CASES[name], False, False, _scr(label), bias), WG32))
    for nslots in T.SLOT_COUNTS:
        for E, cout, split in T.SLOT_SHAPES:
            nb = cout // split if split else 1
            out.append((cid('slot_sum', nslots, E, cout, split), *B.own('slot_sum', nslots=nslots, slot_stride=E + 5, e=E, cout=cout, split=split,
                                                                         d1=BUF if nb > 1 else 0, d2=BUF if nb > 2 else 0),
                        'slot_sum16_kernel' if nslots >= 32 else 'slot_sum_kernel'))
    for case in T.NORM_CASES:
        C, Bn, shape, use_ss, tail = case
        for tag, det, dy16 in (('dgp 0', False, True), ('dgp 1', True, True), ('fp32 dy', True, False)):
            out.append((cid('norm16', case, tag), *norm_ex(C, Bn, shape, use_ss, tail, det, dy16), 'norm_bwd_reduce_kernel'))
    for case in T.ATTN_CASES:
        Bn, Fr, H, W, heads, temporal = case
        L = Fr if temporal else H * W
        for io16 in (True, False):
            if io16 and L > 16:
                continue                                     # rejected by the entry point: the test expects VdxError, nothing launches
            for pad in (0, T.PAD):
                out.append((cid('core io', case, io16, pad), *core_io(case, io16, pad), 'attn_core_bwd16_kernel' if L <= 16 else 'attn_core_bwd_kernel'))
    for case in T.FUSED_CASES:
        for x16 in (True, False):
            out.append((cid('fused ex', case, x16), *B.fused(int(x16), *case), 'attn_bwd16x_kernel'))
    for NF, H, W in T.SLA_CASES:
        for io16 in (True, False):
            for pad in (0, T.PAD):
                out.append((cid('sla io', (NF, H, W), io16, pad), *sla_io(NF, H * W, io16, pad), 'sla_bwd_a16_kernel'))
    for case in T.DGRAD_CASES:
        k, Bn, Fr, H, W, cin, cout = case
        for mode, dy16 in T.DGRAD_MODES:
            for row0 in (0, cin // 2):
                out.append((cid('dgrad rows', case, mode, dy16, row0), *dgrad_rows(mode, dy16, k, (Bn, Fr, H, W), cin, cout, row0, cin // 2),
                            'conv_igemm_kernel' if mode == 'f16' else None))
    for D, cout, lead in T.FINAL_CASES:
        npix = lead[0] * lead[1] * lead[2] * lead[3]
        for x16 in (False, True):
            for label in SCRATCH[:2]:
                out.append((cid('final_conv', D, cout, lead, x16, label), *final_conv(D, cout, npix, x16, _scr(label)), 'final_conv_dx_kernel'))
    for Cin, D, k in T.INIT_CASES:
        for label in SCRATCH[:2]:
            s = _scr(label)
            out.append((cid('init_conv', Cin, D, k, label), *B.own('init_conv_backward_weights', batch=2, cin=Cin, frames=3, h=20, w=12, cout=D, k=k,
                                                                    scratch=BUF if s else 0, scratch_floats=s), 'init_conv_wgrad_kernel'))
    for dim, cond_dim in T.TIME_MLP_CASES:
        out.append((cid('time_mlp', dim, cond_dim), *B.own('time_mlp_backward', dim=dim, batch=5, cond_dim=cond_dim, cond_mask=BUF if cond_dim else 0,
                                                            dnull=BUF if cond_dim else 0), 'time_mlp_bwd_kernel'))
    return out


def _conv_backward_cases():
    import test_gpu_conv_backward as T
    out = []
    for mode in ('f32', 'bf16'):
        for case in T.CASES:
            Bn, Fr, H, W, Cin, Cout, k, stride, kind = case
            Ho, Wo = (2 * H, 2 * W) if kind else (H // stride, W // stride)
            out.append((cid('cb dgrad', mode, case), *dgrad_fwd(mode, case), None))
            for bf in ((0, 1) if mode == 'bf16' else (0,)):
                out.append((cid('cb wgrad', mode, case, bf), *wgrad_plain(bf, (Bn, Fr, H, W, Cin), Cout, k=k, stride=stride, kind=kind), None))
            out.append((cid('cb colsum', mode, case), *B.own('colsum', rows=Bn * Fr * Ho * Wo, c=Cout), 'colsum_kernel'))
    sh = (2, 2, 8, 8, 32)
    for bf in (0, 1):
        out.append((cid('cb concat', bf), *wgrad_plain(bf, sh, 32, c1=16), WG16 if bf else WG32))
        out.append((cid('cb prologue', bf), *wgrad_plain(bf, sh, 32, pro=True), WG16 if bf else WG32))
    out.append((cid('cb concat 1x1 256'), *wgrad_plain(1, sh, 256, c1=16, k=1), WG1X1))
    for case in T.NORM_CASES:
        out.append((cid('cb norm', case), *norm_plain(*case), 'norm_bwd_reduce_kernel'))
    for case in T.ATTN_CASES:
        for bf in (0, 1):
            out.append((cid('cb core', case, bf), *core_ex(case, bf), None))
    for case in T.FUSED_CASES:
        out.append((cid('cb fused', case), 'temporal_attention_backward_fused', dict(zip(('batch', 'frames', 'h', 'w'), case)), 'attn_bwd16x_kernel'))
    for NF, H, W in T.SLA_CASES:
        for bf in (0, 1):
            out.append((cid('cb sla', (NF, H, W), bf), 'sla_core_backward_ex', dict(nframes=NF, npix=H * W, heads=8, bf16_operands=bf),
                        'sla_bwd_a16_kernel' if bf else 'sla_bwd_a_kernel'))
    return out


def ss_calls(name):
    """the (layers of the call, label) pairs test_resblock_scale_shift_backward issues for one case of _ss_backward_cases.CASES"""
    import _ss_backward_cases as SC
    nl = len(SC.CASES[name]['widths'])
    seen = [(nl, 'slots'), (nl, 'atomics'), (nl, 'short')]
    for which in SC.stages(nl):
        if (len(which), 'slots') not in seen:
            seen.append((len(which), 'slots'))
    return seen


def _ss_cases():
    import _ss_backward_cases as SC
    out = []
    for name, c in SC.CASES.items():
        for n, label in ss_calls(name):
            out.append((cid('ss', name, n, label), *ss_bwd(n, c['temb_dim'], c['B'], label), 'resblock_ss_bwd_kernel'))
    # test_chain_norm_backward_to_time_mlp_backward: C 64, B 3, pixels (2, 8, 8), two layers over temb 64, the stem at dim 16
    out.append((cid('ss chain', 'norm'), *norm_ex(64, 3, (2, 8, 8), True, False, True, True), 'norm_bwd_reduce_kernel'))
    out.append((cid('ss chain', 'ss'), *ss_bwd(2, 64, 3, 'slots'), 'resblock_ss_bwd_kernel'))
    out.append((cid('ss chain', 'time_mlp'), *B.own('time_mlp_backward', dim=16, batch=3, cond_dim=0, cond_mask=0, dnull=0), 'time_mlp_bwd_kernel'))
    return out


def _long_cases():
    import test_gpu_long_attention_backward as T
    out = []
    for case in T.CASES:
        c6 = (*case, False)
        out.append((cid('long', case, 'separate'), *core_ex(c6, 0), T.NEW[0]))
        for pad in (0, T.PAD):
            out.append((cid('long', case, 'io', pad), *core_io(c6, False, pad), T.NEW[0]))
    out.append((cid('long', '64 tokens'), *core_ex((1, 2, 8, 8, 8, False), 0), 'attn_core_bwd_kernel'))
    return out


def parity_calls():
    """[(case id, entry, values, expected kernel or None)]"""
    out = _backward_forms_cases() + _conv_backward_cases() + _ss_cases() + _long_cases()
    ids = [c[0] for c in out]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return out


def call(entry, vals):
    """[status, [[kernel, label], ...]] of one call (a data gradient is a call of the forward conv entries)"""
    return B.F.call(entry, vals) if entry.startswith('conv_forward') else B.call(entry, vals)


def record():
    return {c: call(entry, vals) for c, entry, vals, _ in parity_calls()}


# ---- closure ---------------------------------------------------------------------------------------------------------------------------
def covered(table, skip=(), calls=None):
    """{form: [case ids]} of the launches (first + tails) of the backward parity table"""
    out = {}
    for c, entry, vals, _ in (calls or parity_calls()):
        recs = table.get(c, (0, []))[1]
        if recs and c not in skip:
            for f in forms_of(entry, vals, recs):
                out.setdefault(f, []).append(c)
    return out


FORWARD_CONV = ('conv_igemm_kernel', 'conv3x3_ws_kernel', 'conv4x4_ws_kernel', 'conv1x1_pw_kernel', 'conv64p_kernel', 'conv64q_kernel', 'conv64r_kernel',
                'conv64d_kernel', 'resample32_kernel')


def forward_covered(fwd_table=None):
    """the data-gradient forms tests/golden/parity_routes.json reaches (forward conv kernels only)"""
    return {form(*recs[0]) for status, recs in (fwd_table or _golden('parity_routes.json')).values() if recs and recs[0][0] in FORWARD_CONV}


def closure(table, exempt=(), skip=(), net=None, calls=None, fwd=None):
    """The network forms (tails included) that no backward parity case of `table` (less `skip`) launches, that the forward parity table
    does not reach either (data-gradient forms), and that are not exempt, sorted"""
    have = covered(table, skip, calls)
    fwd = forward_covered() if fwd is None else fwd
    return sorted(f for f in (net if net is not None else network_forms()) if f not in have and f not in fwd and f not in exempt)


# ---- binding on the GPU ----------------------------------------------------------------------------------------------------------------
_TABLE = None


def golden_row(case_id):
    global _TABLE
    if _TABLE is None:
        _TABLE = _golden('bwd_parity_routes.json')
    return _TABLE[case_id]


def assert_chain(case_id, rec, calls=1, **hint):
    """rec: the launches recorded around `calls` identical calls of the case: each call's first launch is the golden row's, and what
    follows it is tail_forms of that first launch"""
    assert rec, f'{case_id}: no launch on record'
    want = golden_row(case_id)[1][0]
    assert len(rec) % calls == 0, f'{case_id}: {len(rec)} launches in {calls} calls: {rec}'
    n = len(rec) // calls
    for i in range(calls):
        one = rec[i * n:(i + 1) * n]
        assert list(one[0]) == want, f'{case_id}: the device route {list(one[0])} differs from the route recorded on the CPU {want}'
        got = [(k, PR._LABEL.match(s).group(1) or '', '') for k, s in one[1:]]
        assert got == tail_forms(*one[0], **hint), f'{case_id}: behind {one[0]} the device launched {one[1:]}, tail_forms says {tail_forms(*one[0], **hint)}'


@contextlib.contextmanager
def bound(case_id, calls=1, **hint):
    """with bound(id): the call under test -- records its launches and asserts the whole chain against the golden row and tail_forms"""
    from _launch_hook import launches
    with launches() as rec:
        yield rec
    assert_chain(case_id, rec, calls, **hint)


if __name__ == '__main__':
    print('{\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v)}' for k, v in record().items()) + '\n}')
