"""CPU test of the link between the kernel-level BACKWARD parity cases and the kernel forms the reverse pass of the networks routes to
(tests/_bwd_parity_routes.py), the twin of tests/test_host_parity_routes.py.

tests/golden/backward_routes.json pins the first launch of every block of model_backward for the training rows of the N, Y, dim-128, tiny
and long networks; tests/golden/bwd_parity_routes.json pins the same for every call of the kernel-level backward parity tests
(test_gpu_backward_forms, test_gpu_conv_backward, test_gpu_ss_backward, the cores of test_gpu_long_attention_backward), recorded through
the launch hook without a device, and the GPU tests assert their launch chains against it.  Here: the table is what the library routes
today, every case reaches the kernel its test says it tests, the form rule and the tail rule on literal labels, and the closure: every
form of the network rows, the launches behind the first included, is launched by at least one parity case -- a retuned patch rule or slot
threshold that moves the only case of a form to another kernel fails the closure for that form, by name."""
import pytest
import torch

import _bwd_parity_routes as BR

# with a device an accepted call would launch its kernel on the stand-in host pointers: never run these calls on a GPU
pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason='accepted calls would launch kernels on stand-in host pointers; the table is recorded without a device')

HIP = -2
TABLE = BR._golden('bwd_parity_routes.json')
CALLS = BR.parity_calls()
NET = BR.network_forms()
FWD = BR.forward_covered()

# Network forms without a kernel-level parity case: {form: a reason a reader can verify}.  None today.  No form that a row of the N or Y
# networks reaches may stand here, and the rest (dim-128, tiny, long) may hold at most a tenth of all network forms.
EXEMPT = {}
PROTECTED = ('N training', 'Y training')


def _closure(**kw):
    return BR.closure(TABLE, EXEMPT, net=NET, calls=CALLS, fwd=FWD, **kw)


def test_the_table_covers_exactly_the_cases():
    assert list(TABLE) == [c[0] for c in CALLS]
    for cid, (status, recs) in TABLE.items():                          # every parity case launches something
        assert status == HIP and recs, (cid, status, recs)
        assert all(kernel.endswith('_kernel') and label for kernel, label in recs), cid


@pytest.mark.parametrize('group', sorted({c[0].split(':')[0] for c in CALLS}))
def test_route_of_every_case(group):
    wrong = []
    for cid, entry, vals, _ in CALLS:
        if cid.split(':')[0] == group:
            got = BR.call(entry, vals)
            if got != TABLE[cid]:
                wrong.append((cid, got, TABLE[cid]))
    assert not wrong, wrong


def test_every_case_reaches_the_kernel_its_test_names():
    wrong = [(cid, want, TABLE[cid][1][0]) for cid, _, _, want in CALLS if want is not None and TABLE[cid][1][0][0] != want]
    assert not wrong, wrong


def test_form_rule():
    f = BR.form
    assert f('conv_wgrad16_kernel', '<NT 9, NG 2, PF 1, X16 1, DY16 1> conv3x3 512->512 40x8x8 +prologue +db patch 8x8 chunks28 det 1') == \
        ('conv_wgrad16_kernel', '<NT 9, NG 2, PF 1, X16 1, DY16 1>', 'conv3x3 +prologue +db patch 8x8 det 1')
    assert f('conv_wgrad_kernel', '<NT 8> conv4x4 16->16 8x16x16 s2 +db patch 4x8 chunks16 det 1') == ('conv_wgrad_kernel', '<NT 8>', 'conv4x4 s2 +db patch 4x8 det 1')
    assert f('conv_wgrad_kernel', '<NT 8> conv4x4 64->64 8x2x2 up +db patch 4x8 chunks8 det 0') == ('conv_wgrad_kernel', '<NT 8>', 'conv4x4 up +db patch 4x8 det 0')
    assert f('wgrad1x1_kernel', '<X16 0, DY16 0, NCO 4> conv1x1 64->768 rows32 split256 slots1 det 1') == ('wgrad1x1_kernel', '<X16 0, DY16 0, NCO 4>', 'conv1x1 split256 det 1')
    assert f('norm_bwd_reduce_kernel', '<2> C512 batch4 pix2560 nwg40 ln 1 ss 0 dss 0 dgp 1') == ('norm_bwd_reduce_kernel', '<2>', 'ln 1 ss 0 dss 0 dgp 1')
    assert f('attn_core_bwd_kernel', 'L4 nseq512 heads8') == ('attn_core_bwd_kernel', '', '')
    assert f('sla_bwd_a16_kernel', '<io16 1> N256 NF8 heads8') == ('sla_bwd_a16_kernel', '<io16 1>', '')
    assert f('time_mlp_bwd_kernel', 'dim16 time_dim64 cond0 B2') == ('time_mlp_bwd_kernel', '', 'cond0')
    assert f('final_conv_dx_kernel', 'D16 Cout1 npix32') == ('final_conv_dx_kernel', '', 'Cout1')
    assert f('resblock_ss_bwd_w_kernel', 'layers8 temb64 B2 kb8 det 1') == ('resblock_ss_bwd_w_kernel', '', 'kb8 det 1')
    assert f('init_conv_wgrad_kernel', 'conv7x7 1->16 8x16x16 slots8 det 1') == ('init_conv_wgrad_kernel', '', 'conv7x7 det 1')
    assert f('slot_sum_kernel', 'slots4 E36864 Cout64 split0') == ('slot_sum_kernel', '', 'Cout64 split0')
    # a data-gradient label is a forward label: the forward rule's answer
    lab = '<1, 128, 2, 8, 2> conv3x3 256->128 2x9x17 +res'
    assert f('conv_igemm_kernel', lab) == BR.PR.form('conv_igemm_kernel', lab) == ('conv_igemm_kernel', '<1, 128, 2, 8, 2>', 'conv3x3 +res')
    # patch, det and the prologue tell forms apart; chunks do not
    a = '<NT 9, NG 2, PF 1, X16 1, DY16 1> conv3x3 64->64 32x64x64 +prologue +db patch 8x16 chunks256 det 1'
    assert f('conv_wgrad16_kernel', a) == f('conv_wgrad16_kernel', a.replace('chunks256', 'chunks4').replace('32x64x64', '2x16x16'))
    for other in (a.replace('8x16', '8x8'), a.replace('det 1', 'det 0'), a.replace(' +prologue', ''), a.replace(' +db', ''), a.replace('X16 1', 'X16 0')):
        assert f('conv_wgrad16_kernel', a) != f('conv_wgrad16_kernel', other)


def test_tail_forms_on_the_chains_pinned_on_the_gpu():
    """the literal first labels of tests/test_gpu_backward_routes.py and the chains it pins behind them"""
    t = BR.tail_forms
    s, s16 = ('slot_sum_kernel', '', ''), ('slot_sum16_kernel', '', '')
    w = '<NT 9, NG 2, PF 1, X16 0, DY16 0> conv3x3 64->64 2x16x16 +db patch 8x16 chunks4 det %d'
    assert t('conv_wgrad16_kernel', w % 1) == [s, s] and t('conv_wgrad16_kernel', w % 0) == []
    assert t('conv_wgrad16_kernel', (w % 1).replace(' +db', '')) == [s]
    assert t('conv_wgrad16_kernel', (w % 1).replace('chunks4', 'chunks32')) == [s16, s16]
    assert t('conv_wgrad16_kernel', (w % 1).replace('chunks4', 'chunks31')) == [s, s]
    q = '<X16 0, DY16 0, NCO 4> conv1x1 64->768 rows32 split256 slots1 det 1'
    assert t('wgrad1x1_kernel', q, db=True) == [s, s] and t('wgrad1x1_kernel', q, db=False) == [s]
    assert t('wgrad1x1_kernel', q.replace('slots1', 'slots158'), db=True) == [s16, s16]
    for vpl, C in ((1, 64), (2, 512)):
        assert t('norm_bwd_reduce_kernel', f'<{vpl}> C{C} batch2 pix32 nwg1 ln 1 ss 0 dss 0 dgp 1') == [('norm_bwd_finalize_kernel', '', ''), ('norm_bwd_apply_kernel', f'<{vpl}>', '')]
    assert t('sla_bwd_a_kernel', 'N16 NF2 heads8') == [('sla_bwd_b_kernel', '', '')]
    for io in (0, 1):
        assert t('sla_bwd_a16_kernel', f'<io16 {io}> N16 NF2 heads8') == [('sla_bwd_b16_kernel', f'<io16 {io}>', '')]
    assert t('final_conv_dx_kernel', 'D16 Cout1 npix32', x16=0, det=True) == [('final_conv_dw_kernel', '<x16 0>', ''), s, s]
    assert t('final_conv_dx_kernel', 'D16 Cout1 npix32', x16=1, det=False) == [('final_conv_dw_kernel', '<x16 1>', '')]
    assert t('final_conv_dx_kernel', 'D64 Cout1 npix131072', x16=1, det=True) == [('final_conv_dw_kernel', '<x16 1>', ''), s16, s16]
    for n in (2, 8):
        assert t('resblock_ss_bwd_kernel', f'layers{n} temb64 B2', det=True) == [('resblock_ss_bwd_w_kernel', '', ''), s]
    assert t('resblock_ss_bwd_kernel', 'layers34 temb64 B3', det=True) == [('resblock_ss_bwd_w_kernel', '', ''), s16]
    assert t('resblock_ss_bwd_kernel', 'layers2 temb64 B2', det=False) == [('resblock_ss_bwd_w_kernel', '', '')]
    assert t('attn_long_bwd_stats_kernel', 'L256 nseq4 heads8') == [('attn_long_bwd_dkv_kernel', '', ''), ('attn_long_bwd_dq_kernel', '', '')]
    assert t('attn_core_bwd_kernel', 'L64 nseq2 heads8') == [] and t('slot_sum_kernel', 'slots31 E100 Cout0 split0') == []
    # slot_sum16's grid limit: 16 elements per workgroup, 65535 x 16 workgroups
    assert BR._slot_sum(32, 16 * 65535 * 16) == s16 and BR._slot_sum(32, 16 * 65535 * 16 + 1) == s


def test_closure():
    """Every form of the network rows, tails included, is launched by at least one backward parity case, is a data-gradient form the
    forward parity table reaches, or is exempt."""
    missing = _closure()
    have = BR.covered(TABLE, calls=CALLS)
    by_fwd = [f for f in NET if f not in have and f in FWD]
    print(f'{len(NET)} backward network forms ({len(NET) - len(_tails())} first-launch forms + {len(_tails())} behind them), '
          f'{len(have)} forms reached by {len(TABLE)} parity cases, {len(by_fwd)} data-gradient forms covered by the forward table only, {len(EXEMPT)} exempt')
    assert not missing, 'backward network forms no parity case reaches:\n' + '\n'.join(f'  {BR.form_str(f)}   (e.g. {NET[f][0]}, {len(NET[f])} blocks)' for f in missing)


def _tails():
    return {f for f in NET if not f[2] and f[0] in ('slot_sum_kernel', 'slot_sum16_kernel', 'norm_bwd_finalize_kernel', 'norm_bwd_apply_kernel', 'sla_bwd_b_kernel',
                                                     'sla_bwd_b16_kernel', 'final_conv_dw_kernel', 'resblock_ss_bwd_w_kernel', 'attn_long_bwd_dkv_kernel', 'attn_long_bwd_dq_kernel')}


def test_every_tail_kernel_enters_the_closure():
    assert {f[0] for f in _tails()} == {'slot_sum_kernel', 'slot_sum16_kernel', 'norm_bwd_finalize_kernel', 'norm_bwd_apply_kernel', 'sla_bwd_b_kernel', 'sla_bwd_b16_kernel',
                                        'final_conv_dw_kernel', 'resblock_ss_bwd_w_kernel', 'attn_long_bwd_dkv_kernel', 'attn_long_bwd_dq_kernel'}


def test_exemptions_meet_their_conditions():
    have = BR.covered(TABLE, calls=CALLS)
    for f, reason in EXEMPT.items():
        assert f in NET, f'{f}: not a network form'
        assert f not in have and f not in FWD, f'{f}: reached by {have.get(f)}: the exemption is stale'
        assert isinstance(reason, str) and len(reason) > 20, f
        assert not any(cid.startswith(PROTECTED) for cid in NET[f]), f'{f}: reached by an N or Y network row: {NET[f]}'
    assert len(EXEMPT) <= len(NET) // 10


def test_closure_is_sensitive_to_every_single_case():
    """For every form covered by exactly one parity case (and not by the forward table), dropping that case makes the closure fail for
    exactly the forms only that case launches -- and that form is among them."""
    have = BR.covered(TABLE, calls=CALLS)
    single = {f: ids[0] for f, ids in have.items() if len(ids) == 1 and f in NET and f not in FWD}
    assert single, 'no singly covered form: the tables changed shape, look at this test again'
    for f, cid in single.items():
        assert _closure(skip={cid}) == sorted(g for g, c in single.items() if c == cid), (f, cid)
        assert f in _closure(skip={cid})
    # and a table without any case of a kernel misses every form of that kernel, first launches and tails
    for gone in ('conv_wgrad16_kernel', 'norm_bwd_reduce_kernel'):
        skip = {c for c, v in TABLE.items() if v[1][0][0] == gone}
        missing = set(_closure(skip=skip))
        assert {f for f in NET if f[0] == gone} <= missing, gone
    skip = {c for c, v in TABLE.items() if v[1][0][0] == 'norm_bwd_reduce_kernel'}
    assert {f for f in NET if f[0] in ('norm_bwd_finalize_kernel', 'norm_bwd_apply_kernel')} <= set(_closure(skip=skip))
