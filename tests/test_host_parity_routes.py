"""CPU test of the link between the kernel-level forward parity cases and the kernel forms the networks route to (tests/_parity_routes.py).

tests/golden/kernel_routes.json pins which kernel, instantiation and flags every block of the N, Y, dim-128 and tiny networks reaches;
tests/golden/parity_routes.json pins the same for every call of the kernel-level parity tests (test_gpu_conv, test_gpu_blocks,
test_gpu_forward_forms, test_gpu_f16_forms, test_gpu_attention_groups), recorded through the launch hook without a device, and the GPU
tests assert their first launch against it.  Here: the table is what the library routes today, every case reaches the kernel its test
says it tests, and every form of the networks is the first launch of at least one parity case (the closure) -- a retuned threshold that
moves the only case of a form to another kernel fails the closure for that form, by name."""
import pytest
import torch

import _parity_routes as PR
import _route_cases as R

# with a device an accepted call would launch its kernel on the stand-in host pointers: never run these calls on a GPU
pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason='accepted calls would launch kernels on stand-in host pointers; the table is recorded without a device')

HIP = -2
TABLE = PR._golden('parity_routes.json')
CALLS = PR.parity_calls()
NET = PR.network_forms()

# Network forms without a kernel-level parity case: {form: a reason a reader can verify}.  None today.  No form that a row of the N or Y
# networks reaches may stand here, and the rest (dim-128, tiny) may hold at most a tenth of all network forms.
EXEMPT = {}
PROTECTED = ('N sampling', 'N training', 'Y sampling', 'Y training')


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
            got = R.call(entry, vals)
            if got != TABLE[cid]:
                wrong.append((cid, got, TABLE[cid]))
    assert not wrong, wrong


def test_every_case_reaches_the_kernel_its_test_names():
    wrong = [(cid, want, TABLE[cid][1][0]) for cid, _, _, want in CALLS if want is not None and TABLE[cid][1][0][0] != want]
    assert not wrong, wrong


def test_form_rule():
    assert PR.form('conv3x3_ws_kernel', '<16, true> conv3x3 128->128 640x16x16 +prologue') == ('conv3x3_ws_kernel', '<16, true>', 'conv3x3 +prologue')
    assert PR.form('sla_ctx_kernel', '<2> C128 N16384 NF32 nchunk32 io16 0') == ('sla_ctx_kernel', '<2>', 'io16 0')
    assert PR.form('attention_w_kernel', '<fp8 0> C64 L10 nseq262144') == ('attention_w_kernel', '<fp8 0>', '')
    assert PR.form('sla_combine_kernel', 'NF2 nchunk1') == ('sla_combine_kernel', '', '')
    assert PR.form('conv_igemm_kernel', '<1, 64, 2, 8, 2> convT4x4 32->32 3x16x16') != PR.form('conv_igemm_kernel', '<1, 64, 2, 4, 2> conv4x4 32->32 3x32x32 s2')


def test_closure():
    """Every form of the networks is the first launch of at least one parity case, or exempt."""
    missing = PR.closure(TABLE, EXEMPT, net=NET)
    print(f'{len(NET)} network forms, {len(PR.covered(TABLE))} forms reached by {len(TABLE)} parity cases, {len(EXEMPT)} exempt')
    assert not missing, 'network forms no parity case reaches:\n' + '\n'.join(f'  {PR.form_str(f)}   (e.g. {NET[f][0]}, {len(NET[f])} blocks)' for f in missing)


def test_exemptions_meet_their_conditions():
    have = PR.covered(TABLE)
    for f, reason in EXEMPT.items():
        assert f in NET, f'{f}: not a network form'
        assert f not in have, f'{f}: reached by {have.get(f)}: the exemption is stale'
        assert isinstance(reason, str) and len(reason) > 20, f
        assert not any(cid.startswith(PROTECTED) for cid in NET[f]), f'{f}: reached by an N or Y network row: {NET[f]}'
    assert len(EXEMPT) <= len(NET) // 10


def test_closure_is_sensitive_to_every_single_case():
    """For every form covered by exactly one parity case, dropping that case makes the closure fail for exactly that form."""
    single = {f: ids[0] for f, ids in PR.covered(TABLE).items() if len(ids) == 1 and f in NET}
    assert single, 'no singly covered form: the tables changed shape, look at this test again'
    for f, cid in single.items():
        assert PR.closure(TABLE, EXEMPT, skip={cid}, net=NET) == [f], (f, cid)
    # and a table without any case of a kernel misses every form of that kernel
    no_ws = {c: v for c, v in TABLE.items() if v[1][0][0] != 'conv3x3_ws_kernel'}
    assert set(PR.closure(no_ws, EXEMPT, net=NET)) == {f for f in NET if f[0] == 'conv3x3_ws_kernel'}
