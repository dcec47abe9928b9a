"""CPU test of the backward kernel routing of libvdx (tests/_bwd_route_cases.py: the reverse walk of model_backward block by block at
workload shape, the train step's kernels, and each side of every condition of the launchers of wgrad.hip, norm_bwd.hip, attn_bwd.hip,
small_bwd.hip and optim.hip).  As in tests/test_host_routes.py every launcher reports its launch to the hook before its first runtime
call, so without a device the first launch of a call's chain is on record when the call returns VDX_ERR_HIP, having run nothing: status,
kernel and label of every case are compared with the recorded table tests/golden/backward_routes.json.  The label carries every planned
value that selects behaviour (template arguments, patch, chunks / slots, and `det 1|0`: the launch stores per-workgroup slots, or its
scratch did not fit and it adds with float atomics).  The launches after the first of a chain are pinned on the GPU by
tests/test_gpu_backward_routes.py."""
import json
import os

import pytest
import torch

import _bwd_route_cases as R

# with a device an accepted call would launch its kernel on the stand-in host pointers: never run these calls on a GPU
pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason='accepted calls would launch kernels on stand-in host pointers; the table is recorded without a device')

INVALID, HIP = -1, -2
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'backward_routes.json')) as f:
    TABLE = json.load(f)
CASES = R.all_cases()
# refused by the launcher itself, which the entry point reports as VDX_ERR_HIP: the 1x1 stride-2 weight gradient in bf16 operands (its
# staged window exceeds conv_wgrad16_kernel's registers; only the plain entry point lets it through)
REFUSED_BY_LAUNCHER = {'edge: wgrad operands 1 1x1 stride 2'}


def test_the_table_covers_exactly_the_cases():
    assert list(TABLE) == [cid for cid, _, _ in CASES]
    for cid, (status, recs) in TABLE.items():
        if cid.startswith('size: '):                                      # a scratch query: [value, []]
            assert status > 0 and not recs, cid
            continue
        assert status in (INVALID, HIP), cid                              # a launch on record, or a refusal
        assert (len(recs) >= 1 and status == HIP) or (not recs and (status == INVALID or cid in REFUSED_BY_LAUNCHER)), (cid, status, recs)
        assert all(kernel.endswith('_kernel') and label for kernel, label in recs), cid


def test_every_network_block_reports_its_launch():
    for cid, (status, recs) in TABLE.items():
        if not cid.startswith(('edge: ', 'size: ')):
            assert status == HIP and recs, cid


@pytest.mark.parametrize('group', sorted({cid.split(':')[0] for cid, _, _ in CASES}))
def test_route_of_every_case(group):
    wrong = []
    for cid, entry, vals in CASES:
        if cid.split(':')[0] == group:
            got = R.call(entry, vals)
            if got != TABLE[cid]:
                wrong.append((cid, got, TABLE[cid]))
    assert not wrong, wrong
