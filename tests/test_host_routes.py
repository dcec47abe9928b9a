"""CPU test of the forward kernel routing of libvdx (tests/_route_cases.py: every conv, attention and SLA block the network launches, at
workload shape, and each side of every condition of every route predicate).  Every launcher reports its launch to the hook before its
first runtime call, so without a device the first launch of a call's route is on record when the call returns VDX_ERR_HIP, having run
nothing -- status, kernel and label (the template instantiation and the operand shape) of every case are compared with the recorded table
tests/golden/kernel_routes.json.  A threshold, an order of predicates or an instantiation choice that moves shows here as another kernel
or another label.  Launches after the first of a chain (sla_out_w against sla_out8, the long attention's core, the out-projections)
stay pinned by the GPU tests that use tests/_launch_hook.py."""
import json
import os

import pytest
import torch

import _route_cases as R

# with a device an accepted call would launch its kernel on the stand-in host pointers: never run these calls on a GPU
pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason='accepted calls would launch kernels on stand-in host pointers; the table is recorded without a device')

INVALID, HIP = -1, -2
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'kernel_routes.json')) as f:
    TABLE = json.load(f)
CASES = R.all_cases()
# refused by launch_conv itself (a tensor of 4 GiB or more: 32-bit buffer offsets), which the entry point reports as VDX_ERR_HIP
REFUSED_BY_LAUNCHER = {'edge: conv 128 in frames 4096', 'edge: conv4x4_ws down 256 128x128'}


def test_the_table_covers_exactly_the_cases():
    assert list(TABLE) == [cid for cid, _, _ in CASES]
    for cid, (status, recs) in TABLE.items():                          # a launch on record, or a refusal
        assert status in (INVALID, HIP), cid
        assert (len(recs) >= 1 and status == HIP) or (not recs and (status == INVALID or cid in REFUSED_BY_LAUNCHER)), (cid, status, recs)
        assert all(kernel.endswith('_kernel') and label for kernel, label in recs), cid


def test_every_network_block_reports_its_launch():
    for cid, (status, recs) in TABLE.items():
        if not cid.startswith('edge: '):
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
