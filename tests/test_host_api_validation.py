"""CPU test of what the block-level entry points of libvdx accept and reject (tests/_api_cases.py: one base call per entry, one
perturbation at a time).  Without a device a refused call returns VDX_ERR_INVALID with its message and a call that passes validation
returns VDX_ERR_HIP from the launcher's first runtime call, having run nothing -- so status and text of every case are compared with
the recorded table tests/golden/api_validation.json.  A rule lost or loosened in vdx_api.cpp shows here as a wrong status."""
import json
import os

import pytest
import torch

import _api_cases as A

# with a device an accepted call would launch its kernel on the stand-in host pointers: never run these calls on a GPU
pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason='accepted calls would launch kernels on stand-in host pointers; the table is recorded without a device')

INVALID, HIP = -1, -2
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'api_validation.json')) as f:
    TABLE = json.load(f)


def test_the_table_covers_exactly_the_cases():
    assert list(TABLE) == [cid for cid, _, _ in A.all_cases()]
    assert all(status in (INVALID, HIP) and text for status, text in TABLE.values())
    for entry in A.SIGS:                                               # the base call of every entry passes validation
        assert TABLE[f'{entry}: base'][0] == HIP, entry


@pytest.mark.parametrize('entry', list(A.SIGS))
def test_status_and_message_of_every_case(entry):
    wrong = []
    for label, vals in A.cases(entry):
        got = list(A.call(entry, vals))
        if got != TABLE[f'{entry}: {label}']:
            wrong.append((label, got, TABLE[f'{entry}: {label}']))
    assert not wrong, wrong
