"""What the Python host layer launches, path by path (tests/_host_path_cases.py): every sampling chain, the single reverse steps and one
train step of every objective, against tests/golden/host_path_launches.json -- kernel names and shape strings recorded with the same
record() from the commit before the host layer was folded into one chain driver, one objective and one key tree.  A host refactor that
moves, adds or drops a launch, or captures where it replayed, fails here.

Rig: the 16-wide network of tests/test_gpu_sample_loops.py, 4 frames of 8 x 8, B = 2, T = 4, S = 2 for the sequence chains."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

import _host_path_cases as H

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'host_path_launches.json')) as f:
    GOLDEN = json.load(f)

# The third run of these two was no replay in the recording either, so nothing is asserted about it beyond the recorded launches:
# masked + guided is an eager loop (_masked_guided_steps), and the windows of extend() run under different keys
# (split_key(key, n_windows)) on one graph slot, so the first window meets the graph of the last one's seed
REPLAY_NOT_ASSERTED = ('inpaint/guided', 'extend/two_windows')


def test_the_golden_file_covers_the_cases():
    assert sorted(GOLDEN['cases']) == sorted(H.CASES)


@pytest.mark.parametrize('case', H.CASES)
def test_launches_are_the_recorded_ones(case):
    rec, _, pair = H.run(case)
    want = H.decode(GOLDEN, case)
    assert len(rec) == len(want), f'{case}: {len(rec)} launches, recorded {len(want)}'
    for i, (got, exp) in enumerate(zip(rec, want)):
        assert got == exp, f'{case}: launch {i} is {got}, recorded {exp}'
    if case in H.SAMPLING and case not in REPLAY_NOT_ASSERTED:
        again = H.forwards(H.replay_part(rec))
        assert again == 0, f'{case}: the second captured call ran {again} forwards, a replay runs none'
    if pair is not None:
        # p_losses on the same batch, t, noise and masks is the loss the train step returned (the bound of tests/test_gpu_train.py's
        # loss comparison)
        loss, value = pair
        print(f'{case}: train step {loss:.9f}, p_losses {value:.9f}')
        assert abs(loss - value) < 2e-5 * max(1.0, abs(value)), (case, loss, value)
