"""fm_cascade_host -- the host half of the one-call association cascade (csrc/assoc.hip cascade_run) -- against the
oracle's restatement of the reference's stage logic (np_oracle.matching_cost / gate_cost / lsa / assignment_matches /
greedy_match: utils/matching.py, tracker.py:198-248, pinned by the reference-generated goldens) on seeded pairwise
terms.  CPU only: the routine touches no device.  Sizes cross the table-growth boundaries of Numba's set (16, 32, 64
entries), costs carry exact ties, gated pairs, empty groups and label mismatches."""
import numpy as np
import pytest

from cascade_cases import make_case, reference_cascade, run_host


@pytest.mark.parametrize('quantise', [False, True])
def test_cascade_host_equals_reference_logic(quantise):
    rng = np.random.default_rng(11 + quantise)
    sizes = [(1, 1), (3, 7), (7, 3), (8, 9), (9, 8), (16, 17), (17, 16), (20, 50), (50, 20), (33, 31), (50, 50), (64, 70),
             (70, 64), (90, 40), (40, 90), (5, 0 + 1), (130, 130)]
    n = 0
    for nT, nD in sizes:
        for rep in range(12 if nT * nD < 3000 else 4):
            case = make_case(rng, nT, nD, int(rng.integers(0, max(1, nT // 3) + 1)), quantise)
            ref = reference_cascade(*case)
            got = run_host(*case)
            assert got[0] == ref[0], (nT, nD, rep, 'matches')
            assert got[1] == ref[1], (nT, nD, rep, 'unmatched track order')
            assert got[2] == ref[2], (nT, nD, rep, 're-identification')
            assert got[3] == ref[3], (nT, nD, rep, 'new-track detections order')
            n += 1
    assert n > 150


def test_cascade_host_no_detections_left_after_first_group():
    """tracker.py:207-209: once no detection is left the remaining depth groups go to the unmatched list unsolved."""
    rng = np.random.default_rng(5)
    nT, nD = 12, 3
    case = list(make_case(rng, nT, nD, 0, False))
    case[0][:] = 0.1                             # everything matches in the first group
    case[1][:] = 1.0
    case[3][:] = True
    case[4][:] = 0
    case[5][:] = 0
    case[6][:] = False
    case[7] = [[0, 1, 2, 3], [4, 5], [6, 7, 8], [9, 10, 11]]
    case[9] = []
    case[10], case[11] = [], []
    ref = reference_cascade(*case)
    got = run_host(*case)
    assert got == ref and len(ref[0]) == 3 and len(ref[1]) == 9
