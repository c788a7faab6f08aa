"""fm_cascade_host -- the host half of the one-call association cascade (csrc/assoc.hip cascade_run) -- against the
oracle's restatement of the reference's stage logic (np_oracle.matching_cost / gate_cost / lsa / assignment_matches /
greedy_match: utils/matching.py, tracker.py:198-248, pinned by the reference-generated goldens) on seeded pairwise
terms.  CPU only: the routine touches no device.  Sizes cross the table-growth boundaries of Numba's set (16, 32, 64
entries), costs carry exact ties, gated pairs, empty groups and label mismatches."""
import ctypes as C

import numpy as np
import pytest

import np_oracle as o
from cascade_cases import make_case, reference_cascade, run_host
from fastmot_amd import _lib


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


def test_cascade_host_no_detections():
    """nD = 0: nothing is solved; the confirmed rows leave through the stage-1 (inactive) or stage-2 (active) unmatched
    lists in group order, the unconfirmed ones through stage 3."""
    rng = np.random.default_rng(21)
    nT = 11
    case = list(make_case(rng, nT, 0, 2, False))
    rows = rng.permutation(nT).tolist()
    case[7] = [rows[:4], [], rows[4:7]]                     # two non-empty depth groups around an empty one
    case[9] = rows[7:9]
    case[10] = rows[9:]
    active = np.zeros(nT, bool)
    active[rows[1:3] + rows[5:6] + rows[7:8]] = True
    case[8] = active
    ref = reference_cascade(*case)
    conf = rows[:7]
    assert ref == ([], [r for r in conf if not active[r]] + [r for r in conf if active[r]] + rows[7:9], [], [])
    assert 0 < active[conf].sum() < len(conf)
    assert run_host(*case) == ref
    assert run_host(*case, null_terms=True) == ref          # no labels are read for rows that meet no detection


def test_cascade_host_no_rows():
    """nT = 0: the detections at or above conf_thresh start new tracks, the occluded ones first."""
    rng = np.random.default_rng(22)
    nD = 13
    case = list(make_case(rng, 0, nD, 0, False))
    det_conf, docc, p = case[12], case[6], case[13]
    docc[:] = False
    docc[[1, 4, 5, 10]] = True
    det_conf[:] = rng.uniform(p['conf_thresh'] + 0.01, 1., nD)
    det_conf[[0, 4, 7]] = p['conf_thresh'] - 0.1
    det_conf[[1, 2]] = p['conf_thresh']                     # at the threshold: kept
    keep = [d for d in range(nD) if d not in (0, 4, 7)]
    ref = reference_cascade(*case)
    assert ref == ([], [], [], [d for d in keep if docc[d]] + [d for d in keep if not docc[d]])
    assert run_host(*case) == ref


def test_host_fill_equals_the_oracle_cost_exactly():
    """The cost matrix the host way of the cascade fills (fm_stage_cost_host: the one cost rule stage_cost_kernel applies
    too) is the oracle's matching_cost / gate_cost to the bit, for the three stages of an 8 x 9 problem with exact ties."""
    rng = np.random.default_rng(31)
    nT, nD = 8, 9
    feat, maha, iou, has_feat, tlab, dlab, docc, _, _, _, _, _, _, p = make_case(rng, nT, nD, 0, True)
    has_feat[2] = False
    docc[3] = True
    rows, cols = rng.permutation(nT).astype(np.int32), rng.permutation(nD).astype(np.int32)
    reid_labels = rng.integers(0, int(tlab.max()) + 2, nT)
    f = feat[np.ix_(rows, cols)].copy()
    f[(~has_feat[rows])[:, None] | docc[cols][None, :]] = p['fill_val']
    m = maha[np.ix_(rows, cols)]
    exp = {_lib.STAGE_MATCHING: (o.matching_cost(f, m, tlab[rows], dlab[cols], p['motion_weight'], p['max_assoc_cost']),
                                 tlab[rows], p['motion_weight'], p['max_assoc_cost']),
           _lib.STAGE_IOU: (o.gate_cost(iou[np.ix_(rows, cols)], tlab[rows], dlab[cols], p['max_iou_cost']),
                            tlab[rows], 0., p['max_iou_cost']),
           _lib.STAGE_REID: (o.gate_cost(feat[np.ix_(rows, cols)], reid_labels, dlab[cols]), reid_labels, 0., p['max_reid_cost'])}
    assert (m > 9.4877).any() and (m <= 9.4877).any()
    ins = [np.ascontiguousarray(a, t) for a, t in ((feat, np.float64), (maha, np.float64), (iou, np.float64),
                                                    (has_feat, np.uint8), (dlab, np.int64), (docc, np.uint8))]
    lib = _lib.load()
    for stage, (ref, rlab, motion_weight, max_cost) in exp.items():
        assert (ref >= 1e5).any() and (ref < 1e5).any()
        rlab = np.ascontiguousarray(rlab, np.int64)
        got = np.full((nT, nD), -1.)
        _lib.check(lib.fm_stage_cost_host(C.c_int(stage), C.c_int(nT), C.c_int(nD), *(_lib._ptr(a) for a in ins),
                                          C.c_int(nT), _lib._ptr(rows), C.c_int(nD), _lib._ptr(cols), _lib._ptr(rlab),
                                          C.c_double(motion_weight), C.c_double(max_cost), C.c_double(p['fill_val']),
                                          _lib._ptr(got)))
        np.testing.assert_array_equal(got, ref)
