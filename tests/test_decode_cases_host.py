"""The inputs of tests/test_decode_gpu.py and of test_detect_gpu.test_filter_dets_sort_ties_and_signs (tests/decode_cases.py)
have the properties those tests rely on -- proven on the CPU references alone (tests/torch_ref.run_graph, np_oracle): the
forced class ties exist and are maxima, every class wins somewhere for nc <= 7, a threshold fits into a gap ten criteria
wide, 20 to 700 of the 756 rows are candidates; the sort rows repeat their box_conf, carry negative and zero values and
leave few enough NMS survivors for the Python oracle."""
import numpy as np
import pytest

import decode_cases as dc


@pytest.mark.parametrize('form', dc.FORMS)
@pytest.mark.parametrize('nc', dc.CLASS_COUNTS)
def test_decode_heads_have_their_ties_coverage_and_gap(nc, form):
    heads = dc.host_heads(nc, form)
    thresh, k = dc.check_preconditions(heads, nc, form)
    m = dc.model(nc, form)
    rows = dc.oracle_rows(heads, m)
    # boxes of both extremes are among the candidates: sub-pixel (anchor 2) and many times the frame (anchor 1)
    cand = rows[(rows[:, 4] * rows[:, 6]) >= np.float32(thresh)]
    px = cand[:, 2] * dc.SIZE[0] * cand[:, 3] * dc.SIZE[1]
    assert (px < 1e-2).any() and (px > 2 * dc.MAX_AREA).any()
    print(f'DECODECASE nc{nc} {form}: threshold {thresh:.6f}, {k} candidates, scan {dc.scan_shape(nc)}')


def test_scan_shapes_cover_the_class_scan():
    shapes = {nc: dc.scan_shape(nc) for nc in dc.CLASS_COUNTS}
    assert {v[1] for v in shapes.values()} == {0, 1, 2, 3}              # every tail length
    assert shapes[1][0] == shapes[3][0] == 0 and shapes[4] == (1, 0) and shapes[80] == (20, 0) and shapes[128] == (32, 0)
    for nc in dc.CLASS_COUNTS:                                           # the pairs straddle what their names say
        for i, j in dc.tie_pairs(nc):
            assert i < j < nc
    assert (3, 4) in dc.tie_pairs(5) and (4, 5) in dc.tie_pairs(6) and (3, 70) in dc.tie_pairs(80)


@pytest.mark.parametrize('n', dc.SORT_COUNTS + dc.SORT_COUNTS_LARGE)
def test_sort_rows_repeat_and_change_sign(n):
    rows = dc.sort_rows(n)
    srt, idx, ref, survivors = dc.sort_reference(n)
    assert len(srt) == n and sorted(idx.tolist()) == list(range(n))
    assert survivors <= dc.SORT_SURVIVOR_CAP
    if n >= 7:
        assert (rows[:, 4] < 0).any() and ((rows[:, 4] < 0) <= (rows[:, 6] < 0)).all()
        zeros = rows[rows[:, 4] == 0, 4]
        assert np.signbit(zeros).any() and (~np.signbit(zeros)).any()
    if n >= 255:
        repeated = 0
        for c in range(3):
            _, counts = np.unique(rows[rows[:, 5] == c, 4], return_counts=True)
            repeated += counts[counts > 1].sum()
        assert repeated >= n / 2
        assert len(ref[0]) > 0
    # the reference order is (class asc, box_conf desc, index asc), zeros of either sign equal
    key = list(zip(srt[:, 5].tolist(), (-srt[:, 4].astype(float) + 0.0).tolist(), idx.tolist()))
    assert key == sorted(key)
