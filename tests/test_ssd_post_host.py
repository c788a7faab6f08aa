"""CPU: the float64 restatement of the SSD decode + NMS + top-K (tests/ssd_ref.py) on hand-made cases -- the reference
the device kernels of ssd.hip are compared against (tests/test_ssd_detect_gpu.py) has to be right by itself."""
import math

import numpy as np

import ssd_ref


def _boxes(n):
    """n well separated unit-less boxes (no overlap at all)"""
    return np.array([[0.01 * i, 0.0, 0.01 * i + 0.005, 0.005] for i in range(n)])


def test_decode_centre_coding():
    anchors = np.array([[0.5, 0.25, 0.2, 0.4]])
    loc = np.array([[[10 * 0.5, 10 * -0.25, 5 * math.log(2.0), 5 * math.log(0.5)]]])
    boxes, scores = ssd_ref.decode(loc, np.array([[[0.0, math.log(3.0)]]]), anchors, (10, 10, 5, 5))
    cy, cx, h, w = 0.5 * 0.2 + 0.5, -0.25 * 0.4 + 0.25, 0.4, 0.2
    np.testing.assert_allclose(boxes[0, 0], [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], rtol=1e-12)
    np.testing.assert_allclose(scores[0, 0], [0.5, 0.75], rtol=1e-12)
    big = np.array([[[0., 0., 5 * 5., 5 * 5.]]])
    assert np.array_equal(ssd_ref.decode(big, np.zeros((1, 1, 2)), anchors, (10, 10, 5, 5))[0][0, 0], [0., 0., 1., 1.])   # clipped


def test_suppression_just_above_and_just_below_the_threshold():
    # two boxes of equal size shifted by d: IoU = (1 - d) / (1 + d); 0.5 at d = 1 / 3
    def pair(d):
        return np.array([[[0.0, 0.0, 0.3, 0.3], [0.3 * d, 0.0, 0.3 * d + 0.3, 0.3]]])
    scores = np.zeros((1, 2, 2))
    scores[0, :, 1] = [0.9, 0.8]
    rows, which = ssd_ref.nms_topk(pair(1 / 3 - 1e-3), scores, 4, 0.5)          # IoU just above: the second box goes
    assert list(which) == [0, -1, -1, -1] and rows[0, 2] == 0.9
    rows, which = ssd_ref.nms_topk(pair(1 / 3 + 1e-3), scores, 4, 0.5)          # just below: both stay
    assert list(which) == [0, 1, -1, -1]
    # a suppressed box suppresses nothing: c overlaps b (dropped by a) but not a
    boxes = np.array([[[0.0, 0.0, 0.3, 0.3], [0.05, 0.0, 0.35, 0.3], [0.2, 0.0, 0.5, 0.3]]])
    scores = np.zeros((1, 3, 2))
    scores[0, :, 1] = [0.9, 0.8, 0.7]
    assert list(ssd_ref.nms_topk(boxes, scores, 3, 0.5)[1]) == [0, 2, -1]


def test_per_class_topk_truncation_precedes_nms():
    # 6 disjoint boxes, topk 4: only the 4 best of the class are candidates, although all 6 would survive NMS
    scores = np.zeros((1, 6, 2))
    scores[0, :, 1] = [0.3, 0.9, 0.5, 0.8, 0.2, 0.7]
    stats = {}
    rows, which = ssd_ref.nms_topk(_boxes(6)[None], scores, 4, 0.5, stats)
    assert list(which) == [1, 3, 5, 2] and stats['max_candidates'] == 6
    # scores at or below 1e-8 are no candidates
    scores[0, :, 1] = [0.3, 1e-8, 0.5, 5e-9, 0.2, 0.7]
    assert list(ssd_ref.nms_topk(_boxes(6)[None], scores, 6, 0.5)[1]) == [5, 2, 0, 4, -1, -1]


def test_global_topk_across_classes_and_background():
    scores = np.zeros((1, 3, 4))
    scores[0, :, 0] = 0.99                    # background: never reported
    scores[0, :, 1] = [0.6, 0.1, 0.2]
    scores[0, :, 2] = [0.5, 0.7, 0.3]
    scores[0, :, 3] = [0.05, 0.4, 0.8]
    stats = {}
    rows, which = ssd_ref.nms_topk(_boxes(3)[None], scores, 3, 0.5, stats)
    assert stats['max_survivors'] == 9
    assert [tuple(r[1:3]) for r in rows] == [(3, 0.8), (2, 0.7), (1, 0.6)] and list(which) == [2, 1, 0]
    np.testing.assert_array_equal(rows[0, 3:], _boxes(3)[2])


def test_ties_go_to_the_lower_class_then_the_lower_anchor():
    scores = np.zeros((1, 3, 3))
    scores[0, :, 1] = [0.5, 0.5, 0.25]
    scores[0, :, 2] = [0.5, 0.25, 0.5]
    rows, which = ssd_ref.nms_topk(_boxes(3)[None], scores, 6, 0.5)
    assert [(int(r[1]), a) for r, a in zip(rows, which)] == [(1, 0), (1, 1), (2, 0), (2, 2), (1, 2), (2, 1)]
    # within a class the tie decides who is a candidate at all
    assert list(ssd_ref.nms_topk(_boxes(3)[None], scores[:, :, :2], 1, 0.5)[1]) == [0]


def test_padding_rows_and_tiles():
    scores = np.zeros((2, 2, 2))
    scores[1, 0, 1] = 0.4
    rows, which = ssd_ref.nms_topk(np.stack([_boxes(2)] * 2), scores, 3, 0.5)
    assert rows.shape == (6, 7)
    assert np.array_equal(rows[:3], [[0, -1, 0, 0, 0, 0, 0]] * 3)
    assert np.array_equal(rows[3], [1, 1, 0.4, *_boxes(2)[0]]) and np.array_equal(rows[4:], [[1, -1, 0, 0, 0, 0, 0]] * 2)
    assert list(which) == [-1, -1, -1, 0, -1, -1]


def test_split_heads_channel_order():
    a, c = 2, 3
    h = np.arange(1 * 2 * a * (4 + c), dtype=np.float64).reshape(1, 2, a * (4 + c))
    loc, logit = ssd_ref.split_heads([h], [a], c)
    assert loc.shape == (1, 4, 4) and logit.shape == (1, 4, 3)
    assert list(loc[0, 1]) == [4, 5, 6, 7] and list(logit[0, 1]) == [11, 12, 13] and list(loc[0, 2]) == [14, 15, 16, 17]
