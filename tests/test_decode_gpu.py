"""GPU: the anchor-head decode (decode_kernel, detect.hip) off its defaults -- every shape of its class scan (four logits
per 16-byte load, then a scalar tail), forced class ties on both sides of every seam, both head forms, boxes of both
extremes.  The networks and their scripted heads are tests/decode_cases.py's (proven on the CPU by
tests/test_decode_cases_host.py); everything here is asserted on the DEVICE'S OWN head tensors.
  * candidates: oracle=restated (np_oracle.yolo_decode + filter_scale) with the threshold in a gap of the oracle's scores
    ten criteria wide: the SET of original indices is identical, class ids exact, the other columns within the project's
    criterion for this kernel (oracle/detector_check.py: rel 5e-6 of |e| + 1e-3 * scale); worst ratio printed (DECODEBOUND)
  * sort: the device's rows obey (class asc, box_conf desc, original index asc)
  * detections: oracle=np_oracle.nms_finalize on the device's candidates, tlbr and label exact, conf rtol 1e-7
  * class mask: the winner of a tie turned off -- its rows disappear, the tied higher class does not take them"""
import numpy as np
import pytest

import decode_cases as dc
import np_oracle as o
from fastmot_amd.detector import YOLODetector

pytestmark = pytest.mark.gpu

# (vector iterations, tail length) of the class scan each class count must take
SCAN = {1: (0, 1), 3: (0, 3), 4: (1, 0), 5: (1, 1), 6: (1, 2), 7: (1, 3), 80: (20, 0), 128: (32, 0)}
REL = dc.SCORE_REL


def _device_heads(det):
    n = (5 + det.model.NUM_CLASSES) * 3
    return [np.ascontiguousarray(det.backend.read(h, 1)[0].transpose(2, 0, 1)[:n]) for h in det.heads]


def _check_pass(ctx, det, frame, heads, thresh, label):
    """One pass at the configured threshold / mask against the oracle's decode of `heads`: -> (original indices, rows by index)"""
    m = det.model
    dets = det(frame).copy()
    cand = ctx.detect_raw_candidates().copy()                   # sorted rows [k, 8]
    orig = cand[:, 7].copy().view(np.int32)
    assert ctx.detect_last_counts() == (len(cand), len(dets))
    exp, idx = o.filter_scale(dc.oracle_rows(heads, m), det.upscaled_sz, det.bbox_offset, det.label_mask, thresh)
    # 1. the candidate set, no edge allowance
    assert sorted(orig.tolist()) == idx.tolist(), (label, len(orig), len(idx))
    # 2. the rows
    by_orig = np.argsort(orig, kind='stable')
    c = cand[by_orig, :7]
    np.testing.assert_array_equal(c[:, 5], exp[:, 5])
    sz = det.upscaled_sz
    scale = np.array([sz[0], sz[1], sz[0], sz[1], 1, 1, 1], float)
    rel = np.abs(c.astype(float) - exp) / (np.abs(exp) + 1e-3 * scale)
    worst = float(rel[:, [0, 1, 2, 3, 4, 6]].max()) if len(c) else 0.0
    print(f'DECODEBOUND {label:34s} {len(c):4d} rows, worst rel / criterion {worst / REL:.3g}')
    assert worst <= REL, (label, worst)
    # 3. the sort order
    key = list(zip(cand[:, 5].astype(int).tolist(), (-cand[:, 4].astype(float)).tolist(), orig.tolist()))
    assert key == sorted(key)
    # 4. the detections
    tl, lb, cf = o.nms_finalize(c, det.nms_thresh, det.max_area, det.min_aspect_ratio, tie_rank=orig[by_orig])
    np.testing.assert_array_equal(dets.tlbr, tl)
    np.testing.assert_array_equal(dets.label, lb)
    np.testing.assert_allclose(dets.conf, cf, rtol=1e-7)
    return orig[by_orig], c


def _reconfigure(det, thresh, mask=None):
    det.conf_thresh = thresh
    if mask is not None:
        det.label_mask[:] = mask
    det._configure(8192)


@pytest.mark.parametrize('form', dc.FORMS)
@pytest.mark.parametrize('nc', dc.CLASS_COUNTS)
def test_decode_class_scan_ties_and_box_extremes(ctx, nc, form):
    frame = dc.frame()
    m = dc.model(nc, form)
    det = YOLODetector(dc.SIZE, tuple(range(nc)), model=m.__name__, conf_thresh=0.25, nms_thresh=0.5, max_area=dc.MAX_AREA,
                       min_aspect_ratio=0.0, weights=dc.weights(nc, form), max_candidates=8192, reuse_buffers=False)
    try:
        assert det.model.NEW_COORDS == (form == 'new_coords') == det.model.LETTERBOX
        assert (det._cfg.num_classes // 4, det._cfg.num_classes % 4) == SCAN[nc] == dc.scan_shape(nc)   # the route
        det(frame)
        heads = _device_heads(det)
        assert sum(t.shape[1] * t.shape[2] * 3 for t in heads) == dc.N_ROWS
        # the ties, the coverage of the classes, the gap: on the device's tensors
        thresh, k = dc.check_preconditions(heads, nc, form)
        _reconfigure(det, thresh)
        label = f'nc{nc} {form}'
        orig, c = _check_pass(ctx, det, frame, heads, thresh, label)
        assert len(orig) == k
        for pair in dc.tie_pairs(nc) + ([dc.saturated_pair(nc, form)] if dc.saturated_pair(nc, form) else []):
            tied = np.intersect1d(orig, dc.tie_rows(heads, nc, pair))
            assert len(tied) >= 3, (label, pair)
            assert (c[np.isin(orig, tied), 5] == pair[0]).all()             # the lower index wins
        # boxes of both extremes are candidates, survive the NMS and are removed by the final filter
        survivors = sum(len(o.diou_nms(c[c[:, 5] == v, :4], c[c[:, 5] == v, 4], det.nms_thresh, tie_rank=orig[c[:, 5] == v]))
                        for v in np.unique(c[:, 5]))
        any_area = len(o.nms_finalize(c, det.nms_thresh, np.inf, 0.0, tie_rank=orig)[0])
        assert survivors > any_area > ctx.detect_last_counts()[1]             # (zero area; over max_area)
        assert (c[:, 2] * c[:, 3] < 1e-2).any() and (c[:, 2] * c[:, 3] > 2 * dc.MAX_AREA).any()
        if nc >= 3:
            # 5. the class mask: class 1 (the winner of the tie (1, 2)) and class 0 (NEW_COORDS: the winner of the saturated
            # tie (0, nc - 1)) off
            mask = np.ones(nc, bool)
            mask[[0, 1]] = False
            _reconfigure(det, thresh, mask)
            orig2, c2 = _check_pass(ctx, det, frame, heads, thresh, label + ' masked')
            tied = np.intersect1d(orig, dc.tie_rows(heads, nc, (1, 2)))
            assert len(tied) >= 3 and not np.isin(orig2, tied).any()
            assert 0 < len(orig2) < len(orig) and not np.isin(c2[:, 5], [0, 1]).any()
            assert np.isin(orig2, orig).all()                               # nothing took a masked row's place
    finally:
        det.backend.close()
