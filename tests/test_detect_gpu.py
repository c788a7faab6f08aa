"""GPU parity of the detector / extractor pre- and post-processing (detect.hip, extract.hip).
  * filter + DIoU-NMS: oracle=reference (tests/golden/nms_kat.npz from detector.py:322-365) --
    boxes, labels identical, conf equal
  * head decode: oracle=restated (np_oracle.yolo_decode, plugins/yolo_layer.cu:127-230), fp32
    tolerance 2e-6 relative (fast-exp intrinsics differ between vendors)
  * preprocessing: oracle=restated (np_oracle.yolo_preprocess / cv_oracle.reid_preprocess),
    identical uint8 pixels -> fp16 input within 1e-3"""
import functools

import numpy as np
import pytest

import cv_oracle
import decode_cases as dc
import np_oracle as o
from decode_cases import synthetic_frame
from fastmot_amd import _lib
from fastmot_amd.detector import YOLODetector
from fastmot_amd.feature_extractor import FeatureExtractor
from fastmot_amd.models import YOLO, ReID
from fastmot_amd.models.graph import RandomWeights

pytestmark = pytest.mark.gpu


class TinyYOLO(YOLO):
    NUM_CLASSES = 3
    INPUT_SHAPE = (3, 96, 128)
    LAYER_FACTORS = [8, 16, 32]
    SCALES = [1.2, 1.1, 1.05]
    ANCHORS = [[4, 7, 8, 15, 12, 30], [18, 40, 25, 60, 30, 80], [40, 90, 60, 70, 80, 95]]


class TinyLetterbox(TinyYOLO):
    LETTERBOX = True
    NEW_COORDS = True
    SCALES = [2.0, 2.0, 2.0]


@pytest.fixture(params=['fused', 'general'])
def nms_path(ctx, request):
    """Both device paths of the candidate sort + DIoU-NMS: the fused greedy kernel (default, up to 4096 candidates) and
    the three-kernel sort / bit-matrix / scan path (fm_ctx option "nms_path" = 1; beyond 4096 candidates automatically)."""
    ctx.set_option('nms_path', 1 if request.param == 'general' else 0)
    yield request.param
    ctx.set_option('nms_path', 0)


@pytest.mark.parametrize('tag,n_cls', [('p', 1), ('q', 3)])
def test_filter_dets_matches_reference(ctx, golden_dir, tag, n_cls, nms_path):
    g = np.load(golden_dir / 'nms_kat.npz')
    det = YOLODetector((1920, 1080), tuple(range(n_cls)), model='TinyYOLO' if n_cls <= 3 else None,
                       conf_thresh=0.25, nms_thresh=0.5, max_area=800000, min_aspect_ratio=1.2)
    out = ctx.filter_dets(g[f'{tag}_det_out'])
    np.testing.assert_array_equal(out.tlbr, g[f'{tag}_tlbr'])
    np.testing.assert_array_equal(out.label, g[f'{tag}_label'])
    np.testing.assert_allclose(out.conf, g[f'{tag}_conf'], rtol=1e-7)


def test_filter_dets_random_vs_oracle(ctx, nms_path):
    rng = np.random.default_rng(5)
    det = YOLODetector((1920, 1080), (0, 2), model='TinyYOLO', conf_thresh=0.3, nms_thresh=0.45,
                       max_area=200000, min_aspect_ratio=0.5)
    for n in (0, 1, 7, 64, 65, 600, 3000):
        rows = np.stack([rng.uniform(0, 0.9, n), rng.uniform(0, 0.8, n), rng.uniform(0.01, 0.15, n),
                         rng.uniform(0.02, 0.3, n), rng.uniform(0, 1, n), rng.integers(0, 3, n),
                         rng.uniform(0.3, 1, n)], 1).astype(np.float32)
        out = ctx.filter_dets(rows)
        lm = np.array([True, False, True])
        tl, lb, cf = o.filter_dets(rows, [1920, 1080], [0, 0], lm, 0.3, 0.45, 200000, 0.5)
        np.testing.assert_array_equal(out.tlbr, tl)
        np.testing.assert_array_equal(out.label, lb)
        np.testing.assert_allclose(out.conf, cf, rtol=1e-7)


@pytest.mark.parametrize('n', [63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 2559, 2560, 2561, 2688, 2689, 2753])
def test_filter_dets_chunk_boundaries(ctx, n):
    """Candidate counts at the seams of the bit-matrix / scan path: 64-candidate chunks, two chunks per scan iteration,
    an odd number of chunks, and the 2560 rows whose loads the scan pipelines (beyond them rows are fetched at use).
    Every row passes the threshold, so K = n exactly; boxes cluster so that chains of suppression cross the chunks."""
    rng = np.random.default_rng(n)
    det = YOLODetector((1920, 1080), (0, 1, 2), model='TinyYOLO', conf_thresh=0.3, nms_thresh=0.45,
                       max_area=200000, min_aspect_ratio=0.5, max_candidates=16384)
    ctx.set_option('nms_path', 1)
    try:
        centres = rng.uniform(0.1, 0.8, (max(n // 12, 1), 2))
        pick = rng.integers(0, len(centres), n)
        rows = np.stack([centres[pick, 0] + rng.normal(0, 0.01, n), centres[pick, 1] + rng.normal(0, 0.01, n),
                         rng.uniform(0.05, 0.08, n), rng.uniform(0.1, 0.16, n), rng.uniform(0.6, 1, n),
                         rng.integers(0, 3, n), rng.uniform(0.6, 1, n)], 1).astype(np.float32)
        out = ctx.filter_dets(rows, cap=16384)
        assert ctx.detect_last_counts()[0] == n
        lm = np.array([True, True, True])
        tl, lb, cf = o.filter_dets(rows, [1920, 1080], [0, 0], lm, 0.3, 0.45, 200000, 0.5)
        assert 0 < len(tl) < n
        np.testing.assert_array_equal(out.tlbr, tl)
        np.testing.assert_array_equal(out.label, lb)
        np.testing.assert_allclose(out.conf, cf, rtol=1e-7)
    finally:
        ctx.set_option('nms_path', 0)


SIZE, ALL3 = [1920, 1080], np.array([True, True, True])


def _post_detector():
    """A fresh detector for a case of the two tests below (fm_detect_configure also clears a sticky switch to the general
    route that an earlier case may have left)."""
    return YOLODetector((1920, 1080), (0, 1, 2), model='TinyYOLO', conf_thresh=0.3, nms_thresh=0.45,
                        max_area=800000, min_aspect_ratio=0.0, max_candidates=8192)


def _assert_equals_oracle(out, ref):
    tl, lb, cf = ref
    np.testing.assert_array_equal(out.tlbr, tl)
    np.testing.assert_array_equal(out.label, lb)
    np.testing.assert_allclose(out.conf, cf, rtol=1e-7)


@functools.lru_cache(maxsize=None)
def _seam_case(n):
    """Rows like test_filter_dets_chunk_boundaries, in 8 tight clusters: (rows, candidates over the threshold, NMS
    survivors summed over the classes, oracle result) -- computed once for both routes."""
    rng = np.random.default_rng(n)
    centres = rng.uniform(0.1, 0.8, (8, 2))
    pick = rng.integers(0, 8, n)
    rows = np.stack([centres[pick, 0] + rng.normal(0, 0.004, n), centres[pick, 1] + rng.normal(0, 0.004, n),
                     rng.uniform(0.05, 0.08, n), rng.uniform(0.1, 0.16, n), rng.uniform(0.6, 1, n),
                     rng.integers(0, 3, n), rng.uniform(0.6, 1, n)], 1).astype(np.float32)
    d, _ = o.filter_scale(rows, SIZE, [0, 0], ALL3, 0.3)
    survivors = sum(len(o.diou_nms(d[d[:, 5] == c, :4], d[d[:, 5] == c, 4], 0.45)) for c in np.unique(d[:, 5]))
    return rows, len(d), survivors, o.filter_dets(rows, SIZE, [0, 0], ALL3, 0.3, 0.45, 800000, 0.0)


@pytest.mark.parametrize('n', [511, 512, 513, 1500, 2049, 4095, 4096])
def test_filter_dets_greedy_kernel_seams(ctx, n, nms_path):
    """Candidate counts at the seams of the greedy kernel, with few enough survivors that under 'fused' the greedy kernel
    itself resolves the pass (it hands a pass of more than 96 survivors to the general route): the second candidate of a
    thread from 512 on, the steps of its LDS sizing, its capacity of 4096.  The first call may be declined for LDS (the
    size adapts to the counts seen by the context), the second cannot.  (At 513 the one candidate that is a thread's
    second is no survivor: the kernel's final filter beyond a thread's first candidate is checked from 1500 on.)"""
    rows, k, survivors, ref = _seam_case(n)
    assert k == n
    assert survivors <= 80
    det = _post_detector()
    for _ in range(2):
        out = ctx.filter_dets(rows, cap=8192)
        assert ctx.detect_last_counts()[0] == n
        _assert_equals_oracle(out, ref)


def _est32(a, b):
    """float32 restatement of the second-stage estimate of the device's pair test (diou_pretest, nms_core.h)."""
    f32 = np.float32
    a, b = a.astype(f32), b.astype(f32)
    ax1, ay1, bx1, by1 = a[0] + a[2], a[1] + a[3], b[0] + b[2], b[1] + b[3]
    iw, ih = min(ax1, bx1) - max(a[0], b[0]), min(ay1, by1) - max(a[1], b[1])
    inter = f32(iw * ih)
    uni = f32(a[2] * a[3] + b[2] * b[3] - inter)
    ew, eh = max(ax1, bx1) - min(a[0], b[0]), max(ay1, by1) - min(a[1], b[1])
    dx, dy = f32(0.5) * ((a[0] + ax1) - (b[0] + bx1)), f32(0.5) * ((a[1] + ay1) - (b[1] + by1))
    q = f32((dx * dx + dy * dy) / (ew * ew + eh * eh))
    return float(inter / uni - (np.exp2(f32(0.6) * np.log2(q)) if q > 0 else 0))


@functools.lru_cache(maxsize=None)
def _threshold_pairs():
    """40 well-separated pairs (A, B = A shifted in x) on a grid, the shift bisected in float32 on the oracle's verdict
    for that pair alone down to two adjacent float32 values, one suppressed and one kept: odd pairs take the suppressed
    side, even pairs the kept side.  Returns (rows, pairs suppressed, largest |estimate - threshold|, oracle result)."""
    f32 = np.float32
    rng = np.random.default_rng(1)

    def scaled(r):
        return o.filter_scale(np.array([[*r, 1, 0, 1]], f32), SIZE, [0, 0], [True], 0.3)[0][0, :4]

    def suppressed(a, b):
        return len(o.diou_nms(np.array([scaled(a), scaled(b)], f32), np.array([1.0, 0.5]), 0.45)) == 1

    rows, n_suppressed, far = [], 0, 0.
    for p in range(40):
        w, h = rng.uniform(0.03, 0.05), rng.uniform(0.05, 0.08)
        a = np.array([(p % 8) * 0.12 + 0.01, (p // 8) * 0.12 + 0.01, w, h], f32)
        lo, hi = f32(0), f32(w)             # shift 0: identical boxes, suppressed; shift w: disjoint, kept
        while True:
            mid = f32((lo + hi) / 2)
            if mid == lo or mid == hi:
                break
            b = a.copy()
            b[0] = a[0] + mid
            if suppressed(a, b):
                lo = mid
            else:
                hi = mid
        b = a.copy()
        b[0] = a[0] + (lo if p % 2 else hi)
        n_suppressed += suppressed(a, b)
        far = max(far, abs(_est32(scaled(a), scaled(b)) - 0.45))
        rows += [[*a, 0.9, p % 3, 0.9], [*b, 0.8, p % 3, 0.9]]
    rows = np.array(rows, f32)
    return rows, n_suppressed, far, o.filter_dets(rows, SIZE, [0, 0], ALL3, 0.3, 0.45, 800000, 0.0)


def test_filter_dets_pairs_at_the_threshold(ctx, nms_path):
    """Pairs whose DIoU lies one float32 step of the shift on either side of the threshold: the float32 estimate of
    every pair is inside the band in which the device leaves the decision to the reference's float64 arithmetic (band
    1e-4; the restated estimate stays within 5e-5, the device's own a few 1e-6 from that), and that arithmetic must
    decide all 40 as the oracle does -- 20 suppressed, 20 kept."""
    rows, n_suppressed, far, ref = _threshold_pairs()
    assert n_suppressed == 20
    assert len(ref[0]) == 60
    assert far <= 5e-5
    det = _post_detector()
    out = ctx.filter_dets(rows, cap=8192)
    assert ctx.detect_last_counts()[0] == 80
    _assert_equals_oracle(out, ref)


def test_filter_dets_more_candidates_than_the_fused_kernel_holds(ctx):
    """> 4096 candidates over the threshold: the fused kernel flags the pass, the general path takes it over (and the
    following passes, until the count has fallen again); results equal the oracle throughout."""
    rng = np.random.default_rng(9)
    det = YOLODetector((1920, 1080), (0, 1, 2), model='TinyYOLO', conf_thresh=0.3, nms_thresh=0.45,
                       max_area=200000, min_aspect_ratio=0.5, max_candidates=16384)
    lm = np.array([True, True, True])
    for n in (5000, 9000, 2000, 300, 5000):
        rows = np.stack([rng.uniform(0, 0.9, n), rng.uniform(0, 0.8, n), rng.uniform(0.01, 0.15, n),
                         rng.uniform(0.02, 0.3, n), rng.uniform(0, 1, n), rng.integers(0, 3, n),
                         rng.uniform(0.4, 1, n)], 1).astype(np.float32)
        out = ctx.filter_dets(rows, cap=16384)
        tl, lb, cf = o.filter_dets(rows, [1920, 1080], [0, 0], lm, 0.3, 0.45, 200000, 0.5)
        assert ctx.detect_last_counts()[0] == int(((rows[:, 4] * rows[:, 6]) >= np.float32(0.3)).sum())
        np.testing.assert_array_equal(out.tlbr, tl)
        np.testing.assert_array_equal(out.label, lb)
        np.testing.assert_allclose(out.conf, cf, rtol=1e-7)


def _sort_detector(cap):
    return YOLODetector((1920, 1080), (0, 1, 2), model='TinyYOLO', conf_thresh=0.0, nms_thresh=dc.SORT_NMS,
                        max_area=dc.SORT_MAX_AREA, min_aspect_ratio=dc.SORT_MIN_AR, max_candidates=cap)


@pytest.mark.parametrize('cap', [8192, 16448])
def test_filter_dets_sort_ties_and_signs(ctx, cap, nms_path):
    """The candidate sort where its key's fields decide (sort_key, nms_core.h): box_conf quantised to 1/16, so the
    original index orders most neighbours; rows with negative box_conf (and cls_prob: the product passes), -0.0 and +0.0
    (conf_thresh 0 admits them; they rank as equals).  Capacity 8192 takes rank_sort_lds_kernel, 16448 -- the first
    multiple of 64 above 16384 -- the chunked rank_sort_kernel (launch_rank_sort, detect.hip), at counts around its
    256-key chunks and up to its capacity.  The sorted rows equal the host's lexsort bit for bit, the detections the
    oracle's with the original index as the tie-break.  (Beyond 4096 candidates the greedy kernel hands the pass to the
    general route whatever nms_path says: those counts run under 'general' alone.)"""
    counts = dc.SORT_COUNTS + (dc.SORT_COUNTS_LARGE if cap > 16384 and nms_path == 'general' else ())
    det = _sort_detector(cap)
    assert det._cfg.max_candidates == cap and (cap > 16384) == (cap == 16448)      # the sort kernel this capacity takes
    for n in counts:
        want, want_idx, ref, survivors = dc.sort_reference(n)
        assert survivors <= dc.SORT_SURVIVOR_CAP
        det._configure(cap)             # (clears a switch to the general route that the count before may have left)
        out = ctx.filter_dets(dc.sort_rows(n), cap=cap)
        assert ctx.detect_last_counts()[0] == n
        got = ctx.detect_raw_candidates()
        assert got.shape == (n, 8)
        np.testing.assert_array_equal(got[:, 7].copy().view(np.int32), want_idx, err_msg=f'n={n}')
        np.testing.assert_array_equal(np.ascontiguousarray(got[:, :7]).view(np.uint32), want.view(np.uint32), err_msg=f'n={n}')
        _assert_equals_oracle(out, ref)


@pytest.mark.parametrize('model', ['TinyYOLO', 'TinyLetterbox'])
def test_preprocess_decode_end_to_end(ctx, model):
    size = (320, 180)
    det = YOLODetector(size, (0, 1, 2), model=model, conf_thresh=0.1, nms_thresh=0.5,
                       weights=RandomWeights(seed=4), max_candidates=16384, reuse_buffers=False)
    frame = synthetic_frame(*size, seed=1)
    ctx.frame_configure(*size)
    ctx.frame_upload(frame)
    ctx.detect_preprocess_only()
    m = det.model
    inp = det.backend.read(det.graph.input, 1)[0]            # [h, w, 3] RGB
    exp = o.yolo_preprocess(frame, m.INPUT_SHAPE[1:], det.roi if m.LETTERBOX else None)
    np.testing.assert_allclose(inp.transpose(2, 0, 1), exp, rtol=0, atol=6e-4)   # fp16 storage of u8/255
    # the u8 pixels themselves must be identical
    np.testing.assert_array_equal(np.rint(inp.transpose(2, 0, 1) * 255), np.rint(exp * 255))
    dets = det(frame)
    # oracle: decode the engine's own head tensors, then the reference filter
    rows = []
    for i, head in enumerate(det.heads):
        t = det.backend.read(head, 1)[0]                       # [gh, gw, (5+C)*A] fp32
        rows.append(o.yolo_decode(t.transpose(2, 0, 1), m.ANCHORS[i], m.NUM_CLASSES,
                                  (m.INPUT_SHAPE[2], m.INPUT_SHAPE[1]), m.SCALES[i], m.NEW_COORDS))
    rows = np.concatenate(rows)
    tl, lb, cf = o.filter_dets(rows, det.upscaled_sz, det.bbox_offset, det.label_mask, 0.1, 0.5, 800000, 1.2)
    assert len(dets) == len(tl) and len(tl) > 0
    # The output order is by confidence; detections whose confidences agree to ~1e-4 may swap places between
    # the fast-exp device decode and the oracle (seen: 0.2328964 vs 0.2328774), so rows are matched first:
    # every oracle row pairs with the nearest unused device row of the same label.
    order, used = [], np.zeros(len(tl), bool)
    for j in range(len(tl)):
        d = np.abs(dets.tlbr - tl[j]).max(1) + 1e6 * ((dets.label != lb[j]) | used)
        order.append(int(np.argmin(d)))
        used[order[-1]] = True
    order = np.array(order)
    assert (np.abs(order - np.arange(len(tl))) <= 2).all()        # only neighbours swap
    np.testing.assert_array_equal(dets.label[order], lb)
    # boxes come from fp32 fast-exp decode: allow +-1 px on <=1% of coordinates, confidences 5e-6
    diff = np.abs(dets.tlbr[order] - tl)
    assert diff.max() <= 1 and (diff > 0).mean() <= 0.01
    np.testing.assert_allclose(dets.conf[order], cf, rtol=5e-6)


def test_stale_prefetch_is_dropped(ctx):
    """prefetch(f_x) followed by detect_async(f_1) with another frame: postprocess() returns f_1's detections
    (detector passes are collected in the order they were enqueued, so the announced-but-unused pass is
    collected and dropped first); the announced frame itself is recognised by identity and not run twice."""
    size = (320, 180)
    det = YOLODetector(size, (0, 1, 2), model='TinyYOLO', conf_thresh=0.1, nms_thresh=0.5,
                       weights=RandomWeights(seed=4), max_candidates=16384, reuse_buffers=False)
    f0, f1, fx = (synthetic_frame(*size, seed=s) for s in (1, 2, 3))
    want0, want1 = det(f0).copy(), det(f1).copy()
    assert len(want0) and len(want1) and (len(want0) != len(want1) or (want0.tlbr != want1.tlbr).any())
    det.detect_async(f0)
    det.prefetch(fx)
    got0 = det.postprocess().copy()
    det.detect_async(f1)                      # not the announced frame
    got1 = det.postprocess().copy()
    det.detect_async(f0)
    det.prefetch(f1)
    det.postprocess()
    det.detect_async(f1)                      # the announced frame: no second pass
    got1b = det.postprocess().copy()
    for got, want in ((got0, want0), (got1, want1), (got1b, want1)):
        assert len(got) == len(want)
        np.testing.assert_array_equal(got.tlbr, want.tlbr)
        np.testing.assert_array_equal(got.label, want.label)


def test_reid_crop_resize_normalise(ctx):
    size = (640, 360)
    frame = synthetic_frame(*size, seed=2)
    ext = FeatureExtractor('OSNet025', batch_size=8, weights=RandomWeights(seed=3), size=size)
    boxes = np.array([[10.7, 20.2, 70.9, 200.1], [-5., -8., 40., 90.], [600., 300., 700., 400.],
                      [100., 50., 131., 113.], [300., 10., 555., 355.]])
    ext.extract_async(frame, boxes)
    emb = ext.postprocess()
    assert emb.shape == (5, 512)
    np.testing.assert_allclose(np.linalg.norm(emb, axis=1), 1, atol=1e-5)
    inp = ctx.extract_read_input(5, 128, 256)
    exp = cv_oracle.reid_preprocess(frame, boxes).transpose(0, 2, 3, 1)
    np.testing.assert_allclose(inp, exp, rtol=0, atol=2.5e-3)     # fp16 storage of values in [-2.2, 2.7]
    # chunked extraction (n > batch_size) gives the same embeddings row by row
    many = np.concatenate([boxes] * 4)
    ext.extract_async(frame, many)
    emb2 = ext.postprocess()
    np.testing.assert_allclose(emb2[:5], emb, atol=1e-6)
    np.testing.assert_allclose(emb2[15:20], emb, atol=1e-6)


def test_reid_crop_exact_2x_uses_area_average(ctx):
    """cv2.resize(INTER_LINEAR) switches to the INTER_AREA 2x2 mean when the crop is exactly twice the network
    input in both axes (256x512 -> 128x256); crops one pixel off stay bilinear."""
    size = (800, 600)
    frame = synthetic_frame(*size, seed=6)
    ext = FeatureExtractor('OSNet025', batch_size=8, weights=RandomWeights(seed=3), size=size)
    boxes = np.array([[100., 20., 355., 531.], [101., 20., 355., 531.], [300., 60., 555., 571.9]])
    ext.extract_async(frame, boxes)
    ext.postprocess()
    inp = ctx.extract_read_input(3, 128, 256)
    exp = cv_oracle.reid_preprocess(frame, boxes).transpose(0, 2, 3, 1)
    np.testing.assert_allclose(inp, exp, rtol=0, atol=2.5e-3)
    crop = frame[20:532, 100:356].astype(np.int64)
    area = (crop[0::2, 0::2] + crop[0::2, 1::2] + crop[1::2, 0::2] + crop[1::2, 1::2] + 2) >> 2
    mean, std = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
    np.testing.assert_allclose(inp[0], (area[..., ::-1] / 255. - mean) / std, rtol=0, atol=2.5e-3)


def test_reid_split_batches_identical(ctx):
    """Two or four network instances running the parts of a batch concurrently (FM_NET_EXTRACTOR_B.., extract.hip) give
    the same embedding rows, bit for bit, as one instance running the whole batch -- for even, odd and
    below-threshold box counts."""
    size = (640, 360)
    frame = synthetic_frame(*size, seed=4)
    rng = np.random.default_rng(5)
    x0, y0 = rng.uniform(0, 500, 33), rng.uniform(0, 250, 33)
    boxes = np.stack([x0, y0, x0 + rng.uniform(20, 120, 33), y0 + rng.uniform(40, 100, 33)], 1)
    embs = {}
    for split in (4, 2, 1):
        ext = FeatureExtractor('OSNet025', batch_size=32, weights=RandomWeights(seed=3), size=size, split_batches=split)
        assert len(ext.extra_backends) == split - 1
        for n in (33, 32, 9, 7, 1):
            ext.extract_async(frame, boxes[:n])
            embs[split, n] = ext.postprocess().copy()
            assert embs[split, n].shape == (n, 512)
    for n in (33, 32, 9, 7, 1):
        np.testing.assert_array_equal(embs[2, n], embs[1, n])
        np.testing.assert_array_equal(embs[4, n], embs[1, n])


@pytest.mark.parametrize('model', ['TinyYOLO', 'TinyLetterbox', 'YOLOv4_608', 'YOLOv4CSP_640', 'YOLOv4P6_1280'])
def test_fused_input_stem_equals_preprocess_kernel(ctx, model):
    """Round 6: the detector's stem convolution computes the resized / normalised input pixels itself (fm_ctx option
    "fused_input", default 1; stemconv.hip + pixel_source.h) instead of reading the tensor preprocess_kernel wrote.
    Same pixel function on both paths: every head tensor and the detections are equal bit for bit.  The three benchmark
    geometries: 1080p -> 608^2 (stretched), 1080p -> 640^2 (letterboxed), 4K -> 1280^2 (the three-stage stem)."""
    size = {'YOLOv4_608': (1920, 1080), 'YOLOv4CSP_640': (1920, 1080), 'YOLOv4P6_1280': (3840, 2160)}.get(model, (320, 180))
    det = YOLODetector(size, (0, 1, 2), model=model, conf_thresh=0.1, nms_thresh=0.5, weights=RandomWeights(seed=4),
                       max_candidates=65536, reuse_buffers=False)
    frame = synthetic_frame(*size, seed=11)
    outs = {}
    try:
        for fused in (1, 0, 1):
            ctx.set_option('fused_input', fused)
            dets = det(frame)
            heads = [det.backend.read(h, 1).copy() for h in det.heads]
            stem = det.backend.read(det.graph.layers[0]['out'], 1).copy()
            outs.setdefault(fused, []).append((dets, heads, stem))
    finally:
        ctx.set_option('fused_input', 1)
    assert det.graph.layers[0]['op'] in (12, 18)                # FM_OP_STEMCONV / FM_OP_STEM2: the fused path really is in use
    if model == 'YOLOv4CSP_640':
        assert YOLO.get_model(model).LETTERBOX
    if model in ('YOLOv4CSP_640', 'YOLOv4P6_1280'):             # the benchmark tables start with the fused stem launch
        assert det.graph.layers[0]['op'] == 18 and (model != 'YOLOv4P6_1280' or 'stem3_ref' in det.graph.layers[0])
    for dets, heads, stem in outs[1][1:] + outs[0]:
        ref = outs[1][0]
        np.testing.assert_array_equal(stem, ref[2])
        for a, b in zip(heads, ref[1]):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(dets.tlbr, ref[0].tlbr)
        np.testing.assert_array_equal(dets.conf, ref[0].conf)


@pytest.mark.parametrize('model,n', [('OSNet025', 5), ('OSNet025', 19), ('OSNet10', 5)])
def test_fused_input_stem_equals_crop_kernel(ctx, model, n):
    """The same for the ReID network: crop -> resize -> normalise inside OSNet's 7x7 stem (chunked batches included:
    n > batch_size) against crop_resize_kernel + input tensor -- embeddings equal bit for bit."""
    size = (640, 360)
    frame = synthetic_frame(*size, seed=2)
    ext = FeatureExtractor(model, batch_size=8, weights=RandomWeights(seed=3), size=size)
    rng = np.random.default_rng(n)
    tl = rng.uniform([-20, -20], [560, 250], (n, 2))
    boxes = np.concatenate([tl, tl + rng.uniform([8, 16], [140, 300], (n, 2))], axis=1)
    embs = {}
    try:
        for fused in (1, 0):
            ctx.set_option('fused_input', fused)
            ext.extract_async(frame, boxes)
            embs[fused] = ext.postprocess().copy()
    finally:
        ctx.set_option('fused_input', 1)
    # (OSNet-x1.0's first conv has 64 output channels: not a stem-kernel layer, both settings take the crop kernel)
    assert (ext.graph.layers[0]['op'] == 12) == (model == 'OSNet025')
    np.testing.assert_array_equal(embs[1], embs[0])
    if n <= 8:
        inp = ctx.extract_read_input(n, 128, 256)            # (refilled by the front-end kernel on the fused path)
        exp = cv_oracle.reid_preprocess(frame, boxes).transpose(0, 2, 3, 1)
        np.testing.assert_allclose(inp, exp, rtol=0, atol=2.5e-3)


def test_embedding_buffer_growth_keeps_captured_graphs_valid(ctx):
    """The ReID head layer writes its rows through pointers baked into captured graphs.  A batch larger than the
    embedding buffer re-allocates it (device rows + their page-locked mirror): the graphs captured for earlier, smaller
    batches must not survive that (until round 6 they did, and replayed into the freed buffer)."""
    size = (640, 360)
    frame = synthetic_frame(*size, seed=8)
    ext = FeatureExtractor('OSNet025', batch_size=8, weights=RandomWeights(seed=3), size=size)
    rng = np.random.default_rng(1)

    def boxes(n):
        tl = rng.uniform([0, 0], [500, 200], (n, 2))
        return np.concatenate([tl, tl + rng.uniform([10, 20], [120, 150], (n, 2))], axis=1)
    small = boxes(5)
    first = [ext(frame, small).copy() for _ in range(3)]            # eager validation, capture, replay
    many = boxes(150)                                               # > 64 rows (and > 128): the buffers grow
    big = ext(frame, many).copy()
    again = ext(frame, small).copy()
    np.testing.assert_array_equal(first[0], first[2])
    np.testing.assert_array_equal(again, first[0])
    np.testing.assert_array_equal(ext(frame, many), big)
    np.testing.assert_allclose(np.linalg.norm(big, axis=1), 1, atol=1e-5)
