"""GPU: YOLOv8 detectors from their ONNX exports (models/onnx_detector.py, csrc/dfl_decode.h).
  * decode: oracle=restated (yolov8_ref.dfl_decode, float64, on the DEVICE'S OWN head tensors): identical candidate sets,
    every row under the derived bound of yolov8_ref (worst err / bound printed)
  * batched and tiled passes against batch-1 passes / host decodes of each tile
  * NMS and box filters: oracle=np_oracle.nms_finalize on the device's candidates, bit for bit
  * every layer of v8n at 640 x 640 under the per-element bound (tests/layer_check.py)
The networks are tests/yolov8_ref.py modules with seeded weights, exported with torch's exporter into tmp files."""
import numpy as np
import pytest
import torch

import np_oracle as o
import yolov8_ref as R
from fastmot_amd import _lib
from fastmot_amd.detector import YOLODetector
from fastmot_amd.models import YOLO
from test_detect_gpu import synthetic_frame

pytestmark = pytest.mark.gpu

SIZE = (320, 180)
IN_HW = R.TINY_HW
_count = [0]


def _roi(size, in_hw, letterbox):
    """YOLODetector._create_letterbox's ROI (x, y, w, h) inside the input."""
    dst, src = np.array(in_hw[::-1]), np.array(size)
    if not letterbox:
        return None
    s = min(dst / src)
    scaled = np.rint(src * s).astype(int)
    off = ((dst - scaled) / 2).astype(int)
    return int(off[0]), int(off[1]), int(scaled[0]), int(scaled[1])


def _register(tmp_path, net, hw, letterbox):
    _count[0] += 1
    path = tmp_path / f'v8_{_count[0]}.onnx'
    path.write_bytes(R.export(net, hw))
    return YOLO.from_onnx(path, name=f'V8Test{_count[0]}', letterbox=letterbox).__name__


def _tiny_net(nc, forced):
    """The tiny net, optionally with forced class ties (two classes with the same weights and bias: equal logits in every
    cell, and the maximum there) and box logits of +-30."""
    net = R.tiny(nc=nc)
    with torch.no_grad():
        for box, cls in zip(net.detect.cv2, net.detect.cv3):
            if forced:
                box[-1].bias[5] += 30.0         # side l, bin 5
                box[-1].bias[37] -= 30.0        # side r, bin 5
                box[-1].bias[63] += 30.0        # side b, the last bin
                if nc >= 3:
                    a, b = (1, 2) if nc == 3 else (3, 70)
                    cls[-1].weight[b] = cls[-1].weight[a] * 1.0
                    cls[-1].bias[b] = cls[-1].bias[a] * 1.0
                    cls[-1].bias[a] += 1.0
                    cls[-1].bias[b] += 1.0
            else:                               # (logits wide enough that every class wins somewhere)
                cls[-1].weight *= 8.0
                cls[-1].bias.zero_()
    return net


def _tiny_detector(tmp_path, nc, letterbox, frame, size=SIZE, forced=True, frac=0.2, **kw):
    """A detector of the tiny net whose class bias is set so that about `frac` of the cells score over 0.25 on `frame`:
    the shift is read off the DEVICE'S head tensors of a first detector with the unshifted net (a bias moves every logit
    by itself), then the shifted net is exported and built."""
    kw.setdefault('max_candidates', 8192)
    args = dict(conf_thresh=0.25, nms_thresh=0.5, min_aspect_ratio=0.0, **kw)
    net = _tiny_net(nc, forced)
    det = YOLODetector(size, tuple(range(nc)), model=_register(tmp_path, net, IN_HW, letterbox), **args)
    det(frame)
    best = np.concatenate([c.max(0).reshape(-1) for _, c in _device_heads(det, max(det.n_tiles, 1))])
    det.backend.close()
    shift = float(np.log(0.25 / 0.75) - np.quantile(best, 1 - frac))
    with torch.no_grad():
        for cls in net.detect.cv3:
            cls[-1].bias += shift
    return YOLODetector(size, tuple(range(nc)), model=_register(tmp_path, net, IN_HW, letterbox), **args)


def _device_heads(det, n=1, i=0):
    """[(box [64, gh, gw], cls [nc, gh, gw])] of sample i as the device holds them."""
    nc = det.model.NUM_CLASSES
    return [(det.backend.read(b, n)[i].transpose(2, 0, 1)[:64], det.backend.read(c, n)[i].transpose(2, 0, 1)[:nc])
            for b, c in det.heads.levels]


def _gap_threshold(scores, near=0.25):
    """The middle of the widest gap between neighbouring scores among the nine nearest to `near`: no score on the edge."""
    s = np.sort(scores)
    s = s[np.sort(np.argsort(np.abs(s - near))[:9])]
    assert len(s) >= 2
    k = int(np.argmax(np.diff(s)))
    return float((s[k] + s[k + 1]) / 2), float(s[k + 1] - s[k])


def _reconfigure(det, conf_thresh, max_candidates=8192):
    det.conf_thresh = conf_thresh
    det._configure(max_candidates)


def _check_rows(got, heads, det, thresh, label, size=None, offset=None):
    """Device candidates `got` [k, 8] (any order) against the closed form of `heads`: same set, rows under the bound."""
    dec = R.dfl_decode(heads, det.heads.strides, IN_HW)
    rows, bound = R.dfl_rows(dec, IN_HW, det.upscaled_sz if size is None else size, det.bbox_offset if offset is None else offset)
    want = np.flatnonzero((dec['prob'] >= thresh) & det.label_mask[dec['cls']])
    idx = got[:, 7].copy().view(np.int32)
    assert sorted(idx.tolist()) == want.tolist(), (label, len(idx), len(want))
    got = got[np.argsort(idx)].astype(np.float64)
    np.testing.assert_array_equal(got[:, [4, 5]], rows[want][:, [4, 5]])
    err = np.abs(got[:, [0, 1, 2, 3, 6]] - rows[want][:, [0, 1, 2, 3, 6]])
    ratio = float((err / bound[want][:, [0, 1, 2, 3, 6]]).max()) if len(want) else 0.0
    print(f'DFLBOUND {label:28s} {len(want):4d} rows, worst err / bound {ratio:.3g}')
    assert ratio <= 1.0, (label, ratio)
    return len(want), dec


@pytest.mark.parametrize('nc,letterbox', [(1, True), (3, True), (3, False), (80, True), (80, False)])
def test_decode_against_closed_form(ctx, tmp_path, nc, letterbox):
    frame = synthetic_frame(*SIZE, seed=3)
    det = _tiny_detector(tmp_path, nc, letterbox, frame)
    assert det.model.HEAD == 'dfl' and det.model.LETTERBOX == letterbox and det.model.NUM_CLASSES == nc
    det(frame)
    heads = _device_heads(det)
    dec = R.dfl_decode(heads, det.heads.strides, IN_HW)
    if nc >= 3:                     # the forced ties are there, and they are maxima somewhere
        a, b = (1, 2) if nc == 3 else (3, 70)
        assert all(np.array_equal(c[a], c[b]) for _, c in heads)
        assert (dec['cls'] == a).any() and not (dec['cls'] == b).any()
    thresh, gap = _gap_threshold(dec['prob'])
    assert gap / 2 > 10 * dec['dprob'].max()        # (both neighbours lie ten bounds of the device's score away)
    for form in (0, 1):             # 16 lanes per cell, one thread per cell: the same rows, bit for bit
        ctx.set_option('dfl_decode_form', form)
        try:
            _reconfigure(det, thresh)
            det(frame)
            got = ctx.detect_raw_candidates()
        finally:
            ctx.set_option('dfl_decode_form', 0)
        k, _ = _check_rows(got, heads, det, thresh, f'nc{nc} lb{int(letterbox)} form{form}')
        cells = sum(b.shape[1] * b.shape[2] for b, _ in heads)
        assert 10 <= k < cells
        if form == 0:
            first = got[np.argsort(got[:, 7].copy().view(np.int32))]
        else:
            np.testing.assert_array_equal(first.view(np.uint32), got[np.argsort(got[:, 7].copy().view(np.int32))].view(np.uint32))


def test_class_mask(ctx, tmp_path):
    """Only the classes of class_ids leave the decode."""
    frame = synthetic_frame(*SIZE, seed=3)
    det = _tiny_detector(tmp_path, 3, True, frame, forced=False)
    det.label_mask[:] = [True, False, True]
    det(frame)
    heads = _device_heads(det)
    thresh, _ = _gap_threshold(R.dfl_decode(heads, det.heads.strides, IN_HW)['prob'])
    _reconfigure(det, thresh)
    det(frame)
    k, dec = _check_rows(ctx.detect_raw_candidates(), heads, det, thresh, 'class mask')
    assert k > 0 and ((dec['cls'] == 1) & (dec['prob'] >= thresh)).any()        # (the mask removed something)


def _same(a, b):
    assert len(a) == len(b)
    for f in ('tlbr', 'label', 'conf'):
        np.testing.assert_array_equal(a[f], b[f])


def test_detect_batch_equals_batch1(ctx, tmp_path):
    frames = [synthetic_frame(*SIZE, seed=30 + i) for i in range(2)]
    det = _tiny_detector(tmp_path, 3, True, frames[0], max_batch=2)
    want = [det(f) for f in frames]
    assert sum(len(w) for w in want) > 0
    for got, w in zip(det.detect_batch(frames), want):
        _same(got, w)


def test_tiled_pass_equals_host_decode_of_each_tile(ctx, tmp_path):
    size = (160, 64)
    frame = synthetic_frame(*size, seed=5)
    det = _tiny_detector(tmp_path, 3, False, frame, size=size, tiling_grid=(2, 1), tile_overlap=0.25, frac=0.3)
    det(frame)
    tiles = []
    for t in range(2):
        heads = _device_heads(det, 2, t)
        dec = R.dfl_decode(heads, det.heads.strides, IN_HW)
        tiles.append((heads, dec))
    thresh, _ = _gap_threshold(np.concatenate([d['prob'] for _, d in tiles]))
    _reconfigure(det, thresh)
    dets = det(frame)
    assert ctx.detect_last_counts()[0] > 0
    want_tl, want_lb, want_cf, tile_ids = [], [], [], []
    for t, (heads, dec) in enumerate(tiles):
        rows, _ = R.dfl_rows(dec, IN_HW, det.upscaled_sz, det.tile_bbox_offsets[t])
        keep = np.flatnonzero(dec['prob'] >= thresh)
        # (rows in frame pixels already; float32 as the device stores them, then the oracle's NMS + box filters)
        tl, lb, cf = o.nms_finalize(rows[keep][:, :7].astype(np.float32), det.nms_thresh, det.max_area, det.min_aspect_ratio,
                                    tie_rank=keep)
        want_tl.append(tl); want_lb.append(lb); want_cf.append(cf); tile_ids.append(np.full(len(lb), t))
    per_tile = det.last_tile_detections             # one record array per tile, before the merge
    assert [len(x) for x in per_tile] == [len(x) for x in want_lb]
    for got, tl, lb, cf in zip(per_tile, want_tl, want_lb, want_cf):
        np.testing.assert_array_equal(got.label, lb)
        assert len(lb) == 0 or np.abs(got.tlbr - tl).max() <= 1          # (rint of fp32 rows against float64 rows)
        np.testing.assert_allclose(got.conf, cf, rtol=1e-5)
    every = np.concatenate(per_tile).view(np.recarray)
    _same(dets, _lib.merge_tiles(every, np.concatenate(tile_ids), 2, det.merge_thresh))


def test_nms_and_filters_equal_the_oracle(ctx, tmp_path):
    """YOLODetector(...)() end to end: the detections are the oracle's NMS + box filters of the device's candidates."""
    frame = synthetic_frame(*SIZE, seed=8)
    det = _tiny_detector(tmp_path, 3, True, frame, frac=0.5)
    det.min_aspect_ratio = 0.3
    _reconfigure(det, 0.25)
    dets = det(frame)
    cand = ctx.detect_raw_candidates()              # sorted by (class, box_conf desc, index)
    assert len(cand) >= 20
    tl, lb, cf = o.nms_finalize(cand[:, :7], det.nms_thresh, det.max_area, det.min_aspect_ratio,
                                tie_rank=cand[:, 7].copy().view(np.int32))
    assert 0 < len(tl) < len(cand)
    np.testing.assert_array_equal(dets.tlbr, tl)
    np.testing.assert_array_equal(dets.label, lb)
    np.testing.assert_allclose(dets.conf, cf, rtol=1e-7)
    # the measurement hook (scripts/yolov8_timing.py) runs the decode alone and leaves the detector as it was
    assert 0 < ctx.detect_decode_us(2) < 1e4
    _same(det(frame), dets)


def test_overflow_is_an_error_not_a_fault(ctx, tmp_path):
    frame = synthetic_frame(*SIZE, seed=3)
    det = _tiny_detector(tmp_path, 3, True, frame, frac=0.8)
    det(frame)
    assert ctx.detect_last_counts()[0] > 64
    _reconfigure(det, 0.25, max_candidates=4)       # (the capacity is rounded up to 64 rows)
    det.detect_async(frame)
    with pytest.raises(_lib.FastMOTHipError, match=r'error -3: .*overflow'):        # (FM_ERR_STATE)
        det.postprocess()
    _reconfigure(det, 0.25)
    assert len(det(frame)) > 0


def test_mot_step_with_a_v8_detector(ctx, tmp_path):
    from types import SimpleNamespace
    import scenes
    from fastmot_amd import MOT
    from synthetic import SyntheticVideo
    size = (320, 180)
    video = SyntheticVideo(size, n_ids=4, n_frames=6, seed=2)
    name = _register(tmp_path, R.tiny(nc=1, cls_bias=-2.0), IN_HW, True)
    mot = MOT(size, detector_type='YOLO', detector_frame_skip=2, class_ids=(0,),
              yolo_detector_cfg=SimpleNamespace(model=name, conf_thresh=0.25, nms_thresh=0.5, max_area=800000, min_aspect_ratio=0.0),
              feature_extractor_cfgs=(SimpleNamespace(model='OSNet025', batch_size=16),),
              tracker_cfg=SimpleNamespace(**scenes.tracker_kwargs()))
    assert mot.detector.model.HEAD == 'dfl'
    mot.reset(1 / 30.)
    for f in range(video.n_frames):
        mot.step(video.frames[f])
        assert mot.frame_count == f + 1


def test_v8n_640_every_layer_under_the_bound(ctx, tmp_path):
    import layer_check
    from fastmot_amd.engine import NET_DETECTOR
    from fastmot_amd.models.onnx_detector import lower
    g, info = lower(R.export(R.yolov8n(), (640, 640)))
    assert info.strides == [8, 16, 32] and info.num_classes == 80 and len(g.layers) == 66
    x = np.random.default_rng(1).uniform(0, 1, (1, 640, 640, 3)).astype(np.float16)
    ratios = layer_check.run_and_check(ctx, NET_DETECTOR, g, 1, x, 'YOLOv8n_640')
    assert ratios and max(ratios.values()) <= 1.0
