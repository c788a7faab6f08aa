"""GPU: the SSD detector's device stages (ssd.hip) and SSDDetector / MOT on top of them.

  * preprocess: fm_ssd_preprocess_only == SSDDetector.normalize(resize_bgr(frame, region), tiles) rounded to fp16, bit for bit.
  * decode: boxes and scores of fm_ssd_postprocess_host_heads against the float64 reference (tests/ssd_ref.py).  The only
    inexact operations on the device are __expf and the reciprocal of the sigmoid; DECODE_TOL below is 4 x the largest
    difference measured against that reference on this test's inputs (test_decode prints the figure).
  * NMS / top-K: host heads on which the reference's decisions are clear cut (asserted): labels and order exact.
  * end to end: SSDDetector on the device == SSDDetector around the numpy post-process of the device's own head tensors."""
from types import SimpleNamespace

import numpy as np
import pytest

import ssd_ref
from fastmot_amd import NV12Frame, SourceFrame
from fastmot_amd.detector import SSDDetector, bind_frame
from fastmot_amd.models.graph import RandomWeights
from fastmot_amd.utils.nv12 import nv12_to_bgr
from fastmot_amd.videoio import resize_bgr
from test_ssd_topology import TinySSD

pytestmark = pytest.mark.gpu

# 4 x the largest |device - float64 reference| over the scores and boxes of test_decode's inputs: measured 8.25e-8 on the
# scores and 8.61e-8 on the boxes (both lie in [0, 1], where one fp32 ulp is 6e-8: __expf and v_rcp_f32 are good to about an
# ulp each, and the corner is one more rounded add)
DECODE_TOL = 3.5e-7


@pytest.mark.parametrize('size,grid', [((320, 180), (2, 1)), ((320, 180), (2, 2)), ((320, 180), (3, 1)),
                                       ((448, 320), (2, 1)),          # the region is 224 x 160: an exact 2x decimation
                                       ((321, 179), (2, 2))])         # odd frame size
def test_preprocess(ctx, size, grid):
    det = SSDDetector(size, (1,), model='TinySSD', tiling_grid=grid, weights=RandomWeights(seed=1))
    if size == (448, 320):
        assert det.tiling_region_sz == (224, 160)
    frame = np.random.default_rng(size[0] + grid[1]).integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)
    bind_frame(ctx, frame, size)
    ctx.ssd_preprocess_only()
    got = det.net.read(det.graph.input, det.batch_size)                   # [n, H, W, 3] (fp16 values)
    want = np.empty((det.batch_size, *TinySSD.INPUT_SHAPE), np.float32)
    SSDDetector.normalize(resize_bgr(frame, det.tiling_region_sz), det.tiles, want)
    assert np.array_equal(got, want.astype(np.float16).astype(np.float32).transpose(0, 2, 3, 1))
    det.net.close()


class _Small(TinySSD):
    """24 anchors, 2 foreground classes: with topk 64 and no suppression every (anchor, class) comes back."""
    NUM_CLASSES = 3
    TOPK = 64
    NMS_THRESH = 1.0
    SHAPES = [(3, 2), (1, 1)]

    @classmethod
    def feature_map_shapes(cls):
        return cls.SHAPES

    @classmethod
    def anchors(cls):
        rng = np.random.default_rng(5)
        return np.concatenate([rng.uniform(0.1, 0.9, (24, 2)), rng.uniform(0.05, 0.6, (24, 2))], 1).astype(np.float32)


def _configure(ctx, model, n_tiles, topk=None, thresh=None):
    shapes = model.feature_map_shapes()
    ctx.ssd_configure(shapes, [model.anchors_per_cell(k) for k in range(len(shapes))], model.anchors(), model.BOX_SCALES,
                      model.NUM_CLASSES, model.TOPK if topk is None else topk, model.NMS_THRESH if thresh is None else thresh,
                      [(0, 0)] * n_tiles, model.INPUT_SHAPE[:0:-1], model.INPUT_SHAPE[:0:-1])


def _random_heads(model, n_tiles, rng, loc_sigma):
    heads = []
    for k, (h, w) in enumerate(model.feature_map_shapes()):
        a = model.anchors_per_cell(k)
        hd = np.empty((n_tiles, h * w, a * (4 + model.NUM_CLASSES)), np.float32)
        hd[:, :, :a * 4] = rng.normal(0, loc_sigma, (n_tiles, h * w, a * 4))
        hd[:, :, a * 4:] = rng.normal(0, 3, (n_tiles, h * w, a * model.NUM_CLASSES))
        heads.append(hd)
    return heads


def test_decode(ctx):
    rng = np.random.default_rng(21)
    heads = _random_heads(_Small, 2, rng, loc_sigma=6.0)            # (sigma 6 / scales 10, 5: shifts and sizes that also clip)
    _configure(ctx, _Small, 2)
    rows = ctx.ssd_postprocess_host_heads(heads)
    ref, which = ssd_ref.postprocess(heads, _Small)
    assert rows.shape == ref.shape == (2 * 64, 7)
    assert (which >= 0).sum() == 2 * 24 * 2                           # everything came back
    scores = np.sort(ref[which >= 0, 2])
    assert np.diff(scores).min() > 1e-6                               # the order is decided
    assert np.array_equal(rows[:, :2], ref[:, :2])                    # tile, label -- and with them the order
    diff = np.abs(rows[:, 2:].astype(np.float64) - ref[:, 2:])
    inner = ((ref[:, 3:] > 0) & (ref[:, 3:] < 1))[which >= 0]
    print(f'decode: max |device - float64| score {diff[:, 0].max():.3g}, box {diff[:, 1:].max():.3g}; '
          f'{int(inner.sum())} of {inner.size} coordinates unclipped')
    assert inner.sum() > inner.size // 4 and (~inner).sum() > 8
    assert diff.max() <= DECODE_TOL


def _clear_cut_heads(model, n_tiles, seed):
    """Random boxes; scores a random permutation of an even grid in (0, 1) (pairwise distinct by > 1e-4); the last tile sparse."""
    rng = np.random.default_rng(seed)
    heads = _random_heads(model, n_tiles, rng, loc_sigma=3.0)
    n_fg = sum(h.shape[1] * model.anchors_per_cell(k) for k, h in enumerate(heads)) * (model.NUM_CLASSES - 1) * n_tiles
    grid = rng.permutation(n_fg)
    pos = 0
    for k, hd in enumerate(heads):
        a = model.anchors_per_cell(k)
        cls = hd[:, :, a * 4:].reshape(n_tiles, hd.shape[1], a, model.NUM_CLASSES)
        m = cls[..., 1:].size
        s = (grid[pos:pos + m].reshape(cls[..., 1:].shape) + 1.0) / (n_fg + 1.0)
        pos += m
        cls[..., 1:] = np.log(s / (1 - s))
        cls[-1][rng.random(cls[-1].shape) < 0.99] = -30.0             # the last tile: hardly any score above 1e-8
    return heads


def test_nms_and_topk(ctx):
    model, n_tiles = TinySSD, 3
    heads = _clear_cut_heads(model, n_tiles, seed=4)
    stats = {}
    ref, which = ssd_ref.postprocess(heads, model, stats=stats)
    # the reference's decisions are clear cut, and both truncations happen
    assert np.abs(stats['ious'] - model.NMS_THRESH).min() > 1e-4
    fg = np.concatenate([ssd_ref.decode(*ssd_ref.split_heads(heads, [3, 6, 6, 6, 6, 6], model.NUM_CLASSES), model.anchors(),
                                        model.BOX_SCALES)[1][..., 1:].reshape(-1)])
    fg = np.sort(fg[fg > 1e-8])
    assert np.diff(fg).min() > 1e-6
    assert stats['max_candidates'] > model.TOPK and stats['max_survivors'] > model.TOPK
    assert (ref[:, 1] == -1).sum() >= 5 and (ref[:model.TOPK, 1] >= 1).all()       # padding rows in the sparse tile only
    _configure(ctx, model, n_tiles)
    rows = ctx.ssd_postprocess_host_heads(heads)
    assert np.array_equal(rows[:, :2], ref[:, :2])                    # tiles, labels, order
    assert np.abs(rows[:, 2:].astype(np.float64) - ref[:, 2:]).max() <= DECODE_TOL
    pad = ref[:, 1] == -1
    assert np.array_equal(rows[pad], ref[pad].astype(np.float32))     # padding rows exactly (tile, -1, 0, 0, 0, 0, 0)


def _same(a, b):
    assert len(a) == len(b) and np.array_equal(a.label, b.label) and np.array_equal(a.tlbr, b.tlbr)
    assert np.abs(a.conf - b.conf).max(initial=0) <= DECODE_TOL


def _frame(size, seed):
    return np.random.default_rng(seed).integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)


def test_detector_equals_numpy_postprocess_of_its_own_heads(ctx):
    size, kw = (320, 180), dict(model='TinySSD', tiling_grid=(2, 1), conf_thresh=0.3)
    dev = SSDDetector(size, (1, 2, 3, 4), weights=RandomWeights(seed=7), **kw)
    frame = _frame(size, 1)
    out = dev(frame)
    assert len(out) > 0
    heads = [dev.net.read(v, dev.batch_size).reshape(dev.batch_size, v.h * v.w, v.c) for v in dev.heads]

    def ref(batch):
        assert batch.shape == (2, 3, 160, 128)
        return ssd_ref.postprocess(heads, TinySSD)[0].astype(np.float32)
    host = SSDDetector(size, (1, 2, 3, 4), backend=ref, **kw)
    _same(out, host(frame))
    with pytest.raises(AssertionError):
        dev.postprocess()                                             # nothing in flight
    # a SourceFrame(NV12Frame) at capture resolution gives the detections of the converted, resized ndarray
    rng = np.random.default_rng(2)
    surface = rng.integers(0, 256, (360 + 180, 640), dtype=np.uint8)
    y, uv = surface[:360], surface[360:]
    _same(dev(SourceFrame(NV12Frame(y, uv))), dev(resize_bgr(nv12_to_bgr(y, uv), size)))
    dev.net.close()


def test_default_model_still_raises():
    with pytest.raises(NotImplementedError):
        SSDDetector((1920, 1080), (1,))


def test_mot_with_the_ssd_detector(ctx):
    import scenes
    from fastmot_amd.mot import MOT
    from synthetic import SyntheticVideo
    size = (320, 180)
    video = SyntheticVideo(size, n_ids=4, n_frames=5, seed=3)
    mot = MOT(size, detector_type='SSD', detector_frame_skip=1, class_ids=(1, 2),
              ssd_detector_cfg=SimpleNamespace(model='TinySSD', tiling_grid=(2, 1), conf_thresh=0.3, weights=RandomWeights(seed=7)),
              feature_extractor_cfgs=(SimpleNamespace(model='OSNet025', batch_size=16), SimpleNamespace(model='OSNet025', batch_size=16)),
              tracker_cfg=SimpleNamespace(**scenes.tracker_kwargs()))
    assert isinstance(mot.detector, SSDDetector) and mot.detector.backend is None
    mot.reset(1 / 30.)
    for f in range(video.n_frames):
        mot.step(video.frames[f])
    assert mot.frame_count == 5
    list(mot.visible_tracks())
