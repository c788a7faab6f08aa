"""GPU: the SSD detector's device stages (ssd.hip) and SSDDetector / MOT on top of them.

  * preprocess: fm_ssd_preprocess_only == SSDDetector.normalize(resize_bgr(frame, region), tiles) rounded to fp16, bit for bit.
  * decode: boxes and scores of fm_ssd_postprocess_host_heads against the float64 reference (tests/ssd_ref.py).  The only
    inexact operations on the device are __expf and the reciprocal of the sigmoid; DECODE_TOL below is 4 x the largest
    difference measured against that reference on this test's inputs (test_decode prints the figure).
  * NMS / top-K: host heads on which the reference's decisions are clear cut (asserted): labels and order exact.
  * the back end off its defaults (test_backend_*): equal scores, anchor counts around powers of two and at the 4096 limit,
    topk 1 .. 256, 2 and 256 classes, 16 tiles, nms_thresh 0 and 1, an empty tile, zero-area boxes, the configurations
    fm_ssd_configure refuses -- the same reference, labels and order exact, worst differences printed (SSDBOUND).
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


# ------------------------------------------------------------------------------------------- the back end off its defaults
# Inputs on which the float64 reference and the float32 device must agree: class logits are multiples of 0.5 in [-8, 8], so
# equal scores come from equal logits alone (asserted: distinct scores differ by more than 1e-6; beyond +-12 float32's
# sigmoid would saturate where float64 still orders); boxes are random and pairwise distinct, so a row's box identifies
# its anchor (asserted); where suppression is active no compared IoU lies within 1e-4 of the threshold (asserted).
_made = [0]


def _model(shapes, per_cell, n_classes, topk=64, thresh=1.0, seed=5):
    """A model in the pattern of _Small: feature maps `shapes`, per_cell[k] anchors in every cell of map k, random anchors."""
    n = sum(h * w * a for (h, w), a in zip(shapes, per_cell))
    rng = np.random.default_rng(seed)
    table = np.concatenate([rng.uniform(0.1, 0.9, (n, 2)), rng.uniform(0.05, 0.6, (n, 2))], 1).astype(np.float32)
    _made[0] += 1
    return type(f'_Back{_made[0]}', (_Small,), dict(
        NUM_CLASSES=n_classes, TOPK=topk, NMS_THRESH=thresh, SHAPES=list(shapes), PER_CELL=list(per_cell), N_ANCHORS=n,
        anchors_per_cell=classmethod(lambda cls, k: cls.PER_CELL[k]), anchors=classmethod(lambda cls: table)))


def _half_step_heads(model, n_tiles, seed, loc_sigma=3.0, levels=33):
    """Random boxes; class logits drawn from `levels` multiples of 0.5 centred on 0 (33: the whole of [-8, 8])."""
    rng = np.random.default_rng(seed)
    heads = _random_heads(model, n_tiles, rng, loc_sigma)
    for k, hd in enumerate(heads):
        a = model.anchors_per_cell(k)
        hd[:, :, a * 4:] = rng.integers(0, levels, hd[:, :, a * 4:].shape) * 0.5 - (levels - 1) * 0.25
    return heads


def _logit_view(model, heads, k):
    """[n_tiles, cells, anchors of a cell, classes] view of the class logits of head k."""
    a = model.anchors_per_cell(k)
    return heads[k][:, :, a * 4:].reshape(heads[k].shape[0], heads[k].shape[1], a, model.NUM_CLASSES)


def _loc_view(model, heads, k):
    a = model.anchors_per_cell(k)
    return heads[k][:, :, :a * 4].reshape(heads[k].shape[0], heads[k].shape[1], a, 4)


def _reference(model, heads, topk, thresh):
    """ssd_ref.postprocess plus the assertions that make its decisions the device's: -> (rows, anchors, stats, scores)"""
    per_cell = [model.anchors_per_cell(k) for k in range(len(heads))]
    boxes, scores = ssd_ref.decode(*ssd_ref.split_heads(heads, per_cell, model.NUM_CLASSES), model.anchors(), model.BOX_SCALES)
    stats = {}
    ref, which = ssd_ref.nms_topk(boxes, scores, topk, thresh, stats)
    fg = np.unique(scores[..., 1:][scores[..., 1:] > 1e-8])
    assert len(fg) < 2 or np.diff(fg).min() > 1e-6                       # distinct scores are distinct in float32 too
    assert not ((scores[..., 1:] > 1e-9) & (scores[..., 1:] < 1e-7)).any()         # (nothing at the score floor)
    ious = stats['ious']
    if thresh >= 1.0:
        assert (ious < 1 - 1e-4).all()                                   # nothing suppresses
    elif thresh > 0.0:
        assert len(ious) and np.abs(ious - thresh).min() > 1e-4
    # every returned row's box belongs to one anchor of its tile alone
    n_tiles = scores.shape[0]
    for r in np.flatnonzero(which >= 0):
        t = r // topk
        near = (np.abs(boxes[t] - ref[r, 3:]).max(1) < 1e-5).sum()
        assert near == 1, (r, near)
    return ref, which, stats, scores, boxes


def _run_and_compare(ctx, model, heads, n_tiles, topk=None, thresh=None, label=''):
    topk = model.TOPK if topk is None else topk
    thresh = model.NMS_THRESH if thresh is None else thresh
    ref, which, stats, scores, boxes = _reference(model, heads, topk, thresh)
    _configure(ctx, model, n_tiles, topk, thresh)
    rows = ctx.ssd_postprocess_host_heads(heads)
    assert rows.shape == ref.shape == (n_tiles * topk, 7)
    assert np.array_equal(rows[:, :2], ref[:, :2]), label                # tiles, labels, order
    diff = np.abs(rows[:, 2:].astype(np.float64) - ref[:, 2:])
    print(f'SSDBOUND {label:30s} {int((which >= 0).sum()):5d} rows, max |device - float64| score {diff[:, 0].max():.3g}, '
          f'box {diff[:, 1:].max():.3g} (DECODE_TOL {DECODE_TOL:.3g})')
    assert diff.max() <= DECODE_TOL, label                               # (the box identifies the anchor: _reference)
    pad = ref[:, 1] == -1
    assert np.array_equal(rows[pad], ref[pad].astype(np.float32))         # padding rows exactly (tile, -1, 0, 0, 0, 0, 0)
    return ref, which, stats, scores, boxes


def _repeated_share(scores):
    fg = scores[..., 1:].reshape(scores.shape[0], -1)
    rep = tot = 0
    for row in fg:
        _, counts = np.unique(row, return_counts=True)
        rep, tot = rep + counts[counts > 1].sum(), tot + row.size
    return rep / tot


def test_backend_equal_scores(ctx):
    """24 anchors, 3 classes, 2 tiles, logits from nine levels: most foreground scores of a tile repeat, within a class (the
    anchor half of the sort key decides) and across classes (the (class, anchor) half of the top-K key decides)."""
    model = _model([(3, 2), (1, 1)], [3, 6], 3, topk=64)
    heads = _half_step_heads(model, 2, seed=11, levels=9)
    for thresh in (1.0, 0.5):
        ref, which, stats, scores, _ = _run_and_compare(ctx, model, heads, 2, thresh=thresh, label=f'ties thresh {thresh}')
        assert _repeated_share(scores) >= 1 / 3
        got = ref[which >= 0]
        same = (np.diff(got[:, 2]) == 0) & (np.diff(got[:, 0]) == 0)
        assert (same & (np.diff(got[:, 1]) != 0)).any() and (same & (np.diff(got[:, 1]) == 0)).any()   # both halves decided
    assert (ref[:, 1] == -1).any() and len(stats['ious'])                # (at 0.5 something was suppressed)


ANCHOR_LAYOUTS = {1: ([(1, 1)], [1]), 2: ([(1, 1)], [2]), 3: ([(1, 1)], [3]), 255: ([(5, 1)], [51]), 256: ([(2, 2)], [64]),
                  257: ([(2, 2), (1, 1)], [64, 1]), 4096: ([(8, 8)], [64])}


@pytest.mark.parametrize('n_anchors', sorted(ANCHOR_LAYOUTS))
def test_backend_anchor_counts(ctx, n_anchors):
    """Anchor counts at and next to a power of two (the zero keys that pad the bitonic sort to np2), one anchor, the 4096
    that fill the 32 KB of LDS; topk 1, 64 and 256, below and above the anchor count (zero keys among the first K)."""
    shapes, per_cell = ANCHOR_LAYOUTS[n_anchors]
    model = _model(shapes, per_cell, 2, seed=n_anchors)
    assert model.N_ANCHORS == n_anchors and max(per_cell) <= 64
    heads = _half_step_heads(model, 1, seed=n_anchors)
    for topk in (1, 64, 256):
        ref, which, _, scores, _ = _run_and_compare(ctx, model, heads, 1, topk=topk, label=f'{n_anchors} anchors topk {topk}')
        assert (which >= 0).sum() == min(topk, n_anchors)                # (every score is above the floor)
        if n_anchors >= 255:
            assert _repeated_share(scores) >= 1 / 3


@pytest.mark.parametrize('n_classes', [2, 256])
def test_backend_class_counts(ctx, n_classes):
    """2 and 256 classes at 24 anchors: one list and 255 lists under the 256-thread reduction of ssd_topk_kernel."""
    model = _model([(3, 2), (1, 1)], [3, 6], n_classes, topk=64)
    heads = _half_step_heads(model, 1, seed=n_classes)
    top = [(255, 2), (255, 0), (254, 1), (129, 1), (128, 0), (1, 1)]         # (class, anchor of the first cell)
    if n_classes == 256:            # the highest score in the last threads of the reduction and on both sides of its halves
        for k in range(len(heads)):
            np.minimum(_logit_view(model, heads, k), 7.5, out=_logit_view(model, heads, k))
        for c, a in top:
            _logit_view(model, heads, 0)[0, 0, a, c] = 8.0
    ref, which, _, _, _ = _run_and_compare(ctx, model, heads, 1, thresh=1.0, label=f'{n_classes} classes')
    assert (which >= 0).sum() == min(64, 24 * (n_classes - 1))
    if n_classes == 256:
        assert [(int(r[1]), int(a)) for r, a in zip(ref[:6], which[:6])] == sorted(top)
        assert len(np.unique(ref[:, 1])) > 20


def test_backend_sixteen_tiles(ctx):
    model = _model([(3, 2), (1, 1)], [3, 6], 3, topk=20)
    heads = _half_step_heads(model, 16, seed=16)
    assert all(not np.array_equal(h[0], h[t]) for h in heads for t in range(1, 16))         # different heads per tile
    ref, which, _, _, _ = _run_and_compare(ctx, model, heads, 16, thresh=1.0, label='16 tiles')
    assert np.array_equal(ref[:, 0], np.repeat(np.arange(16), 20)) and (which >= 0).all()


@pytest.mark.parametrize('thresh', [0.0, 1.0])
def test_backend_threshold_extremes(ctx, thresh):
    """nms_thresh 0: any overlap suppresses (asserted on the reference: every pair of boxes either overlaps by more than
    1e-4 of IoU and 1e-5 in both axes or is apart by more than 1e-5 in one); nms_thresh 1: nothing does."""
    model = _model([(3, 2), (1, 1)], [3, 6], 3, topk=64)
    heads = _half_step_heads(model, 2, seed=23, loc_sigma=1.0)
    ref, which, stats, _, boxes = _run_and_compare(ctx, model, heads, 2, thresh=thresh, label=f'nms_thresh {thresh}')
    if thresh == 1.0:
        assert (which >= 0).sum() == 2 * 24 * 2
        return
    for b in boxes:
        i, j = np.triu_indices(len(b), 1)
        iw = np.minimum(b[i, 2], b[j, 2]) - np.maximum(b[i, 0], b[j, 0])
        ih = np.minimum(b[i, 3], b[j, 3]) - np.maximum(b[i, 1], b[j, 1])
        iou = np.array([ssd_ref.iou(b[p], b[q]) for p, q in zip(i, j)])
        assert (((iw > 1e-5) & (ih > 1e-5) & (iou > 1e-4)) | (iw < -1e-5) | (ih < -1e-5)).all()
        assert ((iw > 0) & (ih > 0)).any() and ((iw < 0) | (ih < 0)).any()
    assert 0 < (which >= 0).sum() < 2 * 24 * 2 and (stats['ious'] > 0).any() and (stats['ious'] == 0).any()


def test_backend_empty_tile_and_zero_area_boxes(ctx):
    """Tile 1 holds -30 everywhere: nothing exceeds 1e-8, the tile is padding rows only.  In tiles 0 and 2 four anchors are
    shifted out of the image by forty anchor heights: their boxes clip to zero area (exactly, ymin = ymax = 1), carry the
    highest scores, and neither suppress nor are suppressed at nms_thresh 0."""
    model = _model([(3, 2), (1, 1)], [3, 6], 3, topk=64)
    heads = _half_step_heads(model, 3, seed=31, loc_sigma=1.0)
    _loc_view(model, heads, 0)[:, :4, 0, 0] = 400.0                      # ty / 10 = 40 anchor heights (>= 0.05 each) down
    _logit_view(model, heads, 0)[:, :4, 0, 1] = 8.0
    for k in range(len(heads)):
        _logit_view(model, heads, k)[1] = -30.0
    ref, which, stats, scores, boxes = _run_and_compare(ctx, model, heads, 3, thresh=0.0, label='empty tile, zero area')
    flat = [0, 3, 6, 9]                                                  # anchor 0 of cells 0 .. 3 of the first map
    for t in (0, 2):
        assert (boxes[t, flat, 1] == 1).all() and (boxes[t, flat, 3] == 1).all()
        got = which[t * 64:(t + 1) * 64]
        assert np.isin(flat, got[ref[t * 64:(t + 1) * 64, 1] == 1]).all()        # all four came back for class 1
        assert (ref[t * 64:t * 64 + 4, 2] > 0.9996).all()
    assert np.array_equal(ref[64:128], np.tile([1., -1, 0, 0, 0, 0, 0], (64, 1)))
    assert (which[64:128] == -1).all()


def _raw_cfg(model, n_tiles, topk, n_classes=None, per_cell=None, tile_xy=(0, 0), n_rows=None):
    """An fm_ssd_cfg filled as Context.ssd_configure fills it, with the fields a refusal needs overridden."""
    from fastmot_amd import _lib
    cfg = _lib.SsdCfg()
    shapes = model.feature_map_shapes()
    per_cell = [model.anchors_per_cell(k) for k in range(len(shapes))] if per_cell is None else per_cell
    n = sum(h * w * a for (h, w), a in zip(shapes, per_cell))
    rng = np.random.default_rng(0)
    table = np.ascontiguousarray(np.concatenate([rng.uniform(0.1, 0.9, (n, 2)), rng.uniform(0.05, 0.6, (n, 2))], 1), np.float32)
    cfg.input_tensor, cfg.in_w, cfg.in_h, cfg.n_heads = 0, 128, 160, len(shapes)
    for k, ((h, w), a) in enumerate(zip(shapes, per_cell)):
        cfg.head_tensor[k], cfg.map_w[k], cfg.map_h[k], cfg.n_anchors[k] = -1, w, h, a
    cfg.anchors, cfg.n_anchor_rows = table.ctypes.data, n if n_rows is None else n_rows
    cfg.box_scales[:] = [10., 10., 5., 5.]
    cfg.num_classes, cfg.topk, cfg.nms_thresh = model.NUM_CLASSES if n_classes is None else n_classes, topk, 0.5
    cfg.n_tiles = n_tiles
    for t in range(min(n_tiles, _lib.FM_MAX_SSD_TILES)):
        cfg.tile_x[t], cfg.tile_y[t] = tile_xy
    cfg.region_w, cfg.region_h = 128, 160
    return cfg, table


def test_backend_refusals(ctx):
    """What the kernels' LDS arrays and index fields cannot hold is refused by fm_ssd_configure on the host, before any
    launch, with the bad-argument error -- and the context is left without an SSD state: a caller that goes on after the
    error cannot launch with the configuration it tried to replace."""
    import ctypes as C
    from fastmot_amd import _lib
    small = _model([(3, 2), (1, 1)], [3, 6], 3)
    cases = {
        '4097 anchors': _raw_cfg(_model([(8, 8), (1, 1)], [64, 1], 2), 1, 64),
        'topk 0': _raw_cfg(small, 1, 0),
        'topk 257': _raw_cfg(small, 1, 257),
        '1 class': _raw_cfg(small, 1, 64, n_classes=1),
        '257 classes': _raw_cfg(small, 1, 64, n_classes=257),
        '17 tiles': _raw_cfg(small, 17, 64),
        '65 anchors per cell': _raw_cfg(_model([(1, 1)], [65], 2), 1, 64),
        'a tile outside the region': _raw_cfg(small, 2, 64, tile_xy=(1, 0)),
    }
    heads = _half_step_heads(small, 1, seed=1)
    for what, (cfg, table) in cases.items():
        _configure(ctx, small, 1)                                        # a valid state first
        assert ctx.ssd_postprocess_host_heads(heads).shape == (64, 7)
        assert ctx.lib.fm_ssd_configure(ctx._ctx, C.byref(cfg)) == -2, what          # FM_ERR_ARG
        with pytest.raises(_lib.FastMOTHipError, match=r'error -2: .*bad argument.*ssd'):
            ctx.ssd_postprocess_host_heads(heads)                        # no state: refused, nothing launched
    _configure(ctx, small, 1)
    assert ctx.ssd_postprocess_host_heads(heads).shape == (64, 7)


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
