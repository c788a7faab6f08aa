"""CPU: the host side of tiled YOLO detection (YOLODetector(tiling_grid=...)).
  * geometry: the tile rectangles / tiling region of the helper both detectors call (detector.generate_tiles) for the
    three cases worked out by hand, equal to SSDDetector._generate_tiles for the same grid and overlap, and the box
    transform handed to the decode
  * merge: the library's fm_detect_merge_tiles == SSDDetector.merge_dets (the restated reference, pinned by
    reference-generated goldens in test_ssd_detector.py) on seeded cases, exactly, as row sets per class
  * errors: a grid of more tiles than a pass takes, tiling with max_batch > 1 and tiling with a detector look-ahead
    raise ValueError before any device call
No detector is constructed here: that needs the device (tests/test_tiled_detect_gpu.py)."""
from types import SimpleNamespace

import numpy as np
import pytest

from fastmot_amd import _lib
from fastmot_amd.detector import SSDDetector, YOLODetector, generate_tiles, tile_box_transforms, check_tiling
from fastmot_amd.models import SSD

TILE_WH = (128, 96)          # TinyYOLO's input (tests/test_detect_gpu.py)
FRAME = (320, 180)


# ---------------------------------------------------------------------------------------- geometry
GEOMETRY = [
    ((2, 1), 0.25, (224, 96), [(0, 0), (96, 0)]),
    ((2, 2), 0.25, (224, 168), [(0, 0), (96, 0), (0, 72), (96, 72)]),
    ((3, 1), 0.3, (307, 96), [(0, 0), (90, 0), (179, 0)]),
]


class _TileSSD(SSD):
    """An SSD model description with the tile size of the tests (no network: SSDDetector gets a backend)."""
    INPUT_SHAPE = (3, TILE_WH[1], TILE_WH[0])
    NUM_CLASSES = 3
    TOPK = 10


@pytest.mark.parametrize('grid,overlap,region,origins', GEOMETRY)
def test_geometry(grid, overlap, region, origins):
    tiles, reg = generate_tiles(TILE_WH, grid, overlap)
    assert tuple(int(v) for v in reg) == region
    assert [tuple(int(v) for v in t[:2]) for t in tiles] == origins
    np.testing.assert_array_equal(tiles[:, 2:] - tiles[:, :2], np.tile(np.array(TILE_WH) - 1., (len(tiles), 1)))
    # the function SSDDetector calls is this helper, and its results did not move
    ssd = SSDDetector(FRAME, (1,), model='_TileSSD', tile_overlap=overlap, tiling_grid=grid, backend=lambda b: None)
    np.testing.assert_array_equal(ssd.tiles, tiles)
    assert tuple(ssd.tiling_region_sz) == tuple(reg)
    # every tile lies inside the region (the kernels resize the frame to the region and read tile pixels from it)
    assert (tiles[:, 2] < reg[0]).all() and (tiles[:, 3] < reg[1]).all() and (tiles[:, :2] >= 0).all()


@pytest.mark.parametrize('grid,overlap,region,origins', GEOMETRY)
def test_box_transform(grid, overlap, region, origins):
    """A box in fractions of tile t, through the decode's `* upscaled_sz - offset`, lands where the tile lies in the frame."""
    tiles, reg = generate_tiles(TILE_WH, grid, overlap)
    size, offsets = tile_box_transforms(FRAME, TILE_WH, tiles, reg)
    scale = np.array(FRAME, float) / np.array(reg, float)
    np.testing.assert_array_equal(size, np.array(TILE_WH, float) * scale)
    for t, off in zip(tiles, offsets):
        np.testing.assert_array_equal(np.zeros(2) * size - off, t[:2] * scale)                  # the tile's corner
        np.testing.assert_allclose(np.ones(2) * size - off, (t[:2] + TILE_WH) * scale, rtol=1e-15)


# ---------------------------------------------------------------------------------------- merge
def tiled_detections(grid, overlap, seed, n_boxes=24, classes=(0, 1)):
    """Objects of a 320 x 180 frame as the tiles of `grid` would report them: every box clipped to every tile (scaled to
    the frame) that keeps at least 6 pixels of it in each direction, each edge jittered by -1..1, a random confidence;
    tile-major, like the union of the per-tile detections of a tiled pass."""
    rng = np.random.default_rng(seed)
    tiles, reg = generate_tiles(TILE_WH, grid, overlap)
    scale = np.array(FRAME, float) / np.array(reg, float)
    w, h = rng.integers(12, 60, n_boxes), rng.integers(20, 90, n_boxes)
    x, y = rng.integers(0, FRAME[0] - w), rng.integers(0, FRAME[1] - h)
    label = rng.choice(classes, n_boxes)
    rows, ids = [], []
    for ti, t in enumerate(tiles):
        tx0, ty0 = np.rint(t[:2] * scale)
        tx1, ty1 = np.rint((t[2:] + 1) * scale) - 1
        for b in range(n_boxes):
            x0, y0, x1, y1 = max(x[b], tx0), max(y[b], ty0), min(x[b] + w[b] - 1, tx1), min(y[b] + h[b] - 1, ty1)
            if x1 - x0 + 1 < 6 or y1 - y0 + 1 < 6:
                continue
            tlbr = np.array([x0, y0, x1, y1], float) + rng.integers(-1, 2, 4)
            rows.append((tlbr, label[b], rng.uniform(0.3, 1.0)))
            ids.append(ti)
    dets = np.array(rows, _lib.DET_DTYPE).view(np.recarray) if rows else np.zeros(0, _lib.DET_DTYPE).view(np.recarray)
    return dets, np.array(ids, int), len(tiles)


def row_set(dets):
    """Rows ordered by (label, tlbr, conf): the comparison of two merges is one of row sets per class."""
    d = np.asarray(dets)
    keys = (d['conf'], d['tlbr'][:, 3], d['tlbr'][:, 2], d['tlbr'][:, 1], d['tlbr'][:, 0], d['label'])
    return d[np.lexsort(keys)] if len(d) else d


def assert_same_merge(dets, ids, n_tiles, thresh):
    want = SSDDetector.merge_dets(dets, ids, n_tiles, thresh)
    got = _lib.merge_tiles(dets, ids, n_tiles, thresh)
    a, b = row_set(got), row_set(want)
    assert len(a) == len(b)
    np.testing.assert_array_equal(a['tlbr'], b['tlbr'])
    np.testing.assert_array_equal(a['label'], b['label'])
    np.testing.assert_array_equal(a['conf'], b['conf'])
    assert (np.diff(got.label) >= 0).all()                      # ordered by class
    return got


# rows in -> rows out of the generator above for seeds 0..7, pinned so that it cannot change silently (its draw order is
# this file's own: the counts lie in the ranges of the feature's description, 45-54 -> 20-27 and 25-33 -> 23-24, or next
# to them)
MERGE_COUNTS = {
    (2, 2): [(50, 26), (54, 28), (56, 26), (51, 24), (59, 23), (46, 24), (53, 22), (50, 23)],
    (2, 1): [(31, 24), (32, 24), (32, 24), (31, 24), (34, 23), (29, 24), (32, 24), (31, 23)],
}


@pytest.mark.parametrize('grid', [(2, 2), (2, 1)])
@pytest.mark.parametrize('seed', range(8))
def test_merge_equals_reference_restatement(grid, seed):
    dets, ids, n_tiles = tiled_detections(grid, 0.25, seed)
    got = assert_same_merge(dets, ids, n_tiles, 0.6)
    assert len(got) < len(dets)                                 # at least one group was merged
    assert (len(dets), len(got)) == MERGE_COUNTS[grid][seed]


def test_merge_keeps_the_set_order_inside_a_class():
    """Inside a class the survivors keep the iteration order of the reference's set (the library sorts by class with a
    stable sort).  The oracle's `argsort` is stable only where NumPy sorts by insertion, up to 16 rows: a case that small
    is compared in order, row by row."""
    dets, ids, n_tiles = tiled_detections((2, 2), 0.25, 3, n_boxes=6)
    want = SSDDetector.merge_dets(dets, ids, n_tiles, 0.6)
    assert 2 <= len(want) <= 16 and len(want) < len(dets) and len(set(want.label)) == 2
    got = _lib.merge_tiles(dets, ids, n_tiles, 0.6)
    np.testing.assert_array_equal(got.tlbr, want.tlbr)
    np.testing.assert_array_equal(got.label, want.label)
    np.testing.assert_array_equal(got.conf, want.conf)


def test_merge_edge_cases():
    none = np.zeros(0, _lib.DET_DTYPE).view(np.recarray)
    assert len(_lib.merge_tiles(none, np.zeros(0, int), 4, 0.6)) == 0
    dets, ids, n_tiles = tiled_detections((2, 2), 0.25, 1)
    one = assert_same_merge(dets[:1], ids[:1], n_tiles, 0.6)
    assert len(one) == 1
    # one class only
    dets, ids, n_tiles = tiled_detections((2, 2), 0.25, 2, classes=(1,))
    got = assert_same_merge(dets, ids, n_tiles, 0.6)
    assert len(got) < len(dets) and set(got.label) == {1}
    # thresholds at the ends of the range
    for thresh in (0., 1.):
        assert_same_merge(dets, ids, n_tiles, thresh)


def test_merge_across_the_set_growth_boundaries():
    """The survivors' order is that of a hash set whose table is sized by the number of rows (16 slots up to 8 rows, 32
    up to 16, 64 up to 32, 128 up to 64, 256 beyond) and shrinks while rows are discarded: row counts on both sides of
    every boundary."""
    seen = set()
    for n_boxes in (2, 3, 4, 6, 8, 12, 16, 24, 32, 40, 48):
        for seed in (11, 12):
            dets, ids, n_tiles = tiled_detections((2, 2), 0.25, seed, n_boxes)
            assert_same_merge(dets, ids, n_tiles, 0.6)
            for cut in (8, 9, 16, 17, 32, 33, 64, 65):          # exactly at and just past each boundary
                if len(dets) >= cut:
                    assert_same_merge(dets[:cut], ids[:cut], n_tiles, 0.6)
                    seen.add(cut)
            seen.add(int(np.searchsorted([8, 16, 32, 64], len(dets))))
    assert {8, 9, 16, 17, 32, 33, 64, 65} <= seen and {0, 1, 2, 3, 4} <= seen


# ---------------------------------------------------------------------------------------- errors
def test_errors_come_before_any_device_call(monkeypatch):
    import fastmot_amd.detector as detector_mod
    from fastmot_amd.mot import MOT

    def no_device(*a, **k):
        raise AssertionError('the configuration check must come before the device context')
    monkeypatch.setattr(detector_mod, 'get_context', no_device)
    with pytest.raises(ValueError, match=str(_lib.FM_MAX_DET_BATCH)):
        YOLODetector(FRAME, (1,), tiling_grid=(4, 2))
    with pytest.raises(ValueError, match='max_batch'):
        YOLODetector(FRAME, (1,), tiling_grid=(2, 1), max_batch=2)
    with pytest.raises(ValueError, match='detector_lookahead'):
        MOT(FRAME, detector_type='YOLO', detector_frame_skip=1, detector_lookahead=2,
            yolo_detector_cfg=SimpleNamespace(tiling_grid=(2, 1)))
    assert check_tiling((1, 1), max_batch=3) == 1 and check_tiling((2, 2)) == 4         # (untiled: nothing to refuse)
