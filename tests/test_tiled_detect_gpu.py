"""GPU: tiled YOLO detection -- YOLODetector(tiling_grid=...) runs the tiles of one frame as the samples of one network pass.
  * tile pixels: the network input of tile t is the frame resized to the tiling region, cut at the tile (preprocess
    kernel against np_oracle.yolo_preprocess; the fused stem paths against the preprocess kernel, head for head)
  * every tile equals a stand-alone untiled detector that is fed the tile's picture and the tile's box transform:
    heads bit for bit, detections exactly
  * the frame's detections are SSDDetector.merge_dets over the per-tile detections
  * passes are collected in order across prefetches; a stale prefetch is dropped; an overflow is reported on its frame
  * MOT.step with the next-frame prefetch == strictly sequential steps; tiling_grid=(1, 1) == no argument
All comparisons are exact: both sides run the same arithmetic."""
from types import SimpleNamespace

import numpy as np
import pytest

import np_oracle as o
from fastmot_amd import _lib
from fastmot_amd.detector import SSDDetector, YOLODetector, generate_tiles
from fastmot_amd.models.graph import RandomWeights
from synthetic import ScriptedHeadWeights, scripted_head_weights
from test_detect_gpu import TinyYOLO, synthetic_frame  # noqa: F401  (registers the tiny model)
from test_tiled_detect_host import row_set

pytestmark = pytest.mark.gpu

SIZE = (320, 180)
TILE_W, TILE_H = 128, 96
GRIDS = [((2, 1), 0.25), ((1, 2), 0.25), ((2, 2), 0.25), ((3, 1), 0.3)]
GRID_IDS = ['2x1', '1x2', '2x2', '3x1']


def _same(a, b):
    assert len(a) == len(b)
    np.testing.assert_array_equal(a.tlbr, b.tlbr)
    np.testing.assert_array_equal(a.label, b.label)
    np.testing.assert_array_equal(a.conf, b.conf)


def _same_rows(a, b):
    a, b = row_set(a), row_set(b)
    assert len(a) == len(b)
    np.testing.assert_array_equal(a['tlbr'], b['tlbr'])
    np.testing.assert_array_equal(a['label'], b['label'])
    np.testing.assert_array_equal(a['conf'], b['conf'])


_SCRIPT = {}


def tile_as_frame(frame, grid, overlap, t=0):
    """The picture tile t of `frame` shows the network, as a BGR frame of the network's input size."""
    tiles, (rw, rh) = generate_tiles((TILE_W, TILE_H), grid, overlap)
    region = np.rint(o.yolo_preprocess(frame, (rh, rw)) * 255)
    x, y = int(tiles[t][0]), int(tiles[t][1])
    return np.ascontiguousarray(region[::-1, y:y + TILE_H, x:x + TILE_W].transpose(1, 2, 0).astype(np.uint8))


def calibrated(frame, target=150):
    """Head weights that let about `target` candidates per TILE through the confidence threshold: calibrated on one
    untiled pass over a tile's picture (what a tiled pass shows the network is less reduced than the whole frame)."""
    return scripted_head_weights((TILE_W, TILE_H), 'TinyYOLO', 1, tile_as_frame(frame, (2, 2), 0.25), target)


def scripted():
    """The suite's scripted heads, so that NMS has candidates in every tile: calibrated once; a fresh weight source with
    the same parameters per detector (a source is consumed by the build)."""
    if 'w' not in _SCRIPT:
        _SCRIPT['w'] = calibrated(synthetic_frame(*SIZE, seed=70))
    w = _SCRIPT['w']
    return ScriptedHeadWeights(0, w.num_classes, w.label, w.obj_bias, w.obj_gain)


def tiled(grid, overlap, weights=None, **kw):
    kw.setdefault('max_candidates', 16384)
    return YOLODetector(SIZE, (0, 1, 2), model='TinyYOLO', conf_thresh=0.25, nms_thresh=0.5,
                        weights=weights if weights is not None else scripted(), tiling_grid=grid, tile_overlap=overlap, **kw)


def tile_pictures(det, frame):
    """The u8 network input of every tile from the restated preprocessing: RGB [3, 96, 128] each."""
    rw, rh = det.tiling_region_sz
    region = np.rint(o.yolo_preprocess(frame, (rh, rw)) * 255)
    return [region[:, int(t[1]):int(t[1]) + TILE_H, int(t[0]):int(t[0]) + TILE_W] for t in det.tiles]


@pytest.mark.parametrize('grid,overlap', GRIDS, ids=GRID_IDS)
def test_tile_pixels(ctx, grid, overlap):
    det = tiled(grid, overlap, weights=RandomWeights(seed=4), reuse_buffers=False)
    n = det.n_tiles
    frame = synthetic_frame(*SIZE, seed=5)
    heads = {}
    try:
        for fused, graphs in ((0, 1), (0, 0), (1, 1), (1, 0)):
            ctx.set_option('fused_input', fused)
            ctx.set_option('use_graphs', graphs)
            det(frame)
            heads[fused, graphs] = [det.backend.read(h, n) for h in det.heads]
            if not fused:
                inp = det.backend.read(det.graph.input, n)              # [n, h, w, 3] RGB
                for t, want in enumerate(tile_pictures(det, frame)):
                    assert want.shape == (3, TILE_H, TILE_W)
                    np.testing.assert_array_equal(np.rint(inp[t].transpose(2, 0, 1) * 255), want)
    finally:
        ctx.set_option('fused_input', 1)
        ctx.set_option('use_graphs', 1)
    for key, got in heads.items():
        for a, b in zip(got, heads[0, 1]):
            assert np.array_equal(a, b), key
    # the test hook that runs the preprocess kernel alone takes the tiles too
    ctx.frame_upload(frame)
    ctx.detect_preprocess_only()
    inp = det.backend.read(det.graph.input, n)
    for t, want in enumerate(tile_pictures(det, frame)):
        np.testing.assert_array_equal(np.rint(inp[t].transpose(2, 0, 1) * 255), want)


def test_tile_pixels_through_the_single_stem_kernel(ctx, monkeypatch):
    """TinyYOLO's first launch is the fused stem pair / triple (stem2.hip); built without it, layer 0 is the single stem
    convolution (stemconv.hip), the third first-launch path: its tiles against the preprocess kernel's, head for head."""
    monkeypatch.setenv('FASTMOT_STEM2', '0')
    det = tiled((2, 2), 0.25, weights=RandomWeights(seed=4), reuse_buffers=False)
    assert det.graph.layers[0]['op'] == 12                              # FM_OP_STEM: stem_conv_kernel takes the frame
    frame = synthetic_frame(*SIZE, seed=5)
    heads = {}
    try:
        for fused, graphs in ((0, 1), (1, 1), (1, 0)):
            ctx.set_option('fused_input', fused)
            ctx.set_option('use_graphs', graphs)
            det(frame)
            heads[fused, graphs] = [det.backend.read(h, det.n_tiles) for h in det.heads]
            if not fused:
                inp = det.backend.read(det.graph.input, det.n_tiles)
                for t, want in enumerate(tile_pictures(det, frame)):
                    np.testing.assert_array_equal(np.rint(inp[t].transpose(2, 0, 1) * 255), want)
    finally:
        ctx.set_option('fused_input', 1)
        ctx.set_option('use_graphs', 1)
    for key, got in heads.items():
        for a, b in zip(got, heads[0, 1]):
            assert np.array_equal(a, b), key
    # (the tiles differ, so a kernel that gave every sample tile 0's origin would not get here)
    assert not np.array_equal(heads[1, 1][0][0], heads[1, 1][0][1])


@pytest.mark.parametrize('grid,overlap', GRIDS, ids=GRID_IDS)
def test_tiles_equal_standalone_detectors_and_merge(ctx, grid, overlap):
    frame = synthetic_frame(*SIZE, seed=6)
    probe = tiled(grid, overlap, reuse_buffers=False)                   # (geometry and box transforms; runs last)
    pictures = tile_pictures(probe, frame)
    upscaled_sz, offsets = probe.upscaled_sz.copy(), [v.copy() for v in probe.tile_bbox_offsets]
    probe.backend.close()
    alone = []
    for t, rgb in enumerate(pictures):
        # the tile's picture as a BGR frame of the network's input size: at zoom 1 the resize is the identity
        bgr = np.ascontiguousarray(rgb[::-1].transpose(1, 2, 0).astype(np.uint8))
        ref = YOLODetector((TILE_W, TILE_H), (0, 1, 2), model='TinyYOLO', conf_thresh=0.25, nms_thresh=0.5,
                           weights=scripted(), max_candidates=16384, reuse_buffers=False)
        ref.upscaled_sz, ref.bbox_offset = upscaled_sz, offsets[t]
        ref._configure(16384)
        dets = ref(bgr)
        alone.append((dets, [ref.backend.read(h, 1)[0] for h in ref.heads], ctx.detect_last_counts()))
        ref.backend.close()
    det = tiled(grid, overlap, reuse_buffers=False)
    merged = det(frame)
    per_tile = det.last_tile_detections
    assert len(per_tile) == det.n_tiles
    heads = [det.backend.read(h, det.n_tiles) for h in det.heads]
    for t, (dets, ref_heads, counts) in enumerate(alone):
        for h_i, want in enumerate(ref_heads):
            assert np.array_equal(heads[h_i][t], want), (t, h_i)
        assert counts[0] > 0 and len(dets) > 0                          # (NMS had candidates in every tile)
        _same(per_tile[t], dets)
    assert ctx.detect_last_counts() == (sum(c[0] for _, _, c in alone), sum(c[1] for _, _, c in alone))
    # the frame's detections: the restated reference merge over the per-tile detections
    union = np.concatenate(per_tile).view(np.recarray)
    ids = np.concatenate([np.full(len(d), t) for t, d in enumerate(per_tile)])
    _same_rows(merged, SSDDetector.merge_dets(union, ids, det.n_tiles, det.merge_thresh))
    assert (np.diff(merged.label) >= 0).all()
    print(grid, 'per tile', [len(d) for d in per_tile], '->', len(merged))
    assert len(merged) < len(union)                                     # (neighbouring tiles saw the same objects)


def test_ordering_prefetch_stale_and_overflow(ctx):
    """Grid (2, 2): four slots of the result ring per frame, so a pass being collected, a prefetched one and a stale one
    are twelve slots in flight."""
    det = tiled((2, 2), 0.25, max_candidates=65536)
    f = [synthetic_frame(*SIZE, seed=30 + i) for i in range(5)]
    want, tiles, n_cand = [], [], []
    for x in f:
        want.append(det(x))
        tiles.append(det.last_tile_detections)
        n_cand.append(ctx.detect_last_counts()[0])
    assert all(len(w) for w in want)
    for a, b in zip(want, want[1:]):                                        # (frames tell apart by their detections)
        assert len(a) != len(b) or (a.tlbr != b.tlbr).any()
    # prefetch(f1) while f0's pass is uncollected, then collect both
    ctx.set_option('net_timing', 1)
    try:
        det.detect_async(f[0])
        det.prefetch(f[1])
        _same(det.postprocess(), want[0])
        assert ctx.detect_net_ms() is not None                            # (the pass's time, once per frame)
        for t, d in enumerate(det.last_tile_detections):
            _same(d, tiles[0][t])
        det.detect_async(f[1])
        det.prefetch(f[2])
        _same(det.postprocess(), want[1])
        assert ctx.detect_net_ms() is not None
        det.detect_async(f[2])
        _same(det.postprocess(), want[2])
    finally:
        ctx.set_option('net_timing', 0)
    # a stale prefetched frame is dropped, the right frame's detections are returned -- also with the ring full:
    # f3 uncollected, f4 prefetched, then another frame asked for
    det.detect_async(f[3])
    det.prefetch(f[4])
    _same(det.postprocess(), want[3])
    det.detect_async(f[0])                                                  # not the announced frame
    _same(det.postprocess(), want[0])
    # three passes in flight fill the ring: none of their tiles is dropped
    ctx.frame_upload(f[2])
    for _ in range(3):
        ctx.detect_async()
    for _ in range(3):
        _same(ctx.detect_sync(), want[2])
    with pytest.raises(_lib.FastMOTHipError, match='no detector pass'):
        ctx.detect_sync()
    # the batched look-ahead is refused on a tiled detector, and the detector keeps working
    with pytest.raises(ValueError):
        det.prefetch_batch(f[0:2])
    ctx.frame_upload_ahead(1, f[0])
    ctx.frame_upload_ahead(2, f[1])
    with pytest.raises(_lib.FastMOTHipError, match='tiled'):
        ctx.detect_async_ahead(2)
    ctx.next_frame, ctx.ahead_frames = None, []
    _same(det(f[4]), want[4])
    # an overflow in a tile is reported on its own frame's collect, once, and that collect consumes the frame's four
    # slots -- no more, no fewer: two passes are in flight, two collects raise, and then nothing is left in the ring (a
    # collect that consumed one slot per error would leave six behind and return tiles of f0 as f1's)
    assert min(n_cand[:3]) > 4 * 64                                        # (so one tile of each frame holds more than 64)
    det._configure(64)
    det.detect_async(f[0])
    det.prefetch(f[1])
    with pytest.raises(_lib.FastMOTHipError, match='overflow'):
        det.postprocess()
    assert det.last_tile_detections is None
    det.detect_async(f[1])                                                  # (announced: no new pass)
    with pytest.raises(_lib.FastMOTHipError, match='overflow'):
        det.postprocess()
    with pytest.raises(_lib.FastMOTHipError, match='no detector pass'):
        ctx.detect_sync()
    # the next pass, same capacity, is collected as a whole frame again: error or not, exactly its own four slots
    det.detect_async(f[2])
    with pytest.raises(_lib.FastMOTHipError, match='overflow'):
        det.postprocess()
    with pytest.raises(_lib.FastMOTHipError, match='no detector pass'):
        ctx.detect_sync()
    det._configure(65536)
    det.detect_async(f[2])
    det.prefetch(f[3])
    _same(det.postprocess(), want[2])
    det.detect_async(f[3])
    _same(det.postprocess(), want[3])


def test_mot_next_frame_prefetch_changes_nothing(ctx):
    import scenes
    from fastmot_amd import Track
    from fastmot_amd.mot import MOT
    from synthetic import SyntheticVideo
    size = (640, 360)
    video = SyntheticVideo(size, n_ids=8, n_frames=8, seed=14)
    weights = calibrated(video.frames[0])

    def run(prefetch):
        cfg = dict(model='TinyYOLO', conf_thresh=0.25, nms_thresh=0.5, max_area=800000, min_aspect_ratio=1.2,
                   weights=ScriptedHeadWeights(0, weights.num_classes, weights.label, weights.obj_bias, weights.obj_gain),
                   tiling_grid=(2, 1))
        mot = MOT(size, detector_type='YOLO', detector_frame_skip=1, class_ids=(1,),
                  yolo_detector_cfg=SimpleNamespace(**cfg),
                  feature_extractor_cfgs=(SimpleNamespace(model='OSNet025', batch_size=16),),
                  tracker_cfg=SimpleNamespace(**scenes.tracker_kwargs()))
        assert mot.detector.n_tiles == 2 and mot.detector.tiling_region_sz == (224, 96)
        Track._count = 0
        mot.reset(1 / 30.)
        rows, n_dets = [], 0
        for i, frame in enumerate(video.frames):
            nxt = video.frames[i + 1] if prefetch and i + 1 < len(video.frames) else None
            mot.step(frame, nxt) if nxt is not None else mot.step(frame)
            n_dets += sum(len(d) for d in mot.detector.last_tile_detections)
            rows.append([(t.trk_id, tuple(t.tlbr), t.confirmed, t.active, t.age, t.hits)
                         for t in mot.tracker.tracks.values()])
        mot.tracker._clear_tracks()
        return rows, n_dets
    ref, n_dets = run(False)
    assert n_dets > 0 and sum(len(r) for r in ref) > 0
    got, _ = run(True)
    assert got == ref


def test_default_grid_is_the_untiled_detector(ctx):
    frame = synthetic_frame(*SIZE, seed=8)
    kw = dict(model='TinyYOLO', conf_thresh=0.25, nms_thresh=0.5)
    plain = YOLODetector(SIZE, (0, 1, 2), weights=scripted(), **kw)
    want = plain(frame)
    assert len(want) > 0
    det = YOLODetector(SIZE, (0, 1, 2), weights=scripted(), tiling_grid=(1, 1), **kw)
    assert det.n_tiles == 1 and det.tiles is None and det.last_tile_detections is None
    _same(det(frame), want)
    # a tiled detector in between leaves nothing behind in the context (its longer result ring is freed with it)
    tiled((2, 2), 0.25)(frame)
    again = YOLODetector(SIZE, (0, 1, 2), weights=scripted(), **kw)
    _same(again(frame), want)
