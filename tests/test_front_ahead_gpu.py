"""GPU: front-ahead (detect.hip detect_pass, net.hip fm_net_front_prepare) -- the first K layers of a look-ahead pass run on
another stream while the previous pass is still in flight.  No kernel changes, so every comparison is array_equal:
  * forced cuts on the tiny detector, passes enqueued in the prefetch pattern (next pass started before the previous one is
    collected) against the same frames run one at a time with front-ahead off: detections, sorted candidates, head tensors;
    with and without captured graphs, on both candidate streams
  * YOLOv4 @ 608 with the rule's cut on its shared activation arena (reuse_buffers=True)
  * the paths that must not take a front: idle stream (auto), batched and tiled passes, det_front_layers = 0
  * MOT.step(frame, next_frame) over 12 frames: tracks and the detector's own output equal the sequential run
  * net_timing of a pass in two parts: positive, and not longer than the pass took on the host's clock"""
import time

import numpy as np
import pytest

from fastmot_amd.detector import YOLODetector
from fastmot_amd.models.graph import RandomWeights
from test_detect_gpu import TinyLetterbox, TinyYOLO, synthetic_frame  # noqa: F401  (registers the tiny models)

pytestmark = pytest.mark.gpu

OPTIONS = ('det_front_ahead', 'det_front_layers', 'det_front_stream')


@pytest.fixture
def front(ctx):
    """Sets the front-ahead options; puts them (and the two options the tests combine them with) back afterwards."""
    keep = {k: ctx.get_option(k) for k in OPTIONS}

    def set_options(ahead, layers=None, stream=None):
        ctx.set_option('det_front_ahead', ahead)
        if layers is not None:
            ctx.set_option('det_front_layers', layers)
        if stream is not None:
            ctx.set_option('det_front_stream', stream)
    yield set_options
    for k, v in keep.items():
        ctx.set_option(k, v)
    ctx.set_option('use_graphs', 1)
    ctx.set_option('net_timing', 0)


def _same(a, b, tag=''):
    assert len(a) == len(b), tag
    np.testing.assert_array_equal(a.tlbr, b.tlbr, err_msg=str(tag))
    np.testing.assert_array_equal(a.label, b.label, err_msg=str(tag))
    np.testing.assert_array_equal(a.conf, b.conf, err_msg=str(tag))


def _tiny(size=(320, 180), model='TinyLetterbox', **kw):
    return YOLODetector(size, (0, 1, 2), model=model, conf_thresh=0.1, nms_thresh=0.5, weights=RandomWeights(seed=4),
                        max_candidates=16384, **kw)


def _one_at_a_time(ctx, det, frames):
    """-> per frame (detections, sorted candidate rows as bits, head tensors), each frame a pass of its own."""
    out = []
    for f in frames:
        dets = det(f)
        out.append((dets, ctx.detect_raw_candidates().view(np.uint32).copy(), [det.backend.read(h, 1)[0] for h in det.heads]))
    return out


def _pipelined(ctx, det, frames, order, candidates=False):
    """The prefetch pattern of MOT.step: the next frame is uploaded and its pass started before the previous pass is
    collected.  -> detections per pass (and, with `candidates`, the sorted candidate rows per pass: reading them waits for
    the pass, so the run without them is the one that keeps two passes in flight)."""
    dets, cands = [], []
    det.prefetch(frames[order[0]])
    if candidates:
        cands.append(ctx.detect_raw_candidates().view(np.uint32).copy())
    for i, o in enumerate(order):
        det.detect_async(frames[o])                 # (announced: promotes the frame, enqueues nothing)
        if i + 1 < len(order):
            det.prefetch(frames[order[i + 1]])
            if candidates:
                cands.append(ctx.detect_raw_candidates().view(np.uint32).copy())
        dets.append(det.postprocess())
    return dets, cands


ORDER = [0, 1, 2, 0, 2, 1, 1]       # seven passes over three frames: both buffer sets see every frame


# k = 1: the eager first launch alone; 2: tensor 3 is written by the front (layer 0) and by the back (layer 2); 3: back
# layer 3 reads the concat that front layers 0 and 2 wrote; 10: the whole first level, whose output the neck reads 50 layers on
@pytest.mark.parametrize('k,graphs,stream', [(1, 1, 0), (2, 1, 0), (3, 1, 0), (10, 1, 0), (1, 0, 0), (3, 0, 0), (10, 0, 1),
                                            (1, 1, 1), (2, 1, 1), (3, 1, 1), (10, 1, 1)])
def test_forced_cut_equals_one_pass_at_a_time(ctx, front, k, graphs, stream):
    size = (320, 180)
    frames = [synthetic_frame(*size, seed=60 + i) for i in range(3)]
    det = _tiny(size)
    ctx.set_option('use_graphs', graphs)
    front(0)
    want = _one_at_a_time(ctx, det, frames)
    assert len({len(w[0]) for w in want}) > 1 and all(len(w[1]) for w in want)      # (the frames tell apart; candidates to sort)
    assert ctx.front_info()[2] == 0
    front(2, k, stream)
    dets, _ = _pipelined(ctx, det, frames, ORDER)
    heads = [det.backend.read(h, 1)[0] for h in det.heads]
    assert ctx.front_info()[0] == k and ctx.front_info()[2] == len(ORDER)
    for i, (got, o) in enumerate(zip(dets, ORDER)):
        _same(got, want[o][0], f'pass {i}, frame {o}')
    for got, exp in zip(heads, want[ORDER[-1]][2]):
        np.testing.assert_array_equal(got, exp)
    dets, cands = _pipelined(ctx, det, frames, ORDER, candidates=True)
    for i, (got, c, o) in enumerate(zip(dets, cands, ORDER)):
        _same(got, want[o][0], f'pass {i}, frame {o} (candidates read)')
        np.testing.assert_array_equal(c, want[o][1], err_msg=f'pass {i}, frame {o}')
    # ... and a pass of the whole table between passes in two parts lands on whichever set is selected
    front(0)
    _same(det(frames[2]), want[2][0])
    front(2)
    dets, _ = _pipelined(ctx, det, frames, ORDER[:3])
    for got, o in zip(dets, ORDER):
        _same(got, want[o][0])


def test_tiny_yolo_without_letterbox(ctx, front):
    size = (320, 180)
    frames = [synthetic_frame(*size, seed=70 + i) for i in range(3)]
    det = _tiny(size, model='TinyYOLO')
    front(0)
    want = _one_at_a_time(ctx, det, frames)
    front(2, 3, 0)
    dets, _ = _pipelined(ctx, det, frames, ORDER)
    for got, o in zip(dets, ORDER):
        _same(got, want[o][0])
    for got, exp in zip([det.backend.read(h, 1)[0] for h in det.heads], want[ORDER[-1]][2]):
        np.testing.assert_array_equal(got, exp)


def test_yolov4_608_rule_cut_on_the_arena(ctx, front):
    """The benchmark's detector, activations in the shared arena: the front's tensors must have left it, or the front of
    pass p + 1 overwrites what the tail of pass p still reads."""
    from synthetic import scripted_head_weights
    size = (1920, 1080)
    frames = [synthetic_frame(*size, seed=40 + i) for i in range(2)]
    weights = scripted_head_weights(size, 'YOLOv4_608', 1, frames[0], 600)
    det = YOLODetector(size, (1,), model='YOLOv4_608', conf_thresh=0.25, nms_thresh=0.5, weights=weights)
    front(0)
    want = _one_at_a_time(ctx, det, frames)
    assert all(len(w[1]) for w in want)
    front(2, -1, ctx.get_option('det_front_stream'))
    order = [0, 1, 1, 0]
    dets, _ = _pipelined(ctx, det, frames, order)
    k, nbytes, passes = ctx.front_info()
    assert k == 8 and passes == len(order) and 0 < nbytes <= 512 << 20   # rows 0-7: the 304 x 304 and 152 x 152 levels
    for got, o in zip(dets, order):
        _same(got, want[o][0])
    for got, exp in zip([det.backend.read(h, 1)[0] for h in det.heads], want[order[-1]][2]):
        np.testing.assert_array_equal(got, exp)


def test_paths_that_take_no_front(ctx, front):
    size = (320, 180)
    frames = [synthetic_frame(*size, seed=80 + i) for i in range(3)]
    det = _tiny(size, max_batch=2)
    front(0)
    want = [det(f) for f in frames]
    # auto on an idle stream: every pass is collected before the next is enqueued
    front(1, 3)
    for f, w in zip(frames, want):
        det.prefetch(f)
        det.detect_async(f)
        _same(det.postprocess(), w)
    # forced, but the cut is 0 / the pass is sequential / the pass is batched
    front(2, 0)
    dets, _ = _pipelined(ctx, det, frames, ORDER)
    for got, o in zip(dets, ORDER):
        _same(got, want[o])
    front(2, 3)
    for f, w in zip(frames, want):
        _same(det(f), w)
    for got, w in zip(det.detect_batch(frames[:2]), want):
        _same(got, w)
    assert ctx.front_info()[2] == 0
    # a tiled detector: its passes are batched passes over the tiles
    front(0)
    tiled = YOLODetector(size, (0, 1, 2), model='TinyYOLO', conf_thresh=0.1, nms_thresh=0.5, weights=RandomWeights(seed=4),
                         max_candidates=16384, tiling_grid=(2, 1))
    want_t = [tiled(f) for f in frames]
    front(2, 3)
    dets, _ = _pipelined(ctx, tiled, frames, ORDER)
    for got, o in zip(dets, ORDER):
        _same(got, want_t[o])
    assert ctx.front_info()[2] == 0


def test_mot_step_with_next_frame(ctx, front):
    from synthetic import SyntheticVideo
    from fastmot_amd import Track
    from test_mot_gpu import build_mot
    size = (960, 540)
    video = SyntheticVideo(size, n_ids=8, n_frames=12, seed=13)
    runs = []
    for prefetch, ahead in ((False, 0), (True, 0), (True, 1), (True, 2)):
        mot = build_mot(size, video, 1)
        front(ahead, -1)
        Track._count = 0
        mot.reset(1 / 30.)
        rows = []
        for f in range(video.n_frames):
            mot.detector._frame_idx = f
            nxt = video.frames[f + 1] if prefetch and f + 1 < video.n_frames else None
            mot.step(video.frames[f], next_frame=nxt)
            real = mot.detector.last_real
            rows.append(([(t.trk_id, tuple(t.tlbr), t.confirmed, t.active, t.age, t.hits)
                          for t in mot.tracker.tracks.values()], real.tlbr.tobytes(), real.conf.tobytes()))
        if ahead == 2:      # the 160 x 288 detector's first layer writes an 80 x 144 map: the rule gives it a front
            assert ctx.front_info()[0] >= 1 and ctx.front_info()[2] == video.n_frames - 1
        runs.append(rows)
        mot.tracker._clear_tracks()
    assert runs[0] == runs[1] == runs[2] == runs[3]
    assert len(runs[0][-1][0]) >= 6


def test_net_timing_of_a_pass_in_two_parts(ctx, front):
    size = (320, 180)
    frames = [synthetic_frame(*size, seed=90 + i) for i in range(2)]
    det = _tiny(size)
    front(2, 3, 0)
    det.prefetch(frames[0])
    det.detect_async(frames[0])
    det.postprocess()                       # (graphs captured)
    ctx.set_option('net_timing', 1)
    for f in (frames[1], frames[0]):
        t0 = time.perf_counter()
        det.prefetch(f)
        det.detect_async(f)
        det.postprocess()
        wall_ms = (time.perf_counter() - t0) * 1e3
        ms = ctx.detect_net_ms()
        print(f'net_timing {ms:.4f} ms, enqueue -> collection {wall_ms:.4f} ms')
        assert ms is not None and 0 < ms <= wall_ms
    assert ctx.front_info()[2] == 3
