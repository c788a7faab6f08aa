"""GPU: the batched detector pass (fm_detect_async_ahead, YOLODetector.detect_batch / prefetch_batch).
  * every head tensor of sample i of a batch-n pass is array_equal to a batch-1 pass on frame i (the detector network
    takes every reduction-order choice from the batch-1 geometry), fused stem input or preprocess kernel, graphs or not
  * detections of detect_batch == n sequential detect_async / postprocess, exactly
  * frames are collected in enqueue order across batch and single passes; stale announced frames are dropped;
    a batch larger than the network's max_batch is an error; an overflow is reported on each frame's own collect"""
import numpy as np
import pytest

from fastmot_amd import _lib
from fastmot_amd.detector import DeviceFrame, YOLODetector
from fastmot_amd.models.graph import RandomWeights
from test_detect_gpu import TinyLetterbox, TinyYOLO, synthetic_frame  # noqa: F401  (registers the tiny models)

pytestmark = pytest.mark.gpu


def _frames(size, n, seed=20):
    return [synthetic_frame(*size, seed=seed + i) for i in range(n)]


def _same(a, b):
    assert len(a) == len(b)
    np.testing.assert_array_equal(a.tlbr, b.tlbr)
    np.testing.assert_array_equal(a.label, b.label)
    np.testing.assert_array_equal(a.conf, b.conf)


@pytest.mark.parametrize('model', ['TinyYOLO', 'TinyLetterbox', 'YOLOv4_608', 'YOLOv4CSP_640', 'YOLOv4P6_1280'])
def test_batch_heads_equal_batch1(ctx, model):
    """Heads of a batched pass == heads of batch-1 passes, bit for bit.  YOLOv4-P6 @ 1280 (config[4]): 4K frames,
    max_batch 2, the default option combination only (its batch-1 pass is compared with the reference, tensor by tensor
    and layer by layer, in test_fullsize_gpu.py)."""
    full = model.startswith('YOLOv4')
    p6 = model == 'YOLOv4P6_1280'
    size = (3840, 2160) if p6 else (1920, 1080) if full else (320, 180)
    max_batch = 2 if p6 else 3
    det = YOLODetector(size, (0, 1, 2), model=model, conf_thresh=0.1, nms_thresh=0.5, weights=RandomWeights(seed=4),
                       max_candidates=65536, reuse_buffers=False, max_batch=max_batch)
    frames = _frames(size, max_batch)
    # (full-size models: one of the two stem paths with graphs off, to bound the suite's time)
    cases = [(1, 1)] if p6 else [(1, 1), (0, 1), (1, 0)] if full else [(1, 1), (0, 1), (1, 0), (0, 0)]
    try:
        for fused, graphs in cases:
            ctx.set_option('fused_input', fused)
            ctx.set_option('use_graphs', graphs)
            ref = []
            for f in frames:
                det(f)
                ref.append([det.backend.read(h, 1)[0] for h in det.heads])
            for n in range(2, max_batch + 1):
                det.detect_batch(frames[:n])
                for h_i, h in enumerate(det.heads):
                    got = det.backend.read(h, n)
                    for i in range(n):
                        assert np.array_equal(got[i], ref[i][h_i]), (fused, graphs, n, i, h_i)
    finally:
        ctx.set_option('fused_input', 1)
        ctx.set_option('use_graphs', 1)
    if model in ('YOLOv4_608', 'YOLOv4P6_1280'):
        assert det.graph.layers[0]['op'] in (12, 18)          # the fused stem really ran on the fused path


@pytest.mark.parametrize('model', ['TinyYOLO', 'YOLOv4_608'])
def test_detect_batch_equals_sequential(ctx, model):
    from synthetic import scripted_head_weights
    size = (1920, 1080) if model == 'YOLOv4_608' else (320, 180)
    frames = _frames(size, 5, seed=40)
    weights = scripted_head_weights(size, model, 1, frames[0], 600)
    det = YOLODetector(size, (1,), model=model, conf_thresh=0.25, nms_thresh=0.5, weights=weights, max_batch=3)
    seq, cands = [], 0
    for f in frames:
        seq.append(det(f))
        cands += ctx.detect_last_counts()[0]
    assert cands > 0                                        # (the sort + NMS of every frame has candidates to work on)
    for n in (2, 3):
        for got, want in zip(det.detect_batch(frames[:n]), seq):
            _same(got, want)
    got = det.detect_batch(frames)                          # 5 frames, max_batch 3: passes of 3 and 2
    assert len(got) == 5
    for g, w in zip(got, seq):
        _same(g, w)


def test_ordering_stale_and_errors(ctx):
    size = (320, 180)
    det = YOLODetector(size, (0, 1, 2), model='TinyYOLO', conf_thresh=0.1, nms_thresh=0.5,
                       weights=RandomWeights(seed=4), max_candidates=16384, reuse_buffers=False, max_batch=3)
    f = _frames(size, 8, seed=60)
    want = [det(x) for x in f]
    assert len({len(w) for w in want}) > 1                  # (frames tell apart by their detections)
    ctx.set_option('net_timing', 1)
    try:
        # batch pass, single pass, batch pass: collected in frame order; the pass's time on its first frame only
        det.detect_async(f[0])
        det.prefetch_batch(f[1:3])
        got = [det.postprocess()]
        for x in f[1:3]:
            det.detect_async(x)
            got.append(det.postprocess())
            assert (ctx.detect_net_ms() is not None) == (x is f[1])
        det.prefetch(f[3])
        det.detect_async(f[3])
        got.append(det.postprocess())
        det.prefetch_batch(f[4:7])
        for x in f[4:7]:
            det.detect_async(x)
            got.append(det.postprocess())
        for g, w in zip(got, want[:7]):
            _same(g, w)
    finally:
        ctx.set_option('net_timing', 0)
    # a frame other than the announced one: the stale results are dropped, this frame's are returned
    det.prefetch_batch(f[1:4])
    det.detect_async(f[1])
    _same(det.postprocess(), want[1])
    det.detect_async(f[7])                                  # f[2], f[3] were announced
    _same(det.postprocess(), want[7])
    det.prefetch_batch(f[0:2])
    det.detect_async(f[5])
    _same(det.postprocess(), want[5])
    # more frames than the network's batch: an error, and the detector keeps working
    with pytest.raises(ValueError):
        det.prefetch_batch(f[0:4])
    ctx.frame_upload_ahead(4, f[3])
    for k in (1, 2, 3):
        ctx.frame_upload_ahead(k, f[k - 1])
    with pytest.raises(_lib.FastMOTHipError):
        ctx.detect_async_ahead(4)
    ctx.next_frame, ctx.ahead_frames = None, []
    for g, w in zip(det.detect_batch(f[2:5]), want[2:5]):
        _same(g, w)


def test_resident_frames_and_upload_slots_mix(ctx):
    """Look-ahead slots pointing at ring frames and at upload slots in one pass, then promoted step by step."""
    size = (320, 180)
    det = YOLODetector(size, (0, 1, 2), model='TinyYOLO', conf_thresh=0.1, nms_thresh=0.5,
                       weights=RandomWeights(seed=4), max_candidates=16384, max_batch=3)
    f = _frames(size, 6, seed=80)
    want = [det(x) for x in f]
    ctx.frame_configure(size[0], size[1], 6)
    for i, x in enumerate(f):
        ctx.frame_ring_store(i, x)
    mixed = [f[0], DeviceFrame(1), f[2]]
    for g, w in zip(det.detect_batch(mixed), want[:3]):
        _same(g, w)
    det.detect_async(f[3])
    _same(det.postprocess(), want[3])
    det.prefetch_batch([DeviceFrame(4), f[5], f[1]])
    for x, w in ((None, want[4]), (f[5], want[5]), (f[1], want[1])):
        x = det._announced[0] if x is None else x
        det.detect_async(x)
        _same(det.postprocess(), w)
        assert ctx.frame_read().tobytes() == (f[x.index] if isinstance(x, DeviceFrame) else x).tobytes()


def test_overflow_is_reported_per_frame(ctx):
    """Each frame of a batched pass reports its own candidate-list overflow on its own collect, and the ring stays in
    order: the frames after it, and the passes after it, are collected normally."""
    from synthetic import scripted_head_weights
    size = (320, 180)
    frames = _frames(size, 3, 90)
    weights = scripted_head_weights(size, 'TinyYOLO', 1, frames[0], 300)
    det = YOLODetector(size, (0, 1, 2), model='TinyYOLO', conf_thresh=0.25, nms_thresh=0.5, weights=weights,
                       max_candidates=65536, max_batch=2)
    want = [det(x) for x in frames]
    n = ctx.detect_last_counts()[0]
    assert n > 64
    det._configure(64)
    det.prefetch_batch(frames[:2])
    for x in frames[:2]:
        det.detect_async(x)
        with pytest.raises(_lib.FastMOTHipError, match='overflow'):
            det.postprocess()
    det._configure(65536)
    det.prefetch_batch(frames[1:3])
    for x, w in zip(frames[1:3], want[1:3]):
        det.detect_async(x)
        _same(det.postprocess(), w)
