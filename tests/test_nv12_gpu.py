"""GPU: NV12 ingest (fm_frame_upload_nv12 / fm_frame_upload_ahead_nv12 / fm_frame_ring_store_nv12, csrc/nv12.hip).
The conversion is integer arithmetic, so every comparison is np.array_equal between ctx.frame_read() and
fastmot_amd.utils.nv12.nv12_to_bgr (pinned by known answers in test_nv12_host.py); the detector and MOT.step must
give, on NV12Frames, exactly what they give on the converted BGR ndarrays."""
import ctypes as C

import numpy as np
import pytest

from fastmot_amd import NV12Frame, _lib
from fastmot_amd.utils.nv12 import bgr_to_nv12, nv12_to_bgr

pytestmark = pytest.mark.gpu

FM_ERR_ARG = -2


def configure(ctx, w, h, ring=0):
    ctx.frame_configure(w, h, ring)
    ctx.next_frame, ctx.ahead_frames, ctx.bound_frame = None, [], None


def pitched(rng, w, h, pitch, matrix='bt601'):
    """Random full-range NV12 frame, rows `pitch` bytes apart (the padding random too), uv in an array of its own."""
    ybuf = rng.integers(0, 256, (h, pitch), dtype=np.uint8)
    uvbuf = rng.integers(0, 256, (h // 2, pitch), dtype=np.uint8)
    return NV12Frame(ybuf[:, :w], uvbuf[:, :w], matrix)


def ref_of(f):
    return nv12_to_bgr(f.y, f.uv, f.matrix)


def pitches(w):
    return sorted({w, w + 2, -(-w // 64) * 64, -(-w // 256) * 256})


@pytest.mark.parametrize('matrix', ['bt601', 'bt709'])
def test_every_yuv_triple(ctx, matrix):
    """One 4096 x 4096 frame: its 2048 x 2048 chroma blocks enumerate the 65 536 (U, V) pairs 64 times over, and the 64
    blocks of a pair hold the 256 Y values, four each."""
    n = 4096
    b = np.arange((n // 2) * (n // 2), dtype=np.int64).reshape(n // 2, n // 2)
    pair, group = b % 65536, b // 65536
    uv = np.empty((n // 2, n), np.uint8)
    uv[:, 0::2], uv[:, 1::2] = pair >> 8, pair & 255
    y = np.empty((n, n), np.uint8)
    for r in range(2):
        for c in range(2):
            y[r::2, c::2] = 4 * group + 2 * r + c
    seen = np.zeros((65536, 256), bool)
    seen[np.repeat(np.repeat(pair, 2, 0), 2, 1).ravel(), y.ravel()] = True
    assert seen.all()
    configure(ctx, n, n)
    try:
        ctx.frame_upload(NV12Frame(y, uv, matrix))
        got = ctx.frame_read()
    finally:
        configure(ctx, 16, 16)                   # (releases the 4096 x 4096 buffers)
    assert np.array_equal(got, nv12_to_bgr(y, uv, matrix))


@pytest.mark.parametrize('w', [2, 6, 8, 10, 14, 16, 18, 70, 130, 258])
def test_shapes_and_pitches(ctx, w):
    rng = np.random.default_rng(w)
    for h in (2, 6):
        configure(ctx, w, h, 1)
        for i, pitch in enumerate(pitches(w)):
            f = pitched(rng, w, h, pitch, ('bt601', 'bt709')[i % 2])
            ctx.frame_upload(f)
            assert np.array_equal(ctx.frame_read(), ref_of(f)), (w, h, pitch, 'upload')
            g = pitched(rng, w, h, pitch)
            ctx.frame_ring_store(0, g)
            ctx.frame_ring_select(0)
            assert np.array_equal(ctx.frame_read(), ref_of(g)), (w, h, pitch, 'ring')
        pinned = ctx.pinned_nv12_frames(2, 'bt709')
        for p in pinned:
            assert p.pitch == w and p.size == (w, h)
            p.y[...] = rng.integers(0, 256, (h, w), dtype=np.uint8)
            p.uv[...] = rng.integers(0, 256, (h // 2, w), dtype=np.uint8)
        ctx.frame_upload(pinned[0])
        assert np.array_equal(ctx.frame_read(), ref_of(pinned[0])), (w, h, 'pinned upload')
        ctx.frame_upload_next(pinned[1])
        ctx.frame_promote_next()
        assert np.array_equal(ctx.frame_read(), ref_of(pinned[1])), (w, h, 'pinned ahead')


@pytest.mark.parametrize('size', [(136, 10), (70, 6)])      # 8-byte accesses / the byte path
def test_every_ingest_path(ctx, size):
    w, h = size
    rng = np.random.default_rng(7)
    configure(ctx, w, h, 3)
    nv = [pitched(rng, w, h, (w, w + 2, 256)[i % 3], ('bt601', 'bt709')[i % 2]) for i in range(12)]
    bgr = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(5)]

    ctx.frame_upload(nv[0])
    assert np.array_equal(ctx.frame_read(), ref_of(nv[0]))

    # look-ahead slots 1..4, then four promotes (twice: the second round finds every slot's buffers in use)
    for base in (1, 5):
        for k in range(1, _lib.FM_MAX_DET_BATCH + 1):
            ctx.frame_upload_ahead(k, nv[base + k - 1])
        for k in range(1, _lib.FM_MAX_DET_BATCH + 1):
            ctx.frame_promote_next()
            assert np.array_equal(ctx.frame_read(), ref_of(nv[base + k - 1])), (base, k)

    # the ring: NV12 into index 1 of 3 leaves its neighbours as they were
    for i in range(3):
        ctx.frame_ring_store(i, bgr[i])
    ctx.frame_ring_store(1, nv[9])
    for i, want in enumerate((bgr[0], ref_of(nv[9]), bgr[2])):
        ctx.frame_ring_select(i)
        assert np.array_equal(ctx.frame_read(), want), i

    # BGR and NV12 through the same slots, in turn
    for f in (bgr[3], nv[10], bgr[4], nv[11]):
        ctx.frame_upload(f)
        assert np.array_equal(ctx.frame_read(), f if isinstance(f, np.ndarray) else ref_of(f))
    ctx.frame_upload_next(nv[10])
    ctx.frame_upload_next(nv[11])                # replaces the frame of slot 1 before it was promoted
    ctx.frame_promote_next()
    assert np.array_equal(ctx.frame_read(), ref_of(nv[11]))
    for f in (bgr[3], nv[10], bgr[4], nv[9]):
        ctx.frame_upload_next(f)
        ctx.frame_promote_next()
        assert np.array_equal(ctx.frame_read(), f if isinstance(f, np.ndarray) else ref_of(f))
    # the ring was not touched by any of the uploads
    for i, want in enumerate((bgr[0], ref_of(nv[9]), bgr[2])):
        ctx.frame_ring_select(i)
        assert np.array_equal(ctx.frame_read(), want), i


@pytest.mark.parametrize('size', [(2, 2), (6, 2), (8, 2), (10, 4), (24, 2)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_staged_frames_at_every_ring_address(ctx, size):
    """One kernel converts staged frames and device surfaces, choosing its loads and stores by address.  A ring of three
    frames lies w * h * 3 bytes apart in one allocation: 6x2 puts frame 1 at byte 36 (4-byte aligned only) with runs of six
    pixels, which store bytes; 10x4 (120 bytes a frame) has rows 30 bytes apart, so its whole runs begin 8-byte aligned,
    2 mod 4 and 4-byte aligned in turn and take all three store branches; 8x2 and 24x2 take the 8-byte stores throughout.
    Each destination holds a sentinel first; the converter writes its frame, w * h * 3 bytes, and leaves the ring frames
    on either side of it as they were."""
    w, h = size
    rng = np.random.default_rng(w * 16 + h)
    ring = 3
    configure(ctx, w, h, ring)
    sentinel = np.full((h, w, 3), 0xA5, np.uint8)
    for index in range(ring):
        for i in range(ring):
            ctx.frame_ring_store(i, sentinel)
        f = pitched(rng, w, h, (w, w + 2)[index & 1], ('bt601', 'bt709')[index & 1])
        ctx.frame_ring_store(index, f)
        for i in range(ring):
            ctx.frame_ring_select(i)
            assert np.array_equal(ctx.frame_read(), ref_of(f) if i == index else sentinel), (index, i)
    in_ring = ref_of(f)
    for matrix in ('bt601', 'bt709'):
        f = pitched(rng, w, h, w, matrix)
        ctx.frame_upload(sentinel)
        ctx.frame_upload(f)
        assert np.array_equal(ctx.frame_read(), ref_of(f)), (matrix, 'upload')
        g = pitched(rng, w, h, w + 2, matrix)
        ctx.frame_upload_ahead(1, sentinel)
        ctx.frame_upload_ahead(1, g)
        ctx.frame_promote_next()
        assert np.array_equal(ctx.frame_read(), ref_of(g)), (matrix, 'ahead')
    for i in range(ring):                                    # the uploads went to buffers of their own
        ctx.frame_ring_select(i)
        assert np.array_equal(ctx.frame_read(), in_ring if i == ring - 1 else sentinel), i
    configure(ctx, 16, 16)


def test_errors(ctx):
    lib = ctx.lib
    w, h = 16, 4
    configure(ctx, w, h, 1)
    rng = np.random.default_rng(3)
    before = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    ctx.frame_upload(before)
    ctx.frame_ring_store(0, before)
    f = pitched(rng, w, h, w)
    y, uv = _lib._ptr(f.y), _lib._ptr(f.uv)
    c = C.c_int
    calls = [lambda p, m: lib.fm_frame_upload_nv12(ctx.handle, y, uv, c(p), c(m)),
             lambda p, m: lib.fm_frame_upload_ahead_nv12(ctx.handle, c(1), y, uv, c(p), c(m)),
             lambda p, m: lib.fm_frame_ring_store_nv12(ctx.handle, c(0), y, uv, c(p), c(m))]
    for call in calls:
        for pitch, matrix in ((w - 2, 0), (0, 0), (w, 2), (w, -1)):
            assert call(pitch, matrix) == FM_ERR_ARG
            assert b'bad argument' in lib.fm_last_error()
    for k in (0, _lib.FM_MAX_DET_BATCH + 1):
        assert lib.fm_frame_upload_ahead_nv12(ctx.handle, c(k), y, uv, c(w), c(0)) == FM_ERR_ARG
        assert b'bad argument' in lib.fm_last_error()
    for index in (-1, 1):
        assert lib.fm_frame_ring_store_nv12(ctx.handle, c(index), y, uv, c(w), c(0)) == FM_ERR_ARG
        assert b'bad argument' in lib.fm_last_error()
    assert lib.fm_frame_upload_nv12(ctx.handle, None, uv, c(w), c(0)) == FM_ERR_ARG
    with pytest.raises(_lib.FastMOTHipError):                    # no frame in slot 1: none of the calls above put one there
        ctx.frame_promote_next()
    assert np.array_equal(ctx.frame_read(), before)              # nothing was copied or launched
    ctx.frame_ring_select(0)
    assert np.array_equal(ctx.frame_read(), before)
    with pytest.raises(ValueError):                              # a frame of another size than the context's
        ctx.frame_upload(pitched(rng, w + 2, h, w + 2))
    # frame sizes that are not even: BGR frames pass, NV12 frames are refused
    for ow, oh in ((15, 4), (16, 5)):
        configure(ctx, ow, oh, 1)
        for call in calls:
            assert call(16, 0) == FM_ERR_ARG
            assert b'bad argument' in lib.fm_last_error()
    configure(ctx, w, h)


def test_detector_on_nv12_frames_equals_bgr(ctx):
    from fastmot_amd.detector import YOLODetector
    from fastmot_amd.models.graph import RandomWeights
    from test_detect_batch_gpu import _same
    from test_detect_gpu import TinyYOLO, synthetic_frame  # noqa: F401  (registers the tiny model)
    size = (320, 180)
    det = YOLODetector(size, (0, 1, 2), model='TinyYOLO', conf_thresh=0.1, nms_thresh=0.5, weights=RandomWeights(seed=4),
                       max_candidates=16384, reuse_buffers=False, max_batch=2)
    planes = [bgr_to_nv12(synthetic_frame(*size, seed=80 + i)) for i in range(2)]
    want = det.detect_batch([nv12_to_bgr(y, uv) for y, uv in planes])
    assert sum(len(d) for d in want) > 0
    for got, ref in zip(det.detect_batch([NV12Frame(y, uv) for y, uv in planes]), want):
        _same(got, ref)
    for (y, uv), ref in zip(planes, want):          # one frame at a time: __call__ and prefetch
        f = NV12Frame(y, uv)
        _same(det(f), ref)
        det.prefetch(f)
        det.detect_async(f)
        _same(det.postprocess(), ref)


@pytest.mark.parametrize('mode', ['steps', 'next_frame', 'ring'])
def test_mot_on_nv12_frames_equals_bgr(ctx, mode):
    from synthetic import SyntheticVideo
    from fastmot_amd import Track
    from fastmot_amd.detector import DeviceFrame
    from test_mot_gpu import build_mot
    size = (960, 540)
    video = SyntheticVideo(size, n_ids=10, n_frames=16)
    planes = [bgr_to_nv12(f) for f in video.frames]
    sources = {'nv12': [NV12Frame(y, uv) for y, uv in planes], 'bgr': [nv12_to_bgr(y, uv) for y, uv in planes]}
    runs = {}
    for kind, frames in sources.items():
        if mode == 'ring':
            configure(ctx, size[0], size[1], video.n_frames)
            for i, fr in enumerate(frames):
                ctx.frame_ring_store(i, fr)
            frames = [DeviceFrame(i) for i in range(video.n_frames)]
        mot = build_mot(size, video, 1)
        Track._count = 0
        mot.reset(1 / 30.)
        rows = []
        for f in range(video.n_frames):
            mot.detector._frame_idx = f
            nxt = frames[f + 1] if mode != 'steps' and f + 1 < video.n_frames else None
            mot.step(frames[f], next_frame=nxt)
            rows.append([(t.trk_id, tuple(t.tlbr), t.confirmed, t.active, t.age, t.hits) for t in mot.tracker.tracks.values()])
        mot.tracker._clear_tracks()
        runs[kind] = rows
    assert runs['nv12'] == runs['bgr']
    assert len(runs['bgr'][-1]) >= 8


def test_draw_needs_host_bgr_frames(ctx):
    from synthetic import SyntheticVideo
    from test_mot_gpu import build_mot
    size = (960, 540)
    video = SyntheticVideo(size, n_ids=4, n_frames=1)
    mot = build_mot(size, video, 1)
    mot.draw = True
    mot.reset(1 / 30.)
    with pytest.raises(TypeError):
        mot.step(NV12Frame(*bgr_to_nv12(video.frames[0])))
    mot.tracker._clear_tracks()
