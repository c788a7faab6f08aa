"""GPU: JPEG ingest (fm_frame_upload_jpeg / fm_frame_upload_ahead_jpeg / fm_frame_ring_store_jpeg, csrc/jpeg.hip).
The decode is integer arithmetic, so every comparison is np.array_equal between ctx.frame_read() and Pillow's decode of
the same file; the detector, MOT.step and the frame loop must give, on JPEGFrames, exactly what they give on the
Pillow-decoded ndarrays."""
import ctypes as C
import io
import itertools

import numpy as np
import pytest

import jpeg_cases as jc
from fastmot_amd import JPEGFrame, NV12Frame, _lib
from fastmot_amd.utils import jpeg as J
from fastmot_amd.utils.nv12 import nv12_to_bgr

pytestmark = pytest.mark.gpu

FM_ERR_ARG = -2


def configure(ctx, w, h, ring=0):
    ctx.frame_configure(w, h, ring)
    ctx.next_frame, ctx.ahead_frames, ctx.bound_frame = None, [], None


@pytest.mark.parametrize('size', jc.SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_frame_equals_pillow(ctx, size):
    configure(ctx, *size)
    for sub in jc.SUBSAMPLINGS:
        for label, data in jc.cases(size, sub):
            ctx.frame_upload(JPEGFrame(data))
            assert np.array_equal(ctx.frame_read(), jc.pillow_bgr(data)), label


@pytest.mark.parametrize('size', [(1920, 1080), (1916, 1076)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_full_frame_equals_pillow(ctx, size):
    """Frame scale; neither dimension of the second size is a multiple of 8: partial blocks on both edges."""
    data = jc.encode(jc.content('textured', *size), '420', 90)
    configure(ctx, *size)
    try:
        ctx.frame_upload(JPEGFrame(data))
        got = ctx.frame_read()
    finally:
        configure(ctx, 16, 16)
    assert np.array_equal(got, jc.pillow_bgr(data))


def jpeg_frames(rng, w, h, n, buffers=None):
    """n JPEGFrames of random images, subsampling / quality / restarts in turn, with Pillow's decode of each."""
    out = []
    for i in range(n):
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        data = jc.encode(rgb, jc.SUBSAMPLINGS[i % 4], (75, 95, 30)[i % 3], (0, 2)[i % 2])
        out.append((JPEGFrame(data, buffer=None if buffers is None else buffers[i]), jc.pillow_bgr(data)))
    return out


@pytest.mark.parametrize('size', [(136, 10), (70, 6)])      # 8-byte stores / the byte path
def test_every_ingest_path(ctx, size):
    w, h = size
    rng = np.random.default_rng(7)
    configure(ctx, w, h, 3)
    pinned = ctx.pinned_jpeg_buffers(6)
    assert all(b.dtype == np.int16 and b.size >= J.max_coefficients(w, h) + J.QT_ENTRIES for b in pinned)
    jp = jpeg_frames(rng, w, h, 12, [pinned[i] if i < 6 else None for i in range(12)])    # page-locked and pageable buffers
    bgr = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(5)]
    y, uv = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8)
    nv = (NV12Frame(y, uv), nv12_to_bgr(y, uv))

    ctx.frame_upload(jp[0][0])
    assert np.array_equal(ctx.frame_read(), jp[0][1])

    # look-ahead slots 1..4, then four promotes (twice: the second round finds every slot's buffers in use)
    for base in (0, 6):
        for k in range(1, _lib.FM_MAX_DET_BATCH + 1):
            ctx.frame_upload_ahead(k, jp[base + k - 1][0])
        for k in range(1, _lib.FM_MAX_DET_BATCH + 1):
            ctx.frame_promote_next()
            assert np.array_equal(ctx.frame_read(), jp[base + k - 1][1]), (base, k)

    # the ring: a JPEG into index 1 of 3 leaves its neighbours as they were
    for i in range(3):
        ctx.frame_ring_store(i, bgr[i])
    ctx.frame_ring_store(1, jp[9][0])
    ring = (bgr[0], jp[9][1], bgr[2])
    for i, want in enumerate(ring):
        ctx.frame_ring_select(i)
        assert np.array_equal(ctx.frame_read(), want), i

    # JPEG, BGR and NV12 frames through the same slots, in every order of the three
    kinds = {'jpeg': jp[10], 'bgr': (bgr[3], bgr[3]), 'nv12': nv}
    for order in itertools.permutations(kinds):
        for name in order:
            frame, want = kinds[name]
            ctx.frame_upload(frame)
            assert np.array_equal(ctx.frame_read(), want), (order, name, 'upload')
        for name in order:
            frame, want = kinds[name]
            ctx.frame_upload_next(frame)
            ctx.frame_promote_next()
            assert np.array_equal(ctx.frame_read(), want), (order, name, 'ahead')
    ctx.frame_upload_next(jp[10][0])
    ctx.frame_upload_next(jp[11][0])               # replaces the frame of slot 1 before it was promoted
    ctx.frame_promote_next()
    assert np.array_equal(ctx.frame_read(), jp[11][1])
    # the ring was not touched by any of the uploads
    for i, want in enumerate(ring):
        ctx.frame_ring_select(i)
        assert np.array_equal(ctx.frame_read(), want), i

    # another size and back: the staging buffers are freed and made again
    configure(ctx, w + 8, h + 3, 1)
    other = jpeg_frames(rng, w + 8, h + 3, 3)
    ctx.frame_upload(other[0][0])
    assert np.array_equal(ctx.frame_read(), other[0][1])
    ctx.frame_upload_next(other[1][0])
    ctx.frame_promote_next()
    assert np.array_equal(ctx.frame_read(), other[1][1])
    ctx.frame_ring_store(0, other[2][0])
    ctx.frame_ring_select(0)
    assert np.array_equal(ctx.frame_read(), other[2][1])
    configure(ctx, w, h, 1)
    for frame, want in jp[6:9]:
        ctx.frame_upload(frame)
        assert np.array_equal(ctx.frame_read(), want)
    ctx.frame_upload_next(jp[3][0])
    ctx.frame_promote_next()
    assert np.array_equal(ctx.frame_read(), jp[3][1])
    ctx.frame_ring_store(0, jp[4][0])
    ctx.frame_ring_select(0)
    assert np.array_equal(ctx.frame_read(), jp[4][1])


def test_errors(ctx):
    lib = ctx.lib
    w, h = 16, 4
    configure(ctx, w, h, 1)
    rng = np.random.default_rng(3)
    before = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    ctx.frame_upload(before)
    ctx.frame_ring_store(0, before)
    good = JPEGFrame(jc.encode(jc.content('noise', w, h), '420', 75))
    wrong = JPEGFrame(jc.encode(jc.content('noise', w + 8, h), '420', 75))
    c = C.c_int

    def args(f, info=None):
        return C.byref(f.info if info is None else info), _lib._ptr(f.coef), _lib._ptr(f.qt)

    calls = [lambda *a: lib.fm_frame_upload_jpeg(ctx.handle, *a),
             lambda *a: lib.fm_frame_upload_ahead_jpeg(ctx.handle, c(1), *a),
             lambda *a: lib.fm_frame_ring_store_jpeg(ctx.handle, c(0), *a)]
    tampered = []
    for field, value in (('coef_count', good.info.coef_count + 64), ('ncomp', 2), ('width', w + 1)):
        info = J.JpegInfo.from_buffer_copy(good.info)
        setattr(info, field, value)
        tampered.append(info)
    info = J.JpegInfo.from_buffer_copy(good.info)
    info.hsamp[0] = 4
    tampered.append(info)
    for call in calls:
        assert call(*args(wrong)) == FM_ERR_ARG                      # an image of another size than the context's frames
        assert b'bad argument' in lib.fm_last_error()
        for info in tampered:                                        # a layout fm_jpeg_info cannot have returned
            assert call(*args(good, info)) == FM_ERR_ARG
        assert call(None, _lib._ptr(good.coef), _lib._ptr(good.qt)) == FM_ERR_ARG
        assert call(C.byref(good.info), None, _lib._ptr(good.qt)) == FM_ERR_ARG
        assert call(C.byref(good.info), _lib._ptr(good.coef), None) == FM_ERR_ARG
    for k in (0, _lib.FM_MAX_DET_BATCH + 1):
        assert lib.fm_frame_upload_ahead_jpeg(ctx.handle, c(k), *args(good)) == FM_ERR_ARG
        assert b'bad argument' in lib.fm_last_error()
    for index in (-1, 1):
        assert lib.fm_frame_ring_store_jpeg(ctx.handle, c(index), *args(good)) == FM_ERR_ARG
        assert b'bad argument' in lib.fm_last_error()
    with pytest.raises(_lib.FastMOTHipError):                    # no frame in slot 1: none of the calls above put one there
        ctx.frame_promote_next()
    assert np.array_equal(ctx.frame_read(), before)              # nothing was copied or launched
    ctx.frame_ring_select(0)
    assert np.array_equal(ctx.frame_read(), before)
    for method in (ctx.frame_upload, ctx.frame_upload_next, lambda f: ctx.frame_ring_store(0, f)):
        with pytest.raises(ValueError):
            method(wrong)
    ctx.frame_upload(good)                                       # and the calls still work
    assert np.array_equal(ctx.frame_read(), good.to_bgr())


def clip_files(frames, quality=90):
    """A synthetic clip as JPEG files: (file bytes, Pillow's decode) per frame."""
    files = [jc.encode(np.ascontiguousarray(f[:, :, ::-1]), '420', quality) for f in frames]
    return files, [jc.pillow_bgr(d) for d in files]


def test_detector_on_jpeg_frames_equals_bgr(ctx):
    from fastmot_amd.detector import YOLODetector
    from fastmot_amd.models.graph import RandomWeights
    from test_detect_batch_gpu import _same
    from test_detect_gpu import TinyYOLO, synthetic_frame  # noqa: F401  (registers the tiny model)
    size = (320, 180)
    det = YOLODetector(size, (0, 1, 2), model='TinyYOLO', conf_thresh=0.1, nms_thresh=0.5, weights=RandomWeights(seed=4),
                       max_candidates=16384, reuse_buffers=False, max_batch=2)
    files, decoded = clip_files([synthetic_frame(*size, seed=80 + i) for i in range(2)])
    want = det.detect_batch(decoded)
    assert sum(len(d) for d in want) > 0
    for got, ref in zip(det.detect_batch([JPEGFrame(d) for d in files]), want):
        _same(got, ref)
    for d, ref in zip(files, want):                 # one frame at a time: __call__ and prefetch
        f = JPEGFrame(d)
        _same(det(f), ref)
        det.prefetch(f)
        det.detect_async(f)
        _same(det.postprocess(), ref)


@pytest.mark.parametrize('mode', ['steps', 'next_frame', 'lookahead2'])
def test_mot_on_jpeg_frames_equals_bgr(ctx, mode):
    from synthetic import SyntheticVideo
    from fastmot_amd import Track
    size = (960, 540)
    video = SyntheticVideo(size, n_ids=10, n_frames=13)
    files, decoded = clip_files(video.frames)
    sources = {'jpeg': [JPEGFrame(d) for d in files], 'bgr': decoded}
    runs = {}
    for kind, frames in sources.items():
        if mode == 'lookahead2':
            from test_mot_lookahead_gpu import build_mot, run_steps
            runs[kind] = run_steps(ctx, build_mot(size, video, 2), frames, 2)
            continue
        from test_mot_gpu import build_mot
        mot = build_mot(size, video, 1)
        Track._count = 0
        mot.reset(1 / 30.)
        rows = []
        for f in range(video.n_frames):
            mot.detector._frame_idx = f
            nxt = frames[f + 1] if mode == 'next_frame' and f + 1 < video.n_frames else None
            mot.step(frames[f], next_frame=nxt)
            rows.append([(t.trk_id, tuple(t.tlbr), t.confirmed, t.active, t.age, t.hits) for t in mot.tracker.tracks.values()])
        mot.tracker._clear_tracks()
        runs[kind] = rows
    assert runs['jpeg'] == runs['bgr']              # ids, boxes and the order of the dict
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
        mot.step(JPEGFrame(clip_files(video.frames)[0][0]))
    mot.tracker._clear_tracks()


def test_videoio_and_frame_loop(ctx, tmp_path):
    """An image sequence with one progressive JPEG and one PNG in the middle: gpu_decode yields JPEGFrames except at
    those two files, the frame loop writes the same result rows either way, a size that forces a resize or an output
    being written keeps every frame an ndarray."""
    from PIL import Image
    from synthetic import SyntheticVideo
    from fastmot_amd import Track, VideoIO
    from fastmot_amd.readahead import track_stream
    from test_mot_gpu import build_mot
    size = (960, 540)
    video = SyntheticVideo(size, n_ids=10, n_frames=10)
    # (Pillow finds the format from the content, so the PNG may carry the sequence's .jpg name)
    for i, f in enumerate(video.frames):
        im = Image.fromarray(np.ascontiguousarray(f[:, :, ::-1]))
        path = tmp_path / f'{i + 1:06d}.jpg'
        if i == 4:
            im.save(path, 'PNG')
        else:
            im.save(path, 'JPEG', quality=90, progressive=(i == 3))
    uri = str(tmp_path / '%06d.jpg')

    def frames_of(stream):
        stream.start_capture()
        out = []
        try:
            while True:
                f = stream.read()
                if f is None:
                    return out
                out.append(f)
        finally:
            stream.release()

    host = frames_of(VideoIO(size, uri, buffer_size=4))
    assert len(host) == 10 and all(isinstance(f, np.ndarray) for f in host)
    stream = VideoIO(size, uri, buffer_size=4, gpu_decode=True)
    assert stream.resolution == size and not stream.do_resize
    gpu = frames_of(stream)
    assert [isinstance(f, JPEGFrame) for f in gpu] == [i not in (3, 4) for i in range(10)]
    configure(ctx, *size)
    for g, want in zip(gpu, host):
        if isinstance(g, JPEGFrame):
            ctx.frame_upload(g)
            g = ctx.frame_read()
        assert np.array_equal(g, want)
    small = frames_of(VideoIO((480, 270), uri, buffer_size=4, gpu_decode=True))        # every frame needs a resize
    assert len(small) == 10 and all(isinstance(f, np.ndarray) and f.shape == (270, 480, 3) for f in small)
    written = VideoIO(size, uri, str(tmp_path / 'out' / '%06d.png'), buffer_size=4, gpu_decode=True)
    assert all(isinstance(f, np.ndarray) for f in frames_of(written))

    rows = []
    for gpu_decode in (False, True):
        mot = build_mot(size, video, 1)
        Track._count = 0
        mot.reset(1 / 30.)
        mot.detector._frame_idx = 0
        stream = VideoIO(size, uri, buffer_size=4, gpu_decode=gpu_decode)
        stream.start_capture()
        txt = io.StringIO()
        try:
            assert track_stream(stream, mot, txt=txt, resize_to=size) == 10
        finally:
            stream.release()
        mot.tracker._clear_tracks()
        rows.append(txt.getvalue())
    assert rows[0] == rows[1] and rows[0].count('\n') > 20
