"""GPU: frames at capture resolution (fm_frame_upload_src / fm_frame_upload_ahead_src / fm_frame_ring_store_src,
csrc/resize.hip).  The resize is integer arithmetic, so every comparison is np.array_equal between ctx.frame_read() and
videoio.resize_bgr of the same pixels; the detector, MOT.step and the frame loop must give, on SourceFrames, exactly what
they give on the ndarrays resize_bgr makes of them."""
import ctypes as C
import io

import numpy as np
import pytest

import jpeg_cases as jc
from fastmot_amd import JPEGFrame, NV12Frame, SourceFrame, _lib
from fastmot_amd.utils import jpeg as J
from fastmot_amd.utils import source as S
from fastmot_amd.utils.nv12 import nv12_to_bgr
from fastmot_amd.videoio import resize_bgr

pytestmark = pytest.mark.gpu

FM_ERR_ARG = -2


def configure(ctx, w, h, ring=0):
    ctx.frame_configure(w, h, ring)
    ctx.next_frame, ctx.ahead_frames, ctx.bound_frame = None, [], None


def random_frame(rng, w, h):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


# (source, frame): every path of the kernel -- see the ids
KERNEL_CASES = [
    ((37, 23), (16, 10), 'down-8-byte-stores'),
    ((37, 23), (19, 11), 'down-byte-path-odd'),
    ((64, 48), (32, 24), 'mean-2x2'),
    ((64, 48), (32, 23), '2x-in-one-axis-is-not-the-mean'),
    ((20, 12), (32, 18), 'up'),
    ((24, 40), (40, 24), 'one-axis-up-one-down'),
    ((8, 8), (8, 6), 'one-axis-unchanged'),
    ((1, 1), (8, 6), 'source-1x1'),
    ((2, 1), (8, 6), 'source-2x1'),
    ((66, 50), (33, 25), 'mean-2x2-byte-path'),
    ((1920, 1080), (1280, 720), 'full-size'),
    ((3840, 2160), (1920, 1080), 'full-size-mean-2x2'),
]


@pytest.mark.parametrize('src,dst', [c[:2] for c in KERNEL_CASES], ids=[c[2] for c in KERNEL_CASES])
def test_kernel_equals_resize_bgr(ctx, src, dst):
    img = random_frame(np.random.default_rng(src[0] * 7 + dst[1]), *src)
    configure(ctx, *dst)
    try:
        ctx.frame_upload(SourceFrame(img))
        got = ctx.frame_read()
    finally:
        if dst[0] > 100:
            configure(ctx, 16, 16)          # (gives the full-size buffers back)
    assert got.shape == (dst[1], dst[0], 3)
    assert np.array_equal(got, resize_bgr(img, dst))


def test_value_extremes(ctx):
    """A 256 -> 255 ramp pair (every byte value beside its successor, rising and falling, under nearly every fraction) and a
    constant-255 frame: the clamp and the >> 4 / >> 16 truncations at their extremes."""
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    pair = np.concatenate([ramp, ramp[:, ::-1]], 0)                # (2, 256, 3)
    pair[:, :, 1] = 255 - pair[:, :, 1]
    configure(ctx, 255, 2)
    ctx.frame_upload(SourceFrame(pair))
    assert np.array_equal(ctx.frame_read(), resize_bgr(pair, (255, 2)))
    for src, dst in (((37, 23), (16, 10)), ((32, 20), (16, 10)), ((5, 3), (16, 10))):
        white = np.full((src[1], src[0], 3), 255, np.uint8)
        configure(ctx, *dst)
        ctx.frame_upload(SourceFrame(white))
        got = ctx.frame_read()
        assert np.array_equal(got, resize_bgr(white, dst)) and (got == 255).all()


@pytest.mark.parametrize('pinned', [False, True], ids=['pageable', 'pinned'])
def test_every_destination(ctx, pinned):
    src, dst = (37, 23), (16, 10)
    rng = np.random.default_rng(11)
    configure(ctx, *dst, 3)
    n = 8
    if pinned:
        imgs = ctx.pinned_source_frames(n, src)
        assert imgs.shape == (n, 23, 37, 3) and imgs.dtype == np.uint8
        imgs[...] = rng.integers(0, 256, imgs.shape, dtype=np.uint8)
    else:
        imgs = rng.integers(0, 256, (n, 23, 37, 3), dtype=np.uint8)
    want = [resize_bgr(i, dst) for i in imgs]
    frames = [SourceFrame(i) for i in imgs]
    plain = [random_frame(rng, *dst) for _ in range(3)]

    ctx.frame_upload(frames[0])
    assert np.array_equal(ctx.frame_read(), want[0])
    ctx.frame_upload_next(frames[1])
    ctx.frame_promote_next()
    assert np.array_equal(ctx.frame_read(), want[1])
    ctx.frame_upload_next(frames[2])
    ctx.frame_upload_ahead(2, frames[3])
    for i in (2, 3):
        ctx.frame_promote_next()
        assert np.array_equal(ctx.frame_read(), want[i]), i
    # all four look-ahead slots, twice: the second round finds every slot's buffers in use; plain frames in between
    for base in (0, 4):
        for k in range(1, _lib.FM_MAX_DET_BATCH + 1):
            ctx.frame_upload_ahead(k, frames[base + k - 1])
        for k in range(1, _lib.FM_MAX_DET_BATCH + 1):
            ctx.frame_promote_next()
            assert np.array_equal(ctx.frame_read(), want[base + k - 1]), (base, k)
        ctx.frame_upload_next(plain[0])
        ctx.frame_promote_next()
        assert np.array_equal(ctx.frame_read(), plain[0])
    # the ring: a source frame into index 1 of 3 leaves its neighbours as they were
    for i in range(3):
        ctx.frame_ring_store(i, plain[i])
    ctx.frame_ring_store(1, frames[5])
    for i, w in enumerate((plain[0], want[5], plain[2])):
        ctx.frame_ring_select(i)
        assert np.array_equal(ctx.frame_read(), w), i


def nv12_source(rng, w, h, pitch):
    surface = rng.integers(0, 256, (h + h // 2, pitch), dtype=np.uint8)
    y, uv = surface[:h, :w], surface[h:, :w]
    return NV12Frame(y, uv), nv12_to_bgr(y, uv)


def test_every_kind(ctx):
    rng = np.random.default_rng(12)
    dst = (32, 18)
    configure(ctx, *dst, 1)
    cases = []
    nv, bgr = nv12_source(rng, 40, 24, 48)
    cases.append(('nv12 40x24 pitch 48', SourceFrame(nv), resize_bgr(bgr, dst)))
    nv, bgr = nv12_source(rng, 64, 36, 64)                            # the 2 x 2 mean behind the conversion
    cases.append(('nv12 64x36', SourceFrame(nv), resize_bgr(bgr, dst)))
    for size in ((40, 24), (37, 23)):
        for sub in ('420', '444'):
            data = jc.encode(jc.content('noise', *size, seed=size[0]), sub, 90)
            cases.append((f'jpeg {size} {sub}', SourceFrame(JPEGFrame(data)), resize_bgr(J.decode_bgr(data), dst)))
            assert np.array_equal(J.decode_bgr(data), jc.pillow_bgr(data))
    img = random_frame(rng, 40, 24)
    cases.append(('bgr', SourceFrame(img), resize_bgr(img, dst)))
    # every kind through every destination, the kinds following each other through the same staging
    for label, frame, want in cases:
        ctx.frame_upload(frame)
        assert np.array_equal(ctx.frame_read(), want), (label, 'upload')
    for label, frame, want in cases:
        ctx.frame_upload_next(frame)
        ctx.frame_promote_next()
        assert np.array_equal(ctx.frame_read(), want), (label, 'ahead')
    for label, frame, want in cases:
        ctx.frame_ring_store(0, frame)
        ctx.frame_ring_select(0)
        assert np.array_equal(ctx.frame_read(), want), (label, 'ring')


def test_regrow_and_equal_size(ctx):
    rng = np.random.default_rng(13)
    dst = (16, 10)
    configure(ctx, *dst, 1)
    for through in ('upload', 'ahead', 'ring'):
        for src in ((37, 23), (64, 48), (37, 23)):
            img = random_frame(rng, *src)
            if through == 'upload':
                ctx.frame_upload(SourceFrame(img))
            elif through == 'ahead':
                ctx.frame_upload_next(SourceFrame(img))
                ctx.frame_promote_next()
            else:
                ctx.frame_ring_store(0, SourceFrame(img))
                ctx.frame_ring_select(0)
            assert np.array_equal(ctx.frame_read(), resize_bgr(img, dst)), (through, src)
    # JPEG staging grows as well
    for size in ((24, 16), (70, 40), (24, 16)):
        data = jc.encode(jc.content('noise', *size), '420', 85)
        ctx.frame_upload_next(SourceFrame(JPEGFrame(data)))
        ctx.frame_promote_next()
        assert np.array_equal(ctx.frame_read(), resize_bgr(jc.pillow_bgr(data), dst)), size
    # a source of the frame size is the plain upload
    img = random_frame(rng, *dst)
    nv, nv_bgr = nv12_source(rng, 16, 10, 16)
    data = jc.encode(jc.content('noise', *dst), '420', 85)
    for frame, want in ((img, img), (nv, nv_bgr), (JPEGFrame(data), jc.pillow_bgr(data))):
        for method in ('upload', 'ahead', 'ring'):
            got = []
            for f in (frame, SourceFrame(frame)):
                if method == 'upload':
                    ctx.frame_upload(f)
                elif method == 'ahead':
                    ctx.frame_upload_next(f)
                    ctx.frame_promote_next()
                else:
                    ctx.frame_ring_store(0, f)
                    ctx.frame_ring_select(0)
                got.append(ctx.frame_read())
            assert np.array_equal(got[0], want) and np.array_equal(got[1], want), method
    # a new frame size frees the staging; the path works again afterwards
    configure(ctx, 19, 11)
    img = random_frame(rng, 37, 23)
    ctx.frame_upload(SourceFrame(img))
    assert np.array_equal(ctx.frame_read(), resize_bgr(img, (19, 11)))


def test_refusals(ctx):
    lib = ctx.lib
    dst = (16, 10)
    configure(ctx, *dst, 1)
    rng = np.random.default_rng(14)
    before = random_frame(rng, *dst)
    ctx.frame_upload(before)
    ctx.frame_ring_store(0, before)
    c = C.c_int
    img = random_frame(rng, 37, 23)
    good = SourceFrame(img)
    surface = rng.integers(0, 256, (36, 48), dtype=np.uint8)
    jp = JPEGFrame(jc.encode(jc.content('noise', 40, 24), '420', 75))

    def desc(**kw):
        d = S.FrameSrc.from_buffer_copy(good.describe())
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def nv12(w, h, pitch=48, matrix=0):
        return desc(kind=S.FM_SRC_NV12, width=w, height=h, y=surface.ctypes.data, uv=surface.ctypes.data + 24 * 48, pitch=pitch, matrix=matrix)

    def jpeg(w, h, info=None, **kw):
        d = desc(kind=S.FM_SRC_JPEG, width=w, height=h, info=C.pointer(jp.info if info is None else info),
                 coef=jp.coef.ctypes.data, qt=jp.qt.ctypes.data)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def without(d, field):
        setattr(d, field, None)
        return d

    tampered = J.JpegInfo.from_buffer_copy(jp.info)
    tampered.coef_count += 64
    bad = [desc(kind=3), desc(kind=-1), desc(width=0), desc(height=0), desc(width=-5), desc(width=S.MAX_DIM + 1),
           desc(height=S.MAX_DIM + 1), desc(bgr=None),
           nv12(39, 24), nv12(40, 23), nv12(40, 24, pitch=38), nv12(40, 24, matrix=2), without(nv12(40, 24), 'y'), without(nv12(40, 24), 'uv'),
           jpeg(37, 23), jpeg(40, 25), jpeg(40, 24, tampered), jpeg(40, 24, coef=None), jpeg(40, 24, qt=None),
           without(jpeg(40, 24), 'info')]
    keep = [jp, surface, tampered, img]                               # (what the descriptions point into)
    calls = [lambda d: lib.fm_frame_upload_src(ctx.handle, d),
             lambda d: lib.fm_frame_upload_ahead_src(ctx.handle, c(1), d),
             lambda d: lib.fm_frame_ring_store_src(ctx.handle, c(0), d)]
    for call in calls:
        for i, d in enumerate(bad):
            assert call(C.byref(d)) == FM_ERR_ARG, i
            assert b'bad argument' in lib.fm_last_error()
        assert call(None) == FM_ERR_ARG
    for d in (good.describe(), nv12(40, 24), jpeg(40, 24)):           # each of these is a valid source ...
        for k in (0, _lib.FM_MAX_DET_BATCH + 1):                       # ... refused for the slot
            assert lib.fm_frame_upload_ahead_src(ctx.handle, c(k), C.byref(d)) == FM_ERR_ARG
        for index in (-1, 1):
            assert lib.fm_frame_ring_store_src(ctx.handle, c(index), C.byref(d)) == FM_ERR_ARG
    with pytest.raises(_lib.FastMOTHipError):
        ctx.frame_upload_ahead(5, good)
    with pytest.raises(_lib.FastMOTHipError):                     # no frame in slot 1: none of the calls above put one there
        ctx.frame_promote_next()
    assert np.array_equal(ctx.frame_read(), before)                   # nothing was copied or launched
    ctx.frame_ring_select(0)
    assert np.array_equal(ctx.frame_read(), before)
    with pytest.raises(ValueError):
        NV12Frame(surface[:23, :39], surface[24:35, :39])             # an odd NV12 source never becomes a SourceFrame
    with pytest.raises(ValueError):
        SourceFrame(np.zeros((0, 16, 3), np.uint8))
    for d, want in ((nv12(40, 24), resize_bgr(nv12_to_bgr(surface[:24, :40], surface[24:, :40]), dst)),
                    (jpeg(40, 24), resize_bgr(jp.to_bgr(), dst)), (good.describe(), resize_bgr(img, dst))):
        assert lib.fm_frame_upload_src(ctx.handle, C.byref(d)) == 0   # and the calls still work
        assert np.array_equal(ctx.frame_read(), want)
    del keep


# ------------------------------------------------------------------------------------------------------ end to end
class ScaledVideo:
    """A SyntheticVideo rendered at `ratio` times the tracker's size; its scripted detections in the tracker's coordinates."""

    def __init__(self, video, ratio):
        self.video, self.ratio = video, ratio
        self.frames, self.n_frames, self.n_ids = video.frames, video.n_frames, video.n_ids

    def detections(self, frame_idx, label=1, labels=None):
        dets = self.video.detections(frame_idx, label, labels)
        dets.tlbr = np.rint(dets.tlbr / self.ratio)
        return dets


SIZE = (960, 540)
_clips = {}


def clip(ratio):
    """(video in tracker coordinates, capture-resolution frames, the same frames resized on the host); made once."""
    if ratio not in _clips:
        from synthetic import SyntheticVideo
        src = (int(SIZE[0] * ratio), int(SIZE[1] * ratio))
        video = ScaledVideo(SyntheticVideo(src, n_ids=10, n_frames=11, seed=21), ratio)
        _clips[ratio] = (video, video.frames, [resize_bgr(f, SIZE) for f in video.frames])
    return _clips[ratio]


def run_mot(mot, frames, mode):
    from fastmot_amd import Track
    Track._count = 0
    mot.reset(1 / 30.)
    rows = []
    for f in range(len(frames)):
        mot.detector._frame_idx = f
        if mode == 'lookahead2':
            mot.step(frames[f], next_frames=frames[f + 1:f + 3])
        else:
            mot.step(frames[f], next_frame=frames[f + 1] if mode == 'next_frame' and f + 1 < len(frames) else None)
        real = mot.detector.last_real                              # the network's own output: it read the resized frame
        rows.append(([(t.trk_id, tuple(t.tlbr), t.confirmed, t.active, t.age, t.hits) for t in mot.tracker.tracks.values()],
                     real.tlbr.tolist(), real.conf.tolist()))
    mot.tracker._clear_tracks()
    return rows


@pytest.mark.parametrize('mode', ['steps', 'next_frame', 'lookahead2'])
@pytest.mark.parametrize('ratio', [2, 1.5], ids=['2x', '1.5x'])
def test_mot_on_source_frames_equals_resized(ctx, ratio, mode):
    video, captured, resized = clip(ratio)
    runs = []
    for frames in ([SourceFrame(f) for f in captured], resized):
        if mode == 'lookahead2':
            from test_mot_lookahead_gpu import build_mot
            mot = build_mot(SIZE, video, 2)
        else:
            from test_mot_gpu import build_mot
            mot = build_mot(SIZE, video, 1)
        runs.append(run_mot(mot, frames, mode))
    assert runs[0] == runs[1]                                       # ids, boxes, the order of the dict, the detector's rows
    assert len(runs[1][-1][0]) >= 8


def test_draw_needs_host_pixels(ctx):
    from test_mot_gpu import build_mot
    video, captured, _ = clip(2)
    mot = build_mot(SIZE, video, 1)
    mot.draw = True
    mot.reset(1 / 30.)
    with pytest.raises(ValueError, match='host pixels'):
        mot.step(SourceFrame(captured[0]))
    mot.tracker._clear_tracks()


def test_detector_on_source_frames_equals_resized(ctx):
    from fastmot_amd.detector import YOLODetector
    from fastmot_amd.models.graph import RandomWeights
    from test_detect_batch_gpu import _same
    from test_detect_gpu import TinyYOLO, synthetic_frame  # noqa: F401  (registers the tiny model)
    size = (320, 180)
    det = YOLODetector(size, (0, 1, 2), model='TinyYOLO', conf_thresh=0.1, nms_thresh=0.5, weights=RandomWeights(seed=4),
                       max_candidates=16384, reuse_buffers=False, max_batch=2)
    captured = [synthetic_frame(480, 270, seed=80 + i) for i in range(2)]
    want = det.detect_batch([resize_bgr(f, size) for f in captured])
    assert sum(len(d) for d in want) > 0
    frames = [SourceFrame(f) for f in captured]
    for got, ref in zip(det.detect_batch(frames), want):
        _same(got, ref)
    for f, ref in zip(frames, want):                # one frame at a time: __call__ and prefetch
        _same(det(f), ref)
        det.prefetch(f)
        det.detect_async(f)
        _same(det.postprocess(), ref)


def test_videoio_frame_loop(ctx, tmp_path):
    """JPEG files of the 1.5x clip: gpu_resize + gpu_decode hand every frame over as a SourceFrame of a JPEGFrame, and the
    frame loop writes the result file it writes from Pillow-decoded, host-resized frames."""
    from fastmot_amd import VideoIO
    from fastmot_amd.readahead import track_stream
    from test_mot_gpu import build_mot
    video, captured, _ = clip(1.5)
    for i, f in enumerate(captured):
        (tmp_path / f'{i + 1:06d}.jpg').write_bytes(jc.encode(np.ascontiguousarray(f[:, :, ::-1]), '420', 90))
    uri = str(tmp_path / '%06d.jpg')
    results = []
    for on in (False, True):
        mot = build_mot(SIZE, video, 1)
        from fastmot_amd import Track
        Track._count = 0
        mot.reset(1 / 30.)
        mot.detector._frame_idx = 0
        stream = VideoIO(SIZE, uri, buffer_size=4, gpu_resize=on, gpu_decode=on)
        kinds = set()
        read = stream.read

        def noting_read():
            f = read()
            if f is not None:
                kinds.add(type(f.frame).__name__ if isinstance(f, SourceFrame) else 'host ' + type(f).__name__)
            return f
        stream.read = noting_read
        stream.start_capture()
        txt = io.StringIO()
        try:
            assert track_stream(stream, mot, txt=txt, resize_to=SIZE) == len(captured)
        finally:
            stream.release()
        mot.tracker._clear_tracks()
        assert kinds == ({'JPEGFrame'} if on else {'host ndarray'})
        results.append(txt.getvalue())
    assert results[0] == results[1] and results[0].count('\n') > 20
