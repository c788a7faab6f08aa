"""GPU: Bayer ingest (fm_frame_upload_bayer / fm_frame_upload_ahead_bayer / fm_frame_ring_store_bayer), csrc/bayer.hip.
The demosaicing is integer arithmetic, so every comparison is np.array_equal against fastmot_amd.utils.bayer (pinned by
a float64 statement in test_bayer_host.py).

The kernel's tile is 128 x 16 output pixels with a 2-sample halo.  Sizes: 2x2 (a frame that is all halo), 3x5 and 4x3
(reflection lands on both parities), 34x18 (3 W = 102: rows that begin 8-byte aligned, 4-byte aligned and neither, so
all three store paths; two tiles down), 33x7 (odd: every source row at another alignment), 130x6 (a second tile that
begins inside a row, 2 pixels wide), 1920x2 (15 tiles a row, everything aligned), 12x35 (three tiles down: halos that
come from the neighbouring tile), 257x33 (three tiles each way, odd)."""
import ctypes as C

import numpy as np
import pytest

from fastmot_amd import BayerFrame, SourceFrame, _lib
from fastmot_amd.utils.bayer import METHODS, PATTERNS, bayer_to_bgr, colour_planes, mosaic
from fastmot_amd.videoio import resize_bgr

pytestmark = pytest.mark.gpu

FM_ERR_ARG = -2
SIZES = [(2, 2), (3, 5), (4, 3), (34, 18), (33, 7), (130, 6), (1920, 2), (12, 35), (257, 33)]
ids = lambda s: f'{s[0]}x{s[1]}'
WB, BLACK = (1.7, 0.9, 2.3), 9          # non-default gains and black level


def configure(ctx, w, h, ring=0):
    ctx.frame_configure(w, h, ring)
    ctx.next_frame, ctx.ahead_frames, ctx.bound_frame = None, [], None


def make(ctx, rng, w, h, pattern, depth=8, method='mhc', wb=(1., 1., 1.), black=0, pad=0, pinned=False, samples=None):
    """A mosaic of random samples whose rows lie `pad` samples further apart than their width (the padding random too),
    in fm_host_alloc memory when `pinned`; the first row all 0 and the last all 2^depth - 1."""
    dtype = np.uint8 if depth == 8 else np.uint16
    buf = _lib.pinned_empty(ctx.lib, (h, w + pad), dtype) if pinned else np.empty((h, w + pad), dtype)
    buf[...] = rng.integers(0, 1 << depth, buf.shape).astype(dtype)
    buf[0, :w], buf[-1, :w] = 0, (1 << depth) - 1
    if samples is not None:
        buf[:, :w] = samples
    return BayerFrame(buf[:, :w], pattern, None, depth, method, wb, black)


def combos():
    """Every (pattern, method) at depth 8 with default and non-default gains / black; every other depth with both methods
    and non-default gains, the patterns taking turns."""
    out = [(p, 8, m, wb, black) for p in PATTERNS for m in METHODS for wb, black in (((1., 1., 1.), 0), (WB, BLACK))]
    names = sorted(PATTERNS)
    for i, depth in enumerate((10, 12, 14, 16)):
        for j, m in enumerate(METHODS):
            out.append((names[(i + 2 * j) % 4], depth, m, (1.2, 1., 16.) if j else (0.5, 1.1, 1.), (1 << depth) // 16 * j))
    return out


@pytest.mark.parametrize('size', SIZES, ids=ids)
def test_upload_equals_bayer_to_bgr(ctx, size):
    w, h = size
    rng = np.random.default_rng(w * 131 + h)
    configure(ctx, w, h)
    for pattern, depth, method, wb, black in combos():
        for pad in (0, 5):
            for pinned in (False, True):
                f = make(ctx, rng, w, h, pattern, depth, method, wb, black, pad, pinned)
                assert f.pitch == (w + pad) * (1 if depth == 8 else 2)
                ctx.frame_upload(f)
                assert np.array_equal(ctx.frame_read(), f.to_bgr()), (pattern, depth, method, wb, black, pad, pinned)
    for depth in (8, 12):
        f = ctx.pinned_bayer_frames(1, 'gbrg', depth, method='bilinear', wb=WB, black=BLACK)[0]
        assert f.size == (w, h) and f.pitch == w * (1 if depth == 8 else 2) and f.rows.dtype == (np.uint8 if depth == 8 else np.uint16)
        f.rows[...] = rng.integers(0, 1 << depth, f.rows.shape).astype(f.rows.dtype)
        ctx.frame_upload(f)
        assert np.array_equal(ctx.frame_read(), bayer_to_bgr(f.rows, size, 'gbrg', depth, 'bilinear', WB, BLACK))


def test_phase_checkerboards(ctx):
    """One colour's positions 255 and the rest 0, and the inverse, at 34x18."""
    w, h = 34, 18
    rng = np.random.default_rng(7)
    configure(ctx, w, h)
    for pattern in PATTERNS:
        for mask in colour_planes((w, h), pattern):
            for board in (np.where(mask, 255, 0), np.where(mask, 0, 255)):
                for method in METHODS:
                    f = make(ctx, rng, w, h, pattern, method=method, pad=3, samples=board.astype(np.uint8))
                    ctx.frame_upload(f)
                    assert np.array_equal(ctx.frame_read(), f.to_bgr()), (pattern, method)


@pytest.mark.parametrize('size', SIZES, ids=ids)
def test_other_entry_points(ctx, size):
    w, h = size
    rng = np.random.default_rng(w * 137 + h)
    configure(ctx, w, h, 2)
    for i, (pattern, depth, method, wb, black) in enumerate(combos()):
        a, b, c = (make(ctx, rng, w, h, pattern, depth, method, wb, black, pad, pinned)
                   for pad, pinned in ((0, bool(i & 1)), (3, False), (3, True)))
        ctx.frame_upload_ahead(1, a)
        ctx.frame_upload_ahead(2, b)
        for f in (a, b):
            ctx.frame_promote_next()
            assert np.array_equal(ctx.frame_read(), f.to_bgr()), (pattern, depth, method, 'ahead')
        ctx.frame_upload_next(c)
        ctx.frame_promote_next()
        assert np.array_equal(ctx.frame_read(), c.to_bgr()), (pattern, depth, method, 'next')
        ctx.frame_ring_store(1, b)
        ctx.frame_ring_store(0, a)
        for k, f in enumerate((a, b)):
            ctx.frame_ring_select(k)
            assert np.array_equal(ctx.frame_read(), f.to_bgr()), (pattern, depth, method, 'ring', k)


@pytest.mark.parametrize('src,dst', [((40, 24), (20, 12)), ((37, 21), (34, 18))], ids=['exact2x', 'linear'])
def test_source_frame_of_another_size(ctx, src, dst):
    rng = np.random.default_rng(src[0])
    configure(ctx, dst[0], dst[1], 1)
    for i, (pattern, depth, method, wb, black) in enumerate(combos()):
        for pad in (0, 3):
            f = make(ctx, rng, src[0], src[1], pattern, depth, method, wb, black, pad, pinned=bool(i & 1))
            want = resize_bgr(f.to_bgr(), dst)
            ctx.frame_upload(SourceFrame(f))
            assert np.array_equal(ctx.frame_read(), want), (pattern, depth, method, pad, 'upload')
            for k in (1, 2):
                ctx.frame_upload_ahead(k, SourceFrame(f))
            for k in (1, 2):
                ctx.frame_promote_next()
                assert np.array_equal(ctx.frame_read(), want), (pattern, depth, method, pad, 'ahead', k)
            ctx.frame_ring_store(0, SourceFrame(f))
            ctx.frame_ring_select(0)
            assert np.array_equal(ctx.frame_read(), want), (pattern, depth, method, pad, 'ring')
    for call in (ctx.frame_upload, ctx.frame_upload_next, lambda x: ctx.frame_upload_ahead(2, x), lambda x: ctx.frame_ring_store(0, x)):
        with pytest.raises(ValueError):                          # a bare BayerFrame of another size is not resized silently
            call(f)
    on_size = make(ctx, rng, dst[0], dst[1], 'grbg', 12, wb=WB, black=BLACK)
    ctx.frame_upload(SourceFrame(on_size))                       # a SourceFrame of the configured size is the plain upload
    assert np.array_equal(ctx.frame_read(), on_size.to_bgr())


def test_bad_arguments(ctx):
    lib = ctx.lib
    w, h = 16, 6
    configure(ctx, w, h, 1)
    rng = np.random.default_rng(3)
    before = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    ctx.frame_upload(before)
    ctx.frame_ring_store(0, before)
    good = make(ctx, rng, w, h, 'grbg', wb=WB, black=BLACK)
    deep = make(ctx, rng, w, h, 'bggr', 12, 'bilinear', black=4095)
    c = C.c_int

    def desc(of=good, **kw):
        d = type(of.describe()).from_buffer_copy(of.describe())
        for k, v in kw.items():
            setattr(d, k, v)
        return C.byref(d)

    calls = [lambda d: lib.fm_frame_upload_bayer(ctx.handle, d),
             lambda d: lib.fm_frame_upload_ahead_bayer(ctx.handle, c(1), d),
             lambda d: lib.fm_frame_ring_store_bayer(ctx.handle, c(0), d)]
    bad = [dict(data=None), dict(pattern=-1), dict(pattern=4), dict(method=-1), dict(method=2), dict(depth=0), dict(depth=7), dict(depth=9),
           dict(depth=11), dict(depth=18), dict(depth=32), dict(depth=-8), dict(width=1), dict(height=1), dict(width=0), dict(height=0),
           dict(width=-4), dict(width=16385), dict(height=16385), dict(pitch=w - 1), dict(pitch=0), dict(pitch=-w),
           dict(of=deep, pitch=2 * w - 1), dict(depth=10), dict(gain_r=0), dict(gain_g=0), dict(gain_b=0), dict(gain_r=4097), dict(gain_g=4097),
           dict(gain_b=4097), dict(gain_g=-256), dict(black=-1), dict(black=256), dict(of=deep, black=4096), dict(of=deep, depth=10)]
    for call in calls:
        for kw in bad:
            assert call(desc(**kw)) == FM_ERR_ARG, kw
            assert b'bad argument' in lib.fm_last_error()
        assert call(None) == FM_ERR_ARG
    for k in (0, _lib.FM_MAX_DET_BATCH + 1):
        assert lib.fm_frame_upload_ahead_bayer(ctx.handle, c(k), desc()) == FM_ERR_ARG
    for index in (-1, 1):
        assert lib.fm_frame_ring_store_bayer(ctx.handle, c(index), desc()) == FM_ERR_ARG
    with pytest.raises(_lib.FastMOTHipError):                    # no frame in slot 1: none of the calls above put one there
        ctx.frame_promote_next()
    assert np.array_equal(ctx.frame_read(), before)              # nothing was copied or launched
    ctx.frame_ring_select(0)
    assert np.array_equal(ctx.frame_read(), before)
    # the same descriptions, unmodified, are accepted -- and the extremes of every range
    assert lib.fm_frame_upload_bayer(ctx.handle, desc()) == 0
    assert np.array_equal(ctx.frame_read(), good.to_bgr())
    assert lib.fm_frame_upload_bayer(ctx.handle, desc(of=deep)) == 0
    assert np.array_equal(ctx.frame_read(), deep.to_bgr())
    assert lib.fm_frame_upload_bayer(ctx.handle, desc(gain_r=1, gain_g=4096, gain_b=4096, black=255)) == 0
    assert np.array_equal(ctx.frame_read(), BayerFrame(good.data, 'grbg', wb=(1 / 256, 16, 16), black=255).to_bgr())


# ---- MOT.step
def test_tracks_on_bayer_frames_equal_bgr_frames(ctx):
    """The demosaiced frames are not the original ones (demosaicing is lossy): the tracker is compared on the pixels
    `to_bgr()` states, which is what the device frame holds."""
    from synthetic import SyntheticVideo
    from test_packed_gpu import SIZE, run_mot
    video = SyntheticVideo(SIZE, n_ids=8, n_frames=8, seed=4)
    raw = [mosaic(np.ascontiguousarray(f), 'rggb') for f in video.frames]
    eight = [BayerFrame(m, 'rggb') for m in raw]
    twelve = [BayerFrame(m.astype(np.uint16) << 4, 'rggb', depth=12) for m in raw]
    bgr = [f.to_bgr() for f in eight]
    assert not np.array_equal(bgr[0], video.frames[0])
    assert all(np.array_equal(f.to_bgr(), b) for f, b in zip(twelve, bgr))      # (s << 4 at depth 12 prepares to s)
    want = run_mot(video, bgr)
    assert len(want[-1]) >= 6                # (the detections follow the scene, whatever the pixels: as in the packed test)
    assert run_mot(video, eight) == want
    assert run_mot(video, twelve) == want


def test_draw_refuses_bayer_frames(ctx):
    from synthetic import SyntheticVideo
    from test_mot_gpu import build_mot
    from test_packed_gpu import SIZE
    video = SyntheticVideo(SIZE, n_ids=2, n_frames=1, seed=4)
    mot = build_mot(SIZE, video, 1)
    mot.draw = True
    mot.reset(1 / 30.)
    try:
        with pytest.raises(TypeError):
            mot.step(BayerFrame(mosaic(video.frames[0], 'rggb'), 'rggb'))
    finally:
        mot.tracker._clear_tracks()
