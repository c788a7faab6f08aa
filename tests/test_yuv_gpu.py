"""GPU: planar YCbCr ingest (fm_frame_upload_planar / fm_frame_upload_ahead_planar / fm_frame_ring_store_planar) and the
I420 export (fm_frame_export_i420 / fm_i420_from_bgr), csrc/yuv.hip.  Both conversions are integer arithmetic, so every
comparison is np.array_equal against fastmot_amd.utils.yuv (pinned by NV12's functions and by hand in test_yuv_host.py).

Sizes: 1 and 2 (a single thread, no row pair), 3x5 / 7x3 / 9x2 (odd chroma width, a last row without a partner, a second
thread of one pixel), 8x8 (the aligned 8-byte path alone), 17x9 and 33x31 (whole runs beside ragged ones, rows that start
at every alignment), 64x36 (everything aligned), 130x70 (more than one workgroup: 17 x 35 threads for 4:2:0)."""
import ctypes as C

import numpy as np
import pytest

import overlay_cases as cases
from fastmot_amd import PlanarFrame, SourceFrame, _lib
from fastmot_amd.utils.yuv import bgr_to_planar420, chroma_shape, planar_to_bgr
from fastmot_amd.videoio import resize_bgr

pytestmark = pytest.mark.gpu

FM_ERR_ARG = -2
SIZES = [(1, 1), (2, 2), (3, 5), (7, 3), (8, 8), (9, 2), (17, 9), (33, 31), (64, 36), (130, 70)]
CHROMAS = ['420', '422', '444', 'mono']
ids = lambda s: f'{s[0]}x{s[1]}'


def configure(ctx, w, h, ring=0):
    ctx.frame_configure(w, h, ring)
    ctx.next_frame, ctx.ahead_frames, ctx.bound_frame = None, [], None


def pitched(rng, w, h, chroma, pad, matrix='bt601', extremes=False):
    """A frame of random planes whose rows lie `pad` bytes further apart than their width (the padding random too).
    extremes: Y in {0, 15, 16, 235, 255} x U, V in {0, 128, 255} instead."""
    def plane(rows, cols, values):
        buf = rng.integers(0, 256, (rows, cols + pad), dtype=np.uint8)
        view = buf[:, :cols]
        if values is not None:
            view[...] = rng.choice(np.array(values, np.uint8), (rows, cols))
        return view
    y = plane(h, w, (0, 15, 16, 235, 255) if extremes else None)
    cs = chroma_shape((w, h), chroma)
    if cs is None:
        return PlanarFrame(y, chroma=chroma, matrix=matrix)
    c = (0, 128, 255) if extremes else None
    return PlanarFrame(y, plane(cs[0], cs[1], c), plane(cs[0], cs[1], c), chroma, matrix)


def flat(planes):
    return np.concatenate([p.reshape(-1) for p in planes])


@pytest.mark.parametrize('size', SIZES, ids=ids)
def test_upload_equals_planar_to_bgr(ctx, size):
    w, h = size
    rng = np.random.default_rng(w * 131 + h)
    configure(ctx, w, h, 1)
    for chroma in CHROMAS:
        for matrix in ('bt601', 'bt709'):
            for pad in (0, 3):
                for extremes in (False, True):
                    f = pitched(rng, w, h, chroma, pad, matrix, extremes)
                    assert f.pitch == (w + pad if h > 1 else w)
                    ctx.frame_upload(f)
                    assert np.array_equal(ctx.frame_read(), f.to_bgr()), (chroma, matrix, pad, extremes)


@pytest.mark.parametrize('size', SIZES, ids=ids)
def test_other_entry_points(ctx, size):
    w, h = size
    rng = np.random.default_rng(w * 137 + h)
    configure(ctx, w, h, 2)
    for i, chroma in enumerate(CHROMAS):
        matrix = ('bt601', 'bt709')[i & 1]
        a, b, c = (pitched(rng, w, h, chroma, pad, matrix) for pad in (0, 3, 3))
        ctx.frame_upload_ahead(1, a)
        ctx.frame_upload_ahead(2, b)
        for f in (a, b):
            ctx.frame_promote_next()
            assert np.array_equal(ctx.frame_read(), f.to_bgr()), (chroma, 'ahead')
        ctx.frame_upload_next(c)
        ctx.frame_promote_next()
        assert np.array_equal(ctx.frame_read(), c.to_bgr()), (chroma, 'next')
        ctx.frame_ring_store(1, b)
        ctx.frame_ring_store(0, a)
        for k, f in enumerate((a, b)):
            ctx.frame_ring_select(k)
            assert np.array_equal(ctx.frame_read(), f.to_bgr()), (chroma, 'ring', k)
        pinned = ctx.pinned_planar_frames(2, chroma, matrix)
        for p in pinned:
            assert p.size == (w, h) and p.pitch == w and p.chroma == chroma and p.matrix == matrix
            for plane in (p.y, p.u, p.v):
                if plane is not None:
                    plane[...] = rng.integers(0, 256, plane.shape, dtype=np.uint8)
        ctx.frame_upload(pinned[0])
        assert np.array_equal(ctx.frame_read(), pinned[0].to_bgr()), (chroma, 'pinned upload')
        ctx.frame_upload_ahead(1, pinned[1])
        ctx.frame_promote_next()
        assert np.array_equal(ctx.frame_read(), pinned[1].to_bgr()), (chroma, 'pinned ahead')


@pytest.mark.parametrize('src', [(66, 38), (128, 72)], ids=ids)
def test_source_frame_of_another_size(ctx, src):
    w, h = 64, 36
    rng = np.random.default_rng(src[0])
    configure(ctx, w, h, 1)
    for chroma in CHROMAS:
        for pad in (0, 3):
            f = pitched(rng, src[0], src[1], chroma, pad, 'bt709')
            want = resize_bgr(f.to_bgr(), (w, h))
            ctx.frame_upload(SourceFrame(f))
            assert np.array_equal(ctx.frame_read(), want), (chroma, pad, 'upload')
            ctx.frame_upload_ahead(1, SourceFrame(f))
            ctx.frame_promote_next()
            assert np.array_equal(ctx.frame_read(), want), (chroma, pad, 'ahead')
            ctx.frame_ring_store(0, SourceFrame(f))
            ctx.frame_ring_select(0)
            assert np.array_equal(ctx.frame_read(), want), (chroma, pad, 'ring')
    with pytest.raises(ValueError):                              # a bare PlanarFrame of another size is not resized silently
        ctx.frame_upload(f)
    on_size = pitched(rng, w, h, '420', 0)
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
    good = pitched(rng, w, h, '420', 0)
    c = C.c_int

    def desc(**kw):
        d = type(good.describe()).from_buffer_copy(good.describe())
        for k, v in kw.items():
            setattr(d, k, v)
        return C.byref(d)

    calls = [lambda d: lib.fm_frame_upload_planar(ctx.handle, d),
             lambda d: lib.fm_frame_upload_ahead_planar(ctx.handle, c(1), d),
             lambda d: lib.fm_frame_ring_store_planar(ctx.handle, c(0), d)]
    bad = [dict(y=None), dict(u=None), dict(v=None), dict(chroma=4), dict(chroma=-1), dict(matrix=2), dict(matrix=-1),
           dict(pitch_y=w - 1), dict(pitch_y=0), dict(pitch_c=w // 2 - 1), dict(width=0), dict(height=0), dict(width=16385),
           dict(height=16385), dict(chroma=2, pitch_c=w - 1), dict(width=-4)]
    for call in calls:
        for kw in bad:
            assert call(desc(**kw)) == FM_ERR_ARG, kw
            assert b'bad argument' in lib.fm_last_error()
        assert call(None) == FM_ERR_ARG
    for k in (0, _lib.FM_MAX_DET_BATCH + 1):
        assert lib.fm_frame_upload_ahead_planar(ctx.handle, c(k), desc()) == FM_ERR_ARG
    for index in (-1, 1):
        assert lib.fm_frame_ring_store_planar(ctx.handle, c(index), desc()) == FM_ERR_ARG
    with pytest.raises(_lib.FastMOTHipError):                    # no frame in slot 1: none of the calls above put one there
        ctx.frame_promote_next()
    assert np.array_equal(ctx.frame_read(), before)              # nothing was copied or launched
    ctx.frame_ring_select(0)
    assert np.array_equal(ctx.frame_read(), before)
    # mono needs no chroma planes
    assert lib.fm_frame_upload_planar(ctx.handle, desc(chroma=3, u=None, v=None, pitch_c=0)) == 0
    assert np.array_equal(ctx.frame_read(), planar_to_bgr(good.y, None, None, 'mono'))


@pytest.mark.parametrize('size', SIZES, ids=ids)
def test_export_equals_bgr_to_planar420(ctx, size):
    w, h = size
    rng = np.random.default_rng(w * 139 + h)
    configure(ctx, w, h)
    for extremes in (False, True):
        frame = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if extremes:
            frame = rng.choice(np.array([0, 1, 127, 128, 254, 255], np.uint8), (h, w, 3))
        ctx.frame_upload(frame)
        got = ctx.frame_export_i420()
        assert got.dtype == np.uint8 and got.shape == (w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2),)
        assert np.array_equal(got, flat(bgr_to_planar420(ctx.frame_read())))
        assert np.array_equal(ctx.frame_read(), frame)
        # host pixels: contiguous, and rows with a padded pitch
        assert np.array_equal(ctx.i420_from_bgr(frame), flat(bgr_to_planar420(frame)))
        wide = rng.integers(0, 256, (h, w + 5, 3), dtype=np.uint8)
        assert np.array_equal(ctx.i420_from_bgr(wide[:, :w]), flat(bgr_to_planar420(wide[:, :w])))
    # a frame that was uploaded as planar 4:2:0 comes back through the same pair of kernels
    f = pitched(rng, w, h, '420', 0)
    ctx.frame_upload(f)
    assert np.array_equal(ctx.frame_export_i420(), flat(bgr_to_planar420(f.to_bgr())))


def c_int(v):
    return C.c_int(v)


def test_export_into_pinned_memory(ctx):
    w, h = 33, 31
    configure(ctx, w, h)
    frame = cases.noise(w, h, 5)
    ctx.frame_upload(frame)
    need = ctx.lib.fm_i420_bound(C.c_int(w), C.c_int(h))
    out = _lib.pinned_empty(ctx.lib, (need + 8,), np.uint8)
    out[...] = 0xA5
    n = C.c_size_t(0)
    assert ctx.lib.fm_frame_export_i420(ctx.handle, c_int(0), _lib._ptr(out), C.c_size_t(need), C.byref(n)) == 0
    assert n.value == need and np.array_equal(out[:need], flat(bgr_to_planar420(frame))) and (out[need:] == 0xA5).all()


@pytest.mark.parametrize('size', [(67, 35), (80, 48)], ids=ids)
def test_overlay_export(ctx, size):
    w, h = size
    ow, oh = (80, 48) if size != (80, 48) else (67, 35)          # a picture of another frame size is no picture of this one
    configure(ctx, ow, oh)
    ctx.frame_upload(cases.noise(ow, oh, 29))
    ctx.frame_render_overlay(*cases.scene_commands(ow, oh))
    configure(ctx, w, h)
    frame = cases.noise(w, h, 30)
    ctx.frame_upload(frame)
    with pytest.raises(_lib.FastMOTHipError):
        ctx.overlay_export_i420()
    ctx.frame_render_overlay(*cases.scene_commands(w, h))
    drawn = ctx.overlay_read()
    assert (drawn != frame).any()
    assert np.array_equal(ctx.overlay_export_i420(), flat(bgr_to_planar420(drawn)))
    assert np.array_equal(ctx.frame_export_i420(), flat(bgr_to_planar420(frame)))      # the bare frame is still the frame
    assert np.array_equal(ctx.frame_read(), frame)


def test_export_errors(ctx):
    lib = ctx.lib
    w, h = 17, 9
    configure(ctx, w, h)
    frame = cases.noise(w, h, 31)
    ctx.frame_upload(frame)
    need = lib.fm_i420_bound(c_int(w), c_int(h))
    assert need == 17 * 9 + 2 * 9 * 5
    assert lib.fm_i420_bound(c_int(0), c_int(4)) == 0 and lib.fm_i420_bound(c_int(4), c_int(16385)) == 0
    out = np.full(need + 16, 0xA5, np.uint8)
    n = C.c_size_t(0)
    host = np.ascontiguousarray(frame)
    calls = [lambda cap: lib.fm_frame_export_i420(ctx.handle, c_int(0), _lib._ptr(out), C.c_size_t(cap), C.byref(n)),
             lambda cap: lib.fm_i420_from_bgr(ctx.handle, _lib._ptr(host), c_int(w), c_int(h), C.c_size_t(3 * w), _lib._ptr(out),
                                              C.c_size_t(cap), C.byref(n))]
    for call in calls:
        n.value = 0
        assert call(need - 1) == FM_ERR_ARG                      # one byte short: the needed length, nothing written
        assert n.value == need and (out == 0xA5).all()
        assert call(need) == 0
        assert n.value == need and np.array_equal(out[:need], flat(bgr_to_planar420(frame))) and (out[need:] == 0xA5).all()
        out[...] = 0xA5
    assert lib.fm_frame_export_i420(ctx.handle, c_int(2), _lib._ptr(out), C.c_size_t(out.size), C.byref(n)) == FM_ERR_ARG
    assert lib.fm_frame_export_i420(ctx.handle, c_int(0), None, C.c_size_t(out.size), C.byref(n)) == FM_ERR_ARG
    assert lib.fm_frame_export_i420(ctx.handle, c_int(0), _lib._ptr(out), C.c_size_t(out.size), None) == FM_ERR_ARG
    assert lib.fm_i420_from_bgr(ctx.handle, _lib._ptr(host), c_int(w), c_int(h), C.c_size_t(3 * w - 1), _lib._ptr(out),
                                C.c_size_t(out.size), C.byref(n)) == FM_ERR_ARG
    assert lib.fm_i420_from_bgr(ctx.handle, None, c_int(w), c_int(h), C.c_size_t(3 * w), _lib._ptr(out), C.c_size_t(out.size),
                                C.byref(n)) == FM_ERR_ARG
    assert (out == 0xA5).all()
    with pytest.raises(ValueError):
        ctx.i420_from_bgr(frame[..., 0])
