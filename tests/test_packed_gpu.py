"""GPU: packed 4:2:2 / RGB ingest (fm_frame_upload_packed / fm_frame_upload_ahead_packed / fm_frame_ring_store_packed),
csrc/packed.hip.  The conversions are integer arithmetic, so every comparison is np.array_equal against
fastmot_amd.utils.packed (pinned by the planar reference and a float formula in test_packed_host.py).

Sizes: 1x1 and 2x2 (a single thread, half a macropixel), 3x5 (an odd width: a spare luma byte, ragged runs only), 34x18
(3 W = 102: rows that begin 8-byte aligned, 4-byte aligned and neither, so all three store paths, and all load paths of
the 3-byte layouts), 33x7 (odd, several threads per row), 130x6 (17 threads a row), 1920x2 (240 threads a row: a second
workgroup, which begins inside a row; everything aligned), 12x3 (a whole run beside a run of exactly four pixels)."""
import ctypes as C

import numpy as np
import pytest

from fastmot_amd import PackedFrame, SourceFrame, _lib
from fastmot_amd.utils.packed import MATRICES, packed_to_bgr, row_bytes
from fastmot_amd.videoio import resize_bgr

pytestmark = pytest.mark.gpu

FM_ERR_ARG = -2
SIZES = [(1, 1), (2, 2), (3, 5), (34, 18), (33, 7), (130, 6), (1920, 2), (12, 3)]
RGB_FORMATS = ['rgb', 'bgr', 'rgbx', 'bgrx', 'xrgb', 'xbgr']
YUV_FORMATS = ['yuy2', 'uyvy', 'yvyu']
ids = lambda s: f'{s[0]}x{s[1]}'


def configure(ctx, w, h, ring=0):
    ctx.frame_configure(w, h, ring)
    ctx.next_frame, ctx.ahead_frames, ctx.bound_frame = None, [], None


def combos():
    """Every (format, matrix) the library distinguishes: the matrix is not used by the RGB family."""
    return [(f, m) for f in YUV_FORMATS for m in MATRICES] + [(f, 'bt601') for f in RGB_FORMATS]


def make(ctx, rng, w, h, fmt, pad, matrix='bt601', pinned=False):
    """A frame of random bytes whose rows lie `pad` bytes further apart than their width (the padding random too), in
    fm_host_alloc memory when `pinned`; the first row all 0 and the last all 255 where there is more than one."""
    rb = row_bytes(w, fmt)
    buf = _lib.pinned_empty(ctx.lib, (h, rb + pad), np.uint8) if pinned else np.empty((h, rb + pad), np.uint8)
    buf[...] = rng.integers(0, 256, buf.shape, dtype=np.uint8)
    if h > 1:
        buf[0, :rb], buf[-1, :rb] = 0, 255
    return PackedFrame(buf[:, :rb], fmt, (w, h), matrix)


@pytest.mark.parametrize('size', SIZES, ids=ids)
def test_upload_equals_packed_to_bgr(ctx, size):
    w, h = size
    rng = np.random.default_rng(w * 131 + h)
    configure(ctx, w, h)
    for fmt, matrix in combos():
        for pad in (0, 5):
            for pinned in (False, True):
                f = make(ctx, rng, w, h, fmt, pad, matrix, pinned)
                assert f.pitch == (row_bytes(w, fmt) + pad if h > 1 else row_bytes(w, fmt))
                ctx.frame_upload(f)
                assert np.array_equal(ctx.frame_read(), f.to_bgr()), (fmt, matrix, pad, pinned)
    f = ctx.pinned_packed_frames(1, 'uyvy', 'bt709-full')[0]
    assert f.size == (w, h) and f.pitch == row_bytes(w, 'uyvy')
    f.rows[...] = rng.integers(0, 256, f.rows.shape, dtype=np.uint8)
    ctx.frame_upload(f)
    assert np.array_equal(ctx.frame_read(), packed_to_bgr(f.rows, size, 'uyvy', 'bt709-full'))


@pytest.mark.parametrize('size', SIZES, ids=ids)
def test_other_entry_points(ctx, size):
    w, h = size
    rng = np.random.default_rng(w * 137 + h)
    configure(ctx, w, h, 2)
    for i, (fmt, matrix) in enumerate(combos()):
        a, b, c = (make(ctx, rng, w, h, fmt, pad, matrix, pinned) for pad, pinned in ((0, bool(i & 1)), (3, False), (3, True)))
        ctx.frame_upload_ahead(1, a)
        ctx.frame_upload_ahead(2, b)
        for f in (a, b):
            ctx.frame_promote_next()
            assert np.array_equal(ctx.frame_read(), f.to_bgr()), (fmt, matrix, 'ahead')
        ctx.frame_upload_next(c)
        ctx.frame_promote_next()
        assert np.array_equal(ctx.frame_read(), c.to_bgr()), (fmt, matrix, 'next')
        ctx.frame_ring_store(1, b)
        ctx.frame_ring_store(0, a)
        for k, f in enumerate((a, b)):
            ctx.frame_ring_select(k)
            assert np.array_equal(ctx.frame_read(), f.to_bgr()), (fmt, matrix, 'ring', k)


@pytest.mark.parametrize('size', [(1, 1), (5, 1), (8, 1), (9, 3), (11, 2)], ids=ids)
def test_staged_rgb_at_every_ring_address(ctx, size):
    """One kernel converts staged RGB frames and device tensors, choosing loads and stores by address.  A ring of three
    frames of w * h * 3 bytes puts frames 1 and 2, and with widths of 5, 9 and 11 the rows inside them, at every residue
    mod 8; the 3-byte sources' rows lie at the same residues in their staging.  Each destination holds a sentinel first;
    the converter writes its frame, w * h * 3 bytes, and leaves the ring frames on either side of it as they were."""
    w, h = size
    rng = np.random.default_rng(w * 139 + h)
    ring = 3
    configure(ctx, w, h, ring)
    sentinel = np.full((h, w, 3), 0xA5, np.uint8)
    for fmt in ('rgb', 'bgr', 'rgbx', 'xbgr'):
        for index in range(ring):
            for i in range(ring):
                ctx.frame_ring_store(i, sentinel)
            f = make(ctx, rng, w, h, fmt, (0, 3)[index & 1], pinned=bool(index & 2))
            ctx.frame_ring_store(index, f)
            for i in range(ring):
                ctx.frame_ring_select(i)
                assert np.array_equal(ctx.frame_read(), f.to_bgr() if i == index else sentinel), (fmt, index, i)
        in_ring = f.to_bgr()
        a, b = make(ctx, rng, w, h, fmt, 0), make(ctx, rng, w, h, fmt, 5, pinned=True)
        ctx.frame_upload(sentinel)
        ctx.frame_upload(a)
        assert np.array_equal(ctx.frame_read(), a.to_bgr()), (fmt, 'upload')
        ctx.frame_upload_ahead(1, sentinel)
        ctx.frame_upload_ahead(1, b)
        ctx.frame_promote_next()
        assert np.array_equal(ctx.frame_read(), b.to_bgr()), (fmt, 'ahead')
        for i in range(ring):                                    # the uploads went to buffers of their own
            ctx.frame_ring_select(i)
            assert np.array_equal(ctx.frame_read(), in_ring if i == ring - 1 else sentinel), (fmt, i)


@pytest.mark.parametrize('src,dst', [((40, 24), (20, 12)), ((37, 21), (34, 18))], ids=['exact2x', 'linear'])
def test_source_frame_of_another_size(ctx, src, dst):
    rng = np.random.default_rng(src[0])
    configure(ctx, dst[0], dst[1], 1)
    for i, (fmt, matrix) in enumerate(combos()):
        for pad in (0, 3):
            f = make(ctx, rng, src[0], src[1], fmt, pad, matrix, pinned=bool(i & 1))
            want = resize_bgr(f.to_bgr(), dst)
            ctx.frame_upload(SourceFrame(f))
            assert np.array_equal(ctx.frame_read(), want), (fmt, matrix, pad, 'upload')
            for k in (1, 2):
                ctx.frame_upload_ahead(k, SourceFrame(f))
            for k in (1, 2):
                ctx.frame_promote_next()
                assert np.array_equal(ctx.frame_read(), want), (fmt, matrix, pad, 'ahead', k)
            ctx.frame_ring_store(0, SourceFrame(f))
            ctx.frame_ring_select(0)
            assert np.array_equal(ctx.frame_read(), want), (fmt, matrix, pad, 'ring')
    with pytest.raises(ValueError):                              # a bare PackedFrame of another size is not resized silently
        ctx.frame_upload(f)
    on_size = make(ctx, rng, dst[0], dst[1], 'bgrx', 0)
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
    good = make(ctx, rng, w, h, 'yuy2', 0)
    rgbx = make(ctx, rng, w, h, 'rgbx', 0)
    c = C.c_int

    def desc(of=good, **kw):
        d = type(of.describe()).from_buffer_copy(of.describe())
        for k, v in kw.items():
            setattr(d, k, v)
        return C.byref(d)

    calls = [lambda d: lib.fm_frame_upload_packed(ctx.handle, d),
             lambda d: lib.fm_frame_upload_ahead_packed(ctx.handle, c(1), d),
             lambda d: lib.fm_frame_ring_store_packed(ctx.handle, c(0), d)]
    bad = [dict(data=None), dict(format=-1), dict(format=9), dict(matrix=2), dict(matrix=15), dict(matrix=18), dict(matrix=-1),
           dict(pitch=2 * w - 1), dict(pitch=0), dict(pitch=-2 * w), dict(width=0), dict(height=0), dict(width=16385),
           dict(height=16385), dict(width=-4), dict(of=rgbx, pitch=4 * w - 1), dict(of=rgbx, matrix=2), dict(format=3)]
    for call in calls:
        for kw in bad:
            assert call(desc(**kw)) == FM_ERR_ARG, kw
            assert b'bad argument' in lib.fm_last_error()
        assert call(None) == FM_ERR_ARG
    for k in (0, _lib.FM_MAX_DET_BATCH + 1):
        assert lib.fm_frame_upload_ahead_packed(ctx.handle, c(k), desc()) == FM_ERR_ARG
    for index in (-1, 1):
        assert lib.fm_frame_ring_store_packed(ctx.handle, c(index), desc()) == FM_ERR_ARG
    with pytest.raises(_lib.FastMOTHipError):                    # no frame in slot 1: none of the calls above put one there
        ctx.frame_promote_next()
    assert np.array_equal(ctx.frame_read(), before)              # nothing was copied or launched
    ctx.frame_ring_select(0)
    assert np.array_equal(ctx.frame_read(), before)
    # the same descriptions, unmodified, are accepted
    assert lib.fm_frame_upload_packed(ctx.handle, desc()) == 0
    assert np.array_equal(ctx.frame_read(), good.to_bgr())
    assert lib.fm_frame_upload_packed(ctx.handle, desc(of=rgbx, matrix=17)) == 0
    assert np.array_equal(ctx.frame_read(), rgbx.to_bgr())


# ---- MOT.step
SIZE = (960, 540)          # the smallest size the MOT tests run the tracker at


def to_yuy2(frame):
    """A BGR frame as YUY2 bytes (H, 2 W): bgr_to_planar420's luma, its chroma rows used for both rows of a pair."""
    from fastmot_amd.utils.yuv import bgr_to_planar420
    y, u, v = bgr_to_planar420(frame)
    h, w = y.shape
    out = np.empty((h, w // 2, 4), np.uint8)
    out[..., 0], out[..., 2] = y[:, 0::2], y[:, 1::2]
    out[..., 1], out[..., 3] = np.repeat(u, 2, axis=0), np.repeat(v, 2, axis=0)
    return out.reshape(h, 2 * w)


def run_mot(video, frames):
    from fastmot_amd import Track
    from test_mot_gpu import build_mot
    mot = build_mot(SIZE, video, 1)
    Track._count = 0
    mot.reset(1 / 30.)
    rows = []
    try:
        for i, frame in enumerate(frames):
            mot.detector._frame_idx = i
            mot.step(frame, next_frame=frames[i + 1] if i + 1 < len(frames) else None)
            rows.append([(t.trk_id, tuple(t.tlbr), t.confirmed, t.active, t.age, t.hits) for t in mot.tracker.tracks.values()])
    finally:
        mot.tracker._clear_tracks()
    return rows


def test_tracks_on_packed_frames_equal_bgr_frames(ctx):
    from synthetic import SyntheticVideo
    video = SyntheticVideo(SIZE, n_ids=8, n_frames=8, seed=4)
    rng = np.random.default_rng(5)
    bgr = [np.ascontiguousarray(f) for f in video.frames]
    rgbx = [PackedFrame(np.concatenate([f[..., ::-1], rng.integers(0, 256, f.shape[:2] + (1,), dtype=np.uint8)], axis=-1), 'rgbx')
            for f in bgr]
    assert np.array_equal(rgbx[0].to_bgr(), bgr[0])
    want = run_mot(video, bgr)
    assert len(want[-1]) >= 6
    assert run_mot(video, rgbx) == want
    yuy2 = [PackedFrame(to_yuy2(f), 'yuy2', SIZE) for f in bgr]
    assert run_mot(video, yuy2) == run_mot(video, [f.to_bgr() for f in yuy2])


def test_draw_refuses_packed_frames(ctx):
    from synthetic import SyntheticVideo
    from test_mot_gpu import build_mot
    video = SyntheticVideo(SIZE, n_ids=2, n_frames=1, seed=4)
    mot = build_mot(SIZE, video, 1)
    mot.draw = True
    mot.reset(1 / 30.)
    try:
        with pytest.raises(TypeError):
            mot.step(PackedFrame(np.ascontiguousarray(video.frames[0][..., ::-1]), 'rgb'))
    finally:
        mot.tracker._clear_tracks()
