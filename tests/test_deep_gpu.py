"""GPU: 9- to 16-bit YCbCr ingest (fm_frame_upload_deep / fm_frame_upload_ahead_deep / fm_frame_ring_store_deep),
csrc/deep.hip.  The conversion is integer arithmetic, so every comparison is np.array_equal against DeepFrame.to_bgr()
(fastmot_amd/utils/deep.py, pinned by NV12's function, a derived bound and by hand in test_deep_host.py).

Sizes: test_yuv_gpu.py's, for its reasons -- 1 and 2 (a single thread, no row pair), 3x5 / 7x3 / 9x2 (odd chroma width,
a last row without a partner, a second thread of one pixel), 8x8 (the aligned vector path alone), 17x9 and 33x31 (whole
runs beside ragged ones, rows that start at every alignment), 64x36 (everything aligned), 130x70 (more than one workgroup).
Semi-planar frames have even sizes: the even ones of those, and 18x10 (a ragged second thread with whole U, V pairs)."""
import ctypes as C

import numpy as np
import pytest

import lens_cases as lc
from fastmot_amd import DeepFrame, LensMap, SourceFrame, VideoIO, _lib
from fastmot_amd.utils.lens import remap_bgr
from fastmot_amd.utils.yuv import bgr_to_planar420, chroma_shape
from fastmot_amd.videoio import resize_bgr

pytestmark = pytest.mark.gpu

FM_ERR_ARG = -2
SIZES = [(1, 1), (2, 2), (3, 5), (7, 3), (8, 8), (9, 2), (17, 9), (33, 31), (64, 36), (130, 70)]
SEMI_SIZES = [(2, 2), (8, 8), (18, 10), (64, 36), (130, 70)]
CHROMAS = ['420', '422', '444', 'mono']
KINDS = [('planar', c) for c in CHROMAS] + [('semiplanar', '420')]
DEPTHS = [10, 12, 16]
MATRICES = ['bt601', 'bt709', 'bt2020']
ids = lambda s: f'{s[0]}x{s[1]}'


def configure(ctx, w, h, ring=0):
    ctx.frame_configure(w, h, ring)
    ctx.next_frame, ctx.ahead_frames, ctx.bound_frame = None, [], None


@pytest.fixture(autouse=True)
def no_lens_left_behind(ctx):
    yield
    ctx.frame_set_lens(None)


def pitched(rng, w, h, kind, depth, pad=0, matrix='bt709', extremes=False, stray=False):
    """A frame of random samples whose rows lie `pad` bytes (even) further apart than their width (the padding random
    too).  extremes: Y in {0, (16 << s) - 1, 16 << s, 235 << s, max} x U, V in {0, 128 << s, max} instead.  stray: random
    bits where the layout has none -- above the sample for planar, below it for semi-planar."""
    layout, chroma = kind
    s, top = depth - 8, (1 << depth) - 1
    semi = layout == 'semiplanar'

    def plane(rows, cols, values):
        buf = rng.integers(0, 1 << 16, (rows, cols + pad // 2), dtype=np.uint16)
        view = buf[:, :cols]
        if values is None:
            v = rng.integers(0, top + 1, (rows, cols), dtype=np.uint16)
        else:
            v = rng.choice(np.array(values, np.uint16), (rows, cols))
        junk = rng.integers(0, 1 << (16 - depth), (rows, cols), dtype=np.uint16) if stray else np.zeros((rows, cols), np.uint16)
        view[...] = (v << (16 - depth)) | junk if semi else v | (junk << depth if depth < 16 else 0)
        return view

    yv = (0, (16 << s) - 1, 16 << s, 235 << s, top) if extremes else None
    cv = (0, 128 << s, top) if extremes else None
    y = plane(h, w, yv)
    if semi:
        return DeepFrame.semiplanar(y, plane(h // 2, w, cv), depth, matrix)
    cs = chroma_shape((w, h), chroma)
    if cs is None:
        return DeepFrame(y, chroma=chroma, depth=depth, matrix=matrix)
    return DeepFrame(y, plane(cs[0], cs[1], cv), plane(cs[0], cs[1], cv), chroma, depth, matrix)


def kinds_for(size):
    return [k for k in KINDS if k[0] == 'planar' or size in SEMI_SIZES]


@pytest.mark.parametrize('size', SIZES + [(18, 10)], ids=ids)
def test_upload_equals_to_bgr(ctx, size):
    w, h = size
    rng = np.random.default_rng(w * 131 + h)
    configure(ctx, w, h, 1)
    n = 0
    for kind in kinds_for(size):
        for depth in DEPTHS:
            for matrix in MATRICES:
                for pad in (0, 6):
                    for extremes in (False, True):
                        n += 1
                        f = pitched(rng, w, h, kind, depth, pad, matrix, extremes, stray=bool(n & 1) ^ bool(n & 4))
                        assert f.pitch == (2 * w + pad if h > 1 else 2 * w)
                        ctx.frame_upload(f)
                        assert np.array_equal(ctx.frame_read(), f.to_bgr()), (kind, depth, matrix, pad, extremes)


@pytest.mark.parametrize('size', SIZES + [(18, 10)], ids=ids)
def test_other_entry_points(ctx, size):
    w, h = size
    rng = np.random.default_rng(w * 137 + h)
    configure(ctx, w, h, 2)
    for i, kind in enumerate(kinds_for(size)):
        layout, chroma = kind
        matrix, depth = MATRICES[i % 3], DEPTHS[i % 3]
        a, b, c = (pitched(rng, w, h, kind, depth, pad, matrix, stray=True) for pad in (0, 6, 6))
        ctx.frame_upload_ahead(1, a)
        ctx.frame_upload_ahead(2, b)
        for f in (a, b):
            ctx.frame_promote_next()
            assert np.array_equal(ctx.frame_read(), f.to_bgr()), (kind, 'ahead')
        ctx.frame_upload_next(c)
        ctx.frame_promote_next()
        assert np.array_equal(ctx.frame_read(), c.to_bgr()), (kind, 'next')
        ctx.frame_ring_store(1, b)
        ctx.frame_ring_store(0, a)
        for k, f in enumerate((a, b)):
            ctx.frame_ring_select(k)
            assert np.array_equal(ctx.frame_read(), f.to_bgr()), (kind, 'ring', k)
        semi = layout == 'semiplanar'
        pinned = ctx.pinned_deep_frames(2, chroma, depth, matrix, semiplanar=semi)
        for p in pinned:
            assert p.size == (w, h) and p.pitch == 2 * w and p.chroma == chroma and p.matrix == matrix and p.depth == depth
            assert p.layout == layout
            for plane in (p.y, p.u, p.v, p.uv):
                if plane is not None:
                    plane[...] = rng.integers(0, 1 << 16, plane.shape, dtype=np.uint16)
        ctx.frame_upload(pinned[0])
        assert np.array_equal(ctx.frame_read(), pinned[0].to_bgr()), (kind, 'pinned upload')
        ctx.frame_upload_ahead(1, pinned[1])
        ctx.frame_promote_next()
        assert np.array_equal(ctx.frame_read(), pinned[1].to_bgr()), (kind, 'pinned ahead')
    with pytest.raises(ValueError):
        ctx.pinned_deep_frames(1, '444', semiplanar=True)


def test_444_depth_16_in_lookahead_slot_2(ctx):
    """Six bytes per pixel through a look-ahead slot whose own page-locked and device buffers hold three: the staging is
    the family's own and grows -- first for a small layout, then for the largest."""
    w, h = 130, 70
    rng = np.random.default_rng(7)
    configure(ctx, w, h)
    small = pitched(rng, w, h, ('planar', 'mono'), 10, 6)
    big = pitched(rng, w, h, ('planar', '444'), 16, 6, 'bt2020')
    other = pitched(rng, w, h, ('planar', '444'), 16, 0, 'bt601')
    ctx.frame_upload_ahead(1, small)
    ctx.frame_upload_ahead(2, small)
    ctx.frame_upload_ahead(2, big)                                 # regrown while the first copy may be in flight
    ctx.frame_upload_ahead(3, other)
    for f in (small, big, other):
        ctx.frame_promote_next()
        assert np.array_equal(ctx.frame_read(), f.to_bgr())
    ctx.frame_upload(big)
    assert np.array_equal(ctx.frame_read(), big.to_bgr())


@pytest.mark.parametrize('src', [(66, 38), (128, 72)], ids=ids)
def test_source_frame_of_another_size(ctx, src):
    w, h = 64, 36
    rng = np.random.default_rng(src[0])
    configure(ctx, w, h, 1)
    for i, kind in enumerate(KINDS):
        for pad in (0, 6):
            f = pitched(rng, src[0], src[1], kind, DEPTHS[i % 3], pad, MATRICES[i % 3], stray=True)
            want = resize_bgr(f.to_bgr(), (w, h))
            ctx.frame_upload(SourceFrame(f))
            assert np.array_equal(ctx.frame_read(), want), (kind, pad, 'upload')
            ctx.frame_upload_ahead(1, SourceFrame(f))
            ctx.frame_promote_next()
            assert np.array_equal(ctx.frame_read(), want), (kind, pad, 'ahead')
            ctx.frame_ring_store(0, SourceFrame(f))
            ctx.frame_ring_select(0)
            assert np.array_equal(ctx.frame_read(), want), (kind, pad, 'ring')
    with pytest.raises(ValueError):                              # a bare DeepFrame of another size is not resized silently
        ctx.frame_upload(f)
    with pytest.raises(ValueError):
        ctx.frame_upload_ahead(1, f)
    with pytest.raises(ValueError):
        ctx.frame_ring_store(0, f)
    with pytest.raises(TypeError):
        SourceFrame(f).describe()
    on_size = pitched(rng, w, h, ('semiplanar', '420'), 10)
    ctx.frame_upload(SourceFrame(on_size))                       # a SourceFrame of the configured size is the plain upload
    assert np.array_equal(ctx.frame_read(), on_size.to_bgr())


@pytest.mark.parametrize('dst', [(26, 14), (38, 30)], ids=['off-size', 'on-size'])
def test_source_frame_with_a_lens(ctx, dst):
    src = (38, 30)
    rng = np.random.default_rng(dst[0])
    configure(ctx, dst[0], dst[1], 1)
    # a small barrel lens: the test models' coefficients around the centre of a 38 x 30 source, zoomed out so that the
    # border shows
    lens = LensMap.pinhole((25., 24.5, 18.5, 14.25), lc.D_BARREL, src, dst, zoom=0.6, border=lc.BORDER)
    outside = (lens.xy < 0).any(-1) | (lens.xy[..., 0] > 32 * (src[0] - 1)) | (lens.xy[..., 1] > 32 * (src[1] - 1))
    assert 0.02 < outside.mean() < 0.7
    for i, kind in enumerate(KINDS):
        f = pitched(rng, src[0], src[1], kind, DEPTHS[i % 3], 6, MATRICES[i % 3])
        want = remap_bgr(f.to_bgr(), lens)
        wrapped = SourceFrame(f, lens=lens)
        ctx.frame_upload(wrapped)
        assert np.array_equal(ctx.frame_read(), want), (kind, 'upload')
        ctx.frame_upload_ahead(1, wrapped)
        ctx.frame_upload_ahead(2, wrapped)
        for k in (1, 2):
            ctx.frame_promote_next()
            assert np.array_equal(ctx.frame_read(), want), (kind, 'ahead', k)
        ctx.frame_ring_store(0, wrapped)
        ctx.frame_ring_select(0)
        assert np.array_equal(ctx.frame_read(), want), (kind, 'ring')
    # while the map is set a deep frame of another size than the map's is refused by the raw call
    other = pitched(rng, 16, 6, ('planar', '420'), 10)
    assert ctx.lib.fm_frame_upload_deep(ctx.handle, C.byref(other.describe())) == FM_ERR_ARG


def test_bad_arguments(ctx):
    lib = ctx.lib
    w, h = 16, 6
    configure(ctx, w, h, 1)
    rng = np.random.default_rng(3)
    before = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    ctx.frame_upload(before)
    ctx.frame_ring_store(0, before)
    good = pitched(rng, w, h, ('planar', '420'), 10)
    semi = pitched(rng, w, h, ('semiplanar', '420'), 10)
    c = C.c_int

    def desc(frame=good, **kw):
        d = type(frame.describe()).from_buffer_copy(frame.describe())
        for k, v in kw.items():
            setattr(d, k, v)
        return C.byref(d)

    calls = [lambda d: lib.fm_frame_upload_deep(ctx.handle, d),
             lambda d: lib.fm_frame_upload_ahead_deep(ctx.handle, c(1), d),
             lambda d: lib.fm_frame_ring_store_deep(ctx.handle, c(0), d)]
    bad = [dict(depth=8), dict(depth=17), dict(depth=0), dict(layout=2), dict(layout=-1), dict(chroma=4), dict(chroma=-1),
           dict(matrix=3), dict(matrix=-1), dict(matrix=16), dict(pitch_y=2 * w + 1), dict(pitch_y=2 * w - 2), dict(pitch_y=0),
           dict(pitch_c=w + 1), dict(pitch_c=w - 2), dict(chroma=2, pitch_c=2 * w - 2), dict(y=None), dict(u=None), dict(v=None),
           dict(width=0), dict(height=0), dict(width=16385), dict(height=16385), dict(width=-4)]
    bad_semi = [dict(width=w - 1), dict(height=h - 1), dict(chroma=1), dict(chroma=3), dict(u=None), dict(y=None),
                dict(pitch_c=2 * w - 2), dict(pitch_c=2 * w + 1), dict(depth=8), dict(depth=17)]
    for call in calls:
        for kw in bad:
            assert call(desc(**kw)) == FM_ERR_ARG, kw
            assert b'bad argument' in lib.fm_last_error()
        for kw in bad_semi:
            assert call(desc(semi, **kw)) == FM_ERR_ARG, ('semiplanar', kw)
        assert call(None) == FM_ERR_ARG
    for k in (0, _lib.FM_MAX_DET_BATCH + 1):
        assert lib.fm_frame_upload_ahead_deep(ctx.handle, c(k), desc()) == FM_ERR_ARG
    for index in (-1, 1):
        assert lib.fm_frame_ring_store_deep(ctx.handle, c(index), desc()) == FM_ERR_ARG
    with pytest.raises(_lib.FastMOTHipError):                    # no frame in slot 1: none of the calls above put one there
        ctx.frame_promote_next()
    assert np.array_equal(ctx.frame_read(), before)              # nothing was copied or launched
    ctx.frame_ring_select(0)
    assert np.array_equal(ctx.frame_read(), before)
    # mono needs no chroma planes; a semi-planar frame no v
    assert lib.fm_frame_upload_deep(ctx.handle, desc(chroma=3, u=None, v=None, pitch_c=0)) == 0
    assert np.array_equal(ctx.frame_read(), DeepFrame(good.y, chroma='mono').to_bgr())
    assert lib.fm_frame_upload_deep(ctx.handle, desc(semi)) == 0
    assert np.array_equal(ctx.frame_read(), semi.to_bgr())


def test_videoio_gpu_decode_uploads_the_host_paths_pixels(ctx, tmp_path):
    from test_deep_host import CLIPS, read_all, write_clip
    for size, token, chroma, depth in CLIPS:
        path = tmp_path / f'{token}.y4m'
        write_clip(path, size, token, chroma, depth)
        host = read_all(VideoIO(size, str(path), deep_color=True, yuv_matrix='bt2020'))
        gpu = read_all(VideoIO(size, str(path), deep_color=True, gpu_decode=True, yuv_matrix='bt2020'))
        assert len(host) == len(gpu) == 3
        configure(ctx, *size)
        for a, b in zip(host, gpu):
            assert isinstance(a, np.ndarray) and isinstance(b, DeepFrame)
            ctx.frame_upload(b)
            assert np.array_equal(ctx.frame_read(), a), token
        small = (max(size[0] // 2, 1), max(size[1] // 2, 1))
        host = read_all(VideoIO(small, str(path), deep_color=True))
        gpu = read_all(VideoIO(small, str(path), deep_color=True, gpu_decode=True, gpu_resize=True))
        configure(ctx, *small)
        for a, b in zip(host, gpu):
            assert isinstance(b, SourceFrame)
            ctx.frame_upload(b)
            assert np.array_equal(ctx.frame_read(), a), (token, 'resized')


def test_tracks_on_deep_frames_equal_bgr_frames(ctx):
    """MOT.step on 420p10 and P010 frames, each with next_frame prefetch: the tracks, ids and boxes of the run on the
    to_bgr() arrays."""
    from synthetic import SyntheticVideo
    from test_packed_gpu import SIZE, run_mot
    video = SyntheticVideo(SIZE, n_ids=8, n_frames=8, seed=4)
    rng = np.random.default_rng(6)
    planar, semi = [], []
    for f in video.frames:
        # the clip at 10 bits: its 8-bit planes with two random bits below them
        y, u, v = ((p.astype(np.uint16) << 2) | rng.integers(0, 4, p.shape, dtype=np.uint16) for p in bgr_to_planar420(f))
        planar.append(DeepFrame(y, u, v, '420', 10, 'bt601'))
        uv = np.empty((SIZE[1] // 2, SIZE[0]), np.uint16)
        uv[:, 0::2], uv[:, 1::2] = u << 6, v << 6
        semi.append(DeepFrame.semiplanar(y << 6, uv, 10, 'bt601'))
    bgr = [f.to_bgr() for f in planar]
    assert np.array_equal(semi[0].to_bgr(), bgr[0])
    want = run_mot(video, bgr)
    assert len(want[-1]) >= 6
    assert run_mot(video, planar) == want
    assert run_mot(video, semi) == want
