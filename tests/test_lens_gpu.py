"""GPU: the correction map behind the described-source calls (fm_frame_remap_set, csrc/remap.hip).  The arithmetic is
integer, so every comparison is np.array_equal against fastmot_amd.utils.lens.remap_bgr (pinned by a float64 statement
and by the compiled host twin in test_lens_host.py).

A thread owns 8 output pixels of a row and takes the vector path when the destination's width is a multiple of 8.
Shapes (lens_cases.SHAPES): 1x1 -> 1x1; 2x2 -> 8x1 (one vector thread); 3x3 -> 14x14 (the boundary table: X and Y over
every value at which a tap enters or leaves the source); 37x29 -> 13x7 (byte path, odd everything); 37x29 -> 64x48
(magnification, vector path); 640x360 -> 426x240 (the lens models; byte path, 426 % 8 = 2, several blocks);
640x360 -> 640x360 (an on-size source with a map that is not the identity); 16384x2 -> 24x3 (the largest offsets).
Random maps are drawn over [-2, sw + 1] x [-2, sh + 1], so all four sides and corners fall outside; the border is
(7, 130, 255)."""
import ctypes as C

import numpy as np
import pytest

import jpeg_cases as jc
import lens_cases as lc
from fastmot_amd import BayerFrame, JPEGFrame, LensMap, NV12Frame, PackedFrame, PlanarFrame, SourceFrame, _lib
from fastmot_amd.utils.lens import remap_bgr
from fastmot_amd.utils.nv12 import nv12_to_bgr
from fastmot_amd.utils.yuv import frame_bytes
from fastmot_amd.videoio import resize_bgr

pytestmark = pytest.mark.gpu

FM_ERR_ARG = -2


def configure(ctx, w, h, ring=0):
    ctx.frame_configure(w, h, ring)
    ctx.next_frame, ctx.ahead_frames, ctx.bound_frame = None, [], None


@pytest.fixture(autouse=True)
def no_lens_left_behind(ctx):
    yield
    ctx.frame_set_lens(None)


def source_frames(ctx, rng, src, n, pinned):
    """n random frames of the source size -- for the boundary table's 3 x 3 source values in {0, 255}."""
    sw, sh = src
    buf = ctx.pinned_source_frames(n, src) if pinned else np.empty((n, sh, sw, 3), np.uint8)
    buf[...] = rng.integers(0, 256, buf.shape, dtype=np.uint8)
    if src == (3, 3):
        for i, f in enumerate(lc.boundary_frames()[:n]):
            buf[i] = f
    return [buf[i] for i in range(n)]


@pytest.mark.parametrize('shape', lc.SHAPES, ids=lc.shape_id)
def test_every_entry_point(ctx, shape):
    src, dst = shape
    rng = np.random.default_rng(src[0] * 31 + dst[0])
    configure(ctx, dst[0], dst[1], 2)
    lens = lc.lens_for(rng, src, dst)
    for pinned in (True, False):
        frames = source_frames(ctx, rng, src, 5, pinned)
        want = [remap_bgr(f, lens) for f in frames]
        wrapped = [SourceFrame(f, lens=lens) for f in frames]
        ctx.frame_upload(wrapped[0])
        assert np.array_equal(ctx.frame_read(), want[0]), (pinned, 'upload')
        ctx.frame_upload_next(wrapped[1])
        ctx.frame_promote_next()
        assert np.array_equal(ctx.frame_read(), want[1]), (pinned, 'next')
        ctx.frame_upload_ahead(1, wrapped[2])
        ctx.frame_upload_ahead(2, wrapped[3])
        for i in (2, 3):
            ctx.frame_promote_next()
            assert np.array_equal(ctx.frame_read(), want[i]), (pinned, 'ahead', i)
        ctx.frame_ring_store(1, wrapped[4])
        ctx.frame_ring_store(0, wrapped[0])
        for k, i in ((0, 0), (1, 4)):
            ctx.frame_ring_select(k)
            assert np.array_equal(ctx.frame_read(), want[i]), (pinned, 'ring', k)
    if src == (3, 3):                                    # the rest of the boundary table's sources
        for f in lc.boundary_frames():
            ctx.frame_upload(SourceFrame(f, lens=lens))
            assert np.array_equal(ctx.frame_read(), remap_bgr(f, lens))


@pytest.mark.parametrize('model', ['barrel', 'pincushion', 'fisheye', 'fisheye-zoom0.6'])
def test_models(ctx, model):
    rng = np.random.default_rng(len(model))
    configure(ctx, lc.DST[0], lc.DST[1], 1)
    lens = lc.models()[model]
    a, b = source_frames(ctx, rng, lc.SRC, 2, pinned=True)
    ctx.frame_upload(SourceFrame(a, lens=lens))
    assert np.array_equal(ctx.frame_read(), remap_bgr(a, lens))
    ctx.frame_upload_next(SourceFrame(b, lens=lens))
    ctx.frame_ring_store(0, SourceFrame(a, lens=lens))
    ctx.frame_promote_next()
    assert np.array_equal(ctx.frame_read(), remap_bgr(b, lens))
    ctx.frame_ring_select(0)
    assert np.array_equal(ctx.frame_read(), remap_bgr(a, lens))


def to_yuy2(rng, w, h):
    return rng.integers(0, 256, (h, 4 * ((w + 1) // 2)), dtype=np.uint8)


def frame_kinds(rng, size):
    """(label, frame, the BGR pixels it converts to) for every frame kind a SourceFrame takes, at `size` (odd) -- NV12 and
    Bayer, which need even / >= 2 sizes, one pixel larger."""
    w, h = size
    even = (w + 1, h + 1)
    out = []
    surface = rng.integers(0, 256, (even[1] + even[1] // 2, even[0] + 6), dtype=np.uint8)
    y, uv = surface[:even[1], :even[0]], surface[even[1]:, :even[0]]
    out.append(('nv12', NV12Frame(y, uv), nv12_to_bgr(y, uv)))
    data = jc.encode(jc.content('noise', w, h, seed=3), '420', 90)
    jpeg = JPEGFrame(data)
    out.append(('jpeg', jpeg, jpeg.to_bgr()))
    planar = PlanarFrame.from_buffer(rng.integers(0, 256, frame_bytes(size, '420'), dtype=np.uint8), size, '420', 'bt709')
    out.append(('planar420', planar, planar.to_bgr()))
    yuy2 = PackedFrame(to_yuy2(rng, w, h), 'yuy2', size)
    out.append(('yuy2', yuy2, yuy2.to_bgr()))
    bgrx = PackedFrame(rng.integers(0, 256, (h, w, 4), dtype=np.uint8), 'bgrx')
    out.append(('bgrx', bgrx, bgrx.to_bgr()))
    bayer = BayerFrame(rng.integers(0, 4096, (even[1], even[0])).astype(np.uint16), 'rggb', depth=12)
    out.append(('rggb12', bayer, bayer.to_bgr()))
    return out


@pytest.mark.parametrize('dst', [(26, 14), (37, 29)], ids=['off-size', 'on-size'])
def test_every_frame_kind(ctx, dst):
    """NV12, JPEG, planar 4:2:0 of odd size, yuy2, bgrx and Bayer rggb12 inside SourceFrame(f, lens=...): each equals
    remap_bgr of the BGR frame it converts to.  On size: a source of the configured size is staged and remapped too."""
    rng = np.random.default_rng(dst[0])
    src = (37, 29)
    configure(ctx, dst[0], dst[1], 1)
    lenses = {}
    for label, frame, bgr in frame_kinds(rng, src):
        size = frame.size
        lens = lenses.setdefault(size, lc.random_lens(rng, size, dst))      # (two source sizes: two maps, one switch)
        want = remap_bgr(bgr, lens)
        wrapped = SourceFrame(frame, lens=lens)
        ctx.frame_upload(wrapped)
        assert np.array_equal(ctx.frame_read(), want), (label, 'upload')
        ctx.frame_upload_ahead(1, wrapped)
        ctx.frame_upload_ahead(2, wrapped)
        for k in (1, 2):
            ctx.frame_promote_next()
            assert np.array_equal(ctx.frame_read(), want), (label, 'ahead', k)
        ctx.frame_upload(SourceFrame(np.zeros(bgr.shape, np.uint8), lens=lens))
        ctx.frame_ring_store(0, wrapped)
        ctx.frame_ring_select(0)
        assert np.array_equal(ctx.frame_read(), want), (label, 'ring')


def test_switching(ctx):
    """Lens A, lens B, no lens, A again, an ahead slot filled before each switch: every frame equals its own expectation."""
    rng = np.random.default_rng(8)
    src, dst = (37, 29), (24, 16)
    configure(ctx, dst[0], dst[1], 1)
    a, b = lc.random_lens(rng, src, dst), lc.random_lens(rng, src, dst, border=(0, 0, 0))
    f = source_frames(ctx, rng, src, 8, pinned=True)
    want = lambda frame, lens: resize_bgr(frame, dst) if lens is None else remap_bgr(frame, lens)
    i = 0
    previous = None
    for lens in (a, b, None, a):
        ctx.frame_upload(SourceFrame(f[i], lens=lens))   # (switches)
        assert np.array_equal(ctx.frame_read(), want(f[i], lens)), i
        if previous is not None:
            ctx.frame_promote_next()                     # the slot filled under the previous setting, before the switch
            assert np.array_equal(ctx.frame_read(), want(*previous)), i
        ctx.frame_upload_next(SourceFrame(f[i + 1], lens=lens))
        previous = (f[i + 1], lens)
        i += 2
    ctx.frame_promote_next()
    assert np.array_equal(ctx.frame_read(), want(*previous))
    # an identity map at equal size returns the frame itself; without a lens such a frame is the plain upload
    configure(ctx, src[0], src[1])
    y, x = np.meshgrid(np.arange(src[1], dtype=np.float64), np.arange(src[0], dtype=np.float64), indexing='ij')
    identity = LensMap.from_arrays(x, y, src, lc.BORDER)
    ctx.frame_upload(SourceFrame(f[0], lens=identity))
    assert np.array_equal(ctx.frame_read(), f[0])
    mirror = LensMap.from_arrays(src[0] - 1 - x, y, src)
    ctx.frame_upload(SourceFrame(f[1], lens=mirror))
    assert np.array_equal(ctx.frame_read(), f[1][:, ::-1])
    ctx.frame_upload(SourceFrame(f[2]))
    assert np.array_equal(ctx.frame_read(), f[2])
    with pytest.raises(ValueError):                      # a map that gives frames of another size than the context's
        ctx.frame_set_lens(a)
    with pytest.raises(ValueError):
        ctx.frame_upload(SourceFrame(f[3], lens=a))
    assert np.array_equal(ctx.frame_read(), f[2])


def test_bad_arguments(ctx):
    lib = ctx.lib
    src, dst, other = (20, 12), (16, 6), (22, 12)
    configure(ctx, dst[0], dst[1], 1)
    rng = np.random.default_rng(3)
    lens = lc.random_lens(rng, src, dst)
    before = rng.integers(0, 256, (dst[1], dst[0], 3), dtype=np.uint8)
    ctx.frame_upload(before)
    ctx.frame_ring_store(0, before)
    c = C.c_int
    p = lambda a: C.c_void_p(a.__array_interface__['data'][0])
    border = (C.c_uint8 * 3)(*lens.border)
    good_xy = lens.xy

    def remap_set(sw=src[0], sh=src[1], xy=good_xy, border=border):
        return lib.fm_frame_remap_set(ctx.handle, c(sw), c(sh), None if xy is None else p(xy), border)

    def entry(comp, value):
        xy = np.array(good_xy)
        xy[dst[1] - 1, dst[0] - 1, comp] = value
        return xy

    bgr = rng.integers(0, 256, (src[1], src[0], 3), dtype=np.uint8)
    probe = SourceFrame(bgr, lens=lens)

    def check_map_is(want_lens):
        """By a direct call, so that the Python side sets nothing."""
        assert lib.fm_frame_upload_src(ctx.handle, C.byref(probe.describe())) == 0
        assert np.array_equal(ctx.frame_read(), remap_bgr(bgr, want_lens) if want_lens is not None else resize_bgr(bgr, dst))
        ctx.frame_upload(before)

    bad_sets = [dict(xy=None), dict(border=None), dict(xy=entry(0, -65)), dict(xy=entry(0, 32 * (src[0] + 1) + 1)), dict(xy=entry(1, -65)),
                dict(xy=entry(1, 32 * (src[1] + 1) + 1)), dict(sw=0), dict(sh=0), dict(sw=-1), dict(sh=-1), dict(sw=16385), dict(sh=16385)]
    for state in (None, lens):                           # with no map set, and with one: a refused set touches neither
        ctx.frame_set_lens(state)
        for kw in bad_sets:
            assert remap_set(**kw) == FM_ERR_ARG, kw
            assert b'bad argument' in lib.fm_last_error()
        assert lib.fm_frame_remap_set(None, c(src[0]), c(src[1]), p(good_xy), border) == FM_ERR_ARG
        assert lib.fm_frame_remap_clear(None) == FM_ERR_ARG
        assert np.array_equal(ctx.frame_read(), before)
        check_map_is(state)
    for comp, value in ((0, -64), (0, 32 * (src[0] + 1)), (1, -64), (1, 32 * (src[1] + 1))):     # the ends of the range are in it
        assert remap_set(xy=entry(comp, value)) == 0
    ctx.frame_set_lens(lens)

    # a source of another size while a map is set, on all twelve calls
    ow, oh = other
    img = rng.integers(0, 256, (oh, ow, 3), dtype=np.uint8)
    planar = PlanarFrame.from_buffer(rng.integers(0, 256, frame_bytes(other, '420'), dtype=np.uint8), other, '420')
    packed = PackedFrame(rng.integers(0, 256, (oh, ow, 4), dtype=np.uint8), 'bgrx')
    bayer = BayerFrame(rng.integers(0, 256, (oh, ow), dtype=np.uint8), 'rggb')
    families = [('src', SourceFrame(img), img), ('planar', planar, planar.to_bgr()), ('packed', packed, packed.to_bgr()),
                ('bayer', bayer, bayer.to_bgr())]
    calls = []
    for name, frame, pixels in families:
        d = C.byref(frame.describe())
        calls += [(name, 'upload', lambda d=d, n=name: getattr(lib, f'fm_frame_upload_{n}')(ctx.handle, d), pixels),
                  (name, 'ahead', lambda d=d, n=name: getattr(lib, f'fm_frame_upload_ahead_{n}')(ctx.handle, c(1), d), pixels),
                  (name, 'ring', lambda d=d, n=name: getattr(lib, f'fm_frame_ring_store_{n}')(ctx.handle, c(0), d), pixels)]
    assert len(calls) == 12
    for name, what, call, _ in calls:
        assert call() == FM_ERR_ARG, (name, what)
        assert b'bad argument' in lib.fm_last_error()
    with pytest.raises(_lib.FastMOTHipError):                    # no frame in slot 1: none of the calls above put one there
        ctx.frame_promote_next()
    assert np.array_equal(ctx.frame_read(), before)              # nothing was copied or launched
    ctx.frame_ring_select(0)
    assert np.array_equal(ctx.frame_read(), before)
    check_map_is(lens)
    # the same calls, unmodified, are accepted once the map is gone (and resize) ...
    ctx.frame_set_lens(None)
    for name, what, call, pixels in calls:
        assert call() == 0, (name, what)
        if what == 'ahead':
            ctx.frame_promote_next()
        elif what == 'ring':
            ctx.frame_ring_select(0)
        assert np.array_equal(ctx.frame_read(), resize_bgr(pixels, dst)), (name, what)
        ctx.frame_upload(before)
    # ... and sources of the map's size while it is set
    ctx.frame_set_lens(lens)
    check_map_is(lens)


# ---- MOT.step
def test_tracks_on_lens_frames_equal_host_remapped_frames(ctx):
    from synthetic import SyntheticVideo
    from test_packed_gpu import SIZE, run_mot
    video = SyntheticVideo(SIZE, n_ids=8, n_frames=8, seed=4)
    scale = SIZE[0] / lc.SRC[0]
    k = [420. * scale, 415. * scale, (322.5 + 0.5) * scale - 0.5, (178.25 + 0.5) * scale - 0.5]
    lens = LensMap.pinhole(k, lc.D_BARREL, SIZE, SIZE, border=lc.BORDER)     # the barrel model at the tracker's size
    bgr = [np.ascontiguousarray(f) for f in video.frames]
    host = [remap_bgr(f, lens) for f in bgr]
    assert not np.array_equal(host[0], bgr[0])
    want = run_mot(video, host)
    assert len(want[-1]) >= 6                # (the detections follow the scene, whatever the pixels: as in the packed test)
    assert run_mot(video, [SourceFrame(f, lens=lens) for f in bgr]) == want
    assert np.array_equal(ctx.frame_read(), host[-1])            # the tracker saw the corrected frame
