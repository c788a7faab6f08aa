"""Host side of the lens path: the arithmetic of csrc/remap_pixel.h as numpy (utils.lens.remap_bgr) and as compiled
(fm_remap_bgr_host) against a float64 statement, the quantisation, the two camera models with their inverses, maps from
arrays, and VideoIO(lens=...).  test_lens_gpu.py compares the kernel (csrc/remap.hip) with remap_bgr bit for bit."""
import ctypes as C

import numpy as np
import pytest

import lens_cases as lc
from fastmot_amd import LensMap, SourceFrame, VideoIO, _lib
from fastmot_amd.utils.lens import quantise, remap_bgr, remap_bgr_host

FM_ERR_ARG = -2


# ---- the arithmetic
def test_integer_formula_is_float64_bilinear_rounded_half_up():
    """All 32 x 32 fractions x 1000 random byte quadruples (per channel: 3000): quadruple i is the 2 x 2 block at columns
    2i, 2i + 1 of a 2000 x 2 source, and the destination's 32 x 32 tile i walks the fractions over it (40 x 25 tiles)."""
    rng = np.random.default_rng(1)
    n = 1000
    frame = rng.integers(0, 256, (2, 2 * n, 3), dtype=np.uint8)
    frame[:, :8] = np.array([[0, 0, 255, 255, 0, 255, 255, 0], [0, 255, 0, 255, 255, 0, 255, 0]], np.uint8)[..., None]   # extremes
    f = np.arange(32)
    quad = np.arange(n).reshape(25, 1, 40, 1)                                # the tiles lie 25 down, 40 across
    xy = np.empty((25, 32, 40, 32, 2), np.int32)
    xy[..., 0] = 64 * quad + f[None, None, None, :]
    xy[..., 1] = f[None, :, None, None]
    lens = LensMap(xy.reshape(25 * 32, 40 * 32, 2), (2 * n, 2))
    a, b = (f / 32.)[None, :, None], (f / 32.)[:, None, None]              # (1, 32, 1), (32, 1, 1)
    p = frame.astype(np.float64).reshape(2, n, 2, 3)                        # [row][quad][col][channel]
    want = np.empty((25, 32, 40, 32, 3))
    for i in range(n):
        top = (1. - a) * p[0, i, 0] + a * p[0, i, 1]
        bot = (1. - a) * p[1, i, 0] + a * p[1, i, 1]
        want[i // 40, :, i % 40] = np.floor((1. - b) * top + b * bot + 0.5)
    want = want.reshape(25 * 32, 40 * 32, 3).astype(np.uint8)
    assert np.array_equal(remap_bgr(frame, lens), want)
    assert np.array_equal(remap_bgr_host(frame, lens), want)


@pytest.mark.parametrize('shape', lc.SHAPES, ids=lc.shape_id)
def test_compiled_twin_equals_numpy(shape):
    (sw, sh), dst = shape
    rng = np.random.default_rng(sw * 7 + dst[0])
    lens = lc.lens_for(rng, (sw, sh), dst)
    frames = lc.boundary_frames() if (sw, sh) == (3, 3) else [rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)]
    for frame in frames:
        assert np.array_equal(remap_bgr_host(frame, lens), remap_bgr(frame, lens))


def test_models_compiled_twin_equals_numpy():
    rng = np.random.default_rng(2)
    frame = rng.integers(0, 256, (lc.SRC[1], lc.SRC[0], 3), dtype=np.uint8)
    for name, lens in lc.models().items():
        assert np.array_equal(remap_bgr_host(frame, lens), remap_bgr(frame, lens)), name


def test_boundary_table_known_answers():
    """A white 3 x 3 source with a black border: a coordinate whose taps are all inside is 255, all outside 0, and on the
    way in the value is the inside taps' weight."""
    lens = lc.boundary_lens(border=(0, 0, 0))
    out = remap_bgr(np.full((3, 3, 3), 255, np.uint8), lens)[..., 0].astype(int)
    vals = lc.boundary_values(3)
    wx = np.array([np.clip(min(v + 32, 64 + 32 - v), 0, 32) for v in vals])         # weight of the inside columns, of 32
    want = (np.outer(wx, wx) * 255 + 512) >> 10
    assert np.array_equal(out, want)
    assert want[0, 0] == 0 and want[5, 5] == 255 and want[2, 5] == 0 and want[3, 5] == (32 * 255 + 512) >> 10


def test_host_twin_bad_arguments():
    lib = _lib.load()
    src, dst = np.zeros((3, 3, 3), np.uint8), np.zeros((2, 2, 3), np.uint8)
    xy = np.zeros((2, 2, 2), np.int32)
    border = (C.c_uint8 * 3)(1, 2, 3)
    p = lambda a: C.c_void_p(a.__array_interface__['data'][0])

    def call(src=p(src), sw=3, sh=3, xy=xy, dst=p(dst), dw=2, dh=2, border=border):
        return lib.fm_remap_bgr_host(src, C.c_int(sw), C.c_int(sh), None if xy is None else p(xy), dst, C.c_int(dw), C.c_int(dh), border)

    assert call() == 0
    for kw in (dict(src=None), dict(xy=None), dict(dst=None), dict(border=None), dict(sw=0), dict(sh=0), dict(sw=-1), dict(sw=16385),
               dict(sh=16385), dict(dw=0), dict(dh=0), dict(dw=16385)):
        assert call(**kw) == FM_ERR_ARG, kw
        assert b'bad argument' in lib.fm_last_error()
    for c, v in ((0, -65), (0, 32 * 4 + 1), (1, -65), (1, 32 * 4 + 1)):
        bad = xy.copy()
        bad[1, 1, c] = v
        assert call(xy=bad) == FM_ERR_ARG, (c, v)
    for c, v in ((0, -64), (0, 32 * 4), (1, -64), (1, 32 * 4)):
        ok = xy.copy()
        ok[1, 1, c] = v
        assert call(xy=ok) == 0, (c, v)


# ---- quantisation and validation
def test_quantise():
    x = np.array([[0.5 / 32, 1.5 / 32, 2.5 / 32, -0.5 / 32, -1.5 / 32, 3.49 / 32, 1.0, np.nan, np.inf, -np.inf, 1e30, -1e30, 1e308, -2.1, 11.0, 12.0]])
    xy = quantise(x, x, (10, 7))
    assert xy.dtype == np.int32 and xy.shape == (1, 16, 2)
    assert list(xy[0, :, 0]) == [0, 2, 2, 0, -2, 3, 32, -64, -64, -64, 352, -64, 352, -64, 352, 352]
    assert list(xy[0, :, 1]) == [0, 2, 2, 0, -2, 3, 32, -64, -64, -64, 256, -64, 256, -64, 256, 256]
    lens = LensMap(xy, (10, 7))                                   # everything quantise makes is in range
    out = remap_bgr(np.full((7, 10, 3), 200, np.uint8), lens)
    assert np.all(out[0, 7:] == 0) and np.all(out[0, 6] == 200)   # the non-finite and far-outside entries are fully outside


def test_lensmap_validates():
    xy = np.zeros((4, 6, 2), np.int32)
    lens = LensMap(xy, (5, 3), border=(1, 2, 3))
    assert lens.dst_size == (6, 4) and lens.src_size == (5, 3) and lens.border == (1, 2, 3)
    assert lens.xy.flags.c_contiguous and not lens.xy.flags.writeable and lens.xy.dtype == np.int32
    xy[0, 0, 0] = 5                                               # the caller's array is not the map's
    assert lens.xy[0, 0, 0] == 0
    strided = LensMap(np.zeros((4, 6, 4), np.int32)[..., ::2], (5, 3))
    assert strided.xy.flags.c_contiguous
    for bad in (np.zeros((4, 6), np.int32), np.zeros((4, 6, 3), np.int32), np.zeros((4, 6, 2), np.int64), np.zeros((4, 6, 2), np.float32),
                np.zeros((0, 6, 2), np.int32), np.zeros((4, 6, 2), np.int32).tolist()):
        with pytest.raises(ValueError):
            LensMap(bad, (5, 3))
    for c, v, ok in ((0, -65, False), (0, -64, True), (0, 32 * 6, True), (0, 32 * 6 + 1, False),
                     (1, -65, False), (1, -64, True), (1, 32 * 4, True), (1, 32 * 4 + 1, False)):
        m = np.zeros((4, 6, 2), np.int32)
        m[3, 5, c] = v
        if ok:
            LensMap(m, (5, 3))
        else:
            with pytest.raises(ValueError):
                LensMap(m, (5, 3))
    for size in ((0, 3), (5, 0), (16385, 3)):
        with pytest.raises(ValueError):
            LensMap(np.zeros((4, 6, 2), np.int32), size)
    for border in ((0, 0), (0, 0, 256), (-1, 0, 0)):
        with pytest.raises(ValueError):
            LensMap(np.zeros((4, 6, 2), np.int32), (5, 3), border)
    with pytest.raises(ValueError):
        lens.to_source([[0., 0.]])                                # only the model constructors know an inverse
    with pytest.raises(ValueError):
        remap_bgr(np.zeros((4, 5, 3), np.uint8), lens)            # a frame of another size
    with pytest.raises(ValueError):
        SourceFrame(np.zeros((4, 5, 3), np.uint8), lens=lens)
    assert SourceFrame(np.zeros((3, 5, 3), np.uint8), lens=lens).lens is lens
    assert SourceFrame(np.zeros((3, 5, 3), np.uint8)).lens is None


# ---- the models
def test_pinhole_without_distortion_is_the_scale_map():
    (sw, sh), (dw, dh) = lc.SRC, lc.DST
    for d in ((0, 0, 0, 0), (0, 0, 0, 0, 0), (0,) * 8):
        lens = LensMap.pinhole(lc.K_PINHOLE, d, lc.SRC, lc.DST)
        u, v = np.meshgrid(np.arange(dw, dtype=np.float64), np.arange(dh, dtype=np.float64))
        # pixel centres: destination pixel u covers source [u sw / dw, (u + 1) sw / dw), whatever the principal point is
        want = np.stack([(u + 0.5) * sw / dw - 0.5, (v + 0.5) * sh / dh - 0.5], axis=-1)
        got = lens.to_source(np.stack([u, v], axis=-1))
        assert np.max(np.abs(got - want)) < 1e-9
        assert np.max(np.abs(lens.xy - quantise(want[..., 0], want[..., 1], lc.SRC))) <= 1      # (a tie may fall either way)
    zoomed = LensMap.pinhole(lc.K_PINHOLE, (0, 0, 0, 0), lc.SRC, lc.DST, zoom=2.0)
    centre = zoomed.to_source([[(322.5 + 0.5) * dw / sw - 0.5, (178.25 + 0.5) * dh / sh - 0.5]])
    assert np.allclose(centre, [[322.5, 178.25]], atol=1e-9)
    corner = zoomed.to_source([[-0.5, -0.5]])                      # the picture's corner: half as far from the centre as without zoom
    assert np.allclose(corner, [[322.5 + (-0.5 - 322.5) / 2, 178.25 + (-0.5 - 178.25) / 2]], atol=1e-9)
    explicit = LensMap.pinhole(lc.K_PINHOLE, lc.D_BARREL, lc.SRC, lc.DST, new_camera_matrix=(300., 290., 200., 100.))
    assert np.allclose(explicit.to_source([[200., 100.]]), [[322.5, 178.25]], atol=1e-9)        # principal point to principal point
    for bad in ((0, 0, 0), (0,) * 6, (0,) * 9, (np.nan, 0, 0, 0)):
        with pytest.raises(ValueError):
            LensMap.pinhole(lc.K_PINHOLE, bad, lc.SRC, lc.DST)
    with pytest.raises(ValueError):
        LensMap.fisheye(lc.K_FISHEYE, (0, 0, 0, 0, 0), lc.SRC, lc.DST)


def test_models_inside_outside_and_round_trip():
    """Round trip to_destination(to_source(p)) over the whole destination grid: 1e-6 px, the stop criterion (1e-12 in
    normalised units) times the focal length with three orders of margin."""
    dw, dh = lc.DST
    u, v = np.meshgrid(np.arange(dw, dtype=np.float64), np.arange(dh, dtype=np.float64))
    grid = np.stack([u, v], axis=-1)
    outside = {}
    for name, lens in lc.models().items():
        back = lens.to_destination(lens.to_source(grid))
        err = np.max(np.abs(back - grid))
        print(name, 'round trip', err)
        assert err < 1e-6, name
        x, y = lens.xy[..., 0], lens.xy[..., 1]
        outside[name] = float(np.mean((x < 0) | (x > 32 * (lc.SRC[0] - 1)) | (y < 0) | (y > 32 * (lc.SRC[1] - 1))))
        # the map IS the closed form, quantised
        src = lens.to_source(grid)
        assert np.array_equal(lens.xy, quantise(src[..., 0], src[..., 1], lc.SRC)), name
    print(outside)
    assert outside['barrel'] == 0 and outside['fisheye'] == 0
    assert 0.09 < outside['pincushion'] < 0.096 and 0.058 < outside['fisheye-zoom0.6'] < 0.064     # the border is exercised
    _, _, _, (nfx, nfy, ncx, ncy) = lc.fisheye(0.6)._model
    theta = np.degrees(np.arctan(np.hypot((grid[..., 0] - ncx) / nfx, (grid[..., 1] - ncy) / nfy)))
    assert 69. < theta.max() < 70.


def test_from_config():
    cfg = {'model': 'fisheye', 'camera_matrix': lc.K_FISHEYE, 'dist_coeffs': list(lc.D_FISHEYE), 'zoom': 0.6, 'border': list(lc.BORDER)}
    lens = LensMap.from_config(cfg, lc.SRC, lc.DST)
    assert np.array_equal(lens.xy, lc.fisheye(0.6).xy) and lens.border == lc.BORDER
    flat = LensMap.from_config({'camera_matrix': [420., 415., 322.5, 178.25], 'dist_coeffs': lc.D_BARREL}, lc.SRC, lc.DST)
    assert np.array_equal(flat.xy, lc.barrel().xy) and flat.border == (0, 0, 0)
    for bad in ({'model': 'thin-prism', 'camera_matrix': lc.K_PINHOLE, 'dist_coeffs': lc.D_BARREL}, {'camera_matrix': lc.K_PINHOLE},
                {'camera_matrix': lc.K_PINHOLE, 'dist_coeffs': lc.D_BARREL, 'zooom': 1}):
        with pytest.raises(ValueError):
            LensMap.from_config(bad, lc.SRC, lc.DST)


# ---- maps from arrays
def test_from_arrays_rotation_mirror_translation():
    rng = np.random.default_rng(4)
    sw, sh = 23, 17
    frame = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    border = lc.BORDER
    # rotation by 90 degrees (np.rot90: counter-clockwise): destination sh x sw ... as (W, H) = (sh, sw)
    v, u = np.meshgrid(np.arange(sw, dtype=np.float64), np.arange(sh, dtype=np.float64), indexing='ij')    # dst rows v < sw, columns u < sh
    rot = LensMap.from_arrays(sw - 1 - v, u, (sw, sh), border)
    assert rot.dst_size == (sh, sw)
    assert np.array_equal(remap_bgr(frame, rot), np.rot90(frame))
    assert np.array_equal(remap_bgr_host(frame, rot), np.rot90(frame))
    # mirror
    y, x = np.meshgrid(np.arange(sh, dtype=np.float64), np.arange(sw, dtype=np.float64), indexing='ij')
    mirror = LensMap.from_arrays(sw - 1 - x, y, (sw, sh), border)
    assert np.array_equal(remap_bgr(frame, mirror), frame[:, ::-1])
    # identity: the frame itself
    assert np.array_equal(remap_bgr(frame, LensMap.from_arrays(x, y, (sw, sh), border)), frame)
    # translation by (+5, -3): dst(x, y) = src(x - 5, y + 3); the vacated band is the border colour
    shift = LensMap.from_arrays(x - 5, y + 3, (sw, sh), border)
    for fn in (remap_bgr, remap_bgr_host):
        out = fn(frame, shift)
        assert np.array_equal(out[:sh - 3, 5:], frame[3:, :sw - 5])
        assert np.all(out[:, :5] == border) and np.all(out[sh - 3:] == border)


# ---- VideoIO
def test_videoio_lens(tmp_path):
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (4, lc.SRC[1], lc.SRC[0], 3), dtype=np.uint8)
    path = str(tmp_path / 'stack.npy')
    np.save(path, frames)
    cfg = {'model': 'pinhole', 'camera_matrix': lc.K_PINHOLE, 'dist_coeffs': list(lc.D_PINCUSHION), 'border': list(lc.BORDER)}
    want_lens = lc.pincushion()

    def frames_of(stream):
        stream.start_capture()
        out = []
        while (f := stream.read()) is not None:
            out.append(f)
        stream.release()
        return out

    stream = VideoIO(lc.DST, path, buffer_size=2, lens=cfg)
    assert np.array_equal(stream.lens.xy, want_lens.xy) and stream.lens.border == lc.BORDER
    got = frames_of(stream)
    assert len(got) == 4 and all(isinstance(f, np.ndarray) for f in got)
    assert all(np.array_equal(g, remap_bgr(f, want_lens)) for g, f in zip(got, frames))

    stream = VideoIO(lc.DST, path, buffer_size=2, lens=cfg, gpu_resize=True)
    got = frames_of(stream)
    assert len(got) == 4 and all(isinstance(f, SourceFrame) for f in got)
    assert all(f.lens is stream.lens for f in got)                        # one object for all frames: the context never switches
    assert all(np.array_equal(g.frame, f) for g, f in zip(got, frames))

    # frames already at `size`: wrapped too under gpu_resize, remapped here without it; an output keeps host pixels
    on_size = lc.barrel(dst=lc.SRC)
    stream = VideoIO(lc.SRC, path, buffer_size=2, lens=on_size, gpu_resize=True)
    assert not stream.do_resize and stream.lens is on_size
    got = frames_of(stream)
    assert all(isinstance(f, SourceFrame) and f.lens is on_size for f in got)
    got = frames_of(VideoIO(lc.SRC, path, buffer_size=2, lens=on_size))
    assert all(np.array_equal(g, remap_bgr(f, on_size)) for g, f in zip(got, frames))
    got = frames_of(VideoIO(lc.SRC, path, str(tmp_path / 'out.npy'), buffer_size=2, lens=on_size, gpu_resize=True))
    assert all(np.array_equal(g, remap_bgr(f, on_size)) for g, f in zip(got, frames))
    with pytest.raises(ValueError):
        VideoIO(lc.DST, path, lens=on_size)                               # a map for another destination size
    # no lens: as before
    got = frames_of(VideoIO(lc.SRC, path, buffer_size=2, gpu_resize=True))
    assert all(isinstance(f, np.ndarray) for f in got)
