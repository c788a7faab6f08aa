"""CPU: the numpy statement of the packed-frame conversions (fastmot_amd/utils/packed.py) against the planar reference and
an independent float formula, PackedFrame's validation, VideoIO(pixel_format=...) over '.npy' stacks, and the library's
entry points without a context."""
import ctypes as C

import numpy as np
import pytest

from fastmot_amd import NV12Frame, PackedFrame, PlanarFrame, VideoIO, _lib
from fastmot_amd.utils import packed as P
from fastmot_amd.utils.packed import FORMATS, packed_to_bgr, row_bytes
from fastmot_amd.utils.yuv import planar_to_bgr

FM_ERR_ARG = -2
YUV_FORMATS = ['yuy2', 'uyvy', 'yvyu']
RGB_FORMATS = ['rgb', 'bgr', 'rgbx', 'bgrx', 'xrgb', 'xbgr']
# the decimals of the full-range matrices: CVR, CUB, CUG, CVG
DECIMALS = {'bt601-full': (1.402, 1.772, -0.344136, -0.714136), 'bt709-full': (1.5748, 1.8556, -0.187324, -0.468124)}


def interleave(y, u, v, fmt, pad, rng):
    """Planes y (H, W), u, v (H, ceil(W / 2)) -> (H, 4 * ceil(W / 2) + pad) bytes in the layout `fmt`, written byte by
    byte from the layout's table in the issue (not from FORMATS); padding and an odd width's spare luma byte random."""
    h, w = y.shape
    nm = (w + 1) // 2
    buf = rng.integers(0, 256, (h, 4 * nm + pad), dtype=np.uint8)
    order = {'yuy2': 'YUyV', 'uyvy': 'UYVy', 'yvyu': 'YVyU'}[fmt]
    for r in range(h):
        for m in range(nm):
            for k, what in enumerate(order):
                if what == 'Y':
                    buf[r, 4 * m + k] = y[r, 2 * m]
                elif what == 'y':
                    if 2 * m + 1 < w:
                        buf[r, 4 * m + k] = y[r, 2 * m + 1]
                else:
                    buf[r, 4 * m + k] = (u if what == 'U' else v)[r, m]
    return buf


@pytest.mark.parametrize('fmt', YUV_FORMATS)
def test_limited_range_422_equals_the_planar_reference(fmt):
    rng = np.random.default_rng(11)
    for w in (1, 2, 3, 5, 33, 34):
        for h in (1, 2, 7):
            for pad in (0, 5):
                y = rng.integers(0, 256, (h, w), dtype=np.uint8)
                u = rng.integers(0, 256, (h, (w + 1) // 2), dtype=np.uint8)
                v = rng.integers(0, 256, (h, (w + 1) // 2), dtype=np.uint8)
                y[0] = 0                                   # rows of all-0 and all-255 bytes
                u[0] = v[0] = 0
                if h > 1:
                    y[1] = u[1] = v[1] = 255
                data = interleave(y, u, v, fmt, pad, rng)
                for matrix in ('bt601', 'bt709'):
                    want = planar_to_bgr(y, u, v, '422', matrix)
                    assert np.array_equal(packed_to_bgr(data, (w, h), fmt, matrix), want), (w, h, pad, matrix)
                    f = PackedFrame(data, fmt, (w, h), matrix)
                    assert f.size == (w, h) and f.shape == (h, w, 3) and f.pitch == (data.shape[1] if h > 1 else 4 * ((w + 1) // 2))
                    assert np.array_equal(f.to_bgr(), want)
    assert FORMATS['yuyv'] is FORMATS['yuy2']


@pytest.mark.parametrize('fmt', RGB_FORMATS)
def test_rgb_family_is_the_index_permutation(fmt):
    offsets = {'rgb': (3, 0, 1, 2), 'bgr': (3, 2, 1, 0), 'rgbx': (4, 0, 1, 2), 'bgrx': (4, 2, 1, 0), 'xrgb': (4, 1, 2, 3),
               'xbgr': (4, 3, 2, 1)}                      # the issue's table: bpp, byte offsets of R, G, B
    bpp, r, g, b = offsets[fmt]
    rng = np.random.default_rng(12)
    for w, h in ((1, 1), (3, 2), (34, 7)):
        px = rng.integers(0, 256, (h, w, bpp), dtype=np.uint8)
        want = np.stack([px[..., b], px[..., g], px[..., r]], axis=-1)
        assert np.array_equal(packed_to_bgr(px, None, fmt), want)
        assert np.array_equal(packed_to_bgr(px, (w, h), fmt, 'bt709-full'), want)       # the matrix is not used
        wide = rng.integers(0, 256, (h, w * bpp + 7), dtype=np.uint8)                   # a padded pitch
        wide[:, :w * bpp] = px.reshape(h, -1)
        assert np.array_equal(packed_to_bgr(wide, (w, h), fmt), want)
        for f in (PackedFrame(px, fmt), PackedFrame(wide, fmt, (w, h)), PackedFrame(wide[:, :w * bpp], fmt, (w, h))):
            assert f.size == (w, h) and np.array_equal(f.to_bgr(), want)
            assert f.pitch == (bpp * w if h == 1 or f.data is px else wide.shape[1])
    for alias, name in (('rgba', 'rgbx'), ('bgra', 'bgrx'), ('argb', 'xrgb'), ('abgr', 'xbgr')):
        assert FORMATS[alias] is FORMATS[name]
    assert row_bytes(5, 'rgb') == 15 and row_bytes(5, 'bgrx') == 20 and row_bytes(5, 'uyvy') == 12 and row_bytes(4, 'yuy2') == 8


def test_full_range_constants():
    for name, dec in DECIMALS.items():
        assert P.FULL_COEF[name] == tuple(round(c * 2 ** 20) for c in dec)
    assert P.MATRICES == {'bt601': 0, 'bt709': 1, 'bt601-full': 16, 'bt709-full': 17}


@pytest.mark.parametrize('matrix', sorted(DECIMALS))
def test_full_range_against_float64_over_all_triples(matrix):
    """All 2^24 (Y, U, V): the integer result is within 1 of clip(floor(float64 formula + 0.5)) in every channel and
    equal to it for at least 99 % of the triples (the coefficients are rounded to 2^-21 relative: a disagreement needs a
    float result within about 1e-4 of a half)."""
    cvr, cub, cug, cvg = DECIMALS[matrix]
    u = np.arange(256, dtype=np.uint8)[:, None].repeat(256, 1)
    v = np.arange(256, dtype=np.uint8)[None, :].repeat(256, 0)
    uf, vf = u.astype(np.float64) - 128, v.astype(np.float64) - 128
    chroma = np.stack([cub * uf, cvg * vf + cug * uf, cvr * vf], axis=-1)              # B, G, R
    worst, equal = 0, 0
    for yv in range(256):
        got = P.full_range_to_bgr(np.full((256, 256), yv, np.uint8), u, v, matrix).astype(np.int32)
        want = np.clip(np.floor(yv + chroma + 0.5), 0, 255).astype(np.int32)
        d = np.abs(got - want)
        worst = max(worst, int(d.max()))
        equal += int((d.max(axis=-1) == 0).sum())
    share = equal / 2 ** 24
    print(f'{matrix}: worst channel difference {worst}, equal triples {share:.6%}')
    assert worst <= 1
    assert share >= 0.99


def test_full_range_through_packed_to_bgr():
    rng = np.random.default_rng(13)
    w, h = 5, 3
    y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    u, v = (rng.integers(0, 256, (h, 3), dtype=np.uint8) for _ in range(2))
    cols = np.arange(w) >> 1
    for fmt in YUV_FORMATS:
        data = interleave(y, u, v, fmt, 3, rng)
        for matrix in DECIMALS:
            assert np.array_equal(packed_to_bgr(data, (w, h), fmt, matrix), P.full_range_to_bgr(y, u[:, cols], v[:, cols], matrix))
    # grey stays grey, black black and white white
    grey = np.array([[0, 128, 77, 128, 255, 128, 3, 128]], np.uint8)
    assert packed_to_bgr(grey, (4, 1), 'yuy2', 'bt601-full').tolist() == [[[0] * 3, [77] * 3, [255] * 3, [3] * 3]]


def test_packed_frame_validation():
    rng = np.random.default_rng(14)
    w, h = 6, 4
    yuv = rng.integers(0, 256, (h, 2 * w), dtype=np.uint8)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    with pytest.raises(ValueError):
        PackedFrame(yuv, 'nv12', (w, h))                          # unknown format
    with pytest.raises(ValueError):
        PackedFrame(yuv, 'yuy2', (w, h), matrix='bt2020')         # unknown matrix
    with pytest.raises(ValueError):
        PackedFrame(rgb, 'rgb', matrix='bt601-limited')
    with pytest.raises(ValueError):
        PackedFrame(yuv[:, :2 * w - 1], 'yuy2', (w, h))           # rows one byte short
    with pytest.raises(ValueError):
        PackedFrame(np.lib.stride_tricks.as_strided(yuv, (h, 2 * w), (2 * w - 1, 1)), 'yuy2', (w, h))   # pitch below the row
    with pytest.raises(ValueError):
        PackedFrame(yuv[::-1], 'yuy2', (w, h))                    # negative pitch
    with pytest.raises(ValueError):
        PackedFrame(np.zeros((h, 4 * w), np.uint8)[:, ::2], 'yuy2', (w, h))            # bytes not adjacent
    with pytest.raises(ValueError):
        PackedFrame(np.zeros((h, w, 6), np.uint8)[:, :, ::2], 'rgb')
    with pytest.raises(ValueError):
        PackedFrame(np.zeros((h, 2 * w, 3), np.uint8)[:, ::2], 'rgb')
    with pytest.raises(ValueError):
        PackedFrame(rgb, 'rgbx')                                  # 3 bytes per pixel where the layout has 4
    with pytest.raises(ValueError):
        PackedFrame(rgb, 'yuy2')                                  # a 4:2:2 frame is rows of bytes
    with pytest.raises(ValueError):
        PackedFrame(yuv, 'yuy2')                                  # ... and needs its size
    with pytest.raises(ValueError):
        PackedFrame(yuv, 'yuy2', (w, h + 1))
    with pytest.raises(ValueError):
        PackedFrame(rgb, 'rgb', (w + 1, h))
    for size in ((0, h), (w, 0)):                                 # empty
        with pytest.raises(ValueError):
            PackedFrame(np.zeros((size[1], 2 * size[0]), np.uint8), 'yuy2', size)
        with pytest.raises(ValueError):
            PackedFrame.from_buffer(bytes(64), size, 'yuy2')
    with pytest.raises(ValueError):
        PackedFrame(np.zeros((0, w, 3), np.uint8), 'rgb')
    with pytest.raises(TypeError):
        PackedFrame(yuv.astype(np.int16), 'yuy2', (w, h))
    with pytest.raises(TypeError):
        PackedFrame(yuv.tolist(), 'yuy2', (w, h))
    # from_buffer
    buf = rng.integers(0, 256, 16 * (h - 1) + 12 + 3, dtype=np.uint8)
    f = PackedFrame.from_buffer(buf, (w, h), 'uyvy', pitch=16, matrix='bt709-full')
    assert f.pitch == 16 and f.matrix == 'bt709-full' and f.format == 'uyvy' and f.size == (w, h)
    rows = np.stack([buf[16 * r:16 * r + 12] for r in range(h)])
    assert np.array_equal(f.to_bgr(), packed_to_bgr(rows, (w, h), 'uyvy', 'bt709-full'))
    assert PackedFrame.from_buffer(bytes(buf[:48]), (w, h), 'yuy2').pitch == 12
    with pytest.raises(ValueError):
        PackedFrame.from_buffer(buf, (w, h), 'uyvy', pitch=11)    # short pitch
    with pytest.raises(ValueError):
        PackedFrame.from_buffer(buf[:16 * (h - 1) + 11], (w, h), 'uyvy', pitch=16)     # short buffer
    with pytest.raises(ValueError):
        PackedFrame.from_buffer(buf, (w, h), 'i420')
    with pytest.raises(ValueError):
        PackedFrame.from_buffer(buf, (w, h), 'uyvy', matrix='bt2020')
    with pytest.raises(ValueError):
        PackedFrame.from_buffer(np.zeros((8, 32), np.uint8)[:, ::2], (w, h), 'uyvy')
    # the description the library gets
    d = f.describe()
    assert (d.format, d.width, d.height, d.pitch, d.matrix) == (7, w, h, 16, 17) and d.data == buf.__array_interface__['data'][0]
    assert f.describe() is d and f.data.base is not None          # the frame keeps its array


def test_struct_matches_header():
    """fm_frame_packed as a C compiler lays it out (LP64): five int32, then an 8-byte aligned pointer."""
    F = P.FramePacked
    assert [getattr(F, n).offset for n in ('format', 'width', 'height', 'pitch', 'matrix', 'data')] == [0, 4, 8, 12, 16, 24]
    assert C.sizeof(F) == 32


def test_other_frame_kinds_keep_their_matrices():
    y, uv = np.zeros((4, 4), np.uint8), np.zeros((2, 4), np.uint8)
    for matrix in ('bt601-full', 'bt709-full', 'bt2020'):
        with pytest.raises(ValueError):
            NV12Frame(y, uv, matrix)
        with pytest.raises(ValueError):
            PlanarFrame(y, chroma='mono', matrix=matrix)
    from fastmot_amd.utils.nv12 import MATRICES
    assert sorted(MATRICES) == ['bt601', 'bt709']


def test_source_frame_takes_a_packed_frame():
    from fastmot_amd import SourceFrame
    f = PackedFrame(np.zeros((5, 7, 4), np.uint8), 'bgrx')
    s = SourceFrame(f)
    assert s.size == (7, 5) and s.shape == (5, 7, 3) and s.frame is f
    with pytest.raises(TypeError):
        s.describe()


def test_packed_entry_points_refuse_null_arguments():
    lib = _lib.load()
    d = PackedFrame(np.zeros((3, 5, 3), np.uint8), 'rgb').describe()
    c = C.c_int
    for rc in (lib.fm_frame_upload_packed(None, None), lib.fm_frame_upload_packed(None, C.byref(d)),
               lib.fm_frame_upload_ahead_packed(None, c(1), None), lib.fm_frame_upload_ahead_packed(None, c(1), C.byref(d)),
               lib.fm_frame_ring_store_packed(None, c(0), None), lib.fm_frame_ring_store_packed(None, c(0), C.byref(d))):
        assert rc == FM_ERR_ARG
        assert b'bad argument' in lib.fm_last_error()


# ---- VideoIO(pixel_format=...)
def read_all(video):
    video.start_capture()
    out = []
    while True:
        f = video.read()
        if f is None:
            break
        out.append(f)
    video.release()
    return out


@pytest.fixture(scope='module')
def stacks(tmp_path_factory):
    d = tmp_path_factory.mktemp('packed')
    rng = np.random.default_rng(15)
    out = {'yuy2': rng.integers(0, 256, (4, 18, 68), dtype=np.uint8),             # 34 x 18
           'rgbx': rng.integers(0, 256, (4, 18, 34, 4), dtype=np.uint8),
           'bgr': rng.integers(0, 256, (4, 18, 34, 3), dtype=np.uint8)}
    for name, a in out.items():
        np.save(d / f'{name}.npy', a)
    np.save(d / 'rgbx_rows.npy', out['rgbx'].reshape(4, 18, -1))
    return d, out


def test_videoio_converts_on_the_capture_thread(stacks):
    from fastmot_amd.videoio import resize_bgr
    d, data = stacks
    for fmt, matrix in (('yuy2', 'bt601'), ('yuy2', 'bt709-full'), ('rgbx', 'bt601')):
        video = VideoIO((34, 18), str(d / f'{fmt}.npy'), pixel_format=fmt, yuv_matrix=matrix)
        assert video.resolution == (34, 18)
        got = read_all(video)
        assert len(got) == 4
        for g, raw in zip(got, data[fmt]):
            assert isinstance(g, np.ndarray) and np.array_equal(g, packed_to_bgr(raw.reshape(18, -1), (34, 18), fmt, matrix))
    got = read_all(VideoIO((34, 18), str(d / 'rgbx_rows.npy'), pixel_format='rgba'))
    assert np.array_equal(got[3], packed_to_bgr(data['rgbx'][3], None, 'rgbx'))
    # another size: resized here, as every other input is
    got = read_all(VideoIO((17, 9), str(d / 'yuy2.npy'), pixel_format='yuy2'))
    assert np.array_equal(got[0], resize_bgr(packed_to_bgr(data['yuy2'][0], (34, 18), 'yuy2'), (17, 9)))
    # stream_cfg reaches it as a keyword
    video = VideoIO((34, 18), str(d / 'yuy2.npy'), None, **{'buffer_size': 3, 'pixel_format': 'yuyv'})
    assert np.array_equal(read_all(video)[0], packed_to_bgr(data['yuy2'][0], (34, 18), 'yuy2'))


def test_videoio_frame_kinds(stacks):
    """gpu_decode / gpu_resize choose the frame kind as they do for a '.y4m' input (no GPU is touched by reading)."""
    from fastmot_amd import SourceFrame
    d, data = stacks
    got = read_all(VideoIO((34, 18), str(d / 'yuy2.npy'), pixel_format='yuy2', gpu_decode=True, yuv_matrix='bt601-full'))
    assert all(isinstance(g, PackedFrame) and g.size == (34, 18) and g.matrix == 'bt601-full' for g in got) and len(got) == 4
    assert np.array_equal(got[2].to_bgr(), packed_to_bgr(data['yuy2'][2], (34, 18), 'yuy2', 'bt601-full'))
    got = read_all(VideoIO((17, 9), str(d / 'rgbx.npy'), pixel_format='rgbx', gpu_decode=True))
    assert all(isinstance(g, np.ndarray) and g.shape == (9, 17, 3) for g in got)       # no gpu_resize: host pixels
    got = read_all(VideoIO((17, 9), str(d / 'rgbx.npy'), pixel_format='rgbx', gpu_decode=True, gpu_resize=True))
    assert all(isinstance(g, SourceFrame) and isinstance(g.frame, PackedFrame) and g.size == (34, 18) for g in got)
    got = read_all(VideoIO((34, 18), str(d / 'rgbx.npy'), str(d / 'o.npy'), pixel_format='rgbx', gpu_decode=True))
    assert all(isinstance(g, np.ndarray) for g in got)                                  # an output that needs host pixels


def test_videoio_refuses_at_open(stacks, tmp_path):
    d, data = stacks
    with pytest.raises(ValueError):
        VideoIO((34, 18), str(d / 'rgbx.npy'), pixel_format='rgb')                     # 4 bytes per pixel, not 3
    with pytest.raises(ValueError):
        VideoIO((34, 18), str(d / 'rgbx.npy'), pixel_format='yuy2')                    # a 4-D stack is no 4:2:2 stack
    with pytest.raises(ValueError):
        VideoIO((34, 18), str(d / 'bgr.npy'), pixel_format='i420')
    np.save(tmp_path / 'odd.npy', np.zeros((2, 6, 10), np.uint8))
    with pytest.raises(ValueError):
        VideoIO((5, 6), str(tmp_path / 'odd.npy'), pixel_format='uyvy')                # row bytes no multiple of 4
    with pytest.raises(ValueError):
        VideoIO((5, 6), str(tmp_path / 'odd.npy'), pixel_format='rgb')                 # ... nor of 3
    np.save(tmp_path / 'f32.npy', np.zeros((2, 6, 12), np.float32))
    with pytest.raises(ValueError):
        VideoIO((6, 6), str(tmp_path / 'f32.npy'), pixel_format='uyvy')
    with pytest.raises(ValueError):
        VideoIO((34, 18), str(d / 'yuy2.npy'), pixel_format='yuy2', yuv_matrix='bt2020')
    with pytest.raises(ValueError):
        VideoIO((34, 18), str(d / 'missing-%06d.png'), pixel_format='rgb')             # the option belongs to '.npy' stacks


def test_videoio_without_pixel_format_is_unchanged(stacks):
    d, data = stacks
    for kw in ({}, {'pixel_format': None}):
        got = read_all(VideoIO((34, 18), str(d / 'bgr.npy'), **kw))
        assert len(got) == 4 and all(np.array_equal(g, raw) for g, raw in zip(got, data['bgr']))
    with pytest.raises(RuntimeError):                                                   # and a 3-D stack is still no BGR stack
        VideoIO((34, 18), str(d / 'yuy2.npy'))
