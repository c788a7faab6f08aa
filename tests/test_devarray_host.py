"""CPU: frames in device memory (DeviceArrayFrame) -- the numpy statement `utils.devarray.to_bgr` against independent
statements of the four conversions, the parsing of `__cuda_array_interface__` (fake objects that carry a hand-written
dict: nothing here touches a GPU), fm_frame_device_check rule by rule, and the ctypes struct against the header."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from fastmot_amd import DeviceArrayFrame, SourceFrame, _lib
from fastmot_amd.utils import devarray as D
from fastmot_amd.utils.nv12 import nv12_to_bgr
from fastmot_amd.utils.packed import packed_to_bgr

ROOT = Path(__file__).resolve().parents[1]
FM_ERR_ARG = -2
PTR = 0x7f0000100000          # an address no test dereferences


class Fake:
    """An object that publishes a hand-written __cuda_array_interface__."""

    def __init__(self, shape, typestr='|u1', ptr=PTR, strides=None, version=2, **extra):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(ptr, False), strides=strides,
                                             version=version, **extra)


# ---- to_bgr
def test_hwc_equals_packed_to_bgr():
    rng = np.random.default_rng(1)
    for c, orders in ((3, ['rgb', 'bgr']), (4, ['rgbx', 'bgrx', 'xrgb', 'xbgr', 'rgba', 'bgra', 'argb', 'abgr'])):
        a = rng.integers(0, 256, (7, 5, c), dtype=np.uint8)
        for order in orders:
            assert np.array_equal(D.to_bgr(a, order), packed_to_bgr(a, None, order)), order
    a = rng.integers(0, 256, (7, 5, 4), dtype=np.uint8)
    assert np.array_equal(D.to_bgr(a, 'rgb'), a[..., [2, 1, 0]])          # 'rgb' on four bytes: 'rgbx'
    assert np.array_equal(D.to_bgr(a, 'xbgr'), a[..., [1, 2, 3]])


def test_chw_u8_is_a_permutation():
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (3, 6, 9), dtype=np.uint8)
    assert np.array_equal(D.to_bgr(a, 'bgr'), a.transpose(1, 2, 0))
    assert np.array_equal(D.to_bgr(a, 'rgb'), a[::-1].transpose(1, 2, 0))
    assert D.to_bgr(a, 'rgb').flags.c_contiguous


def test_nv12_equals_nv12_to_bgr():
    rng = np.random.default_rng(3)
    y, uv = rng.integers(0, 256, (6, 8), dtype=np.uint8), rng.integers(0, 256, (3, 8), dtype=np.uint8)
    for matrix in ('bt601', 'bt709'):
        assert np.array_equal(D.to_bgr((y, uv), matrix=matrix), nv12_to_bgr(y, uv, matrix))
    with pytest.raises(ValueError):
        D.to_bgr((y, uv), matrix='bt601-full')


def float_reference(x, scale):
    """The float conversions without float32 arithmetic: the float64 product of two float32 values is exact (48 bits), its
    rounding to float32 is the IEEE float32 product; np.round rounds half to even."""
    with np.errstate(invalid='ignore', over='ignore'):
        p = (np.asarray(x, np.float32).astype(np.float64) * float(scale)).astype(np.float32).astype(np.float64)
        r = np.round(p)
    r[np.isnan(r)] = 0
    return np.clip(r, 0, 255).astype(np.uint8)


def test_float_rounding_at_exact_halves():
    k = np.arange(0, 256, dtype=np.float32)
    halves = (k + np.float32(0.5)).reshape(1, 1, -1).repeat(3, axis=0)             # exact in float32 (and in float16)
    want = np.minimum(np.where(k % 2 == 0, k, k + 1), 255).astype(np.uint8)         # half to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    got = D.to_bgr(halves, 'bgr', float_range=(0, 255))
    assert np.array_equal(got[0, :, 0], want) and np.array_equal(got[0, :, 2], want)
    assert np.array_equal(D.to_bgr(halves.astype(np.float16), 'bgr', float_range=(0, 255))[0, :, 1], want)
    # (k + 0.5) / 255 is no float32: the product decides, rounded once
    x = ((np.arange(0, 256) + 0.5) / 255).astype(np.float32).reshape(1, 1, -1).repeat(3, axis=0)
    assert np.array_equal(D.to_bgr(x, 'bgr'), float_reference(x, 255).transpose(1, 2, 0))
    for nudge in (-1, 1):                                                           # ... and its float32 neighbours
        y = np.nextafter(x, np.float32(nudge * 9), dtype=np.float32)
        assert np.array_equal(D.to_bgr(y, 'bgr'), float_reference(y, 255).transpose(1, 2, 0))


def test_float_special_values():
    x = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, -1e-3, -5.0, 1.0, 1.0 + 2 ** -20, 1.002, 7.5, 3e38, -3e38, 1e-45, 0.25],
                 np.float32)
    want01 = np.array([0, 0, 255, 0, 0, 0, 0, 255, 255, 255, 255, 255, 0, 0, 64], np.uint8)
    want255 = np.array([0, 0, 255, 0, 0, 0, 0, 1, 1, 1, 8, 255, 0, 0, 0], np.uint8)
    planes = x.reshape(1, 1, -1).repeat(3, axis=0)
    assert np.array_equal(D.to_bgr(planes, 'rgb')[0, :, 0], want01)
    assert np.array_equal(D.to_bgr(planes, 'rgb', float_range=(0, 255))[0, :, 2], want255)
    assert np.array_equal(D.quantise(x), float_reference(x, 255))
    for bad in ((0, 2), (1, 0), None, (0, 1, 2), 255):
        with pytest.raises(ValueError):
            D.to_bgr(planes, 'rgb', float_range=bad)


def test_every_float16_bit_pattern():
    x = np.arange(65536, dtype=np.uint16).view(np.float16)
    for rng_, scale in (((0, 1), 255), ((0, 255), 1)):
        got = D.quantise(x, rng_)
        assert np.array_equal(got, float_reference(x.astype(np.float32), scale))
    # the product of a float16 (11 bits) and 255 (8 bits) is exact in float32: the plain float64 statement holds too
    with np.errstate(invalid='ignore', over='ignore'):
        r = np.round(x.astype(np.float64) * 255)
    r[np.isnan(r)] = 0
    assert np.array_equal(D.quantise(x), np.clip(r, 0, 255).astype(np.uint8))


def test_to_bgr_refuses_what_the_frame_refuses():
    for shape, dtype in (((3, 5, 3), np.uint8), ((3, 5, 4), np.uint8), ((5, 6, 3), np.float32), ((5, 6), np.uint8), ((5, 6, 2), np.uint8),
                         ((3, 5, 6), np.int16), ((4, 5, 6), np.uint8), ((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            D.to_bgr(np.zeros(shape, dtype))
    with pytest.raises(ValueError):
        D.to_bgr(np.zeros((4, 5, 3), np.uint8), 'rgbx')
    # a shape that is both layouts is whichever `layout` says
    a = np.random.default_rng(4).integers(0, 256, (3, 5, 3), dtype=np.uint8)
    assert np.array_equal(D.to_bgr(a, 'bgr', layout='hwc'), a) and np.array_equal(D.to_bgr(a, 'bgr', layout='chw'), a.transpose(1, 2, 0))
    for shape, dtype, layout in (((4, 5, 3), np.uint8, 'chw'), ((3, 5, 6), np.uint8, 'hwc'), ((3, 5, 3), np.float32, 'hwc'), ((3, 5, 3), np.uint8, 'nv12')):
        with pytest.raises(ValueError):
            D.to_bgr(np.zeros(shape, dtype), layout=layout)
    with pytest.raises(ValueError):
        D.to_bgr(np.zeros((3, 5, 6), np.uint8), 'bgrx')


# ---- interface parsing
def test_contiguous_frames():
    f = DeviceArrayFrame(Fake((5, 7, 3)))
    assert (f.layout, f.size, f.shape, f.order) == ('hwc', (7, 5), (5, 7, 3), 'rgb')
    assert f.planes == [(PTR, 21)] and f.stream == 0 and not f.ready and f.done()
    d = f.descriptor()
    assert (d.width, d.height, d.layout, d.dtype, d.format, d.flags) == (7, 5, D.FM_DEV_HWC, D.FM_DEV_U8, 0, 0)
    assert (d.plane[0], d.plane[1], d.plane[2], d.pitch[0], d.stream) == (PTR, None, None, 21, None)
    f = DeviceArrayFrame(Fake((5, 7, 4)), order='bgr', ready=True)
    assert (f.order, f.format_id, f.planes, f.descriptor().flags) == ('bgrx', 3, [(PTR, 28)], D.FM_DEV_READY)
    assert DeviceArrayFrame(Fake((5, 7, 4)), order='argb').format_id == 4
    for typestr, dt, es in (('|u1', D.FM_DEV_U8, 1), ('<f2', D.FM_DEV_F16, 2), ('<f4', D.FM_DEV_F32, 4)):
        f = DeviceArrayFrame(Fake((3, 5, 7), typestr), order='bgr', float_range=(0, 255))
        assert (f.layout, f.size, f.dtype_id, f.format_id, f.scale) == ('chw', (7, 5), dt, D.FM_DEV_ORDER_BGR, 1.0)
        assert f.planes == [(PTR + c * 35 * es, 7 * es) for c in range(3)]
        assert f.descriptor().scale == 1.0 and DeviceArrayFrame(Fake((3, 5, 7), typestr)).descriptor().scale == 255.0
    assert 'hwc 7x5 uint8 rgb' in DeviceArrayFrame(Fake((5, 7, 3))).describe()
    # (3, H, 3 | 4) is both: `layout` decides
    assert DeviceArrayFrame(Fake((3, 5, 3)), layout='hwc').size == (5, 3) and DeviceArrayFrame(Fake((3, 5, 4)), layout='chw').size == (4, 5)
    assert DeviceArrayFrame(Fake((3, 5, 3), '<f4')).layout == 'chw'                    # (float frames are (3, H, W) only)


def test_strided_and_offset_views():
    # rows of a wider (H, 40, 3) array, from its pixel 2 on: an odd pitch is fine
    f = DeviceArrayFrame(Fake((5, 7, 3), ptr=PTR + 7, strides=(121, 3, 1)))
    assert f.planes == [(PTR + 7, 121)]
    # planes far apart, rows padded, an odd element offset
    f = DeviceArrayFrame(Fake((3, 5, 7), '<f2', ptr=PTR + 6, strides=(1000, 18, 2)))
    assert f.planes == [(PTR + 6, 18), (PTR + 1006, 18), (PTR + 2006, 18)]
    # a single row: its stride means nothing
    assert DeviceArrayFrame(Fake((1, 7, 3), strides=(0, 3, 1))).planes == [(PTR, 21)]
    assert DeviceArrayFrame(Fake((3, 1, 7), '<f4', strides=(64, 0, 4))).planes == [(PTR, 28), (PTR + 64, 28), (PTR + 128, 28)]
    # a broadcast channel: three planes at one address
    assert DeviceArrayFrame(Fake((3, 5, 7), strides=(0, 7, 1))).planes == [(PTR, 7)] * 3


def test_rejections():
    for kw in (dict(layout='chw'), dict(layout='nv12')):
        with pytest.raises(ValueError):
            DeviceArrayFrame(Fake((5, 7, 3)), **kw)
    bad = [dict(shape=(3, 5, 3)), dict(shape=(3, 5, 4)),                       # both layouts
           dict(shape=(5, 7, 3), strides=(42, 6, 2)), dict(shape=(5, 7, 3), strides=(42, 6, 1)),      # inner strides
           dict(shape=(3, 5, 7), typestr='<f4', strides=(280, 56, 8)), dict(shape=(3, 5, 7), strides=(35, 1, 5)),
           dict(shape=(5, 7, 3), strides=(-21, 3, 1)), dict(shape=(3, 5, 7), strides=(-35, 7, 1)),    # negative strides
           dict(shape=(3, 5, 7), strides=(35, -7, 1)), dict(shape=(5, 7, 3), strides=(21, 3, -1)),
           dict(shape=(5, 7, 3), strides=(20, 3, 1)), dict(shape=(3, 5, 7), typestr='<f2', strides=(70, 12, 2)),   # pitch < row
           dict(shape=(5, 7, 3), typestr='<f4'), dict(shape=(5, 7, 3), typestr='<f2'),                # float HWC
           dict(shape=(3, 5, 7), typestr='<f8'), dict(shape=(3, 5, 7), typestr='<i2'), dict(shape=(3, 5, 7), typestr='>f4'),
           dict(shape=(5, 7)), dict(shape=(5, 7, 2)), dict(shape=(2, 5, 7, 3)), dict(shape=(0, 7, 3)), dict(shape=(3, 5, 0)),
           dict(shape=(5, 7, 3), ptr=0), dict(shape=(3, 5, 7), typestr='<f4', ptr=PTR + 2),           # null, misaligned
           dict(shape=(3, 5, 7), typestr='<f4', strides=(142, 28, 4)), dict(shape=(3, 5, 7), typestr='<f2', strides=(70, 15, 2)),
           dict(shape=(5, 16385, 3)), dict(shape=(3, 16385, 4), typestr='<f4'),
           dict(shape=(5, 7, 3), strides=(21, 3)), dict(shape=(5, 7, 3), mask=object())]
    for kw in bad:
        with pytest.raises(ValueError):
            DeviceArrayFrame(Fake(**kw))
    for order in ('rgbx', 'yuy2', 'xyz', None, 3):
        with pytest.raises(ValueError):
            DeviceArrayFrame(Fake((5, 7, 3)), order=order)
    for order in ('rgbx', 'xbgr', 'uyvy'):
        with pytest.raises(ValueError):
            DeviceArrayFrame(Fake((3, 5, 7)), order=order)
    with pytest.raises(ValueError):
        DeviceArrayFrame(Fake((5, 7, 4)), order='yvyu')
    with pytest.raises(ValueError):
        DeviceArrayFrame(Fake((3, 5, 7), '<f4'), float_range=(0, 100))
    with pytest.raises(ValueError):
        DeviceArrayFrame(Fake((5, 7, 3)), stream=-1)
    for host in (np.zeros((5, 7, 3), np.uint8), [[1]], None):
        with pytest.raises(TypeError):
            DeviceArrayFrame(host)


def test_stream_pick_up():
    class S:
        cuda_stream = 0x5555
    assert DeviceArrayFrame(Fake((5, 7, 3))).stream == 0                                      # v2: none published
    assert DeviceArrayFrame(Fake((5, 7, 3), version=3, stream=None)).stream == 0
    assert DeviceArrayFrame(Fake((5, 7, 3), version=3, stream=0x1234)).stream == 0x1234
    assert DeviceArrayFrame(Fake((5, 7, 3), version=3, stream=1)).stream == 1                 # legacy default: hipStreamLegacy
    assert DeviceArrayFrame(Fake((5, 7, 3), version=3, stream=2)).stream == 2                 # per thread: hipStreamPerThread
    assert DeviceArrayFrame(Fake((5, 7, 3), version=3, stream=0x1234), stream=0x99).stream == 0x99    # the argument wins
    assert DeviceArrayFrame(Fake((5, 7, 3)), stream=S()).stream == 0x5555
    assert DeviceArrayFrame(Fake((5, 7, 3), version=3, stream=0x1234)).descriptor().stream == 0x1234
    f = DeviceArrayFrame.nv12(Fake((4, 6), version=3, stream=0x77), Fake((2, 6), ptr=PTR + 4096, version=3, stream=0x88))
    assert f.stream == 0x77


def test_nv12_shape_rules():
    f = DeviceArrayFrame.nv12(Fake((4, 6), strides=(9, 1)), Fake((2, 6), ptr=PTR + 4096, strides=(11, 1)), 'bt709', ready=True)
    assert (f.layout, f.size, f.shape, f.matrix_id, f.planes) == ('nv12', (6, 4), (4, 6, 3), 1, [(PTR, 9), (PTR + 4096, 11)])
    d = f.descriptor()
    assert (d.layout, d.matrix, d.format, d.plane[2], d.pitch[1], d.flags) == (D.FM_DEV_NV12, 1, 0, None, 11, 1)
    assert 'nv12 6x4 uint8 bt709' in f.describe()
    assert DeviceArrayFrame.nv12(Fake((2, 6), strides=(9, 1)), Fake((1, 6), strides=(0, 1))).planes == [(PTR, 9), (PTR, 6)]    # (a single row's stride means nothing)
    for y, uv in (((5, 6), (2, 6)), ((4, 5), (2, 5)), ((4, 6), (2, 4)), ((4, 6), (4, 6)), ((4, 6), (2, 3, 2)), ((0, 6), (0, 6))):
        with pytest.raises(ValueError):
            DeviceArrayFrame.nv12(Fake(y), Fake(uv))
    with pytest.raises(ValueError):
        DeviceArrayFrame.nv12(Fake((4, 6)), Fake((2, 6)), matrix='bt601-full')
    with pytest.raises(ValueError):
        DeviceArrayFrame.nv12(Fake((4, 6), strides=(5, 1)), Fake((2, 6)))
    with pytest.raises(ValueError):
        DeviceArrayFrame.nv12(Fake((4, 6), strides=(12, 2)), Fake((2, 6)))
    with pytest.raises(ValueError):
        DeviceArrayFrame.nv12(Fake((4, 6)), Fake((2, 6), strides=(-6, 1)))
    with pytest.raises(TypeError):
        DeviceArrayFrame.nv12(Fake((4, 6), '<f2'), Fake((2, 6)))


def test_source_frame_takes_a_device_frame():
    f = DeviceArrayFrame(Fake((5, 7, 4)), 'bgrx')
    s = SourceFrame(f)
    assert s.size == (7, 5) and s.shape == (5, 7, 3) and s.frame is f and s.lens is None
    with pytest.raises(TypeError):
        s.describe()


# ---- the C side
def test_struct_matches_header():
    """fm_frame_device as a C compiler lays it out (LP64), and its fields as the header names them, in order."""
    F = D.FrameDevice
    names = ['plane', 'pitch', 'width', 'height', 'layout', 'dtype', 'format', 'matrix', 'scale', 'stream', 'flags']
    assert [n for n, _ in F._fields_] == names
    assert [getattr(F, n).offset for n in names] == [0, 24, 48, 52, 56, 60, 64, 68, 72, 80, 88]
    assert C.sizeof(F) == 96
    text = (ROOT / 'include' / 'fastmot_hip.h').read_text()
    body = re.search(r'struct fm_frame_device \{(.*?)\n\};', text, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    decl = [re.sub(r'\[\d+\]', '', part).split()[-1].lstrip('*') for stmt in body.split(';') for part in stmt.split(',') if part.strip()]
    assert decl == names
    consts = dict(re.findall(r'#define (FM_DEV_\w+) (\d+)', text))
    for name in ('FM_DEV_HWC', 'FM_DEV_CHW', 'FM_DEV_NV12', 'FM_DEV_U8', 'FM_DEV_F16', 'FM_DEV_F32', 'FM_DEV_ORDER_RGB',
                 'FM_DEV_ORDER_BGR', 'FM_DEV_READY'):
        assert int(consts[name]) == getattr(D, name), name


def check(frame=None, **kw):
    d = D.FrameDevice.from_buffer_copy((frame or DeviceArrayFrame(Fake((6, 8, 3)))).descriptor())
    for k, v in kw.items():
        if k in ('plane', 'pitch'):
            for i, x in v.items():
                getattr(d, k)[i] = x
        else:
            setattr(d, k, v)
    return _lib.load().fm_frame_device_check(C.byref(d))


def test_device_check_rules():
    lib = _lib.load()
    hwc4 = DeviceArrayFrame(Fake((6, 8, 4)), 'xrgb')
    f16 = DeviceArrayFrame(Fake((3, 6, 8), '<f2'))
    f32 = DeviceArrayFrame(Fake((3, 6, 8), '<f4'), 'bgr', float_range=(0, 255))
    u8 = DeviceArrayFrame(Fake((3, 6, 8)))
    nv12 = DeviceArrayFrame.nv12(Fake((6, 8)), Fake((3, 8), ptr=PTR + 4096))
    for good in (None, hwc4, f16, f32, u8, nv12):
        assert check(good) == 0
    assert check(width=16384, pitch={0: 3 * 16384}) == 0 and check(height=16384) == 0 and check(height=1, width=1) == 0
    assert check(flags=D.FM_DEV_READY) == 0 and check(f32, scale=255.0) == 0 and check(pitch={0: 1 << 40}) == 0
    assert check(u8, scale=0.0) == 0 and check(matrix=99) == 0                # not read for these layouts
    bad = [dict(width=0), dict(height=0), dict(width=-8), dict(width=16385, pitch={0: 1 << 20}), dict(height=16385),    # dims
           dict(layout=-1), dict(layout=3), dict(dtype=-1), dict(dtype=3),                                          # layout, dtype
           dict(dtype=D.FM_DEV_F32, scale=255.0, pitch={0: 96}), dict(dtype=D.FM_DEV_F16, scale=1.0, pitch={0: 48}),    # float HWC
           dict(format=-1), dict(format=6), dict(format=8),                                                         # HWC: RGB family only
           dict(frame=u8, format=2), dict(frame=u8, format=-1), dict(frame=f32, format=3),                          # CHW: two orders
           dict(pitch={0: 23}), dict(pitch={0: 0}), dict(pitch={0: -24}), dict(pitch={0: (1 << 40) + 1}),               # pitches
           dict(frame=hwc4, pitch={0: 31}), dict(frame=f32, pitch={1: 28}), dict(frame=f16, pitch={2: 14}), dict(frame=u8, pitch={0: 7}),
           dict(plane={0: None}), dict(plane={1: PTR}), dict(plane={2: PTR}),                                       # planes
           dict(frame=u8, plane={1: None}), dict(frame=u8, plane={2: None}), dict(frame=f32, plane={0: None}),
           dict(frame=f32, plane={0: PTR + 2}), dict(frame=f32, plane={2: PTR + 1}), dict(frame=f16, plane={1: PTR + 1}),   # alignment
           dict(frame=f32, pitch={0: 34}), dict(frame=f32, pitch={1: 33}), dict(frame=f16, pitch={2: 17}),
           dict(frame=f32, scale=0.0), dict(frame=f32, scale=2.0), dict(frame=f16, scale=254.0), dict(frame=f16, scale=float('nan')),
           dict(frame=f32, scale=-255.0),
           dict(flags=2), dict(flags=3), dict(flags=-1),
           dict(frame=nv12, width=7, pitch={0: 8}), dict(frame=nv12, height=5), dict(frame=nv12, width=2, height=1),    # NV12
           dict(frame=nv12, matrix=2), dict(frame=nv12, matrix=16), dict(frame=nv12, matrix=-1), dict(frame=nv12, format=1),
           dict(frame=nv12, dtype=D.FM_DEV_F16), dict(frame=nv12, plane={1: None}), dict(frame=nv12, plane={2: PTR}),
           dict(frame=nv12, pitch={0: 7}), dict(frame=nv12, pitch={1: 7})]
    for kw in bad:
        assert check(**kw) == FM_ERR_ARG, kw
        assert b'bad argument' in lib.fm_last_error(), kw
    assert lib.fm_frame_device_check(None) == FM_ERR_ARG and b'bad argument' in lib.fm_last_error()


def test_entry_points_refuse_null_arguments():
    """No context, no description: refused before any HIP call (this runs without a GPU)."""
    lib = _lib.load()
    d = C.byref(DeviceArrayFrame(Fake((6, 8, 3))).descriptor())
    t = C.c_uint64(77)
    calls = [lambda c, f: lib.fm_frame_upload_device(c, f),
             lambda c, f: lib.fm_frame_upload_ahead_device(c, C.c_int(1), f, C.byref(t)),
             lambda c, f: lib.fm_frame_ring_store_device(c, C.c_int(0), f)]
    for call in calls:
        for c, f in ((None, d), (None, None)):
            assert call(c, f) == FM_ERR_ARG
            assert b'bad argument' in lib.fm_last_error()
    assert t.value == 77
    for wait in (0, 1):
        assert lib.fm_frame_device_done(None, C.c_uint64(1), C.c_int(wait)) == FM_ERR_ARG
        assert b'bad argument' in lib.fm_last_error()
