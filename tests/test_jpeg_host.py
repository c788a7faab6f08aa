"""CPU: the host half of the JPEG ingest path.  fastmot_amd/utils/jpeg.py (the numpy statement of the decode) against
Pillow, bit for bit; fm_jpeg_info / fm_jpeg_entropy_decode (csrc/jpeg_host.hip) against the numpy parser, entry for
entry; unsupported files; truncated and corrupted files with guard bytes around the output buffers.  Nothing here
touches a GPU: the two functions need no context."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_cases as jc
from fastmot_amd import JPEGFrame, _lib
from fastmot_amd.utils import jpeg as J

FM_ERR_ARG, FM_ERR_UNSUPPORTED = -2, -4
GUARD = 64                  # int16 elements on either side of an output buffer
PATTERN = 0x5A5A


def native_decode(lib, data, guard=False):
    """(rc of fm_jpeg_info, rc of fm_jpeg_entropy_decode or None, info, coef, qt); with `guard`, both outputs lie between
    guard elements, which are checked."""
    info = J.JpegInfo()
    rc = lib.fm_jpeg_info(data, C.c_size_t(len(data)), C.byref(info))
    if rc:
        return rc, None, info, None, None
    n = info.coef_count
    assert 0 < n <= 3 * 65535 * 72            # (what a header can describe at most in these tests)
    cbuf = np.full(n + 2 * GUARD, PATTERN, np.int16)
    qbuf = np.full(J.QT_ENTRIES + 2 * GUARD, PATTERN, np.uint16)
    coef, qt = cbuf[GUARD:GUARD + n], qbuf[GUARD:GUARD + J.QT_ENTRIES]
    rc2 = lib.fm_jpeg_entropy_decode(data, C.c_size_t(len(data)), C.byref(info), _lib._ptr(coef), _lib._ptr(qt))
    if guard:
        for buf, m in ((cbuf, n), (qbuf, J.QT_ENTRIES)):
            assert (buf[:GUARD] == PATTERN).all() and (buf[GUARD + m:] == PATTERN).all(), 'guard bytes overwritten'
    return rc, rc2, info, coef, qt


@pytest.mark.parametrize('subsampling', jc.SUBSAMPLINGS)
@pytest.mark.parametrize('size', jc.SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_numpy_decode_equals_pillow_and_native_decoder_equals_numpy(size, subsampling):
    lib = _lib.load()
    for label, data in jc.cases(size, subsampling):
        hd = J.parse(data)
        coef, qt = J.entropy_decode(data, hd)
        # 1. the documented arithmetic is Pillow's
        assert np.array_equal(J.coefficients_to_bgr(coef, qt, hd), jc.pillow_bgr(data)), label
        # 2. the C parser and Huffman decoder give the numpy parser's fields, coefficients and tables
        rc, rc2, info, ncoef, nqt = native_decode(lib, data, guard=True)
        assert (rc, rc2) == (0, 0), (label, lib.fm_last_error())
        for name in ('width', 'height', 'ncomp', 'mcu_w', 'mcu_h', 'mcus_x', 'mcus_y', 'restart_interval', 'coef_count'):
            assert getattr(info, name) == getattr(hd, name), (label, name)
        for name in ('hsamp', 'vsamp', 'blocks_w', 'blocks_h', 'coef_offset'):
            assert list(getattr(info, name)) == list(getattr(hd, name)), (label, name)
        assert (info.width, info.height) == size and info.unsupported == 0
        assert bool(info.restart_interval) == bool(label[4])
        assert np.array_equal(ncoef, coef), label
        assert np.array_equal(nqt, qt), label


def test_decode_bgr_and_frame_object():
    data = jc.encode(jc.content('textured', 70, 46), '420', 90)
    want = jc.pillow_bgr(data)
    assert np.array_equal(J.decode_bgr(data), want)
    f = JPEGFrame(data)
    assert f.size == (70, 46) and f.shape == (46, 70, 3)
    assert f.coef.dtype == np.int16 and f.coef.size == f.info.coef_count and f.qt.dtype == np.uint16 and f.qt.size == 192
    assert np.array_equal(f.to_bgr(), want)
    # a buffer handed in: decoded in place; too small a buffer is refused
    buf = np.zeros(J.max_coefficients(70, 46) + J.QT_ENTRIES, np.int16)
    g = JPEGFrame(data, buffer=buf)
    assert np.shares_memory(g.coef, buf) and np.array_equal(g.coef, f.coef) and np.array_equal(g.qt, f.qt)
    with pytest.raises(ValueError):
        JPEGFrame(data, buffer=np.zeros(100, np.int16))
    with pytest.raises(ValueError):
        JPEGFrame(b'not a jpeg at all')
    # a wanted size: a file of another size is refused from its header alone, before anything is allocated -- also one
    # whose (damaged) header claims 65535 x 65535, for which 25 GB of coefficients would be needed
    assert JPEGFrame(data, size=(70, 46)).size == (70, 46)
    with pytest.raises(J.WrongSizeJPEG):
        JPEGFrame(data, size=(46, 70))
    at = data.index(b'\xff\xc0') + 5
    huge = data[:at] + b'\xff\xff\xff\xff' + data[at + 4:]
    info = J.JpegInfo()
    assert _lib.load().fm_jpeg_info(huge, C.c_size_t(len(huge)), C.byref(info)) == 0 and info.width == info.height == 65535
    with pytest.raises(J.WrongSizeJPEG):
        JPEGFrame(huge, size=(70, 46))


def test_unsupported_files():
    lib = _lib.load()
    rgb = jc.content('textured', 40, 24)

    def save(im, **kw):
        buf = io.BytesIO()
        im.save(buf, 'JPEG', **kw)
        return buf.getvalue()

    # custom Huffman tables are ordinary baseline JPEG
    for sub in jc.SUBSAMPLINGS:
        data = jc.encode(rgb, sub, 85, optimize=True)
        assert np.array_equal(JPEGFrame(data).to_bgr(), jc.pillow_bgr(data)), sub
        assert np.array_equal(J.decode_bgr(data), jc.pillow_bgr(data)), sub
    unsupported = {'progressive': (save(Image.fromarray(rgb), progressive=True), 1),
                   'cmyk': (save(Image.fromarray(rgb).convert('CMYK')), 5)}
    for name, (data, code) in unsupported.items():
        info = J.JpegInfo()
        assert lib.fm_jpeg_info(data, C.c_size_t(len(data)), C.byref(info)) == FM_ERR_UNSUPPORTED, name
        assert info.unsupported == code, name
        with pytest.raises(ValueError, match='progressive' if name == 'progressive' else 'CMYK'):
            JPEGFrame(data)
        with pytest.raises(J.UnsupportedJPEG):
            J.parse(data)
    # an info that is not the file's is refused before anything is written
    data = jc.encode(rgb, '420', 85)
    rc, rc2, info, coef, qt = native_decode(lib, data)
    assert (rc, rc2) == (0, 0)
    info.coef_count -= 64
    assert lib.fm_jpeg_entropy_decode(data, C.c_size_t(len(data)), C.byref(info), _lib._ptr(coef), _lib._ptr(qt)) == FM_ERR_ARG


ROBUSTNESS_FILES = {'420_restarts': lambda: jc.encode(jc.content('noise', 24, 20, 1), '420', 75, 2),
                    '444': lambda: jc.encode(jc.content('noise', 17, 9, 2), '444', 75),
                    'grey': lambda: jc.encode(jc.content('noise', 16, 16, 3), 'grey', 75)}


@pytest.mark.parametrize('which', sorted(ROBUSTNESS_FILES))
def test_truncated_files(which):
    """Every prefix of the file: an error, or -- when only trailing padding / the EOI marker is cut -- the full decode."""
    lib = _lib.load()
    data = ROBUSTNESS_FILES[which]()
    rc, rc2, _, full, full_qt = native_decode(lib, data, guard=True)
    assert (rc, rc2) == (0, 0)
    complete = 0
    for n in range(len(data)):
        rc, rc2, _, coef, qt = native_decode(lib, data[:n], guard=True)
        if rc == 0 and rc2 == 0:
            assert np.array_equal(coef, full) and np.array_equal(qt, full_qt), n
            complete += 1
        else:
            assert (rc if rc else rc2) in (FM_ERR_ARG, FM_ERR_UNSUPPORTED), n
            assert lib.fm_last_error()
            with pytest.raises(ValueError):
                JPEGFrame(data[:n])
    assert complete <= 3          # the two bytes of EOI, at most one byte of padding bits


@pytest.mark.parametrize('which', sorted(ROBUSTNESS_FILES))
def test_corrupted_files(which):
    """2000 seeded single-byte corruptions: some status comes back, nothing is written outside the buffers."""
    lib = _lib.load()
    data = ROBUSTNESS_FILES[which]()
    rng = np.random.default_rng(len(data))
    statuses = set()
    for _ in range(2000):
        bad = bytearray(data)
        bad[int(rng.integers(len(data)))] = int(rng.integers(256))
        rc, rc2, _, _, _ = native_decode(lib, bytes(bad), guard=True)
        status = rc if rc else rc2
        assert status in (0, FM_ERR_ARG, FM_ERR_UNSUPPORTED)
        statuses.add(status)
        try:                        # the numpy decoder refuses what it cannot decode, and never anything else
            J.decode_bgr(bytes(bad))
        except ValueError:
            pass
    assert 0 in statuses and FM_ERR_ARG in statuses
