"""CPU: the numpy statement of the NV12 -> BGR conversion (fastmot_amd/utils/nv12.py), the NV12Frame handle's
validation, and the C ABI's three NV12 entry points.  The GPU kernel is compared with `nv12_to_bgr` bit for bit in
test_nv12_gpu.py, so the known answers here pin both."""
import zlib

import numpy as np
import pytest

from fastmot_amd import NV12Frame
from fastmot_amd.utils.nv12 import bgr_to_nv12, nv12_to_bgr, yuv_to_bgr

# (Y, U, V) -> BGR under bt601 | bt709
KNOWN = [((16, 128, 128), [0, 0, 0], [0, 0, 0]),
         ((235, 128, 128), [255, 255, 255], [255, 255, 255]),
         ((81, 90, 240), [0, 0, 254], [0, 24, 255]),
         ((145, 54, 34), [1, 255, 0], [0, 216, 0]),
         ((41, 240, 110), [255, 0, 0], [255, 15, 0]),
         ((0, 0, 0), [0, 154, 0], [0, 96, 0]),
         ((255, 255, 255), [255, 125, 255], [255, 184, 255]),
         ((128, 64, 200), [1, 97, 245], [0, 106, 255]),
         ((200, 255, 0), [255, 255, 10], [255, 255, 0])]


@pytest.mark.parametrize('yuv,bt601,bt709', KNOWN)
def test_known_answers(yuv, bt601, bt709):
    y = np.full((2, 2), yuv[0], np.uint8)
    uv = np.array([[yuv[1], yuv[2]]], np.uint8)
    for matrix, want in (('bt601', bt601), ('bt709', bt709)):
        got = nv12_to_bgr(y, uv, matrix)
        assert got.shape == (2, 2, 3) and got.dtype == np.uint8
        assert (got == np.array(want, np.uint8)).all(), (matrix, got[0, 0].tolist(), want)
    assert nv12_to_bgr(y, uv).tolist() == nv12_to_bgr(y, uv, 'bt601').tolist()      # the default matrix


def test_all_triples_crc():
    r = np.arange(256, dtype=np.uint8)
    y, u, v = (a.ravel() for a in np.meshgrid(r, r, r, indexing='ij'))
    assert zlib.crc32(yuv_to_bgr(y, u, v, 'bt601').tobytes()) == 1969820439


def test_chroma_is_shared_by_the_2x2_block_without_interpolation():
    rng = np.random.default_rng(0)
    y = rng.integers(0, 256, (6, 10), dtype=np.uint8)
    uv = rng.integers(0, 256, (3, 10), dtype=np.uint8)
    got = nv12_to_bgr(y, uv, 'bt709')
    for r in range(6):
        for c in range(10):
            px = yuv_to_bgr(y[r, c], uv[r // 2, c // 2 * 2], uv[r // 2, c // 2 * 2 + 1], 'bt709')
            assert (got[r, c] == px).all()


def test_nv12frame_validation():
    y = np.zeros((4, 6), np.uint8)
    uv = np.zeros((2, 6), np.uint8)
    f = NV12Frame(y, uv)
    assert (f.size, f.pitch, f.matrix, f.matrix_id, f.shape) == ((6, 4), 6, 'bt601', 0, (4, 6, 3))
    assert NV12Frame(y, uv, 'bt709').matrix_id == 1
    with pytest.raises(ValueError):
        NV12Frame(y, uv, 'bt2020')
    with pytest.raises(ValueError):                      # odd width / odd height
        NV12Frame(np.zeros((4, 5), np.uint8), np.zeros((2, 5), np.uint8))
    with pytest.raises(ValueError):
        NV12Frame(np.zeros((3, 6), np.uint8), np.zeros((1, 6), np.uint8))
    with pytest.raises(ValueError):                      # uv shape
        NV12Frame(y, np.zeros((2, 3), np.uint8))
    with pytest.raises(ValueError):
        NV12Frame(y, np.zeros((4, 6), np.uint8))
    with pytest.raises(ValueError):
        NV12Frame(y, np.zeros((2, 3, 2), np.uint8))
    with pytest.raises(TypeError):                       # dtype
        NV12Frame(y.astype(np.int16), uv)
    with pytest.raises(TypeError):
        NV12Frame(y, uv.astype(np.float32))
    with pytest.raises(TypeError):
        NV12Frame(y.tolist(), uv)
    wide = np.zeros((4, 12), np.uint8)
    with pytest.raises(ValueError):                      # element stride 2; row stride < width
        NV12Frame(wide[:, ::2], uv)
    with pytest.raises(ValueError):
        NV12Frame(np.lib.stride_tricks.as_strided(wide, (4, 6), (4, 1)), np.lib.stride_tricks.as_strided(wide, (2, 6), (4, 1)))
    with pytest.raises(ValueError):                      # unequal strides
        NV12Frame(wide[:, :6], uv)
    big = np.zeros((6, 16), np.uint8)                    # both planes views of one pitched surface
    f = NV12Frame(big[:4, :6], big[4:, :6])
    assert f.pitch == 16 and f.size == (6, 4)


def test_from_buffer():
    rng = np.random.default_rng(1)
    w, h, pitch = 6, 4, 16
    buf = rng.integers(0, 256, pitch * 8 + pitch * 2, dtype=np.uint8)      # Y plane's height aligned to 8 rows
    f = NV12Frame.from_buffer(buf, (w, h), pitch=pitch, uv_offset=pitch * 8, matrix='bt709')
    assert (f.size, f.pitch, f.matrix) == ((w, h), pitch, 'bt709')
    rows = buf.reshape(10, pitch)
    assert (f.y == rows[:4, :w]).all() and (f.uv == rows[8:, :w]).all()
    assert np.shares_memory(f.y, buf) and np.shares_memory(f.uv, buf)
    g = NV12Frame.from_buffer(bytes(range(36)), (6, 4))                    # defaults: pitch = W, uv behind Y
    assert g.pitch == 6 and g.y[3, 5] == 23 and g.uv[0, 0] == 24 and g.uv[1, 5] == 35
    with pytest.raises(ValueError):
        NV12Frame.from_buffer(buf[:30], (6, 4))
    with pytest.raises(ValueError):
        NV12Frame.from_buffer(buf, (6, 4), pitch=4)
    with pytest.raises(ValueError):
        NV12Frame.from_buffer(buf, (6, 4), pitch=16, uv_offset=32)
    with pytest.raises(ValueError):
        NV12Frame.from_buffer(buf, (5, 4))


def test_round_trip_on_a_smooth_image():
    """bgr_to_nv12 -> nv12_to_bgr.  Measured on this image when the test was written: the largest difference of a
    channel is 5 grey levels (B 5, G 2, R 3), the mean 1.0.  The two 8-bit quantisations (Y to 219 levels, chroma rounded
    twice) and the chroma of a 2 x 2 block standing for four pixels whose B and R differ by up to 3 levels along the
    gradients account for it; the bound below is that measurement plus one level."""
    h, w = 64, 96
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([xx * 255 // (w - 1), yy * 255 // (h - 1), (xx + yy) * 255 // (w + h - 2)], -1).astype(np.uint8)
    y, uv = bgr_to_nv12(img)
    assert y.shape == (h, w) and uv.shape == (h // 2, w) and y.dtype == uv.dtype == np.uint8
    assert y.min() >= 16 and y.max() <= 235 and uv.min() >= 16 and uv.max() <= 240      # limited range
    diff = np.abs(nv12_to_bgr(y, uv).astype(int) - img)
    print('round trip: max', diff.max(axis=(0, 1)), 'mean', diff.mean())
    assert diff.max() <= 6
    with pytest.raises(ValueError):
        bgr_to_nv12(img[:63])


def test_bgr_to_nv12_rounds_the_block_mean_half_up():
    img = np.zeros((2, 2, 3), np.uint8)
    img[0, 0] = (255, 0, 0)                     # pure blue: U = 240, V = 110; the other three: U = V = 128
    y, uv = bgr_to_nv12(img)
    assert y.tolist() == [[41, 16], [16, 16]]
    assert uv.tolist() == [[(240 + 3 * 128 + 2) >> 2, (110 + 3 * 128 + 2) >> 2]] == [[156, 124]]


def test_library_exports_the_nv12_entry_points():
    from fastmot_amd import _lib
    from test_abi import declared_symbols
    lib = _lib.load()
    syms = declared_symbols()
    for name in ('fm_frame_upload_nv12', 'fm_frame_upload_ahead_nv12', 'fm_frame_ring_store_nv12'):
        assert name in syms and hasattr(lib, name), name
