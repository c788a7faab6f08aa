"""CPU: the numpy statement of the Bayer demosaicing (fastmot_amd/utils/bayer.py) against an independent float64
statement -- the 5 x 5 kernels of Malvar, He and Cutler (and the bilinear averaging kernels) correlated over the
index-reflected sample plane --, the sample preparation against its float formula over every sample value, BayerFrame's
validation, VideoIO(pixel_format='rggb' ...) over '.npy' stacks, and the library's entry points without a context."""
import ctypes as C

import numpy as np
import pytest

from fastmot_amd import BayerFrame, SourceFrame, VideoIO, _lib
from fastmot_amd.utils import bayer as B
from fastmot_amd.utils.bayer import DEPTHS, METHODS, PATTERNS, bayer_to_bgr, mosaic

FM_ERR_ARG = -2
SIZES = [(2, 2), (3, 5), (4, 3), (33, 7), (64, 48)]
# where R sits in the 2 x 2 tile: (row, column)
R_AT = {'rggb': (0, 0), 'grbg': (0, 1), 'gbrg': (1, 0), 'bggr': (1, 1)}

# ---- the float64 statement.  The paper's kernels, in eighths.
G_AT_RB = [[0, 0, -1, 0, 0],
           [0, 0, 2, 0, 0],
           [-1, 2, 4, 2, -1],
           [0, 0, 2, 0, 0],
           [0, 0, -1, 0, 0]]
RB_AT_G_ROW = [[0, 0, .5, 0, 0],              # R (B) at a green position whose row holds R (B): its neighbours left and right
               [0, -1, 0, -1, 0],
               [-1, 4, 5, 4, -1],
               [0, -1, 0, -1, 0],
               [0, 0, .5, 0, 0]]
RB_AT_BR = [[0, 0, -1.5, 0, 0],
            [0, 2, 0, 2, 0],
            [-1.5, 0, 6, 0, -1.5],
            [0, 2, 0, 2, 0],
            [0, 0, -1.5, 0, 0]]
MHC_KERNELS = [np.array(k, np.float64) / 8 for k in (G_AT_RB, RB_AT_G_ROW, np.transpose(RB_AT_G_ROW), RB_AT_BR)]
BILINEAR_KERNELS = [np.array(k, np.float64) for k in (
    [[0, .25, 0], [.25, 0, .25], [0, .25, 0]], [[0, 0, 0], [.5, 0, .5], [0, 0, 0]], [[0, .5, 0], [0, 0, 0], [0, .5, 0]],
    [[.25, 0, .25], [0, 0, 0], [.25, 0, .25]])]


def reflected(i, n):
    """Reflect-101, written out: walk back from the edge that was passed."""
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * (n - 1) - i
    return i


def correlate(p, k):
    h, w = p.shape
    r = k.shape[0] // 2
    out = np.zeros((h, w), np.float64)
    ys = [[reflected(y + d, h) for y in range(h)] for d in range(-r, r + 1)]
    xs = [[reflected(x + d, w) for x in range(w)] for d in range(-r, r + 1)]
    for a in range(2 * r + 1):
        for b in range(2 * r + 1):
            if k[a, b]:
                out += k[a, b] * p[np.ix_(ys[a], xs[b])]
    return out


def float_demosaic(p, pattern, method, seen=None):
    """p: prepared samples (H, W) -> BGR uint8 by the float64 statement.  seen: a set that collects 'low' / 'high' when a
    value that is used left 0..255 before the clip."""
    h, w = p.shape
    p = p.astype(np.float64)
    raw = [np.floor(correlate(p, k) + 0.5) for k in (MHC_KERNELS if method == 'mhc' else BILINEAR_KERNELS)]
    g_at_rb, at_g_row, at_g_col, at_opposite = (np.clip(r, 0, 255) for r in raw)
    ry, rx = R_AT[pattern]
    out = np.zeros((h, w, 3), np.uint8)
    for y in range(h):
        for x in range(w):
            r_row, r_col = y % 2 == ry, x % 2 == rx
            if r_row and r_col:
                px = (at_opposite[y, x], g_at_rb[y, x], p[y, x])
            elif not r_row and not r_col:
                px = (p[y, x], g_at_rb[y, x], at_opposite[y, x])
            elif r_row:                       # green, R left and right, B above and below
                px = (at_g_col[y, x], p[y, x], at_g_row[y, x])
            else:
                px = (at_g_row[y, x], p[y, x], at_g_col[y, x])
            out[y, x] = px
            if seen is not None:
                used = (raw[0][y, x], raw[3][y, x]) if r_row == r_col else (raw[1][y, x], raw[2][y, x])
                if min(used) < 0:
                    seen.add('low')
                if max(used) > 255:
                    seen.add('high')
    return out


def contents(rng, w, h, pattern):
    """Random samples with a first row of 0 and a last row of 255, and the 0 / 255 checkerboards at the mosaic's phase:
    one colour's positions 255 and the rest 0, and the inverse -- so that both clamps of 'mhc' are reached."""
    a = rng.integers(0, 256, (h, w), dtype=np.uint8)
    a[0], a[-1] = 0, 255
    out = [a]
    for mask in B.colour_planes((w, h), pattern):
        out += [np.where(mask, 255, 0).astype(np.uint8), np.where(mask, 0, 255).astype(np.uint8)]
    return out


@pytest.mark.parametrize('method', sorted(METHODS))
@pytest.mark.parametrize('pattern', sorted(PATTERNS))
def test_bayer_to_bgr_equals_the_float_statement(pattern, method):
    rng = np.random.default_rng(21)
    seen = set()
    for w, h in SIZES:
        for data in contents(rng, w, h, pattern):
            got = bayer_to_bgr(data, (w, h), pattern, method=method)
            assert got.dtype == np.uint8 and got.shape == (h, w, 3)
            assert np.array_equal(got, float_demosaic(data, pattern, method, seen)), (w, h)
            assert np.array_equal(bayer_to_bgr(data, None, pattern, 8, method), got)
    assert seen == ({'low', 'high'} if method == 'mhc' else set())      # both clamps of 'mhc' are reached; bilinear has none


def test_pattern_ids_say_where_red_sits():
    assert PATTERNS == {'rggb': 0, 'grbg': 1, 'gbrg': 2, 'bggr': 3} and METHODS == {'bilinear': 0, 'mhc': 1}
    assert tuple(DEPTHS) == (8, 10, 12, 14, 16)
    for name, pid in PATTERNS.items():
        assert R_AT[name] == (pid >> 1, pid & 1)
        is_r, is_g, is_b = B.colour_planes((5, 3), name)
        ry, rx = R_AT[name]
        for y in range(3):
            for x in range(5):
                want = 'r' if (y % 2, x % 2) == (ry, rx) else 'b' if (y % 2, x % 2) == (1 - ry, 1 - rx) else 'g'
                assert (is_r[y, x], is_g[y, x], is_b[y, x]) == (want == 'r', want == 'g', want == 'b')


@pytest.mark.parametrize('depth', DEPTHS)
def test_sample_preparation_over_every_sample_value(depth):
    s = np.arange(1 << depth, dtype=np.uint8 if depth == 8 else np.uint16)
    data = np.stack([s, s])                                   # (2, 2^depth): every value at an even and an odd row
    size = (data.shape[1], 2)
    planes = B.colour_planes(size, 'rggb')
    for black in (0, (1 << depth) // 16 + 1):
        for gain in (1, 256, 300, 4096):
            for which in range(3):                            # the gain under test on one colour, 256 on the others
                g = [256, 256, 256]
                g[which] = gain
                got = B.prepare(data, size, 'rggb', depth, tuple(g), black)
                v = np.maximum(data.astype(np.float64) - black, 0)
                for i, mask in enumerate(planes):
                    want = np.minimum(255, np.floor(v * g[i] / 256 / 2. ** (depth - 8) + 0.5))
                    assert np.array_equal(got[mask], want[mask].astype(np.int32)), (depth, black, gain, which, i)
    if depth == 8:
        assert np.array_equal(B.prepare(data, size, 'bggr'), data)
    # through bayer_to_bgr: a position's own colour is its prepared sample, with the gain of that colour
    f = bayer_to_bgr(data, size, 'rggb', depth, 'mhc', wb=(300 / 256, 1, 16), black=3)
    p = B.prepare(data, size, 'rggb', depth, (300, 256, 4096), 3)
    for ch, mask in zip((2, 1, 0), planes):
        assert np.array_equal(f[..., ch][mask], p[mask])
    assert B.gains((1, 0.5, 16)) == (256, 128, 4096) and B.gains((1 / 256, 1.17, 1)) == (1, 300, 256)


@pytest.mark.parametrize('size', [(7, 5), (33, 7), (5, 2)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_a_constant_colour_is_reproduced(size):
    w, h = size
    for colour in ((10, 200, 90), (255, 0, 255), (0, 0, 0), (255, 255, 255), (1, 254, 3)):
        bgr = np.broadcast_to(np.array(colour, np.uint8), (h, w, 3))
        for pattern in PATTERNS:
            for method in METHODS:
                assert np.array_equal(bayer_to_bgr(mosaic(bgr, pattern), None, pattern, method=method), bgr), (colour, pattern, method)


def test_mosaic_keeps_every_positions_own_colour():
    rng = np.random.default_rng(22)
    bgr = rng.integers(0, 256, (9, 14, 3), dtype=np.uint8)
    for pattern in PATTERNS:
        m = mosaic(bgr, pattern)
        assert m.shape == (9, 14) and m.dtype == np.uint8
        ry, rx = R_AT[pattern]
        assert m[ry, rx] == bgr[ry, rx, 2] and m[1 - ry, 1 - rx] == bgr[1 - ry, 1 - rx, 0]
        assert m[ry, 1 - rx] == bgr[ry, 1 - rx, 1] and m[1 - ry, rx] == bgr[1 - ry, rx, 1]
        for method in METHODS:
            out = bayer_to_bgr(m, None, pattern, method=method)
            for ch, mask in zip((2, 1, 0), B.colour_planes((14, 9), pattern)):
                assert np.array_equal(out[..., ch][mask], bgr[..., ch][mask])
    wide = mosaic(bgr.astype(np.uint16) << 4, 'grbg')
    assert wide.dtype == np.uint16 and np.array_equal(wide >> 4, mosaic(bgr, 'grbg'))


def psnr(a, b):
    return 10 * np.log10(255. ** 2 / np.mean((a.astype(np.float64) - b) ** 2))


def test_mhc_beats_bilinear_on_a_correlated_picture():
    """128 x 96, one luminance under three slowly varying channel factors.  Measured: 34.8 dB against 31.1 dB."""
    y, x = np.mgrid[0:96, 0:128].astype(np.float64)
    lum = 0.5 + 0.25 * np.sin((x * x + y * y) / 600) + 0.2 * (((x // 8) + (y // 8)).astype(np.int64) & 1)
    tint = np.stack([0.6 * (0.8 + 0.2 * np.sin(x / 40)), 0.9 * (0.8 + 0.2 * np.cos(y / 50)), 0.75 * (0.8 + 0.2 * np.sin((x + y) / 60))], axis=-1)
    bgr = np.rint(255 * lum[..., None] * tint).astype(np.uint8)
    for pattern in PATTERNS:
        m = mosaic(bgr, pattern)
        got = {method: psnr(bayer_to_bgr(m, None, pattern, method=method), bgr) for method in METHODS}
        print(pattern, got)
        assert got['mhc'] >= got['bilinear'] + 2, (pattern, got)


def test_bayer_frame_validation():
    rng = np.random.default_rng(23)
    w, h = 6, 4
    m8 = rng.integers(0, 256, (h, w), dtype=np.uint8)
    m16 = rng.integers(0, 4096, (h, w)).astype(np.uint16)
    f = BayerFrame(m8, 'grbg')
    assert f.size == (w, h) and f.shape == (h, w, 3) and f.pitch == w and f.depth == 8 and f.method == 'mhc' and f.pattern == 'grbg'
    assert np.array_equal(f.to_bgr(), bayer_to_bgr(m8, (w, h), 'grbg'))
    f = BayerFrame(m16, 'bggr', depth=12, method='bilinear', wb=(2, 1, 1.5), black=64)
    assert f.pitch == 2 * w and np.array_equal(f.to_bgr(), bayer_to_bgr(m16, None, 'bggr', 12, 'bilinear', (2, 1, 1.5), 64))
    # dtype against depth
    for data, depth in ((m16, 8), (m8, 10), (m8, 16), (m8.astype(np.int8), 8), (m16.astype(np.int16), 12), (m16.astype(np.float32), 12),
                        (m16.astype('>u2'), 12)):
        with pytest.raises(TypeError):
            BayerFrame(data, 'rggb', depth=depth)
    with pytest.raises(TypeError):
        BayerFrame(m8.tolist(), 'rggb')
    for depth in (0, 9, 11, 32, None, '8'):
        with pytest.raises(ValueError):
            BayerFrame(m8, 'rggb', depth=depth)
    with pytest.raises(ValueError):
        BayerFrame(m8, 'rgbg')                                    # unknown pattern
    with pytest.raises(ValueError):
        BayerFrame(m8, 0)
    with pytest.raises(ValueError):
        BayerFrame(m8, 'rggb', method='vng')
    # shapes, and sizes below 2
    with pytest.raises(ValueError):
        BayerFrame(np.zeros((h, w, 1), np.uint8), 'rggb')
    with pytest.raises(ValueError):
        BayerFrame(np.zeros(w * h, np.uint8), 'rggb', (w, h))
    for shape in ((1, w), (h, 1), (0, w), (h, 0)):
        with pytest.raises(ValueError):
            BayerFrame(np.zeros(shape, np.uint8), 'rggb')
    for size in ((1, h), (w, 1), (0, h), (-2, h)):
        with pytest.raises(ValueError):
            BayerFrame(m8, 'rggb', size)
    with pytest.raises(ValueError):
        BayerFrame(m8, 'rggb', (w, h + 1))                        # rows
    with pytest.raises(ValueError):
        BayerFrame(m8, 'rggb', (w + 1, h))                        # rows one sample short
    # pitch and views
    big = rng.integers(0, 256, (h + 2, w + 5), dtype=np.uint8)
    f = BayerFrame(big[1:1 + h, 2:2 + w], 'gbrg')
    assert f.pitch == w + 5 and f.size == (w, h) and np.array_equal(f.to_bgr(), bayer_to_bgr(big[1:1 + h, 2:2 + w].copy(), None, 'gbrg'))
    f = BayerFrame(big[:h], 'gbrg', (w, h))                       # (H, pitch) with size
    assert f.pitch == w + 5 and f.rows.shape == (h, w) and np.array_equal(f.to_bgr(), bayer_to_bgr(big[:h, :w].copy(), None, 'gbrg'))
    f = BayerFrame(big[::2, :w][:2], 'gbrg')                      # every other row: a pitch of two rows
    assert f.pitch == 2 * (w + 5) and f.size == (w, 2)
    big16 = rng.integers(0, 1024, (h, w + 3)).astype(np.uint16)
    f = BayerFrame(big16[:, 1:1 + w], 'rggb', depth=10)
    assert f.pitch == 2 * (w + 3) and np.array_equal(f.to_bgr(), bayer_to_bgr(big16[:, 1:1 + w].copy(), None, 'rggb', 10))
    with pytest.raises(ValueError):
        BayerFrame(big[:h, ::2], 'rggb')                          # samples not adjacent
    with pytest.raises(ValueError):
        BayerFrame(m8[::-1], 'rggb')                              # negative pitch
    with pytest.raises(ValueError):
        BayerFrame(np.lib.stride_tricks.as_strided(m8, (h, w), (w - 1, 1)), 'rggb')       # pitch below the row
    with pytest.raises(ValueError):
        BayerFrame(np.broadcast_to(m8[0], (h, w)), 'rggb')        # pitch 0
    # gain and black ranges
    for wb in ((0, 1, 1), (1, 16.01, 1), (1, 1, -1), (1, 1), (1, 1, float('nan')), (1, 1 / 600, 1), 'abc', None):
        with pytest.raises(ValueError):
            BayerFrame(m8, 'rggb', wb=wb)
    assert BayerFrame(m8, 'rggb', wb=(1 / 256, 16, 1.17)).gains == (1, 4096, 300)
    for depth, black in ((8, 256), (8, -1), (12, 4096), (8, 1.5)):
        with pytest.raises(ValueError):
            BayerFrame(m8 if depth == 8 else m16, 'rggb', depth=depth, black=black)
    assert BayerFrame(m16, 'rggb', depth=12, black=4095).black == 4095
    # from_buffer
    buf = rng.integers(0, 256, 16 * (h - 1) + w + 3, dtype=np.uint8)
    f = BayerFrame.from_buffer(buf, (w, h), 'grbg', pitch=16, method='bilinear', wb=(1, 1, 2), black=7)
    assert f.pitch == 16 and f.size == (w, h) and f.method == 'bilinear' and f.black == 7 and f.gains == (256, 256, 512)
    rows = np.stack([buf[16 * r:16 * r + w] for r in range(h)])
    assert np.array_equal(f.to_bgr(), bayer_to_bgr(rows, None, 'grbg', 8, 'bilinear', (1, 1, 2), 7))
    assert BayerFrame.from_buffer(bytes(buf[:w * h]), (w, h), 'rggb').pitch == w
    raw16 = rng.integers(0, 1 << 14, (h, 10)).astype('<u2')
    f = BayerFrame.from_buffer(raw16.tobytes(), (w, h), 'bggr', pitch=20, depth=14)
    assert f.pitch == 20 and np.array_equal(f.to_bgr(), bayer_to_bgr(raw16[:, :w].copy(), None, 'bggr', 14))
    assert np.array_equal(BayerFrame.from_buffer(raw16, (w, h), 'bggr', pitch=20, depth=14).to_bgr(), f.to_bgr())
    with pytest.raises(ValueError):
        BayerFrame.from_buffer(buf, (w, h), 'grbg', pitch=w - 1)                          # short pitch
    with pytest.raises(ValueError):
        BayerFrame.from_buffer(buf[:16 * (h - 1) + w - 1], (w, h), 'grbg', pitch=16)      # short buffer
    with pytest.raises(ValueError):
        BayerFrame.from_buffer(raw16.tobytes(), (w, h), 'bggr', pitch=13, depth=14)       # half a sample
    with pytest.raises(ValueError):
        BayerFrame.from_buffer(buf, (w, 1), 'grbg')
    with pytest.raises(ValueError):
        BayerFrame.from_buffer(buf, (w, h), 'yuy2')
    with pytest.raises(ValueError):
        BayerFrame.from_buffer(buf, (w, h), 'rggb', depth=9)
    with pytest.raises(ValueError):
        BayerFrame.from_buffer(np.zeros((8, 32), np.uint8)[:, ::2], (w, h), 'rggb')
    # the description the library gets
    f = BayerFrame.from_buffer(buf, (w, h), 'gbrg', pitch=16, wb=(2, 1, 0.5), black=5)
    d = f.describe()
    assert (d.pattern, d.width, d.height, d.pitch, d.depth, d.method, d.black, d.gain_r, d.gain_g, d.gain_b) == (2, w, h, 16, 8, 1, 5, 512, 256, 128)
    assert d.data == buf.__array_interface__['data'][0] and f.describe() is d


def test_struct_matches_header():
    """fm_frame_bayer as a C compiler lays it out (LP64): ten int32 in the header's order, then an 8-byte aligned pointer."""
    import re
    from pathlib import Path
    text = (Path(__file__).resolve().parents[1] / 'include' / 'fastmot_hip.h').read_text()
    body = re.search(r'struct fm_frame_bayer \{(.*?)\};', text, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    ints = re.search(r'int32_t([^;]*);', body).group(1).replace(' ', '').split(',')
    assert ints == ['pattern', 'width', 'height', 'pitch', 'depth', 'method', 'black', 'gain_r', 'gain_g', 'gain_b']
    assert re.search(r'const uint8_t\*\s*data;', body) and body.index('int32_t') < body.index('data;')
    F = B.FrameBayer
    assert [name for name, _ in F._fields_] == ints + ['data']
    assert [getattr(F, n).offset for n in ints] == list(range(0, 40, 4)) and F.data.offset == 40
    assert C.sizeof(F) == 48
    for name, value in (('FM_BAYER_RGGB', 0), ('FM_BAYER_GRBG', 1), ('FM_BAYER_GBRG', 2), ('FM_BAYER_BGGR', 3), ('FM_BAYER_BILINEAR', 0),
                        ('FM_BAYER_MHC', 1)):
        assert re.search(rf'#define {name} {value}\b', text)


def test_source_frame_takes_a_bayer_frame():
    f = BayerFrame(np.zeros((5, 7), np.uint8), 'bggr')
    s = SourceFrame(f)
    assert s.size == (7, 5) and s.shape == (5, 7, 3) and s.frame is f
    with pytest.raises(TypeError):
        s.describe()


def test_bayer_entry_points_refuse_null_arguments():
    lib = _lib.load()
    d = BayerFrame(np.zeros((3, 5), np.uint8), 'rggb').describe()
    c = C.c_int
    for rc in (lib.fm_frame_upload_bayer(None, None), lib.fm_frame_upload_bayer(None, C.byref(d)),
               lib.fm_frame_upload_ahead_bayer(None, c(1), None), lib.fm_frame_upload_ahead_bayer(None, c(1), C.byref(d)),
               lib.fm_frame_ring_store_bayer(None, c(0), None), lib.fm_frame_ring_store_bayer(None, c(0), C.byref(d))):
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
    d = tmp_path_factory.mktemp('bayer')
    rng = np.random.default_rng(24)
    out = {'u8': rng.integers(0, 256, (4, 18, 34), dtype=np.uint8),                # 34 x 18
           'u16': rng.integers(0, 4096, (4, 18, 34)).astype(np.uint16),
           'bgr': rng.integers(0, 256, (4, 18, 34, 3), dtype=np.uint8)}
    for name, a in out.items():
        np.save(d / f'{name}.npy', a)
    return d, out


def test_videoio_converts_on_the_capture_thread(stacks):
    from fastmot_amd.videoio import resize_bgr
    d, data = stacks
    for pattern in PATTERNS:
        video = VideoIO((34, 18), str(d / 'u8.npy'), pixel_format=pattern)
        assert video.resolution == (34, 18)
        got = read_all(video)
        assert len(got) == 4
        for g, raw in zip(got, data['u8']):
            assert isinstance(g, np.ndarray) and np.array_equal(g, bayer_to_bgr(raw, (34, 18), pattern))
    got = read_all(VideoIO((34, 18), str(d / 'u16.npy'), pixel_format='grbg12', demosaic='bilinear', white_balance=(1.5, 1, 2), black_level=64))
    assert len(got) == 4
    for g, raw in zip(got, data['u16']):
        assert np.array_equal(g, bayer_to_bgr(raw, None, 'grbg', 12, 'bilinear', (1.5, 1, 2), 64))
    got = read_all(VideoIO((34, 18), str(d / 'u16.npy'), pixel_format='bggr16'))
    assert np.array_equal(got[1], bayer_to_bgr(data['u16'][1], None, 'bggr', 16))
    # another size: resized here, as every other input is
    got = read_all(VideoIO((17, 9), str(d / 'u8.npy'), pixel_format='rggb'))
    assert np.array_equal(got[0], resize_bgr(bayer_to_bgr(data['u8'][0], None, 'rggb'), (17, 9)))
    # stream_cfg reaches it as keywords
    video = VideoIO((34, 18), str(d / 'u8.npy'), None, **{'buffer_size': 3, 'pixel_format': 'gbrg', 'demosaic': 'bilinear', 'black_level': 3})
    assert np.array_equal(read_all(video)[0], bayer_to_bgr(data['u8'][0], None, 'gbrg', 8, 'bilinear', black=3))


def test_videoio_frame_kinds(stacks):
    """gpu_decode / gpu_resize choose the frame kind as they do for a packed stack (no GPU is touched by reading)."""
    d, data = stacks
    got = read_all(VideoIO((34, 18), str(d / 'u16.npy'), pixel_format='rggb12', gpu_decode=True, demosaic='bilinear',
                           white_balance=(2, 1, 1), black_level=16))
    assert len(got) == 4 and all(isinstance(g, BayerFrame) and g.size == (34, 18) and g.depth == 12 and g.method == 'bilinear'
                                 and g.gains == (512, 256, 256) and g.black == 16 and g.pattern == 'rggb' for g in got)
    assert np.array_equal(got[2].to_bgr(), bayer_to_bgr(data['u16'][2], None, 'rggb', 12, 'bilinear', (2, 1, 1), 16))
    got = read_all(VideoIO((17, 9), str(d / 'u8.npy'), pixel_format='bggr', gpu_decode=True))
    assert all(isinstance(g, np.ndarray) and g.shape == (9, 17, 3) for g in got)       # no gpu_resize: host pixels
    got = read_all(VideoIO((17, 9), str(d / 'u8.npy'), pixel_format='bggr', gpu_decode=True, gpu_resize=True))
    assert all(isinstance(g, SourceFrame) and isinstance(g.frame, BayerFrame) and g.size == (34, 18) for g in got)
    got = read_all(VideoIO((34, 18), str(d / 'u8.npy'), pixel_format='bggr', gpu_decode=True, gpu_resize=True))
    assert all(isinstance(g, BayerFrame) for g in got)                                  # on size: bare
    got = read_all(VideoIO((34, 18), str(d / 'u8.npy'), str(d / 'o.npy'), pixel_format='bggr', gpu_decode=True))
    assert all(isinstance(g, np.ndarray) for g in got)                                  # an output that needs host pixels


def test_videoio_refuses_at_open(stacks, tmp_path):
    d, data = stacks
    with pytest.raises(ValueError):
        VideoIO((34, 18), str(d / 'u8.npy'), pixel_format='rggb12')                    # uint8 where the depth wants uint16
    with pytest.raises(ValueError):
        VideoIO((34, 18), str(d / 'u16.npy'), pixel_format='rggb')
    with pytest.raises(ValueError):
        VideoIO((34, 18), str(d / 'bgr.npy'), pixel_format='rggb')                     # a 4-D stack is no mosaic stack
    with pytest.raises(ValueError):
        VideoIO((34, 18), str(d / 'bgr.npy'), pixel_format='i420')                     # stays what it was
    for bad in ('rggb8', 'rggb9', 'rgbg', 'RGGB'):
        with pytest.raises(ValueError):
            VideoIO((34, 18), str(d / 'u8.npy'), pixel_format=bad)
    np.save(tmp_path / 'thin.npy', np.zeros((2, 6, 1), np.uint8))
    with pytest.raises(ValueError):
        VideoIO((1, 6), str(tmp_path / 'thin.npy'), pixel_format='rggb')               # one sample wide
    np.save(tmp_path / 'f32.npy', np.zeros((2, 6, 12), np.float32))
    with pytest.raises(ValueError):
        VideoIO((12, 6), str(tmp_path / 'f32.npy'), pixel_format='rggb16')
    with pytest.raises(ValueError):
        VideoIO((34, 18), str(d / 'u8.npy'), pixel_format='rggb', demosaic='vng')
    with pytest.raises(ValueError):
        VideoIO((34, 18), str(d / 'u8.npy'), pixel_format='rggb', white_balance=(1, 1, 17))
    with pytest.raises(ValueError):
        VideoIO((34, 18), str(d / 'u8.npy'), pixel_format='rggb', black_level=256)
    with pytest.raises(ValueError):
        VideoIO((34, 18), str(d / 'missing-%06d.png'), pixel_format='rggb')            # the option belongs to '.npy' stacks


def test_videoio_without_pixel_format_is_unchanged(stacks):
    d, data = stacks
    for kw in ({}, {'pixel_format': None}, {'demosaic': 'bilinear', 'black_level': 9}):
        got = read_all(VideoIO((34, 18), str(d / 'bgr.npy'), **kw))
        assert len(got) == 4 and all(np.array_equal(g, raw) for g, raw in zip(got, data['bgr']))
    with pytest.raises(RuntimeError):                                                   # and a 3-D stack is still no BGR stack
        VideoIO((34, 18), str(d / 'u8.npy'))
