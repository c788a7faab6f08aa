"""CPU: 9- to 16-bit YCbCr frames (fastmot_amd/utils/deep.py), the deep tokens of YUV4MPEG2 text and VideoIO's deep '.y4m'
source on the host path.  The numpy functions here are what test_deep_gpu.py holds the kernel of csrc/deep.hip to, so they
are pinned by NV12's function (shift consistency), by the real-number formula (a derived bound) and by values worked out
by hand."""
import numpy as np
import pytest

from fastmot_amd import DeepFrame, VideoIO
from fastmot_amd.utils import deep
from fastmot_amd.utils.deep import MATRICES, deep_frame_bytes, deep_to_bgr, deep_yuv_to_bgr, semiplanar_to_bgr
from fastmot_amd.utils.nv12 import MATRICES as NV12_MATRICES, yuv_to_bgr
from fastmot_amd.utils.yuv import chroma_shape, parse_y4m_header
from fastmot_amd.videoio import resize_bgr

# the real-number matrices: (cy, cvr, cub, cug, cvg).  'bt601' is the formula the NV12 constants were rounded from
# (OpenCV's), not the exact BT.601 ratios.
def _real(kr, kb):
    kg, c = 1 - kr - kb, 255 / 224
    return (255 / 219, 2 * (1 - kr) * c, 2 * (1 - kb) * c, -2 * (1 - kb) * kb / kg * c, -2 * (1 - kr) * kr / kg * c)


REAL = {'bt601': (1.164, 1.596, 2.018, -0.391, -0.813), 'bt709': _real(0.2126, 0.0722), 'bt2020': _real(0.2627, 0.0593)}
# |integer result - clipped unrounded real value|: half a step of rounding, plus three coefficients each off by at most
# 2^-21 (rounded to 20 fractional bits) times sample magnitudes below 2^8: 3 * 2^-13 < 2^-11
BOUND = 0.5 + 2.0 ** -11


def real_bgr(Y, U, V, depth, matrix):
    """The float64 formula, unrounded and unclipped, [..., 3] in B, G, R order."""
    cy, cvr, cub, cug, cvg = REAL[matrix]
    s = depth - 8
    y = np.maximum(Y.astype(np.float64) - (16 << s), 0) * cy
    u, v = U.astype(np.float64) - (128 << s), V.astype(np.float64) - (128 << s)
    return np.stack([y + cub * u, y + cug * u + cvg * v, y + cvr * v], -1) / (1 << s)


def check_against_real(Y, U, V, depth, matrix):
    got = deep_yuv_to_bgr(Y, U, V, depth, matrix).astype(np.float64)
    real = real_bgr(Y, U, V, depth, matrix)
    dev = np.abs(got - np.clip(real, 0, 255)).max()
    assert dev <= BOUND, (matrix, depth, dev)
    half_up = np.clip(np.floor(real + 0.5), 0, 255)
    assert np.abs(got - half_up).max() <= 1, (matrix, depth)
    return dev, (got != half_up).mean()


def test_matrices():
    for name in ('bt601', 'bt709'):
        assert MATRICES[name] == NV12_MATRICES[name]               # ids and the five constants
    assert MATRICES['bt2020'][0] == 2
    want = tuple(int(np.floor(c * 2 ** 20 + 0.5)) for c in _real(0.2627, 0.0593))
    assert MATRICES['bt2020'][1] == want == (1220945, 1760217, 2245811, -196426, -682019)
    for name, (_, consts) in MATRICES.items():                     # every constant is within 2^-21 of its real value
        assert all(abs(c / 2 ** 20 - r) <= 2.0 ** -21 for c, r in zip(consts, REAL[name])), name
    with pytest.raises(ValueError):
        deep.matrix_id('bt601-full')


@pytest.mark.parametrize('depth', [9, 10, 12, 14, 16])
@pytest.mark.parametrize('matrix', ['bt601', 'bt709'])
def test_shift_consistency(matrix, depth):
    """Samples that are 8-bit samples shifted left by s convert to what the 8-bit arithmetic gives, bit for bit."""
    s = depth - 8
    Y, U = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
    for V in (0, 1, 16, 77, 127, 128, 129, 200, 240, 254, 255):
        v8 = np.full(Y.shape, V, np.uint8)
        got = deep_yuv_to_bgr(Y.astype(np.uint16) << s, U.astype(np.uint16) << s, v8.astype(np.uint16) << s, depth, matrix)
        assert np.array_equal(got, yuv_to_bgr(Y, U, v8, matrix)), V


@pytest.mark.parametrize('depth', [10, 12, 16])
@pytest.mark.parametrize('matrix', ['bt601', 'bt709', 'bt2020'])
def test_close_to_the_real_formula_random(matrix, depth):
    rng = np.random.default_rng(depth * 7 + MATRICES[matrix][0])
    Y, U, V = rng.integers(0, 1 << depth, (3, 1 << 20), dtype=np.int64)
    dev, share = check_against_real(Y, U, V, depth, matrix)
    print(f'{matrix} depth {depth}: largest deviation {dev:.6f}, share differing from the rounded float {share:.2e}')


@pytest.mark.parametrize('matrix', ['bt601', 'bt709', 'bt2020'])
def test_close_to_the_real_formula_all_luma(matrix):
    """Every Y of depth 10 against a chroma lattice that holds 0, 1, the centre and its neighbours, and the maximum."""
    lattice = np.unique(np.concatenate([np.arange(0, 1024, 37), [0, 1, 511, 512, 513, 1022, 1023]]))
    Y, U, V = np.meshgrid(np.arange(1024), lattice, lattice, indexing='ij')
    check_against_real(Y, U, V, 10, matrix)


def test_hand_checked_values():
    one = lambda Y, U, V, d, m='bt709': deep_yuv_to_bgr(Y, U, V, d, m).tolist()
    for d in (9, 10, 12, 14, 16):
        s = d - 8
        for m in MATRICES:
            assert one(16 << s, 128 << s, 128 << s, d, m) == [0, 0, 0]             # black
            assert one(235 << s, 128 << s, 128 << s, d, m) == [255, 255, 255]     # white: (219 CY + 2^19) >> 20 = 255
            assert one((16 << s) - 1, 128 << s, 128 << s, d, m) == [0, 0, 0]      # below black: the luma term is clamped
            assert one(0, 128 << s, 128 << s, d, m) == [0, 0, 0]
    # depth 10, BT.709: y = (500 - 64) 1220945 = 532332020, u = -112, v = 188, h = 2^21
    #   B = (534429172 - 248081568) >> 22 = 286347604 >> 22 = 68    G = 454419508 >> 22 = 108    R = 887836272 >> 22 = 211
    assert one(500, 400, 700, 10) == [68, 108, 211]
    assert one(500, 400, 700, 10, 'bt601') == [70, 100, 202]
    assert one(500, 400, 700, 10, 'bt2020') == [67, 102, 206]
    assert one(2000, 2500, 1800, 12) == [187, 129, 99]
    # depth 16: the sums pass 2^32 (the 64-bit case).  BT.709, (40000, 20000, 50000): 15689728256, 37196868512 and
    # 76364171408, >> 28: 58, 138 and 284 -> 255
    assert one(40000, 20000, 50000, 16) == [58, 138, 255]
    assert one(40000, 20000, 50000, 16, 'bt601') == [63, 128, 255]
    assert one(40000, 20000, 50000, 16, 'bt2020') == [56, 129, 255]
    # saturating chroma: B's sum is 147727221321 (about 2^37.1), R's 13549751983 -> 50; and the negative extreme
    assert one(65535, 65535, 0, 16) == [255, 255, 50]
    assert one(0, 0, 65535, 16) == [0, 0, 229]
    assert one(65535, 65535, 0, 16, 'bt2020') == [255, 255, 65]
    assert one(0, 0, 65535, 16, 'bt2020') == [0, 0, 215]
    assert one(65535, 65535, 0, 16, 'bt601') == [255, 255, 75]
    with pytest.raises(ValueError):
        one(0, 0, 0, 8)
    with pytest.raises(ValueError):
        one(0, 0, 0, 17)


def planes(rng, w, h, chroma, depth, stray=False):
    top = 1 << (16 if stray else depth)
    y = rng.integers(0, top, (h, w), dtype=np.uint16)
    cs = chroma_shape((w, h), chroma)
    if cs is None:
        return y, None, None
    return y, rng.integers(0, top, cs, dtype=np.uint16), rng.integers(0, top, cs, dtype=np.uint16)


def test_chroma_sample_per_pixel():
    rng = np.random.default_rng(3)
    w, h = 7, 5
    for chroma, (sh, sv) in {'420': (1, 1), '422': (1, 0), '444': (0, 0)}.items():
        y, u, v = planes(rng, w, h, chroma, 12)
        got = deep_to_bgr(y, u, v, chroma, 12, 'bt2020')
        for r in range(h):
            for c in range(w):
                want = deep_yuv_to_bgr(y[r, c], u[r >> sv, c >> sh], v[r >> sv, c >> sh], 12, 'bt2020')
                assert np.array_equal(got[r, c], want), (chroma, r, c)
    y = planes(rng, w, h, 'mono', 12)[0]
    assert np.array_equal(deep_to_bgr(y, None, None, 'mono', 12), deep_yuv_to_bgr(y, np.full_like(y, 2048), np.full_like(y, 2048), 12))


@pytest.mark.parametrize('depth', [10, 12, 16])
def test_stray_bits_are_masked(depth):
    rng = np.random.default_rng(depth)
    w, h = 10, 6
    rs = 16 - depth
    # planar: bits above `depth` do not reach the arithmetic
    y, u, v = planes(rng, w, h, '420', depth, stray=True)
    mask = (1 << depth) - 1
    assert np.array_equal(deep_to_bgr(y, u, v, '420', depth), deep_to_bgr(y & mask, u & mask, v & mask, '420', depth))
    if depth < 16:
        assert (y > mask).any()
    # semi-planar: the low bits are ignored
    ys = rng.integers(0, 1 << 16, (h, w), dtype=np.uint16)
    uv = rng.integers(0, 1 << 16, (h // 2, w), dtype=np.uint16)
    clean = lambda p: (p >> rs) << rs
    assert np.array_equal(semiplanar_to_bgr(ys, uv, depth), semiplanar_to_bgr(clean(ys), clean(uv), depth))
    # ... and the frame is planar 4:2:0 of the de-interleaved planes, shifted right
    want = deep_to_bgr(ys >> rs, uv[:, 0::2] >> rs, uv[:, 1::2] >> rs, '420', depth, 'bt2020')
    assert np.array_equal(semiplanar_to_bgr(ys, uv, depth, 'bt2020'), want)
    assert np.array_equal(DeepFrame.semiplanar(ys, uv, depth, 'bt2020').to_bgr(), want)


def test_frame_checks_and_describe():
    rng = np.random.default_rng(4)
    w, h = 7, 5
    y, u, v = planes(rng, w, h, '420', 10)
    f = DeepFrame(y, u, v)
    assert f.size == (w, h) and f.shape == (h, w, 3) and f.chroma == '420' and f.depth == 10 and f.matrix == 'bt709'
    assert f.layout == 'planar' and f.pitch == 2 * w and f.pitch_c == 2 * 4
    assert np.array_equal(f.to_bgr(), deep_to_bgr(y, u, v, '420', 10, 'bt709'))
    d = f.describe()
    assert (d.width, d.height, d.chroma, d.matrix, d.depth, d.layout, d.pitch_y, d.pitch_c) == (w, h, 0, 1, 10, 0, 14, 8)
    assert d.y == y.ctypes.data and d.u == u.ctypes.data and d.v == v.ctypes.data
    assert f.describe() is d
    # views into larger arrays: pitches in bytes, not copied
    wide = rng.integers(0, 1024, (h, w + 3), dtype=np.uint16)
    cw = rng.integers(0, 1024, (2, 3, 4 + 5), dtype=np.uint16)
    g = DeepFrame(wide[:, :w], cw[0, :, :4], cw[1, :, :4], '420', 12, 'bt2020')
    assert g.pitch == 2 * (w + 3) and g.pitch_c == 2 * 9 and g.y.base is wide and g.matrix_id == 2
    m = DeepFrame(y, chroma='mono', depth=16)
    assert m.pitch_c == 0 and not m.describe().u and not m.describe().v
    with pytest.raises(TypeError):
        DeepFrame(y.astype(np.uint8), u, v)
    with pytest.raises(TypeError):
        DeepFrame(y, u.astype(np.int16), v)
    with pytest.raises(TypeError):
        DeepFrame(y.tolist(), u, v)
    for bad in (dict(chroma='411'), dict(depth=8), dict(depth=17), dict(depth=10.0), dict(matrix='bt709-full'), dict(matrix=None)):
        with pytest.raises(ValueError):
            DeepFrame(y, u, v, **bad)
    with pytest.raises(ValueError):
        DeepFrame(y, u, v[:, :3])                                  # shape of a chroma plane
    with pytest.raises(ValueError):
        DeepFrame(y, u, None)
    with pytest.raises(ValueError):
        DeepFrame(y, u, v, 'mono')
    with pytest.raises(ValueError):
        DeepFrame(y, u, cw[1, :, :4])                              # u and v with different pitches
    with pytest.raises(ValueError):
        DeepFrame(wide[:, ::2], chroma='mono')                    # samples of a row not adjacent
    odd = np.ndarray((h, w), np.uint16, np.zeros(h * (2 * w + 1), np.uint8), 0, (2 * w + 1, 2))
    with pytest.raises(ValueError, match='odd'):
        DeepFrame(odd, chroma='mono')
    with pytest.raises(ValueError):
        DeepFrame(np.empty((0, 4), np.uint16), chroma='mono')


def test_semiplanar_frame():
    rng = np.random.default_rng(5)
    w, h = 10, 6
    y = rng.integers(0, 1 << 16, (h, w + 2), dtype=np.uint16)[:, :w]
    uv = rng.integers(0, 1 << 16, (h // 2, w + 2), dtype=np.uint16)[:, :w]
    f = DeepFrame.semiplanar(y, uv)
    assert f.layout == 'semiplanar' and f.chroma == '420' and f.depth == 10 and f.matrix == 'bt709' and f.size == (w, h)
    assert f.pitch == f.pitch_c == 2 * (w + 2) and f.uv is uv and f.u is None
    d = f.describe()
    assert (d.layout, d.chroma, d.depth, d.pitch_y, d.pitch_c) == (1, 0, 10, 24, 24) and d.u == uv.ctypes.data and not d.v
    with pytest.raises(TypeError):
        DeepFrame.semiplanar(y.astype(np.uint8), uv)
    with pytest.raises(ValueError):
        DeepFrame.semiplanar(y[:5], uv)                            # odd height
    with pytest.raises(ValueError):
        DeepFrame.semiplanar(y[:, :9], uv[:, :9])                  # odd width
    with pytest.raises(ValueError):
        DeepFrame.semiplanar(y, uv[:2])
    with pytest.raises(ValueError):
        DeepFrame.semiplanar(y, uv, depth=8)
    with pytest.raises(ValueError):
        DeepFrame.semiplanar(y, uv, matrix='bt2100')


def test_from_buffer_forms():
    rng = np.random.default_rng(6)
    w, h = 7, 5
    n = deep_frame_bytes((w, h), '420')
    assert n == 2 * (35 + 2 * 12)
    words = rng.integers(0, 1024, n // 2 + 3, dtype=np.uint16)
    for buf in (words, words.view(np.uint8), words.tobytes()):
        f = DeepFrame.from_buffer(buf, (w, h), '420', 10, 'bt2020')
        assert np.array_equal(f.y.ravel(), words[:35]) and np.array_equal(f.u.ravel(), words[35:47])
        assert np.array_equal(f.v.ravel(), words[47:59]) and f.matrix == 'bt2020' and f.pitch == 14 and f.pitch_c == 8
    assert np.shares_memory(DeepFrame.from_buffer(words, (w, h)).y, words)          # not copied
    mono = DeepFrame.from_buffer(words, (w, h), 'mono', 16)
    assert mono.u is None and np.array_equal(mono.y.ravel(), words[:35])
    with pytest.raises(ValueError):
        DeepFrame.from_buffer(words.view(np.uint8)[:n - 1], (w, h), '420')
    with pytest.raises(ValueError):
        DeepFrame.from_buffer(words, (0, h))
    with pytest.raises(TypeError):
        DeepFrame.from_buffer(words.astype(np.float32), (w, h))
    with pytest.raises(ValueError):
        DeepFrame.from_buffer(np.zeros((40, 40), np.uint16)[:, ::2], (w, h))
    # a decoder surface: pitch and uv_offset in bytes
    w, h, pitch, rows = 10, 6, 32, 8
    surf = rng.integers(0, 1 << 16, (rows + h // 2) * pitch // 2, dtype=np.uint16)
    f = DeepFrame.semiplanar_from_buffer(surf, (w, h), pitch=pitch, uv_offset=rows * pitch, depth=12)
    grid = surf.reshape(-1, pitch // 2)
    assert np.array_equal(f.y, grid[:h, :w]) and np.array_equal(f.uv, grid[rows:rows + h // 2, :w])
    assert f.pitch == f.pitch_c == pitch and f.depth == 12 and np.shares_memory(f.y, surf)
    g = DeepFrame.semiplanar_from_buffer(surf.tobytes(), (w, h), pitch=pitch, uv_offset=rows * pitch, depth=12)
    assert np.array_equal(g.to_bgr(), f.to_bgr())
    packed = DeepFrame.semiplanar_from_buffer(surf, (w, h))
    assert packed.pitch == 2 * w and np.array_equal(packed.uv.ravel(), surf[w * h:w * h + w * h // 2])
    for bad in (dict(pitch=2 * w - 2), dict(pitch=2 * w + 1), dict(pitch=pitch, uv_offset=pitch * (h - 1)), dict(pitch=pitch, uv_offset=rows * pitch + 1)):
        with pytest.raises(ValueError):
            DeepFrame.semiplanar_from_buffer(surf, (w, h), **bad)
    with pytest.raises(ValueError):
        DeepFrame.semiplanar_from_buffer(surf, (9, 6))
    with pytest.raises(ValueError):
        DeepFrame.semiplanar_from_buffer(surf[:w * h + w * h // 2 - 1], (w, h))


DEEP_TOKENS = ([(f'C{c}p{d}', c, d) for c in ('420', '422', '444') for d in (9, 10, 12, 14, 16)] +
               [(f'Cmono{d}', 'mono', d) for d in (9, 10, 12, 16)])


def test_y4m_header_deep_tokens():
    for token, chroma, depth in DEEP_TOKENS:
        line = f'YUV4MPEG2 W34 H18 F25:1 Ip {token} XCOLORRANGE=LIMITED\n'
        info = parse_y4m_header(line, deep=True)
        assert (info['size'], info['chroma'], info['depth'], info['interlace']) == ((34, 18), chroma, depth, 'p'), token
        assert parse_y4m_header(line.encode(), deep=True) == info
        with pytest.raises(ValueError, match=token):
            parse_y4m_header(line)                                 # without the flag nothing changes
        with pytest.raises(ValueError, match=token):
            parse_y4m_header(line, deep=False)
    for token, chroma in (('C420jpeg', '420'), ('C422', '422'), ('Cmono', 'mono')):
        info = parse_y4m_header(f'YUV4MPEG2 W4 H4 {token}', deep=True)
        assert info['chroma'] == chroma and info['depth'] == 8
        assert 'depth' not in parse_y4m_header(f'YUV4MPEG2 W4 H4 {token}')
    assert parse_y4m_header('YUV4MPEG2 W4 H4', deep=True)['depth'] == 8
    for bad in ('C420p11', 'C420p8', 'Cmono14', 'C411p10', 'C444alpha', 'C420p10le', 'It', 'XCOLORRANGE=FULL'):
        with pytest.raises(ValueError, match=bad):
            parse_y4m_header(f'YUV4MPEG2 W4 H4 {bad}', deep=True)


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


CLIPS = [((34, 18), 'C420p10', '420', 10), ((7, 5), 'C444p12', '444', 12), ((9, 4), 'Cmono16', 'mono', 16)]


def write_clip(path, size, token, chroma, depth, n=3, seed=0):
    """A hand-written deep .y4m of n random frames; returns the frames' planes."""
    rng = np.random.default_rng(seed)
    out = [f'YUV4MPEG2 W{size[0]} H{size[1]} F25:1 Ip A1:1 {token}\n'.encode()]
    frames = []
    for _ in range(n):
        p = planes(rng, size[0], size[1], chroma, depth)
        frames.append(p)
        out.append(b'FRAME\n' + b''.join(x.astype('<u2').tobytes() for x in p if x is not None))
    path.write_bytes(b''.join(out))
    return frames


@pytest.mark.parametrize('size,token,chroma,depth', CLIPS, ids=[c[1] for c in CLIPS])
def test_videoio_reads_a_deep_y4m(tmp_path, size, token, chroma, depth):
    path = tmp_path / 'deep.y4m'
    frames = write_clip(path, size, token, chroma, depth)
    for matrix in ('bt601', 'bt709', 'bt2020'):
        video = VideoIO(size, str(path), deep_color=True, yuv_matrix=matrix)
        assert video.resolution == size and video.cap_fps == 25
        got = read_all(video)
        assert len(got) == 3
        for g, p in zip(got, frames):
            assert isinstance(g, np.ndarray) and np.array_equal(g, deep_to_bgr(*p, chroma, depth, matrix))
    small = (max(size[0] // 2, 1), max(size[1] // 2, 1))
    for other in (small, (size[0] + 3, size[1] + 1)):
        got = read_all(VideoIO(other, str(path), deep_color=True))
        assert len(got) == 3
        for g, p in zip(got, frames):
            assert np.array_equal(g, resize_bgr(deep_to_bgr(*p, chroma, depth, 'bt601'), other))
    # gpu_decode: DeepFrames over the same samples (of another size: wrapped under gpu_resize, host pixels without)
    got = read_all(VideoIO(size, str(path), deep_color=True, gpu_decode=True, yuv_matrix='bt2020'))
    for g, p in zip(got, frames):
        assert isinstance(g, DeepFrame) and (g.chroma, g.depth, g.matrix, g.size) == (chroma, depth, 'bt2020', size)
        assert np.array_equal(g.to_bgr(), deep_to_bgr(*p, chroma, depth, 'bt2020'))
    from fastmot_amd import SourceFrame
    got = read_all(VideoIO(small, str(path), deep_color=True, gpu_decode=True, gpu_resize=True))
    assert all(isinstance(g, SourceFrame) and isinstance(g.frame, DeepFrame) for g in got)
    got = read_all(VideoIO(small, str(path), deep_color=True, gpu_decode=True))
    assert all(isinstance(g, np.ndarray) and g.shape == (small[1], small[0], 3) for g in got)
    # without the flag the stream is refused, with the token named
    with pytest.raises(ValueError, match=token):
        VideoIO(size, str(path))
    with pytest.raises(ValueError, match=token):
        VideoIO(size, str(path), gpu_decode=True, yuv_matrix='bt709')
    with pytest.raises(ValueError):
        VideoIO(size, str(path), deep_color=True, yuv_matrix='bt709-full')


def test_videoio_deep_color_and_8_bit_files(tmp_path):
    """The flag changes nothing for an 8-bit file: same pixels, and 'bt2020' stays refused for it."""
    from fastmot_amd.utils.yuv import planar_to_bgr
    rng = np.random.default_rng(9)
    y, u, v = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((18, 34), (9, 17), (9, 17)))
    p = tmp_path / 'eight.y4m'
    p.write_bytes(b'YUV4MPEG2 W34 H18 F25:1 C420jpeg\nFRAME\n' + y.tobytes() + u.tobytes() + v.tobytes())
    for flag in (False, True):
        got = read_all(VideoIO((34, 18), str(p), deep_color=flag, yuv_matrix='bt709'))
        assert len(got) == 1 and np.array_equal(got[0], planar_to_bgr(y, u, v, '420', 'bt709'))
        with pytest.raises(ValueError):
            VideoIO((34, 18), str(p), deep_color=flag, yuv_matrix='bt2020')
    for bad in (b'XCOLORRANGE=FULL', b'It'):
        q = tmp_path / 'bad.y4m'
        q.write_bytes(b'YUV4MPEG2 W34 H18 F25:1 C420p10 ' + bad + b'\n')
        with pytest.raises(ValueError):
            VideoIO((34, 18), str(q), deep_color=True)


@pytest.mark.parametrize('cut', ['payload', 'frame_header'])
def test_truncated_last_deep_frame_ends_the_stream(tmp_path, cut):
    size, token, chroma, depth = CLIPS[0]
    path = tmp_path / 'deep.y4m'
    frames = write_clip(path, size, token, chroma, depth)
    data = path.read_bytes()
    n = 6 + deep_frame_bytes(size, chroma)
    p = tmp_path / 'cut.y4m'
    p.write_bytes(data[:len(data) - (n // 2 if cut == 'payload' else n - 3)])
    got = read_all(VideoIO(size, str(p), deep_color=True))
    assert len(got) == 2
    for g, f in zip(got, frames):
        assert np.array_equal(g, deep_to_bgr(*f, chroma, depth, 'bt601'))
