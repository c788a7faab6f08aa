"""CPU: planar YCbCr frames and YUV4MPEG2 text (fastmot_amd/utils/yuv.py), and VideoIO's '.y4m' source and output on the
host path.  The numpy functions here are what test_yuv_gpu.py holds the kernels of csrc/yuv.hip to, so they are pinned by
NV12's functions (test_nv12_host.py pins those) and by values worked out by hand."""
from fractions import Fraction

import numpy as np
import pytest

from fastmot_amd import PlanarFrame, VideoIO
from fastmot_amd.utils.nv12 import bgr_to_nv12, nv12_to_bgr
from fastmot_amd.utils.yuv import (I420Image, bgr_to_planar420, chroma_shape, frame_bytes, parse_y4m_header, planar_to_bgr,
                                   y4m_header)
from fastmot_amd.videoio import resize_bgr


def planes(rng, w, h, chroma):
    y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    cs = chroma_shape((w, h), chroma)
    if cs is None:
        return y, None, None
    return y, rng.integers(0, 256, cs, dtype=np.uint8), rng.integers(0, 256, cs, dtype=np.uint8)


@pytest.mark.parametrize('matrix', ['bt601', 'bt709'])
def test_420_on_even_sizes_is_nv12(matrix):
    rng = np.random.default_rng(1)
    for w, h in ((2, 2), (8, 6), (34, 18)):
        y, u, v = planes(rng, w, h, '420')
        uv = np.empty((h // 2, w), np.uint8)
        uv[:, 0::2], uv[:, 1::2] = u, v
        assert np.array_equal(planar_to_bgr(y, u, v, '420', matrix), nv12_to_bgr(y, uv, matrix))


def test_bgr_to_planar420_on_even_sizes_is_bgr_to_nv12():
    rng = np.random.default_rng(2)
    for w, h in ((2, 2), (8, 6), (34, 18)):
        f = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        y, u, v = bgr_to_planar420(f)
        ny, nuv = bgr_to_nv12(f)
        assert np.array_equal(y, ny) and np.array_equal(u, nuv[:, 0::2]) and np.array_equal(v, nuv[:, 1::2])


def test_chroma_sample_per_pixel():
    """Pixel (r, c) uses sample (r >> sv, c >> sh): a frame with constant Y makes the chroma index visible."""
    rng = np.random.default_rng(3)
    w, h = 7, 5
    for chroma, (sh, sv) in {'420': (1, 1), '422': (1, 0), '444': (0, 0)}.items():
        y, u, v = planes(rng, w, h, chroma)
        got = planar_to_bgr(y, u, v, chroma)
        for r in range(h):
            for c in range(w):
                one = planar_to_bgr(y[r:r + 1, c:c + 1], u[r >> sv:(r >> sv) + 1, c >> sh:(c >> sh) + 1],
                                    v[r >> sv:(r >> sv) + 1, c >> sh:(c >> sh) + 1], '444')
                assert np.array_equal(got[r, c], one[0, 0]), (chroma, r, c)


def test_hand_checked_values():
    one = lambda Y, U, V, m='bt601': planar_to_bgr(*(np.array([[x]], np.uint8) for x in (Y, U, V)), '420', m)[0, 0].tolist()
    # a 1 x 1 frame: (1220542 * (Y - 16) + 2^19) >> 20 with neutral chroma
    assert one(16, 128, 128) == [0, 0, 0]
    assert one(235, 128, 128) == [255, 255, 255]
    assert one(126, 128, 128) == [128, 128, 128]          # (110 * 1220542 + 524288) >> 20 = 128
    # Y below 16 is black, Y = 255 saturates
    assert one(0, 128, 128) == one(15, 128, 128) == [0, 0, 0]
    assert one(255, 128, 128) == [255, 255, 255]
    # U = 255, V = 128 at Y = 126: B = (134259620 + 2116026 * 127 + 524288) >> 20 = 384 -> 255,
    # G = (134259620 - 409993 * 127 + 524288) >> 20 = 78, R unchanged
    assert one(126, 255, 128) == [255, 78, 128]
    # mono: B = G = R
    y = np.array([[0, 16, 100, 235, 255]], np.uint8)
    m = planar_to_bgr(y, None, None, 'mono')
    assert np.array_equal(m[..., 0], m[..., 1]) and np.array_equal(m[..., 1], m[..., 2])
    assert m[0, :, 0].tolist() == [0, 0, 98, 255, 255]    # (84 * 1220542 + 524288) >> 20 = 98

    # BGR -> I420, 1 x 1: the pixel four times over is the pixel
    for bgr, yuv in (((0, 0, 0), (16, 128, 128)), ((255, 255, 255), (235, 128, 128)), ((255, 0, 0), (41, 240, 110)),
                     ((0, 0, 255), (82, 90, 240))):
        got = bgr_to_planar420(np.array([[bgr]], np.uint8))
        assert tuple(int(p[0, 0]) for p in got) == yuv, bgr
    # 3 x 3: black except a blue last column and a red last row (the corner is red).  U of blue 240, of red 90, of black 128.
    f = np.zeros((3, 3, 3), np.uint8)
    f[:, 2] = (255, 0, 0)
    f[2, :] = (0, 0, 255)
    y, u, v = bgr_to_planar420(f)
    assert y.shape == (3, 3) and u.shape == v.shape == (2, 2)
    assert u.tolist() == [[128, 240],      # top right: column 2 twice over, rows 0 and 1 -> four blue pixels
                          [90, 90]]        # bottom row: row 2 twice over -> four red pixels
    assert v.tolist() == [[128, 110], [240, 240]]
    # ... and when the last column decides only half of a mean: rows 0..1 of columns 2..3 -> column 2 counted twice
    g = np.zeros((2, 3, 3), np.uint8)
    g[0, 2] = (255, 0, 0)                  # U 240 twice, 128 twice: (736 + 2) >> 2 = 184
    assert bgr_to_planar420(g)[1].tolist() == [[128, 184]]


def test_header_parser():
    h = parse_y4m_header(b'YUV4MPEG2 W1920 H1080 F30000:1001 Ip A1:1 C420jpeg XYSCSS=420JPEG XCOLORRANGE=LIMITED\n')
    assert h['size'] == (1920, 1080) and h['fps'] == Fraction(30000, 1001) and h['chroma'] == '420' and h['interlace'] == 'p'
    assert h['aspect'] == '1:1'
    base = 'YUV4MPEG2 W6 H4 F25:1'
    for c, want in (('C420', '420'), ('C420jpeg', '420'), ('C420mpeg2', '420'), ('C420paldv', '420'), ('C422', '422'), ('C444', '444'),
                    ('Cmono', 'mono'), ('', '420')):
        assert parse_y4m_header(f'{base} {c}'.strip())['chroma'] == want
    assert parse_y4m_header(base + ' I?')['interlace'] == '?'
    assert parse_y4m_header(base)['interlace'] == '?'
    assert parse_y4m_header('YUV4MPEG2 W6 H4 F0:0')['fps'] is None
    assert parse_y4m_header('YUV4MPEG2 W6 H4')['fps'] is None
    assert parse_y4m_header(base + ' Xanything=1 XCOLORRANGE=LIMITED')['size'] == (6, 4)
    for bad in ('It', 'Ib', 'Im', 'Ct', 'Cb', 'Cm', 'C411', 'C444alpha', 'C420p10', 'C422p10', 'C444p12', 'C420p16', 'Cmono16',
                'XCOLORRANGE=FULL', 'F30', 'Q1'):
        with pytest.raises(ValueError, match=bad.replace('=', '.')):
            parse_y4m_header(f'{base} {bad}')
    with pytest.raises(ValueError):
        parse_y4m_header('YUV4MPEG W6 H4')
    with pytest.raises(ValueError):
        parse_y4m_header('YUV4MPEG2 W6')
    assert y4m_header(34, 18, (30000, 1001)) == b'YUV4MPEG2 W34 H18 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n'
    assert parse_y4m_header(y4m_header(34, 18, (25, 1)))['fps'] == 25


def test_planar_frame_validation():
    rng = np.random.default_rng(4)
    w, h = 7, 5
    for chroma in ('420', '422', '444'):
        y, u, v = planes(rng, w, h, chroma)
        f = PlanarFrame(y, u, v, chroma)
        assert f.size == (w, h) and f.shape == (h, w, 3) and f.pitch == w and f.pitch_c == u.shape[1]
        assert np.array_equal(f.to_bgr(), planar_to_bgr(y, u, v, chroma))
        with pytest.raises(ValueError):                          # wrong plane shape
            PlanarFrame(y, u[:, :-1], v[:, :-1], chroma)
        with pytest.raises(ValueError):
            PlanarFrame(y, u[:-1], v[:-1], chroma)
        with pytest.raises(ValueError):                          # u and v of different pitch
            PlanarFrame(y, u, np.zeros((u.shape[0], u.shape[1] + 1), np.uint8)[:, :-1], chroma)
        with pytest.raises(ValueError):                          # negative pitch
            PlanarFrame(y[::-1], u, v, chroma)
        with pytest.raises(ValueError):                          # pitch shorter than a row (overlapping rows)
            PlanarFrame(np.lib.stride_tricks.as_strided(y, (h, w), (w - 1, 1)), u, v, chroma)
        with pytest.raises(ValueError):                          # element stride 2
            PlanarFrame(np.zeros((h, 2 * w), np.uint8)[:, ::2], u, v, chroma)
        with pytest.raises(TypeError):
            PlanarFrame(y.astype(np.int16), u, v, chroma)
        with pytest.raises(TypeError):
            PlanarFrame(y.tolist(), u, v, chroma)
        with pytest.raises(ValueError):
            PlanarFrame(y, None, None, chroma)
    with pytest.raises(ValueError):
        PlanarFrame(y, u, v, 'mono')
    with pytest.raises(ValueError):
        PlanarFrame(y, u, v, '411')
    with pytest.raises(ValueError):
        PlanarFrame(y, u, v, '444', matrix='bt2020')
    assert PlanarFrame(y, chroma='mono').pitch_c == 0
    # strided views, and one contiguous surface
    big = rng.integers(0, 256, (h, w + 9), dtype=np.uint8)
    cbig = rng.integers(0, 256, (2, 3, 11), dtype=np.uint8)
    f = PlanarFrame(big[:, 2:2 + w], cbig[0, :, :4], cbig[1, :, :4])
    assert f.pitch == w + 9 and f.pitch_c == 11
    buf = rng.integers(0, 256, frame_bytes((w, h), '420') + 5, dtype=np.uint8)
    f = PlanarFrame.from_buffer(buf, (w, h), '420', 'bt709')
    assert np.array_equal(f.y.ravel(), buf[:35]) and np.array_equal(f.u.ravel(), buf[35:47]) and np.array_equal(f.v.ravel(), buf[47:59])
    assert f.matrix == 'bt709'
    with pytest.raises(ValueError):
        PlanarFrame.from_buffer(buf[:58], (w, h), '420')
    with pytest.raises(ValueError):
        I420Image(buf[:58], (w, h))
    assert np.array_equal(I420Image(buf[:59], (w, h)).to_bgr('bt709'), f.to_bgr())


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
def clip(tmp_path_factory):
    """Five 34 x 18 frames written to a .y4m on the host path; (path, frames, what a reader must give back)."""
    d = tmp_path_factory.mktemp('y4m')
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, (18, 34, 3), dtype=np.uint8) for _ in range(5)]
    np.save(d / 'seed.npy', np.stack(frames))
    path = d / 'clip.y4m'
    video = VideoIO((34, 18), str(d / 'seed.npy'), output_uri=str(path), frame_rate=Fraction(30000, 1001))
    for f in frames:
        video.write(f)
    video.release()
    return path, frames, [planar_to_bgr(*bgr_to_planar420(f), '420') for f in frames]


def test_videoio_round_trip(clip):
    path, frames, want = clip
    data = path.read_bytes()
    head = y4m_header(34, 18, (30000, 1001))
    assert data.startswith(head) and len(data) == len(head) + 5 * (6 + frame_bytes((34, 18), '420'))
    video = VideoIO((34, 18), str(path), frame_rate=7)
    assert video.cap_fps == pytest.approx(30000 / 1001) and video.resolution == (34, 18)
    got = read_all(video)
    assert len(got) == 5
    for g, w in zip(got, want):
        assert isinstance(g, np.ndarray) and np.array_equal(g, w)
    # gpu_decode with an output that needs host pixels: ndarrays still
    video = VideoIO((34, 18), str(path), output_uri=str(path.parent / 'o.npy'), gpu_decode=True)
    assert all(isinstance(g, np.ndarray) for g in read_all(video))


def test_videoio_resizes_on_the_host(clip):
    path, frames, want = clip
    got = read_all(VideoIO((17, 9), str(path)))
    assert len(got) == 5
    for g, w in zip(got, want):
        assert np.array_equal(g, resize_bgr(w, (17, 9)))


def test_videoio_matrix_and_unknown_rate(clip, tmp_path):
    path, frames, want = clip
    data = path.read_bytes()
    head = y4m_header(34, 18, (30000, 1001))
    p = tmp_path / 'norate.y4m'
    p.write_bytes(data.replace(head, b'YUV4MPEG2 W34 H18 F0:0 C420mpeg2\n').replace(b'FRAME\n', b'FRAME Ip\n', 1))
    video = VideoIO((34, 18), str(p), frame_rate=12, yuv_matrix='bt709')
    assert video.cap_fps == 12
    got = read_all(video)
    assert len(got) == 5
    assert np.array_equal(got[0], planar_to_bgr(*bgr_to_planar420(frames[0]), '420', 'bt709'))
    with pytest.raises(ValueError):
        VideoIO((34, 18), str(p), yuv_matrix='bt2020')
    q = tmp_path / 'deep.y4m'
    q.write_bytes(b'YUV4MPEG2 W34 H18 F25:1 C420p10\n')
    with pytest.raises(ValueError, match='C420p10'):
        VideoIO((34, 18), str(q))


@pytest.mark.parametrize('cut', ['payload', 'frame_header'])
def test_truncated_last_frame_ends_the_stream(clip, tmp_path, cut):
    path, frames, want = clip
    data = path.read_bytes()
    n = 6 + frame_bytes((34, 18), '420')
    p = tmp_path / 'cut.y4m'
    p.write_bytes(data[:len(data) - (n // 2 if cut == 'payload' else n - 3)])
    got = read_all(VideoIO((34, 18), str(p)))
    assert len(got) == 4
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_y4m_output_checks(tmp_path, clip):
    path, frames, want = clip
    video = VideoIO((34, 18), str(path), output_uri=str(tmp_path / 'o.y4m'))
    y, u, v = bgr_to_planar420(frames[0])
    video.write(I420Image(np.concatenate([y.ravel(), u.ravel(), v.ravel()]), (34, 18)))
    video.write(frames[0])
    with pytest.raises(ValueError):
        video.write(frames[0][:, :32])
    with pytest.raises(TypeError):
        video.write(PlanarFrame(y, u, v))
    video.release()
    got = read_all(VideoIO((34, 18), str(tmp_path / 'o.y4m')))
    assert len(got) == 2 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[0])
