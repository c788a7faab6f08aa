"""Host side of the capture-resolution ingest path: SourceFrame, VideoIO(gpu_resize=True), the argument checks of
fm_frame_*_src that need no device, and known answers that pin videoio.resize_bgr -- the statement the GPU kernel
(csrc/resize.hip) is compared with bit for bit in test_source_frame_gpu.py."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import jpeg_cases as jc
from fastmot_amd import JPEGFrame, NV12Frame, SourceFrame, VideoIO, _lib
from fastmot_amd.utils import source as S
from fastmot_amd.videoio import resize_bgr

FM_ERR_ARG = -2


# ------------------------------------------------------------------------------------------------ resize_bgr pinned
def test_resize_bgr_known_answers_ramp_5x3_to_3x2():
    """p[y][x][c] = 10 x + 40 y + 3 c.  Horizontal 5 -> 3 (scale 5/3): d = 0: f = 1/3 -> (s, s') = (0, 1), (a0, a1) =
    (rint(1365.33), rint(682.67)) = (1365, 683); d = 1: f = 2.0 -> (2, 3), (2048, 0); d = 2: f = 3 2/3 -> (3, 4),
    (683, 1365).  Vertical 3 -> 2 (scale 1.5): d = 0: f = .25 -> (0, 1), (1536, 512); d = 1: f = 1.75 -> (1, 2), (512, 1536).
    out[0][0][0]: S0 = 0 * 1365 + 10 * 683 = 6830, S1 = 40 * 1365 + 50 * 683 = 88750; S0 >> 4 = 426, S1 >> 4 = 5546;
    (1536 * 426) >> 16 = 9, (512 * 5546) >> 16 = 43; (9 + 43 + 2) >> 2 = 13   (the real-valued answer is 13.33).
    out[0][1][0]: S0 = 20 * 2048 = 40960, S1 = 60 * 2048 = 122880; >> 4: 2560, 7680; (1536 * 2560) >> 16 = 60,
    (512 * 7680) >> 16 = 60; (60 + 60 + 2) >> 2 = 30.   The other entries likewise; a channel adds 3."""
    yy, xx, cc = np.meshgrid(np.arange(3), np.arange(5), np.arange(3), indexing='ij')
    ramp = (10 * xx + 40 * yy + 3 * cc).astype(np.uint8)
    want = [[[13, 16, 19], [30, 33, 36], [46, 49, 52]], [[73, 76, 79], [90, 93, 96], [106, 109, 112]]]
    got = resize_bgr(ramp, (3, 2))
    assert got.dtype == np.uint8 and got.tolist() == want


def test_resize_bgr_known_answers_block_4x4_to_2x2():
    """Exactly 2x in both axes: the rounded 2 x 2 mean (a + b + c + d + 2) >> 2, not the interpolation.
    Channel 0: (0 + 1 + 3 + 4 + 2) >> 2 = 2, (2 + 255 + 255 + 255 + 2) >> 2 = 192, (7 + 7 + 8 + 9 + 2) >> 2 = 8,
    (100 + 101 + 102 + 104 + 2) >> 2 = 102; channel 1 is 255 - p, channel 2 is p // 2."""
    p = np.array([[0, 1, 2, 255], [3, 4, 255, 255], [7, 7, 100, 101], [8, 9, 102, 104]], np.uint8)
    img = np.stack([p, 255 - p, p // 2], 2).astype(np.uint8)
    assert resize_bgr(img, (2, 2)).tolist() == [[[2, 253, 1], [192, 63, 96]], [[8, 247, 4], [102, 153, 51]]]
    # twice the size in ONE axis only interpolates: columns 2x, rows 4 -> 3
    assert resize_bgr(img, (2, 3)).shape == (3, 2, 3)
    assert resize_bgr(img, (4, 4)) is img


# ------------------------------------------------------------------------------------------------------ SourceFrame
def test_source_frame_kinds_and_validation():
    rng = np.random.default_rng(0)
    bgr = rng.integers(0, 256, (24, 40, 3), dtype=np.uint8)
    f = SourceFrame(bgr)
    assert f.size == (40, 24) and f.shape == (24, 40, 3) and f.frame is bgr
    d = f.describe()
    assert (d.kind, d.width, d.height, d.bgr) == (S.FM_SRC_BGR, 40, 24, bgr.ctypes.data) and f.describe() is d
    flipped = SourceFrame(bgr[:, ::-1])                # not contiguous: copied once
    assert flipped.frame.flags.c_contiguous and np.array_equal(flipped.frame, bgr[:, ::-1])

    surface = rng.integers(0, 256, (36, 48), dtype=np.uint8)
    nv = NV12Frame(surface[:24, :40], surface[24:, :40], 'bt709')
    f = SourceFrame(nv)
    d = f.describe()
    assert f.size == (40, 24) and f.shape == (24, 40, 3)
    assert (d.kind, d.width, d.height, d.pitch, d.matrix) == (S.FM_SRC_NV12, 40, 24, 48, 1)
    assert d.y == surface.ctypes.data and d.uv == surface.ctypes.data + 24 * 48

    jp = JPEGFrame(jc.encode(jc.content('noise', 37, 23), '420', 80))
    f = SourceFrame(jp)
    d = f.describe()
    assert f.size == (37, 23) and f.shape == (23, 37, 3)
    assert d.kind == S.FM_SRC_JPEG and (d.info.contents.width, d.info.contents.height) == (37, 23)
    assert d.coef == jp.coef.ctypes.data and d.qt == jp.qt.ctypes.data

    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), np.float32),
                np.zeros((0, 4, 3), np.uint8), np.zeros((4, 0, 3), np.uint8)):
        with pytest.raises(ValueError):
            SourceFrame(bad)
    with pytest.raises(ValueError):
        SourceFrame(np.zeros((1, S.MAX_DIM + 1, 3), np.uint8))
    for bad in (None, [[1, 2, 3]], f):
        with pytest.raises(TypeError):
            SourceFrame(bad)


def test_struct_matches_header():
    """fm_frame_src as a C compiler lays it out (LP64): three int32, then 8-byte aligned pointers."""
    F = S.FrameSrc
    assert [getattr(F, n).offset for n in ('kind', 'width', 'height', 'bgr', 'y', 'uv', 'pitch', 'matrix', 'info', 'coef', 'qt')] == \
        [0, 4, 8, 16, 24, 32, 40, 44, 48, 56, 64]
    assert C.sizeof(F) == 72
    header = (Path(__file__).resolve().parents[1] / 'include' / 'fastmot_hip.h').read_text()
    for name, value in (('FM_SRC_BGR', S.FM_SRC_BGR), ('FM_SRC_NV12', S.FM_SRC_NV12), ('FM_SRC_JPEG', S.FM_SRC_JPEG),
                        ('FM_SRC_MAX_DIM', S.MAX_DIM)):
        assert f'#define {name} {value}\n' in header


def test_src_entry_points_refuse_null_arguments():
    lib = _lib.load()
    d = SourceFrame(np.zeros((3, 5, 3), np.uint8)).describe()
    c = C.c_int
    for rc in (lib.fm_frame_upload_src(None, None), lib.fm_frame_upload_src(None, C.byref(d)),
               lib.fm_frame_upload_ahead_src(None, c(1), None), lib.fm_frame_upload_ahead_src(None, c(1), C.byref(d)),
               lib.fm_frame_ring_store_src(None, c(0), None), lib.fm_frame_ring_store_src(None, c(0), C.byref(d))):
        assert rc == FM_ERR_ARG
        assert b'bad argument' in lib.fm_last_error()


# ---------------------------------------------------------------------------------------------------------- VideoIO
SRC, SIZE = (40, 24), (32, 18)


def kind(f):
    if isinstance(f, SourceFrame):
        return 'src:' + type(f.frame).__name__
    return type(f).__name__


@pytest.fixture(scope='module')
def sequence(tmp_path_factory):
    """Six files '%06d.jpg': baseline JPEG 40x24, PNG 40x24, baseline JPEG 32x18 (on size), progressive JPEG 40x24,
    PNG 32x18 (on size), baseline JPEG 37x23 (4:4:4)."""
    from PIL import Image
    d = tmp_path_factory.mktemp('seq')
    rng = np.random.default_rng(5)
    spec = [('JPEG', SRC, {}), ('PNG', SRC, {}), ('JPEG', SIZE, {}), ('JPEG', SRC, {'progressive': True}), ('PNG', SIZE, {}),
            ('JPEG', (37, 23), {'subsampling': 0})]
    for i, (fmt, (w, h), kw) in enumerate(spec):
        rgb = np.kron(rng.integers(0, 256, (h // 4 + 1, w // 4 + 1, 3)).astype(np.uint8), np.ones((4, 4, 1), np.uint8))[:h, :w]
        if fmt == 'JPEG':
            kw = dict(quality=90, **kw)
        Image.fromarray(np.ascontiguousarray(rgb)).save(d / f'{i + 1:06d}.jpg', fmt, **kw)
    return str(d / '%06d.jpg')


def frames_of(stream):
    stream.start_capture()
    out = []
    try:
        while True:
            f = stream.read()
            if f is None:
                return out
            out.append(f)
    finally:
        stream.release()


def parent_frames(uri):
    """What the VideoIO without gpu_resize / gpu_decode has always returned: Pillow's decode, resize_bgr."""
    from PIL import Image
    out = []
    for i in range(6):
        with Image.open(uri % (i + 1)) as im:
            out.append(resize_bgr(np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1]), SIZE))
    return out


def host_pixels(f):
    """The frame a stage would read, computed on the host."""
    if isinstance(f, SourceFrame):
        inner = f.frame.to_bgr() if isinstance(f.frame, JPEGFrame) else f.frame
        return resize_bgr(inner, SIZE)
    return f.to_bgr() if isinstance(f, JPEGFrame) else f


def test_videoio_gpu_resize_frame_types(sequence):
    want = parent_frames(sequence)
    off = frames_of(VideoIO(SIZE, sequence, buffer_size=3))
    assert [kind(f) for f in off] == ['ndarray'] * 6
    assert all(np.array_equal(a, b) for a, b in zip(off, want))

    stream = VideoIO(SIZE, sequence, buffer_size=3, gpu_resize=True)
    assert stream.resolution == SRC and stream.do_resize and stream.cap_dt == 1 / 30
    got = frames_of(stream)
    assert [kind(f) for f in got] == ['src:ndarray', 'src:ndarray', 'ndarray', 'src:ndarray', 'ndarray', 'src:ndarray']
    assert [f.shape for f in got] == [(24, 40, 3), (24, 40, 3), (18, 32, 3), (24, 40, 3), (18, 32, 3), (23, 37, 3)]
    assert all(np.array_equal(host_pixels(a), b) for a, b in zip(got, want))

    stream = VideoIO(SIZE, sequence, buffer_size=3, gpu_resize=True, gpu_decode=True)
    assert stream.resolution == SRC and stream.do_resize
    got = frames_of(stream)
    assert [kind(f) for f in got] == ['src:JPEGFrame', 'src:ndarray', 'JPEGFrame', 'src:ndarray', 'ndarray', 'src:JPEGFrame']
    assert [f.size for f in got if not isinstance(f, np.ndarray)] == [(40, 24), (40, 24), (32, 18), (40, 24), (37, 23)]
    assert all(np.array_equal(host_pixels(a), b) for a, b in zip(got, want))

    # gpu_decode alone: as before this change -- only the on-size JPEG is decoded on the GPU, everything else is host pixels
    got = frames_of(VideoIO(SIZE, sequence, buffer_size=3, gpu_decode=True))
    assert [kind(f) for f in got] == ['ndarray', 'ndarray', 'JPEGFrame', 'ndarray', 'ndarray', 'ndarray']
    assert all(np.array_equal(host_pixels(a), b) for a, b in zip(got, want))


def test_videoio_output_keeps_host_pixels(sequence, tmp_path):
    want = parent_frames(sequence)
    for kw in ({'gpu_resize': True}, {'gpu_resize': True, 'gpu_decode': True}):
        got = frames_of(VideoIO(SIZE, sequence, str(tmp_path / 'out' / '%06d.png'), buffer_size=3, **kw))
        assert [kind(f) for f in got] == ['ndarray'] * 6
        assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_videoio_on_size_sequence_is_untouched(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(6)
    frames = [rng.integers(0, 256, (18, 32, 3), dtype=np.uint8) for _ in range(3)]
    for i, f in enumerate(frames):
        Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(tmp_path / f'{i:06d}.png')
    stream = VideoIO(SIZE, str(tmp_path / '%06d.png'), buffer_size=2, gpu_resize=True)
    assert not stream.do_resize
    got = frames_of(stream)
    assert [kind(f) for f in got] == ['ndarray'] * 3 and all(np.array_equal(a, b) for a, b in zip(got, frames))


def test_stream_cfg_reaches_videoio(sequence):
    """`"gpu_resize": true` in a configuration file's stream_cfg: app.py calls VideoIO(resize_to, uri, output, **stream_cfg)."""
    stream_cfg = {'resolution': [1920, 1080], 'frame_rate': 30, 'buffer_size': 3, 'gpu_resize': True}
    stream = VideoIO(SIZE, sequence, None, **stream_cfg)
    try:
        assert stream.gpu_resize and isinstance(stream.read(), SourceFrame)
    finally:
        stream.release()
