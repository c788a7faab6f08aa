"""GPU: the JPEG output path -- utils.jpeg.encode_bgr / MOT.encode_frame / VideoIO(gpu_encode=True) over csrc/jpegenc.hip.

Pillow (libjpeg-turbo) is the judge.  The reference file is `jpeg_cases.encode(rgb, '420', q, restart_marker_rows=1)`:
this Pillow takes the keyword, so files are compared byte for byte from SOS to EOI where the size is a multiple of 16,
and coefficient for coefficient (utils.jpeg.entropy_decode) everywhere.  At other sizes the encoder must equal
tests/jpegenc_ref.py on ALL blocks, dummy blocks included, and Pillow on the blocks jpegenc_ref.interior_mask names;
with libjpeg's rule for the chroma rows below the image (test_jpegenc_host.py) the files equal Pillow's there too."""
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_cases as jc
import jpegenc_ref as R
from fastmot_amd import JPEGFrame, SourceFrame, VideoIO
from fastmot_amd.utils import jpeg as J

pytestmark = pytest.mark.gpu


def bgr_of(kind, w, h):
    rgb = jc.content(kind, w, h, seed=w * 1000 + h)
    return rgb, np.ascontiguousarray(rgb[:, :, ::-1])


def pillow_file(rgb, q):
    return jc.encode(rgb, '420', q, restart_marker_rows=1)


def scan_of(data):
    return data[data.index(b'\xff\xda'):]


def pillow_rgb(data):
    with Image.open(io.BytesIO(data)) as im:
        im.load()
        return np.asarray(im.convert('RGB')), im.size


@pytest.mark.parametrize('size', [(16, 16), (48, 32), (64, 48)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_files_equal_pillows_byte_for_byte(ctx, size):
    """Every Huffman category up to DC 11 / AC 10 (checkerboard at quality 100), 0xFF stuffing (noise), EOB / ZRL (black)."""
    w, h = size
    stuffed = False
    for q in (30, 75, 95, 100):
        for kind in jc.CONTENTS:
            rgb, bgr = bgr_of(kind, w, h)
            want = pillow_file(rgb, q)
            got = J.encode_bgr(bgr, q, ctx)
            assert scan_of(got) == scan_of(want), (q, kind)
            assert got == want, (q, kind)                       # (the marker segments are Pillow's too)
            assert np.array_equal(J.entropy_decode(got)[0], J.entropy_decode(want)[0]), (q, kind)
            stuffed |= b'\xff\x00' in scan_of(got)
    assert stuffed


@pytest.mark.parametrize('size', [(1, 1), (9, 17), (31, 33), (38, 50), (70, 130), (18, 258)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_edge_sizes(ctx, size):
    w, h = size
    mask = R.interior_mask(w, h)
    for q, kind in ((30, 'noise'), (75, 'gradient'), (95, 'noise'), (100, 'checkerboard'), (75, 'white')):
        rgb, bgr = bgr_of(kind, w, h)
        got = J.encode_bgr(bgr, q, ctx)
        coef, qt = J.entropy_decode(got)
        ref, rqt = R.encode_coefficients(bgr, q)
        assert np.array_equal(qt, rqt), (q, kind)
        assert np.array_equal(coef, ref), (q, kind)
        want = pillow_file(rgb, q)
        assert np.array_equal(coef[mask], J.entropy_decode(want)[0][mask]), (q, kind)
        assert got == want, (q, kind)
        assert pillow_rgb(got)[1] == size
        assert len(got) <= J.encode_bound(w, h)


def test_several_workgroups_and_mcu_rows(ctx):
    rgb, bgr = bgr_of('noise', 272, 48)                         # 17 MCUs per row: 5 workgroups of the DCT kernel, 102 blocks per row
    got = J.encode_bgr(bgr, 90, ctx)
    assert np.array_equal(J.entropy_decode(got)[0], R.encode_coefficients(bgr, 90)[0])
    assert got == pillow_file(rgb, 90)
    rgb, bgr = bgr_of('noise', 16, 160)                         # 10 MCU rows: RST0..7, RST0
    got = J.encode_bgr(bgr, 75, ctx)
    assert got == pillow_file(rgb, 75)
    scan = got[J.parse(got).scan_offset:]
    marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    assert marks == [0xD0 + (i & 7) for i in range(9)]


def test_strided_rows_and_arguments(ctx):
    rgb, bgr = bgr_of('noise', 48, 32)
    wide = np.zeros((32, 80, 3), np.uint8)
    wide[:, :48] = bgr
    assert J.encode_bgr(wide[:, :48], 75, ctx) == pillow_file(rgb, 75)          # a pitch
    pinned = ctx.pinned_source_frames(1, (48, 32))
    pinned[0] = bgr
    assert J.encode_bgr(pinned[0], 75, ctx) == pillow_file(rgb, 75)             # page-locked pixels: no staging copy
    for q in (0, 101):
        with pytest.raises(ValueError):
            J.encode_bgr(bgr, q, ctx)
    with pytest.raises(ValueError):
        J.encode_bgr(bgr[:, :, 0], 75, ctx)
    # a larger frame after a smaller one (the buffers grow), then the smaller one again
    rgb2, bgr2 = bgr_of('textured', 640, 368)
    assert J.encode_bgr(bgr2, 75, ctx) == pillow_file(rgb2, 75)
    assert J.encode_bgr(bgr, 75, ctx) == pillow_file(rgb, 75)


def test_round_trip_through_the_gpu_decoder(ctx):
    _, bgr = bgr_of('textured', 70, 46)
    data = J.encode_bgr(bgr, 90, ctx)
    ctx.frame_configure(70, 46, 0)
    ctx.next_frame, ctx.ahead_frames, ctx.bound_frame = None, [], None
    ctx.frame_upload(JPEGFrame(data))
    assert np.array_equal(ctx.frame_read(), jc.pillow_bgr(data))
    # ... and the frame that lies there now encodes to what its host pixels encode to
    assert ctx.frame_encode_jpeg(90) == J.encode_bgr(jc.pillow_bgr(data), 90, ctx)


@pytest.mark.parametrize('kind', ['ndarray', 'jpeg', 'source'])
def test_mot_encode_frame(ctx, kind):
    """MOT.encode_frame after a step == encode_bgr of the host pixels the tracker saw; the steps' results are the same
    with and without the calls.  960 x 540: the smallest frame the MOT GPU tests use (540 is no multiple of 16)."""
    from synthetic import SyntheticVideo
    from fastmot_amd import Track
    from fastmot_amd.videoio import resize_bgr
    from test_mot_gpu import build_mot
    size = (960, 540)
    video = SyntheticVideo(size, n_ids=6, n_frames=4, seed=2)
    if kind == 'ndarray':
        frames, pixels = list(video.frames), list(video.frames)
    elif kind == 'jpeg':
        files = [jc.encode(np.ascontiguousarray(f[:, :, ::-1]), '420', 90) for f in video.frames]
        frames, pixels = [JPEGFrame(d) for d in files], [jc.pillow_bgr(d) for d in files]
    else:
        big = [np.ascontiguousarray(np.repeat(np.repeat(f, 2, 0), 2, 1)) for f in video.frames]
        big[1][::2, ::2] ^= 0x40                                 # (not every 2 x 2 mean is one of its four pixels)
        frames, pixels = [SourceFrame(b) for b in big], [resize_bgr(b, size) for b in big]
    runs = []
    for encode in (False, True):
        mot = build_mot(size, video, 1)
        Track._count = 0
        mot.reset(1 / 30.)
        if encode:
            with pytest.raises(RuntimeError):
                mot.encode_frame()
        rows = []
        for f in range(video.n_frames):
            mot.detector._frame_idx = f
            mot.step(frames[f], next_frame=frames[f + 1] if f + 1 < video.n_frames else None)
            if encode:
                got = mot.encode_frame(80)
                assert got == J.encode_bgr(pixels[f], 80, ctx), f
                assert pillow_rgb(got)[1] == size
            rows.append([(t.trk_id, tuple(t.tlbr), t.confirmed, t.active, t.age, t.hits) for t in mot.tracker.tracks.values()])
        mot.tracker._clear_tracks()
        runs.append(rows)
    assert runs[0] == runs[1]
    assert len(runs[0][-1]) >= 1


def test_videoio_gpu_encode(ctx, tmp_path):
    size = (64, 48)
    frames = [bgr_of(kind, *size) for kind in ('textured', 'noise', 'gradient')]
    for i, (rgb, _) in enumerate(frames):
        Image.fromarray(rgb).save(tmp_path / f'{i:06d}.png')
    uri = str(tmp_path / '%06d.png')
    want = [pillow_rgb(jc.encode(rgb, '420', 85))[0] for rgb, _ in frames]      # Pillow's own encode, decoded by Pillow
    ready = J.encode_bgr(frames[0][1], 40, ctx)                                  # bytes that already are a JPEG

    stream = VideoIO(size, uri, str(tmp_path / 'seq' / '%06d.jpg'), gpu_encode=True, jpeg_quality=85)
    for _, bgr in frames:
        stream.write(bgr)
    stream.write(ready)
    with pytest.raises(TypeError):
        stream.write(JPEGFrame(ready))
    with pytest.raises(ValueError):
        stream.write(b'not a jpeg')
    stream.release()
    for i in range(3):
        got, sz = pillow_rgb((tmp_path / 'seq' / f'{i:06d}.jpg').read_bytes())
        assert sz == size and np.array_equal(got, want[i]), i
    assert (tmp_path / 'seq' / '000003.jpg').read_bytes() == ready

    stream = VideoIO(size, uri, str(tmp_path / 'out.mjpeg'), gpu_encode=True, jpeg_quality=85)
    for _, bgr in frames:
        stream.write(bgr)
    stream.write(ready)
    stream.release()
    data = (tmp_path / 'out.mjpeg').read_bytes()
    parts = [b'\xff\xd8' + p for p in data.split(b'\xff\xd8')[1:]]              # (SOI cannot occur inside a file: 0xFF is stuffed)
    assert len(parts) == 4 and parts[3] == ready
    for i in range(3):
        got, sz = pillow_rgb(parts[i])
        assert sz == size and np.array_equal(got, want[i]), i
        assert parts[i] == (tmp_path / 'seq' / f'{i:06d}.jpg').read_bytes()


def test_track_stream_writes_gpu_only_frames(ctx, tmp_path):
    """gpu_decode + gpu_encode: the frames never exist as host pixels, track_stream writes MOT.encode_frame() for them."""
    from synthetic import SyntheticVideo
    from fastmot_amd import Track
    from fastmot_amd.readahead import track_stream
    from test_mot_gpu import build_mot
    size = (960, 540)
    video = SyntheticVideo(size, n_ids=6, n_frames=3, seed=4)
    (tmp_path / 'in').mkdir()
    files = [jc.encode(np.ascontiguousarray(f[:, :, ::-1]), '420', 90) for f in video.frames]
    for i, d in enumerate(files):
        (tmp_path / 'in' / f'{i + 1:06d}.jpg').write_bytes(d)
    mot = build_mot(size, video, 1)
    Track._count = 0
    mot.reset(1 / 30.)
    stream = VideoIO(size, str(tmp_path / 'in' / '%06d.jpg'), str(tmp_path / 'out' / '%06d.jpg'), buffer_size=4,
                     gpu_decode=True, gpu_encode=True, jpeg_quality=70)
    stream.start_capture()
    seen = []

    class Spy:                                       # the stream, recording what kind of frame it hands out
        resolution, gpu_encode, jpeg_quality, write = stream.resolution, stream.gpu_encode, stream.jpeg_quality, stream.write

        @staticmethod
        def read():
            seen.append(stream.read())
            return seen[-1]

    try:
        assert track_stream(Spy, mot, write_frames=True) == 3
    finally:
        stream.release()
        mot.tracker._clear_tracks()
    assert all(isinstance(f, JPEGFrame) for f in seen[:3])
    for i, d in enumerate(files):
        assert (tmp_path / 'out' / f'{i:06d}.jpg').read_bytes() == J.encode_bgr(jc.pillow_bgr(d), 70, ctx), i
