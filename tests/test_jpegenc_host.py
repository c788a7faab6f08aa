"""CPU: the host half of the JPEG output path and the numpy statement of the encoder's arithmetic.

tests/jpegenc_ref.py (BGR -> quantised coefficients, and their Huffman coding) is pinned against Pillow (libjpeg-turbo):
the reference file is `jpeg_cases.encode(rgb, '420', q, restart_marker_rows=1)` -- this Pillow takes the keyword, so the
comparisons are on coefficients (through utils.jpeg.entropy_decode) AND on the file's bytes.  The host helpers of csrc/jpegenc_host.hip (quality -> tables, header, segment gathering, argument
checks) need no context and no GPU.

The padded-block finding: with plain edge replication of the full-resolution planes the restatement differed from
Pillow at 38x50, 70x130 and 18x258, in the last chroma block row only.  The cause is a rule, not an artefact: libjpeg
averages the chroma first and repeats the last AVERAGED row below the image (the last pair of pixel rows, not the last
row twice), which only shows at even heights.  The restatement and the kernel follow that rule, and with it every
coefficient and every file byte equals Pillow's at every size here; the comparison on the blocks whose samples all
exist (jpegenc_ref.interior_mask), which the padding cannot touch, is kept beside it.

A reinterpretation of the issue, stated as one: its condition that the blocks left out of that comparison "stay under
half of an image's blocks" cannot hold as worded.  Counted over the MCU-padded grid with "all source pixels inside the
image", 38x50 leaves out exactly half (36 of 72) and 31x33 more than half (20 of 36).  Here the blocks are counted over
those that hold at least one image sample, the chroma part of the mask takes the blocks whose chroma samples all exist
(a superset of the issue's), and 9x17 and 18x258 -- the latter added by this file -- are exempt because images narrower
than 32 pixels cannot have half of their blocks interior.  The check only guards the mask against being vacuous: the
same test asserts equality with Pillow on EVERY block, padded and dummy ones included, which is more than was asked."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_cases as jc
import jpegenc_ref as R
from fastmot_amd import VideoIO, _lib
from fastmot_amd.utils import jpeg as J

FM_ERR_ARG = -2
MULTIPLES = [(16, 16), (64, 48), (48, 32)]
OTHERS = [(1, 1), (9, 17), (31, 33), (38, 50), (70, 130), (18, 258)]
QUALITIES = [30, 75, 95, 100]


def bgr_of(kind, w, h):
    rgb = jc.content(kind, w, h, seed=w * 1000 + h)
    return rgb, np.ascontiguousarray(rgb[:, :, ::-1])


def pillow_file(rgb, q):
    return jc.encode(rgb, '420', q, restart_marker_rows=1)


@pytest.mark.parametrize('size', MULTIPLES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_restatement_equals_pillow_on_multiples_of_16(size):
    w, h = size
    for q in QUALITIES:
        for kind in jc.CONTENTS:
            rgb, bgr = bgr_of(kind, w, h)
            data = pillow_file(rgb, q)
            coef, qt = J.entropy_decode(data)
            mine, mqt = R.encode_coefficients(bgr, q)
            assert np.array_equal(mqt, qt), (q, kind)
            assert np.array_equal(mine, coef), (q, kind)
            # ... and coded with the encoder's own header and segment gathering, the same FILE
            head = J.encode_header(w, h, q)
            assert J.encode_assemble(w, h, q, R.entropy_segments(mine, J.parse(head))) == data, (q, kind)


@pytest.mark.parametrize('size', OTHERS, ids=lambda s: f'{s[0]}x{s[1]}')
def test_restatement_equals_pillow_on_interior_blocks(size):
    w, h = size
    mask = R.interior_mask(w, h)
    # blocks that hold at least one image sample, per component (luma 8 x 8, chroma 16 x 16 pixels each)
    own = -(-w // 8) * -(-h // 8) + 2 * (-(-w // 16) * -(-h // 16))         # (ceil(ceil(w / 2) / 8) = ceil(w / 16))
    left_out = own - int(mask.sum()) // 64
    if size == (1, 1):
        assert not mask.any()                       # every block contains padding
    elif size not in ((9, 17), (18, 258)):                           # (too narrow for half of their blocks to be interior)
        assert 2 * left_out < own, (left_out, own)
    for q in QUALITIES:
        for kind in jc.CONTENTS:
            rgb, bgr = bgr_of(kind, w, h)
            data = pillow_file(rgb, q)
            coef, qt = J.entropy_decode(data)
            mine, mqt = R.encode_coefficients(bgr, q)
            assert np.array_equal(mqt, qt), (q, kind)
            assert np.array_equal(mine[mask], coef[mask]), (q, kind)
            assert np.array_equal(mine, coef), (q, kind)                 # padded and dummy blocks too
            # the file made of the restatement's coefficients: Pillow's, and one Pillow opens at the right size
            out = J.encode_assemble(w, h, q, R.entropy_segments(mine, J.parse(J.encode_header(w, h, q))))
            assert out == data, (q, kind)
            with Image.open(io.BytesIO(out)) as im:
                im.load()
                assert im.size == size
            assert np.array_equal(J.entropy_decode(out)[0], mine), (q, kind)


@pytest.mark.parametrize('q', [1, 10, 30, 50, 75, 95, 100])
def test_quality_tables_equal_pillows(q):
    with Image.open(io.BytesIO(jc.encode(jc.content('gradient', 16, 16), '420', q))) as im:
        want = im.quantization                      # table id -> 64 values (this Pillow: in zig-zag order)
    luma, chroma = J.encode_tables(q)
    hd = J.parse(J.encode_header(16, 16, q))
    assert np.array_equal(hd.qt[0], luma) and np.array_equal(hd.qt[1], chroma)
    assert np.array_equal(luma, R.quality_tables(q)[0]) and np.array_equal(chroma, R.quality_tables(q)[1])
    pillow_hd = J.parse(jc.encode(jc.content('gradient', 16, 16), '420', q))
    assert np.array_equal(pillow_hd.qt[0], luma) and np.array_equal(pillow_hd.qt[1], chroma)
    assert sorted(want[0]) == sorted(int(v) for v in luma) and sorted(want[1]) == sorted(int(v) for v in chroma)


def test_header_parses_and_equals_pillows():
    for (w, h), q in (((16, 16), 75), ((1, 1), 1), ((1920, 1080), 90), ((16384, 16384), 100)):
        head = J.encode_header(w, h, q)
        hd = J.parse(head)
        assert (hd.width, hd.height, hd.ncomp) == (w, h, 3)
        assert (hd.hsamp[0], hd.vsamp[0], hd.hsamp[1], hd.vsamp[1]) == (2, 2, 1, 1)
        assert hd.restart_interval == hd.mcus_x == -(-w // 16)
        assert hd.scan_offset == len(head)
        assert hd.tq == [0, 1, 1] and hd.td == [0, 1, 1] and hd.ta == [0, 1, 1]
    data = pillow_file(jc.content('noise', 48, 32), 75)
    assert J.encode_header(48, 32, 75) == data[:J.parse(data).scan_offset]      # marker order and contents: Pillow's


def test_argument_checks_and_capacity():
    lib = _lib.load()
    out = np.zeros(4096, np.uint8)
    n = C.c_size_t(0)
    qt = np.zeros(128, np.uint16)
    for q in (0, 101, -3):
        assert lib.fm_jpeg_encode_tables(C.c_int(q), _lib._ptr(qt)) == FM_ERR_ARG
        assert lib.fm_jpeg_encode_header(C.c_int(16), C.c_int(16), C.c_int(q), _lib._ptr(out), C.c_size_t(out.size), C.byref(n)) == FM_ERR_ARG
    for w, h in ((0, 16), (16, 0), (16385, 16), (16, 16385)):
        assert lib.fm_jpeg_encode_header(C.c_int(w), C.c_int(h), C.c_int(75), _lib._ptr(out), C.c_size_t(out.size), C.byref(n)) == FM_ERR_ARG
        assert J.encode_bound(w, h) == 0
    # a capacity that is too small: an error code, the needed length, and nothing written behind the capacity
    full = J.encode_header(48, 32, 75)
    for cap in (0, 1, 100, len(full) - 1):
        buf = np.full(len(full) + 64, 0x5A, np.uint8)
        rc = lib.fm_jpeg_encode_header(C.c_int(48), C.c_int(32), C.c_int(75), _lib._ptr(buf), C.c_size_t(cap), C.byref(n))
        assert rc == FM_ERR_ARG and n.value == len(full) and lib.fm_last_error()
        assert (buf[cap:] == 0x5A).all()
    rgb, bgr = bgr_of('noise', 48, 32)
    coef, _ = R.encode_coefficients(bgr, 75)
    segs = R.entropy_segments(coef, J.parse(full))
    whole = J.encode_assemble(48, 32, 75, segs)
    assert whole == pillow_file(rgb, 75) and len(whole) <= J.encode_bound(48, 32)
    for cap in (0, len(full), len(whole) - 1):
        with pytest.raises(_lib.FastMOTHipError):
            J.encode_assemble(48, 32, 75, segs, capacity=cap)
    # segment lengths that do not fit the segment buffer are refused before anything is read
    lens = np.array([1 << 20, 5], np.uint32)
    data = np.zeros(64, np.uint8)
    rc = lib.fm_jpeg_encode_assemble(C.c_int(48), C.c_int(32), C.c_int(75), _lib._ptr(lens), _lib._ptr(data), C.c_size_t(64), _lib._ptr(out),
                                     C.c_size_t(out.size), C.byref(n))
    assert rc == FM_ERR_ARG
    # the bound holds for the worst content the tests have, at the quality that codes the most bits
    for size in ((16, 16), (31, 33)):
        _, bgr = bgr_of('noise', *size)
        coef, _ = R.encode_coefficients(bgr, 100)
        f = J.encode_assemble(*size, 100, R.entropy_segments(coef, J.parse(J.encode_header(*size, 100))))
        assert len(f) <= J.encode_bound(*size)


def test_rst_markers_cycle():
    w, h = 16, 160
    rgb, bgr = bgr_of('noise', w, h)
    coef, _ = R.encode_coefficients(bgr, 75)
    out = J.encode_assemble(w, h, 75, R.entropy_segments(coef, J.parse(J.encode_header(w, h, 75))))
    assert out == pillow_file(rgb, 75)
    scan = out[J.parse(out).scan_offset:]
    marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    assert marks == [0xD0 + (i & 7) for i in range(9)]


def sequence(tmp_path, n=3, size=(32, 16)):
    for i in range(n):
        Image.fromarray(jc.content('noise', *size, seed=i)).save(tmp_path / f'{i:06d}.png')
    return str(tmp_path / '%06d.png')


def test_videoio_without_gpu_encode_is_unchanged(tmp_path):
    uri = sequence(tmp_path)
    frame = np.ascontiguousarray(jc.content('noise', 32, 16, seed=9)[:, :, ::-1])
    # .mjpeg and every other video URI: refused as before
    for name in ('out.mjpeg', 'out.mp4'):
        with pytest.raises(NotImplementedError):
            VideoIO((32, 16), uri, str(tmp_path / 'o' / name))
    with pytest.raises(NotImplementedError):
        VideoIO((32, 16), uri, str(tmp_path / 'o' / 'out.mp4'), gpu_encode=True)      # the flag adds .mjpeg only
    # .png, .npy and the Pillow .jpg writer: as before, with the flag on as well for .png / .npy (no GPU is touched)
    for kw in ({}, {'gpu_encode': True, 'jpeg_quality': 90}):
        s = VideoIO((32, 16), uri, str(tmp_path / 'p' / '%06d.png'), **kw)
        s.write(frame)
        s.release()
        with Image.open(tmp_path / 'p' / '000000.png') as im:
            assert np.array_equal(np.asarray(im)[:, :, ::-1], frame)
        s = VideoIO((32, 16), uri, str(tmp_path / 'n' / 'out.npy'), **kw)
        s.write(frame)
        s.release()
        assert np.array_equal(np.load(tmp_path / 'n' / 'out.npy')[0], frame)
    s = VideoIO((32, 16), uri, str(tmp_path / 'j' / '%06d.jpg'))
    s.write(frame)
    s.release()
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame[:, :, ::-1])).save(buf, 'JPEG')
    assert (tmp_path / 'j' / '000000.jpg').read_bytes() == buf.getvalue()
    with pytest.raises(ValueError):
        VideoIO((32, 16), uri, str(tmp_path / 'j' / '%06d.jpg'), gpu_encode=True, jpeg_quality=0)
    # stream_cfg of a configuration file reaches the flag like gpu_decode
    s = VideoIO((32, 16), uri, None, **{'gpu_encode': True, 'jpeg_quality': 60})
    assert s.gpu_encode and s.jpeg_quality == 60
    s.release()
