"""CPU: the host half of the object-crop encoder (fm_jpeg_encode_regions_plan / _bound / _assemble of
csrc/jpegenc_host.hip), the region rule both redaction and MOT.encode_objects use (utils.redact.region_rect), the numpy
reference of tests/objenc_cases.py, and utils.snapshots.SnapshotWriter.  No GPU: the device half is tests/test_objenc_gpu.py."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import jpeg_cases as jc
import objenc_cases as oc
from fastmot_amd import _lib
from fastmot_amd.utils import jpeg as J
from fastmot_amd.utils import redact as RD
from fastmot_amd.utils.snapshots import SnapshotWriter

FM_ERR_ARG = -2


def old_region_of(tlbr, cfg, size):
    """utils.redact._region_of's corners as they were before region_rect was split off, restated."""
    import math
    x0, y0, x1, y1 = (float(v) for v in tlbr)
    w, h = x1 - x0 + 1, y1 - y0 + 1
    if not (w > 0 and h > 0):
        return None
    fl, ft, fr, fb = cfg.fractions
    l, t, r, b = x0 + fl * w, y0 + ft * h, x0 + fr * w, y0 + fb * h
    mx, my = cfg.margin * (r - l), cfg.margin * (b - t)
    corners = []
    for lo, hi, extent in ((l - mx, r + mx, size[0]), (t - my, b + my, size[1])):
        slack = (RD.FM_SRC_MAX_DIM - extent) // 2
        corners.append((int(min(max(math.floor(lo), -slack), extent - 1 + slack)),
                        int(min(max(math.ceil(hi) - 1, -slack), extent - 1 + slack))))
    (rx0, rx1), (ry0, ry1) = corners
    return None if rx1 < rx0 or ry1 < ry0 else (rx0, ry0, rx1, ry1)


def test_region_rect_is_the_redaction_rule():
    rng = np.random.default_rng(5)
    size = (640, 360)
    cfgs = [RD.Redact(), RD.Redact(part='head', margin=0.25), RD.Redact(part=(0.1, 0.2, 0.9, 0.6), margin=0)]
    seen_none = 0
    for k in range(400):
        c = rng.uniform(-200, 900, 2)
        wh = rng.uniform(-5, 300, 2) if k % 10 else np.array([np.nan, 4.])
        tlbr = (c[0], c[1], c[0] + wh[0], c[1] + wh[1])
        for cfg in cfgs:
            want = old_region_of(tlbr, cfg, size)
            got = RD.region_rect(tlbr, cfg.fractions, cfg.margin, size)
            assert got == want, (tlbr, cfg.part)
            reg = RD._region_of(tlbr, cfg, size)
            assert (reg is None) == (want is None) and (reg is None or reg[:4] == want)
            seen_none += want is None
            clip = RD.clip_rect(got, size)
            assert clip == (None if want is None else oc.clip(want, size))
            if clip is not None:
                assert 0 <= clip[0] <= clip[2] < size[0] and 0 <= clip[1] <= clip[3] < size[1]
    assert seen_none
    # boxes off the frame on every side yield no image; one that touches it by a pixel does
    for tlbr in ((-50, 10, -1.5, 60), (640, 10, 700, 60), (10, -80, 60, -2), (10, 360, 60, 400), (2000, 2000, 2100, 2100)):
        assert RD.clip_rect(RD.region_rect(tlbr, RD.PARTS['box'], 0., size), size) is None, tlbr
    assert RD.clip_rect(RD.region_rect((-50, -50, 0, 0), RD.PARTS['box'], 0., size), size) == (0, 0, 0, 0)
    assert RD.clip_rect(RD.region_rect((100, 100, 199, 299), RD.PARTS['head'], 0., size), size) == (125, 100, 174, 149)
    assert RD.clip_rect(None, size) is None
    with pytest.raises(ValueError):
        RD.part_fractions('torso')
    with pytest.raises(ValueError):
        RD.part_fractions((0.5, 0, 0.5, 1))
    assert RD.part_fractions('head') == RD.PARTS['head']


def row_bytes(mx):
    return ((mx * 6 * 208 + 1 + 15) & ~15) + 16          # fm_jpegenc_row_bytes: the worst case + the pad byte, to 16, + 16


@pytest.mark.parametrize('shrink', [1, 2, 4])
def test_plan(shrink):
    rects = oc.clipped(oc.RECTS, oc.FRAME)
    plans, totals = _lib.encode_regions_plan(rects, shrink)
    assert len(plans) == 10
    mcu = row = raw = bound = 0
    for p, (x0, y0, x1, y1) in zip(plans, rects):
        w, h = -(-(x1 - x0 + 1) // shrink), -(-(y1 - y0 + 1) // shrink)
        mx, my = -(-w // 16), -(-h // 16)
        assert (p['width'], p['height'], p['mcus_x'], p['mcus_y']) == (w, h, mx, my)
        assert (p['first_mcu'], p['first_block'], p['first_row'], p['raw_offset']) == (mcu, 6 * mcu, row, raw)
        assert p['bound'] == J.encode_bound(w, h) and p['raw_offset'] % 16 == 0 and p['reserved'] == 0
        mcu, row, raw, bound = mcu + mx * my, row + my, raw + row_bytes(mx) * my, bound + J.encode_bound(w, h)
    assert (totals['mcus'], totals['blocks'], totals['rows'], totals['raw_bytes'], totals['bound']) == (mcu, 6 * mcu, row, raw, bound)
    lib = _lib.load()
    assert lib.fm_jpeg_encode_regions_bound(_lib._ptr(rects), C.c_int(len(rects)), C.c_int(shrink)) == bound
    if shrink == 1:
        assert [int(p['mcus_x'] * p['mcus_y']) for p in plans] == [1, 1, 6, 1, 1, 1, 60, 10, 6, 6]
    # n == 0: an empty plan
    plans, totals = _lib.encode_regions_plan(np.zeros((0, 4), np.int32), shrink)
    assert len(plans) == 0 and totals['mcus'] == 0 and totals['rows'] == 0 and totals['bound'] == 0


def plan_error(rects, n=None, shrink=1):
    lib = _lib.load()
    arr = np.ascontiguousarray(rects, np.int32).reshape(-1, 4)
    totals = np.zeros(1, _lib.CROP_TOTALS_DTYPE)
    n = len(arr) if n is None else n
    rc = lib.fm_jpeg_encode_regions_plan(_lib._ptr(arr) if len(arr) else None, C.c_int(n), C.c_int(shrink), None, _lib._ptr(totals))
    assert rc == FM_ERR_ARG
    assert lib.fm_jpeg_encode_regions_bound(_lib._ptr(arr) if len(arr) else None, C.c_int(n), C.c_int(shrink)) == 0
    return lib.fm_last_error().decode()


def test_plan_refusals_name_the_limit():
    ok = [(0, 0, 15, 15)]
    assert 'negative count' in plan_error(ok, n=-1)
    for s in (0, 3, 8, -1):
        assert 'shrink' in plan_error(ok, shrink=s)
    for bad in ((5, 0, 4, 10), (0, 9, 10, 8), (-1, 0, 10, 10), (0, -1, 10, 10), (0, 0, 16384, 10)):
        assert 'rectangle 1' in plan_error(ok + [bad]), bad
    assert 'FM_OBJENC_MAX_REGIONS' in plan_error(ok * (_lib.FM_OBJENC_MAX_REGIONS + 1))
    _lib.encode_regions_plan(ok * _lib.FM_OBJENC_MAX_REGIONS)                        # the limit itself is taken
    big = (0, 0, 16 * 128 - 1, 16 * 64 - 1)                                         # 8192 MCUs
    plans, totals = _lib.encode_regions_plan([big, big])
    assert totals['mcus'] == _lib.FM_OBJENC_MAX_MCUS
    assert 'FM_OBJENC_MAX_MCUS' in plan_error([big, big, (0, 0, 0, 0)])
    _lib.encode_regions_plan([big, big, (0, 0, 0, 0)], shrink=2)                    # (a quarter of the MCUs)
    with pytest.raises(_lib.FastMOTHipError, match='FM_OBJENC_MAX_MCUS'):
        _lib.encode_regions_plan([big, big, big])
    with pytest.raises(ValueError):
        _lib.encode_regions_plan([(0.5, 0, 3, 3)])


def test_shrink_two_is_resize_bgr_on_an_even_crop():
    from fastmot_amd.videoio import resize_bgr
    bgr = oc.frame_bgr('noise')
    crop = bgr[10:70, 4:52]                                                          # 48 x 60
    assert np.array_equal(oc.shrink_mean(crop, 2), resize_bgr(np.ascontiguousarray(crop), (24, 30)))
    # an odd crop: the last column / row are means of fewer pixels, and the size rounds up
    odd = oc.shrink_mean(bgr[0:5, 0:7], 4)
    assert odd.shape == (2, 2, 3)
    assert np.array_equal(odd[1, 1], (bgr[4:5, 4:7].astype(np.int64).sum((0, 1)) + 1) // 3)
    assert np.array_equal(odd[0, 0], (bgr[0:4, 0:4].astype(np.int64).sum((0, 1)) + 8) // 16)
    assert oc.shrink_mean(bgr[:1, :1], 4).shape == (1, 1, 3)


def test_the_reference_has_the_properties_the_gpu_tests_lean_on():
    stuffed = 0
    for q in oc.QUALITIES:
        refs = oc.references('noise', q)
        assert len(refs) == 10 and refs[oc.THIRD] == refs[oc.DUPLICATE]
        assert oc.rst_markers(refs[oc.TALL]) == [0xD0 + (i & 7) for i in range(9)]               # RST0..7, RST0
        assert refs[oc.WHOLE] == jc.encode(jc.content('noise', *oc.FRAME, seed=1), '420', q, restart_marker_rows=1)
        stuffed += sum(b'\xff\x00' in r[J.parse(r).scan_offset:] for r in refs)
    assert stuffed >= 1
    hd = J.parse(oc.references('checkerboard', 100)[oc.WHOLE])
    assert (hd.width, hd.height) == oc.FRAME


def stuffed_segments(data):
    """The byte-stuffed restart segments of a file's scan (split at RSTn, EOI dropped)."""
    scan = data[J.parse(data).scan_offset:-2]
    segs, cur, i = [], bytearray(), 0
    while i < len(scan):
        if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7:
            segs.append(bytes(cur))
            cur = bytearray()
            i += 2
        else:
            cur.append(scan[i])
            i += 1
    segs.append(bytes(cur))
    return segs


@pytest.mark.parametrize('shrink', [1, 2])
def test_assemble_rebuilds_every_file(shrink):
    """The segments of all reference files, concatenated in row order as the device leaves them -> the files, each with
    its own header and its restart markers from RST0."""
    refs = oc.references('noise', 75, shrink)
    plans, totals = _lib.encode_regions_plan(oc.clipped(oc.RECTS, oc.FRAME), shrink)
    segs = [s for r in refs for s in stuffed_segments(r)]
    assert len(segs) == totals['rows']
    assert tuple(_lib.encode_regions_assemble(plans, 75, segs)) == refs
    assert sum(len(r) for r in refs) <= totals['bound']
    with pytest.raises(_lib.FastMOTHipError, match='the output holds'):
        _lib.encode_regions_assemble(plans, 75, segs, capacity=sum(len(r) for r in refs) - 1)
    for q in (0, 101):
        with pytest.raises(_lib.FastMOTHipError):
            _lib.encode_regions_assemble(plans, q, segs)


def test_assemble_refuses_inconsistent_segment_lengths():
    lib = _lib.load()
    plans, totals = _lib.encode_regions_plan([(0, 0, 15, 31), (0, 0, 15, 15)])            # rows: 2 + 1
    out = np.full(8192, 0x5A, np.uint8)
    offsets = np.zeros(3, np.uintp)
    data = np.zeros(64, np.uint8)

    def call(lens, segs_bytes=64, p=plans):
        lens = np.array(lens, np.uint32)
        return lib.fm_jpeg_encode_regions_assemble(_lib._ptr(p), C.c_int(len(p)), C.c_int(75), _lib._ptr(lens), _lib._ptr(data),
                                                   C.c_size_t(segs_bytes), _lib._ptr(out), C.c_size_t(out.size), _lib._ptr(offsets))
    assert call([5, 5, 5]) == 0
    assert offsets[0] == 0 and offsets[2] < out.size
    out[:] = 0x5A
    for lens in ([1 << 20, 5, 5], [5, 5, 1 << 20], [16, 16, 33], [0xFFFFFFFF, 0, 0], [48, 16, 1]):
        assert call(lens) == FM_ERR_ARG, lens
        assert 'segment lengths' in lib.fm_last_error().decode()
        assert (out == 0x5A).all()                                                        # refused before anything is written
    assert call([16, 16, 16], segs_bytes=47) == FM_ERR_ARG
    assert call([16, 16, 16], segs_bytes=48) == 0
    # plans whose rows are not numbered without gaps are refused as well
    broken = plans.copy()
    broken['first_row'][1] = 3
    assert call([5, 5, 5], p=broken) == FM_ERR_ARG


class FakeMot:
    """What SnapshotWriter needs of a MOT: frame_count and encode_objects()."""

    def __init__(self, script):
        self.script, self.frame_count, self.options = script, 0, []

    def step(self):
        self.frame_count += 1

    def encode_objects(self, **options):
        self.options.append(options)
        return [SimpleNamespace(trk_id=t, label=1, rect=rect, size=(rect[2] - rect[0] + 1, rect[3] - rect[1] + 1),
                                data=f'{t}@{self.frame_count}'.encode())
                for t, rect in self.script[self.frame_count - 1]]


SCRIPT = [[(1, (0, 0, 9, 9))],
          [(1, (0, 0, 19, 9)), (2, (5, 5, 6, 6))],
          [(1, (0, 0, 9, 19)), (2, (5, 5, 5, 5))],           # track 1: the same area as before -> the earlier one stays
          [(2, (0, 0, 30, 30)), (7, (1, 1, 2, 2))]]


def run_writer(tmp_path, **kw):
    mot = FakeMot(SCRIPT)
    writer = SnapshotWriter(tmp_path / 'snaps', **kw)
    for _ in SCRIPT:
        mot.step()
        writer.update(mot)
    before_close = sorted(str(p.relative_to(tmp_path / 'snaps')) for p in (tmp_path / 'snaps').rglob('*.jpg'))
    writer.close()
    writer.close()
    files = {str(p.relative_to(tmp_path / 'snaps')): p.read_bytes() for p in (tmp_path / 'snaps').rglob('*.jpg')}
    return mot, before_close, files


def test_snapshot_writer_all(tmp_path):
    mot, before, files = run_writer(tmp_path, policy='all', quality=60, part='head')
    assert files == {'000001/000001.jpg': b'1@1', '000001/000002.jpg': b'1@2', '000002/000002.jpg': b'2@2', '000001/000003.jpg': b'1@3',
                     '000002/000003.jpg': b'2@3', '000002/000004.jpg': b'2@4', '000007/000004.jpg': b'7@4'}
    assert before == sorted(files) and mot.options == [dict(quality=60, part='head')] * 4


def test_snapshot_writer_all_every_second_frame(tmp_path):
    mot, _, files = run_writer(tmp_path, policy='all', every=2)
    assert sorted(files) == ['000001/000001.jpg', '000001/000003.jpg', '000002/000003.jpg'] and len(mot.options) == 2


def test_snapshot_writer_first(tmp_path):
    _, before, files = run_writer(tmp_path, policy='first')
    assert files == {'000001.jpg': b'1@1', '000002.jpg': b'2@2', '000007.jpg': b'7@4'} and before == sorted(files)


def test_snapshot_writer_largest(tmp_path):
    _, before, files = run_writer(tmp_path, policy='largest')
    assert before == []                                                                   # kept in memory until close()
    assert files == {'000001.jpg': b'1@2', '000002.jpg': b'2@4', '000007.jpg': b'7@4'}


def test_snapshot_writer_arguments(tmp_path):
    with pytest.raises(ValueError):
        SnapshotWriter(tmp_path, policy='best')
    with pytest.raises(ValueError):
        SnapshotWriter(tmp_path, every=0)
    writer = SnapshotWriter(tmp_path / 'a' / 'b')
    writer.close()
    with pytest.raises(RuntimeError):
        writer.update(FakeMot(SCRIPT))


def test_track_stream_drives_the_writer():
    from fastmot_amd.readahead import track_stream
    calls = []

    class Stream:
        frames = [object(), object(), None]
        resolution = (4, 4)

        @classmethod
        def read(cls):
            return cls.frames.pop(0) if cls.frames else None

    class Mot:
        frame_count = 0

        def step(self, frame, next_frame=None):
            self.frame_count += 1

    class Snap:
        def update(self, mot):
            calls.append(mot.frame_count)

        def close(self):
            calls.append('closed')

    assert track_stream(Stream, Mot(), snapshots=Snap()) == 2
    assert calls == [1, 2, 'closed']
