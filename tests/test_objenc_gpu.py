"""GPU: object crops as JPEG files -- ctx.frame_encode_regions / MOT.encode_objects / SnapshotWriter over the table form of
the encoder's kernels (csrc/jpegenc.hip).  Pillow is the judge (tests/objenc_cases.py): every file is compared
byte for byte, and coefficient for coefficient through utils.jpeg.entropy_decode."""
import ctypes as C

import numpy as np
import pytest

import jpeg_cases as jc
import objenc_cases as oc
from fastmot_amd import _lib
from fastmot_amd.utils import jpeg as J

pytestmark = pytest.mark.gpu
FM_ERR_ARG = -2


def upload(ctx, bgr):
    h, w = bgr.shape[:2]
    ctx.frame_configure(w, h, 0)
    ctx.next_frame, ctx.ahead_frames, ctx.bound_frame = None, [], None
    ctx.frame_upload(np.ascontiguousarray(bgr))


def check_files(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(J.entropy_decode(g)[0], J.entropy_decode(w)[0]), (what, i)
        assert g == w, (what, i)


@pytest.mark.parametrize('kind', ['noise', 'checkerboard'])
def test_rect_list(ctx, kind):
    """The list of objenc_cases.RECTS in one call: 1 x 1, an odd byte offset, padding that must be the crop's own, a rect
    flush with the corner, clipped ones, the whole frame, ten MCU rows, a duplicate, one row of six MCUs."""
    bgr = oc.frame_bgr(kind)
    upload(ctx, bgr)
    rects = oc.clipped(oc.RECTS, oc.FRAME)
    stuffed = 0
    for q in oc.QUALITIES if kind == 'noise' else (100,):         # checkerboard at 100: DC 11 / AC 10 categories
        got = ctx.frame_encode_regions(rects, q)
        check_files(got, oc.references(kind, q), (kind, q))
        assert got[oc.WHOLE] == ctx.frame_encode_jpeg(q)           # a table of one image == the whole-frame path
        assert got[oc.THIRD] == got[oc.DUPLICATE]
        assert oc.rst_markers(got[oc.TALL]) == [0xD0 + (i & 7) for i in range(9)]
        assert oc.rst_markers(got[oc.WHOLE])[:1] == [0xD0]         # ... and restarts at RST0 in the file behind it
        stuffed += sum(b'\xff\x00' in g[J.parse(g).scan_offset:] for g in got)
    assert stuffed >= 1 or kind != 'noise'


@pytest.mark.parametrize('shrink', [2, 4])
def test_shrink(ctx, shrink):
    bgr = oc.frame_bgr('noise')
    upload(ctx, bgr)
    rects = oc.clipped(oc.RECTS, oc.FRAME)
    for q in (30, 95):
        got = ctx.frame_encode_regions(rects, q, shrink=shrink)
        check_files(got, oc.references('noise', q, shrink), (shrink, q))
        for g, r in zip(got, rects):
            hd = J.parse(g)
            assert (hd.width, hd.height) == (-(-(r[2] - r[0] + 1) // shrink), -(-(r[3] - r[1] + 1) // shrink))


def test_a_row_wider_than_the_scan_workgroup(ctx):
    """720 x 48, rect (8, 8, 711, 39): 44 MCUs, 264 blocks per row (per > 1 in the scan kernel), beside a 1-MCU image."""
    bgr = np.ascontiguousarray(jc.content('noise', 720, 48, seed=3)[:, :, ::-1])
    upload(ctx, bgr)
    rects = np.array([(8, 8, 711, 39), (700, 40, 700, 40), (0, 0, 719, 47)], np.int32)
    for q in (75, 100):
        check_files(ctx.frame_encode_regions(rects, q), [oc.reference(bgr, r, q) for r in rects], q)
    assert J.parse(ctx.frame_encode_regions(rects[:1], 75)[0]).mcus_x == 44


def test_none_and_one_and_refusals(ctx):
    bgr = oc.frame_bgr('noise')
    upload(ctx, bgr)
    lib = ctx.lib
    assert ctx.frame_encode_regions(np.zeros((0, 4), np.int32)) == []
    out = np.zeros(1 << 16, np.uint8)

    def call(rects, n=None, shrink=1, quality=75, which=0, cap=None, o=out):
        arr = np.ascontiguousarray(rects, np.int32).reshape(-1, 4)
        n = len(arr) if n is None else n
        offs = np.full(max(n, 0) + 1, 77, np.uintp)
        rc = lib.fm_frame_encode_regions(ctx.handle, C.c_int(which), _lib._ptr(arr) if len(arr) else None, C.c_int(n), C.c_int(shrink),
                                         C.c_int(quality), _lib._ptr(o), C.c_size_t(out.size if cap is None else cap), _lib._ptr(offs))
        return rc, offs, lib.fm_last_error().decode()

    rc, offs, _ = call([])                                          # n == 0 succeeds with offsets[0] == 0
    assert rc == 0 and offs[0] == 0
    one = [(5, 3, 20, 18)]
    rc, offs, _ = call(one)                                         # n == 1
    assert rc == 0 and offs[0] == 0 and out[:offs[1]].tobytes() == oc.reference(bgr, one[0], 75)
    assert ctx.frame_encode_regions(one, 75) == [oc.reference(bgr, one[0], 75)]
    bound = lib.fm_jpeg_encode_regions_bound(_lib._ptr(np.array(one, np.int32)), C.c_int(1), C.c_int(1))
    for args, word in ((dict(rects=one, n=-1), 'negative count'), (dict(rects=one, shrink=3), 'shrink'),
                       (dict(rects=one, quality=0), 'quality'), (dict(rects=one, quality=101), 'quality'),
                       (dict(rects=[(0, 0, 96, 10)]), 'outside the 96x160 frame'), (dict(rects=[(0, 0, 10, 160)]), 'outside the 96x160 frame'),
                       (dict(rects=[(9, 0, 8, 10)]), 'rectangle 0'), (dict(rects=[(-1, 0, 8, 10)]), 'rectangle 0'),
                       (dict(rects=one * (_lib.FM_OBJENC_MAX_REGIONS + 1)), 'FM_OBJENC_MAX_REGIONS'),
                       (dict(rects=one, cap=bound - 1), 'below the bound'), (dict(rects=one, which=2), 'bad argument'),
                       (dict(rects=one, which=1), 'no overlay picture')):
        rc, _, msg = call(**args)
        assert rc == FM_ERR_ARG and word in msg, (args.keys(), msg)
    rc, _, _ = call(one, cap=bound)
    assert rc == 0
    for bad in (dict(quality=0), dict(shrink=3)):
        with pytest.raises(ValueError):
            ctx.frame_encode_regions(one, **bad)
    with pytest.raises(_lib.FastMOTHipError, match='outside the 96x160 frame'):
        ctx.frame_encode_regions([(0, 0, 96, 10)])
    assert ctx.frame_encode_regions(one, 75) == [oc.reference(bgr, one[0], 75)]      # (and the encoder still works)
    # the overlay buffer as the source: a rectangle painted over the crop's corner shows in the file
    cmds = np.zeros(1, _lib.OVERLAY_CMD_DTYPE)
    cmds[0] = (_lib.OVL_RECT_FILL, 0, 0, 11, 9, (0, 0, 255), 1, 0, 0)
    ctx.frame_render_overlay(cmds)
    drawn = ctx.overlay_read()
    assert not np.array_equal(drawn, bgr)
    assert ctx.frame_encode_regions(one, 75, overlay=True) == [oc.reference(drawn, one[0], 75)]
    assert ctx.frame_encode_regions(one, 75) == [oc.reference(bgr, one[0], 75)]


@pytest.fixture(scope='module')
def many():
    """300 seeded rects on a 320 x 240 frame and their Pillow files, computed once."""
    bgr = np.ascontiguousarray(jc.content('textured', 320, 240, seed=11)[:, :, ::-1])
    bgr[60:120, 100:200] = np.random.default_rng(2).integers(0, 256, (60, 100, 3), dtype=np.uint8)
    bgr.setflags(write=False)
    rects = oc.random_rects(300, (320, 240), seed=4)
    return bgr, rects, [oc.reference(bgr, r, 85) for r in rects]


def test_three_hundred_rects_in_one_call(ctx, many, monkeypatch):
    """Many workgroups of every kernel, table entries beyond one wavefront, hundreds of rows for the prefix pass -- in ONE
    library call; then the same list in chunks of three."""
    bgr, rects, want = many
    upload(ctx, bgr)
    calls = []
    real = type(ctx)._encode_regions_call
    monkeypatch.setattr(type(ctx), '_encode_regions_call', lambda self, arr, *a: calls.append(len(arr)) or real(self, arr, *a))
    check_files(ctx.frame_encode_regions(rects, 85), want, 'one call')
    assert calls == [300]
    del calls[:]
    monkeypatch.setattr(type(ctx), 'OBJENC_CHUNK_REGIONS', 3)
    check_files(ctx.frame_encode_regions(rects, 85), want, 'chunks of 3')
    assert calls == [3] * 100
    del calls[:]
    monkeypatch.setattr(type(ctx), 'OBJENC_CHUNK_REGIONS', _lib.FM_OBJENC_MAX_REGIONS)
    monkeypatch.setattr(type(ctx), 'OBJENC_CHUNK_MCUS', 40)              # ... and split by the MCU limit
    check_files(ctx.frame_encode_regions(rects[:40], 85), want[:40], 'chunks of 40 MCUs')
    assert len(calls) > 1 and sum(calls) == 40


def test_the_buffers_grow(ctx, many):
    bgr, rects, want = many
    upload(ctx, bgr)
    small, large = rects[:2], np.concatenate([rects, [(0, 0, 319, 239)] * 3]).astype(np.int32)
    whole = oc.reference(bgr, (0, 0, 319, 239), 85)
    assert ctx.frame_encode_regions(small, 85) == want[:2]
    assert ctx.frame_encode_regions(large, 85) == want + [whole] * 3
    assert ctx.frame_encode_regions(small, 85) == want[:2]
    assert ctx.frame_encode_jpeg(85) == whole                             # the whole-frame path shares the buffers


SIZE = (960, 540)


def run_mot(video, check=None, redact=None):
    from fastmot_amd import Track
    from test_mot_gpu import build_mot
    mot = build_mot(SIZE, video, 1)
    mot.redact = redact
    Track._count = 0
    mot.reset(1 / 30.)
    rows = []
    try:
        if check:
            with pytest.raises(RuntimeError):
                mot.encode_objects()
        for f in range(video.n_frames):
            mot.detector._frame_idx = f
            mot.step(video.frames[f], next_frame=video.frames[f + 1] if f + 1 < video.n_frames else None)
            if check:
                check(mot, f)
            rows.append([(t.trk_id, tuple(t.tlbr), t.confirmed, t.active, t.age, t.hits) for t in mot.tracker.tracks.values()])
    finally:
        mot.tracker._clear_tracks()
    return rows


@pytest.fixture(scope='module')
def video():
    from synthetic import SyntheticVideo
    return SyntheticVideo(SIZE, n_ids=6, n_frames=4, seed=2)


@pytest.fixture(scope='module')
def plain_rows(ctx, video):
    return run_mot(video)


def expected_rects(mot, part, margin, confirmed=True):
    from fastmot_amd.utils import redact as RD
    out = []
    for t in mot.tracker.tracks.values():
        if t.active and (t.confirmed or not confirmed):
            rect = RD.clip_rect(RD.region_rect(t.tlbr, RD.part_fractions(part), margin, SIZE), SIZE)
            if rect is not None:
                out.append((t.trk_id, int(t.label), rect))
    return out


def check_objects(objs, want_rects, picture, q, shrink=1):
    assert [(o.trk_id, o.label, o.rect) for o in objs] == want_rects
    for o in objs:
        assert o.data == oc.reference(picture, o.rect, q, shrink), o.trk_id
        hd = J.parse(o.data)
        assert (hd.width, hd.height) == o.size


def test_mot_encode_objects(ctx, video, plain_rows):
    """After every step: every crop equals the reference on the host pixels of that frame; with overlays=True on the
    picture render_frame() returns; encode_frame / render_frame are what they were; the tracks do not change."""
    seen = []

    def check(mot, f):
        pixels = video.frames[f]
        frame_file, drawn = mot.encode_frame(80), mot.render_frame()
        objs = mot.encode_objects(80)
        check_objects(objs, expected_rects(mot, 'box', 0.), pixels, 80)
        heads = mot.encode_objects(60, part='head', margin=0.2, shrink=2, confirmed=False)
        check_objects(heads, expected_rects(mot, 'head', 0.2, confirmed=False), pixels, 60, 2)
        check_objects(mot.encode_objects(80, overlays=True), expected_rects(mot, 'box', 0.), drawn, 80)
        assert mot.encode_objects(80, classes=[99]) == []
        assert mot.encode_frame(80) == frame_file and np.array_equal(mot.render_frame(), drawn)
        assert np.array_equal(ctx.frame_read(), pixels)
        for bad in (dict(quality=0), dict(shrink=3), dict(part='torso'), dict(margin=-1)):
            with pytest.raises(ValueError):
                mot.encode_objects(**bad)
        seen.append(len(objs))

    assert run_mot(video, check) == plain_rows
    assert sum(seen) >= 4 and any(len(row) for row in plain_rows)


def test_mot_encode_objects_redacted(ctx, video, plain_rows):
    """With MOT(redact=...) the crops are cut from the redacted picture, whatever `overlays` says."""
    from fastmot_amd.utils.redact import Redact, build_regions, redact_bgr
    cfg = Redact(mode='pixelate', part='head', margin=0.1, cells=4)
    seen = []

    def check(mot, f):
        regions = build_regions(mot.tracker.tracks.values(), mot._last_detections, cfg, SIZE)
        bare = redact_bgr(video.frames[f].copy(), regions)
        objs = mot.encode_objects(80, overlays=False)
        check_objects(objs, expected_rects(mot, 'box', 0.), bare, 80)
        if objs:
            assert any(o.data != oc.reference(video.frames[f], o.rect, 80) for o in objs)      # not the tracker's frame
        check_objects(mot.encode_objects(80, overlays=True), expected_rects(mot, 'box', 0.), mot.render_frame(), 80)
        seen.append(len(objs))

    assert run_mot(video, check, redact=cfg) == plain_rows
    assert sum(seen) >= 4


def test_track_stream_writes_snapshots(ctx, video, tmp_path):
    from fastmot_amd import Track
    from fastmot_amd.readahead import track_stream
    from fastmot_amd.utils.snapshots import SnapshotWriter
    from test_mot_gpu import build_mot
    mot = build_mot(SIZE, video, 1)
    Track._count = 0
    mot.reset(1 / 30.)
    returned = {}

    class Writer(SnapshotWriter):                    # records what encode_objects returned for each step
        def update(self, m):
            for o in m.encode_objects(**self.encode_options):
                returned[f'{o.trk_id:06d}/{m.frame_count:06d}.jpg'] = o.data
            super().update(m)

    frames = list(video.frames)

    class Stream:                                    # (the injected detector counts its own frames from 0)
        resolution = SIZE

        @staticmethod
        def read():
            return frames.pop(0) if frames else None

    writer = Writer(tmp_path / 'snaps', 'all', quality=70)
    try:
        n = track_stream(Stream, mot, snapshots=writer)
    finally:
        mot.tracker._clear_tracks()
    assert n == video.n_frames and returned
    files = {str(p.relative_to(tmp_path / 'snaps')): p.read_bytes() for p in (tmp_path / 'snaps').rglob('*.jpg')}
    assert files == returned
    with pytest.raises(RuntimeError):
        writer.update(mot)                           # track_stream closed it
