"""CPU: redaction regions -- fm_redact_check's refusals, the library's host twin (csrc/redact_pixel.h, the text the kernels
are compiled from, through fm_redact_render_host) against the numpy statement tests/redact_ref.py, the proof that the
cases see each mistake the reference can be switched to, and utils.redact.build_regions.  Every comparison is exact."""
from types import SimpleNamespace

import numpy as np
import pytest

import redact_cases as cases
import redact_ref as R
from fastmot_amd import _lib
from fastmot_amd.utils.redact import Redact, build_regions, redact_bgr

FM_ERR_ARG = -2


@pytest.fixture(scope='module')
def frame():
    return cases.noise(cases.W, cases.H, 31)


@pytest.fixture(scope='module')
def wanted(frame):
    """name -> the clean reference picture of every case, computed once."""
    return {name: R.render(frame, regions) for name, regions in cases.all_lists().items()}


def test_check_refuses_malformed_lists_and_writes_nothing(frame):
    w, h = cases.W, cases.H
    good = R.as_array([R.region(1, 1, 9, 9), R.region(-5, -5, 50, 50, R.SMOOTH, R.ELLIPSE, 256)])
    assert _lib.redact_check(good, w, h) == 0
    lim = _lib.FM_OVERLAY_MAX_COORD
    assert _lib.redact_check(R.as_array([R.region(lim, lim, -lim, -lim)]), w, h) == 0           # the limits; empty
    assert _lib.redact_check(R.as_array([R.region(-lim, -lim, -lim + 16383, -lim + 16383, cell=2)]), w, h) == 0
    assert _lib.redact_check(np.zeros(0, _lib.REDACT_REGION_DTYPE), w, h) == 0                   # the empty list is a list
    assert _lib.load().fm_redact_check(None, 1, w, h) == FM_ERR_ARG                              # a null list with n > 0

    def bad(regions, size=(w, h)):
        assert _lib.redact_check(regions, *size) == FM_ERR_ARG
        if size == (w, h):
            pixels = frame.copy()
            with pytest.raises(_lib.FastMOTHipError):
                _lib.redact_render_host(pixels, regions)
            assert np.array_equal(pixels, frame)            # the good region in front of the bad one changed nothing either
    lead = R.as_array([R.region(0, 0, w, h, R.FILL, color=(9, 9, 9))])

    def with_field(field, value):
        r = R.as_array([R.region(2, 2, 12, 12)])
        r[field] = value
        return np.concatenate([lead, r])
    for mode in (-1, 3):
        bad(with_field('mode', mode))
    for shape in (-1, 2):
        bad(with_field('shape', shape))
    for cell in (0, 1, 257, -4):
        bad(with_field('cell', cell))
    bad(with_field('reserved', 1))
    for field in ('x0', 'y0', 'x1', 'y1'):
        for v in (lim + 1, -lim - 1, 2 ** 31 - 1, -2 ** 31):
            bad(with_field(field, v))
    bad(np.concatenate([lead, R.as_array([R.region(-10, 0, 16374, 5)])]))                      # 16385 wide
    bad(np.concatenate([lead, R.as_array([R.region(0, -10, 5, 16374)])]))                      # 16385 high
    assert _lib.redact_check(R.as_array([R.region(-10, 0, 16373, 5)]), w, h) == 0
    bad(np.tile(lead, _lib.FM_REDACT_MAX_REGIONS + 1))                                          # too long a list
    assert _lib.redact_check(np.tile(lead, _lib.FM_REDACT_MAX_REGIONS), w, h) == 0
    # too many cells in all: 2048 x 1024 cells of side 2 are 2 x the cap; the same list on a small frame has few cells
    big = R.as_array([R.region(0, 0, 4095, 2047, cell=2)])
    assert _lib.FM_REDACT_MAX_CELLS == 1 << 20
    bad(big, (4096, 2048))
    assert _lib.redact_check(big, w, h) == 0
    half = R.as_array([R.region(0, 0, 2047, 1023, cell=2)])                                     # 2^19 cells each
    assert _lib.redact_check(np.concatenate([half, half]), 4096, 2048) == 0
    bad(np.concatenate([half, half, R.as_array([R.region(0, 0, 1, 1)])]), (4096, 2048))
    big['mode'] = R.FILL                                                                        # FILL has no cells
    assert _lib.redact_check(big, 4096, 2048) == 0
    for size in ((0, 5), (5, 0), (16385, 5), (5, 16385)):
        bad(good, size)


def test_host_twin_equals_reference(frame, wanted):
    lists = cases.all_lists()
    assert len(lists) > 100
    changed = 0
    for name, regions in lists.items():
        arr = R.as_array(regions)
        assert _lib.redact_check(arr, cases.W, cases.H) == 0, name
        got = redact_bgr(frame.copy(), arr)
        assert np.array_equal(got, wanted[name]), name
        changed += bool((got != frame).any())
        if name == 'empty' or name.startswith('outside'):
            assert np.array_equal(got, frame), name
    assert changed > 90
    # a strided frame: only its own pixels change
    wide = np.zeros((cases.H, cases.W + 5, 3), np.uint8)
    wide[:, :cases.W] = frame
    redact_bgr(wide[:, :cases.W], R.as_array(lists['overlap_abc']))
    assert np.array_equal(wide[:, :cases.W], wanted['overlap_abc']) and not wide[:, cases.W:].any()


def test_list_order_decides_where_regions_overlap(wanted):
    a, b, c = wanted['overlap_abc'], wanted['overlap_cba'], wanted['overlap_bca']
    assert (a != b).any() and (a != c).any() and (b != c).any()
    # every region computes from the original: where only the LAST region of a list lies on top, the pictures of two lists
    # that end with the same region agree there -- and 'with_empty' (empty regions, then the first) is that region alone
    only_first = R.render(cases.noise(cases.W, cases.H, 31), cases.overlapping()[:1])
    assert np.array_equal(wanted['with_empty'], only_first)
    r = cases.overlapping()[0]
    assert np.array_equal(c[r['y0']:r['y1'] + 1, r['x0']:r['x1'] + 1], only_first[r['y0']:r['y1'] + 1, r['x0']:r['x1'] + 1])


@pytest.mark.parametrize('mistake', R.MISTAKES)
def test_cases_see_every_mistake_of_the_reference(frame, wanted, mistake):
    """The case list is only worth something if a kernel that makes the mistake fails it."""
    seen = [name for name, regions in cases.all_lists().items() if (R.render(frame, regions, mistake) != wanted[name]).any()]
    assert seen, mistake
    print(mistake, len(seen), seen[:6])


def track(tlbr, label=1, age=0, hits=5, confirm_hits=3):
    t = SimpleNamespace(tlbr=np.asarray(tlbr, float), label=label, age=age, hits=hits, confirm_hits=confirm_hits)
    t.active, t.confirmed = age < 2, hits >= confirm_hits
    return t


def dets(rows):
    out = np.zeros(len(rows), [('tlbr', float, 4), ('label', int), ('conf', float)]).view(np.recarray)
    for k, (tlbr, label) in enumerate(rows):
        out[k].tlbr, out[k].label, out[k].conf = tlbr, label, 0.9
    return out


def corners(regions):
    return [tuple(int(r[f]) for f in ('x0', 'y0', 'x1', 'y1')) for r in regions]


def test_build_regions_geometry():
    size = (320, 180)
    box = track((100, 40, 139, 119))                       # 40 x 80
    # no margin: the box itself; c = ceil(80 / 8) = 10
    reg = build_regions([box], None, Redact(margin=0), size)
    assert corners(reg) == [(100, 40, 139, 119)] and reg['cell'].tolist() == [10]
    assert reg['mode'].tolist() == [R.PIXELATE] and reg['shape'].tolist() == [R.RECT] and reg['reserved'].tolist() == [0]
    # margin 0.1: 4 columns and 8 rows on every side
    reg = build_regions([box], None, Redact(margin=0.1), size)
    assert corners(reg) == [(96, 32, 143, 127)] and reg['cell'].tolist() == [12]               # ceil(96 / 8)
    # fractions round outwards: a 41 x 81 box, margin 0.1 -> [95.9, 145.1) x [31.9, 129.1)
    reg = build_regions([track((100, 40, 140, 120))], None, Redact(margin=0.1), size)
    assert corners(reg) == [(95, 31, 145, 129)]
    # 'head': the upper quarter, middle half
    reg = build_regions([box], None, Redact(part='head', margin=0, mode='smooth', shape='ellipse'), size)
    assert corners(reg) == [(110, 40, 129, 59)] and reg['cell'].tolist() == [3]                 # ceil(20 / 8)
    assert reg['mode'].tolist() == [R.SMOOTH] and reg['shape'].tolist() == [R.ELLIPSE]
    reg = build_regions([box], None, Redact(part=(0.5, 0.5, 1, 1), margin=0, cell=7, mode='fill', color=(1, 2, 3)), size)
    assert corners(reg) == [(120, 80, 139, 119)] and reg['cell'].tolist() == [7] and reg['color'].tolist() == [[1, 2, 3]]
    # cells -> c is clamped into 2..256
    assert build_regions([track((0, 0, 7, 7))], None, Redact(margin=0), size)['cell'].tolist() == [2]
    assert build_regions([track((0, 0, 4999, 99))], None, Redact(margin=0, cells=4), size)['cell'].tolist() == [256]
    for kw in (dict(mode='blur'), dict(shape='circle'), dict(part='face'), dict(part=(0.5, 0, 0.5, 1)), dict(cell=1), dict(cell=257),
               dict(targets=()), dict(targets=('faces',)), dict(margin=-1), dict(color=(0, 0, 256))):
        with pytest.raises(ValueError):
            Redact(**kw)
    assert Redact.coerce(None) is None and Redact.coerce(dict(mode='fill')).mode == 'fill'
    assert Redact.coerce(SimpleNamespace(part='head')).fractions == (0.25, 0., 0.75, 0.25)


def test_build_regions_targets_classes_and_boxes_beyond_the_frame():
    size = (320, 180)
    confirmed, fresh = track((10, 10, 29, 49)), track((50, 10, 69, 49), hits=1)
    coasting, lost = track((90, 10, 109, 49), age=1), track((130, 10, 149, 49), age=2)
    other = track((170, 10, 189, 49), label=3)
    assert not fresh.confirmed and coasting.active and not lost.active
    tracks = [confirmed, fresh, coasting, lost, other]
    found = dets([((200, 20, 219, 59), 1), ((240, 20, 259, 59), 3)])
    cfg = Redact(margin=0)
    assert corners(build_regions(tracks, found, cfg, size)) == [(10, 10, 29, 49), (50, 10, 69, 49), (90, 10, 109, 49), (170, 10, 189, 49),
                                                                (200, 20, 219, 59), (240, 20, 259, 59)]      # tracks, then detections
    assert corners(build_regions(tracks, found, Redact(margin=0, classes=(1,)), size)) == \
        [(10, 10, 29, 49), (50, 10, 69, 49), (90, 10, 109, 49), (200, 20, 219, 59)]
    assert corners(build_regions(tracks, found, Redact(margin=0, targets='detections'), size)) == [(200, 20, 219, 59), (240, 20, 259, 59)]
    assert len(build_regions(tracks, found, Redact(margin=0, targets=('tracks',)), size)) == 4
    assert len(build_regions([], dets([]), cfg, size)) == 0 and len(build_regions([], None, cfg, size)) == 0
    # boxes beyond the frame, wholly outside, absurdly large, or degenerate
    wild = [track((-40, -30, 20, 50)), track((300, 150, 400, 260)), track((1000, 1000, 1100, 1200)),
            track((-1e7, -1e7, 1e7, 1e7)), track((50, 50, 40, 60)), track((np.nan, 0, 10, 10))]
    reg = build_regions(wild, None, Redact(margin=0.25), size)
    assert len(reg) == 4 and corners(reg)[0] == (-56, -51, 36, 71)
    assert _lib.redact_check(reg, *size) == 0
    assert int(reg[3]['x1']) - int(reg[3]['x0']) + 1 <= _lib.FM_SRC_MAX_DIM and int(reg[3]['x0']) < 0 and int(reg[3]['x1']) >= size[0]
    pixels = cases.noise(*size, 5)
    want = R.render(pixels, reg)
    assert np.array_equal(redact_bgr(pixels.copy(), reg), want) and (want != pixels).all(axis=2).mean() > 0.9


def test_track_stream_writes_redacted_host_frames():
    """The frame loop writes the array it read: with MOT(redact=...) it is redacted in place first, unless draw=True has
    done so in the step; without `redact` it is written as it was read."""
    from fastmot_amd.readahead import track_stream
    frames = [cases.noise(cases.W, cases.H, 40 + k) for k in range(3)]
    regions = R.as_array(cases.overlapping())

    class Stream:
        def __init__(self):
            self.todo, self.written = [f.copy() for f in frames], []

        def read(self):
            return self.todo.pop(0) if self.todo else None

        def write(self, frame):
            self.written.append(frame.copy())

    class Mot:
        frame_count = 0

        def __init__(self, redact, draw):
            self.redact, self.draw, self.calls = redact, draw, 0

        def step(self, frame, next_frame=None):
            self.frame_count += 1

        def redact_frame(self, frame):
            self.calls += 1
            return redact_bgr(frame, regions)

    for redact, draw, redacted in ((Redact(), False, True), (Redact(), True, False), (None, False, False)):
        stream, mot = Stream(), Mot(redact, draw)
        assert track_stream(stream, mot, write_frames=True) == 3
        assert mot.calls == (3 if redacted else 0)
        for got, f in zip(stream.written, frames):
            assert np.array_equal(got, R.render(f, regions) if redacted else f)


def test_mot_accepts_redact_settings_only():
    from fastmot_amd.mot import MOT
    with pytest.raises(ValueError, match='redact mode'):
        MOT((160, 120), redact={'mode': 'blur'})
    with pytest.raises(TypeError, match='redact'):
        MOT((160, 120), redact='pixelate')
