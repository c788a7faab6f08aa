"""CPU: the overlay command list -- its numpy statement (tests/overlay_ref.py) against Pillow's ImageDraw, the library's
host renderer (csrc/overlay_pixel.h, the text the kernel is compiled from, through fm_overlay_render_host) against the
numpy statement, and utils.overlay.build_commands + the host renderer against Visualizer.render, all bit for bit.

The equality with Pillow is that of the Pillow this was written with (12.2.0: its rectangle, line and ellipse
rasterisers and the FreeType default font); the GPU tests compare with the host renderer, not with Pillow."""
import itertools

import numpy as np
import pytest
from PIL import Image, ImageDraw, ImageFont

import overlay_cases as cases
import overlay_ref as R
from fastmot_amd import _lib
from fastmot_amd.utils.visualization import Visualizer

FM_ERR_ARG = -2


def pillow(frame, draw_fn):
    """`frame` (BGR) after draw_fn(ImageDraw) -- the way visualization._Canvas draws and commits."""
    img = Image.fromarray(np.ascontiguousarray(frame[..., ::-1]))
    draw_fn(ImageDraw.Draw(img))
    return np.asarray(img)[..., ::-1]


def rgb(bgr):
    return int(bgr[2]), int(bgr[1]), int(bgr[0])


def test_reference_rectangles_equal_pillow():
    base = cases.noise(12, 12, 3)
    col = (10, 200, 90)
    for x0, y0, x1, y1 in itertools.product(range(10), repeat=4):
        if x1 < x0 or y1 < y0:
            continue
        want = pillow(base, lambda d: d.rectangle([x0, y0, x1, y1], fill=rgb(col)))
        assert np.array_equal(R.render(base.copy(), R.rect_fill(x0, y0, x1, y1, col)), want), (x0, y0, x1, y1)
        for t in (1, 2):
            want = pillow(base, lambda d: d.rectangle([x0, y0, x1, y1], outline=rgb(col), width=t))
            assert np.array_equal(R.render(base.copy(), R.rect_outline(x0, y0, x1, y1, col, t)), want), (x0, y0, x1, y1, t)


def segments():
    rng = np.random.default_rng(11)
    w, h = 96, 64
    segs = np.stack([rng.integers(-10, w + 10, 2000), rng.integers(-10, h + 10, 2000),
                     rng.integers(-10, w + 10, 2000), rng.integers(-10, h + 10, 2000)], axis=1).tolist()
    segs += [[3, 9, 80, 9], [80, 9, 3, 9], [7, 2, 7, 60], [7, 60, 7, 2], [5, 5, 5, 5], [-3, 70, -3, 70], [4, 4, 50, 50], [50, 4, 4, 50],
             [90, 60, 60, 30], [-5, -5, 40, 40], [0, 0, 95, 63], [95, 0, 0, 63], [10, 10, 11, 40], [10, 10, 40, 11], [10, 10, 40, 9]]
    return w, h, segs


def test_reference_lines_equal_pillow_and_the_closed_form_equals_the_error_term():
    w, h, segs = segments()
    base = cases.noise(w, h, 4)
    for i, (x0, y0, x1, y1) in enumerate(segs):
        col = (i % 256, (i * 3) % 256, 255 - i % 200)
        want = pillow(base, lambda d: d.line([(x0, y0), (x1, y1)], fill=rgb(col), width=1))
        assert np.array_equal(R.render(base.copy(), R.line(x0, y0, x1, y1, col)), want), (x0, y0, x1, y1)
        xs, ys = R.line_points(x0, y0, x1, y1)
        assert list(zip(xs.tolist(), ys.tolist())) == R.line_points_stepwise(x0, y0, x1, y1), (x0, y0, x1, y1)
    # float coordinates are truncated towards zero, and a polyline is its segments
    pts = [(-0.7, 3.9), (20.99, 11.2), (40.5, -0.9), (63.2, 50.7)]
    want = pillow(base, lambda d: d.line(pts, fill=(1, 2, 3), width=1))
    ipts = [(int(x), int(y)) for x, y in pts]
    assert ipts[0] == (0, 3) and ipts[2] == (40, 0)
    cmds = np.concatenate([R.line(*a, *b, (3, 2, 1)) for a, b in zip(ipts, ipts[1:])])
    assert np.array_equal(R.render(base.copy(), cmds), want)


def test_reference_dot_equals_pillow():
    base = cases.noise(9, 7, 5)
    for x, y in [(0, 0), (8, 6), (8, 0), (0, 6), (4, 0), (0, 3), (8, 3), (4, 6), (4, 3), (9, 3), (-1, 2)]:
        want = pillow(base, lambda d: d.ellipse([x - 1, y - 1, x + 1, y + 1], fill=(30, 20, 10)))
        got = R.render(base.copy(), R.dot(x, y, (10, 20, 30)))
        assert np.array_equal(got, want), (x, y)
    assert (R.render(np.zeros((5, 5, 3), np.uint8), R.dot(2, 2, (1, 1, 1)))[..., 0] ==
            [[0, 0, 0, 0, 0], [0, 0, 1, 0, 0], [0, 1, 1, 1, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, 0]]).all()      # the plus, not the square


def test_reference_masks_equal_pillow_text():
    from fastmot_amd.utils.overlay import text_mask
    font = ImageFont.load_default()
    w, h = 90, 40
    base = cases.noise(w, h, 6)
    rng = np.random.default_rng(7)
    for text in ('7', '407', 'person: 0.87', 'visible: 12'):
        alpha, (dx, dy), bbox = text_mask(text)
        assert ((alpha > 0) & (alpha < 255)).any()            # anti-aliased: a real 'L' mask
        tw, th = alpha.shape[1], alpha.shape[0]
        for x, y in [(5, 6), (-tw // 2, 9), (w - tw // 2, 9), (7, -dy - th // 2), (7, h - dy - th // 2)]:
            ink = tuple(int(v) for v in rng.integers(0, 256, 3))
            want = pillow(base, lambda d: d.text((x, y), text, fill=rgb(ink), font=font))
            blob = bytearray()
            got = R.render(base.copy(), R.mask(x + dx, y + dy, alpha, ink, blob), blob)
            assert np.array_equal(got, want), (text, x, y)
            assert (got != base).any()
        assert bbox == tuple(ImageDraw.Draw(Image.new('RGB', (1, 1))).textbbox((0, 0), text, font=font))


def all_lists(w, h):
    lists = dict(cases.primitive_lists(w, h))
    lists.update(cases.painter_lists(w, h))
    lists['scene'] = cases.scene_commands(w, h)
    return lists


@pytest.mark.parametrize('size', [(67, 35), (80, 48), (1, 1)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_host_renderer_equals_reference(size):
    w, h = size
    base = cases.noise(w, h, 8)
    for name, (cmds, masks) in all_lists(w, h).items():
        assert _lib.overlay_check(cmds, masks, w, h) == 0, name
        want = R.render(base.copy(), cmds, masks)
        got = _lib.overlay_render_host(base.copy(), cmds, masks)
        assert np.array_equal(got, want), name
        if name not in ('empty', 'outside'):
            assert (got != base).any() or (w, h) == (1, 1), name
        else:
            assert np.array_equal(got, base), name
    # the segments and rectangles of the Pillow comparisons, through the C code as well
    _, _, segs = segments()
    cmds = np.concatenate([R.line(*s, (i % 256, 7, 255 - i % 256)) for i, s in enumerate(segs)] +
                          [R.rect_outline(x0, y0, x1, y1, (x0 * 20, y1 * 20, 99), t)
                           for x0, y0, x1, y1 in itertools.product((0, 3, 4, 9), repeat=4) if x1 >= x0 and y1 >= y0 for t in (1, 2, 3, 8)])
    assert np.array_equal(_lib.overlay_render_host(base.copy(), cmds), R.render(base.copy(), cmds))
    # a strided frame: only its own pixels change
    wide = np.zeros((h, w + 5, 3), np.uint8)
    wide[:, :w] = base
    _lib.overlay_render_host(wide[:, :w], *all_lists(w, h)['scene'])
    assert np.array_equal(wide[:, :w], R.render(base.copy(), *all_lists(w, h)['scene'])) and not wide[:, w:].any()


@pytest.mark.parametrize('flags', [cases.ALL_FLAGS, {}], ids=['all_flags', 'no_flags'])
def test_build_commands_equals_visualizer(flags):
    w, h = 160, 120
    base = cases.noise(w, h, 9)
    tracks, dets, klt, bg_prev, bg_cur, caption = cases.scene(w, h)
    assert any(len(t.bboxes) > 8 for t in tracks) and any(t.trk_id >= 100 for t in tracks)
    want = base.copy()
    Visualizer(**flags).render(want, tracks, dets, klt, bg_prev, bg_cur, caption=caption)
    cmds, masks = cases.scene_commands(w, h, flags)
    got = _lib.overlay_render_host(base.copy(), cmds, masks)
    assert np.array_equal(got, want)
    assert np.array_equal(R.render(base.copy(), cmds, masks), want)
    kinds = set(cmds['kind'].tolist())
    assert kinds == ({R.OVL_RECT_FILL, R.OVL_RECT_OUTLINE, R.OVL_LINE, R.OVL_DOT, R.OVL_MASK} if flags else
                     {R.OVL_RECT_FILL, R.OVL_RECT_OUTLINE, R.OVL_MASK})
    if flags:
        bare = base.copy()
        Visualizer().render(bare, tracks, dets, klt, bg_prev, bg_cur, caption=caption)
        assert (want != bare).sum() > 1000               # the flags drew something: the comparison is not of bare boxes


def test_check_refuses_malformed_lists_and_writes_nothing():
    w, h = 40, 30
    base = cases.noise(w, h, 10)
    blob = bytearray()
    good = np.concatenate([R.rect_fill(1, 1, 5, 5, (1, 2, 3)), R.mask(2, 2, cases.glyphs('7'), (0, 0, 0), blob)])
    assert _lib.overlay_check(good, blob, w, h) == 0
    lim = _lib.FM_OVERLAY_MAX_COORD
    assert _lib.overlay_check(R.line(-lim, lim, lim, -lim, (0, 0, 0)), b'', w, h) == 0          # the limits themselves
    assert _lib.overlay_check(R.rect_outline(0, 0, 9, 9, (0, 0, 0), 8), b'', w, h) == 0

    def bad(cmds, masks=b''):
        frame = base.copy()
        assert _lib.overlay_check(cmds, masks, w, h) == FM_ERR_ARG
        with pytest.raises(_lib.FastMOTHipError):
            _lib.overlay_render_host(frame, cmds, masks)
        assert np.array_equal(frame, base)                # a good command in front of the bad one drew nothing either
    lead = R.rect_fill(0, 0, w, h, (9, 9, 9))
    bad(np.concatenate([lead, R.cmd(5, 1, 1, 2, 2)]))                                  # unknown kinds
    bad(np.concatenate([lead, R.cmd(-1, 1, 1, 2, 2)]))
    bad(np.concatenate([lead, R.rect_outline(1, 1, 9, 9, (0, 0, 0), 0)]))              # thickness outside 1..8
    bad(np.concatenate([lead, R.rect_outline(1, 1, 9, 9, (0, 0, 0), 9)]))
    for field in ('x0', 'y0', 'x1', 'y1'):                                             # a coordinate beyond +-2^20
        for v in (lim + 1, -lim - 1, 2 ** 31 - 1, -2 ** 31):
            c = R.line(1, 1, 5, 5, (0, 0, 0))
            c[field] = v
            bad(np.concatenate([lead, c]))
    m = R.mask(2, 2, cases.glyphs('7'), (0, 0, 0), bytearray(blob))
    for off, mw, mh in [(len(blob), 1, 1), (len(blob) + 1, 0, 0), (len(blob) - 3, 2, 2), (0, len(blob), 2), (0, -1, 4), (0, 4, -1),
                        (0, lim, lim), (2 ** 32 - 1, 1, 1), (0, 65536, 65536)]:         # rectangles not inside the blob
        c = m.copy()
        c['mask_off'], c['x1'], c['y1'] = off, mw, mh
        bad(np.concatenate([lead, c]), blob)
    bad(np.concatenate([lead, m]), b'')                                                # a mask and no blob
    bad(np.tile(lead, _lib.FM_OVERLAY_MAX_CMDS + 1))                                   # too long a list
    assert _lib.overlay_check(np.tile(lead, 16), b'', w, h) == 0
    bad(lead, bytes(_lib.FM_OVERLAY_MAX_MASK_BYTES + 1))                               # too large a blob
    assert _lib.overlay_check(lead, bytes(_lib.FM_OVERLAY_MAX_MASK_BYTES), w, h) == 0
    assert _lib.overlay_check(np.zeros(0, R.OVERLAY_CMD_DTYPE), b'', w, h) == 0        # the empty list is a list


def test_draw_and_gpu_draw_exclude_each_other():
    from fastmot_amd.mot import MOT
    with pytest.raises(ValueError, match='gpu_draw'):
        MOT((160, 120), draw=True, gpu_draw=True)
