"""Redaction of tracked objects in the pictures that leave the tracker (MOT(redact=...); fastmot_hip.h
fm_frame_render_redacted): the `Redact` settings, the region list built from a step's tracks and detections, and the host
twin that redacts a host frame.  The arithmetic is the library's (csrc/redact_pixel.h), integer and exact; this module
only decides WHERE: which boxes, which part of them, how large the cells.

What is NOT covered, by design: `ctx.frame_read()`, the frame the caller handed to `step`, and the ReID crops are the
unredacted picture -- the tracker must see it.  Only `MOT.render_frame()`, `MOT.encode_frame()`, `MOT.export_frame_i420()`
and, with `draw=True`, the host frame drawn on are redacted."""
import math
from types import SimpleNamespace

import numpy as np

from .._lib import (REDACT_REGION_DTYPE, REDACT_PIXELATE, REDACT_SMOOTH, REDACT_FILL, REDACT_RECT, REDACT_ELLIPSE,
                    FM_SRC_MAX_DIM, redact_render_host)

MODES = {'pixelate': REDACT_PIXELATE, 'smooth': REDACT_SMOOTH, 'fill': REDACT_FILL}
SHAPES = {'rect': REDACT_RECT, 'ellipse': REDACT_ELLIPSE}
# (left, top, right, bottom) as fractions of the box: 'head' is the upper middle of a person box, not a face detector
PARTS = {'box': (0., 0., 1., 1.), 'head': (0.25, 0., 0.75, 0.25)}
TARGETS = ('tracks', 'detections')


class Redact:
    """Settings of the redaction.

    mode     'pixelate' (default: every pixel takes its cell's mean), 'smooth' (bilinear between the cell means: the same
             information without the blocks) or 'fill' (`color`).
    shape    'rect' (default) or 'ellipse' (the ellipse inscribed in the region).
    part     which part of a box is redacted: 'box' (default, all of it), 'head' (the upper quarter, middle half) or four
             fractions (left, top, right, bottom) of the box, 0 <= left < right <= 1 and 0 <= top < bottom <= 1.
    margin   fraction of the part's width / height added on every side (default 0.1): boxes jitter from frame to frame.
    cells    number of cells across the LONGER side of a region (default 8): c = clamp(ceil(side / cells), 2, 256), so a
             person near the camera is not left recognisable by a cell size chosen for a far one.
    cell     a fixed cell side 2..256 instead (default None: use `cells`).
    classes  labels to redact (default None: every label).
    targets  which boxes (default both): 'tracks' -- every ACTIVE track, confirmed or not, at its current box, so that a
             person tracked by KLT between detector frames stays covered -- and 'detections' -- this step's detections,
             so that a person is covered from the first frame they are detected, not from the frame their track is
             confirmed.
    color    B, G, R of 'fill' (default black).

    Fractions become pixels OUTWARDS: with the box's inclusive corners (x0, y0, x1, y1) as the extent [x0, x1 + 1), the
    part and its margin give a real-valued extent [l, r); the region's corners are floor(l) and ceil(r) - 1, so rounding
    never uncovers anything.  A box may reach beyond the frame; a region is cut where its side would exceed the library's
    limit (FM_SRC_MAX_DIM), which only boxes many times the frame's size meet."""

    def __init__(self, mode='pixelate', shape='rect', part='box', margin=0.1, cells=8, cell=None, classes=None,
                 targets=TARGETS, color=(0, 0, 0)):
        if mode not in MODES:
            raise ValueError(f'redact mode {mode!r}: one of {sorted(MODES)}')
        if shape not in SHAPES:
            raise ValueError(f'redact shape {shape!r}: one of {sorted(SHAPES)}')
        if isinstance(part, str):
            if part not in PARTS:
                raise ValueError(f'redact part {part!r}: one of {sorted(PARTS)} or four box fractions')
            fractions = PARTS[part]
        else:
            fractions = tuple(float(v) for v in part)
            if len(fractions) != 4 or not (0 <= fractions[0] < fractions[2] <= 1 and 0 <= fractions[1] < fractions[3] <= 1):
                raise ValueError('redact part: (left, top, right, bottom) fractions with 0 <= left < right <= 1, 0 <= top < bottom <= 1')
        if not 0 <= float(margin) <= 4:
            raise ValueError('redact margin outside 0..4')
        if cell is not None and not 2 <= int(cell) <= 256:
            raise ValueError('redact cell outside 2..256')
        if int(cells) < 1:
            raise ValueError('redact cells must be at least 1')
        targets = (targets,) if isinstance(targets, str) else tuple(targets)
        if not targets or any(t not in TARGETS for t in targets):
            raise ValueError(f'redact targets: a non-empty subset of {TARGETS}')
        color = tuple(int(v) for v in color)
        if len(color) != 3 or any(not 0 <= v <= 255 for v in color):
            raise ValueError('redact color: three values 0..255 (B, G, R)')
        self.mode, self.shape, self.part, self.fractions = mode, shape, part, fractions
        self.margin, self.cells, self.cell = float(margin), int(cells), None if cell is None else int(cell)
        self.classes = None if classes is None else frozenset(int(v) for v in classes)
        self.targets, self.color = targets, color

    @classmethod
    def coerce(cls, value):
        """None, a Redact, a dictionary or a namespace of its keywords (the `"redact"` entry of `mot_cfg`) -> Redact or None."""
        if value is None or isinstance(value, cls):
            return value
        if isinstance(value, SimpleNamespace):
            value = vars(value)
        if isinstance(value, dict):
            return cls(**value)
        raise TypeError('redact: None, a Redact, or a dictionary of its settings')


def region_rect(tlbr, fractions, margin, size):
    """The pixel rectangle of a part of a box: `fractions` (left, top, right, bottom) of the box `tlbr` (inclusive corners),
    widened by `margin` times the part's width / height on every side and rounded OUTWARDS (the class docstring above)
    -> (x0, y0, x1, y1) with inclusive corners, or None for an empty or NaN box.  The rectangle may reach beyond the frame
    of `size` (w, h); it is cut only where a side would exceed the library's limit.  One rule for what is redacted and for
    what MOT.encode_objects crops (which then clips with `clip_rect`)."""
    x0, y0, x1, y1 = (float(v) for v in tlbr)
    w, h = x1 - x0 + 1, y1 - y0 + 1
    if not (w > 0 and h > 0):                      # (NaN as well)
        return None
    fl, ft, fr, fb = fractions
    l, t, r, b = x0 + fl * w, y0 + ft * h, x0 + fr * w, y0 + fb * h
    mx, my = margin * (r - l), margin * (b - t)
    corners = []
    for lo, hi, extent in ((l - mx, r + mx, size[0]), (t - my, b + my, size[1])):
        slack = (FM_SRC_MAX_DIM - extent) // 2     # the frame and this much on either side: a side within the limit
        a = min(max(math.floor(lo), -slack), extent - 1 + slack)
        z = min(max(math.ceil(hi) - 1, -slack), extent - 1 + slack)
        corners.append((int(a), int(z)))
    (rx0, rx1), (ry0, ry1) = corners
    if rx1 < rx0 or ry1 < ry0:
        return None
    return rx0, ry0, rx1, ry1


def clip_rect(rect, size):
    """A rectangle (inclusive corners, or None) cut to the frame of `size` (w, h) -> (x0, y0, x1, y1), or None when no pixel
    of it lies inside the frame."""
    if rect is None:
        return None
    x0, y0, x1, y1 = max(rect[0], 0), max(rect[1], 0), min(rect[2], size[0] - 1), min(rect[3], size[1] - 1)
    return None if x1 < x0 or y1 < y0 else (x0, y0, x1, y1)


def part_fractions(part):
    """'box', 'head' or four fractions (left, top, right, bottom) of a box -> the fractions; ValueError otherwise."""
    if isinstance(part, str):
        if part not in PARTS:
            raise ValueError(f'part {part!r}: one of {sorted(PARTS)} or four box fractions')
        return PARTS[part]
    fractions = tuple(float(v) for v in part)
    if len(fractions) != 4 or not (0 <= fractions[0] < fractions[2] <= 1 and 0 <= fractions[1] < fractions[3] <= 1):
        raise ValueError('part: (left, top, right, bottom) fractions with 0 <= left < right <= 1, 0 <= top < bottom <= 1')
    return fractions


def _region_of(tlbr, cfg, size):
    rect = region_rect(tlbr, cfg.fractions, cfg.margin, size)
    if rect is None:
        return None
    rx0, ry0, rx1, ry1 = rect
    side = max(rx1 - rx0 + 1, ry1 - ry0 + 1)
    cell = cfg.cell if cfg.cell is not None else min(256, max(2, -(-side // cfg.cells)))
    return rx0, ry0, rx1, ry1, cell


def build_regions(tracks, detections, cfg, size):
    """The region list (ndarray of _lib.REDACT_REGION_DTYPE) of one step: `tracks` (any iterable of Track; the inactive ones
    are left out here), then `detections` (records with tlbr and label), filtered by `cfg.classes`, each box cut to
    `cfg.part`, widened by `cfg.margin` and rounded outwards.  `size` (w, h) is the frame's.  Later regions win where
    they overlap; every region computes from the original frame, so the order matters only there."""
    boxes = []
    if 'tracks' in cfg.targets:
        boxes += [(t.tlbr, t.label) for t in tracks if t.active]
    if 'detections' in cfg.targets and detections is not None:
        boxes += [(d.tlbr, d.label) for d in detections]
    rows = []
    for tlbr, label in boxes:
        if cfg.classes is not None and int(label) not in cfg.classes:
            continue
        reg = _region_of(tlbr, cfg, size)
        if reg is not None:
            rows.append(reg)
    out = np.zeros(len(rows), REDACT_REGION_DTYPE)
    if rows:
        arr = np.asarray(rows, np.int64)
        out['x0'], out['y0'], out['x1'], out['y1'], out['cell'] = arr.T
        out['mode'], out['shape'], out['color'] = MODES[cfg.mode], SHAPES[cfg.shape], cfg.color
    return out


def redact_bgr(frame, regions):
    """Redacts the host frame (HxWx3 uint8 BGR, writeable) IN PLACE by a region list and returns it: the library's host
    twin of the GPU path (fm_redact_render_host), the same picture bit for bit.  A malformed list raises and writes
    nothing."""
    return redact_render_host(frame, regions)
