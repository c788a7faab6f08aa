"""Redaction of a frame by a region list, in numpy integers: what fm_redact_render_host, the cell-mean kernel of
csrc/redact.hip and the tile pass of csrc/overlay.hip must compute.  Written from the definitions, not from the C text.

A region is a dict (`region(...)`) or a row of fastmot_amd._lib.REDACT_REGION_DTYPE.  `render(frame, regions)` returns the
redacted copy.  `render(..., mistake=NAME)` makes one of the mistakes a kernel can make (MISTAKES); the tests assert that
their cases tell each of them from the clean result."""
import numpy as np

PIXELATE, SMOOTH, FILL = 0, 1, 2
RECT, ELLIPSE = 0, 1

MISTAKES = ('truncated_mean', 'full_cell_divisor', 'clipped_anchor', 'unclamped_neighbours', 'wrong_clamp_range',
            'reads_earlier_output', 'ellipse_32bit')


def region(x0, y0, x1, y1, mode=PIXELATE, shape=RECT, cell=4, color=(0, 0, 0)):
    return dict(x0=x0, y0=y0, x1=x1, y1=y1, mode=mode, shape=shape, cell=cell, color=tuple(color))


def as_array(regions):
    """The list as rows of fm_redact_region."""
    from fastmot_amd._lib import REDACT_REGION_DTYPE
    out = np.zeros(len(regions), REDACT_REGION_DTYPE)
    for k, r in enumerate(regions):
        r = _fields(r)
        for f in ('x0', 'y0', 'x1', 'y1', 'mode', 'shape', 'cell'):
            out[k][f] = r[f]
        out[k]['color'] = r['color']
    return out


def _fields(r):
    if isinstance(r, dict):
        return r
    return dict(x0=int(r['x0']), y0=int(r['y0']), x1=int(r['x1']), y1=int(r['y1']), mode=int(r['mode']), shape=int(r['shape']),
                cell=int(r['cell']), color=tuple(int(v) for v in r['color']))


def _inside(r, xs, ys, mistake):
    """[rows, columns] bool: which pixels of the columns xs and rows ys belong to the shape."""
    if r['shape'] == RECT:
        return np.ones((len(ys), len(xs)), bool)
    kind = np.int32 if mistake == 'ellipse_32bit' else np.int64          # (int32 arrays wrap around silently)
    a, b = np.array([r['x1'] - r['x0'] + 1], kind), np.array([r['y1'] - r['y0'] + 1], kind)
    dx = (2 * (xs - r['x0']) + 1).astype(kind) - a
    dy = (2 * (ys - r['y0']) + 1).astype(kind) - b
    return (dx * dx * b * b)[None, :] + (dy * dy * a * a)[:, None] <= a * a * b * b


def _means(src, r, box, anchor, mistake):
    """([jmax - jmin + 1, imax - imin + 1, 3] int64 means of the existing cells, (imin, imax, jmin, jmax))."""
    c = r['cell']
    ax, ay = anchor
    cx0, cy0, cx1, cy1 = box
    imin, imax, jmin, jmax = (cx0 - ax) // c, (cx1 - ax) // c, (cy0 - ay) // c, (cy1 - ay) // c
    means = np.zeros((jmax - jmin + 1, imax - imin + 1, 3), np.int64)
    for j in range(jmin, jmax + 1):
        ya, yb = max(ay + j * c, cy0), min(ay + (j + 1) * c - 1, cy1)
        for i in range(imin, imax + 1):
            xa, xb = max(ax + i * c, cx0), min(ax + (i + 1) * c - 1, cx1)
            n = (xb - xa + 1) * (yb - ya + 1)
            assert n > 0
            sums = src[ya:yb + 1, xa:xb + 1].reshape(-1, 3).astype(np.int64).sum(axis=0)
            if mistake == 'truncated_mean':
                means[j - jmin, i - imin] = sums // n
            elif mistake == 'full_cell_divisor':
                means[j - jmin, i - imin] = (sums + c * c // 2) // (c * c)
            else:
                means[j - jmin, i - imin] = (sums + n // 2) // n
    return means, (imin, imax, jmin, jmax)


def _values(src, r, box, xs, ys, mistake):
    """[rows, columns, 3] int64: the region's value at every pixel of the columns xs and rows ys."""
    if r['mode'] == FILL:
        return np.broadcast_to(np.array(r['color'], np.int64), (len(ys), len(xs), 3))
    c = r['cell']
    anchor = (max(r['x0'], 0), max(r['y0'], 0)) if mistake == 'clipped_anchor' else (r['x0'], r['y0'])
    means, (imin, imax, jmin, jmax) = _means(src, r, box, anchor, mistake)
    ax, ay = anchor
    if r['mode'] == PIXELATE:
        return means[((ys - ay) // c - jmin)[:, None], ((xs - ax) // c - imin)[None, :]]
    u, v = 2 * (xs - ax) + 1 - c, 2 * (ys - ay) + 1 - c
    i0, j0 = u // (2 * c), v // (2 * c)                      # (floor division)
    fx, fy = (u - 2 * c * i0)[None, :, None], (v - 2 * c * j0)[:, None, None]
    lo_i, hi_i, lo_j, hi_j = imin, imax, jmin, jmax
    if mistake == 'wrong_clamp_range':                       # the grid of the unclipped rectangle
        lo_i, lo_j, hi_i, hi_j = 0, 0, (r['x1'] - ax) // c, (r['y1'] - ay) // c

    def mean(i, j):
        if mistake != 'unclamped_neighbours':
            i, j = np.clip(i, lo_i, hi_i), np.clip(j, lo_j, hi_j)
        exists = ((j >= jmin) & (j <= jmax))[:, None] & ((i >= imin) & (i <= imax))[None, :]
        got = means[(np.clip(j, jmin, jmax) - jmin)[:, None], (np.clip(i, imin, imax) - imin)[None, :]]
        return np.where(exists[:, :, None], got, 0)          # (a cell that does not exist: whatever the read finds)
    d = 2 * c
    return ((d - fx) * (d - fy) * mean(i0, j0) + fx * (d - fy) * mean(i0 + 1, j0) + (d - fx) * fy * mean(i0, j0 + 1) +
            fx * fy * mean(i0 + 1, j0 + 1) + 2 * c * c) // (4 * c * c)


def render(frame, regions, mistake=None):
    """The redacted copy of `frame` (HxWx3 uint8 BGR)."""
    assert mistake is None or mistake in MISTAKES
    h, w = frame.shape[:2]
    out = frame.copy()
    for r in regions:
        r = _fields(r)
        if r['x1'] < r['x0'] or r['y1'] < r['y0']:
            continue
        box = cx0, cy0, cx1, cy1 = max(r['x0'], 0), max(r['y0'], 0), min(r['x1'], w - 1), min(r['y1'], h - 1)
        if cx0 > cx1 or cy0 > cy1:
            continue
        xs, ys = np.arange(cx0, cx1 + 1, dtype=np.int64), np.arange(cy0, cy1 + 1, dtype=np.int64)
        src = out.copy() if mistake == 'reads_earlier_output' else frame
        vals = _values(src, r, box, xs, ys, mistake)
        patch = out[cy0:cy1 + 1, cx0:cx1 + 1]
        patch[...] = np.where(_inside(r, xs, ys, mistake)[:, :, None], np.clip(vals, 0, 255).astype(np.uint8), patch)
    return out
