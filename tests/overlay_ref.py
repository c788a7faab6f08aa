"""The overlay command list in numpy: what fm_overlay_render_host and the kernel of csrc/overlay.hip must compute.

No Pillow in here -- tests/test_overlay_host.py pins every rule below against Pillow's ImageDraw, and the C code against
this file.  Commands are rows of fastmot_amd._lib.OVERLAY_CMD_DTYPE (fm_overlay_cmd), applied in order; colours BGR."""
import numpy as np

from fastmot_amd._lib import OVERLAY_CMD_DTYPE, OVL_RECT_FILL, OVL_RECT_OUTLINE, OVL_LINE, OVL_DOT, OVL_MASK


def cmd(kind, x0, y0, x1=0, y1=0, color=(0, 0, 0), thickness=1, mask_off=0):
    out = np.zeros(1, OVERLAY_CMD_DTYPE)
    out['kind'], out['x0'], out['y0'], out['x1'], out['y1'] = kind, x0, y0, x1, y1
    out['color'], out['thickness'], out['mask_off'] = color, thickness, mask_off
    return out


def rect_fill(x0, y0, x1, y1, color):
    return cmd(OVL_RECT_FILL, x0, y0, x1, y1, color)


def rect_outline(x0, y0, x1, y1, color, thickness=1):
    return cmd(OVL_RECT_OUTLINE, x0, y0, x1, y1, color, thickness)


def line(x0, y0, x1, y1, color):
    return cmd(OVL_LINE, x0, y0, x1, y1, color)


def dot(x, y, color):
    return cmd(OVL_DOT, x, y, color=color)


def mask(x, y, alpha, color, blob):
    """MASK command for the 2-D uint8 `alpha` at (x, y); appends its bytes to the bytearray `blob`."""
    off = len(blob)
    blob += np.ascontiguousarray(alpha, np.uint8).tobytes()
    return cmd(OVL_MASK, x, y, alpha.shape[1], alpha.shape[0], color, mask_off=off)


def line_points(x0, y0, x1, y1):
    """Bresenham with the error term e = 2 minor - major and a minor step when e >= 0 before the add, both ends included,
    in closed form: i steps along the major axis the minor axis has moved (2 minor i + major) // (2 major)."""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    xs, ys = (1 if x1 >= x0 else -1), (1 if y1 >= y0 else -1)
    if dx > dy:
        i = np.arange(dx + 1, dtype=np.int64)
        return x0 + xs * i, y0 + ys * ((2 * dy * i + dx) // (2 * dx))
    i = np.arange(dy + 1, dtype=np.int64)
    if dy == 0:
        return np.array([x0], np.int64), np.array([y0], np.int64)
    return x0 + xs * ((2 * dx * i + dy) // (2 * dy)), y0 + ys * i


def line_points_stepwise(x0, y0, x1, y1):
    """The same line by running the error term, as a rasteriser does (the closed form is checked against this)."""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    xs, ys = (1 if x1 >= x0 else -1), (1 if y1 >= y0 else -1)
    pts = []
    x, y = x0, y0
    if dx > dy:
        e = 2 * dy - dx
        for _ in range(dx):
            pts.append((x, y))
            if e >= 0:
                y += ys
                e -= 2 * dx
            e += 2 * dy
            x += xs
    else:
        e = 2 * dx - dy
        for _ in range(dy):
            pts.append((x, y))
            if e >= 0:
                x += xs
                e -= 2 * dy
            e += 2 * dx
            y += ys
    pts.append((x1, y1))
    return pts


def _put(frame, xs, ys, color):
    h, w = frame.shape[:2]
    xs, ys = np.asarray(xs, np.int64).ravel(), np.asarray(ys, np.int64).ravel()
    ok = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
    frame[ys[ok], xs[ok]] = color


def _span(frame, x0, x1, y0, y1, color):
    """Every pixel of [x0, x1] x [y0, y1] (inclusive, clipped)."""
    h, w = frame.shape[:2]
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w - 1), min(y1, h - 1)
    if x0 <= x1 and y0 <= y1:
        frame[y0:y1 + 1, x0:x1 + 1] = color


def render(frame, cmds, masks=b''):
    """Applies the list to `frame` (HxWx3 uint8 BGR) in place and returns it."""
    h, w = frame.shape[:2]
    masks = np.frombuffer(bytes(masks), np.uint8)
    for c in np.asarray(cmds, OVERLAY_CMD_DTYPE).reshape(-1):
        kind, x0, y0, x1, y1 = (int(c[k]) for k in ('kind', 'x0', 'y0', 'x1', 'y1'))
        color = c['color']
        if kind == OVL_RECT_FILL:
            _span(frame, x0, x1, y0, y1, color)
        elif kind == OVL_RECT_OUTLINE:
            if x1 < x0 or y1 < y0:
                continue
            t = int(c['thickness'])
            for i in range(t):
                _span(frame, x0, x1, y0 + i, y0 + i, color)
                _span(frame, x0, x1, y1 - i, y1 - i, color)
                # the sides: lines WITHOUT their last point from y0 + t towards y1 - t + 1
                ya, yb = y0 + t, y1 - t + 1
                lo, hi = (ya, yb - 1) if yb > ya else (yb + 1, ya)
                for x in (x1 - i, x0 + i):
                    _span(frame, x, x, lo, hi, color)
        elif kind == OVL_LINE:
            _put(frame, *line_points(x0, y0, x1, y1), color)
        elif kind == OVL_DOT:
            _put(frame, [x0, x0 - 1, x0 + 1, x0, x0], [y0, y0, y0, y0 - 1, y0 + 1], color)
        elif kind == OVL_MASK:
            mw, mh = x1, y1
            m = masks[int(c['mask_off']):int(c['mask_off']) + mw * mh].reshape(mh, mw).astype(np.uint32)
            cx0, cy0, cx1, cy1 = max(x0, 0), max(y0, 0), min(x0 + mw, w), min(y0 + mh, h)
            if cx0 >= cx1 or cy0 >= cy1:
                continue
            m = m[cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0, None]
            bg = frame[cy0:cy1, cx0:cx1].astype(np.uint32)
            t = m * color.astype(np.uint32) + (255 - m) * bg + 128
            frame[cy0:cy1, cx0:cx1] = ((t + (t >> 8)) >> 8).astype(np.uint8)
        else:
            raise ValueError(f'unknown kind {kind}')
    return frame
