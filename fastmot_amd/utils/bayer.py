"""Bayer frames: the host-side handle that MOT.step accepts for a raw colour-filter mosaic (BayerFrame) -- what
industrial and embedded cameras hand out: GigE Vision / USB3 Vision `BayerRG8` / `BayerRG12`, V4L2 `SRGGB8` / `SRGGB10`,
CSI sensors --, and the numpy statement of what csrc/bayer.hip computes on the GPU.

A frame is `H` rows of `W` samples, one per pixel, `pitch` bytes apart: uint8 for depth 8, little-endian uint16 with the
value in the low bits for depths 10, 12, 14 and 16 (the unpacked form of `SRGGB10` / `BayerRG12`).

Pattern: the 2 x 2 tile, with an id that says where R sits (FM_BAYER_* of include/fastmot_hip.h):
    'rggb' (0)  R G     'grbg' (1)  G R     'gbrg' (2)  G B     'bggr' (3)  B G
                G B                 B G                 R G                 G R
bit 0 of the id is the column parity of R, bit 1 its row parity; B sits at the opposite parity in both directions, G at
the other two positions.

Sample preparation, per sample and before any interpolation: with the black level `black` (0 <= black < 2^depth) and
the white-balance gain of the colour the sample's position carries, in 1/256 units (1 <= gain <= 4096, 256 = 1.0),
    v = max(s - black, 0)        p = min(255, (v * gain + (1 << (depth - 1))) >> depth)
which is p == s for the defaults at depth 8; every product stays below 2^28.

Borders: index reflection without repeating the edge (reflect-101) in both directions, `reflect(i, n)`: with
m = 2 (n - 1), i <- i mod m, and i <- m - i where i >= n.  m is even, so a reflected index keeps its parity -- its
colour --, which is why width and height must be >= 2 (a one-sample-wide mosaic has no second colour); odd sizes (a
cropped ROI) are fine.

Methods.  A position's own colour is p unchanged.  With c the centre sample, N, S, E, W its neighbours, card their sum,
hor = E + W, ver = N + S, diag the sum of the four diagonals, h2 / v2 the sums of the two samples at distance 2
horizontally / vertically:
    'bilinear' (0)   G at R / B: (card + 2) >> 2;   R / B at G: (a + b + 1) >> 1 of the two neighbours of that colour (left
                     and right in the row that holds the colour, above and below otherwise);   R at B, B at R: (diag + 2) >> 2
    'mhc' (1)        Malvar-He-Cutler's gradient-corrected 5 x 5 filters in sixteenths, clip((sum + 8) >> 4, 0, 255) of
                     G at R / B                                   8 c + 4 card - 2 (h2 + v2)
                     R / B at G, that colour left and right      10 c + 8 hor - 2 diag - 2 h2 + v2
                     R / B at G, that colour above and below     10 c + 8 ver - 2 diag - 2 v2 + h2
                     R at B, B at R                              12 c + 4 diag - 3 (h2 + v2)
                     (|sum| <= 28 * 255; the shift is arithmetic)
All of it is integer and exact, so the GPU kernel equals `bayer_to_bgr` bit for bit.  'mhc' is the better picture where
the channels are correlated, as they are in photographs; on channels that have nothing to do with each other it is the
worse one, which is why the method is a parameter.
"""
import ctypes as C

import numpy as np

PATTERNS = {'rggb': 0, 'grbg': 1, 'gbrg': 2, 'bggr': 3}
METHODS = {'bilinear': 0, 'mhc': 1}
DEPTHS = (8, 10, 12, 14, 16)
GAIN_MAX = 4096         # in 1/256 units


def pattern_id(pattern):
    try:
        return PATTERNS[pattern]
    except (KeyError, TypeError):
        raise ValueError(f'pattern must be one of {sorted(PATTERNS)}, not {pattern!r}') from None


def method_id(method):
    try:
        return METHODS[method]
    except (KeyError, TypeError):
        raise ValueError(f'method must be one of {sorted(METHODS)}, not {method!r}') from None


def _depth(depth):
    if depth not in DEPTHS or isinstance(depth, bool):
        raise ValueError(f'depth must be one of {DEPTHS}, not {depth!r}')
    return int(depth)


def gains(wb):
    """White-balance factors (R, G, B) -> the integer gains in 1/256 units the arithmetic uses."""
    try:
        r, g, b = (float(x) for x in wb)
    except (TypeError, ValueError):
        raise ValueError(f'wb must be three gains (R, G, B), not {wb!r}') from None
    out = tuple(int(round(256. * x)) if np.isfinite(x) else 0 for x in (r, g, b))
    if not all(1 <= x <= GAIN_MAX for x in out):
        raise ValueError(f'wb gains {wb!r} outside 1/256 .. 16')
    return out


def _black(black, depth):
    if int(black) != black or not 0 <= black < (1 << depth):
        raise ValueError(f'black level {black!r} outside 0..{(1 << depth) - 1}')
    return int(black)


def reflect(i, n):
    """Reflect-101 of the indices `i` into 0..n-1 (n >= 2)."""
    m = 2 * (n - 1)
    i = np.mod(i, m)
    return np.where(i >= n, m - i, i)


def colour_planes(size, pattern):
    """Boolean (H, W) masks of the positions that carry R, G and B."""
    pid = pattern_id(pattern)
    w, h = size
    cx = ((np.arange(w) ^ pid) & 1)[None, :]             # 0: a column R sits in
    cy = ((np.arange(h) ^ (pid >> 1)) & 1)[:, None]      # 0: a row R sits in
    is_r, is_b = (cx == 0) & (cy == 0), (cx == 1) & (cy == 1)
    return is_r, ~(is_r | is_b), is_b


def _rows(data, size, depth):
    """`data` as an (H, >= W) view of samples."""
    depth = _depth(depth)
    data = np.asarray(data)
    want = np.uint8 if depth == 8 else np.uint16
    if data.dtype != want or (data.dtype.itemsize > 1 and data.dtype.byteorder == '>'):
        raise TypeError(f'samples of depth {depth} must be {"uint8" if depth == 8 else "little-endian uint16"}, not {data.dtype}')
    if data.ndim != 2:
        raise ValueError(f'a mosaic is an (H, W) or an (H, pitch) array, not {data.shape}')
    if size is None:
        w, h = data.shape[1], data.shape[0]
    else:
        w, h = int(size[0]), int(size[1])
    if w < 2 or h < 2:
        raise ValueError(f'a mosaic is at least 2x2, not {w}x{h}')
    if data.shape[0] != h:
        raise ValueError(f'array of {data.shape[0]} rows, size says {h}')
    if data.strides[1] != data.dtype.itemsize:
        raise ValueError('the samples of a row must be adjacent')
    if data.shape[1] < w:
        raise ValueError(f'rows of {data.shape[1]} samples < {w}')
    return data, (w, h)


def prepare(samples, size, pattern, depth=8, gain=(256, 256, 256), black=0):
    """The prepared 8-bit samples (H, W) int32: black level, the position's gain, the depth."""
    w, h = size
    s = np.asarray(samples)[:h, :w].astype(np.int64)
    g = np.zeros((h, w), np.int64)
    for mask, value in zip(colour_planes(size, pattern), gain):
        g[mask] = value
    v = np.maximum(s - black, 0)
    return np.minimum(255, (v * g + (1 << (depth - 1))) >> depth).astype(np.int32)


def demosaic(p, pattern, method='mhc'):
    """Prepared samples (H, W) -> BGR (H, W, 3) uint8."""
    mid = method_id(method)
    p = np.asarray(p, np.int32)
    h, w = p.shape
    pad = p[np.ix_(reflect(np.arange(-2, h + 2), h), reflect(np.arange(-2, w + 2), w))]

    def at(dy, dx):
        return pad[2 + dy:2 + dy + h, 2 + dx:2 + dx + w]

    c = at(0, 0)
    hor, ver = at(0, -1) + at(0, 1), at(-1, 0) + at(1, 0)
    card = hor + ver
    diag = at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1)
    if mid == METHODS['bilinear']:
        g_at_site, other_at_site = (card + 2) >> 2, (diag + 2) >> 2
        lr_at_g, ud_at_g = (hor + 1) >> 1, (ver + 1) >> 1
    else:
        h2, v2 = at(0, -2) + at(0, 2), at(-2, 0) + at(2, 0)
        fin = lambda s: np.clip((s + 8) >> 4, 0, 255)
        g_at_site = fin(8 * c + 4 * card - 2 * (h2 + v2))
        other_at_site = fin(12 * c + 4 * diag - 3 * (h2 + v2))
        lr_at_g = fin(10 * c + 8 * hor - 2 * diag - 2 * h2 + v2)
        ud_at_g = fin(10 * c + 8 * ver - 2 * diag - 2 * v2 + h2)
    is_r, is_g, is_b = colour_planes((w, h), pattern)
    r_row = np.broadcast_to(((np.arange(h) ^ (PATTERNS[pattern] >> 1)) & 1)[:, None] == 0, (h, w))   # rows R sits in
    out = np.empty((h, w, 3), np.uint8)
    red = np.where(is_r, c, np.where(is_b, other_at_site, np.where(r_row, lr_at_g, ud_at_g)))
    blue = np.where(is_b, c, np.where(is_r, other_at_site, np.where(r_row, ud_at_g, lr_at_g)))
    out[..., 2], out[..., 1], out[..., 0] = red, np.where(is_g, c, g_at_site), blue
    return out


def bayer_to_bgr(data, size, pattern, depth=8, method='mhc', wb=(1., 1., 1.), black=0):
    """Bayer mosaic -> BGR frame (H, W, 3) uint8.  data: (H, >= W) uint8 (depth 8) or uint16 samples; size: (W, H), or
    None for the array's own; pattern: a key of PATTERNS; method: a key of METHODS; wb: gains (R, G, B), quantised to
    1/256; black: the black level in sample units."""
    pattern_id(pattern)
    method_id(method)
    rows, (w, h) = _rows(data, size, depth)
    return demosaic(prepare(rows, (w, h), pattern, depth, gains(wb), _black(black, depth)), pattern, method)


def mosaic(bgr, pattern):
    """The inverse sampling: BGR (H, W, 3) -> the (H, W) mosaic that keeps, at every position, the channel it carries."""
    bgr = np.asarray(bgr)
    if bgr.ndim != 3 or bgr.shape[2] != 3:
        raise ValueError('frame must be HxWx3')
    is_r, is_g, is_b = colour_planes(bgr.shape[1::-1], pattern)
    return np.where(is_r, bgr[..., 2], np.where(is_b, bgr[..., 0], bgr[..., 1])).astype(bgr.dtype)


class FrameBayer(C.Structure):
    """fm_frame_bayer of include/fastmot_hip.h."""
    _fields_ = [('pattern', C.c_int32), ('width', C.c_int32), ('height', C.c_int32), ('pitch', C.c_int32), ('depth', C.c_int32),
                ('method', C.c_int32), ('black', C.c_int32), ('gain_r', C.c_int32), ('gain_g', C.c_int32), ('gain_b', C.c_int32),
                ('data', C.c_void_p)]


class BayerFrame:
    """Host frame that is a raw Bayer mosaic; MOT.step, the detectors and the ctx frame calls accept it wherever they
    accept a PackedFrame.  The samples cross to the device as they are (1 byte per pixel at depth 8, 2 above), where
    csrc/bayer.hip demosaics them into the BGR frame every stage reads: `to_bgr()` bit for bit.

    data: (H, W) uint8, or (H, pitch) uint8 with `size` = (W, H), for depth 8; (H, W) uint16 for depths 10, 12, 14 and 16
    -- possibly a view into a larger array: the samples of a row are adjacent, the rows `pitch` bytes apart.  It is not
    copied: it must stay unmodified until the step that uses the frame has returned.  wb: white-balance gains (R, G, B),
    quantised to round(256 g); black: the black level in sample units."""

    def __init__(self, data, pattern, size=None, depth=8, method='mhc', wb=(1., 1., 1.), black=0):
        self.pattern_id = pattern_id(pattern)
        self.method_id = method_id(method)
        if not isinstance(data, np.ndarray):
            raise TypeError('a mosaic must be an ndarray')
        rows, (w, h) = _rows(data, size, depth)
        self.gains = gains(wb)
        self.black = _black(black, depth)
        need = w * rows.dtype.itemsize
        pitch = rows.strides[0]
        if pitch < need:
            raise ValueError(f'row stride {pitch} < the {need} bytes of a row')
        self.data, self.rows = data, rows[:, :w]
        self.pattern, self.method, self.depth = pattern, method, int(depth)
        self.pitch = pitch
        self.size = (w, h)
        self.shape = (h, w, 3)          # of the BGR frame it becomes on the device
        self._desc = None

    @classmethod
    def from_buffer(cls, buf, size, pattern, pitch=None, depth=8, method='mhc', wb=(1., 1., 1.), black=0):
        """One contiguous surface: `size` = (W, H), rows `pitch` bytes apart (default: the bytes of a row)."""
        pattern_id(pattern)
        bps = 1 if _depth(depth) == 8 else 2
        w, h = size
        if w < 2 or h < 2:
            raise ValueError(f'a mosaic is at least 2x2, not {w}x{h}')
        need = w * bps
        pitch = need if pitch is None else pitch
        if pitch < need:
            raise ValueError(f'pitch {pitch} < the {need} bytes of a row')
        if pitch % bps:
            raise ValueError(f'pitch {pitch} is no multiple of the {bps} bytes of a sample')
        if isinstance(buf, np.ndarray):
            if not buf.flags.c_contiguous:
                raise ValueError('a mosaic surface must be one contiguous buffer')
            if buf.dtype.itemsize not in (1, bps) or buf.dtype.kind != 'u':
                raise TypeError(f'a mosaic surface of depth {depth} must be uint8' + (' or uint16' if bps == 2 else ''))
            flat = buf.reshape(-1).view(np.uint8)
        else:
            flat = np.frombuffer(buf, np.uint8)
        total = pitch * (h - 1) + need
        if flat.size < total:
            raise ValueError(f'buffer of {flat.size} bytes < {total} bytes of a {w}x{h} surface of depth {depth}')
        if bps == 2:
            if flat.__array_interface__['data'][0] & 1:
                raise ValueError('16-bit samples must lie at an even address')
            flat = flat[:flat.size & ~1].view('<u2')
        rows = np.lib.stride_tricks.as_strided(flat, (h, w), (pitch, bps))
        return cls(rows, pattern, (w, h), depth, method, wb, black)

    def to_bgr(self):
        return demosaic(prepare(self.rows, self.size, self.pattern, self.depth, self.gains, self.black), self.pattern, self.method)

    def describe(self):
        """The fm_frame_bayer that describes this frame (it points into the array, which this object keeps alive)."""
        d = self._desc
        if d is None:
            d = FrameBayer(pattern=self.pattern_id, width=self.size[0], height=self.size[1], pitch=self.pitch, depth=self.depth,
                           method=self.method_id, black=self.black, gain_r=self.gains[0], gain_g=self.gains[1],
                           gain_b=self.gains[2], data=self.rows.__array_interface__['data'][0])
            self._desc = d
        return d
