"""Packed frames: the host-side handle that MOT.step accepts for packed 4:2:2 (YUY2 / UYVY / YVYU) and for packed RGB
in any channel order, with or without a fourth byte (PackedFrame), and the numpy statement of what csrc/packed.hip
computes on the GPU.

Packed 4:2:2 is the raw format of every UVC / V4L2 camera and of most capture cards; RGB is what Pillow, imageio and
torchvision deliver, BGRx what `nvvidconv` / `appsink` hand out.  A frame is `H` rows of `row_bytes(W, fmt)` bytes,
`pitch` >= that apart:

    RGB family     bytes per pixel, byte offsets of R, G, B (a fourth byte is ignored)
      'rgb'            3   0 1 2        'bgr'            3   2 1 0
      'rgbx' / 'rgba'  4   0 1 2        'bgrx' / 'bgra'  4   2 1 0
      'xrgb' / 'argb'  4   1 2 3        'xbgr' / 'abgr'  4   3 2 1
    the output is the byte permutation into B, G, R; no matrix is involved.

    4:2:2 family   one 4-byte macropixel carries two horizontally adjacent pixels
      'yuy2' / 'yuyv'  Y0 U Y1 V        'uyvy'  U Y0 V Y1        'yvyu'  Y0 V Y1 U
    a row holds ceil(W / 2) macropixels; for an odd W the last macropixel's second luma byte is no pixel.  Pixel (r, c)
    uses luma sample c of its row and the U, V of macropixel c >> 1: nearest replication, `planar_to_bgr(..., '422')`.

Matrices, in an id space of this family's own (FM_PACKED_* of include/fastmot_hip.h):
    'bt601' (0), 'bt709' (1): limited range, the constants and formula of `utils.nv12.yuv_to_bgr`;
    'bt601-full' (16), 'bt709-full' (17): full ("JPEG") range,
        y = Y << 20, u = U - 128, v = V - 128, h = 1 << 19
        R = sat8((y + h + CVR v) >> 20)   G = sat8((y + h + CVG v + CUG u) >> 20)   B = sat8((y + h + CUB u) >> 20)
    with round(c * 2^20) of BT.601's 1.402, 1.772, -0.344136, -0.714136 and BT.709's 1.5748, 1.8556, -0.187324,
    -0.468124 for CVR, CUB, CUG, CVG.  Every partial sum fits 32 bits: |y + h| < 2^28.1, |C * 128| < 2^27.9 per term.
All of it is integer and exact, so the GPU kernels equal `packed_to_bgr` bit for bit.
"""
import ctypes as C

import numpy as np

from .nv12 import SHIFT, yuv_to_bgr

# name -> (FM_PACKED_* format id, family, bytes per pixel (of a macropixel's half: 2), layout)
#   'rgb' family: layout = byte offsets of R, G, B; '422' family: layout = byte offsets of Y0, U, V (Y1 = Y0 + 2)
FORMATS = {
    'rgb': (0, 'rgb', 3, (0, 1, 2)), 'bgr': (1, 'rgb', 3, (2, 1, 0)),
    'rgbx': (2, 'rgb', 4, (0, 1, 2)), 'bgrx': (3, 'rgb', 4, (2, 1, 0)),
    'xrgb': (4, 'rgb', 4, (1, 2, 3)), 'xbgr': (5, 'rgb', 4, (3, 2, 1)),
    'yuy2': (6, '422', 2, (0, 1, 3)), 'uyvy': (7, '422', 2, (1, 0, 2)), 'yvyu': (8, '422', 2, (0, 3, 1)),
}
for _alias, _name in (('rgba', 'rgbx'), ('bgra', 'bgrx'), ('argb', 'xrgb'), ('abgr', 'xbgr'), ('yuyv', 'yuy2')):
    FORMATS[_alias] = FORMATS[_name]

# name -> FM_PACKED_BT* id.  (`utils.nv12.MATRICES` is the NV12 / planar calls' id space and has no full-range entry.)
MATRICES = {'bt601': 0, 'bt709': 1, 'bt601-full': 16, 'bt709-full': 17}
# full range: (CVR, CUB, CUG, CVG)
FULL_COEF = {
    'bt601-full': (1470104, 1858077, -360853, -748826),
    'bt709-full': (1651297, 1945738, -196423, -490864),
}


def format_id(fmt):
    try:
        return FORMATS[fmt][0]
    except (KeyError, TypeError):
        raise ValueError(f'format must be one of {sorted(FORMATS)}, not {fmt!r}') from None


def matrix_id(matrix):
    try:
        return MATRICES[matrix]
    except (KeyError, TypeError):
        raise ValueError(f'matrix must be one of {sorted(MATRICES)}, not {matrix!r}') from None


def row_bytes(width, fmt):
    """Bytes of one row of `width` pixels: bpp * width, or 4 * ceil(width / 2) for the 4:2:2 family."""
    format_id(fmt)
    _, family, bpp, _ = FORMATS[fmt]
    return 4 * ((width + 1) // 2) if family == '422' else bpp * width


def full_range_to_bgr(y, u, v, matrix):
    """Element-wise full-range conversion of equally shaped uint8 arrays Y, U, V -> uint8 array [..., 3] in B, G, R order."""
    cvr, cub, cug, cvg = FULL_COEF[matrix]
    yy = (np.asarray(y, np.int32) << SHIFT) + np.int32(1 << (SHIFT - 1))
    uu = np.asarray(u, np.int32) - 128
    vv = np.asarray(v, np.int32) - 128
    out = np.empty(yy.shape + (3,), np.uint8)
    out[..., 2] = np.clip((yy + cvr * vv) >> SHIFT, 0, 255)
    out[..., 1] = np.clip((yy + cvg * vv + cug * uu) >> SHIFT, 0, 255)
    out[..., 0] = np.clip((yy + cub * uu) >> SHIFT, 0, 255)
    return out


def _rows(data, size, fmt):
    """`data` as an (H, >= row bytes) uint8 view."""
    format_id(fmt)
    data = np.asarray(data)
    if data.dtype != np.uint8:
        raise TypeError('packed pixels must be uint8')
    w, h = (int(size[0]), int(size[1])) if size is not None else (None, None)
    _, family, bpp, _ = FORMATS[fmt]
    if data.ndim == 3:
        if family != 'rgb' or data.shape[2] != bpp:
            raise ValueError(f'a three-dimensional array must be (H, W, {bpp}) of an RGB-family format; {fmt!r} got {data.shape}')
        if size is not None and (data.shape[1], data.shape[0]) != (w, h):
            raise ValueError(f'array of {data.shape[1]}x{data.shape[0]} pixels, size says {w}x{h}')
        h, w = data.shape[:2]
        if not h or not w:
            raise ValueError(f'empty frame {w}x{h}')
        if data.strides[2] != 1 or data.strides[1] != bpp:
            raise ValueError('the bytes of a row must be adjacent')
        data = np.lib.stride_tricks.as_strided(data, (h, w * bpp), (data.strides[0], 1))
    elif data.ndim == 2:
        if size is None:
            raise ValueError('an (H, pitch) array of bytes needs `size` = (W, H)')
        if w <= 0 or h <= 0:
            raise ValueError(f'empty frame {w}x{h}')
        if data.shape[0] != h:
            raise ValueError(f'array of {data.shape[0]} rows, size says {h}')
        if data.shape[1] and data.strides[1] != 1:
            raise ValueError('the bytes of a row must be adjacent (element stride 1)')
        if data.shape[1] < row_bytes(w, fmt):
            raise ValueError(f'rows of {data.shape[1]} bytes < {row_bytes(w, fmt)} bytes of {w} {fmt} pixels')
    else:
        raise ValueError('packed pixels must be an (H, W, bpp) or an (H, pitch) array')
    return data, (w, h)


def packed_to_bgr(data, size, fmt, matrix='bt601'):
    """Packed frame -> BGR frame (H, W, 3) uint8.  data: (H, pitch) uint8 with pitch >= row_bytes(W, fmt), or (H, W, bpp)
    for the RGB family (`size` may then be None); size: (W, H); fmt: a key of FORMATS; matrix: a key of MATRICES (not used
    by the RGB family)."""
    matrix_id(matrix)
    rows, (w, h) = _rows(data, size, fmt)
    _, family, bpp, layout = FORMATS[fmt]
    if family == 'rgb':
        px = rows[:, :w * bpp].reshape(h, w, bpp)
        r, g, b = layout
        return np.ascontiguousarray(px[..., [b, g, r]])
    y0, uo, vo = layout
    cols = np.arange(w)
    mp = rows[:, :4 * ((w + 1) // 2)].reshape(h, -1, 4)
    y = mp[:, cols >> 1, y0 + 2 * (cols & 1)]
    u, v = mp[:, cols >> 1, uo], mp[:, cols >> 1, vo]
    if matrix in FULL_COEF:
        return full_range_to_bgr(y, u, v, matrix)
    return yuv_to_bgr(y, u, v, matrix)


class FramePacked(C.Structure):
    """fm_frame_packed of include/fastmot_hip.h."""
    _fields_ = [('format', C.c_int32), ('width', C.c_int32), ('height', C.c_int32), ('pitch', C.c_int32), ('matrix', C.c_int32),
                ('data', C.c_void_p)]


class PackedFrame:
    """Host frame in a packed layout; MOT.step, the detectors and the ctx frame calls accept it wherever they accept a
    PlanarFrame.  The rows cross to the device as they are (2 bytes per pixel for 4:2:2, 3 or 4 for RGB), where
    csrc/packed.hip converts them to the BGR frame every stage reads: `to_bgr()` bit for bit.

    data: (H, W, bpp) uint8 for the RGB family, or (H, pitch) uint8 with `size` = (W, H) for any format -- possibly a view
    into a larger array: the bytes of a row are adjacent, the rows `pitch` >= row_bytes(W, fmt) apart.  It is not copied:
    it must stay unmodified until the step that uses the frame has returned."""

    def __init__(self, data, fmt, size=None, matrix='bt601'):
        self.format_id = format_id(fmt)
        self.matrix_id = matrix_id(matrix)
        if not isinstance(data, np.ndarray):
            raise TypeError('packed pixels must be an ndarray')
        rows, (w, h) = _rows(data, size, fmt)
        need = row_bytes(w, fmt)
        pitch = rows.strides[0] if h > 1 else need           # (the stride of a single row means nothing)
        if pitch < need:
            raise ValueError(f'row stride {pitch} < the {need} bytes of a row')
        self.data, self.rows = data, rows
        self.format, self.matrix = fmt, matrix
        self.pitch = pitch
        self.size = (w, h)
        self.shape = (h, w, 3)          # of the BGR frame it becomes on the device
        self._desc = None

    @classmethod
    def from_buffer(cls, buf, size, fmt, pitch=None, matrix='bt601'):
        """One contiguous surface: `size` = (W, H), rows `pitch` bytes apart (default: row_bytes(W, fmt))."""
        format_id(fmt)
        w, h = size
        if w <= 0 or h <= 0:
            raise ValueError(f'empty frame {w}x{h}')
        need = row_bytes(w, fmt)
        pitch = need if pitch is None else pitch
        if pitch < need:
            raise ValueError(f'pitch {pitch} < the {need} bytes of a row')
        if isinstance(buf, np.ndarray):
            if not buf.flags.c_contiguous:
                raise ValueError('packed surface must be one contiguous buffer')
            flat = buf.reshape(-1)
        else:
            flat = np.frombuffer(buf, np.uint8)
        if flat.dtype != np.uint8:
            raise TypeError('packed surface must be uint8')
        total = pitch * (h - 1) + need
        if flat.size < total:
            raise ValueError(f'buffer of {flat.size} bytes < {total} bytes of a {w}x{h} {fmt} surface')
        return cls(np.lib.stride_tricks.as_strided(flat, (h, need), (pitch, 1)), fmt, (w, h), matrix)

    def to_bgr(self):
        return packed_to_bgr(self.rows, self.size, self.format, self.matrix)

    def describe(self):
        """The fm_frame_packed that describes this frame (it points into the array, which this object keeps alive)."""
        d = self._desc
        if d is None:
            d = FramePacked(format=self.format_id, width=self.size[0], height=self.size[1], pitch=self.pitch,
                            matrix=self.matrix_id, data=self.rows.__array_interface__['data'][0])
            self._desc = d
        return d
