"""NV12 frames: the host-side handle that MOT.step accepts, and the numpy statement of the conversion that
csrc/nv12.hip computes on the GPU.

NV12 is what hardware video decoders, capture cards and cameras deliver: a full-resolution Y plane (H rows) followed by
a half-resolution plane of interleaved U, V bytes (H / 2 rows of W bytes), usually with a row pitch larger than the
width.  The conversion to BGR is integer arithmetic and exact, so the GPU kernel equals `nv12_to_bgr` bit for bit:

    SHIFT = 20, h = 1 << 19, y = max(Y - 16, 0) * CY, u = U - 128, v = V - 128
    R = sat8((y + h + CVR * v) >> 20)
    G = sat8((y + h + CVG * v + CUG * u) >> 20)
    B = sat8((y + h + CUB * u) >> 20)

with an arithmetic shift, and the chroma sample of a 2 x 2 block used for all four of its pixels (no interpolation).
"""
import numpy as np

SHIFT = 20
# name -> (FM_NV12_* value of include/fastmot_hip.h, (CY, CVR, CUB, CUG, CVG))
MATRICES = {
    'bt601': (0, (1220542, 1673527, 2116026, -409993, -852492)),   # OpenCV's COLOR_YUV2BGR_NV12 constants
    'bt709': (1, (1220945, 1879825, 2215014, -223607, -558796)),   # limited range, round(coef * 2^20)
}


def matrix_id(matrix):
    try:
        return MATRICES[matrix][0]
    except (KeyError, TypeError):
        raise ValueError(f'matrix must be one of {sorted(MATRICES)}, not {matrix!r}') from None


def yuv_to_bgr(y, u, v, matrix='bt601'):
    """Element-wise conversion of equally shaped uint8 arrays Y, U, V -> uint8 array [..., 3] in B, G, R order."""
    matrix_id(matrix)
    cy, cvr, cub, cug, cvg = MATRICES[matrix][1]
    yy = np.maximum(np.asarray(y, np.int32) - 16, 0) * np.int32(cy) + np.int32(1 << (SHIFT - 1))
    uu = np.asarray(u, np.int32) - 128
    vv = np.asarray(v, np.int32) - 128
    out = np.empty(yy.shape + (3,), np.uint8)
    out[..., 2] = np.clip((yy + cvr * vv) >> SHIFT, 0, 255)
    out[..., 1] = np.clip((yy + cvg * vv + cug * uu) >> SHIFT, 0, 255)
    out[..., 0] = np.clip((yy + cub * uu) >> SHIFT, 0, 255)
    return out


def nv12_to_bgr(y, uv, matrix='bt601'):
    """Y plane (H, W) + interleaved UV plane (H / 2, W), both uint8 -> BGR frame (H, W, 3) uint8."""
    y, uv = np.asarray(y), np.asarray(uv)
    _check_planes(y, uv)
    u = np.repeat(np.repeat(uv[:, 0::2], 2, axis=0), 2, axis=1)
    v = np.repeat(np.repeat(uv[:, 1::2], 2, axis=0), 2, axis=1)
    return yuv_to_bgr(y, u, v, matrix)


def bgr_to_nv12(frame):
    """BGR frame (H, W, 3) uint8 with even H and W -> (y, uv): BT.601 limited range, for making NV12 test data.

    Every pixel is converted with the usual 8-bit integer form, rounded to nearest by the + 128 before the shift:
        Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16
        U = ((-38 R - 74 G + 112 B + 128) >> 8) + 128
        V = ((112 R - 94 G - 18 B + 128) >> 8) + 128
    The chroma sample of a 2 x 2 block is the mean of its four pixels' U (V) values rounded half up, (sum + 2) >> 2."""
    frame = np.asarray(frame)
    if frame.ndim != 3 or frame.shape[2] != 3 or frame.dtype != np.uint8:
        raise ValueError('frame must be uint8 HxWx3')
    h, w = frame.shape[:2]
    if h % 2 or w % 2 or not h or not w:
        raise ValueError(f'NV12 needs an even, non-zero frame size, not {w}x{h}')
    b, g, r = (frame[..., i].astype(np.int32) for i in range(3))
    y = (((66 * r + 129 * g + 25 * b + 128) >> 8) + 16).astype(np.uint8)
    u = ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128
    v = ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128
    uv = np.empty((h // 2, w), np.uint8)
    for plane, first in ((u, 0), (v, 1)):
        s = plane[0::2, 0::2] + plane[0::2, 1::2] + plane[1::2, 0::2] + plane[1::2, 1::2]
        uv[:, first::2] = (s + 2) >> 2
    return y, uv


def _check_planes(y, uv):
    if y.dtype != np.uint8 or uv.dtype != np.uint8:
        raise TypeError('NV12 planes must be uint8')
    if y.ndim != 2 or uv.ndim != 2:
        raise ValueError('y must have shape (H, W) and uv shape (H / 2, W)')
    h, w = y.shape
    if h % 2 or w % 2 or not h or not w:
        raise ValueError(f'NV12 needs an even, non-zero frame size, not {w}x{h}')
    if uv.shape != (h // 2, w):
        raise ValueError(f'uv must have shape {(h // 2, w)} for a {w}x{h} frame, not {uv.shape}')


class NV12Frame:
    """Host frame in NV12 layout; MOT.step, the detectors and the ctx frame calls accept it wherever they accept a BGR
    ndarray.  1.5 bytes per pixel cross to the device, where csrc/nv12.hip converts them to the BGR frame every stage reads.

    y: (H, W) uint8, uv: (H / 2, W) uint8 (U, V interleaved); H and W even.  The planes may be views into larger
    arrays: elements of a row are adjacent, and both planes have the same row stride, the `pitch` (>= W).  The planes are
    not copied: they must stay unmodified until the step that uses the frame has returned."""

    def __init__(self, y, uv, matrix='bt601'):
        self.matrix_id = matrix_id(matrix)
        if not isinstance(y, np.ndarray) or not isinstance(uv, np.ndarray):
            raise TypeError('NV12 planes must be ndarrays')
        _check_planes(y, uv)
        h, w = y.shape
        pitch = y.strides[0]
        if y.strides[1] != 1 or uv.strides[1] != 1:
            raise ValueError('the bytes of a row must be adjacent (element stride 1)')
        if pitch < w:
            raise ValueError(f'row stride {pitch} < width {w}')
        if uv.shape[0] > 1 and uv.strides[0] != pitch:      # (the stride of a single row means nothing)
            raise ValueError(f'both planes must have the same row stride: y {pitch}, uv {uv.strides[0]}')
        self.y, self.uv, self.matrix = y, uv, matrix
        self.pitch = pitch
        self.size = (w, h)
        self.shape = (h, w, 3)          # of the BGR frame it becomes on the device

    @classmethod
    def from_buffer(cls, buf, size, pitch=None, uv_offset=None, matrix='bt601'):
        """One contiguous decoder surface: `size` = (W, H), rows `pitch` bytes apart (default W), the UV plane
        `uv_offset` bytes after the start of the Y plane (default pitch * H; decoders that align the Y plane's height
        put it further back)."""
        w, h = size
        if w <= 0 or h <= 0 or w % 2 or h % 2:
            raise ValueError(f'NV12 needs an even, non-zero frame size, not {w}x{h}')
        pitch = w if pitch is None else pitch
        if pitch < w:
            raise ValueError(f'pitch {pitch} < width {w}')
        uv_offset = pitch * h if uv_offset is None else uv_offset
        if uv_offset < pitch * (h - 1) + w:
            raise ValueError(f'uv_offset {uv_offset} lies inside the Y plane')
        if isinstance(buf, np.ndarray):
            if not buf.flags.c_contiguous:
                raise ValueError('NV12 surface must be one contiguous buffer')
            flat = buf.reshape(-1)
        else:
            flat = np.frombuffer(buf, np.uint8)
        if flat.dtype != np.uint8:
            raise TypeError('NV12 surface must be uint8')
        need = uv_offset + pitch * (h // 2 - 1) + w
        if flat.size < need:
            raise ValueError(f'buffer of {flat.size} bytes < {need} bytes of a {w}x{h} surface')
        as_strided = np.lib.stride_tricks.as_strided
        y = as_strided(flat, (h, w), (pitch, 1))
        uv = as_strided(flat[uv_offset:], (h // 2, w), (pitch, 1))
        return cls(y, uv, matrix)
