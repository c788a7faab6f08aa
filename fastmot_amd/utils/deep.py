"""Deep YCbCr frames, 9 to 16 bits per sample: the host-side handle that MOT.step accepts (DeepFrame) and the numpy
statement of what csrc/deep.hip computes on the GPU.

Two layouts of little-endian 16-bit words:

  * planar -- Y, U and V planes of `utils.yuv.chroma_shape` ('420', '422', '444', 'mono'), the sample in the LOW bits:
    libavcodec's yuv420p10le and the payload of a YUV4MPEG2 'C420p10' frame.  Bits above `depth` are masked off.
  * semi-planar -- a Y plane and a plane of interleaved U, V of (H / 2, W) words, the sample in the HIGH bits
    (sample = word >> (16 - depth), the low bits are ignored): P010 / P012 / P016, what a hardware HEVC / AV1 Main10
    decoder delivers.  Even W and H.

The arithmetic, for depth d in 9..16, s = d - 8, limited range:

    y = max(Y - (16 << s), 0) * CY, u = U - (128 << s), v = V - (128 << s), h = 1 << (19 + s)
    R = sat8((y + h + CVR * v) >> (20 + s))
    G = sat8((y + h + CVG * v + CUG * u) >> (20 + s))
    B = sat8((y + h + CUB * u) >> (20 + s))

with arithmetic shifts and 64-bit sums (the largest partial sum at d = 16 is about 2^37.2).  Pixel (r, c) takes the
chroma sample (r >> sv, c >> sh): nearest replication, as `utils.yuv.planar_to_bgr`.  It is integer and exact, so the
GPU kernel equals `deep_to_bgr` bit for bit.  Two properties (tests/test_deep_host.py):

  * shift consistency: for samples that are 8-bit samples shifted left by s the result is `utils.nv12.yuv_to_bgr` of the
    8-bit samples, bit for bit (the shared matrices);
  * closeness to the real-number formula: |result - clipped unrounded float64 value| <= 0.5 + 2^-11 -- three
    coefficients are each off by at most 2^-21 after rounding to 20 fractional bits, times magnitudes below 2^8 --, so the
    result is within 1 of the float64 formula rounded half up.  Measured over 2^22 random triples per (matrix, depth in
    10, 12, 16): the largest deviation was 0.500137 ('bt2020', depth 16; the bound is 0.500488), and the share of
    samples that differ from the rounded float value 2.4e-5 for 'bt709' and 2.7e-5 for 'bt2020'.  For 'bt601' the float
    formula is the one the NV12 constants were rounded from (1.164, 1.596, 2.018, 0.391, 0.813), not the exact BT.601
    ratios; its three-decimal coefficients put real values exactly on a half more often, where the constants, rounded
    down, decide the other way: 3.1e-5 at depth 16, 6.4e-5 at 12, 2.2e-4 at 10.

Not read: full-range deep YCbCr (its scale 255 / (2^d - 1) is no power of two and needs constants per depth), transfer
functions (PQ / HLG: the matrix is applied and nothing else, as for every other frame kind), big-endian samples,
P210 / P410, v210 and other packed 10-bit words.
"""
import ctypes as C

import numpy as np

from .nv12 import MATRICES as _NV12_MATRICES, SHIFT
from .yuv import CHROMAS, chroma_id, chroma_shape, frame_bytes

KR_2020, KB_2020 = 0.2627, 0.0593


def _bt2020():
    kr, kb = KR_2020, KB_2020
    kg = 1 - kr - kb
    c = 255 / 224
    real = (255 / 219, 2 * (1 - kr) * c, 2 * (1 - kb) * c, -2 * (1 - kb) * kb / kg * c, -2 * (1 - kr) * kr / kg * c)
    return tuple(int(round(x * (1 << SHIFT))) for x in real)


# name -> (FM_DEEP_BT* value of include/fastmot_hip.h, (CY, CVR, CUB, CUG, CVG)).  An id space of this family's own:
# `utils.nv12.MATRICES` is the NV12 / planar calls' and has no BT.2020 entry.
MATRICES = {
    'bt601': (0, _NV12_MATRICES['bt601'][1]),
    'bt709': (1, _NV12_MATRICES['bt709'][1]),
    'bt2020': (2, _bt2020()),      # non-constant luminance: (1220945, 1760217, 2245811, -196426, -682019)
}
LAYOUT_PLANAR, LAYOUT_SEMIPLANAR = 0, 1     # FM_DEEP_PLANAR, FM_DEEP_SEMIPLANAR
MIN_DEPTH, MAX_DEPTH = 9, 16


def matrix_id(matrix):
    try:
        return MATRICES[matrix][0]
    except (KeyError, TypeError):
        raise ValueError(f'matrix must be one of {sorted(MATRICES)}, not {matrix!r}') from None


def check_depth(depth):
    if isinstance(depth, bool) or not isinstance(depth, (int, np.integer)) or not MIN_DEPTH <= depth <= MAX_DEPTH:
        raise ValueError(f'depth must be an integer in {MIN_DEPTH}..{MAX_DEPTH}, not {depth!r}')
    return int(depth)


def deep_yuv_to_bgr(y, u, v, depth, matrix='bt709'):
    """Element-wise conversion of equally shaped integer arrays of `depth`-bit samples Y, U, V (bits above `depth` are
    masked off) -> uint8 array [..., 3] in B, G, R order."""
    depth = check_depth(depth)
    matrix_id(matrix)
    cy, cvr, cub, cug, cvg = MATRICES[matrix][1]
    s = depth - 8
    mask = (1 << depth) - 1
    yy = np.maximum((np.asarray(y).astype(np.int64) & mask) - (16 << s), 0) * cy + (1 << (SHIFT - 1 + s))
    uu = (np.asarray(u).astype(np.int64) & mask) - (128 << s)
    vv = (np.asarray(v).astype(np.int64) & mask) - (128 << s)
    out = np.empty(yy.shape + (3,), np.uint8)
    out[..., 2] = np.clip((yy + cvr * vv) >> (SHIFT + s), 0, 255)
    out[..., 1] = np.clip((yy + cvg * vv + cug * uu) >> (SHIFT + s), 0, 255)
    out[..., 0] = np.clip((yy + cub * uu) >> (SHIFT + s), 0, 255)
    return out


def _check_plane(p, name):
    if p.dtype != np.uint16:
        raise TypeError(f'planes must be uint16, {name} is {p.dtype}')
    if p.ndim != 2:
        raise ValueError('planes must be two-dimensional')


def _check_planes(y, u, v, chroma):
    chroma_id(chroma)
    planes = (y,) if chroma == 'mono' else (y, u, v)
    if chroma == 'mono' and (u is not None or v is not None):
        raise ValueError("a 'mono' frame has no chroma planes")
    for name, p in zip('yuv', planes):
        if p is None:
            raise ValueError(f'a {chroma!r} frame needs the planes y, u and v')
        _check_plane(p, name)
    h, w = y.shape
    if not h or not w:
        raise ValueError(f'empty frame {w}x{h}')
    want = chroma_shape((w, h), chroma)
    for name, p in zip('uv', planes[1:]):
        if p.shape != want:
            raise ValueError(f'{name} must have shape {want} for a {w}x{h} {chroma} frame, not {p.shape}')


def _check_semiplanar(y, uv):
    _check_plane(y, 'y')
    _check_plane(uv, 'uv')
    h, w = y.shape
    if h % 2 or w % 2 or not h or not w:
        raise ValueError(f'a semi-planar frame needs an even, non-zero size, not {w}x{h}')
    if uv.shape != (h // 2, w):
        raise ValueError(f'uv must have shape {(h // 2, w)} for a {w}x{h} frame, not {uv.shape}')


def deep_to_bgr(y, u, v, chroma, depth=10, matrix='bt709'):
    """Planar: Y (H, W) and the U, V planes of `chroma` ('420', '422', '444'; 'mono': u = v = None), all uint16 with
    the samples in the low `depth` bits -> BGR frame (H, W, 3) uint8.  Pixel (r, c) uses the chroma sample
    (r >> sv, c >> sh), as `utils.yuv.planar_to_bgr`.  Limited range; matrix 'bt601' / 'bt709' / 'bt2020'."""
    y = np.asarray(y)
    u = None if u is None else np.asarray(u)
    v = None if v is None else np.asarray(v)
    _check_planes(y, u, v, chroma)
    depth = check_depth(depth)
    h, w = y.shape
    if chroma == 'mono':
        full = np.full((h, w), 128 << (depth - 8), np.uint16)
        return deep_yuv_to_bgr(y, full, full, depth, matrix)
    _, sh, sv = CHROMAS[chroma]
    rows, cols = np.arange(h) >> sv, np.arange(w) >> sh
    return deep_yuv_to_bgr(y, u[rows][:, cols], v[rows][:, cols], depth, matrix)


def semiplanar_to_bgr(y, uv, depth=10, matrix='bt709'):
    """P010 / P012 / P016: Y (H, W) and interleaved UV (H / 2, W), uint16 with the samples in the HIGH `depth` bits ->
    BGR frame (H, W, 3) uint8: `deep_to_bgr` of the de-interleaved planes shifted right by 16 - depth, '420'."""
    y, uv = np.asarray(y), np.asarray(uv)
    _check_semiplanar(y, uv)
    rs = 16 - check_depth(depth)
    return deep_to_bgr(y >> rs, uv[:, 0::2] >> rs, uv[:, 1::2] >> rs, '420', depth, matrix)


def deep_frame_bytes(size, chroma):
    """Bytes of one contiguous deep Y, U, V surface (a deep Y4M frame's payload): twice `utils.yuv.frame_bytes`."""
    return 2 * frame_bytes(size, chroma)


class FrameDeep(C.Structure):
    """fm_frame_deep of include/fastmot_hip.h."""
    _fields_ = [('width', C.c_int32), ('height', C.c_int32), ('chroma', C.c_int32), ('matrix', C.c_int32),
                ('depth', C.c_int32), ('layout', C.c_int32),
                ('y', C.c_void_p), ('u', C.c_void_p), ('v', C.c_void_p), ('pitch_y', C.c_int32), ('pitch_c', C.c_int32)]


def _address(arr):
    return arr.__array_interface__['data'][0]


def _pitch(plane, what):
    rows, width = plane.shape
    if plane.strides[1] != 2:
        raise ValueError('the samples of a row must be adjacent (element stride 2 bytes)')
    pitch = plane.strides[0] if rows > 1 else 2 * width       # (the stride of a single row means nothing)
    if pitch < 2 * width:
        raise ValueError(f'{what} row stride {pitch} < the {2 * width} bytes of a row')
    if pitch % 2:
        raise ValueError(f'{what} row stride {pitch} is odd')
    return pitch


def _words(buf, what):
    """`buf` (an ndarray of uint8 or uint16, or anything with the buffer protocol) as a flat uint8 array."""
    if isinstance(buf, np.ndarray):
        if not buf.flags.c_contiguous:
            raise ValueError(f'{what} must be one contiguous buffer')
        if buf.dtype not in (np.uint8, np.uint16):
            raise TypeError(f'{what} must be uint8 or uint16')
        return buf.reshape(-1).view(np.uint8)
    return np.frombuffer(buf, np.uint8)


class DeepFrame:
    """Host frame in 9- to 16-bit YCbCr; MOT.step, the detectors and the ctx frame calls accept it wherever they accept a
    PlanarFrame.  Two bytes per sample (3 per pixel for 4:2:0) cross to the device, where csrc/deep.hip converts them at
    full precision to the BGR frame every stage reads: `to_bgr()` bit for bit.

    DeepFrame(y, u, v, chroma, depth, matrix): planar -- y (H, W) uint16; u, v: uint16 planes of
    `chroma_shape((W, H), chroma)` (None for 'mono'); samples in the low `depth` bits, higher bits are masked off.
    DeepFrame.semiplanar(y, uv, depth, matrix): P010 / P012 / P016 -- uv (H / 2, W) uint16, U and V interleaved; even W
    and H; samples in the high `depth` bits, lower bits are ignored.
    The planes may be views into larger arrays: samples of a row are adjacent, the luma rows are `pitch` BYTES apart
    (even, >= 2 W), the rows of u and of v (of uv) `pitch_c` -- the same for both.  The planes are not copied: they must
    stay unmodified until the step that uses the frame has returned."""

    def __init__(self, y, u=None, v=None, chroma='420', depth=10, matrix='bt709'):
        self.matrix_id = matrix_id(matrix)
        self.chroma_id = chroma_id(chroma)
        self.depth = check_depth(depth)
        for p in (y, u, v):
            if p is not None and not isinstance(p, np.ndarray):
                raise TypeError('planes must be ndarrays')
        if y is None:
            raise ValueError('the y plane is missing')
        _check_planes(y, u, v, chroma)
        h, w = y.shape
        self.pitch = _pitch(y, 'luma')
        self.pitch_c = 0
        if chroma != 'mono':
            self.pitch_c = _pitch(u, 'chroma')
            if _pitch(v, 'chroma') != self.pitch_c:
                raise ValueError(f'u and v must have the same row stride: u {self.pitch_c}, v {v.strides[0]}')
        self.y, self.u, self.v, self.uv = y, u, v, None
        self.layout = 'planar'
        self.chroma, self.matrix = chroma, matrix
        self.size = (w, h)
        self.shape = (h, w, 3)          # of the BGR frame it becomes on the device
        self._desc = None

    @classmethod
    def semiplanar(cls, y, uv, depth=10, matrix='bt709'):
        """P010 (depth 10), P012 (12) or P016 (16): a Y plane and the plane of interleaved U, V."""
        self = cls.__new__(cls)
        self.matrix_id = matrix_id(matrix)
        self.chroma_id = chroma_id('420')
        self.depth = check_depth(depth)
        if not isinstance(y, np.ndarray) or not isinstance(uv, np.ndarray):
            raise TypeError('planes must be ndarrays')
        _check_semiplanar(y, uv)
        h, w = y.shape
        self.pitch = _pitch(y, 'luma')
        self.pitch_c = _pitch(uv, 'chroma')
        self.y, self.u, self.v, self.uv = y, None, None, uv
        self.layout = 'semiplanar'
        self.chroma, self.matrix = '420', matrix
        self.size = (w, h)
        self.shape = (h, w, 3)
        self._desc = None
        return self

    @classmethod
    def from_buffer(cls, buf, size, chroma='420', depth=10, matrix='bt709'):
        """Planar: one contiguous surface -- Y, then U, then V, 16-bit little-endian samples, every row packed to its
        width: the payload of a deep Y4M frame, or a software decoder's picture copied out.  `buf`: uint16 or uint8
        ndarray, or bytes."""
        w, h = size
        if w <= 0 or h <= 0:
            raise ValueError(f'empty frame {w}x{h}')
        cs = chroma_shape(size, chroma)
        flat = _words(buf, 'deep planar surface')
        need = deep_frame_bytes(size, chroma)
        if flat.size < need:
            raise ValueError(f'buffer of {flat.size} bytes < {need} bytes of a {w}x{h} {chroma} 16-bit surface')
        words = flat[:need].view('<u2')
        y = words[:w * h].reshape(h, w)
        if cs is None:
            return cls(y, None, None, chroma, depth, matrix)
        n = cs[0] * cs[1]
        return cls(y, words[w * h:w * h + n].reshape(cs), words[w * h + n:w * h + 2 * n].reshape(cs), chroma, depth, matrix)

    @classmethod
    def semiplanar_from_buffer(cls, buf, size, pitch=None, uv_offset=None, depth=10, matrix='bt709'):
        """Semi-planar: one contiguous decoder surface -- `size` = (W, H), rows `pitch` BYTES apart (default 2 W; even),
        the UV plane `uv_offset` bytes after the start of the Y plane (default pitch * H; even; decoders that align the
        Y plane's height put it further back)."""
        w, h = size
        if w <= 0 or h <= 0 or w % 2 or h % 2:
            raise ValueError(f'a semi-planar frame needs an even, non-zero size, not {w}x{h}')
        pitch = 2 * w if pitch is None else pitch
        if pitch < 2 * w or pitch % 2:
            raise ValueError(f'pitch {pitch} must be even and at least the {2 * w} bytes of a row')
        uv_offset = pitch * h if uv_offset is None else uv_offset
        if uv_offset < pitch * (h - 1) + 2 * w:
            raise ValueError(f'uv_offset {uv_offset} lies inside the Y plane')
        if uv_offset % 2:
            raise ValueError(f'uv_offset {uv_offset} is odd')
        flat = _words(buf, 'semi-planar surface')
        need = uv_offset + pitch * (h // 2 - 1) + 2 * w
        if flat.size < need:
            raise ValueError(f'buffer of {flat.size} bytes < {need} bytes of a {w}x{h} surface')
        y = np.ndarray((h, w), '<u2', flat, 0, (pitch, 2))
        uv = np.ndarray((h // 2, w), '<u2', flat, uv_offset, (pitch, 2))
        return cls.semiplanar(y, uv, depth, matrix)

    def to_bgr(self):
        if self.layout == 'semiplanar':
            return semiplanar_to_bgr(self.y, self.uv, self.depth, self.matrix)
        return deep_to_bgr(self.y, self.u, self.v, self.chroma, self.depth, self.matrix)

    def describe(self):
        """The fm_frame_deep that describes this frame (it points into the planes, which this object keeps alive)."""
        d = self._desc
        if d is None:
            d = FrameDeep(width=self.size[0], height=self.size[1], chroma=self.chroma_id, matrix=self.matrix_id,
                          depth=self.depth, y=_address(self.y), pitch_y=self.pitch, pitch_c=self.pitch_c)
            if self.layout == 'semiplanar':
                d.layout, d.u = LAYOUT_SEMIPLANAR, _address(self.uv)
            else:
                d.layout = LAYOUT_PLANAR
                if self.u is not None:
                    d.u, d.v = _address(self.u), _address(self.v)
            self._desc = d
        return d
