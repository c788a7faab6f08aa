"""Planar YCbCr frames and YUV4MPEG2 (.y4m) text: the host-side handle that MOT.step accepts (PlanarFrame), the numpy
statement of what csrc/yuv.hip computes on the GPU in both directions, and the header of the one video container that
needs no codec.

Planar I420 is what software decoders (libavcodec, libvpx, dav1d) hand out and what `ffmpeg -f yuv4mpegpipe`, mpv and
the x264 tooling write: a Y plane (H, W), then a U and a V plane of

    '420': ((H + 1) // 2, (W + 1) // 2)    '422': (H, (W + 1) // 2)    '444': (H, W)    'mono': none (U = V = 128)

samples.  Odd sizes are legal: the chroma planes round up.  In: pixel (r, c) takes the chroma sample (r >> sv, c >> sh)
and is converted by `utils.nv12.yuv_to_bgr` -- NV12's arithmetic, matrices and ids.  Out: `bgr_to_planar420`, the 8-bit
BT.601 form `utils.nv12.bgr_to_nv12` documents.  Both are integer and exact, so the GPU kernels equal them bit for bit.
"""
import ctypes as C
from fractions import Fraction

import numpy as np

from .nv12 import matrix_id, yuv_to_bgr

# name -> (FM_YUV_* value of include/fastmot_hip.h, log2 of the columns, of the rows per chroma sample)
CHROMAS = {'420': (0, 1, 1), '422': (1, 1, 0), '444': (2, 0, 0), 'mono': (3, 0, 0)}


def chroma_id(chroma):
    try:
        return CHROMAS[chroma][0]
    except (KeyError, TypeError):
        raise ValueError(f'chroma must be one of {sorted(CHROMAS)}, not {chroma!r}') from None


def chroma_shape(size, chroma):
    """(rows, columns) of the U and V planes of a `size` = (W, H) frame; None for 'mono'."""
    chroma_id(chroma)
    if chroma == 'mono':
        return None
    _, sh, sv = CHROMAS[chroma]
    w, h = size
    return ((h + (1 << sv) - 1) >> sv, (w + (1 << sh) - 1) >> sh)


def frame_bytes(size, chroma):
    """Bytes of one contiguous Y, U, V surface (a Y4M frame's payload)."""
    cs = chroma_shape(size, chroma)
    return size[0] * size[1] + (2 * cs[0] * cs[1] if cs else 0)


def _check_planes(y, u, v, chroma):
    chroma_id(chroma)
    planes = (y,) if chroma == 'mono' else (y, u, v)
    if chroma == 'mono' and (u is not None or v is not None):
        raise ValueError("a 'mono' frame has no chroma planes")
    for p in planes:
        if p is None:
            raise ValueError(f'a {chroma!r} frame needs the planes y, u and v')
        if p.dtype != np.uint8:
            raise TypeError('planes must be uint8')
        if p.ndim != 2:
            raise ValueError('planes must be two-dimensional')
    h, w = y.shape
    if not h or not w:
        raise ValueError(f'empty frame {w}x{h}')
    want = chroma_shape((w, h), chroma)
    for name, p in zip('uv', planes[1:]):
        if p.shape != want:
            raise ValueError(f'{name} must have shape {want} for a {w}x{h} {chroma} frame, not {p.shape}')


def planar_to_bgr(y, u, v, chroma, matrix='bt601'):
    """Y (H, W) and the U, V planes of `chroma` ('420', '422', '444'; 'mono': u = v = None), all uint8 -> BGR frame
    (H, W, 3) uint8.  Pixel (r, c) uses the chroma sample (r >> sv, c >> sh): nearest replication with no siting filter,
    exactly what `nv12_to_bgr` does -- so Y4M's C420jpeg, C420mpeg2 and C420paldv, which differ only in where the chroma
    samples are sited, convert alike.  Limited range; matrix 'bt601' / 'bt709' as for NV12."""
    y = np.asarray(y)
    u = None if u is None else np.asarray(u)
    v = None if v is None else np.asarray(v)
    _check_planes(y, u, v, chroma)
    h, w = y.shape
    if chroma == 'mono':
        full = np.full((h, w), 128, np.uint8)
        return yuv_to_bgr(y, full, full, matrix)
    _, sh, sv = CHROMAS[chroma]
    rows, cols = np.arange(h) >> sv, np.arange(w) >> sh
    return yuv_to_bgr(y, u[rows][:, cols], v[rows][:, cols], matrix)


def bgr_to_planar420(frame):
    """BGR frame (H, W, 3) uint8 -> (y, u, v): planar 4:2:0, BT.601 limited range, with `bgr_to_nv12`'s arithmetic:
        Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16
        U = ((-38 R - 74 G + 112 B + 128) >> 8) + 128,  V = ((112 R - 94 G - 18 B + 128) >> 8) + 128
    per pixel, and (sum of the four pixels' U (V) + 2) >> 2 per 2 x 2 block.  Odd sizes: the missing column / row is the
    last one repeated, so the chroma planes are ((H + 1) // 2, (W + 1) // 2).  For even sizes the result is
    `bgr_to_nv12`'s, de-interleaved."""
    frame = np.asarray(frame)
    if frame.ndim != 3 or frame.shape[2] != 3 or frame.dtype != np.uint8:
        raise ValueError('frame must be uint8 HxWx3')
    h, w = frame.shape[:2]
    if not h or not w:
        raise ValueError(f'empty frame {w}x{h}')
    b, g, r = (frame[..., i].astype(np.int32) for i in range(3))
    y = (((66 * r + 129 * g + 25 * b + 128) >> 8) + 16).astype(np.uint8)
    rows = np.minimum(np.arange(2 * ((h + 1) // 2)), h - 1)
    cols = np.minimum(np.arange(2 * ((w + 1) // 2)), w - 1)
    out = []
    for plane in (((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128, ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128):
        p = plane[rows][:, cols]
        out.append(np.ascontiguousarray(((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2).astype(np.uint8)))
    return y, out[0], out[1]


class FramePlanar(C.Structure):
    """fm_frame_planar of include/fastmot_hip.h."""
    _fields_ = [('width', C.c_int32), ('height', C.c_int32), ('chroma', C.c_int32), ('matrix', C.c_int32),
                ('y', C.c_void_p), ('u', C.c_void_p), ('v', C.c_void_p), ('pitch_y', C.c_int32), ('pitch_c', C.c_int32)]


def _address(arr):
    return arr.__array_interface__['data'][0]


def _pitch(plane, what):
    rows, width = plane.shape
    if plane.strides[1] != 1:
        raise ValueError('the bytes of a row must be adjacent (element stride 1)')
    pitch = plane.strides[0] if rows > 1 else width       # (the stride of a single row means nothing)
    if pitch < width:
        raise ValueError(f'{what} row stride {pitch} < width {width}')
    return pitch


class PlanarFrame:
    """Host frame in planar YCbCr layout; MOT.step, the detectors and the ctx frame calls accept it wherever they accept
    an NV12Frame.  W * H + the chroma planes' bytes (1.5 per pixel for '420') cross to the device, where csrc/yuv.hip
    converts them to the BGR frame every stage reads: `to_bgr()` bit for bit.

    y: (H, W) uint8; u, v: uint8 planes of `chroma_shape((W, H), chroma)` (None for 'mono').  The planes may be views into
    larger arrays: elements of a row are adjacent, the luma rows are one `pitch` apart, the rows of u and of v one
    `pitch_c` -- the same for both.  The planes are not copied: they must stay unmodified until the step that uses the
    frame has returned."""

    def __init__(self, y, u=None, v=None, chroma='420', matrix='bt601'):
        self.matrix_id = matrix_id(matrix)
        self.chroma_id = chroma_id(chroma)
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
        self.y, self.u, self.v = y, u, v
        self.chroma, self.matrix = chroma, matrix
        self.size = (w, h)
        self.shape = (h, w, 3)          # of the BGR frame it becomes on the device
        self._desc = None

    @classmethod
    def from_buffer(cls, buf, size, chroma='420', matrix='bt601'):
        """One contiguous surface -- Y, then U, then V, every row packed to its width: the payload of a Y4M frame, or a
        software decoder's picture copied out."""
        w, h = size
        if w <= 0 or h <= 0:
            raise ValueError(f'empty frame {w}x{h}')
        cs = chroma_shape(size, chroma)
        if isinstance(buf, np.ndarray):
            if not buf.flags.c_contiguous:
                raise ValueError('planar surface must be one contiguous buffer')
            flat = buf.reshape(-1)
        else:
            flat = np.frombuffer(buf, np.uint8)
        if flat.dtype != np.uint8:
            raise TypeError('planar surface must be uint8')
        need = frame_bytes(size, chroma)
        if flat.size < need:
            raise ValueError(f'buffer of {flat.size} bytes < {need} bytes of a {w}x{h} {chroma} surface')
        y = flat[:w * h].reshape(h, w)
        if cs is None:
            return cls(y, None, None, chroma, matrix)
        n = cs[0] * cs[1]
        return cls(y, flat[w * h:w * h + n].reshape(cs), flat[w * h + n:w * h + 2 * n].reshape(cs), chroma, matrix)

    def to_bgr(self):
        return planar_to_bgr(self.y, self.u, self.v, self.chroma, self.matrix)

    def describe(self):
        """The fm_frame_planar that describes this frame (it points into the planes, which this object keeps alive)."""
        d = self._desc
        if d is None:
            d = FramePlanar(width=self.size[0], height=self.size[1], chroma=self.chroma_id, matrix=self.matrix_id,
                            y=_address(self.y), pitch_y=self.pitch, pitch_c=self.pitch_c)
            if self.u is not None:
                d.u, d.v = _address(self.u), _address(self.v)
            self._desc = d
        return d


class I420Image:
    """A frame as planar 4:2:0 bytes (MOT.export_frame_i420, ctx.frame_export_i420): `data`, a 1-D uint8 array of Y, then
    U, then V -- the payload of a Y4M frame -- and `size` = (W, H).  VideoIO.write takes it for a '.y4m' output."""

    def __init__(self, data, size):
        data = np.asarray(data)
        size = (int(size[0]), int(size[1]))
        if data.dtype != np.uint8 or data.ndim != 1 or data.size != frame_bytes(size, '420'):
            raise ValueError(f'data must be the {frame_bytes(size, "420")} uint8 bytes of a {size[0]}x{size[1]} I420 frame')
        self.data, self.size = data, size

    def planes(self):
        f = PlanarFrame.from_buffer(self.data, self.size, '420')
        return f.y, f.u, f.v

    def to_bgr(self, matrix='bt601'):
        return planar_to_bgr(*self.planes(), '420', matrix)


# ---- YUV4MPEG2 text
Y4M_MAGIC = b'YUV4MPEG2'
FRAME_MAGIC = b'FRAME'
_Y4M_CHROMA = {'420': '420', '420jpeg': '420', '420mpeg2': '420', '420paldv': '420', '422': '422', '444': '444', 'mono': 'mono'}
# the C tokens of 9- to 16-bit streams (read only with parse_y4m_header(..., deep=True)): name -> (chroma, depth)
_Y4M_DEEP_CHROMA = {f'{c}p{d}': (c, d) for c in ('420', '422', '444') for d in (9, 10, 12, 14, 16)}
_Y4M_DEEP_CHROMA.update({f'mono{d}': ('mono', d) for d in (9, 10, 12, 16)})


def parse_y4m_header(line, deep=False):
    """The stream header line of a YUV4MPEG2 file (bytes or str, with or without its newline) -> dict with `size` (W, H),
    `fps` (a Fraction, or None for F0:0 / no F), `chroma` ('420', '422', '444', 'mono'), `interlace` ('p' or '?') and
    `aspect` (the A token's text, or None).  C420 / C420jpeg / C420mpeg2 / C420paldv are all '420' (see planar_to_bgr);
    no C token means 420.  X... tokens are ignored, except XCOLORRANGE=FULL.  ValueError naming the token for everything
    this library does not read: interlaced material (It / Ib / Im), C411, C444alpha, 9- to 16-bit samples
    (C420p10 ...), full range, malformed or missing W / H.
    deep=True: C420p9 / p10 / p12 / p14 / p16, the C422p* and C444p* forms and Cmono9 / 10 / 12 / 16 parse too -- samples
    are little-endian 16-bit words with the value in the low bits (utils.deep.DeepFrame), a frame's payload is twice
    `frame_bytes` -- and the result gains `depth` (8 for the tokens above)."""
    if isinstance(line, (bytes, bytearray, memoryview)):
        line = bytes(line).decode('ascii', 'replace')
    tokens = line.rstrip('\n').split(' ')
    if tokens[0] != Y4M_MAGIC.decode():
        raise ValueError(f'not a YUV4MPEG2 stream: it begins with {tokens[0][:16]!r}')
    out = {'size': None, 'fps': None, 'chroma': '420', 'interlace': '?', 'aspect': None}
    if deep:
        out['depth'] = 8
    w = h = None
    for tok in tokens[1:]:
        if not tok:
            continue
        tag, val = tok[0], tok[1:]
        try:
            if tag == 'W':
                w = int(val)
            elif tag == 'H':
                h = int(val)
            elif tag == 'F':
                num, den = (int(x) for x in val.split(':'))
                if num < 0 or den < 0 or (den == 0) != (num == 0):
                    raise ValueError
                out['fps'] = Fraction(num, den) if num else None
            elif tag == 'I':
                if val not in ('p', '?'):
                    raise ValueError
                out['interlace'] = val
            elif tag == 'A':
                out['aspect'] = val
            elif tag == 'C':
                if deep and val in _Y4M_DEEP_CHROMA:
                    out['chroma'], out['depth'] = _Y4M_DEEP_CHROMA[val]
                else:
                    out['chroma'] = _Y4M_CHROMA[val]
                    if deep:
                        out['depth'] = 8
            elif tag == 'X':
                if tok.upper() == 'XCOLORRANGE=FULL':
                    raise ValueError
            else:
                raise ValueError
        except (ValueError, KeyError):
            raise ValueError(f'unsupported YUV4MPEG2 header token {tok!r}') from None
    if w is None or h is None or w <= 0 or h <= 0:
        raise ValueError(f'YUV4MPEG2 header without a valid W / H: {line.strip()!r}')
    out['size'] = (w, h)
    return out


def fps_ratio(frame_rate):
    """A frame rate (int, float or Fraction) as the (numerator, denominator) of a Y4M F token: 30 -> (30, 1),
    29.97... -> (30000, 1001)."""
    f = Fraction(frame_rate).limit_denominator(1001)
    if f <= 0:
        raise ValueError(f'frame rate {frame_rate} is not positive')
    return f.numerator, f.denominator


def y4m_header(width, height, fps_ratio):
    """The stream header this library writes: progressive, square pixels, 4:2:0 (chroma as `bgr_to_planar420` averages
    it: centred, 'jpeg' siting), limited range."""
    num, den = fps_ratio
    return f'YUV4MPEG2 W{int(width)} H{int(height)} F{int(num)}:{int(den)} Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n'.encode('ascii')
