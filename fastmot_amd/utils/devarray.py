"""Frames that already lie in GPU memory: the handle that MOT.step accepts for them (DeviceArrayFrame), and the numpy
statement of what csrc/devsrc.hip computes from them (to_bgr).

A hardware decoder's NV12 surface, `torchvision.io.decode_jpeg(device='cuda')`, a torch or CuPy preprocessing pipeline,
a GPU ISP, another model's output: such a frame never needs to see the host.  A DeviceArrayFrame describes the memory
where it lies -- pointer, pitches, layout, the producer's stream --, no byte crosses PCIe and no host copy is made; a
kernel reads it and writes the BGR frame every stage reads.  This module does not import torch or CuPy: it reads the
`__cuda_array_interface__` dict that all of them publish (on ROCm too) and nothing else.

Four conversions, chosen by shape and dtype:

    (H, W, 3) / (H, W, 4) uint8   HWC: `utils.packed.packed_to_bgr` of the same bytes, `order` one of 'rgb', 'bgr' (3 bytes)
                                  or 'rgbx' / 'rgba', 'bgrx' / 'bgra', 'xrgb' / 'argb', 'xbgr' / 'abgr' (4)
    (3, H, W) uint8               CHW: the planes in `order` 'rgb' or 'bgr', permuted into B, G, R
    (3, H, W) float16 / float32   CHW: v = float32(x) * scale in float32 -- scale 255 for `float_range` (0, 1), 1 for
                                  (0, 255) --, rounded half to even, NaN -> 0, clamped to 0..255
    y (H, W) + uv (H / 2, W)      NV12 (DeviceArrayFrame.nv12): `utils.nv12.nv12_to_bgr`, a pitch per plane

All of it is exact, so the GPU frame equals `to_bgr` bit for bit.
"""
import ctypes as C

import numpy as np

from .nv12 import matrix_id, nv12_to_bgr
from .packed import FORMATS, packed_to_bgr

FM_DEV_HWC, FM_DEV_CHW, FM_DEV_NV12 = 0, 1, 2
FM_DEV_U8, FM_DEV_F16, FM_DEV_F32 = 0, 1, 2
FM_DEV_ORDER_RGB, FM_DEV_ORDER_BGR = 0, 1
FM_DEV_READY = 1
MAX_DIM = 16384         # FM_SRC_MAX_DIM of include/fastmot_hip.h

# numpy dtype -> (FM_DEV_* dtype, element bytes)
DTYPES = {np.dtype(np.uint8): (FM_DEV_U8, 1), np.dtype(np.float16): (FM_DEV_F16, 2), np.dtype(np.float32): (FM_DEV_F32, 4)}
_RGB_FAMILY = sorted(k for k, v in FORMATS.items() if v[1] == 'rgb')


class FrameDevice(C.Structure):
    """fm_frame_device of include/fastmot_hip.h."""
    _fields_ = [('plane', C.c_void_p * 3), ('pitch', C.c_int64 * 3), ('width', C.c_int32), ('height', C.c_int32),
                ('layout', C.c_int32), ('dtype', C.c_int32), ('format', C.c_int32), ('matrix', C.c_int32),
                ('scale', C.c_float), ('stream', C.c_void_p), ('flags', C.c_int32)]


def scale_of(float_range):
    """The factor of the float conversions: 255 for values in (0, 1), 1 for values in (0, 255)."""
    try:
        lo, hi = float_range
    except (TypeError, ValueError):
        lo = hi = None
    if lo == 0 and hi == 1:
        return 255.0
    if lo == 0 and hi == 255:
        return 1.0
    raise ValueError(f'float_range must be (0, 1) or (0, 255), not {float_range!r}')


def infer_layout(shape, dtype, order='rgb', layout=None):
    """(layout, (W, H), format id, canonical order) of an array of `shape` and `dtype`: 'hwc' for (H, W, 3 | 4) uint8, 'chw'
    for (3, H, W) uint8 / float16 / float32.  ValueError for anything else and for a shape that is both -- unless
    `layout` ('hwc' / 'chw') says which it is."""
    shape = tuple(int(s) for s in shape)
    dtype = np.dtype(dtype)
    if dtype not in DTYPES:
        raise ValueError(f'a device frame is uint8, float16 or float32, not {dtype}')
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f'a device frame is (H, W, 3), (H, W, 4) or (3, H, W), not {shape}')
    hwc = dtype == np.uint8 and shape[2] in (3, 4)
    chw = shape[0] == 3
    if layout is not None:
        if layout not in ('hwc', 'chw'):
            raise ValueError(f"layout must be 'hwc', 'chw' or None, not {layout!r}")
        if not (hwc if layout == 'hwc' else chw):
            raise ValueError(f'{dtype} {shape} is no {layout} frame')
        hwc, chw = layout == 'hwc', layout == 'chw'
    if hwc and chw:
        raise ValueError(f"shape {shape} is both (H, W, {shape[2]}) and (3, H, W): say which with layout='hwc' or layout='chw'")
    if not isinstance(order, str):
        raise ValueError(f'order must be a string, not {order!r}')
    if hwc:
        h, w, c = shape
        name = order.lower()
        if c == 4 and name in ('rgb', 'bgr'):              # (the default order for a 4-byte pixel: the fourth byte is ignored)
            name += 'x'
        if name not in _RGB_FAMILY or FORMATS[name][2] != c:
            raise ValueError(f'order of a {c}-byte pixel must be one of {[k for k in _RGB_FAMILY if FORMATS[k][2] == c]}, not {order!r}')
        return 'hwc', (w, h), FORMATS[name][0], name
    if chw:
        _, h, w = shape
        name = order.lower()
        if name not in ('rgb', 'bgr'):
            raise ValueError(f"order of a (3, H, W) frame must be 'rgb' or 'bgr', not {order!r}")
        return 'chw', (w, h), FM_DEV_ORDER_RGB if name == 'rgb' else FM_DEV_ORDER_BGR, name
    if shape[2] in (3, 4):
        raise ValueError(f'an (H, W, {shape[2]}) frame is uint8, not {dtype}: float frames are (3, H, W)')
    raise ValueError(f'a device frame is (H, W, 3), (H, W, 4) or (3, H, W), not {shape}')


def quantise(x, float_range=(0, 1)):
    """The float conversions' arithmetic on an array of float16 / float32: float32(x) * scale in float32, rounded half to
    even, NaN -> 0, clamped to 0..255 -> uint8."""
    with np.errstate(invalid='ignore', over='ignore'):
        v = np.rint(np.asarray(x).astype(np.float32) * np.float32(scale_of(float_range)))
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.clip(v, 0, 255).astype(np.uint8)


def to_bgr(data, order='rgb', float_range=(0, 1), matrix='bt601', layout=None):
    """What csrc/devsrc.hip makes of a device frame, on host arrays: `data` is an ndarray (H, W, 3 | 4) uint8 or (3, H, W)
    uint8 / float16 / float32 with `order` (and `float_range`, and `layout` for a shape that is both), or a pair
    (y, uv) of NV12 planes with `matrix` -> BGR frame (H, W, 3) uint8."""
    if isinstance(data, (tuple, list)):
        y, uv = data
        return nv12_to_bgr(y, uv, matrix)
    data = np.asarray(data)
    layout, _, _, name = infer_layout(data.shape, data.dtype, order, layout)
    if layout == 'hwc':
        return packed_to_bgr(np.ascontiguousarray(data), None, name)
    planes = data if name == 'bgr' else data[::-1]
    if data.dtype != np.uint8:
        planes = quantise(planes, float_range)
    return np.ascontiguousarray(np.moveaxis(planes, 0, 2))


def parse_interface(obj):
    """The fields of `obj.__cuda_array_interface__` a frame needs -> dict(shape, dtype, ptr, strides (bytes; those of a
    C-contiguous array when the interface says None), stream (the interface's, v3; None when it has none))."""
    try:
        cai = obj.__cuda_array_interface__
    except AttributeError:
        raise TypeError(f'{type(obj).__name__} has no __cuda_array_interface__: a device frame is a torch / CuPy / Numba '
                        'array in GPU memory (host arrays go to the host frame kinds)') from None
    shape = tuple(int(s) for s in cai['shape'])
    typestr = cai['typestr']
    if typestr[0] == '>':
        raise ValueError(f'big-endian elements ({typestr!r}) are not read')
    dtype = np.dtype(typestr)
    data = cai['data']
    ptr = int(data[0]) if isinstance(data, (tuple, list)) else int(data)
    strides = cai.get('strides')
    if strides is None:
        strides, step = [], dtype.itemsize
        for n in reversed(shape):
            strides.append(step)
            step *= max(n, 1)
        strides = tuple(reversed(strides))
    else:
        strides = tuple(int(s) for s in strides)
        if len(strides) != len(shape):
            raise ValueError(f'strides {strides} do not go with shape {shape}')
    if cai.get('mask') is not None:
        raise ValueError('masked arrays are not read')
    return dict(shape=shape, dtype=dtype, ptr=ptr, strides=strides, stream=cai.get('stream'))


def _stream_handle(stream):
    """A stream argument as the integer fm_frame_device.stream takes: None / 0 -> the null stream; the interface's 1
    (legacy default stream) and 2 (per-thread default stream) are HIP's own handles for those."""
    if stream is None:
        return 0
    stream = int(getattr(stream, 'cuda_stream', stream))       # (a torch.cuda.Stream is taken as well)
    if stream < 0:
        raise ValueError(f'stream must be a hipStream_t handle, not {stream}')
    return stream


def _rows(info, what, elem):
    """(pitch, pointer) of a 2-D plane whose interface fields are `info`: adjacent elements, rows a positive pitch apart."""
    (h, w), (s0, s1) = info['shape'], info['strides']
    if min(s0, s1) < 0:
        raise ValueError(f'{what}: negative strides {info["strides"]} are not read')
    if s1 != elem and w > 1:
        raise ValueError(f'{what}: the elements of a row must be adjacent (stride {elem}), not {s1} bytes apart')
    pitch = s0 if h > 1 else w * elem                            # (the stride of a single row means nothing)
    if pitch < w * elem:
        raise ValueError(f'{what}: row stride {pitch} < the {w * elem} bytes of a row')
    return pitch


class DeviceArrayFrame:
    """A frame in GPU memory; MOT.step, the detectors and the ctx frame calls accept it wherever they accept a PackedFrame,
    inside a SourceFrame (any size, with or without a LensMap) too.  Nothing is copied to or through the host:
    csrc/devsrc.hip reads the array where it lies and writes the BGR frame every stage reads, `to_bgr` bit for bit.

    array: any object with `__cuda_array_interface__` (a torch-ROCm tensor, a CuPy or Numba array) on the context's device,
        (H, W, 3) or (H, W, 4) uint8, or (3, H, W) uint8 / float16 / float32 -- possibly a view of a larger array: the
        elements of a pixel (HWC) or of a row (CHW) are adjacent, rows and planes any non-negative stride apart.  A shape
        that is both, such as (3, H, 3), raises ValueError unless `layout` ('hwc' or 'chw') says which it is; a negative
        stride or an inner stride other than the element size always does.
    order: the channel order -- 'rgb' or 'bgr', and for 4-byte pixels 'rgbx', 'bgrx', 'xrgb', 'xbgr' (and their
        'rgba' .. 'abgr' aliases; 'rgb' / 'bgr' stand for 'rgbx' / 'bgrx' there).
    float_range: (0, 1) or (0, 255), what the values of a float frame span.
    stream: the stream the work that fills the array was enqueued on -- a hipStream_t as an integer, or an object with
        `.cuda_stream`; the conversion is ordered behind everything that stream holds at the time of the call.  Default:
        the interface's own `stream` where it publishes one (version 3), the null stream otherwise.  torch publishes
        version 2: hand over `torch.cuda.current_stream().cuda_stream` when the producer ran on a side stream.
    ready: the data is complete already (the producer was synchronised): nothing is recorded or waited for.

    Lifetime.  The context keeps a reference to the frame -- and through it to `array` -- until the device has finished
    reading it, prunes those references at every later frame call and waits for all of them in `close()`: the caller may
    DROP the array right after `step`.  The caller must not OVERWRITE it before `done()` says so (`wait()` blocks until
    then): a frame handed over as `next_frame` is converted while the current step runs, not before the call returns.

    One HIP runtime.  torch and CuPy wheels bring a ROCm copy of their own; of two copies in a process the one loaded
    first serves both, and only then does the library know the producer's pointers and streams.  Import the producer
    before the first context is created (`import torch` above `import fastmot_amd` does it); a pointer from a second
    runtime is refused as not being device memory."""

    def __init__(self, array, order='rgb', float_range=(0, 1), stream=None, ready=False, layout=None):
        info = parse_interface(array)
        self.layout, (w, h), self.format_id, self.order = infer_layout(info['shape'], info['dtype'], order, layout)
        self.dtype = info['dtype']
        self.dtype_id, elem = DTYPES[self.dtype]
        self.scale = scale_of(float_range)
        self.matrix = None
        strides, ptr = info['strides'], info['ptr']
        if min(strides) < 0:
            raise ValueError(f'negative strides {strides} are not read')
        if self.layout == 'hwc':
            c = info['shape'][2]
            if strides[2] != 1 or (strides[1] != c and w > 1):
                raise ValueError(f'the bytes of a row must be adjacent (strides {c}, 1), not {strides[1:]}')
            pitch = strides[0] if h > 1 else w * c
            need = w * c
            planes = [(ptr, pitch)]
        else:
            if strides[2] != elem and w > 1:
                raise ValueError(f'the elements of a row must be adjacent (stride {elem}), not {strides[2]} bytes apart')
            pitch = strides[1] if h > 1 else w * elem
            need = w * elem
            planes = [(ptr + c * strides[0], pitch) for c in range(3)]
        if pitch < need:
            raise ValueError(f'row stride {pitch} < the {need} bytes of a row')
        self._finish(array, planes, (w, h), 0, info['stream'] if stream is None else stream, ready, elem)

    @classmethod
    def nv12(cls, y, uv, matrix='bt601', stream=None, ready=False):
        """An NV12 frame from two device arrays: y (H, W) uint8 and uv (H / 2, W) uint8 (U, V interleaved), H and W even --
        NV12Frame's shape rules; each plane has a pitch of its own, and the two need not lie in one allocation.  `matrix`:
        'bt601' or 'bt709'.  `stream` / `ready`: as the constructor's (the interface's stream is the Y plane's)."""
        self = cls.__new__(cls)
        mid = matrix_id(matrix)
        iy, iuv = parse_interface(y), parse_interface(uv)
        if iy['dtype'] != np.uint8 or iuv['dtype'] != np.uint8:
            raise TypeError('NV12 planes must be uint8')
        if len(iy['shape']) != 2 or len(iuv['shape']) != 2:
            raise ValueError('y must have shape (H, W) and uv shape (H / 2, W)')
        h, w = iy['shape']
        if h % 2 or w % 2 or not h or not w:
            raise ValueError(f'NV12 needs an even, non-zero frame size, not {w}x{h}')
        if iuv['shape'] != (h // 2, w):
            raise ValueError(f'uv must have shape {(h // 2, w)} for a {w}x{h} frame, not {iuv["shape"]}')
        planes = [(iy['ptr'], _rows(iy, 'y', 1)), (iuv['ptr'], _rows(iuv, 'uv', 1))]
        self.layout, self.format_id, self.order = 'nv12', 0, None
        self.dtype, self.dtype_id, self.scale = np.dtype(np.uint8), FM_DEV_U8, 1.0
        self.matrix = matrix
        self._finish((y, uv), planes, (w, h), mid, iy['stream'] if stream is None else stream, ready, 1)
        return self

    def _finish(self, array, planes, size, matrix_id_, stream, ready, elem):
        w, h = size
        if not (1 <= w <= MAX_DIM and 1 <= h <= MAX_DIM):
            raise ValueError(f'frame size {w}x{h} outside 1..{MAX_DIM}')
        for ptr, pitch in planes:
            if not ptr:
                raise ValueError('the array has no memory (a null pointer)')
            if ptr % elem or pitch % elem:
                raise ValueError(f'pointer {ptr:#x} / pitch {pitch} is no multiple of the element size {elem}')
        self.array = array              # keeps the memory alive as long as this object lives
        self.planes = planes
        self.matrix_id = matrix_id_
        self.stream = _stream_handle(stream)
        self.ready = bool(ready)
        self.size = (w, h)
        self.shape = (h, w, 3)          # of the BGR frame it becomes
        self._desc = None
        self._pending = []              # (weak reference to the context, ticket) of the look-ahead uploads that may still read the array

    def descriptor(self):
        """The fm_frame_device that describes this frame (it points into the array, which this object keeps alive)."""
        d = self._desc
        if d is None:
            d = FrameDevice(width=self.size[0], height=self.size[1],
                            layout={'hwc': FM_DEV_HWC, 'chw': FM_DEV_CHW, 'nv12': FM_DEV_NV12}[self.layout], dtype=self.dtype_id,
                            format=self.format_id, matrix=self.matrix_id, scale=self.scale, stream=self.stream or None,
                            flags=FM_DEV_READY if self.ready else 0)
            for i, (ptr, pitch) in enumerate(self.planes):
                d.plane[i], d.pitch[i] = ptr, pitch
            self._desc = d
        return d

    def describe(self):
        """One line for logs: layout, size, element type, order / matrix, pointers, pitches, stream, state."""
        what = self.matrix if self.layout == 'nv12' else self.order
        planes = ' '.join(f'{ptr:#x}+{pitch}' for ptr, pitch in self.planes)
        state = 'ready' if self.ready else f'stream {self.stream:#x}'
        return (f'DeviceArrayFrame {self.layout} {self.size[0]}x{self.size[1]} {self.dtype.name} {what} planes [{planes}] '
                f'{state}, {"consumed" if self.done() else "being read"}')

    __repr__ = describe

    def done(self):
        """True when no upload of this frame can still read the array: it may be overwritten."""
        self._pending = [(ref, t) for ref, t in self._pending if ref() is not None and not ref().device_frame_done(t)]
        return not self._pending

    def wait(self):
        """Blocks until `done()`."""
        pending, self._pending = self._pending, []
        contexts = {}
        for ref, t in pending:
            ctx = ref()
            if ctx is not None:             # (a context that is gone waited for its frames when it was closed)
                ctx.device_frame_done(t, wait=True)
                contexts[id(ctx)] = ctx
        for ctx in contexts.values():
            ctx.device_frames_prune()
        return self
