"""Frames at capture resolution: the host-side handle that MOT.step accepts for a frame whose size is not the tracker's.

The reference resizes every captured frame to the tracker's `size` on the host before anything else sees it
(cv2.resize in its VideoIO; 1280 x 720 from 1920 x 1080 sources in its default configuration).  A `SourceFrame` wraps
the frame as it was captured -- a BGR ndarray, an NV12Frame, a JPEGFrame, a PlanarFrame, a PackedFrame, a BayerFrame, a DeepFrame or (already in GPU memory) a DeviceArrayFrame -- and is uploaded at that resolution; the
kernel of csrc/resize.hip then writes the `size` BGR frame that every stage reads.  The resize is cv2.resize's 8-bit
INTER_LINEAR arithmetic, integer and exact: the device frame equals `videoio.resize_bgr(frame, size)` bit for bit (for
an NV12Frame / JPEGFrame / PlanarFrame / PackedFrame / BayerFrame / DeepFrame: of the BGR frame it converts / decodes to)."""
import ctypes as C

import numpy as np

from .bayer import BayerFrame
from .deep import DeepFrame
from .devarray import DeviceArrayFrame
from .jpeg import JPEGFrame, JpegInfo
from .lens import LensMap
from .nv12 import NV12Frame
from .packed import PackedFrame
from .yuv import PlanarFrame

FM_SRC_BGR, FM_SRC_NV12, FM_SRC_JPEG = 0, 1, 2
MAX_DIM = 16384         # FM_SRC_MAX_DIM of include/fastmot_hip.h


class FrameSrc(C.Structure):
    """fm_frame_src of include/fastmot_hip.h."""
    _fields_ = [('kind', C.c_int32), ('width', C.c_int32), ('height', C.c_int32),
                ('bgr', C.c_void_p),
                ('y', C.c_void_p), ('uv', C.c_void_p), ('pitch', C.c_int32), ('matrix', C.c_int32),
                ('info', C.POINTER(JpegInfo)), ('coef', C.c_void_p), ('qt', C.c_void_p)]


def _address(arr):
    return arr.__array_interface__['data'][0]


class SourceFrame:
    """Host frame at capture resolution; MOT.step, the detectors, the feature extractor, the tracker and the ctx frame
    calls accept it wherever they accept a BGR ndarray, whatever the tracker's frame size is.

    frame: a BGR ndarray (H, W, 3) uint8, an NV12Frame, a JPEGFrame, a PlanarFrame, a PackedFrame, a BayerFrame, a DeepFrame or a DeviceArrayFrame, at most 16384 pixels in either direction.  It
    is not copied (an ndarray that is not C-contiguous is, once): it must stay unmodified until the step that uses the
    frame has returned.  `size` is the SOURCE's (W, H) and `shape` its (H, W, 3); the frame every stage reads has the
    size of the context it is uploaded to.

    lens: a LensMap for frames of this size (utils/lens.py), or None.  With one, the kernel of csrc/remap.hip takes the
    resize's place and the device frame equals `utils.lens.remap_bgr(frame, lens)` bit for bit -- also for a frame that
    already has the tracker's size.  Hand every frame of a stream the SAME LensMap object: the context switches maps,
    and synchronises, when a frame carries another object than the one it has set."""

    def __init__(self, frame, lens=None):
        if isinstance(frame, SourceFrame):
            raise TypeError('frame is a SourceFrame already')
        if isinstance(frame, (NV12Frame, JPEGFrame, PlanarFrame, PackedFrame, BayerFrame, DeepFrame, DeviceArrayFrame)):
            w, h = frame.size
        elif isinstance(frame, np.ndarray):
            if frame.ndim != 3 or frame.shape[2] != 3 or frame.dtype != np.uint8:
                raise ValueError('frame must be uint8 HxWx3')
            h, w = frame.shape[:2]
            frame = np.ascontiguousarray(frame)
        else:
            raise TypeError(f'frame must be a BGR ndarray, an NV12Frame, a JPEGFrame, a PlanarFrame, a PackedFrame, a BayerFrame, a DeepFrame or a DeviceArrayFrame, not {type(frame).__name__}')
        if not (1 <= w <= MAX_DIM and 1 <= h <= MAX_DIM):
            raise ValueError(f'source size {w}x{h} outside 1..{MAX_DIM}')
        if lens is not None:
            if not isinstance(lens, LensMap):
                raise TypeError(f'lens must be a LensMap, not {type(lens).__name__}')
            if lens.src_size != (w, h):
                raise ValueError(f'the lens map is for {lens.src_size[0]}x{lens.src_size[1]} frames, this one is {w}x{h}')
        self.lens = lens
        self.frame = frame
        self.size = (w, h)
        self.shape = (h, w, 3)
        self._desc = None

    def describe(self):
        """The fm_frame_src that describes this frame (it points into `self.frame`, which this object keeps alive).  A
        PlanarFrame has a description of its own, `frame.describe()`: the ctx frame calls hand that one to fm_frame_*_planar,
        which take every size; so have a PackedFrame (fm_frame_*_packed), a BayerFrame (fm_frame_*_bayer), a DeepFrame (fm_frame_*_deep) and a DeviceArrayFrame (fm_frame_*_device)."""
        if isinstance(self.frame, PlanarFrame):
            raise TypeError('a planar source is described by its PlanarFrame (fm_frame_planar), not by fm_frame_src')
        if isinstance(self.frame, PackedFrame):
            raise TypeError('a packed source is described by its PackedFrame (fm_frame_packed), not by fm_frame_src')
        if isinstance(self.frame, BayerFrame):
            raise TypeError('a Bayer source is described by its BayerFrame (fm_frame_bayer), not by fm_frame_src')
        if isinstance(self.frame, DeepFrame):
            raise TypeError('a deep source is described by its DeepFrame (fm_frame_deep), not by fm_frame_src')
        if isinstance(self.frame, DeviceArrayFrame):
            raise TypeError('a source in device memory is described by its DeviceArrayFrame (fm_frame_device), not by fm_frame_src')
        d = self._desc
        if d is None:
            f = self.frame
            d = FrameSrc(width=self.size[0], height=self.size[1])
            if isinstance(f, NV12Frame):
                d.kind, d.y, d.uv, d.pitch, d.matrix = FM_SRC_NV12, _address(f.y), _address(f.uv), f.pitch, f.matrix_id
            elif isinstance(f, JPEGFrame):
                d.kind, d.info, d.coef, d.qt = FM_SRC_JPEG, C.pointer(f.info), _address(f.coef), _address(f.qt)
            else:
                d.kind, d.bgr = FM_SRC_BGR, _address(f)
            self._desc = d
        return d
