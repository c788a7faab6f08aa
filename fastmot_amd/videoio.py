"""VideoIO (API of fastmot/videoio.py:24-277) without OpenCV / GStreamer: threaded capture into a bounded
queue with the reference's semantics (file sources block when the buffer is full, live sources drop),
`cap_dt`, `read()`, `write()`, `release()`.

Sources this implementation can decode:
  * image sequences  'dir/%06d.jpg' (any format Pillow reads; the MOTChallenge layout)  -> Protocol.IMAGE
  * raw frame stacks '*.npy' ([N, H, W, 3] uint8 BGR, memory-mapped; with `pixel_format` a stack of packed RGB / BGRx /
    YUY2 / UYVY ... frames as a camera or an image library hands them out, see VideoIO)  -> Protocol.VIDEO
  * YUV4MPEG2 '*.y4m' (a text header + uncompressed planar YCbCr frames, 4:2:0 / 4:2:2 / 4:4:4 / mono, 8-bit limited
    range -- 9- to 16-bit with `deep_color` --, progressive; a file or a named pipe fed by any decoder: `ffmpeg -i x.mp4 -f yuv4mpegpipe x.y4m`) -> Protocol.VIDEO
Other video containers, cameras and network streams need a decoder this image does not have; they raise
NotImplementedError with the URI.  Outputs: image sequence ('out/%06d.png'), '*.npy' or '*.y4m' (4:2:0); with gpu_encode
also '*.mjpeg' (concatenated JPEG files), and '%06d.jpg' sequences and '.y4m' frames are converted on the GPU.

Frames are BGR uint8 like cv2's; a source whose size differs from `size` is resized with cv2.resize's
INTER_LINEAR arithmetic (imgproc/resize.cpp: 11-bit fixed-point coefficients, exact 2x decimation =
INTER_AREA) so that downstream results do not depend on which VideoIO produced the frame."""
from collections import deque
from enum import Enum
from pathlib import Path
from urllib.parse import urlparse
import logging
import threading

import numpy as np

LOGGER = logging.getLogger(__name__)


class Protocol(Enum):
    IMAGE = 0
    VIDEO = 1
    CSI = 2
    V4L2 = 3
    RTSP = 4
    HTTP = 5


def _lin_coef(dsize, ssize):
    scale = ssize / dsize
    fx = ((np.arange(dsize) + 0.5) * scale - 0.5).astype(np.float32)
    sx = np.floor(fx).astype(np.int32)
    fx = fx - sx.astype(np.float32)
    lo, hi = sx < 0, sx >= ssize - 1
    fx[lo | hi] = 0
    sx[lo] = 0
    sx[hi] = ssize - 1
    a1 = np.rint(fx * np.float32(2048)).astype(np.int32)
    a0 = np.rint((np.float32(1) - fx) * np.float32(2048)).astype(np.int32)
    return sx, np.minimum(sx + 1, ssize - 1), a0, a1


def resize_bgr(img, size):
    """cv2.resize(img, size) for uint8 images, INTER_LINEAR (fixed point, see module docstring)."""
    dw, dh = size
    sh, sw = img.shape[:2]
    if (sw, sh) == (dw, dh):
        return img
    src = img.astype(np.int32)
    if sw == 2 * dw and sh == 2 * dh:
        return ((src[0::2, 0::2] + src[0::2, 1::2] + src[1::2, 0::2] + src[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    x0, x1, ax0, ax1 = _lin_coef(dw, sw)
    y0, y1, ay0, ay1 = _lin_coef(dh, sh)
    rows = src[:, x0] * ax0[None, :, None] + src[:, x1] * ax1[None, :, None]
    s0, s1 = rows[y0] >> 4, rows[y1] >> 4
    out = (((ay0[:, None, None] * s0) >> 16) + ((ay1[:, None, None] * s1) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


class _ImageSequence:
    def __init__(self, pattern, gpu_size=None, any_size=False):
        """gpu_size: (w, h) -- files that are supported baseline JPEGs of exactly this size come back as JPEGFrames
        (entropy-decoded here, on the capture thread; the rest of the decode runs on the GPU when the frame is uploaded),
        every other file as the BGR ndarray Pillow decodes.  None: ndarrays only.  any_size: supported JPEGs of every
        size the GPU resize takes come back as JPEGFrames (the caller wraps those of another size in SourceFrames)."""
        from PIL import Image
        self._open = Image.open
        self.gpu_size = None if gpu_size is None else tuple(gpu_size)
        self.any_size = bool(any_size)
        self.pattern = pattern
        self.index = 0 if Path(pattern % 0).exists() else 1
        if not Path(pattern % self.index).exists():
            raise RuntimeError('Unable to read video stream')

    def read(self):
        path = Path(self.pattern % self.index)
        if not path.exists():
            return None
        self.index += 1
        if self.gpu_size is not None:
            frame = self._read_jpeg(path)
            if frame is not None:
                return frame
        with self._open(path) as im:
            rgb = np.asarray(im.convert('RGB'))
        return np.ascontiguousarray(rgb[:, :, ::-1])

    def _read_jpeg(self, path):
        """JPEGFrame of the file, or None when it is not a supported JPEG of the wanted size (the caller decodes it with
        Pillow then: PNGs, progressive or CMYK JPEGs, a file of another size, a damaged file)."""
        from .utils.jpeg import JPEGFrame
        from .utils.source import MAX_DIM
        data = path.read_bytes()
        if data[:2] != b'\xff\xd8':
            return None
        try:                        # (the size is compared after the header is parsed, before anything is allocated or decoded)
            frame = JPEGFrame(data, size=None if self.any_size else self.gpu_size)
        except ValueError:
            return None
        return frame if max(frame.size) <= MAX_DIM else None


class _FrameStack:
    def __init__(self, path):
        self.frames = np.load(path, mmap_mode='r')
        if self.frames.ndim != 4 or self.frames.shape[3] != 3 or self.frames.dtype != np.uint8:
            raise RuntimeError('Unable to read video stream: expected a [N, H, W, 3] uint8 array')
        self.index = 0

    def read(self):
        if self.index >= len(self.frames):
            return None
        self.index += 1
        return np.array(self.frames[self.index - 1])


class _PackedStack:
    """A '.npy' stack of packed frames in the layout `fmt` (utils.packed.FORMATS), memory-mapped.  Accepted shapes, uint8:
    (N, H, W, bpp) for the RGB family (bpp 3 or 4, as the layout says), and (N, H, row bytes) for every layout -- row bytes
    a multiple of the layout's bytes per pixel for RGB, of 4 for the 4:2:2 family, which carries two pixels in 4 bytes, so
    W = row bytes / 2 (an odd width cannot be told from the shape: such a stack reads as W + 1 wide).  read() returns the
    next frame -- a PackedFrame over a copy of the frame's bytes when `packed` holds for the stack's (W, H), the BGR
    ndarray `packed_to_bgr` makes of it otherwise --, or None at the end."""

    def __init__(self, path, fmt, matrix='bt601', packed=None):
        from .utils import packed as pk
        pk.format_id(fmt)
        pk.matrix_id(matrix)
        self._pk, self.format, self.matrix = pk, fmt, matrix
        self.frames = np.load(path, mmap_mode='r')
        _, family, bpp, _ = pk.FORMATS[fmt]
        shape = self.frames.shape
        unit = 4 if family == '422' else bpp
        ok = self.frames.dtype == np.uint8 and len(shape) in (3, 4) and all(shape[1:])
        if ok and len(shape) == 4:
            ok = family == 'rgb' and shape[3] == bpp
            w = shape[2]
        elif ok:
            ok = shape[2] % unit == 0
            w = shape[2] // (2 if family == '422' else bpp)
        if not ok:
            raise ValueError(f'{path}: a {fmt!r} frame stack is a uint8 array (N, H, row bytes) with row bytes a multiple of {unit}'
                             + (f' or (N, H, W, {bpp})' if family == 'rgb' else '') + f', not {self.frames.dtype} {shape}')
        self.size = (w, shape[1])
        self.packed = bool(packed(self.size)) if packed is not None else False
        self.index = 0

    def read(self):
        if self.index >= len(self.frames):
            return None
        self.index += 1
        data = np.array(self.frames[self.index - 1]).reshape(self.size[1], -1)
        frame = self._pk.PackedFrame(data, self.format, self.size, self.matrix)
        return frame if self.packed else frame.to_bgr()


def _bayer_format(pixel_format):
    """(pattern, depth) of a Bayer `pixel_format` -- 'rggb', 'grbg', 'gbrg' or 'bggr', with '10', '12', '14' or '16' behind it
    for samples deeper than 8 bits --, or None for every other value."""
    from .utils.bayer import PATTERNS
    if not isinstance(pixel_format, str) or pixel_format[:4] not in PATTERNS or pixel_format[4:] not in ('', '10', '12', '14', '16'):
        return None
    return pixel_format[:4], int(pixel_format[4:] or 8)


class _BayerStack:
    """A '.npy' stack (N, H, W) of Bayer mosaics, memory-mapped: uint8 for depth 8, uint16 for the deeper ones, H and W at
    least 2.  read() returns the next frame -- a BayerFrame over a copy of the frame's samples when `bayer` holds for the
    stack's (W, H), the BGR ndarray `bayer_to_bgr` makes of it otherwise --, or None at the end."""

    def __init__(self, path, pattern, depth, method='mhc', wb=None, black=0, bayer=None):
        from .utils import bayer as by
        by.method_id(method)
        self._by, self.pattern, self.depth, self.method = by, pattern, depth, method
        self.wb = (1., 1., 1.) if wb is None else tuple(wb)
        by.gains(self.wb)
        self.black = by._black(black, depth)
        self.frames = np.load(path, mmap_mode='r')
        shape, want = self.frames.shape, np.dtype(np.uint8 if depth == 8 else '<u2')
        if self.frames.dtype != want or len(shape) != 3 or shape[1] < 2 or shape[2] < 2:
            raise ValueError(f'{path}: a {pattern!r} frame stack of depth {depth} is a {want.name} array (N, H, W) with H, W >= 2, '
                             f'not {self.frames.dtype} {shape}')
        self.size = (shape[2], shape[1])
        self.bayer = bool(bayer(self.size)) if bayer is not None else False
        self.index = 0

    def read(self):
        if self.index >= len(self.frames):
            return None
        self.index += 1
        frame = self._by.BayerFrame(np.array(self.frames[self.index - 1]), self.pattern, None, self.depth, self.method, self.wb, self.black)
        return frame if self.bayer else frame.to_bgr()


class _Y4MStream:
    """A YUV4MPEG2 stream, read strictly forward (no seek, no stat: a named pipe works).  `fps`: the header's F ratio as
    a float, None when the stream does not know it (F0:0).  read() returns the next frame -- a PlanarFrame over the
    frame's own buffer when `planar` is set, the BGR ndarray `planar_to_bgr` makes of it otherwise --, or None at the
    end of the stream; a last frame that is cut short ends the stream like that, without an error.  With `deep` a 9- to
    16-bit stream (C420p10 ...) opens too: `depth` is its sample depth, its frames are utils.deep.DeepFrames and
    `deep_to_bgr`'s pixels, and `matrix` may be 'bt2020' for it."""

    def __init__(self, path, planar=None, matrix='bt601', deep=False):
        """planar: a predicate on the stream's (W, H) -- frames come back as PlanarFrames (DeepFrames) where it holds."""
        from .utils import yuv
        from .utils.nv12 import matrix_id
        if not deep:
            matrix_id(matrix)
        self._yuv = yuv
        self.matrix = matrix
        self.file = open(path, 'rb')
        try:
            line = self.file.readline(4096)
            if not line.endswith(b'\n'):
                raise RuntimeError('Unable to read video stream: no YUV4MPEG2 header')
            info = yuv.parse_y4m_header(line, deep=True) if deep else yuv.parse_y4m_header(line)
            self.depth = info.get('depth', 8)
            if self.depth > 8:
                from .utils import deep as deep_mod
                self._deep = deep_mod
                deep_mod.matrix_id(matrix)
            else:
                matrix_id(matrix)
        except Exception:
            self.file.close()
            raise
        self.size, self.chroma = info['size'], info['chroma']
        self.fps = float(info['fps']) if info['fps'] else None
        self.planar = bool(planar(self.size)) if planar is not None else False
        self.frame_bytes = yuv.frame_bytes(self.size, self.chroma) * (2 if self.depth > 8 else 1)

    def read(self):
        line = self.file.readline(4096)          # 'FRAME' + optional parameters up to the newline
        if not line.endswith(b'\n'):
            return None
        if not line.startswith(self._yuv.FRAME_MAGIC):
            raise RuntimeError(f'Unable to read video stream: {line[:16]!r} where a FRAME header belongs')
        buf = np.empty(self.frame_bytes, np.uint8)
        view, got = memoryview(buf), 0
        while got < self.frame_bytes:             # (a pipe hands over what it has)
            n = self.file.readinto(view[got:])
            if not n:
                return None                       # the stream ends inside this frame
            got += n
        if self.depth > 8:
            frame = self._deep.DeepFrame.from_buffer(buf, self.size, self.chroma, self.depth, self.matrix)
        else:
            frame = self._yuv.PlanarFrame.from_buffer(buf, self.size, self.chroma, self.matrix)
        return frame if self.planar else frame.to_bgr()

    def close(self):
        self.file.close()


class VideoIO:
    def __init__(self, size, input_uri,
                 output_uri=None,
                 resolution=(1920, 1080),
                 frame_rate=30,
                 buffer_size=10,
                 proc_fps=30,
                 gpu_decode=False,
                 gpu_resize=False,
                 gpu_encode=False,
                 jpeg_quality=75,
                 yuv_matrix='bt601',
                 pixel_format=None,
                 demosaic='mhc',
                 white_balance=None,
                 black_level=0,
                 lens=None,
                 deep_color=False):
        """Parameters as fastmot/videoio.py:25-58, and (not in the reference; `"gpu_decode": true` / `"gpu_resize": true`
        in the configuration file's stream_cfg reach it through an unmodified app.py):
        gpu_decode: an image sequence's baseline JPEG files whose size is `size` are returned by `read` as JPEGFrames
            -- Huffman-decoded on the capture thread, everything else of the decode done on the GPU by the stage that
            uploads the frame (MOT.step takes them like ndarrays).  Any other file (a PNG, a progressive JPEG, a frame
            that needs resizing) comes back as the BGR ndarray it does today, file by file; so does every file when
            an `output_uri` is set, because frames that are written or drawn on must be host pixels.
        gpu_resize: a frame whose size is not `size` is returned by `read` as a SourceFrame -- the frame as it was
            captured; the stage that uploads it resizes it on the GPU, with `resize_bgr`'s arithmetic bit for bit
            (MOT.step takes them like ndarrays) -- in place of being resized here, on the thread that calls `read`.
            A frame already at `size` comes back as it does today.  Together with gpu_decode, supported baseline JPEG
            files of ANY size come back as JPEGFrames, those of another size than `size` wrapped in a SourceFrame.
            With an `output_uri` everything stays host pixels, as above.
        gpu_encode (`"gpu_encode": true`; jpeg_quality 1..100 goes with it): `write(frame)` to a 'dir/%06d.jpg' / '.jpeg'
            output encodes the frame on the GPU (utils.jpeg.encode_bgr: baseline 4:2:0 with libjpeg's arithmetic) in place
            of the Pillow save, and an `output_uri` ending in '.mjpeg' -- the same files, one behind the other in one file
            -- is accepted.  `write` then also takes `bytes` that already are a JPEG file (MOT.encode_frame: the frame
            the tracker saw, encoded where it lies on the GPU) and writes them as they are; with such an output the
            frames need not be host pixels, so gpu_decode / gpu_resize stay in effect.  '.png' and '.npy' outputs are
            untouched by the flag; without it everything is as it was.
        '.y4m' input (YUV4MPEG2; `cap_fps` is the header's frame rate, `frame_rate` when the header has none): frames are
            converted to BGR here with utils.yuv.planar_to_bgr and `yuv_matrix` ('bt601' / 'bt709'; the format does not
            say which); with gpu_decode `read` returns them as PlanarFrames instead -- 1.5 bytes per pixel are uploaded
            and csrc/yuv.hip converts them, bit for bit the same pixels --, those of another size than `size` wrapped in
            a SourceFrame under gpu_resize and converted and resized here without it.
        '.y4m' output (4:2:0, BT.601 limited range; the header is written with the first frame, from its size and
            `frame_rate`): `write` takes host pixels -- converted with utils.yuv.bgr_to_planar420, on the GPU with
            gpu_encode -- or an utils.yuv.I420Image (MOT.export_frame_i420: the frame the tracker saw, converted where
            it lies on the GPU), written as it is.  With gpu_encode and such an output the frames need not be host
            pixels, so gpu_decode / gpu_resize stay in effect, as for '.mjpeg'.
        pixel_format (`"pixel_format": "yuy2"` in stream_cfg; None: everything as it was): the layout of a '.npy' frame
            stack that holds frames as a camera, a capture card or an image library hands them out -- a key of
            utils.packed.FORMATS: 'rgb', 'bgr', 'rgbx' / 'rgba', 'bgrx' / 'bgra', 'xrgb' / 'argb', 'xbgr' / 'abgr',
            'yuy2' / 'yuyv', 'uyvy', 'yvyu'.  The stack is uint8 (N, H, W, 3 | 4) for the RGB family or (N, H, row bytes)
            for any layout (row bytes = bytes per pixel * W; 4 * ceil(W / 2) for 4:2:2, read as W = row bytes / 2); any
            other shape, and any other kind of input, is a ValueError when the stream is opened.  Frames are converted
            to BGR here with utils.packed.packed_to_bgr and, for 4:2:2, `yuv_matrix` -- which for this option alone also
            takes 'bt601-full' / 'bt709-full', a camera's full-range YCbCr; with gpu_decode `read` returns them as
            PackedFrames instead and csrc/packed.hip converts them, bit for bit the same pixels, those of another size
            than `size` wrapped in a SourceFrame under gpu_resize -- the '.y4m' input's rules for both flags.
            Bayer keys -- 'rggb', 'grbg', 'gbrg', 'bggr' for a uint8 stack (N, H, W) of raw mosaics, the same with '10',
            '12', '14' or '16' behind them ('rggb12') for a uint16 stack of that depth -- follow the same rules with
            utils.bayer.bayer_to_bgr, BayerFrames and csrc/bayer.hip; `demosaic` ('mhc' / 'bilinear'), `white_balance`
            (gains (R, G, B); None: 1.0 each) and `black_level` (in sample units) go with them and with nothing else.
        lens (`"lens": {"model": "pinhole" | "fisheye", "camera_matrix": ..., "dist_coeffs": ..., "zoom": 1.0,
            "border": [b, g, r]}` in stream_cfg, or a utils.lens.LensMap; None: everything as it was): every frame is
            undistorted -- and brought to `size` by the same map -- in place of being resized.  The LensMap is built once,
            from the first frame's resolution (`self.lens`).  Where `read` would return a SourceFrame under gpu_resize it
            returns `SourceFrame(frame, lens=self.lens)`, also for frames already at `size`, and csrc/remap.hip corrects
            them on the GPU; in every other case `read` applies utils.lens.remap_bgr here, on the thread that calls it,
            and returns host pixels (GPU frame kinds of gpu_decode are then converted here too).  The flags decide where
            the work happens, never what the pixels are.
        deep_color (`"deep_color": true` in stream_cfg; False: everything as it was, error messages included): a '.y4m'
            input of 9- to 16-bit samples -- C420p9 / p10 / p12 / p14 / p16, the C422p* and C444p* forms, Cmono9 / 10 /
            12 / 16; little-endian 16-bit words, limited range -- opens.  Its frames are converted to BGR here with
            utils.deep.deep_to_bgr, at full precision, and `yuv_matrix`, which for such a stream, and only there, also
            takes 'bt2020'; with gpu_decode `read` returns them as DeepFrames instead -- 3 bytes per pixel are uploaded
            for 4:2:0 and csrc/deep.hip converts them, bit for bit the same pixels --, those of another size than `size`
            wrapped in a SourceFrame under gpu_resize, and with `lens` under the rules above: the 8-bit '.y4m'
            input's rules for every flag.  An 8-bit '.y4m' file reads as it does without the flag.  XCOLORRANGE=FULL
            and interlaced material stay refused."""
        self.size = tuple(size)
        self.input_uri = input_uri
        self.output_uri = output_uri
        self.resolution = resolution
        assert frame_rate > 0
        self.frame_rate = frame_rate
        assert buffer_size >= 1
        self.buffer_size = buffer_size
        assert proc_fps > 0
        self.proc_fps = proc_fps

        self.protocol = self._parse_uri(self.input_uri)
        self.is_live = self.protocol != Protocol.IMAGE and self.protocol != Protocol.VIDEO
        self.gpu_decode = bool(gpu_decode)
        self.gpu_resize = bool(gpu_resize)
        self.gpu_encode = bool(gpu_encode)
        self.jpeg_quality = int(jpeg_quality)
        if self.gpu_encode and not 1 <= self.jpeg_quality <= 100:
            raise ValueError(f'jpeg_quality {jpeg_quality} outside 1..100')
        out = str(output_uri).lower() if output_uri is not None else ''
        self._mjpeg_out = self.gpu_encode and out.endswith('.mjpeg')
        self._jpeg_out = self._mjpeg_out or (self.gpu_encode and '%' in out and out.endswith(('.jpg', '.jpeg')))
        self._y4m_out = out.endswith('.y4m')
        self.i420_output = self._y4m_out and self.gpu_encode       # `write` takes MOT.export_frame_i420() for GPU-only frames
        # frames that Pillow / numpy write
        host_pixels = output_uri is not None and not self._jpeg_out and not (self._y4m_out and self.gpu_encode)
        self._wrap_sources = self.gpu_resize and not host_pixels
        # a lens without gpu_resize is applied to host pixels: nothing may stay a GPU frame kind then
        gpu_kinds = not host_pixels and (lens is None or self._wrap_sources)
        if pixel_format is not None and not (self.protocol == Protocol.VIDEO and str(self.input_uri).endswith('.npy')):
            raise ValueError(f"pixel_format={pixel_format!r} describes a '.npy' frame stack, not {self.input_uri}")
        if self.protocol == Protocol.IMAGE:
            self.source = _ImageSequence(self.input_uri, self.size if self.gpu_decode and gpu_kinds else None,
                                         any_size=self._wrap_sources)
        elif self.protocol == Protocol.VIDEO and str(self.input_uri).endswith('.npy') and _bayer_format(pixel_format) is not None:
            from .utils.source import MAX_DIM
            on_gpu = self.gpu_decode and gpu_kinds
            pattern, depth = _bayer_format(pixel_format)
            self.source = _BayerStack(self.input_uri, pattern, depth, demosaic, white_balance, black_level,
                                      bayer=lambda size: on_gpu and max(size) <= MAX_DIM and (tuple(size) == self.size or self._wrap_sources))
        elif self.protocol == Protocol.VIDEO and str(self.input_uri).endswith('.npy') and pixel_format is not None:
            from .utils.source import MAX_DIM
            on_gpu = self.gpu_decode and gpu_kinds
            self.source = _PackedStack(self.input_uri, pixel_format, matrix=yuv_matrix, packed=lambda size: on_gpu and max(size) <= MAX_DIM and (
                tuple(size) == self.size or self._wrap_sources))
        elif self.protocol == Protocol.VIDEO and str(self.input_uri).endswith('.npy'):
            self.source = _FrameStack(self.input_uri)
        elif self.protocol == Protocol.VIDEO and str(self.input_uri).lower().endswith('.y4m'):
            from .utils.source import MAX_DIM
            on_gpu = self.gpu_decode and gpu_kinds
            self.source = _Y4MStream(self.input_uri, matrix=yuv_matrix, deep=bool(deep_color), planar=lambda size: on_gpu and max(size) <= MAX_DIM and (
                tuple(size) == self.size or self._wrap_sources))
        else:
            raise NotImplementedError(f'{self.input_uri}: {self.protocol.name} sources need a video decoder '
                                      '(supported here: image sequences, .npy frame stacks and .y4m streams)')

        self.frame_queue = deque([], maxlen=self.buffer_size)
        self.cond = threading.Condition()
        self.exit_event = threading.Event()
        self.cap_thread = threading.Thread(target=self._capture_frames, daemon=True)

        frame = self.source.read()
        if frame is None:
            raise RuntimeError('Unable to read video stream')
        self.frame_queue.append(frame)

        height, width = frame.shape[:2]
        self.resolution = (width, height)
        self.cap_fps = getattr(self.source, 'fps', None) or self.frame_rate     # (only a .y4m stream carries a frame rate)
        self.do_resize = (width, height) != self.size
        self.lens = None
        if lens is not None:
            from .utils.lens import LensMap
            self.lens = lens if isinstance(lens, LensMap) else LensMap.from_config(lens, (width, height), self.size)
            if self.lens.src_size != (width, height) or self.lens.dst_size != self.size:
                raise ValueError(f'the lens map is {self.lens.src_size} -> {self.lens.dst_size}, the stream {(width, height)} -> {self.size}')
        LOGGER.info('%dx%d stream @ %d FPS', width, height, self.cap_fps)

        self._written = 0
        self._stack = None
        self._mjpeg = None
        self._y4m = None
        self._y4m_size = None
        if self.output_uri is not None:
            Path(self.output_uri).parent.mkdir(parents=True, exist_ok=True)
            if str(self.output_uri).endswith('.npy'):
                self._stack = []
            elif self._mjpeg_out:
                self._mjpeg = open(self.output_uri, 'wb')
            elif self._y4m_out:
                self._y4m = open(self.output_uri, 'wb')
            elif '%' not in str(self.output_uri):
                raise NotImplementedError(f'{self.output_uri}: video encoding needs an encoder '
                                          "(supported here: image sequences 'dir/%06d.png', .npy and .y4m)")

    @property
    def cap_dt(self):
        # limit capture interval at processing latency for live sources
        return 1 / min(self.cap_fps, self.proc_fps) if self.is_live else 1 / self.cap_fps

    def start_capture(self):
        """Start capturing from file or device."""
        if not self.cap_thread.is_alive():
            self.cap_thread.start()

    def stop_capture(self):
        """Stop capturing from file or device."""
        with self.cond:
            self.exit_event.set()
            self.cond.notify()
        self.frame_queue.clear()
        if self.cap_thread.is_alive():
            self.cap_thread.join()

    def read(self):
        """Reads the next video frame (None if there are no more frames)."""
        with self.cond:
            while len(self.frame_queue) == 0 and not self.exit_event.is_set():
                self.cond.wait()
            if len(self.frame_queue) == 0 and self.exit_event.is_set():
                return None
            frame = self.frame_queue.popleft()
            self.cond.notify()
        if self.lens is not None:
            if self._wrap_sources:
                from .utils.source import SourceFrame
                return SourceFrame(frame, lens=self.lens)
            from .utils.lens import remap_bgr
            return remap_bgr(frame, self.lens)
        if self._wrap_sources:
            from .utils.source import MAX_DIM, SourceFrame
            if not isinstance(frame, np.ndarray):                 # a JPEGFrame / PlanarFrame / PackedFrame / BayerFrame / DeepFrame, of any size
                return frame if frame.size == self.size else SourceFrame(frame)
            if self.do_resize and frame.shape[:2] != self.size[::-1] and max(frame.shape[:2]) <= MAX_DIM:
                return SourceFrame(frame)
        if self.do_resize and isinstance(frame, np.ndarray):      # (without gpu_resize a JPEGFrame has the wanted size by construction)
            frame = resize_bgr(frame, self.size)
        return frame

    def write(self, frame):
        """Writes the next video frame."""
        assert self.output_uri is not None
        if self._y4m is not None:
            self._write_y4m(frame)
        elif self._jpeg_out:
            if isinstance(frame, (bytes, bytearray, memoryview)):
                data = bytes(frame)
                if data[:2] != b'\xff\xd8':
                    raise ValueError('bytes handed to write must be a JPEG file')
            elif isinstance(frame, np.ndarray):
                from .utils.jpeg import encode_bgr
                data = encode_bgr(frame, self.jpeg_quality)
            else:
                raise TypeError(f'write takes host pixels or JPEG bytes; a {type(frame).__name__} lives on the GPU: '
                                'write MOT.encode_frame() for it')
            if self._mjpeg is not None:
                self._mjpeg.write(data)
            else:
                Path(str(self.output_uri) % self._written).write_bytes(data)
        elif self._stack is not None:
            self._stack.append(np.array(frame))
        else:
            from PIL import Image
            Image.fromarray(np.ascontiguousarray(frame[:, :, ::-1])).save(str(self.output_uri) % self._written)
        self._written += 1

    def _write_y4m(self, frame):
        from .utils import yuv
        if isinstance(frame, yuv.I420Image):
            size, data = frame.size, frame.data
        elif isinstance(frame, np.ndarray):
            if frame.ndim != 3 or frame.shape[2] != 3 or frame.dtype != np.uint8:
                raise ValueError('frame must be uint8 HxWx3')
            size = frame.shape[1::-1]
            if self.gpu_encode:
                from .runtime import get_context
                data = get_context().i420_from_bgr(frame)
            else:
                data = np.concatenate([p.reshape(-1) for p in yuv.bgr_to_planar420(frame)])
        else:
            raise TypeError(f'write takes host pixels or an I420Image; a {type(frame).__name__} lives on the GPU: '
                            'write MOT.export_frame_i420() for it')
        if self._y4m_size is None:
            self._y4m.write(yuv.y4m_header(size[0], size[1], yuv.fps_ratio(self.frame_rate)))
            self._y4m_size = tuple(size)
        elif tuple(size) != self._y4m_size:
            raise ValueError(f'frame is {size[0]}x{size[1]}, the stream {self._y4m_size[0]}x{self._y4m_size[1]}')
        self._y4m.write(yuv.FRAME_MAGIC + b'\n')
        self._y4m.write(memoryview(np.ascontiguousarray(data)))

    def release(self):
        """Cleans up input and output sources."""
        self.stop_capture()
        if self._y4m is not None:
            self._y4m.close()
            self._y4m = None
        if hasattr(self.source, 'close'):
            self.source.close()
        if self._mjpeg is not None:
            self._mjpeg.close()
            self._mjpeg = None
        if self._stack is not None and self._stack:
            np.save(self.output_uri, np.stack(self._stack))

    def _capture_frames(self):
        while not self.exit_event.is_set():
            frame = self.source.read()
            with self.cond:
                if frame is None:
                    self.exit_event.set()
                    self.cond.notify()
                    break
                # keep unprocessed frames in the buffer for file
                if not self.is_live:
                    while (len(self.frame_queue) == self.buffer_size and
                           not self.exit_event.is_set()):
                        self.cond.wait()
                self.frame_queue.append(frame)
                self.cond.notify()

    @staticmethod
    def _parse_uri(uri):
        result = urlparse(str(uri))
        if result.scheme == 'csi':
            protocol = Protocol.CSI
        elif result.scheme == 'rtsp':
            protocol = Protocol.RTSP
        elif result.scheme == 'http':
            protocol = Protocol.HTTP
        else:
            if '/dev/video' in result.path:
                protocol = Protocol.V4L2
            elif '%' in result.path:
                protocol = Protocol.IMAGE
            else:
                protocol = Protocol.VIDEO
        return protocol
