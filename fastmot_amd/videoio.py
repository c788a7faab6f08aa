"""VideoIO (API of fastmot/videoio.py:24-277) without OpenCV / GStreamer: threaded capture into a bounded
queue with the reference's semantics (file sources block when the buffer is full, live sources drop),
`cap_dt`, `read()`, `write()`, `release()`.

Sources this implementation can decode:
  * image sequences  'dir/%06d.jpg' (any format Pillow reads; the MOTChallenge layout)  -> Protocol.IMAGE
  * raw frame stacks '*.npy' ([N, H, W, 3] uint8 BGR, memory-mapped)                     -> Protocol.VIDEO
Video containers, cameras and network streams need a decoder this image does not have; they raise
NotImplementedError with the URI.  Outputs: image sequence ('out/%06d.png') or '*.npy'; with gpu_encode also
'*.mjpeg' (concatenated JPEG files), and '%06d.jpg' sequences are encoded on the GPU.

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
                 jpeg_quality=75):
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
            untouched by the flag; without it everything is as it was."""
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
        host_pixels = output_uri is not None and not self._jpeg_out      # frames that Pillow / numpy write
        self._wrap_sources = self.gpu_resize and not host_pixels
        if self.protocol == Protocol.IMAGE:
            self.source = _ImageSequence(self.input_uri, self.size if self.gpu_decode and not host_pixels else None,
                                         any_size=self._wrap_sources)
        elif self.protocol == Protocol.VIDEO and str(self.input_uri).endswith('.npy'):
            self.source = _FrameStack(self.input_uri)
        else:
            raise NotImplementedError(f'{self.input_uri}: {self.protocol.name} sources need a video decoder '
                                      '(supported here: image sequences and .npy frame stacks)')

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
        self.cap_fps = self.frame_rate          # neither source kind carries a frame rate
        self.do_resize = (width, height) != self.size
        LOGGER.info('%dx%d stream @ %d FPS', width, height, self.cap_fps)

        self._written = 0
        self._stack = None
        self._mjpeg = None
        if self.output_uri is not None:
            Path(self.output_uri).parent.mkdir(parents=True, exist_ok=True)
            if str(self.output_uri).endswith('.npy'):
                self._stack = []
            elif self._mjpeg_out:
                self._mjpeg = open(self.output_uri, 'wb')
            elif '%' not in str(self.output_uri):
                raise NotImplementedError(f'{self.output_uri}: video encoding needs an encoder '
                                          "(supported here: image sequences 'dir/%06d.png' and .npy)")

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
        if self._wrap_sources:
            from .utils.source import MAX_DIM, SourceFrame
            if not isinstance(frame, np.ndarray):                 # a JPEGFrame, of any size
                return frame if frame.size == self.size else SourceFrame(frame)
            if self.do_resize and frame.shape[:2] != self.size[::-1] and max(frame.shape[:2]) <= MAX_DIM:
                return SourceFrame(frame)
        if self.do_resize and isinstance(frame, np.ndarray):      # (without gpu_resize a JPEGFrame has the wanted size by construction)
            frame = resize_bgr(frame, self.size)
        return frame

    def write(self, frame):
        """Writes the next video frame."""
        assert self.output_uri is not None
        if self._jpeg_out:
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

    def release(self):
        """Cleans up input and output sources."""
        self.stop_capture()
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
