"""Object crops as JPEG files (fm_frame_encode_regions, MOT.encode_objects): the shapes test_objenc_host.py and
test_objenc_gpu.py share, and the numpy reference.  The reference of one file is: clip the rectangle to the frame ->
reduce the crop by `shrink` with the block mean (sum + n / 2) / n over the pixels of each s x s block that lie inside
the crop -> Pillow's own encode, jpeg_cases.encode(rgb, '420', q, restart_marker_rows=1)."""
import functools

import numpy as np

import jpeg_cases as jc

FRAME = (96, 160)                       # (width, height) of the rect-list frame
QUALITIES = (30, 75, 95, 100)
# before clipping; what each covers is in the issue's table
RECTS = [(0, 0, 0, 0),                  # 1 x 1
         (5, 3, 20, 18),                # 16 x 16 at an odd byte offset
         (7, 9, 23, 41),                # 17 x 33: its padding must not be the frame's neighbours
         (80, 144, 95, 159),            # flush with the corner
         (-10, -6, 12, 9),              # clipped to 13 x 10
         (90, 150, 120, 200),           # clipped to 6 x 10
         (200, 200, 210, 210),          # omitted
         (0, 0, 95, 159),               # the whole frame
         (40, 0, 55, 159),              # 10 MCU rows: RST wraps and restarts
         (7, 9, 23, 41),                # duplicate of the third
         (0, 50, 95, 65)]               # one row of 6 MCUs
WHOLE, TALL, THIRD, DUPLICATE = 6, 7, 2, 8         # indices into clipped(RECTS, FRAME) (the omitted one is gone)


def clip(rect, size):
    x0, y0, x1, y1 = max(rect[0], 0), max(rect[1], 0), min(rect[2], size[0] - 1), min(rect[3], size[1] - 1)
    return None if x1 < x0 or y1 < y0 else (x0, y0, x1, y1)


def clipped(rects, size):
    """The rectangles that have a pixel inside the frame, clipped, as an (n, 4) int32 array."""
    kept = [c for c in (clip(r, size) for r in rects) if c is not None]
    return np.array(kept, np.int32).reshape(-1, 4)


def shrink_mean(img, s):
    """[h, w, 3] uint8 -> [ceil(h / s), ceil(w / s), 3]: the rounded mean of every s x s block, edge blocks over fewer pixels."""
    if s == 1:
        return img
    h, w = img.shape[:2]
    H, W = -(-h // s), -(-w // s)
    pad = np.zeros((H * s, W * s, 3), np.int64)
    pad[:h, :w] = img
    ones = np.zeros((H * s, W * s), np.int64)
    ones[:h, :w] = 1
    total = pad.reshape(H, s, W, s, 3).sum((1, 3))
    n = ones.reshape(H, s, W, s).sum((1, 3))[:, :, None]
    return ((total + n // 2) // n).astype(np.uint8)


def reference(bgr, rect, quality, shrink=1):
    """The file of one CLIPPED rectangle of a BGR picture."""
    x0, y0, x1, y1 = (int(v) for v in rect)
    crop = shrink_mean(bgr[y0:y1 + 1, x0:x1 + 1], shrink)
    return jc.encode(np.ascontiguousarray(crop[:, :, ::-1]), '420', quality, restart_marker_rows=1)


@functools.lru_cache(maxsize=None)
def frame_bgr(kind):
    """The rect-list frame: 'noise' (seed 1) or 'checkerboard', BGR, read-only."""
    rgb = jc.content(kind, *FRAME, seed=1)
    bgr = np.ascontiguousarray(rgb[:, :, ::-1])
    bgr.setflags(write=False)
    return bgr


@functools.lru_cache(maxsize=None)
def references(kind, quality, shrink=1):
    """The reference files of RECTS on frame_bgr(kind): computed once, shared by the tests."""
    return tuple(reference(frame_bgr(kind), r, quality, shrink) for r in clipped(RECTS, FRAME))


def random_rects(n, size, seed):
    """n seeded rectangles inside a frame of `size`, sides 1..64, every corner parity."""
    rng = np.random.default_rng(seed)
    w = rng.integers(1, 65, n)
    h = rng.integers(1, 65, n)
    x0 = rng.integers(0, size[0] - w + 1)
    y0 = rng.integers(0, size[1] - h + 1)
    return np.stack([x0, y0, x0 + w - 1, y0 + h - 1], 1).astype(np.int32)


def rst_markers(data):
    """The RSTn markers of a file's scan, in order."""
    from fastmot_amd.utils import jpeg as J
    scan = data[J.parse(data).scan_offset:]
    return [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
