"""JPEG test material shared by test_jpeg_host.py and test_jpeg_gpu.py: seeded images, encoded with Pillow at run time,
and Pillow's own decode of them (libjpeg-turbo), which is the judge of every comparison."""
import io
import itertools

import numpy as np
from PIL import Image

# (width, height): multiples of the block and the MCU, a single block, a single pixel (a one-sample chroma plane), sizes
# that are no multiple of 8 or 16 in either direction, several MCU rows and columns
SIZES = [(8, 8), (16, 16), (1, 1), (9, 17), (31, 33), (38, 50), (70, 130), (18, 258)]
SUBSAMPLINGS = ['444', '422', '420', 'grey']
QUALITIES = [30, 75, 95, 100]
CONTENTS = ['gradient', 'noise', 'checkerboard', 'black', 'white']
RESTARTS = [0, 2]


def content(kind, w, h, seed=0):
    """RGB test image [h, w, 3] uint8."""
    y, x = np.mgrid[0:h, 0:w]
    if kind == 'gradient':
        return np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(w + h - 2, 1)], 2).astype(np.uint8)
    if kind == 'noise':
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == 'checkerboard':          # 0 / 255 at pixel pitch: clamps and the largest coefficients
        return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)
    if kind == 'textured':              # smooth structure + noise, for frame-sized images
        img = np.stack([128 + 90 * np.sin(x / 7.) * np.cos(y / 11.), 128 + 80 * np.sin((x + y) / 5.), x * 255. / w], 2)
        return np.clip(img + np.random.default_rng(seed).normal(0, 12, img.shape), 0, 255).astype(np.uint8)
    return np.full((h, w, 3), {'black': 0, 'white': 255}[kind], np.uint8)


def encode(rgb, subsampling='420', quality=75, restart=0, **kw):
    """JPEG file bytes of an RGB image (its first channel for 'grey')."""
    args = dict(quality=quality, **kw)
    if subsampling == 'grey':
        im = Image.fromarray(np.ascontiguousarray(rgb[:, :, 0]))
    else:
        im = Image.fromarray(rgb)
        args['subsampling'] = {'444': 0, '422': 1, '420': 2}[subsampling]
    if restart:
        args['restart_marker_blocks'] = restart
    buf = io.BytesIO()
    im.save(buf, 'JPEG', **args)
    return buf.getvalue()


def pillow_bgr(data):
    """What the image-sequence source of videoio.py makes of the file."""
    with Image.open(io.BytesIO(data)) as im:
        return np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])


def cases(size, subsampling):
    """(label, file bytes) for every quality x content x restart setting at one size and subsampling."""
    w, h = size
    for q, kind, rst in itertools.product(QUALITIES, CONTENTS, RESTARTS):
        yield (size, subsampling, q, kind, rst), encode(content(kind, w, h, seed=w * 1000 + h), subsampling, q, rst)
