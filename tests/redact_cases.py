"""Region lists shared by tests/test_redact_host.py and tests/test_redact_gpu.py: seeded noise frames (on gradients,
rounding and anchoring mistakes hide) and the rectangles at which the cell arithmetic can go wrong."""
import itertools

import numpy as np

import redact_ref as R

W, H = 37, 23                       # both sides odd
MODES = (R.PIXELATE, R.SMOOTH, R.FILL)
SHAPES = (R.RECT, R.ELLIPSE)


def noise(w, h, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# name -> (x0, y0, x1, y1, cell) on the W x H frame
RECTS = {
    'inside': (5, 4, 20, 15, 4),                          # 16 x 12: whole cells only
    'partial_last_cell': (5, 4, 21, 16, 5),               # 17 x 13: the last column and row of cells are 2 and 3 wide
    'left': (-6, 5, 10, 14, 4),
    'right': (30, 5, 44, 14, 4),
    'top': (8, -5, 20, 6, 3),
    'bottom': (8, 17, 20, 30, 6),
    'outside_right': (40, 5, 50, 10, 4),
    'outside_above': (-20, -20, -5, -5, 4),
    'larger': (-10, -8, 50, 40, 7),
    'much_larger': (-150, -100, 180, 130, 16),            # a^2 b^2 = 331^2 231^2 > 2^32
    'one_pixel': (7, 7, 7, 7, 2),
    'one_column': (9, 2, 9, 20, 3),                       # as an ellipse: 1 x N
    'one_row': (2, 11, 30, 11, 5),
    'cell_2': (3, 3, 12, 10, 2),
    'cell_256_one': (-100, -100, 140, 120, 256),          # a single existing cell
    'cell_256_two': (-250, -10, 60, 40, 256),             # the frame's columns 6.. lie in cell 1
    'single_cell': (10, 10, 12, 12, 4),                   # SMOOTH: every neighbour clamps
    'anchor_far_left': (-100, 3, 30, 18, 8),              # imin = 12, and cell 12 has only its last four columns
    'anchor_far_up': (4, -77, 33, 20, 5),
}


def single_lists():
    """name -> [region]: every rectangle in every mode and shape."""
    out = {}
    for (name, (x0, y0, x1, y1, c)), mode, shape in itertools.product(RECTS.items(), MODES, SHAPES):
        out[f'{name}-m{mode}-s{shape}'] = [R.region(x0, y0, x1, y1, mode, shape, c, (200, 10, 77))]
    return out


def overlapping():
    """Three regions that overlap each other, of mixed modes."""
    return [R.region(4, 3, 24, 16, R.PIXELATE, R.RECT, 5), R.region(12, 6, 33, 20, R.SMOOTH, R.ELLIPSE, 4),
            R.region(9, 9, 28, 13, R.FILL, R.RECT, 2, (1, 2, 3))]


def all_lists():
    out = single_lists()
    three = overlapping()
    out['overlap_abc'] = three
    out['overlap_cba'] = three[::-1]
    out['overlap_bca'] = [three[1], three[2], three[0]]
    out['with_empty'] = [R.region(10, 5, 9, 8), R.region(3, 8, 12, 7), three[0]]       # x1 < x0, y1 < y0: nothing
    out['empty'] = []
    return out


def tiled_lists(w, h):
    """For a frame of several 64 x 16 tiles: regions and cells (c = 24) that straddle the tile borders."""
    return {
        'straddle': [R.region(40, 5, 100, 40, R.PIXELATE, R.RECT, 24), R.region(50, 10, 129, 49, R.SMOOTH, R.ELLIPSE, 24),
                     R.region(60, 12, 70, 20, R.FILL, R.ELLIPSE, 2, (9, 8, 7)), R.region(-30, -9, 66, 17, R.SMOOTH, R.RECT, 24)],
        'whole': [R.region(0, 0, w - 1, h - 1, R.PIXELATE, R.ELLIPSE, 24)],
        'whole_smooth': [R.region(-5, -5, w + 5, h + 5, R.SMOOTH, R.RECT, 9)],
    }


def many(w, h, n, seed=3):
    """n person-sized regions of mixed modes and shapes scattered over (and past the edges of) a w x h frame."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        bw, bh = int(rng.integers(w // 30, w // 8)), int(rng.integers(h // 10, h // 3))
        x0, y0 = int(rng.integers(-bw // 2, w - bw // 2)), int(rng.integers(-bh // 2, h - bh // 2))
        side = max(bw, bh)
        out.append(R.region(x0, y0, x0 + bw - 1, y0 + bh - 1, MODES[k % 3], SHAPES[(k // 3) % 2], min(256, max(2, -(-side // 8))),
                            tuple(int(v) for v in rng.integers(0, 256, 3))))
    return out
