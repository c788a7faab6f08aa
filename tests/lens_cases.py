"""Shared by test_lens_host.py and test_lens_gpu.py: the lens models, the random maps and the boundary table."""
import numpy as np

from fastmot_amd import LensMap

SRC, DST = (640, 360), (426, 240)
K_PINHOLE = [[420., 0., 322.5], [0., 415., 178.25], [0., 0., 1.]]
K_FISHEYE = [[230., 0., 322.5], [0., 228., 178.25], [0., 0., 1.]]
D_BARREL = (-0.28, 0.09, 0.001, -0.0007, -0.012)
D_PINCUSHION = (0.12, -0.03, 0.0005, 0.0004, 0.)
D_FISHEYE = (-0.035, 0.012, -0.006, 0.0009)
BORDER = (7, 130, 255)

# (src, dst): smallest frame; one vector thread; the boundary table; byte path, odd everything; magnification on the
# vector path; the models' sizes (byte path, 426 % 8 = 2); an on-size source; the largest offsets
SHAPES = [((1, 1), (1, 1)), ((2, 2), (8, 1)), ((3, 3), (14, 14)), ((37, 29), (13, 7)), ((37, 29), (64, 48)),
          ((640, 360), (426, 240)), ((640, 360), (640, 360)), ((16384, 2), (24, 3))]
shape_id = lambda s: f'{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}'


def barrel(dst=DST, src=SRC, border=BORDER):
    return LensMap.pinhole(K_PINHOLE, D_BARREL, src, dst, border=border)


def pincushion(dst=DST, border=BORDER):
    return LensMap.pinhole(K_PINHOLE, D_PINCUSHION, SRC, dst, border=border)


def fisheye(zoom=1.0, dst=DST, border=BORDER):
    return LensMap.fisheye(K_FISHEYE, D_FISHEYE, SRC, dst, zoom=zoom, border=border)


def models(dst=DST):
    return {'barrel': barrel(dst), 'pincushion': pincushion(dst), 'fisheye': fisheye(1.0, dst), 'fisheye-zoom0.6': fisheye(0.6, dst)}


def random_lens(rng, src, dst, border=BORDER):
    """Coordinates drawn over [-2, sw + 1] x [-2, sh + 1]: all four sides and corners fall outside."""
    (sw, sh), (dw, dh) = src, dst
    return LensMap.from_arrays(rng.uniform(-2., sw + 1., (dh, dw)), rng.uniform(-2., sh + 1., (dh, dw)), src, border)


def boundary_values(s):
    return [-64, -33, -32, -31, -1, 0, 31, 32, 32 * (s - 1) - 1, 32 * (s - 1), 32 * (s - 1) + 1, 32 * s - 1, 32 * s, 32 * s + 32]


def boundary_lens(border=BORDER):
    """3 x 3 source, 14 x 14 destination: X runs over the boundary values along a row, Y down a column."""
    v = np.array(boundary_values(3), np.int32)
    xy = np.stack(np.meshgrid(v, v), axis=-1).astype(np.int32)
    return LensMap(xy, (3, 3), border)


def boundary_frames():
    """3 x 3 sources with values in {0, 255}: both constants, a checkerboard and its inverse, and a random one."""
    rng = np.random.default_rng(33)
    board = ((np.add.outer(np.arange(3), np.arange(3)) & 1) * 255).astype(np.uint8)
    out = [np.zeros((3, 3, 3), np.uint8), np.full((3, 3, 3), 255, np.uint8), np.repeat(board[..., None], 3, axis=2),
           np.repeat((255 - board)[..., None], 3, axis=2), (rng.integers(0, 2, (3, 3, 3)) * 255).astype(np.uint8)]
    return [np.ascontiguousarray(f) for f in out]


def lens_for(rng, src, dst):
    """The map the shape is tested with: the boundary table for 3x3 -> 14x14, a random map for every other shape."""
    return boundary_lens() if (src, dst) == ((3, 3), (14, 14)) else random_lens(rng, src, dst)
