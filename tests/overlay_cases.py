"""Scenes and command lists shared by tests/test_overlay_host.py and tests/test_overlay_gpu.py."""
from collections import deque
from types import SimpleNamespace

import numpy as np

import overlay_ref as R
from fastmot_amd.utils.visualization import Visualizer

ALL_FLAGS = dict(draw_detections=True, draw_confidence=True, draw_covariance=True, draw_klt=True, draw_obj_flow=True,
                 draw_bg_flow=True, draw_trajectory=True)


def noise(w, h, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _track(trk_id, tlbr, n_hist, step, rng, n_kp=5):
    boxes = deque([np.asarray(tlbr, float) + np.asarray(step, float).repeat(2)[[0, 2, 1, 3]] * k for k in range(-n_hist + 1, 1)], maxlen=40)
    a = rng.normal(size=(4, 4))
    cov = np.zeros((8, 8))
    cov[:4, :4] = a @ a.T * 6 + np.eye(4)
    x0, y0, x1, y1 = boxes[-1]
    cur = np.stack([rng.uniform(x0, x1, n_kp), rng.uniform(y0, y1, n_kp)], axis=1).astype(np.float32)
    return SimpleNamespace(trk_id=trk_id, tlbr=boxes[-1], bboxes=boxes, state=(np.zeros(8), cov), keypoints=cur,
                           prev_keypoints=(cur + rng.normal(0, 3, cur.shape)).astype(np.float32))


def scene(w, h, seed=1):
    """Everything Visualizer.render can draw, scaled into a w x h frame: tracks with trajectories longer than 8 boxes
    (one id of three digits), boxes partly and wholly outside the frame, a box smaller than its outline's thickness, a box
    with inverted corners, object and background flow, covariances, detections with confidence text, KLT boxes, a caption."""
    rng = np.random.default_rng(seed)
    sx, sy = w / 160., h / 120.

    def box(x0, y0, x1, y1):
        return [x0 * sx + 0.3, y0 * sy + 0.6, x1 * sx + 0.3, y1 * sy + 0.6]
    tracks = [_track(7, box(20, 30, 60, 100), 13, (2.2 * sx, -1.4 * sy), rng),
              _track(407, box(90, 20, 130, 90), 21, (-1.5 * sx, 1.1 * sy), rng),
              _track(12, box(-15, 60, 18, 110), 9, (1.0 * sx, 0.5 * sy), rng),          # over the left edge
              _track(3, box(140, 95, 175, 140), 17, (0.7 * sx, 0.9 * sy), rng),         # over the bottom right corner
              _track(31, box(-80, -70, -30, -10), 10, (1.0 * sx, 1.0 * sy), rng),       # wholly outside
              _track(5, [w * 0.5, h * 0.4, w * 0.5 + 1.2, h * 0.4 + 2.5], 5, (0.5, 0.5), rng, n_kp=1)]   # degenerate at width 2
    dets = np.rec.array([(tuple(box(22, 28, 58, 97)), 1, 0.87), (tuple(box(88, 22, 133, 92)), 1, 0.5),
                         (tuple(box(150, -10, 190, 30)), 2, 0.31), (tuple(box(300, 300, 340, 360)), 1, 0.99)],
                        dtype=[('tlbr', float, 4), ('label', int), ('conf', float)])
    klt = [np.array(box(24, 33, 63, 104)), np.array(box(-12, 62, 20, 112)), np.array(box(100, 118, 120, 135)),
           np.array(box(75, 70, 66, 52))]                               # inverted corners: drawn normalised, as draw_bbox does
    bg_cur = np.stack([rng.uniform(-3, w + 3, 24), rng.uniform(-3, h + 3, 24)], axis=1).astype(np.float32)
    bg_prev = (bg_cur + rng.normal(0, 4, bg_cur.shape)).astype(np.float32)
    return tracks, dets, klt, bg_prev, bg_cur, f'visible: {len(tracks)}'


def scene_commands(w, h, flags=ALL_FLAGS, seed=1):
    from fastmot_amd.utils.overlay import build_commands
    tracks, dets, klt, bg_prev, bg_cur, caption = scene(w, h, seed)
    return build_commands(Visualizer(**flags), tracks, dets, klt, bg_prev, bg_cur, caption, (w, h))


def glyphs(text):
    from fastmot_amd.utils.overlay import text_mask
    return text_mask(text)[0]


def primitive_lists(w, h):
    """name -> (cmds, masks): each primitive kind alone, primitives wholly outside, lines from far outside."""
    blob = bytearray()
    m = glyphs('person: 0.87')
    out = {
        'empty': (np.zeros(0, R.OVERLAY_CMD_DTYPE), b''),
        'fill': (np.concatenate([R.rect_fill(5, 4, w // 2, h // 2, (10, 200, 30)), R.rect_fill(w - 9, h - 7, w + 20, h + 20, (1, 2, 3)),
                                 R.rect_fill(-5, -5, 2, 1, (255, 0, 255)), R.rect_fill(9, 9, 8, 12, (9, 9, 9))]), b''),
        'outline': (np.concatenate([R.rect_outline(3, 2, w - 4, h - 3, (0, 0, 255), 2), R.rect_outline(-4, 6, 30, h + 8, (250, 250, 0), 1),
                                    R.rect_outline(10, 10, 11, 11, (7, 70, 170), 2), R.rect_outline(20, 5, 20, 19, (90, 10, 0), 2),
                                    R.rect_outline(w - 20, 8, w - 6, 30, (5, 5, 5), 8), R.rect_outline(40, 12, 46, 15, (200, 100, 50), 3)]), b''),
        'line': (np.concatenate([R.line(2, 3, w - 3, h - 5, (255, 255, 255)), R.line(w - 1, 0, 0, h - 1, (0, 255, 0)),
                                 R.line(5, h // 2, w + 30, h // 2, (1, 1, 1)), R.line(w // 3, -9, w // 3, h + 9, (0, 0, 200)),
                                 R.line(8, 8, 8, 8, (255, 0, 0)), R.line(30, 2, 12, 20, (3, 30, 130)), R.line(12, 30, 33, 26, (99, 9, 199))]), b''),
        'dot': (np.concatenate([R.dot(0, 0, (0, 255, 255)), R.dot(w - 1, h - 1, (0, 0, 255)), R.dot(w // 2, 0, (255, 0, 0)),
                                R.dot(0, h // 2, (0, 255, 0)), R.dot(w // 2 + 1, h // 2, (9, 99, 199)), R.dot(w, h // 3, (50, 50, 50))]), b''),
        'far_line': (np.concatenate([R.line(-1000, -1000, 1000, 900, (255, 128, 0)),
                                     R.line(-(1 << 20), -(1 << 20) + 17, 1 << 20, (1 << 20) - 40, (0, 128, 255)),
                                     R.line((1 << 20), 3, -(1 << 20), h - 2, (128, 0, 255))]), b''),
        'outside': (np.concatenate([R.rect_fill(w, 0, w + 50, h, (1, 1, 1)), R.rect_outline(-60, -60, -2, -3, (2, 2, 2), 2),
                                    R.line(-50, -1, w + 50, -1, (3, 3, 3)), R.line(w + 5, -20, w + 80, h + 9, (4, 4, 4)),
                                    R.dot(-2, 5, (5, 5, 5)), R.dot(5, h + 1, (6, 6, 6)),
                                    R.mask(w, 3, m, (7, 7, 7), blob), R.mask(4, -m.shape[0], m, (8, 8, 8), blob)]), None),
    }
    out['outside'] = (out['outside'][0], bytes(blob))
    blob2 = bytearray()
    out['mask'] = (np.concatenate([R.mask(3, 4, m, (0, 0, 0), blob2), R.mask(-7, h - 5, glyphs('407'), (255, 40, 90), blob2),
                                   R.mask(w - 11, -3, glyphs('visible: 12'), (20, 220, 120), blob2), R.mask(w // 2, h // 2, glyphs('7'), (255, 255, 255), blob2)]),
                   bytes(blob2))
    return out


def painter_lists(w, h):
    """Painter's order across binning chunks: 700 filled rectangles over one tile, rectangle k in a colour of k, and the
    same with a line, a mask and an outline last over the same pixel."""
    k = np.arange(700)
    fills = np.zeros(700, R.OVERLAY_CMD_DTYPE)
    fills['kind'] = R.OVL_RECT_FILL
    fills['x0'], fills['y0'] = 2 + k % 5, 1 + k % 3
    fills['x1'], fills['y1'] = 40 - k % 7, 14 - k % 4
    fills['color'] = np.stack([k % 251, (k * 7) % 256, (k * 13 + 5) % 256], axis=1)
    blob = bytearray()
    return {'fills': (fills, b''),
            'line_last': (np.concatenate([fills, R.line(0, 0, 45, 15, (255, 255, 255))]), b''),
            'mask_last': (np.concatenate([fills, R.mask(8, 5, glyphs('407'), (0, 0, 0), blob)]), bytes(blob)),
            'outline_last': (np.concatenate([fills, R.rect_outline(6, 4, 30, 12, (0, 0, 255), 2)]), b'')}
