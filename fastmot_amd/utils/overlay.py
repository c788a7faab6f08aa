"""Visualizer.render as an overlay command list for the GPU (MOT(gpu_draw=True); fastmot_hip.h fm_frame_render_overlay).

`build_commands` emits the primitives of utils/visualization.py in the same order with the same integer geometry --
`tlbr.astype(int)` box corners, `np.rint` key points, every 4th box centre of a trajectory, the 73-point covariance
polylines with Pillow's float -> int truncation, the label background from `textbbox` and the text origin
`(x0 + 1, y0 - (t - y0) + 1)` -- so that the list rendered by the library equals what Pillow draws, bit for bit.  Text
becomes MASK commands: the glyph mask `font.getmask2` returns for the string, which is what `ImageDraw.text` blends.
The library knows no font; the masks are cached per string here (track ids and 'label: conf' texts repeat)."""
import numpy as np
from PIL import Image, ImageDraw, ImageFont

from .._lib import (OVERLAY_CMD_DTYPE, OVL_RECT_FILL, OVL_RECT_OUTLINE, OVL_LINE, OVL_DOT, OVL_MASK,
                    FM_OVERLAY_MAX_COORD)
from .visualization import get_color, covariance_ellipse

_TEXT_CACHE_MAX = 4096
_text_cache = {}
_font = None
_probe = None


def text_mask(text):
    """(alpha [h, w] uint8, (dx, dy) of the mask's top left pixel from the text origin, textbbox at origin (0, 0)) of
    `text` in Pillow's default font, as ImageDraw.text / textbbox use them."""
    global _font, _probe
    hit = _text_cache.get(text)
    if hit is not None:
        return hit
    if _font is None:
        _font = ImageFont.load_default()
        _probe = ImageDraw.Draw(Image.new('RGB', (1, 1)))
    core, offset = _font.getmask2(text, mode=_probe.fontmode)
    w, h = core.size
    alpha = np.frombuffer(bytes(core), np.uint8)[:w * h].reshape(h, w).copy() if w and h else np.zeros((0, 0), np.uint8)
    if _probe.fontmode != 'L':
        alpha = np.where(alpha > 0, 255, 0).astype(np.uint8)
    entry = (alpha, (int(offset[0]), int(offset[1])), tuple(int(v) for v in _probe.textbbox((0, 0), text, font=_font)))
    if len(_text_cache) >= _TEXT_CACHE_MAX:
        _text_cache.clear()
    _text_cache[text] = entry
    return entry


class _List:
    """Rows (kind, x0, y0, x1, y1, b, g, r, thickness, mask_off) and the mask blob of one frame."""

    def __init__(self):
        self.rows = []          # single commands since the last block
        self.blocks = []        # int64 [k, 10] arrays, in list order
        self.blob = bytearray()
        self.offsets = {}

    def flush(self):
        if self.rows:
            self.blocks.append(np.array(self.rows, np.int64))
            self.rows = []

    def add_many(self, kind, x0, y0, x1, y1, color):
        """One command per element of the coordinate arrays (the long runs: polylines, key points)."""
        self.flush()
        block = np.empty((len(x0), 10), np.int64)
        block[:, 0], block[:, 1], block[:, 2], block[:, 3], block[:, 4] = kind, x0, y0, x1, y1
        block[:, 5:8], block[:, 8], block[:, 9] = color, 1, 0
        self.blocks.append(block)

    def add(self, kind, x0, y0, x1, y1, color, thickness=1, mask_off=0):
        self.rows.append((kind, x0, y0, x1, y1, color[0], color[1], color[2], thickness, mask_off))

    def text(self, x, y, text, color):
        alpha, (dx, dy), _ = text_mask(text)
        if alpha.size == 0:
            return
        off = self.offsets.get(text)
        if off is None:
            off = self.offsets[text] = len(self.blob)
            self.blob += alpha.tobytes()
        self.add(OVL_MASK, x + dx, y + dy, alpha.shape[1], alpha.shape[0], color, mask_off=off)

    def polyline(self, xs, ys, color):
        xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
        self.add_many(OVL_LINE, xs[:-1], ys[:-1], xs[1:], ys[1:], color)

    def bbox(self, tlbr, color, thickness, text=None):
        x0, y0, x1, y1 = (int(v) for v in np.asarray(tlbr).astype(int))
        self.add(OVL_RECT_OUTLINE, min(x0, x1), min(y0, y1), max(x0, x1), max(y0, y1), color, thickness)
        if text is not None:
            l, t, r, b = text_mask(text)[2]
            self.add(OVL_RECT_FILL, x0, y0, x0 + (r - l) + 1, y0 + (b - t) + 2, color)
            self.text(x0 + 1, y0 - t + 1, text, (0, 0, 0))

    def feature_match(self, prev_pts, cur_pts, color):
        if len(cur_pts) == 0:
            return
        cur = np.rint(cur_pts).astype(np.int32).reshape(-1, 2)
        self.add_many(OVL_DOT, cur[:, 0], cur[:, 1], 0, 0, color)
        if len(prev_pts) > 0:
            prev = np.rint(prev_pts).astype(np.int32).reshape(-1, 2)
            n = min(len(prev), len(cur))
            self.add_many(OVL_LINE, prev[:n, 0], prev[:n, 1], cur[:n, 0], cur[:n, 1], color)

    def covariance(self, tlbr, covariance):
        x0, y0, x1, y1 = (int(v) for v in np.asarray(tlbr).astype(int))
        for (cx, cy), cov in (((x0, y0), covariance[:2, :2]), ((x1, y1), covariance[2:4, 2:4])):
            (a, b), angle = covariance_ellipse(cov)
            t = np.linspace(0, 2 * np.pi, 73)
            ca, sa = np.cos(np.radians(angle)), np.sin(np.radians(angle))
            xs = cx + a * np.cos(t) * ca - b * np.sin(t) * sa
            ys = cy + a * np.cos(t) * sa + b * np.sin(t) * ca
            # Pillow casts a float coordinate with (int): towards zero
            self.polyline(np.trunc(xs), np.trunc(ys), (255, 255, 255))


def build_commands(visualizer, tracks, detections, klt_bboxes, prev_bg_keypoints, bg_keypoints, caption, size):
    """The picture Visualizer.render(frame, tracks, detections, klt_bboxes, prev_bg_keypoints, bg_keypoints, caption)
    draws, as (cmds: ndarray of _lib.OVERLAY_CMD_DTYPE, masks: bytes) in painter's order.  Every primitive is emitted,
    inside the frame or not: the renderer clips, and its binning drops what touches no tile.  Coordinates are clamped to
    +-FM_OVERLAY_MAX_COORD (2^20), far beyond any frame.  `size` (w, h) is the frame's; the list does not depend on it."""
    out = _List()
    for track in tracks:
        color = get_color(track.trk_id)
        out.bbox(track.tlbr, color, 2, str(track.trk_id))
        if visualizer.draw_trajectory:
            boxes = np.reshape(list(track.bboxes), (len(track.bboxes), 4))[::4]
            centers = ((boxes[:, :2] + boxes[:, 2:]) / 2).astype(np.int32)
            if len(centers) > 1:
                out.polyline(centers[:, 0], centers[:, 1], color)
        if visualizer.draw_obj_flow:
            out.feature_match(track.prev_keypoints, track.keypoints, (0, 255, 255))
        if visualizer.draw_covariance:
            out.covariance(track.tlbr, track.state[1])
    if visualizer.draw_detections:
        for det in detections:
            out.bbox(det.tlbr, (255, 255, 255), 1, f'{det.label}: {det.conf:.2f}' if visualizer.draw_confidence else None)
    if visualizer.draw_klt:
        for tlbr in klt_bboxes:
            out.bbox(tlbr, (0, 0, 0), 1)
    if visualizer.draw_bg_flow:
        out.feature_match(prev_bg_keypoints, bg_keypoints, (0, 0, 255))
    if caption:
        out.text(30, 14, caption, (0, 0, 0))

    out.flush()
    if not out.blocks:
        return np.zeros(0, OVERLAY_CMD_DTYPE), b''
    rows = np.concatenate(out.blocks)
    cmds = np.zeros(len(rows), OVERLAY_CMD_DTYPE)
    kind = rows[:, 0]
    is_mask = kind == OVL_MASK
    lim = FM_OVERLAY_MAX_COORD
    x0, y0 = np.clip(rows[:, 1], -lim, lim), np.clip(rows[:, 2], -lim, lim)
    x1 = np.where(is_mask, rows[:, 3], np.clip(rows[:, 3], -lim, lim))
    y1 = np.where(is_mask, rows[:, 4], np.clip(rows[:, 4], -lim, lim))
    cmds['kind'], cmds['x0'], cmds['y0'], cmds['x1'], cmds['y1'] = kind, x0, y0, x1, y1
    cmds['color'] = rows[:, 5:8]
    cmds['thickness'] = rows[:, 8]
    cmds['mask_off'] = rows[:, 9]
    return cmds, bytes(out.blob)
