"""Overlays on the GPU against the host path they replace for a frame that lives on the device, at 1280x720 and 1920x1080,
a scene of 50 tracks with every Visualizer flag on (trajectories, object and background flow, covariances, detections with
confidence, KLT boxes, caption), in one process, each path in a loop of its own:

(a) fm_frame_render_overlay: HIP-event time of the kernel (fm_overlay_stream_ms) and the host time of the call (list and
    masks staged and copied, kernel, wait);
(b) what MOT.render_frame does around it: utils.overlay.build_commands, the render, the download of the picture;
(c) the host path: ctx.frame_read() + Visualizer.render on the downloaded array.

    python scripts/overlay_timing.py [--iters 40] [--out profiles/overlay.txt]"""
import argparse
import sys
import time
from collections import deque
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

FLAGS = dict(draw_detections=True, draw_confidence=True, draw_covariance=True, draw_klt=True, draw_obj_flow=True,
             draw_bg_flow=True, draw_trajectory=True)


def med(x):
    return float(np.median(x))


def fmt(v):
    return f'median {med(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}'


def scene(w, h, n_tracks=50, seed=0):
    rng = np.random.default_rng(seed)
    tracks = []
    for i in range(n_tracks):
        bw, bh = rng.uniform(0.03, 0.08) * w, rng.uniform(0.1, 0.25) * h
        x0, y0 = rng.uniform(-0.02 * w, w - bw), rng.uniform(-0.02 * h, h - bh)
        v = rng.normal(0, 3, 2)
        boxes = deque([np.array([x0, y0, x0 + bw, y0 + bh]) + np.tile(v, 2) * k for k in range(-29, 1)], maxlen=30)
        a = rng.normal(size=(4, 4))
        cov = np.zeros((8, 8))
        cov[:4, :4] = a @ a.T * 8 + np.eye(4)
        kp = np.stack([rng.uniform(x0, x0 + bw, 40), rng.uniform(y0, y0 + bh, 40)], axis=1).astype(np.float32)
        tracks.append(SimpleNamespace(trk_id=i * 7 + 1, tlbr=boxes[-1], bboxes=boxes, state=(np.zeros(8), cov), keypoints=kp,
                                      prev_keypoints=(kp + rng.normal(0, 2, kp.shape)).astype(np.float32)))
    dets = np.rec.array([(tuple(t.tlbr + rng.normal(0, 2, 4)), 1, float(rng.uniform(0.3, 1))) for t in tracks],
                        dtype=[('tlbr', float, 4), ('label', int), ('conf', float)])
    klt = [t.tlbr + rng.normal(0, 2, 4) for t in tracks]
    bg = np.stack([rng.uniform(0, w, 300), rng.uniform(0, h, 300)], axis=1).astype(np.float32)
    return tracks, dets, klt, (bg + rng.normal(0, 2, bg.shape)).astype(np.float32), bg, f'visible: {n_tracks}'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from fastmot_amd.runtime import get_context
    from fastmot_amd.utils.overlay import build_commands
    from fastmot_amd.utils.visualization import Visualizer
    ctx = get_context()
    vis = Visualizer(**FLAGS)
    lines = []
    for w, h in ((1280, 720), (1920, 1080)):
        frame = np.random.default_rng(1).integers(0, 256, (h, w, 3), dtype=np.uint8)
        ctx.frame_configure(w, h, 0)
        ctx.frame_upload(frame)
        sc = scene(w, h)
        cmds, masks = build_commands(vis, *sc, (w, h))
        for _ in range(5):
            ctx.frame_render_overlay(cmds, masks)
        host_ref = frame.copy()
        vis.render(host_ref, *sc[:5], caption=sc[5])
        same = np.array_equal(ctx.overlay_read(), host_ref)
        dev, call, build, whole, host = [], [], [], [], []
        # three loops, one per path: frame_read synchronises the whole device and Pillow keeps the thread busy for tens
        # of milliseconds, neither of which belongs between two render calls that are being timed
        for _ in range(args.iters):
            t0 = time.perf_counter()
            ctx.frame_render_overlay(cmds, masks)
            call.append((time.perf_counter() - t0) * 1e3)
            dev.append(ctx.overlay_stream_ms())
        for _ in range(args.iters):
            t0 = time.perf_counter()
            c, m = build_commands(vis, *sc, (w, h))
            t1 = time.perf_counter()
            ctx.frame_render_overlay(c, m)
            ctx.overlay_read()
            t2 = time.perf_counter()
            build.append((t1 - t0) * 1e3)
            whole.append((t2 - t0) * 1e3)
        for _ in range(args.iters):
            t0 = time.perf_counter()
            out = ctx.frame_read()
            vis.render(out, *sc[:5], caption=sc[5])
            host.append((time.perf_counter() - t0) * 1e3)
        lines.append(f'{w}x{h}, 50 tracks, all flags: {len(cmds)} commands, {len(masks)} mask bytes, {args.iters} rounds; '
                     f'picture equals Visualizer.render: {same}')
        lines.append(f'(a) overlay kernel (HIP events):              {fmt(dev)}')
        lines.append(f'(a) fm_frame_render_overlay on the host:      {fmt(call)}')
        lines.append(f'(b) build_commands:                           {fmt(build)}')
        lines.append(f'(b) build + render + overlay_read:            {fmt(whole)}')
        lines.append(f'(c) frame_read + Visualizer.render (Pillow):  {fmt(host)}')
        lines.append(f'(b) / (c): {med(whole) / med(host):.2f}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
