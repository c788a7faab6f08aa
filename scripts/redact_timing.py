"""Redaction inside the overlay pass, at 1280x720 and 1920x1080, for the 50-track scene of scripts/overlay_timing.py (every
Visualizer flag on; regions: the 50 tracks and their 50 detections, Redact's defaults per mode), in one process:

(a) fm_frame_render_redacted per mode: HIP-event time of the cell-mean kernel (fm_redact_stream_ms minus
    fm_overlay_stream_ms), of the tile pass (fm_overlay_stream_ms) and of both, beside fm_frame_render_overlay of the same
    scene -- the yardstick -- measured in the same loop, the two calls alternating;
(b) what MOT.render_frame / MOT.encode_frame do around it, with and without `redact`: build_regions + build_commands, the
    render, and the download of the picture or its JPEG encode.

    python scripts/redact_timing.py [--iters 40] [--out profiles/redact.txt]"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'scripts'))

from overlay_timing import FLAGS, scene, med, fmt      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from fastmot_amd.runtime import get_context
    from fastmot_amd.utils.overlay import build_commands
    from fastmot_amd.utils.redact import Redact, build_regions, redact_bgr
    from fastmot_amd.utils.visualization import Visualizer
    from fastmot_amd._lib import overlay_render_host
    ctx = get_context()
    vis = Visualizer(**FLAGS)
    lines = []
    for w, h in ((1280, 720), (1920, 1080)):
        frame = np.random.default_rng(1).integers(0, 256, (h, w, 3), dtype=np.uint8)
        ctx.frame_configure(w, h, 0)
        ctx.frame_upload(frame)
        sc = scene(w, h)
        tracks, dets = sc[0], sc[1]
        for t in tracks:
            t.active, t.label = True, 1
        cmds, masks = build_commands(vis, *sc, (w, h))
        lines.append(f'{w}x{h}, 50 tracks + 50 detections, all flags: {len(cmds)} commands, {args.iters} rounds')
        for mode in ('pixelate', 'smooth', 'fill'):
            cfg = Redact(mode=mode, shape='ellipse' if mode == 'smooth' else 'rect')
            regions = build_regions(tracks, dets, cfg, (w, h))
            for _ in range(5):
                ctx.frame_render_redacted(regions, cmds, masks)
            want = overlay_render_host(redact_bgr(frame.copy(), regions), cmds, masks)
            same = np.array_equal(ctx.overlay_read(), want)
            means, tile, both, plain, call, plain_call = [], [], [], [], [], []
            for _ in range(args.iters):
                t0 = time.perf_counter()
                ctx.frame_render_redacted(regions, cmds, masks)
                call.append((time.perf_counter() - t0) * 1e3)
                both.append(ctx.redact_stream_ms())
                tile.append(ctx.overlay_stream_ms())
                means.append(both[-1] - tile[-1])
                t0 = time.perf_counter()
                ctx.frame_render_overlay(cmds, masks)
                plain_call.append((time.perf_counter() - t0) * 1e3)
                plain.append(ctx.overlay_stream_ms())
            lines.append(f'  {mode} ({cfg.shape}), {len(regions)} regions, cells {int(regions["cell"].min())}..{int(regions["cell"].max())}; '
                         f'picture equals the host twin: {same}')
            lines.append(f'  (a) cell means (HIP events):                  {fmt(means)}')
            lines.append(f'  (a) tile pass with redaction (HIP events):    {fmt(tile)}')
            lines.append(f'  (a) both:                                     {fmt(both)}')
            lines.append(f'  (a) fm_frame_render_overlay, same scene:      {fmt(plain)}')
            lines.append(f'  (a) host time of the call, redacted / plain:  {med(call):.3f} / {med(plain_call):.3f} ms')
        cfg = Redact()
        for what, finish in (('render_frame', ctx.overlay_read), ('encode_frame(overlays=True)', lambda: ctx.overlay_encode_jpeg(75))):
            with_r, without = [], []
            for _ in range(args.iters):
                t0 = time.perf_counter()
                c, m = build_commands(vis, *sc, (w, h))
                ctx.frame_render_redacted(build_regions(tracks, dets, cfg, (w, h)), c, m)
                finish()
                with_r.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                c, m = build_commands(vis, *sc, (w, h))
                ctx.frame_render_overlay(c, m)
                finish()
                without.append((time.perf_counter() - t0) * 1e3)
            lines.append(f'  (b) {what}: lists + render + result, with redact:    {fmt(with_r)}')
            lines.append(f'  (b) {what}: lists + render + result, without:        {fmt(without)}')
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            redact_bgr(frame.copy(), build_regions(tracks, dets, cfg, (w, h)))
            t.append((time.perf_counter() - t0) * 1e3)
        lines.append(f'  host twin (copy + redact_bgr, one thread):     {fmt(t)}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
