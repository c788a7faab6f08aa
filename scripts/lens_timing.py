"""Lens correction on the GPU against the resize it replaces and against the host, for 1920x1080 sources, in one process.

Cases: 1080p -> 720p and 1080p -> 1080p, from page-locked BGR and from page-locked NV12, with the barrel map of
tests/lens_cases.py carried to 1080p.  For each, through fm_frame_upload_ahead_src + fm_frame_promote_next:
  * the remap kernel (HIP events: trace marks 38 .. 31), the slot's whole stream time (marks 30 .. 31: copy, conversion,
    kernel) and the host time of the upload call (asynchronous: what the calling thread pays);
  * the same frames with no lens set -- fm_resize_bgr in the kernel's place (1080p -> 1080p without a lens is the plain
    upload: no kernel at all);
  * utils.lens.remap_bgr of the frame on the host, what a capture thread without the feature would run per frame.

    python scripts/lens_timing.py [--iters 60] [--out profiles/lens_remap.txt]"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(1, str(ROOT / 'tests'))

import lens_cases as lc  # noqa: E402

SRC = (1920, 1080)


def med(x):
    return float(np.median(x))


def fmt(v):
    return f'median {med(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}' if len(v) else 'none (no kernel is launched)'


def barrel(dst):
    from fastmot_amd import LensMap
    s = SRC[0] / lc.SRC[0]
    k = [420. * s, 415. * s, (322.5 + 0.5) * s - 0.5, (178.25 + 0.5) * s - 0.5]
    return LensMap.pinhole(k, lc.D_BARREL, SRC, dst)


def sources(ctx, n):
    """n page-locked BGR frames and n page-locked NV12 frames of the source size, random content."""
    from fastmot_amd import NV12Frame, _lib
    rng = np.random.default_rng(0)
    w, h = SRC
    bgr = ctx.pinned_source_frames(n, SRC)
    bgr[...] = rng.integers(0, 256, bgr.shape, dtype=np.uint8)
    buf = _lib.pinned_empty(ctx.lib, (n, h + h // 2, w), np.uint8)
    buf[...] = rng.integers(0, 256, buf.shape, dtype=np.uint8)
    return [bgr[i] for i in range(n)], [NV12Frame(buf[i, :h], buf[i, h:]) for i in range(n)]


def measure(ctx, frames, iters):
    """-> (kernel ms, stream ms, host ms of the call) per upload, after 5 warm-up uploads."""
    for i in range(5):
        ctx.frame_upload_ahead(1, frames[i % len(frames)])
        ctx.frame_promote_next()
    ctx.trace_start(8 * iters + 64)
    host = []
    for i in range(iters):
        f = frames[i % len(frames)]
        t0 = time.perf_counter()
        ctx.frame_upload_ahead(1, f)
        host.append((time.perf_counter() - t0) * 1e3)
        ctx.frame_promote_next()
    tags, ms = ctx.trace_read()
    kernel, stream = [], []
    t30 = t38 = None
    for tag, t in zip(tags, ms):
        if tag == 30:
            t30, t38 = float(t), None
        elif tag == 38:
            t38 = float(t)
        elif tag == 31 and t30 is not None:
            stream.append(float(t) - t30)
            if t38 is not None:
                kernel.append(float(t) - t38)
            t30 = None
    return kernel, stream, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=60)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'lens_remap.txt'))
    args = ap.parse_args()
    from fastmot_amd import SourceFrame
    from fastmot_amd.runtime import get_context
    from fastmot_amd.utils.lens import remap_bgr
    ctx = get_context()
    lines = [f'scripts/lens_timing.py on {ctx.device_info()["arch"]}; {SRC[0]}x{SRC[1]} page-locked sources, barrel map, {args.iters} uploads per line '
             '(fm_frame_upload_ahead_src + fm_frame_promote_next); kernel / stream: HIP events, call: host perf_counter']
    bgr, nv12 = sources(ctx, 4)
    done = 0
    for dst in ((1280, 720), (1920, 1080)):
        ctx.frame_configure(dst[0], dst[1], 0)
        lens = barrel(dst)
        map_mb, out_mb = lens.xy.nbytes / 1e6, dst[0] * dst[1] * 3 / 1e6
        lines.append(f'--- {SRC[0]}x{SRC[1]} -> {dst[0]}x{dst[1]}: map {map_mb:.1f} MB (int32 pairs), frame written {out_mb:.1f} MB')
        for kind, frames in (('BGR ', bgr), ('NV12', nv12)):
            for label, wrapped in (('lens   ', [SourceFrame(f, lens=lens) for f in frames]), ('no lens', [SourceFrame(f) for f in frames])):
                kernel, stream, host = measure(ctx, wrapped, args.iters)
                what = 'remap kernel ' if label.strip() == 'lens' else 'resize kernel'
                lines.append(f'{kind} {label}: {what} {fmt(kernel)}')
                lines.append(f'{kind} {label}: slot stream   {fmt(stream)}')
                lines.append(f'{kind} {label}: upload call   {fmt(host)}')
        ctx.frame_set_lens(None)
        t = []
        for i in range(3):
            t0 = time.perf_counter()
            remap_bgr(bgr[i], lens)
            t.append((time.perf_counter() - t0) * 1e3)
        lines.append(f'host utils.lens.remap_bgr (numpy) per frame: {fmt(t)}')
        print('\n'.join(lines[done:]), flush=True)
        done = len(lines)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
