"""Tracked objects as JPEG crops: one pass of the GPU encoder for all crops of a frame against the two routes there were
before, on a 1920x1080 'textured' frame (tests/jpeg_cases.content) that lies on the device, at quality 85, in one process:

(a) ctx.frame_encode_regions (fm_frame_encode_regions) at shrink 1 and 2: HIP-event time of the launches on the encoder's
    stream, summed over the library calls of one list, and the host time of the whole Python call (table, launches, wait,
    assembling, bytes objects);
(b) the route without it: ctx.frame_read() + one utils.jpeg.encode_bgr (upload, five launches, synchronise, read-back)
    per crop;
(c) ctx.frame_read() + one Pillow save per crop on one core.

Two region sets: 50 and 300 person-shaped boxes, seeded, of the sizes tests/synthetic.py gives a 1080p frame (40..90 x
120..250 pixels; bench.py's config[1] has 50 such objects, config[4] 300), clipped to the frame.  (d) is
fm_frame_encode_jpeg of the whole frame, for scale and for the parent-commit comparison of profiles/object_encode.txt.

    python scripts/object_encode_timing.py [--iters 40] [--out profiles/object_encode.txt] [--frame-only]"""
import argparse
import io
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(1, str(ROOT / 'tests'))

import jpeg_cases as jc  # noqa: E402

SIZE = (1920, 1080)
QUALITY = 85
# what one fm_frame_encode_regions enqueues, by construction (csrc/jpegenc.hip launch_all): the DCT, scan, pack, stuff,
# prefix and gather kernels behind one copy of the tables
LAUNCHES_PER_CALL = '6 kernels + 1 table copy'


def med(x):
    return float(np.median(x))


def fmt(v):
    return f'median {med(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}'


def boxes(n):
    from synthetic import SyntheticVideo
    from fastmot_amd.utils.redact import region_rect, clip_rect, PARTS
    gt = SyntheticVideo(SIZE, n_ids=n, n_frames=1, seed=100).gt[0]
    rects = [clip_rect(region_rect(b, PARTS['box'], 0., SIZE), SIZE) for b in gt]
    return np.array([r for r in rects if r is not None], np.int32)


def frame_part(ctx, iters, lines):
    dev = []
    for i in range(iters + 5):
        data = ctx.frame_encode_jpeg(QUALITY)
        if i >= 5:
            dev.append(ctx.jpeg_encode_stream_ms())
    lines.append(f'(d) fm_frame_encode_jpeg, whole frame, quality {QUALITY} -> {len(data) / 1e3:.0f} KB, {iters} calls, kernels (HIP events): {fmt(dev)}')
    return med(dev)


def regions_part(ctx, rects, iters, lines):
    from PIL import Image
    from fastmot_amd.utils import jpeg as J
    n = len(rects)
    stream_ms, calls = [], []
    real = type(ctx)._encode_regions_call

    def counted(self, arr, *a):
        out = real(self, arr, *a)
        stream_ms[-1] += self.jpeg_encode_stream_ms()
        calls[-1] += 1
        return out
    type(ctx)._encode_regions_call = counted
    try:
        for shrink in (1, 2):
            host = []
            del stream_ms[:], calls[:]
            for i in range(iters + 5):
                stream_ms.append(0.), calls.append(0)
                t0 = time.perf_counter()
                files = ctx.frame_encode_regions(rects, QUALITY, shrink=shrink)
                host.append((time.perf_counter() - t0) * 1e3)
            mcus = int(_lib_plan_mcus(rects, shrink))
            lines.append(f'(a) frame_encode_regions, {n} crops, shrink {shrink}: {mcus} MCUs, {sum(map(len, files)) / 1e3:.0f} KB in {n} files, '
                         f'{calls[-1]} library call(s) of {LAUNCHES_PER_CALL} each')
            lines.append(f'(a)   kernels on the encoder stream (HIP events): {fmt(stream_ms[5:])}')
            lines.append(f'(a)   whole call on the host:                     {fmt(host[5:])}')
    finally:
        type(ctx)._encode_regions_call = real
    t_b, t_c = [], []
    for i in range(iters + 3):
        t0 = time.perf_counter()
        frame = ctx.frame_read()
        got = [J.encode_bgr(frame[y0:y1 + 1, x0:x1 + 1], QUALITY, ctx) for x0, y0, x1, y1 in rects]
        t_b.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        frame = ctx.frame_read()
        for x0, y0, x1, y1 in rects:
            buf = io.BytesIO()
            Image.fromarray(frame[y0:y1 + 1, x0:x1 + 1, ::-1]).save(buf, 'JPEG', quality=QUALITY, subsampling=2)
        t_c.append((time.perf_counter() - t0) * 1e3)
    same = got == ctx.frame_encode_regions(rects, QUALITY)
    lines.append(f'(b) frame_read + encode_bgr per crop ({n} uploads, {5 * n} launches, {n} synchronises), {sum(map(len, got)) / 1e3:.0f} KB, '
                 f'files equal (a)\'s: {same}: {fmt(t_b[3:])}')
    lines.append(f'(c) frame_read + Pillow save per crop, one core: {fmt(t_c[3:])}')
    t0 = time.perf_counter()
    for _ in range(5):
        ctx.frame_read()
    lines.append(f'    (frame_read alone: {(time.perf_counter() - t0) / 5 * 1e3:.3f} ms)')


def _lib_plan_mcus(rects, shrink):
    w = (rects[:, 2] - rects[:, 0] + shrink) // shrink
    h = (rects[:, 3] - rects[:, 1] + shrink) // shrink
    return (((w + 15) // 16) * ((h + 15) // 16)).sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'object_encode.txt'))
    ap.add_argument('--frame-only', action='store_true', help='only (d): prints its median, writes no file')
    args = ap.parse_args()
    from fastmot_amd.runtime import get_context
    ctx = get_context()
    frame = np.ascontiguousarray(jc.content('textured', *SIZE)[:, :, ::-1])
    ctx.frame_configure(*SIZE, 0)
    ctx.frame_upload(frame)
    lines = [f'scripts/object_encode_timing.py on {ctx.device_info()["name"]}: 1920x1080 textured frame on the device, quality {QUALITY}, '
             f'{args.iters} rounds after warm-up; times are host perf_counter unless marked HIP events']
    if args.frame_only:
        print(f'frame_encode_jpeg_stream_ms {frame_part(ctx, max(args.iters, 60), lines):.4f}')
        return
    frame_part(ctx, args.iters, lines)
    for n in (50, 300):
        regions_part(ctx, boxes(n), args.iters, lines)
    text = '\n'.join(lines) + '\n'
    print(text, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
