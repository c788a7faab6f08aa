"""Bayer ingest against the paths beside it, on one 1920x1080 frame in one process, three alternating rounds of `--iters`
with medians: frame_upload_ahead(1, frame) + frame_promote_next() + a device synchronise from page-locked memory for
BGR, NV12 (the 1.5 bytes-per-pixel yardstick), PackedFrame('rgb') (the kernel that writes the same output from three
times the input), 8-bit Bayer with both methods and 12-bit Bayer -- host-visible time (host clock around the three
calls), HIP-event time of the work on the upload stream (the library's trace marks 30 .. 31) and the conversion kernel
alone (marks 36 / 48 / 49 .. 31) --, and what `bayer_to_bgr` costs the host per frame, which is what the capture thread
is spared.

    python scripts/bayer_ingest_timing.py [--iters 100] [--rounds 3] [--out profiles/bayer_ingest.txt]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SIZE = (1920, 1080)
BYTES_PER_PIXEL = {'BGR': 3, 'NV12': 1.5, 'RGB': 3, 'Bayer8 mhc': 1, 'Bayer8 bilinear': 1, 'Bayer12 mhc': 2}
KERNEL_MARK = {'NV12': 36, 'RGB': 48, 'Bayer8 mhc': 49, 'Bayer8 bilinear': 49, 'Bayer12 mhc': 49}


def med(x):
    return float(np.median(x)) if len(x) else float('nan')


def rounds(x, scale=1., fmt='.3f'):
    return ', '.join(format(v * scale, fmt) for v in x)


def intervals(tags, ms, a, b):
    """Durations from each mark `a` to the next mark `b`."""
    out, t0 = [], None
    for t, m in zip(tags, ms):
        if t == a:
            t0 = m
        elif t == b and t0 is not None:
            out.append(m - t0)
            t0 = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from fastmot_amd.runtime import get_context
    from fastmot_amd.utils.bayer import bayer_to_bgr
    ctx = get_context()
    w, h = SIZE
    rng = np.random.default_rng(0)
    ctx.frame_configure(w, h, 0)
    bgr = ctx.pinned_frames(2)
    bgr[...] = rng.integers(0, 256, bgr.shape, dtype=np.uint8)
    nv = ctx.pinned_nv12_frames(2)
    for f in nv:
        f.y[...] = rng.integers(0, 256, f.y.shape, dtype=np.uint8)
        f.uv[...] = rng.integers(0, 256, f.uv.shape, dtype=np.uint8)
    sources = {'BGR': [bgr[0], bgr[1]], 'NV12': nv, 'RGB': ctx.pinned_packed_frames(2, 'rgb')}
    for f in sources['RGB']:
        f.rows[...] = rng.integers(0, 256, f.rows.shape, dtype=np.uint8)
    for kind, depth, method in (('Bayer8 mhc', 8, 'mhc'), ('Bayer8 bilinear', 8, 'bilinear'), ('Bayer12 mhc', 12, 'mhc')):
        sources[kind] = ctx.pinned_bayer_frames(2, 'rggb', depth, method=method)
        for f in sources[kind]:
            f.rows[...] = rng.integers(0, 1 << depth, f.rows.shape).astype(f.rows.dtype)
    res = {k: {'host': [], 'event': [], 'kernel': []} for k in sources}
    for _ in range(args.rounds):
        for kind, frames in sources.items():
            for i in range(20):                                # warm-up: first launch, staging allocation
                ctx.frame_upload_ahead(1, frames[i & 1])
                ctx.frame_promote_next()
            ctx.synchronize()
            ctx.trace_start(4 * args.iters + 16)
            host = []
            for i in range(args.iters):
                t0 = time.perf_counter()
                ctx.frame_upload_ahead(1, frames[i & 1])
                ctx.frame_promote_next()
                ctx.synchronize()
                host.append((time.perf_counter() - t0) * 1e3)
            tags, ms = ctx.trace_read()
            res[kind]['host'].append(med(host))
            res[kind]['event'].append(med(intervals(tags, ms, 30, 31)))
            if kind in KERNEL_MARK:
                res[kind]['kernel'].append(med(intervals(tags, ms, KERNEL_MARK[kind], 31)))
    for kind in ('Bayer8 mhc', 'Bayer8 bilinear', 'Bayer12 mhc'):       # what was timed is the conversion the tests pin
        f = sources[kind][0]
        ctx.frame_upload_ahead(1, f)
        ctx.frame_promote_next()
        assert np.array_equal(ctx.frame_read(), f.to_bgr())
    lines = [f'# scripts/bayer_ingest_timing.py: {ctx.device_info()["arch"]}; {w}x{h}, page-locked sources, medians of {args.iters} per round, '
             f'{args.rounds} alternating rounds']
    for kind, r in res.items():
        nbytes = w * h * BYTES_PER_PIXEL[kind]
        lines.append(f'{kind:15s} upload_ahead + promote + synchronise: host-visible {med(r["host"]):.3f} ms (rounds {rounds(r["host"])}); '
                     f'upload-stream events {med(r["event"]):.3f} ms (rounds {rounds(r["event"])}); {nbytes / 1e6:.2f} MB over PCIe')
    for kind in KERNEL_MARK:
        k = res[kind]['kernel']
        moved = (BYTES_PER_PIXEL[kind] + 3) * w * h
        lines.append(f'{kind:15s} conversion kernel alone (events {KERNEL_MARK[kind]} .. 31): {med(k) * 1e3:.1f} us (rounds {rounds(k, 1e3, ".1f")}); '
                     f'{BYTES_PER_PIXEL[kind] + 3:g} B/px = {moved / 1e6:.2f} MB -> {moved / 1e9 / (med(k) * 1e-3):.0f} GB/s '
                     '(event pairs around one short kernel also time the launch gap)')
    # the host work the Bayer calls replace
    raw = np.array(sources['Bayer8 mhc'][0].rows)
    host = {'mhc': [], 'bilinear': []}
    for _ in range(3):
        for method in host:
            t0 = time.perf_counter()
            bayer_to_bgr(raw, SIZE, 'rggb', method=method)
            host[method].append((time.perf_counter() - t0) * 1e3)
    lines.append(f'host, per frame: numpy `bayer_to_bgr` of an 8-bit mosaic, mhc {med(host["mhc"]):.0f} ms, bilinear {med(host["bilinear"]):.0f} ms '
                 '(one thread; then 3 bytes per pixel are uploaded)')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    print(json.dumps({kind: {m: med(v) for m, v in r.items() if v} for kind, r in res.items()}))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
