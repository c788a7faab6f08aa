"""NV12 ingest against BGR ingest, three measurements in one process:

1. the upload path -- frame_upload_ahead(1, frame) + frame_promote_next() + a device synchronise, pinned sources, at
   1920x1080 and 3840x2160: host-visible time per frame (host clock around the three calls) and HIP-event time of the
   work on the upload stream (the library's trace marks 30 .. 31: the H2D copy, for NV12 the copy and the conversion);
2. the conversion kernel alone (trace marks 36 .. 31) against the time its 4.5 bytes per pixel need at the HBM peak;
3. MOT.step frames/s on bench.py's config[1] workload with next_frame, BGR frames and NV12 frames of the same content
   (bgr_to_nv12 of the synthetic video), alternating in rounds.

    python scripts/nv12_ingest_timing.py [--iters 200] [--steps 300] [--rounds 3] [--out profiles/nv12_ingest.txt]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(1, str(ROOT / 'tests'))

import bench  # noqa: E402

HBM_PEAK_GBS = 8000.0        # MI355X: 8 TB/s


def med(x):
    return float(np.median(x)) if len(x) else float('nan')


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


def upload_path(ctx, size, iters, lines):
    w, h = size
    rng = np.random.default_rng(0)
    ctx.frame_configure(w, h, 0)
    bgr = ctx.pinned_frames(2)
    bgr[...] = rng.integers(0, 256, bgr.shape, dtype=np.uint8)
    nv = ctx.pinned_nv12_frames(2)
    for f in nv:
        f.y[...] = rng.integers(0, 256, f.y.shape, dtype=np.uint8)
        f.uv[...] = rng.integers(0, 256, f.uv.shape, dtype=np.uint8)
    sources = {'BGR': [bgr[0], bgr[1]], 'NV12': nv}
    res = {k: {'host': [], 'event': [], 'kernel': []} for k in sources}
    for _ in range(3):                                   # alternating rounds
        for kind, frames in sources.items():
            for i in range(20):                          # warm-up: first launch, staging allocation
                ctx.frame_upload_ahead(1, frames[i & 1])
                ctx.frame_promote_next()
            ctx.synchronize()
            ctx.trace_start(4 * iters + 16)
            host = []
            for i in range(iters):
                t0 = time.perf_counter()
                ctx.frame_upload_ahead(1, frames[i & 1])
                ctx.frame_promote_next()
                ctx.synchronize()
                host.append((time.perf_counter() - t0) * 1e3)
            tags, ms = ctx.trace_read()
            res[kind]['host'].append(med(host))
            res[kind]['event'].append(med(intervals(tags, ms, 30, 31)))
            if kind == 'NV12':
                res[kind]['kernel'].append(med(intervals(tags, ms, 36, 31)))
    px = w * h
    for kind in sources:
        r = res[kind]
        nbytes = px * (3 if kind == 'BGR' else 1.5)
        lines.append(f'{w}x{h} {kind:4s} upload_ahead + promote + synchronise: host-visible {med(r["host"]):.3f} ms '
                     f'(rounds {", ".join(f"{x:.3f}" for x in r["host"])}); upload-stream events {med(r["event"]):.3f} ms '
                     f'(rounds {", ".join(f"{x:.3f}" for x in r["event"])}); {nbytes / 1e6:.2f} MB over PCIe '
                     f'= {nbytes / 1e6 / med(r["event"]):.1f} GB/s of the event time')
    k = med(res['NV12']['kernel'])
    floor = 4.5 * px / (HBM_PEAK_GBS * 1e9) * 1e3
    lines.append(f'{w}x{h} nv12_to_bgr_kernel alone (events): {k * 1e3:.1f} us (rounds '
                 f'{", ".join(f"{x * 1e3:.1f}" for x in res["NV12"]["kernel"])}); 4.5 B/px = {4.5 * px / 1e6:.2f} MB -> '
                 f'{4.5 * px / 1e9 / (k * 1e-3):.0f} GB/s, {floor * 1e3:.1f} us at the {HBM_PEAK_GBS / 1e3:.0f} TB/s HBM peak '
                 f'({100 * floor / k:.0f} % of it; event pairs around one short kernel also time the launch gap)')
    return {kind: {m: med(v) for m, v in r.items() if v} for kind, r in res.items()}


def mot_rate(ctx, args, lines):
    from fastmot_amd import Track
    from fastmot_amd.utils.nv12 import bgr_to_nv12
    from synthetic import SyntheticVideo
    cfg = bench.CONFIGS[1]
    size = cfg['size']
    video = SyntheticVideo(size, n_ids=cfg['n_dets'], n_frames=bench.RING, seed=100)
    ctx.frame_configure(size[0], size[1], bench.RING)
    host = ctx.pinned_frames(bench.RING)
    nv = ctx.pinned_nv12_frames(bench.RING)
    for i, fr in enumerate(video.frames):
        host[i] = fr
        y, uv = bgr_to_nv12(fr)
        nv[i].y[...] = y
        nv[i].uv[...] = uv
    sources = {'BGR': [host[i] for i in range(bench.RING)], 'NV12': nv}
    lines.append(f'MOT.step, {cfg["name"]}: {cfg["desc"]}; pinned host frames, next_frame prefetch, {args.steps} timed steps '
                 f'after {args.warmup}, {args.rounds} alternating rounds')

    def run(mot, frames, n, start):
        for s in range(start, start + n):
            i = bench.ping_pong(s, bench.RING)
            mot.detector._frame_idx = i
            mot.step(frames[i], next_frame=frames[bench.ping_pong(s + 1, bench.RING)])

    rates = {k: [] for k in sources}
    for r in range(args.rounds):
        for kind, frames in sources.items():
            mot = bench.build_mot(cfg, video)
            Track._count = 0
            mot.reset(1 / 30.)
            run(mot, frames, args.warmup, 0)
            ctx.synchronize()
            t0 = time.perf_counter()
            run(mot, frames, args.steps, args.warmup)
            ctx.synchronize()
            rates[kind].append(args.steps / (time.perf_counter() - t0))
            mot.tracker._clear_tracks()
            del mot
    for kind, v in rates.items():
        lines.append(f'MOT.step {kind:4s}: median {med(v):.1f} frames/s (rounds {", ".join(f"{x:.1f}" for x in v)})')
    lines.append(f'MOT.step NV12 / BGR: {med(rates["NV12"]) / med(rates["BGR"]):.3f}')
    return rates


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--warmup', type=int, default=60)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from fastmot_amd import models
    from fastmot_amd.runtime import get_context
    models.allow_random_weights()
    ctx = get_context()
    lines = [f'# scripts/nv12_ingest_timing.py: {ctx.device_info()["arch"]}; medians of {args.iters} frames per round, 3 rounds']
    out = {'upload': {}}
    for size in ((1920, 1080), (3840, 2160)):
        out['upload'][f'{size[0]}x{size[1]}'] = upload_path(ctx, size, args.iters, lines)
    out['mot_step_fps'] = mot_rate(ctx, args, lines)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    print(json.dumps(out))
    if args.out:
        Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
