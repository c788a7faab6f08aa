"""Planar I420 in and out against the paths beside it, on one 1920x1080 frame in one process, three alternating rounds
of `--iters` with medians:

(a) the upload path -- frame_upload_ahead(1, frame) + frame_promote_next() + a device synchronise from page-locked
    memory, for BGR, NV12 and I420: host-visible time (host clock around the three calls) and HIP-event time of the work
    on the upload stream (the library's trace marks 30 .. 31), and the conversion kernel alone (marks 36 / 39 .. 31);
(b) the export -- MOT.export_frame_i420's work, ctx.frame_export_i420(), against ctx.frame_read() + bgr_to_planar420;
(c) readahead.track_stream over a `--files`-frame .y4m on bench.py's config[1] workload with gpu_decode on and off.

    python scripts/y4m_timing.py [--iters 100] [--files 100] [--rounds 3] [--out profiles/y4m_io.txt]"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(1, str(ROOT / 'tests'))

import bench  # noqa: E402

SIZE = (1920, 1080)


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


def upload_part(ctx, args, lines):
    w, h = SIZE
    rng = np.random.default_rng(0)
    ctx.frame_configure(w, h, 0)
    bgr = ctx.pinned_frames(2)
    bgr[...] = rng.integers(0, 256, bgr.shape, dtype=np.uint8)
    nv = ctx.pinned_nv12_frames(2)
    pl = ctx.pinned_planar_frames(2, '420')
    for f, g in zip(nv, pl):
        f.y[...] = rng.integers(0, 256, f.y.shape, dtype=np.uint8)
        f.uv[...] = rng.integers(0, 256, f.uv.shape, dtype=np.uint8)
        g.y[...] = f.y                                         # the same picture, de-interleaved
        g.u[...], g.v[...] = f.uv[:, 0::2], f.uv[:, 1::2]
    sources = {'BGR': [bgr[0], bgr[1]], 'NV12': nv, 'I420': pl}
    kernel_mark = {'NV12': 36, 'I420': 39}
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
            if kind in kernel_mark:
                res[kind]['kernel'].append(med(intervals(tags, ms, kernel_mark[kind], 31)))
    from fastmot_amd.utils.nv12 import nv12_to_bgr
    ctx.frame_upload_ahead(1, pl[0])
    ctx.frame_promote_next()
    assert np.array_equal(ctx.frame_read(), nv12_to_bgr(nv[0].y, nv[0].uv))         # both kernels make the same frame of it
    for kind, r in res.items():
        nbytes = w * h * (3 if kind == 'BGR' else 1.5)
        lines.append(f'(a) {kind:4s} upload_ahead + promote + synchronise: host-visible {med(r["host"]):.3f} ms (rounds {rounds(r["host"])}); '
                     f'upload-stream events {med(r["event"]):.3f} ms (rounds {rounds(r["event"])}); {nbytes / 1e6:.2f} MB over PCIe')
    for kind, name in (('NV12', 'nv12_to_bgr_kernel'), ('I420', 'planar_to_bgr_kernel<420>')):
        k = res[kind]['kernel']
        lines.append(f'(a) {name} alone (events {kernel_mark[kind]} .. 31): {med(k) * 1e3:.1f} us (rounds {rounds(k, 1e3, ".1f")}); '
                     f'4.5 B/px = {4.5 * w * h / 1e6:.2f} MB -> {4.5 * w * h / 1e9 / (med(k) * 1e-3):.0f} GB/s '
                     '(event pairs around one short kernel also time the launch gap)')
    nvr, i4 = res['NV12'], res['I420']
    for what in ('host', 'event'):
        lo, hi = min(nvr[what]), max(nvr[what])
        m = med(i4[what])
        inside = 'inside' if lo <= m <= hi else f'{(m - hi if m > hi else m - lo) * 1e3:+.1f} us outside'
        lines.append(f'(a) I420 {what} median {m:.3f} ms against the NV12 rounds {lo:.3f} .. {hi:.3f} ms: {inside} their spread')
    return {kind: {m: med(v) for m, v in r.items() if v} for kind, r in res.items()}


def export_part(ctx, args, lines):
    from fastmot_amd.utils.yuv import bgr_to_planar420
    w, h = SIZE
    rng = np.random.default_rng(1)
    ctx.frame_configure(w, h, 0)
    frame = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    ctx.frame_upload(frame)
    want = np.concatenate([p.reshape(-1) for p in bgr_to_planar420(frame)])
    assert np.array_equal(ctx.frame_export_i420(), want)
    res = {'gpu': [], 'host': []}
    host_iters = max(3, args.iters // 10)                      # (the numpy conversion takes tens of milliseconds)
    for _ in range(args.rounds):
        for _ in range(10):
            ctx.frame_export_i420()
        t = []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            ctx.frame_export_i420()
            t.append((time.perf_counter() - t0) * 1e3)
        res['gpu'].append(med(t))
        t = []
        for _ in range(host_iters):
            t0 = time.perf_counter()
            bgr_to_planar420(ctx.frame_read())
            t.append((time.perf_counter() - t0) * 1e3)
        res['host'].append(med(t))
    lines.append(f'(b) ctx.frame_export_i420() (kernel, 3.11 MB D2H, copy out): {med(res["gpu"]):.3f} ms (rounds {rounds(res["gpu"])})')
    lines.append(f'(b) ctx.frame_read() + bgr_to_planar420 (6.22 MB D2H, numpy; {host_iters} per round): {med(res["host"]):.2f} ms '
                 f'(rounds {rounds(res["host"], 1., ".2f")})')
    return {k: med(v) for k, v in res.items()}


class _Looped:
    """The scripted detections of a clip played forwards and backwards, by step number."""

    def __init__(self, video):
        self.video = video

    def detections(self, step, *a):
        return self.video.detections(bench.ping_pong(step, self.video.n_frames), *a)


class _Head:
    """The first n frames of a stream."""

    def __init__(self, stream, n):
        self.stream, self.left, self.resolution = stream, n, stream.resolution

    def read(self):
        self.left -= 1
        return self.stream.read() if self.left >= 0 else None


def loop_part(ctx, args, tmp, lines):
    from fastmot_amd import Track, VideoIO
    from fastmot_amd.readahead import track_stream
    from fastmot_amd.utils.yuv import bgr_to_planar420, fps_ratio, y4m_header
    from synthetic import SyntheticVideo
    cfg = bench.CONFIGS[1]
    size = cfg['size']
    video = SyntheticVideo(size, n_ids=cfg['n_dets'], n_frames=bench.RING, seed=100)
    path = Path(tmp) / 'clip.y4m'
    planes = [b''.join(p.tobytes() for p in bgr_to_planar420(f)) for f in video.frames]
    with open(path, 'wb') as f:
        f.write(y4m_header(size[0], size[1], fps_ratio(30)))
        for s in range(args.files + 20):
            f.write(b'FRAME\n' + planes[bench.ping_pong(s, bench.RING)])
    lines.append(f'(c) readahead.track_stream, {cfg["name"]}: a .y4m of {args.files + 20} frames {size[0]}x{size[1]} 4:2:0, VideoIO buffer_size 10, '
                 f'next_frame prefetch; {args.rounds} alternating repetitions, each a fresh MOT, the first 20 frames not timed')
    rates = {False: [], True: []}
    for _ in range(args.rounds):
        for gpu_decode in (False, True):
            mot = bench.build_mot(cfg, video)
            mot.detector._video = _Looped(video)
            Track._count = 0
            mot.reset(1 / 30.)
            stream = VideoIO(size, str(path), gpu_decode=gpu_decode)
            stream.start_capture()
            try:
                track_stream(_Head(stream, 20), mot)           # warm-up on the clip's first frames
                ctx.synchronize()
                t0 = time.perf_counter()
                n = track_stream(stream, mot)
                ctx.synchronize()
                rates[gpu_decode].append(n / (time.perf_counter() - t0))
            finally:
                stream.release()
            mot.tracker._clear_tracks()
            del mot
    for gpu_decode, v in rates.items():
        lines.append(f'(c) gpu_decode={gpu_decode!s:5s}: median {med(v):.1f} frames/s (repetitions {rounds(v, 1., ".1f")})')
    lines.append(f'(c) on / off: {med(rates[True]) / med(rates[False]):.2f}')
    return {str(k): v for k, v in rates.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--files', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from fastmot_amd import models
    from fastmot_amd.runtime import get_context
    models.allow_random_weights()
    ctx = get_context()
    lines = [f'# scripts/y4m_timing.py: {ctx.device_info()["arch"]}; {SIZE[0]}x{SIZE[1]}, medians of {args.iters} per round, {args.rounds} alternating rounds']
    out = {'upload': upload_part(ctx, args, lines), 'export': export_part(ctx, args, lines)}
    with tempfile.TemporaryDirectory() as tmp:
        out['track_stream_fps'] = loop_part(ctx, args, tmp, lines)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    print(json.dumps(out))
    if args.out:
        Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
