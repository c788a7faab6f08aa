"""10-bit YCbCr ingest against the 8-bit paths beside it, on one 1920x1080 frame in one process, alternating rounds of
`--iters` with medians:

(a) the upload path -- frame_upload_ahead(1, frame) + frame_promote_next() + a device synchronise from page-locked
    memory, for P010 (semi-planar), planar 420p10, NV12, I420 and BGR: host-visible time (host clock around the three
    calls) and HIP-event time of the work on the upload stream (the library's trace marks 30 .. 31), and the conversion
    kernel alone (marks 58 / 39 / 36 .. 31): deep_to_bgr_kernel beside planar_to_bgr_kernel and nv12_to_bgr_kernel;
(b) the numpy conversion a host thread would do instead, utils.deep.deep_to_bgr of one 420p10 frame;
(c) readahead.track_stream over a `--files`-frame C420p10 .y4m on bench.py's config[1] workload with deep_color, with
    gpu_decode on and off.

    python scripts/deep_timing.py [--iters 100] [--files 60] [--rounds 3] [--out profiles/deep_ingest.txt]"""
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
from y4m_timing import _Head, _Looped, intervals, med, rounds  # noqa: E402

SIZE = (1920, 1080)
BYTES_PER_PIXEL = {'P010': 3., '420p10': 3., 'NV12': 1.5, 'I420': 1.5, 'BGR': 3.}


def upload_part(ctx, args, lines):
    w, h = SIZE
    rng = np.random.default_rng(0)
    ctx.frame_configure(w, h, 0)
    bgr = ctx.pinned_frames(2)
    bgr[...] = rng.integers(0, 256, bgr.shape, dtype=np.uint8)
    nv = ctx.pinned_nv12_frames(2)
    pl = ctx.pinned_planar_frames(2, '420')
    p010 = ctx.pinned_deep_frames(2, '420', 10, 'bt709', semiplanar=True)
    p10 = ctx.pinned_deep_frames(2, '420', 10, 'bt709')
    for f, g, s, d in zip(nv, pl, p010, p10):
        f.y[...] = rng.integers(0, 256, f.y.shape, dtype=np.uint8)
        f.uv[...] = rng.integers(0, 256, f.uv.shape, dtype=np.uint8)
        g.y[...] = f.y
        g.u[...], g.v[...] = f.uv[:, 0::2], f.uv[:, 1::2]
        d.y[...] = rng.integers(0, 1024, d.y.shape, dtype=np.uint16)
        d.u[...] = rng.integers(0, 1024, d.u.shape, dtype=np.uint16)
        d.v[...] = rng.integers(0, 1024, d.v.shape, dtype=np.uint16)
        s.y[...] = d.y << 6                                    # the same picture as a decoder surface
        s.uv[:, 0::2], s.uv[:, 1::2] = d.u << 6, d.v << 6
    sources = {'P010': p010, '420p10': p10, 'NV12': nv, 'I420': pl, 'BGR': [bgr[0], bgr[1]]}
    kernel_mark = {'P010': 58, '420p10': 58, 'NV12': 36, 'I420': 39}
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
    for frames in (p010, p10):                                 # both layouts make the frame the numpy statement makes
        ctx.frame_upload_ahead(1, frames[0])
        ctx.frame_promote_next()
        assert np.array_equal(ctx.frame_read(), p10[0].to_bgr())
    for kind, r in res.items():
        lines.append(f'(a) {kind:6s} upload_ahead + promote + synchronise: host-visible {med(r["host"]):.3f} ms (rounds {rounds(r["host"])}); '
                     f'upload-stream events {med(r["event"]):.3f} ms (rounds {rounds(r["event"])}); '
                     f'{w * h * BYTES_PER_PIXEL[kind] / 1e6:.2f} MB over PCIe')
    names = {'P010': 'deep_to_bgr_kernel<semi-planar, 420>', '420p10': 'deep_to_bgr_kernel<planar, 420>',
             'I420': 'planar_to_bgr_kernel<420>', 'NV12': 'nv12_to_bgr_kernel'}
    for kind, name in names.items():
        k = res[kind]['kernel']
        moved = (BYTES_PER_PIXEL[kind] + 3) * w * h
        lines.append(f'(a) {name} alone (events {kernel_mark[kind]} .. 31): {med(k) * 1e3:.1f} us (rounds {rounds(k, 1e3, ".1f")}); '
                     f'{BYTES_PER_PIXEL[kind] + 3:.1f} B/px = {moved / 1e6:.2f} MB -> {moved / 1e9 / (med(k) * 1e-3):.0f} GB/s '
                     '(event pairs around one short kernel also time the launch gap)')
    return {kind: {m: med(v) for m, v in r.items() if v} for kind, r in res.items()}, p10[0]


def host_part(args, frame, lines):
    from fastmot_amd.utils.deep import deep_to_bgr
    n = max(3, args.iters // 20)                               # (the numpy conversion takes a large fraction of a second)
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        deep_to_bgr(frame.y, frame.u, frame.v, '420', 10, 'bt709')
        t.append((time.perf_counter() - t0) * 1e3)
    lines.append(f'(b) utils.deep.deep_to_bgr of one 420p10 frame on a host thread (numpy, int64): median {med(t):.1f} ms of {n} '
                 f'({", ".join(format(v, ".1f") for v in t)})')
    return med(t)


def loop_part(ctx, args, tmp, lines):
    from fastmot_amd import Track, VideoIO
    from fastmot_amd.readahead import track_stream
    from fastmot_amd.utils.yuv import bgr_to_planar420
    from synthetic import SyntheticVideo
    cfg = bench.CONFIGS[1]
    size = cfg['size']
    video = SyntheticVideo(size, n_ids=cfg['n_dets'], n_frames=bench.RING, seed=100)
    path = Path(tmp) / 'clip.y4m'
    # the clip at 10 bits: its 8-bit planes shifted left by two
    planes = [b''.join((p.astype('<u2') << 2).tobytes() for p in bgr_to_planar420(f)) for f in video.frames]
    with open(path, 'wb') as f:
        f.write(f'YUV4MPEG2 W{size[0]} H{size[1]} F30:1 Ip A1:1 C420p10 XCOLORRANGE=LIMITED\n'.encode())
        for s in range(args.files + 20):
            f.write(b'FRAME\n' + planes[bench.ping_pong(s, bench.RING)])
    lines.append(f'(c) readahead.track_stream, {cfg["name"]}: a C420p10 .y4m of {args.files + 20} frames {size[0]}x{size[1]}, deep_color, '
                 f'VideoIO buffer_size 10, next_frame prefetch; {args.rounds} alternating repetitions, each a fresh MOT, the first 20 frames not timed')
    rates = {False: [], True: []}
    for _ in range(args.rounds):
        for gpu_decode in (False, True):
            mot = bench.build_mot(cfg, video)
            mot.detector._video = _Looped(video)
            Track._count = 0
            mot.reset(1 / 30.)
            stream = VideoIO(size, str(path), gpu_decode=gpu_decode, deep_color=True)
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
    ap.add_argument('--files', type=int, default=60)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from fastmot_amd import models
    from fastmot_amd.runtime import get_context
    models.allow_random_weights()
    ctx = get_context()
    lines = [f'# scripts/deep_timing.py: {ctx.device_info()["arch"]}; {SIZE[0]}x{SIZE[1]}, medians of {args.iters} per round, {args.rounds} alternating rounds']
    upload, frame = upload_part(ctx, args, lines)
    out = {'upload': upload, 'host_deep_to_bgr_ms': host_part(args, frame, lines)}
    with tempfile.TemporaryDirectory() as tmp:
        out['track_stream_fps'] = loop_part(ctx, args, tmp, lines)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    print(json.dumps(out))
    if args.out:
        Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
