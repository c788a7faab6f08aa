"""Capture-resolution ingest (SourceFrame, VideoIO gpu_resize) against the host resize, for 1920x1080 sources and a
1280x720 tracker -- the reference's default configuration --, four measurements in one process:

(a) host time per frame of VideoIO.read() over a .npy stack of 1080p frames with gpu_resize off (videoio.resize_bgr on
    the calling thread: the path as it was) and on (the frame is wrapped), and resize_bgr alone;
(b) the upload -- frame_upload_ahead(1, frame) + frame_promote_next() + a device synchronise, page-locked sources -- of
    the 1080p SourceFrame into a 1280x720 context, against the plain 720p BGR upload and the plain 1080p BGR upload:
    host-visible time and HIP-event time of the work on the upload stream (trace marks 30 .. 31);
(c) resize_bgr_kernel alone (trace marks 38 .. 31) against the time its traffic needs at the HBM peak;
(d) frames/s of readahead.track_stream over a sequence of 1080p JPEG files with `size` 1280x720 (bench.py's config[1]
    networks) with gpu_resize + gpu_decode, gpu_decode only, and neither, alternating.

(a) needs no GPU (--host-only).

    python scripts/source_resize_timing.py [--host-only] [--iters 100] [--files 200] [--rounds 3] [--out profiles/source_resize.txt]"""
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
from jpeg_ingest_timing import _Head, fmt, intervals, med, timed  # noqa: E402

SRC, SIZE = (1920, 1080), (1280, 720)
HBM_PEAK = 8e12           # bytes/s, MI355X


def host_part(args, video, tmp, lines):
    from fastmot_amd import SourceFrame, VideoIO
    from fastmot_amd.videoio import resize_bgr
    n = min(len(video.frames), 16)
    path = Path(tmp) / 'stack.npy'
    np.save(path, np.stack(video.frames[:n]))
    res = {}
    for _ in range(3):                                   # alternating rounds
        for on in (False, True):
            stream = VideoIO(SIZE, str(path), buffer_size=n, gpu_resize=on)
            stream.start_capture()
            while len(stream.frame_queue) < n and not stream.exit_event.is_set():     # the capture thread has finished:
                time.sleep(0.01)                                                      # read() only pops and resizes
            try:
                out = []
                for _i in range(n):
                    t0 = time.perf_counter()
                    f = stream.read()
                    out.append((time.perf_counter() - t0) * 1e3)
                    assert isinstance(f, SourceFrame) == on and f.shape == ((SRC if on else SIZE)[1], (SRC if on else SIZE)[0], 3)
                res.setdefault(on, []).extend(out)
            finally:
                stream.release()
        res.setdefault('resize', []).extend(timed(lambda: resize_bgr(video.frames[0], SIZE), max(args.iters // 10, 3)))
    lines.append(f'(a) VideoIO.read(), {SRC[0]}x{SRC[1]} -> {SIZE[0]}x{SIZE[1]}, frames already in the queue; host, one thread, '
                 f'{len(res[False])} calls each in 3 alternating rounds')
    lines.append(f'(a) gpu_resize off (resize_bgr on the calling thread): {fmt(res[False])}')
    lines.append(f'(a) gpu_resize on  (SourceFrame wrapped):              median {med(res[True]) * 1e3:.1f} us, min {min(res[True]) * 1e3:.1f}')
    lines.append(f'(a) resize_bgr alone:                                  {fmt(res["resize"])}')
    return {str(k): med(v) for k, v in res.items()}


def upload_part(ctx, args, video, lines):
    from fastmot_amd import SourceFrame
    from fastmot_amd.videoio import resize_bgr
    res = {}
    cases = (('BGR 720p', SIZE, SIZE), ('BGR 1080p', SRC, SRC), ('SourceFrame 1080p -> 720p', SRC, SIZE))
    for _ in range(3):
        for name, src, dst in cases:
            ctx.frame_configure(dst[0], dst[1], 0)
            buf = ctx.pinned_source_frames(2, src)
            buf[0] = video.frames[0] if src == SRC else resize_bgr(video.frames[0], src)
            buf[1] = buf[0]
            frames = [SourceFrame(b) for b in buf] if src != dst else [buf[0], buf[1]]
            for i in range(20):                          # warm-up: first launch, staging allocation
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
            r = res.setdefault(name, {'host': [], 'event': [], 'kernel': []})
            r['host'].append(med(host))
            r['event'].append(med(intervals(tags, ms, 30, 31)))
            if src != dst:
                r['kernel'].append(med(intervals(tags, ms, 38, 31)))
                r['kernel_min'] = min(r.get('kernel_min', 1e9), min(intervals(tags, ms, 38, 31)))
                assert np.array_equal(ctx.frame_read(), resize_bgr(video.frames[0], dst))
    for name, src, dst in cases:
        r = res[name]
        lines.append(f'(b) {name:26s} upload_ahead + promote + synchronise: host-visible {med(r["host"]):.3f} ms; upload-stream events '
                     f'{med(r["event"]):.3f} ms (rounds {", ".join(f"{x:.3f}" for x in r["event"])}); {src[0] * src[1] * 3 / 1e6:.2f} MB over PCIe')
    r = res[cases[2][0]]
    traffic = (SRC[0] * SRC[1] + SIZE[0] * SIZE[1]) * 3
    k = med(r['kernel'])
    lines.append(f'(c) resize_bgr_kernel (events 38 .. 31): median {k * 1e3:.1f} us (rounds {", ".join(f"{x * 1e3:.1f}" for x in r["kernel"])}), '
                 f'min {r["kernel_min"] * 1e3:.1f} us; {traffic / 1e6:.2f} MB of traffic = {traffic / HBM_PEAK * 1e6:.1f} us at the 8 TB/s HBM peak '
                 f'({traffic / (k * 1e-3) / 1e12:.2f} TB/s).  One short launch between two events: the interval holds the launch latency and '
                 f'the event overhead of a few us, so the kernel itself is faster than this')
    return {n: {m: (med(v) if isinstance(v, list) else v) for m, v in r.items()} for n, r in res.items()}


class _ScaledLooped:
    """The scripted detections of a capture-resolution clip played forwards and backwards, in the tracker's coordinates."""

    def __init__(self, video, ratio):
        self.video, self.ratio = video, ratio

    def detections(self, step, *a):
        dets = self.video.detections(bench.ping_pong(step, self.video.n_frames), *a)
        dets.tlbr = np.rint(dets.tlbr / self.ratio)
        return dets


def loop_part(ctx, args, video, tmp, lines):
    from PIL import Image
    from fastmot_amd import Track, VideoIO
    from fastmot_amd.readahead import track_stream
    cfg = dict(bench.CONFIGS[1], size=SIZE)
    seq = Path(tmp) / 'seq'
    seq.mkdir()
    for s in range(args.files):
        f = video.frames[bench.ping_pong(s, bench.RING)]
        Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(seq / f'{s + 1:06d}.jpg', 'JPEG', quality=90)
    lines.append(f'(d) readahead.track_stream, {cfg["name"]} networks at size {SIZE[0]}x{SIZE[1]}: {args.files} files {SRC[0]}x{SRC[1]} 4:2:0 quality 90, '
                 f'VideoIO buffer_size 10, next_frame prefetch; {args.rounds} alternating repetitions, each a fresh MOT, the first 20 frames not timed')
    settings = (('gpu_resize + gpu_decode', True, True), ('gpu_decode only', False, True), ('neither', False, False))
    rates = {s[0]: [] for s in settings}
    from types import SimpleNamespace
    from fastmot_amd.videoio import resize_bgr
    first = SimpleNamespace(frames=[resize_bgr(video.frames[0], SIZE)])      # (build_mot scripts the head biases on it)
    for _ in range(args.rounds):
        for name, gpu_resize, gpu_decode in settings:
            mot = bench.build_mot(cfg, first)
            mot.detector._video = _ScaledLooped(video, SRC[0] / SIZE[0])
            Track._count = 0
            mot.reset(1 / 30.)
            stream = VideoIO(SIZE, str(seq / '%06d.jpg'), gpu_decode=gpu_decode, gpu_resize=gpu_resize)
            stream.start_capture()
            try:
                track_stream(_Head(stream, 20), mot)     # warm-up on the sequence's first frames
                ctx.synchronize()
                t0 = time.perf_counter()
                n = track_stream(stream, mot)
                ctx.synchronize()
                rates[name].append(n / (time.perf_counter() - t0))
            finally:
                stream.release()
            mot.tracker._clear_tracks()
            del mot
    for name, v in rates.items():
        lines.append(f'(d) {name:24s}: median {med(v):.1f} frames/s (repetitions {", ".join(f"{x:.1f}" for x in v)})')
    return rates


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--files', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--host-only', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from synthetic import SyntheticVideo
    video = SyntheticVideo(SRC, n_ids=bench.N_DETS, n_frames=bench.RING, seed=100)
    lines, out = [], {}
    with tempfile.TemporaryDirectory() as tmp:
        if args.host_only:
            lines.append('# scripts/source_resize_timing.py --host-only')
            out['host'] = host_part(args, video, tmp, lines)
        else:
            from fastmot_amd import models
            from fastmot_amd.runtime import get_context
            models.allow_random_weights()
            ctx = get_context()
            lines.append(f'# scripts/source_resize_timing.py: {ctx.device_info()["arch"]}')
            out['host'] = host_part(args, video, tmp, lines)
            out['upload'] = upload_part(ctx, args, video, lines)
            out['track_stream_fps'] = loop_part(ctx, args, video, tmp, lines)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    print(json.dumps(out))
    if args.out:
        Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
