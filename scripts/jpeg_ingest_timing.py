"""JPEG ingest against the Pillow path, for one 1920x1080 4:2:0 quality-90 frame encoded by Pillow from a textured
synthetic image, five measurements in one process:

(a) the image-sequence source as it was: videoio._ImageSequence.read (Pillow decode, convert('RGB'), BGR copy), ms;
(b) Pillow's im.load() alone (the whole of libjpeg-turbo's decode);
(c) fm_jpeg_entropy_decode (marker parsing + Huffman decoding, what stays on the host), and JPEGFrame(data) as a whole;
(d) the upload -- frame_upload_ahead(1, frame) + frame_promote_next() + a device synchronise, page-locked sources -- of
    the JPEGFrame against the BGR frame: host-visible time and HIP-event time of the work on the upload stream (trace
    marks 30 .. 31: the H2D copy, for JPEG the copy and the two kernels; 37 .. 31: the kernels alone);
(e) frames/s of readahead.track_stream over a 200-file sequence of such frames (bench.py's config[1] workload) with
    gpu_decode off and on, alternating, three repetitions each.

(a) - (c) are host timings and need no GPU (--host-only); (d) and (e) need one.

    python scripts/jpeg_ingest_timing.py [--host-only] [--iters 100] [--files 200] [--rounds 3] [--out profiles/jpeg_ingest.txt]"""
import argparse
import ctypes as C
import io
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
import jpeg_cases as jc  # noqa: E402


def med(x):
    return float(np.median(x)) if len(x) else float('nan')


def timed(fn, n):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def intervals(tags, ms, a, b):
    out, t0 = [], None
    for t, m in zip(tags, ms):
        if t == a:
            t0 = m
        elif t == b and t0 is not None:
            out.append(m - t0)
            t0 = None
    return out


def fmt(v):
    return f'median {med(v):.2f} ms, min {min(v):.2f}'


def host_part(args, data, tmp, lines):
    from PIL import Image
    from fastmot_amd import JPEGFrame, _lib
    from fastmot_amd.utils.jpeg import JpegInfo
    from fastmot_amd.videoio import _ImageSequence
    lib = _lib.load()
    path = Path(tmp) / '000001.jpg'
    path.write_bytes(data)
    seq = _ImageSequence(str(Path(tmp) / '%06d.jpg'))

    def a():
        seq.index = 1
        assert seq.read() is not None

    def b():
        with Image.open(io.BytesIO(data)) as im:
            im.load()

    info = JpegInfo()
    assert lib.fm_jpeg_info(data, C.c_size_t(len(data)), C.byref(info)) == 0
    buf = np.empty(info.coef_count + 192, np.int16)
    cp, qp = _lib._ptr(buf), _lib._ptr(buf[info.coef_count:])

    def c():
        assert lib.fm_jpeg_entropy_decode(data, C.c_size_t(len(data)), C.byref(info), cp, qp) == 0

    res = {}
    for _ in range(3):                                   # alternating rounds
        for name, fn in (('a', a), ('b', b), ('c', c), ('frame', lambda: JPEGFrame(data, buffer=buf))):
            fn()
            res.setdefault(name, []).extend(timed(fn, args.iters // 3 + 1))
    lines.append(f'frame: 1920x1080 4:2:0 quality 90, {len(data) / 1e3:.0f} KB; host timings, one thread, {len(res["a"])} calls each in 3 alternating rounds')
    lines.append(f'(a) _ImageSequence.read (Pillow decode + convert + BGR copy): {fmt(res["a"])}')
    lines.append(f'(b) Pillow im.load() alone:                                   {fmt(res["b"])}')
    lines.append(f'(c) fm_jpeg_entropy_decode:                                   {fmt(res["c"])}')
    lines.append(f'    JPEGFrame(data) (fm_jpeg_info + entropy decode + Python): {fmt(res["frame"])}')
    lines.append(f'(c) <= (b): {med(res["c"]) <= med(res["b"])} (medians), {min(res["c"]) <= min(res["b"])} (minima)')
    return {k: med(v) for k, v in res.items()}


def upload_part(ctx, args, data, lines):
    from fastmot_amd import JPEGFrame
    w, h = 1920, 1080
    ctx.frame_configure(w, h, 0)
    bgr = ctx.pinned_frames(2)
    bgr[0] = jc.pillow_bgr(data)
    bgr[1] = bgr[0]
    sources = {'BGR': [bgr[0], bgr[1]], 'JPEG': [JPEGFrame(data, buffer=b) for b in ctx.pinned_jpeg_buffers(2)]}
    res = {k: {'host': [], 'event': [], 'kernels': []} for k in sources}
    for _ in range(3):
        for kind, frames in sources.items():
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
            res[kind]['host'].append(med(host))
            res[kind]['event'].append(med(intervals(tags, ms, 30, 31)))
            if kind == 'JPEG':
                res[kind]['kernels'].append(med(intervals(tags, ms, 37, 31)))
    assert np.array_equal(ctx.frame_read(), bgr[0])
    nbytes = {'BGR': w * h * 3, 'JPEG': sources['JPEG'][0].info.coef_count * 2 + 384}
    for kind, r in res.items():
        lines.append(f'(d) {kind:4s} upload_ahead + promote + synchronise: host-visible {med(r["host"]):.3f} ms; upload-stream events '
                     f'{med(r["event"]):.3f} ms (rounds {", ".join(f"{x:.3f}" for x in r["event"])}); {nbytes[kind] / 1e6:.2f} MB over PCIe')
    k = res['JPEG']['kernels']
    lines.append(f'(d) jpeg_idct_kernel + jpeg_to_bgr_kernel (events 37 .. 31): {med(k) * 1e3:.1f} us (rounds {", ".join(f"{x * 1e3:.1f}" for x in k)})')
    return {kind: {m: med(v) for m, v in r.items() if v} for kind, r in res.items()}


class _Looped:
    """The scripted detections of a clip played forwards and backwards, by step number."""

    def __init__(self, video):
        self.video = video

    def detections(self, step, *a):
        return self.video.detections(bench.ping_pong(step, self.video.n_frames), *a)


def loop_part(ctx, args, tmp, lines):
    from PIL import Image
    from fastmot_amd import Track, VideoIO
    from fastmot_amd.readahead import track_stream
    from synthetic import SyntheticVideo
    cfg = bench.CONFIGS[1]
    size = cfg['size']
    video = SyntheticVideo(size, n_ids=cfg['n_dets'], n_frames=bench.RING, seed=100)
    seq = Path(tmp) / 'seq'
    seq.mkdir()
    total = 0
    for s in range(args.files):
        f = video.frames[bench.ping_pong(s, bench.RING)]
        path = seq / f'{s + 1:06d}.jpg'
        Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(path, 'JPEG', quality=90)
        total += path.stat().st_size
    lines.append(f'(e) readahead.track_stream, {cfg["name"]}: {args.files} files 1920x1080 4:2:0 quality 90 (mean {total / args.files / 1e3:.0f} KB), '
                 f'VideoIO buffer_size 10, next_frame prefetch; {args.rounds} alternating repetitions, each a fresh MOT, the first 20 frames not timed')
    rates = {False: [], True: []}
    for _ in range(args.rounds):
        for gpu_decode in (False, True):
            mot = bench.build_mot(cfg, video)
            mot.detector._video = _Looped(video)
            Track._count = 0
            mot.reset(1 / 30.)
            stream = VideoIO(size, str(seq / '%06d.jpg'), gpu_decode=gpu_decode)
            stream.start_capture()
            try:
                head = _Head(stream, 20)
                track_stream(head, mot)                  # warm-up on the sequence's first frames
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
        lines.append(f'(e) gpu_decode={gpu_decode!s:5s}: median {med(v):.1f} frames/s (repetitions {", ".join(f"{x:.1f}" for x in v)})')
    lines.append(f'(e) on / off: {med(rates[True]) / med(rates[False]):.2f}')
    return {str(k): v for k, v in rates.items()}


class _Head:
    """The first n frames of a stream."""

    def __init__(self, stream, n):
        self.stream, self.left, self.resolution = stream, n, stream.resolution

    def read(self):
        self.left -= 1
        return self.stream.read() if self.left >= 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--files', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--host-only', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    data = jc.encode(jc.content('textured', 1920, 1080), '420', 90)
    lines, out = [], {}
    with tempfile.TemporaryDirectory() as tmp:
        if args.host_only:
            lines.append('# scripts/jpeg_ingest_timing.py --host-only')
            out['host'] = host_part(args, data, tmp, lines)
        else:
            from fastmot_amd import models
            from fastmot_amd.runtime import get_context
            models.allow_random_weights()
            ctx = get_context()
            lines.append(f'# scripts/jpeg_ingest_timing.py: {ctx.device_info()["arch"]}')
            out['host'] = host_part(args, data, tmp, lines)
            out['upload'] = upload_part(ctx, args, data, lines)
            out['track_stream_fps'] = loop_part(ctx, args, tmp, lines)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    print(json.dumps(out))
    if args.out:
        Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
