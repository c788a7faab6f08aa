"""JPEG output on the GPU against the Pillow writer, for 1920x1080 frames at quality 75, four measurements in one process:

(a) fm_frame_encode_jpeg on a 'textured' frame (tests/jpeg_cases.content) that lies on the device: HIP-event time of the
    five kernels on the encoder's stream, and the host time of the whole call (kernels, wait, segment gathering, bytes);
(b) VideoIO.write(frame) to 'dir/%06d.jpg' with gpu_encode (upload of the host pixels, encode, file write), host time;
(c) the same call without gpu_encode -- the Pillow save this tree has always done --, alternating with (b);
(d) frames/s of readahead.track_stream (bench.py's config[1] workload) with write_frames=True to such a pattern, the
    writer on the GPU and in Pillow, alternating, each a fresh MOT.

    python scripts/jpeg_encode_timing.py [--iters 60] [--frames 120] [--rounds 3] [--out profiles/jpeg_encode.txt]"""
import argparse
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

SIZE = (1920, 1080)
QUALITY = 75


def med(x):
    return float(np.median(x))


def fmt(v):
    return f'median {med(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}'


def writer(tmp, name, gpu):
    from fastmot_amd import VideoIO
    stack = Path(tmp) / 'in.npy'
    if not stack.exists():
        np.save(stack, np.zeros((1, SIZE[1], SIZE[0], 3), np.uint8))
    return VideoIO(SIZE, str(stack), str(Path(tmp) / name / '%06d.jpg'), gpu_encode=gpu, jpeg_quality=QUALITY)


def call_part(ctx, args, tmp, lines):
    frame = np.ascontiguousarray(jc.content('textured', *SIZE)[:, :, ::-1])
    ctx.frame_configure(*SIZE, 0)
    ctx.frame_upload(frame)
    for _ in range(5):
        data = ctx.frame_encode_jpeg(QUALITY)
    dev, host = [], []
    for _ in range(args.iters):
        t0 = time.perf_counter()
        ctx.frame_encode_jpeg(QUALITY)
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(ctx.jpeg_encode_stream_ms())
    lines.append(f'(a) fm_frame_encode_jpeg, textured 1920x1080 quality {QUALITY} -> {len(data) / 1e3:.0f} KB ({len(data) / frame.nbytes * 100:.1f} % of the frame), {args.iters} calls')
    lines.append(f'(a) kernels on the encoder stream (HIP events): {fmt(dev)}')
    lines.append(f'(a) whole call on the host:                    {fmt(host)}')
    on, off = writer(tmp, 'gpu', True), writer(tmp, 'pillow', False)
    times = {True: [], False: []}
    for i in range(args.iters + 5):
        for gpu, s in ((True, on), (False, off)):
            t0 = time.perf_counter()
            s.write(frame)
            if i >= 5:
                times[gpu].append((time.perf_counter() - t0) * 1e3)
    on.release(), off.release()
    size_off = (Path(tmp) / 'pillow' / '000000.jpg').stat().st_size
    lines.append(f'(b) VideoIO.write, gpu_encode=True  (host pixels uploaded, encoded, file written): {fmt(times[True])}')
    lines.append(f'(c) VideoIO.write, gpu_encode=False (Pillow save, {size_off / 1e3:.0f} KB):                       {fmt(times[False])}')
    lines.append(f'(b) / (c): {med(times[True]) / med(times[False]):.2f}')


class _Clip:
    """A VideoIO whose frames come from a clip in memory, played forwards and backwards n steps long."""

    def __init__(self, stream, frames, n):
        self.stream, self.frames, self.n, self.i = stream, frames, n, 0
        self.resolution, self.gpu_encode, self.jpeg_quality = stream.resolution, stream.gpu_encode, stream.jpeg_quality

    def read(self):
        if self.i >= self.n:
            return None
        self.i += 1
        return self.frames[bench.ping_pong(self.i - 1, len(self.frames))]

    def write(self, frame):
        self.stream.write(frame)


class _Looped:
    def __init__(self, video):
        self.video = video

    def detections(self, step, *a):
        return self.video.detections(bench.ping_pong(step, self.video.n_frames), *a)


def loop_part(ctx, args, tmp, lines):
    from fastmot_amd import Track
    from fastmot_amd.readahead import track_stream
    from synthetic import SyntheticVideo
    cfg = bench.CONFIGS[1]
    assert tuple(cfg['size']) == SIZE
    video = SyntheticVideo(SIZE, n_ids=cfg['n_dets'], n_frames=bench.RING, seed=100)
    lines.append(f'(d) readahead.track_stream, {cfg["name"]}, write_frames=True to %06d.jpg at quality {QUALITY}: {args.frames} frames after 20 '
                 f'warm-up frames, next_frame prefetch; {args.rounds} alternating repetitions, each a fresh MOT')
    rates = {False: [], True: []}
    for r in range(args.rounds):
        for gpu in (False, True):
            mot = bench.build_mot(cfg, video)
            mot.detector._video = _Looped(video)
            Track._count = 0
            mot.reset(1 / 30.)
            out = writer(tmp, f'loop_{r}_{gpu}', gpu)
            try:
                track_stream(_Clip(out, video.frames, 20), mot, write_frames=True)
                ctx.synchronize()
                t0 = time.perf_counter()
                n = track_stream(_Clip(out, video.frames, args.frames), mot, write_frames=True)
                ctx.synchronize()
                rates[gpu].append(n / (time.perf_counter() - t0))
            finally:
                out.release()
            mot.tracker._clear_tracks()
            del mot
    for gpu, v in rates.items():
        lines.append(f'(d) gpu_encode={gpu!s:5s}: median {med(v):.1f} frames/s (repetitions {", ".join(f"{x:.1f}" for x in v)})')
    lines.append(f'(d) on / off: {med(rates[True]) / med(rates[False]):.2f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=60)
    ap.add_argument('--frames', type=int, default=120)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'jpeg_encode.txt'))
    args = ap.parse_args()
    from fastmot_amd import models
    from fastmot_amd.runtime import get_context
    models.allow_random_weights()               # timing only: the networks' values do not matter
    ctx = get_context()
    lines = [f'scripts/jpeg_encode_timing.py on {ctx.device_info()["name"]}; times are host perf_counter unless marked HIP events']
    with tempfile.TemporaryDirectory() as tmp:
        call_part(ctx, args, tmp, lines)
        print('\n'.join(lines), flush=True)
        done = len(lines)
        loop_part(ctx, args, tmp, lines)
        print('\n'.join(lines[done:]), flush=True)
    text = '\n'.join(lines) + '\n'
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
