"""Tiled YOLO detection (YOLODetector(tiling_grid=...)): what a grid of tiles costs, on one MI355X at config[1]
(YOLOv4 @ 608, 1080p frames), everything inside ONE call (boxes of a pool differ between calls):

  1. the stand-alone detector pass -- frame resident, fm_detect_async + fm_detect_sync in a loop, wall clock and the
     HIP-event time of the network launches -- untiled, grid (2, 1) and grid (2, 2)
  2. host time of the cross-tile merge in the library (fm_detect_merge_tiles) against the Python SSDDetector.merge_dets
     on the same per-tile detections (those of the grid (2, 2) pass)
  3. frames/s of readahead.track_stream over bench.py's config[1] workload, untiled against grid (2, 1), alternating rounds
  4. with --parent-tree DIR (a built checkout of the parent commit): the default, untiled bench.py line of this tree
     against the parent's, alternating rounds; the default rate must lie inside the spread of the parent's rounds

The heads are scripted (tests/synthetic.py) so that the sort / NMS kernels have work: calibrated on the whole frame for the
untiled detector and on a tile's picture for the tiled ones (a tile shows the network a less reduced picture).

    python scripts/tiled_detect_timing.py [--steps 200] [--rounds 3] [--parent-tree DIR] [--out profiles/tiled_detect.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(1, str(ROOT / 'tests'))
sys.path.insert(2, str(ROOT / 'oracle'))

import numpy as np  # noqa: E402

import bench  # noqa: E402

CANDIDATES = 1500        # per frame (untiled) / per tile (tiled): bench.py's default regime
MAX_CANDIDATES = 32768   # (more than the 22 743 rows of a 608 x 608 tile: a tile cannot overflow whatever the calibration)


def tile_frame(frame, tile_wh, grid, overlap=0.25, t=0):
    """The picture tile t shows the network, as a BGR frame of the network's input size (restated preprocessing)."""
    import np_oracle
    from fastmot_amd.detector import generate_tiles
    tiles, (rw, rh) = generate_tiles(tile_wh, grid, overlap)
    region = np.rint(np_oracle.yolo_preprocess(frame, (rh, rw)) * 255)
    x, y = int(tiles[t][0]), int(tiles[t][1])
    return np.ascontiguousarray(region[::-1, y:y + tile_wh[1], x:x + tile_wh[0]].transpose(1, 2, 0).astype(np.uint8))


def head_weights(cfg, frame, grid):
    from fastmot_amd import models
    from synthetic import scripted_head_weights
    if grid == (1, 1):
        return scripted_head_weights(cfg['size'], cfg['yolo'], 1, frame, CANDIDATES)
    shape = models.YOLO.get_model(cfg['yolo']).INPUT_SHAPE
    tile_wh = (shape[2], shape[1])
    return scripted_head_weights(tile_wh, cfg['yolo'], 1, tile_frame(frame, tile_wh, grid), CANDIDATES)


def pass_times(ctx, cfg, frame, grid, iters):
    from fastmot_amd.detector import YOLODetector
    det = YOLODetector(cfg['size'], (1,), model=cfg['yolo'], conf_thresh=0.25, nms_thresh=0.5,
                       weights=head_weights(cfg, frame, grid), max_candidates=MAX_CANDIDATES, tiling_grid=grid)
    ctx.set_option('net_timing', 1)
    try:
        dets = det(frame)
        counts = ctx.detect_last_counts()
        for _ in range(10):
            ctx.detect_async()
            ctx.detect_sync()
        wall, net = [], []
        for _ in range(iters):
            t0 = time.perf_counter()
            ctx.detect_async()
            ctx.detect_sync()
            wall.append((time.perf_counter() - t0) * 1e3)
            net.append(ctx.detect_net_ms())
    finally:
        ctx.set_option('net_timing', 0)
    tiles = det.last_tile_detections
    line = (f'stand-alone pass, grid {grid[0]} x {grid[1]}: network {statistics.median(net):.3f} ms (HIP events), '
            f'async + sync {statistics.median(wall):.3f} ms wall; median of {iters}; {counts[0]} candidates, '
            f'{counts[1]} detections before the merge, {len(dets)} returned')
    det.backend.close()
    return line, statistics.median(net), tiles, det


def merge_times(tiles, n_tiles, thresh):
    from fastmot_amd import _lib
    from fastmot_amd.detector import SSDDetector
    union = np.concatenate(tiles).view(np.recarray)
    ids = np.concatenate([np.full(len(d), t) for t, d in enumerate(tiles)])

    def best(fn, reps):
        out = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = fn()
            out.append((time.perf_counter() - t0) * 1e6)
        return statistics.median(out), len(r)
    lib_us, n_lib = best(lambda: _lib.merge_tiles(union, ids, n_tiles, thresh), 200)
    py_us, n_py = best(lambda: SSDDetector.merge_dets(union, ids, n_tiles, thresh), 20)
    assert n_lib == n_py
    return (f'cross-tile merge of {len(union)} rows -> {n_lib}: library {lib_us:.1f} us (ctypes call included), '
            f'Python merge_dets {py_us:.1f} us; medians of 200 / 20')


class Clip:
    """bench.py's clip as a stream for track_stream: n frames, played forwards and backwards; the clock starts when
    frame `mark` is read (the steps before it are warm-up)."""

    def __init__(self, frames, size, n, mark):
        self.frames, self.resolution, self.n, self.mark, self.i, self.t_mark = frames, size, n, mark, 0, None

    def read(self):
        if self.i >= self.n:
            return None
        if self.i == self.mark:
            self.t_mark = time.perf_counter()
        self.i += 1
        return self.frames[bench.ping_pong(self.i - 1, len(self.frames))]


def build_mot(cfg, video, grid):
    """bench.build_mot with the tiling keys passed through yolo_detector_cfg."""
    import fastmot_amd.mot as mot_mod
    orig = mot_mod.MOT

    def with_tiles(*a, **kw):
        y = kw['yolo_detector_cfg']
        y.tiling_grid, y.max_candidates = grid, MAX_CANDIDATES
        y.weights = head_weights(cfg, video.frames[0], grid)
        return orig(*a, **kw)
    mot_mod.MOT = with_tiles
    try:
        return bench.build_mot(cfg, video, nms_candidates=0)
    finally:
        mot_mod.MOT = orig


class CountedVideo:
    """The detections InjectedYOLODetector hands the tracker, by step rather than by frame index set from outside."""

    def __init__(self, video):
        self.video = video

    def __getattr__(self, k):
        return getattr(self.video, k)

    def detections(self, step, label=1, labels=None):
        return self.video.detections(bench.ping_pong(step, bench.RING), label, labels)


def stream_rates(ctx, cfg, video, frames, steps, warmup, rounds, lines):
    from fastmot_amd import Track
    from fastmot_amd.readahead import track_stream
    rates = {(1, 1): [], (2, 1): []}
    for r in range(rounds):
        for grid in rates:
            mot = build_mot(cfg, video, grid)
            mot.detector.bind_video(CountedVideo(video), labels=cfg['labels'])
            Track._count = 0
            mot.reset(1 / 30.)
            clip = Clip(frames, cfg['size'], warmup + steps, warmup)
            assert track_stream(clip, mot) == warmup + steps
            ctx.synchronize()
            rates[grid].append(steps / (time.perf_counter() - clip.t_mark))
            lines.append(f'round {r} track_stream grid {grid[0]} x {grid[1]}: {rates[grid][-1]:.1f} frames/s')
            mot.tracker._clear_tracks()
            del mot
    for grid, v in rates.items():
        lines.append(f'track_stream grid {grid[0]} x {grid[1]}: median {statistics.median(v):.1f} frames/s '
                     f'(runs {", ".join(f"{x:.1f}" for x in v)})')


def bench_ab(parent, steps, warmup, rounds, lines):
    """The default bench.py line, this tree against a built checkout of the parent commit, alternating."""
    fps = {'parent': [], 'this': []}
    for r in range(rounds):
        for name, tree in (('parent', Path(parent)), ('this', ROOT)):
            env = dict(os.environ)
            env.pop('FASTMOT_LIB_PATH', None)
            res = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup),
                                  '--no-cpu-baseline', '--no-variants'], cwd=tree, env=env, stdout=subprocess.PIPE,
                                 stderr=subprocess.PIPE, timeout=600)
            if res.returncode != 0:
                raise RuntimeError(f'bench.py failed in {tree} (exit {res.returncode}):\n{res.stderr.decode()[-2000:]}')
            value = json.loads(res.stdout.decode().strip().splitlines()[-1])['value']
            fps[name].append(value)
            lines.append(f'round {r} bench.py default ({name}): {value:.1f} frames/s')
    lo, hi = min(fps['parent']), max(fps['parent'])
    med = statistics.median(fps['this'])
    inside = lo <= med <= hi or med > hi
    lines.append(f'bench.py default: parent {lo:.1f} .. {hi:.1f} frames/s over {rounds} rounds, this tree median {med:.1f} '
                 f'(runs {", ".join(f"{x:.1f}" for x in fps["this"])}): '
                 f'{"inside the parent spread or above it" if inside else "BELOW the parent spread"}')
    return inside


class Log(list):
    """The result lines: printed and written to the output file as they come (a run cut short keeps what it measured)."""

    def __init__(self, out):
        super().__init__()
        self.out = Path(out) if out else None
        if self.out:
            self.out.parent.mkdir(parents=True, exist_ok=True)
            self.out.write_text('')

    def append(self, line):
        super().append(line)
        print(line, flush=True)
        if self.out:
            with self.out.open('a') as f:
                f.write(line + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--stream-rounds', type=int, default=2)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = Log(args.out)
    cfg = bench.CONFIGS[1]
    lines.append(f'# scripts/tiled_detect_timing.py, {cfg["name"]}: {cfg["desc"]}; one MI355X, one call')
    lines.append(f'# heads scripted for ~{CANDIDATES} candidates per frame (untiled) / per tile (tiled); bench.py and '
                 f'track_stream: {args.steps} timed steps')
    ok = True
    if args.parent_tree:       # (first, in fresh processes: this process has not touched the GPU yet)
        ok = bench_ab(args.parent_tree, args.steps, args.warmup, args.rounds, lines)
    from fastmot_amd import models
    from fastmot_amd.runtime import get_context
    from synthetic import SyntheticVideo
    models.allow_random_weights()
    ctx = get_context()
    size = cfg['size']
    video = SyntheticVideo(size, n_ids=cfg['n_dets'], n_frames=bench.RING, seed=100)
    ctx.frame_configure(size[0], size[1], bench.RING)
    host = ctx.pinned_frames(bench.RING)
    for i, fr in enumerate(video.frames):
        host[i] = fr
    frames = [host[i] for i in range(bench.RING)]
    net = {}
    tiles22 = det22 = None
    for grid in ((1, 1), (2, 1), (2, 2)):
        line, net[grid], tiles, det = pass_times(ctx, cfg, video.frames[0], grid, args.iters)
        lines.append(line)
        if grid == (2, 2):
            tiles22, det22 = tiles, det
    for grid in ((2, 1), (2, 2)):
        lines.append(f'grid {grid[0]} x {grid[1]}: network pass {net[grid] / net[1, 1]:.2f} x the untiled pass, '
                     f'{net[grid] / (grid[0] * grid[1]):.3f} ms per tile')
    lines.append(merge_times(tiles22, det22.n_tiles, det22.merge_thresh))
    stream_rates(ctx, cfg, video, frames, args.steps, args.warmup, args.stream_rounds, lines)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
