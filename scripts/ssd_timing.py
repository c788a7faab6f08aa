"""SSD-MobileNetV1 on the device (SSDDetector, detector_type SSD): what a pass costs on one MI355X at 1080p with the
default 4 x 2 tiling grid (8 tiles of 300 x 300), everything inside ONE call:

  1. with --parent-tree DIR (a built checkout of the parent commit): the default bench.py line of this tree against the
     parent's, alternating rounds (the default line runs no code of the SSD path)
  2. per stage, HIP events on the detector stream: the preprocess kernel, the network pass (batch 8) and decode / NMS /
     top-K, with the separable blocks fused (FASTMOT_SEPCONV=1: one FM_OP_SEPCONV launch each) and unfused (=0:
     FM_OP_DWCONV + pointwise conv); per-layer event times of the 13 blocks in both forms
  3. detect_async + postprocess wall time, frame resident on the host (upload included)

Weights are seeded random (no model file is needed for timing).

    python scripts/ssd_timing.py [--iters 50] [--rounds 3] [--parent-tree DIR] [--out profiles/ssd_detect.txt]"""
import argparse
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(1, str(ROOT / 'tests'))
sys.path.insert(2, str(ROOT / 'scripts'))

import numpy as np  # noqa: E402

from tiled_detect_timing import Log, bench_ab  # noqa: E402

SIZE = (1920, 1080)


def one_form(ctx, fused, frame, iters, lines):
    from fastmot_amd.detector import SSDDetector
    from fastmot_amd.models import graph as G
    os.environ['FASTMOT_SEPCONV'] = '1' if fused else '0'
    det = SSDDetector(SIZE, (1,), model='SSDMobileNetV1')
    name = 'fused (FM_OP_SEPCONV)' if fused else 'unfused (FM_OP_DWCONV + conv)'
    n = det.batch_size
    for _ in range(5):
        dets = det(frame)
    ctx.set_option('net_timing', 1)
    stages, wall = [], []
    try:
        for _ in range(iters):
            t0 = time.perf_counter()
            det.detect_async(frame)
            det.postprocess()
            wall.append((time.perf_counter() - t0) * 1e3)
            stages.append(ctx.ssd_stage_ms())
    finally:
        ctx.set_option('net_timing', 0)
    pre, net, post = (statistics.median(s[i] for s in stages) for i in range(3))
    lines.append(f'{name}: {len(det.graph.layers)} launches at batch {n}; HIP events, median of {iters}: preprocess {pre * 1e3:.1f} us, '
                 f'network {net * 1e3:.1f} us, decode / NMS / top-K {post * 1e3:.1f} us; detect_async + postprocess '
                 f'{statistics.median(wall):.3f} ms wall (upload of the 1080p frame included); {len(dets)} detections')
    per = det.net.profile_layers(n, iters=10) * 1e3
    ops = [d['op'] for d in det.graph.layers]
    blocks = []
    i = 0
    while i < len(ops):
        if ops[i] == G.OP_SEPCONV:
            blocks.append(per[i]); i += 1
        elif ops[i] == G.OP_DWCONV:
            blocks.append(per[i] + per[i + 1]); i += 2
        else:
            i += 1
    lines.append(f'{name}: per-layer event times, sum over all layers {per.sum():.1f} us; the 13 separable blocks {sum(blocks):.1f} us: '
                 + ' '.join(f'{b:.1f}' for b in blocks))
    det.net.close()
    return net, blocks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = Log(args.out)
    lines.append('# scripts/ssd_timing.py: SSDMobileNetV1, 1080p frames, tiling grid 4 x 2 (8 tiles of 300 x 300); one MI355X, one call')
    ok = True
    if args.parent_tree:       # (first, in fresh processes: this process has not touched the GPU yet)
        ok = bench_ab(args.parent_tree, args.steps, args.warmup, args.rounds, lines)
    from fastmot_amd import models
    from fastmot_amd.runtime import get_context
    models.allow_random_weights()
    ctx = get_context()
    frame = np.random.default_rng(0).integers(0, 256, (SIZE[1], SIZE[0], 3), dtype=np.uint8)
    res = {f: one_form(ctx, f, frame, args.iters, lines) for f in (True, False)}
    (nf, bf), (nu, bu) = res[True], res[False]
    lines.append(f'network pass fused / unfused: {nf * 1e3:.1f} / {nu * 1e3:.1f} us ({nf / nu:.2f} x); separable blocks '
                 f'{sum(bf):.1f} / {sum(bu):.1f} us ({sum(bf) / sum(bu):.2f} x)')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
