"""YOLOv8 from ONNX (models/onnx_detector.py, csrc/dfl_decode.h): what a pass costs on one MI355X, everything inside ONE
call, seeded weights (tests/yolov8_ref.py modules exported with torch's exporter), HIP-event times:

  1. with --parent-tree DIR (a built checkout of the parent commit): the default bench.py line of this tree against the
     parent's, alternating rounds (the default line runs YOLOv4: none of the new code)
  2. a v8n and a v8s pass at 640 x 640, batch 1, 1920 x 1080 frames: launches (layers of the table + the decode) and the
     network's time (events around its launches, median of 40 passes), then the per-layer table (fm_net_profile_layers):
     the baseline for later work -- nothing here is tuned
  3. the decode alone (fm_detect_decode_us, each launch between two events, medians of 9 x 20 launches, the forms
     alternating): dfl_decode_kernel (16 lanes per cell) and dfl_decode_cell_kernel (one thread per cell) on the v8n heads
     (8400 cells, 80 classes), once with every cell over the threshold (the seeded weights as they are) and once with none
     (class bias - 8), beside decode_kernel on YOLOv4 @ 608 with 80 classes (22 743 rows)

    python scripts/yolov8_timing.py [--parent-tree DIR] [--out profiles/yolov8_detect.txt]"""
import argparse
import statistics
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(HERE))
sys.path.insert(1, str(HERE / 'tests'))
sys.path.insert(2, str(HERE / 'scripts'))

import numpy as np  # noqa: E402

SIZE = (1920, 1080)


def frame():
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (SIZE[1] // 8 + 1, SIZE[0] // 8 + 1, 3)).astype(np.uint8)
    return np.kron(base, np.ones((8, 8, 1), np.uint8))[:SIZE[1], :SIZE[0]]


def decode_times(ctx, forms, turns=9, iters=20):
    """{form: median over `turns` of the mean of `iters` launches}, the forms alternating; form None: the option untouched."""
    res = {f: [] for f in forms}
    for _ in range(turns):
        for f in forms:
            if f is not None:
                ctx.set_option('dfl_decode_form', f)
            res[f].append(ctx.detect_decode_us(iters))
    if forms != [None]:
        ctx.set_option('dfl_decode_form', 0)
    return {f: statistics.median(v) for f, v in res.items()}


def v8_pass(ctx, tmp, name, net, lines):
    import yolov8_ref as R
    from fastmot_amd import models
    from fastmot_amd.detector import YOLODetector
    from fastmot_amd.models import graph as G
    path = Path(tmp) / f'{name}.onnx'
    path.write_bytes(R.export(net, (640, 640)))
    M = models.YOLO.from_onnx(path, name=f'Timing_{name}')
    det = YOLODetector(SIZE, tuple(range(80)), model=M.__name__, conf_thresh=0.25, nms_thresh=0.5, max_candidates=16384)
    img = frame()
    ctx.set_option('net_timing', 1)
    try:
        det(img)
        for _ in range(10):
            ctx.detect_async()
            ctx.detect_sync()
        net_ms = []
        for _ in range(40):
            ctx.detect_async()
            ctx.detect_sync()
            net_ms.append(ctx.detect_net_ms())
    finally:
        ctx.set_option('net_timing', 0)
    cand = ctx.detect_last_counts()[0]
    g = det.graph
    names = {v: k[3:] for k, v in vars(G).items() if k.startswith('OP_')}
    lines.append(f'{name} @ 640 x 640, batch 1: {len(g.layers)} layer launches + 1 decode; network {statistics.median(net_ms):.3f} ms '
                 f'(HIP events around its launches, median of 40, min {min(net_ms):.3f}); {g.conv_flops() / 1e9:.2f} GFLOP of '
                 f'convolutions; {cand} candidates over 0.25 with seeded weights')
    per = det.backend.profile_layers(1, iters=20)
    lines.append(f'{name} per layer (fm_net_profile_layers, 20 iterations each; sum {per.sum():.3f} ms):')
    lines.append(f'  {"#":>3} {"op":<10} {"k":>1} {"s":>1} {"cin":>5} {"cout":>5} {"out h x w":>10} {"us":>8}')
    for i, (d, ms) in enumerate(zip(g.layers, per)):
        o = d['out']
        lines.append(f'  {i:>3} {names[d["op"]]:<10} {d["k"]:>1} {d["stride"]:>1} {d["cin"]:>5} {d["cout"]:>5} {o.h:>4} x {o.w:<4} {ms * 1e3:>8.2f}')
    return det


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from tiled_detect_timing import Log, bench_ab
    lines = Log(args.out)
    lines.append('# scripts/yolov8_timing.py: YOLOv8 detectors from ONNX (DFL heads); one MI355X, one call, seeded weights')
    ok = True
    if args.parent_tree:       # (first, in fresh processes: this process has not touched the GPU yet)
        ok = bench_ab(args.parent_tree, args.steps, args.warmup, args.rounds, lines)
    else:
        lines.append('bench.py default against the parent: not measured (no --parent-tree)')
    import yolov8_ref as R
    from fastmot_amd import models
    from fastmot_amd.detector import YOLODetector
    from fastmot_amd.runtime import get_context
    ctx = get_context()
    models.allow_random_weights()
    with tempfile.TemporaryDirectory() as tmp:
        det = v8_pass(ctx, tmp, 'YOLOv8n', R.yolov8n(), lines)
        t = decode_times(ctx, [0, 1])
        lines.append(f'decode alone, v8n heads (8400 cells, 80 classes, 3 levels; EVERY cell passes with these seeded weights): dfl_decode_kernel (16 lanes per cell) {t[0]:.2f} us, '
                     f'dfl_decode_cell_kernel (one thread per cell) {t[1]:.2f} us; medians of 9 turns x 20 launches, alternating, '
                     f'each launch between two events')
        det.backend.close()
        # the same heads with the class bias lowered by 8: no cell passes, the decode is the class scan alone -- the two
        # ends between which a real frame lies (a trained network passes about 1 % of its cells)
        path = Path(tmp) / 'v8n_quiet.onnx'
        path.write_bytes(R.export(R.yolov8n(cls_bias=-8.0), (640, 640)))
        M = models.YOLO.from_onnx(path, name='Timing_YOLOv8n_quiet')
        det = YOLODetector(SIZE, tuple(range(80)), model=M.__name__, conf_thresh=0.25, nms_thresh=0.5, max_candidates=16384)
        det(frame())
        t = decode_times(ctx, [0, 1])
        lines.append(f'decode alone, v8n heads, class bias - 8 ({ctx.detect_last_counts()[0]} candidates: the class scan alone): '
                     f'dfl_decode_kernel {t[0]:.2f} us, dfl_decode_cell_kernel {t[1]:.2f} us; measured the same way')
        det.backend.close()
        det = v8_pass(ctx, tmp, 'YOLOv8s', R.yolov8s(), lines)
        det.backend.close()
    det = YOLODetector(SIZE, tuple(range(80)), model='YOLOv4_608', conf_thresh=0.25, nms_thresh=0.5, max_candidates=65536)
    det(frame())
    t = decode_times(ctx, [None])
    lines.append(f'decode alone, YOLOv4 @ 608, 80 classes (22 743 rows): decode_kernel {t[None]:.2f} us, measured the same way')
    det.backend.close()
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
