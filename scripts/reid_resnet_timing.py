"""ResNet-50 as a ReID model (models/onnx_graph.py, FM_OP_POOLHEAD): what a pass costs on one MI355X, everything inside
ONE call:

  1. with --parent-tree DIR (a built checkout of the parent commit): the default bench.py line of this tree against the
     parent's, alternating rounds (the default line runs OSNet: no code of the new path)
  2. a ResNet-50 pass (256 x 128 crops, seeded weights, exported to ONNX by torch and lowered) at batch 16 and 50:
     wall time of run + embedding read-back with the captured graph, the sum of the per-layer HIP-event times, the conv
     roofline figures of fm_net_cost, and the per-layer times by kernel; the same with the streamed conv kernel switched
     off (FASTMOT_CONVS_MAXP=0: its layers go to the DMA-fed kernel) -- the selection threshold was tuned on the detector
     at batch 1
  3. the stem alone from the input tensor, 256 x 128 -> 64 x 32 x 64: FM_OP_STEMPOOL against the conv + max pool pair; and
     the whole ResNet-50 pass with FASTMOT_STEMPOOL=0
  4. the head alone, 2048 channels over 8 x 4: FM_OP_POOLHEAD without FC, with the FC 2048 -> 512 (+ ReLU), and the
     same FC head on FM_OP_HEAD (one thread per output row)

    python scripts/reid_resnet_timing.py [--iters 30] [--rounds 3] [--parent-tree DIR] [--out profiles/reid_resnet.txt]"""
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


def resnet50_pass(ctx, data, batches, iters, lines, label):
    from fastmot_amd.engine import HipNet, NET_EXTRACTOR
    from fastmot_amd.models import graph as G, onnx_graph
    import torch_ref
    g, _ = onnx_graph.lower(data)
    ctx.feat_configure(g.layers[-1]['cout'])
    net = HipNet(ctx, NET_EXTRACTOR, g, max(batches), reuse_buffers=True)
    x = np.random.default_rng(0).normal(0, 1, (max(batches), 256, 128, 3)).astype(np.float16)
    net.write(g.input, x)
    kinds = {}
    for d in g.layers:
        kinds[torch_ref.OP_NAMES[d['op']]] = kinds.get(torch_ref.OP_NAMES[d['op']], 0) + 1
    lines.append(f'{label}: {len(g.layers)} launches ({", ".join(f"{v} {k}" for k, v in sorted(kinds.items()))}); arena '
                 f'{g.arena_bytes / 2 ** 20:.1f} MB at batch {max(batches)}, parameters {len(g.blob) / 2 ** 20:.1f} MB')
    out = {}
    for b in batches:
        for _ in range(3):
            net.run(b)
            net.read_embeddings(b)
        wall = []
        for _ in range(iters):
            t0 = time.perf_counter()
            net.run(b)
            net.read_embeddings(b)
            wall.append((time.perf_counter() - t0) * 1e3)
        per = net.profile_layers(b, iters=5) * 1e3
        flops, nbytes = net.cost(b)
        ms = statistics.median(wall)
        by = {}
        for d, t in zip(g.layers, per):
            k = torch_ref.OP_NAMES[d['op']]
            by[k] = by.get(k, 0.0) + t
        lines.append(f'{label} batch {b}: run + read-back {ms:.3f} ms wall (median of {iters}; min {min(wall):.3f}), {ms / b * 1e3:.1f} us per crop; '
                     f'per-layer events sum {per.sum() / 1e3:.3f} ms ({", ".join(f"{k} {v / 1e3:.3f}" for k, v in sorted(by.items()))}); '
                     f'convs {flops / 1e9:.1f} GFLOP -> {flops / ms / 1e9:.1f} TFLOP/s, {nbytes / 1e6:.0f} MB minimal traffic -> {nbytes / ms / 1e6:.0f} GB/s; '
                     f'head launch {per[-1]:.1f} us, slowest layer {per.argmax()} ({torch_ref.OP_NAMES[g.layers[per.argmax()]["op"]]} '
                     f'k{g.layers[per.argmax()]["k"]} cin {g.layers[per.argmax()]["cin"]} cout {g.layers[per.argmax()]["cout"]}) {per.max():.1f} us')
        out[b] = ms
    net.close()
    return out


def head_alone(ctx, batches, lines):
    from fastmot_amd.engine import HipNet, NET_EXTRACTOR
    from fastmot_amd.models import graph as G
    rng = np.random.default_rng(1)
    C, D, hw = 2048, 512, (8, 4)
    w, b = rng.normal(0, C ** -0.5, (D, C)).astype(np.float32), rng.normal(0, 0.1, D).astype(np.float32)
    forms = {}
    g = G.Graph(None, hw, C)
    g.poolhead('head', g.input)
    forms['FM_OP_POOLHEAD, no FC (2048-d)'] = (g, C)
    g = G.Graph(None, hw, C)
    g.poolhead('head', g.input, fc=(w, b), relu=True)
    forms['FM_OP_POOLHEAD, FC 2048 -> 512 + ReLU (one wavefront per row)'] = (g, D)
    g = G.Graph(G.RandomWeights(seed=1), hw, C)
    g.head('fc', g.input, D)
    forms['FM_OP_HEAD, FC 2048 -> 512 + ReLU (one thread per row)'] = (g, D)
    x = rng.normal(0.3, 1, (max(batches),) + hw + (C,)).astype(np.float16)
    for name, (g, dim) in forms.items():
        g.outputs = [g.input]
        ctx.feat_configure(dim)
        net = HipNet(ctx, NET_EXTRACTOR, g, max(batches))
        net.write(g.input, x)
        times = []
        for bsz in batches:
            net.run(bsz)
            times.append(f'batch {bsz}: {float(net.profile_layers(bsz, iters=20)[0]) * 1e3:.1f} us')
        lines.append(f'head alone, 8 x 4 x 2048, {name}: ' + ', '.join(times))
        net.close()


def stem_alone(ctx, batches, lines):
    from fastmot_amd.engine import HipNet, NET_EXTRACTOR
    from fastmot_amd.models import graph as G
    rng = np.random.default_rng(2)
    w, b = rng.normal(0, (2.0 / 147) ** 0.5, (64, 3, 7, 7)).astype(np.float32), rng.normal(0, 0.2, 64).astype(np.float32)
    x = rng.normal(0, 1, (max(batches), 256, 128, 3)).astype(np.float16)
    for fused in (True, False):
        g = G.Graph(None, (256, 128), 3)
        if fused:
            y = g.stempool('stem', g.input, 64, (w, b), pool_pad=1)
        else:
            y = g.pool(g.conv('stem', g.input, 64, 7, 2, 'relu', pad=3, wb=(w, b)), 3, 2, 1)
        g.outputs = [y]
        net = HipNet(ctx, NET_EXTRACTOR, g, max(batches))
        net.write(g.input, x)
        times = []
        for bsz in batches:
            net.run(bsz)
            per = net.profile_layers(bsz, iters=20) * 1e3
            times.append(f'batch {bsz}: ' + ' + '.join(f'{t:.1f}' for t in per) + (f' = {per.sum():.1f}' if len(per) > 1 else '') + ' us')
        lines.append(f'stem alone, 256 x 128 x 3 -> 64 x 32 x 64, {"FM_OP_STEMPOOL" if fused else "FM_OP_CONV + FM_OP_MAXPOOL"}: ' + ', '.join(times))
        net.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = Log(args.out)
    lines.append('# scripts/reid_resnet_timing.py: ResNet-50 ReID (ONNX -> layer table), 256 x 128 crops; one MI355X, one call')
    ok = True
    if args.parent_tree:       # (first, in fresh processes: this process has not touched the GPU yet)
        ok = bench_ab(args.parent_tree, args.steps, args.warmup, args.rounds, lines)
    import resnet_ref as R
    from fastmot_amd.runtime import get_context
    ctx = get_context()
    data = R.export(R.resnet50(), hw=(256, 128))
    batches = (16, 50)
    base = resnet50_pass(ctx, data, batches, args.iters, lines, 'ResNet-50')
    os.environ['FASTMOT_CONVS_MAXP'] = '0'
    try:
        alt = resnet50_pass(ctx, data, batches, args.iters, lines, 'ResNet-50, FASTMOT_CONVS_MAXP=0')
    finally:
        del os.environ['FASTMOT_CONVS_MAXP']
    lines.append('streamed kernel on / off: ' + ', '.join(f'batch {b}: {base[b]:.3f} / {alt[b]:.3f} ms' for b in batches))
    os.environ['FASTMOT_STEMPOOL'] = '0'
    try:
        unf = resnet50_pass(ctx, data, batches, args.iters, lines, 'ResNet-50, FASTMOT_STEMPOOL=0')
    finally:
        del os.environ['FASTMOT_STEMPOOL']
    lines.append('fused stem on / off: ' + ', '.join(f'batch {b}: {base[b]:.3f} / {unf[b]:.3f} ms' for b in batches))
    ctx.feat_configure(512)
    stem_alone(ctx, batches, lines)
    head_alone(ctx, batches, lines)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
