"""IBN-Net ReID models (models/onnx_graph.py: FM_OP_INSTNORM, GeM in FM_OP_POOLHEAD): what they cost on one MI355X,
everything inside ONE call, seeded weights, HIP-event times, medians of 40 samples, variants alternating:

  1. with --parent-tree DIR (a built checkout of the parent commit): the default bench.py line of this tree against the
     parent's, alternating rounds (the default line runs OSNet: none of the new code)
  2. with --parent-tree: the PLAIN pooled head (2048 channels over 8 x 4, no FC) of this tree against the parent's, fresh
     processes alternating -- the plain instantiation of the template is meant to be the parent's code
  3. a ResNet-50-IBN-a + GeM + BN-neck pass beside the plain ResNet-50 pass (256 x 128 crops) at batch 16 and 50: the two
     networks are created in turn, four times each, ten samples per turn
  4. FM_OP_INSTNORM alone on the layer shapes of ResNet-50-IBN-a and -b, against the time its bytes (one read and one
     write of the view) take at the achievable HBM rate of 6.3 TB/s
  5. the GeM head (p = 3 and p = 2.6) against the plain head at C = 2048

    python scripts/reid_ibn_timing.py [--parent-tree DIR] [--out profiles/reid_ibn.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]
ROOT = Path(os.environ.get('REID_IBN_TIMING_ROOT', HERE))        # (--plain-head-only in a parent checkout: that tree's package)
sys.path.insert(0, str(ROOT))
sys.path.insert(1, str(HERE / 'tests'))
sys.path.insert(2, str(HERE / 'scripts'))

import numpy as np  # noqa: E402

HBM = 6.3e12        # bytes / s, the achievable rate (a float4 copy)
SAMPLES = 40


def one_layer_times(ctx, g, dim, x, batches, samples=SAMPLES):
    """Median HIP-event time in us of the ONE layer of g per batch size."""
    from fastmot_amd.engine import HipNet, NET_EXTRACTOR
    if dim:
        ctx.feat_configure(dim)
    net = HipNet(ctx, NET_EXTRACTOR, g, max(batches))
    try:
        net.write(g.input, x)
        out = {}
        for b in batches:
            net.run(b)
            out[b] = statistics.median(float(net.profile_layers(b, iters=3)[0]) * 1e3 for _ in range(samples))
        return out
    finally:
        net.close()


def plain_head(ctx, batches=(16, 50)):
    from fastmot_amd.models import graph as G
    rng = np.random.default_rng(1)
    g = G.Graph(None, (8, 4), 2048)
    g.poolhead('head', g.input)
    g.outputs = [g.input]
    x = rng.normal(0.3, 1, (max(batches), 8, 4, 2048)).astype(np.float16)
    return one_layer_times(ctx, g, 2048, x, batches)


def plain_head_ab(parent, rounds, lines):
    """The plain head in fresh processes, the parent's package and this one alternating."""
    res = {'parent': [], 'this': []}
    for r in range(rounds):
        for name, tree in (('parent', Path(parent)), ('this', HERE)):
            env = dict(os.environ, REID_IBN_TIMING_ROOT=str(tree))
            env.pop('FASTMOT_LIB_PATH', None)
            p = subprocess.run([sys.executable, str(Path(__file__).resolve()), '--plain-head-only'], cwd=tree, env=env,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
            if p.returncode != 0:
                raise RuntimeError(f'plain head in {tree} failed (exit {p.returncode}):\n{p.stderr.decode()[-2000:]}')
            t = json.loads(p.stdout.decode().strip().splitlines()[-1])
            res[name].append(t)
            lines.append(f'round {r} plain head 8 x 4 x 2048 ({name}): ' + ', '.join(f'batch {b}: {v:.2f} us' for b, v in t.items()))
    ok = True
    for b in res['this'][0]:
        lo, hi = min(t[b] for t in res['parent']), max(t[b] for t in res['parent'])
        med = statistics.median(t[b] for t in res['this'])
        inside = med <= hi
        ok = ok and inside
        lines.append(f'plain head batch {b}: parent {lo:.2f} .. {hi:.2f} us over {rounds} rounds, this tree median {med:.2f} us: '
                     f'{"inside the parent spread or below it" if inside else "ABOVE the parent spread"}')
    return ok


def network_passes(ctx, files, batches, lines, turns=4, per_turn=10):
    from fastmot_amd.engine import HipNet, NET_EXTRACTOR
    from fastmot_amd.models import onnx_graph
    import torch_ref
    x = np.random.default_rng(0).normal(0, 1, (max(batches), 256, 128, 3)).astype(np.float16)
    wall = {(n, b): [] for n in files for b in batches}
    by_op = {}
    for turn in range(turns):
        for name, data in files.items():
            g, _ = onnx_graph.lower(data)
            ctx.feat_configure(g.layers[-1]['cout'])
            net = HipNet(ctx, NET_EXTRACTOR, g, max(batches), reuse_buffers=True)
            try:
                net.write(g.input, x)
                for b in batches:
                    for _ in range(3):
                        net.run(b)
                        net.read_embeddings(b)
                    for _ in range(per_turn):
                        t0 = time.perf_counter()
                        net.run(b)
                        net.read_embeddings(b)
                        wall[name, b].append((time.perf_counter() - t0) * 1e3)
                    if turn == 0:
                        per = net.profile_layers(b, iters=5) * 1e3
                        ops = {}
                        for d, t in zip(g.layers, per):
                            k = torch_ref.OP_NAMES[d['op']]
                            ops[k] = (ops.get(k, (0, 0.0))[0] + 1, ops.get(k, (0, 0.0))[1] + t)
                        by_op[name, b] = (ops, float(per.sum()), net.cost(b))
            finally:
                net.close()
    for name in files:
        for b in batches:
            ms = statistics.median(wall[name, b])
            ops, total, (flops, nbytes) = by_op[name, b]
            lines.append(f'{name} batch {b}: run + read-back {ms:.3f} ms wall (median of {len(wall[name, b])}; min {min(wall[name, b]):.3f}), '
                         f'{ms / b * 1e3:.1f} us per crop; per-layer events sum {total / 1e3:.3f} ms ('
                         + ', '.join(f'{n} {k} {t / 1e3:.3f}' for k, (n, t) in sorted(ops.items())) + f'); fm_net_cost {flops / 1e9:.1f} GFLOP, '
                         f'{nbytes / 1e6:.0f} MB')
    names = list(files)
    for b in batches:
        a, c = (statistics.median(wall[n, b]) for n in names)
        lines.append(f'batch {b}: {names[1]} / {names[0]} = {c:.3f} / {a:.3f} ms = {c / a:.3f}')


def instnorm_alone(ctx, batches, lines):
    from fastmot_amd.models import graph as G
    rng = np.random.default_rng(2)
    shapes = [('IBN-a stage 1', 64, 32, (64, 32)), ('IBN-a stage 2, first block', 128, 64, (64, 32)), ('IBN-a stage 2', 128, 64, (32, 16)),
              ('IBN-a stage 3, first block', 256, 128, (32, 16)), ('IBN-a stage 3', 256, 128, (16, 8)),
              ('IBN-b stem (re-read path)', 64, 64, (128, 64)), ('IBN-b stage 1', 256, 256, (64, 32)), ('IBN-b stage 2', 512, 512, (32, 16))]
    for label, c, cn, hw in shapes:
        g = G.Graph(None, hw, c)
        dst = g.instnorm('in', g.input, rng.uniform(0.5, 1.5, cn), rng.normal(0, 0.3, cn), 1e-5, 'relu')
        g.outputs = [dst]
        x = rng.normal(0, 1, (max(batches),) + hw + (c,)).astype(np.float16)
        t = one_layer_times(ctx, g, 0, x, batches)
        parts = []
        for b in batches:
            nbytes = 2.0 * b * hw[0] * hw[1] * c * 2
            floor = nbytes / HBM * 1e6
            parts.append(f'batch {b}: {t[b]:.2f} us for {nbytes / 1e6:.2f} MB ({floor:.2f} us at 6.3 TB/s: x{t[b] / floor:.1f}, '
                         f'{nbytes / t[b] / 1e6:.2f} TB/s)')
        lines.append(f'instnorm alone, {label}, C {c} cn {cn} over {hw[0]} x {hw[1]}: ' + '; '.join(parts))


def heads_alone(ctx, batches, lines):
    from fastmot_amd.models import graph as G
    rng = np.random.default_rng(1)
    for hw in ((8, 4), (16, 8)):
        x = rng.normal(0.3, 1, (max(batches),) + hw + (2048,)).astype(np.float16)
        scale, shift = rng.uniform(0.5, 1.5, 2048).astype(np.float32), rng.normal(0, 0.3, 2048).astype(np.float32)
        res = {}
        for turn in range(2):       # (plain, p = 3, p = 2.6, and again: alternating)
            for name, gem in (('plain', None), ('GeM p = 3', (3.0, 1e-6)), ('GeM p = 2.6', (2.6, 1e-6))):
                g = G.Graph(None, hw, 2048)
                g.poolhead('head', g.input, neck=(scale, shift), gem=gem)
                g.outputs = [g.input]
                t = one_layer_times(ctx, g, 2048, x, batches, samples=SAMPLES // 2)
                for b in batches:
                    res.setdefault((name, b), []).append(t[b])
        for name in ('plain', 'GeM p = 3', 'GeM p = 2.6'):
            lines.append(f'head alone, {hw[0]} x {hw[1]} x 2048 with BN neck, {name}: ' +
                         ', '.join(f'batch {b}: {statistics.mean(res[name, b]):.2f} us' for b in batches))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--plain-head-only', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.plain_head_only:
        from fastmot_amd.runtime import get_context
        print(json.dumps({str(b): v for b, v in plain_head(get_context()).items()}))
        return 0
    from tiled_detect_timing import Log, bench_ab
    lines = Log(args.out)
    lines.append('# scripts/reid_ibn_timing.py: IBN-Net ReID models (FM_OP_INSTNORM, GeM head), 256 x 128 crops; one MI355X, one call')
    ok = True
    if args.parent_tree:       # (first, in fresh processes: this process has not touched the GPU yet)
        ok = bench_ab(args.parent_tree, args.steps, args.warmup, args.rounds, lines)
        ok = plain_head_ab(args.parent_tree, args.rounds, lines) and ok
    else:
        lines.append('bench.py default against the parent, plain head against the parent: not measured (no --parent-tree)')
    import ibn_ref
    import resnet_ref as R
    from fastmot_amd.runtime import get_context
    ctx = get_context()
    batches = (16, 50)
    files = {'ResNet-50': R.export(R.resnet50(head='bnneck'), hw=(256, 128)),
             'ResNet-50-IBN-a + GeM': R.export(ibn_ref.resnet50_ibn_a(), hw=(256, 128))}
    network_passes(ctx, files, batches, lines)
    instnorm_alone(ctx, batches, lines)
    heads_alone(ctx, batches, lines)
    ctx.feat_configure(512)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
