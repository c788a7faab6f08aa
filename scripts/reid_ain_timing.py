"""torchreid's OSNet-AIN / OSNet-IBN (models/reid.py VARIANT 'ain' / 'ibn'): the fused block tail FM_OP_CONVIN (csrc/convin.hip)
against its unfused form (FASTMOT_CONVIN=0: a linear conv + FM_OP_INSTNORM), on one MI355X, everything inside ONE call, seeded
weights, 256 x 128 crops, the forms alternating:

  1. with --parent-tree DIR (a built checkout of the parent commit): the default bench.py line of this tree against the
     parent's, alternating rounds (the default line runs OSNet: none of the new code)
  2. a 50-crop and a 16-crop pass of OSNetAIN10 and OSNetIBN10, fused and unfused: the networks are created in turn, four
     times each, ten samples per turn (run + read-back, wall clock); OSNet10 beside them
  3. per-layer HIP-event times of the block tails in both forms (fused: the FM_OP_CONVIN layer; unfused: the conv and the
     FM_OP_INSTNORM behind it)

    python scripts/reid_ain_timing.py [--parent-tree DIR] [--out profiles/reid_ain.txt]"""
import argparse
import os
import statistics
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(HERE))
sys.path.insert(1, str(HERE / 'tests'))
sys.path.insert(2, str(HERE / 'scripts'))

import numpy as np  # noqa: E402

BATCHES = (50, 16)


def build(name, fused):
    from fastmot_amd.models import ReID
    from fastmot_amd.models.graph import RandomWeights
    os.environ['FASTMOT_CONVIN'] = '1' if fused else '0'
    try:
        g, _ = ReID.get_model(name).build_graph(RandomWeights(seed=1))
    finally:
        os.environ.pop('FASTMOT_CONVIN', None)
    return g


def tails(g):
    """[(block tail's name, [layer indices])]: the FM_OP_CONVIN layer, or the linear conv + FM_OP_INSTNORM pair."""
    from fastmot_amd.models import graph as G
    out = []
    for i, d in enumerate(g.layers):
        if d['op'] == G.OP_CONVIN:
            out.append((d['name'], [i]))
        elif d['op'] == G.OP_INSTNORM and i > 1 and g.layers[i - 1]['out'].tid == d['ins'][0].tid and g.layers[i - 1]['op'] in G.CONV_OPS \
                and d['name'] != 'conv1.IN':
            out.append((g.layers[i - 1]['name'], [i - 1, i]))
    return out


def passes(ctx, lines, turns=4, per_turn=10):
    from fastmot_amd.engine import HipNet, NET_EXTRACTOR
    x = np.random.default_rng(0).normal(0, 1, (max(BATCHES), 256, 128, 3)).astype(np.float16)
    forms = [('OSNetAIN10', True), ('OSNetAIN10', False), ('OSNetIBN10', True), ('OSNetIBN10', False), ('OSNet10', True)]
    wall = {(f, b): [] for f in forms for b in BATCHES}
    per_layer = {}
    for turn in range(turns):
        for form in forms:
            name, fused = form
            g = build(name, fused)
            ctx.feat_configure(512)
            net = HipNet(ctx, NET_EXTRACTOR, g, max(BATCHES), reuse_buffers=True)
            try:
                net.write(g.input, x)
                for b in BATCHES:
                    for _ in range(3):
                        net.run(b)
                        net.read_embeddings(b)
                    for _ in range(per_turn):
                        t0 = time.perf_counter()
                        net.run(b)
                        net.read_embeddings(b)
                        wall[form, b].append((time.perf_counter() - t0) * 1e3)
                    if turn == 0 and name != 'OSNet10':
                        per = net.profile_layers(b, iters=10) * 1e3
                        per_layer[form, b] = (float(per.sum()), [(n, [float(per[i]) for i in idx]) for n, idx in tails(g)], len(g.layers))
            finally:
                net.close()

    def label(form):
        return f'{form[0]} {"fused (FM_OP_CONVIN)" if form[1] else "FASTMOT_CONVIN=0"}' if form[0] != 'OSNet10' else 'OSNet10'
    for b in BATCHES:
        for form in forms:
            w = wall[form, b]
            lines.append(f'{label(form)}, batch {b}: run + read-back {statistics.median(w):.3f} ms wall (median of {len(w)}; min {min(w):.3f}, '
                         f'max {max(w):.3f}), {statistics.median(w) / b * 1e3:.1f} us per crop')
    verdict = {}
    for name in ('OSNetAIN10', 'OSNetIBN10'):
        for b in BATCHES:
            f, u = statistics.median(wall[(name, True), b]), statistics.median(wall[(name, False), b])
            verdict[name, b] = f <= u
            lines.append(f'{name} batch {b}: fused / unfused = {f:.3f} / {u:.3f} ms = {f / u:.3f} '
                         f'({"fused is not slower" if f <= u else "fused is SLOWER"})')
    for (form, b), (total, ts, n) in sorted(per_layer.items(), key=lambda kv: (kv[0][0][0], -kv[0][1], not kv[0][0][1])):
        lines.append(f'{label(form)}, batch {b}: {n} layers, per-layer events sum {total / 1e3:.3f} ms; tails: ' +
                     '; '.join(f'{n_} ' + ' + '.join(f'{t:.1f}' for t in t_) + (f' = {sum(t_):.1f}' if len(t_) > 1 else '') + ' us' for n_, t_ in ts))
    return verdict


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
    lines.append('# scripts/reid_ain_timing.py: OSNet-AIN / OSNet-IBN, the fused block tail (FM_OP_CONVIN) against FASTMOT_CONVIN=0, '
                 '256 x 128 crops; one MI355X, one call')
    ok = True
    if args.parent_tree:       # (first, in fresh processes: this process has not touched the GPU yet)
        ok = bench_ab(args.parent_tree, args.steps, args.warmup, args.rounds, lines)
    else:
        lines.append('bench.py default against the parent: not measured (no --parent-tree)')
    from fastmot_amd.runtime import get_context
    ctx = get_context()
    verdict = passes(ctx, lines)
    ctx.feat_configure(512)
    lines.append('default form: ' + ('fused (no pass slower)' if all(verdict.values()) else
                                     'see the ratios above: ' + ', '.join(f'{n} batch {b} {"fused" if v else "unfused"}' for (n, b), v in verdict.items())))
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
