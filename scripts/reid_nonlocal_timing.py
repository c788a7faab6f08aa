"""fast-reid's non-local blocks (models/onnx_graph.py: FM_OP_NONLOCAL, csrc/nonlocal.hip): what they cost on one MI355X,
everything inside ONE call, seeded weights, HIP-event times, medians of 40 samples, variants alternating:

  1. with --parent-tree DIR (a built checkout of the parent commit): the default bench.py line of this tree against the
     parent's, alternating rounds (the default line runs OSNet: none of the new code)
  2. FM_OP_NONLOCAL alone at (C, H x W) = (512, 32 x 16) and (1024, 16 x 8), batch 16 and 50, beside two yardsticks that are
     not the code under test: the time its bytes (one read and one write of the view, 2 * N * HW * C * 2) take at the
     achievable HBM rate of 6.3 TB/s, and FM_OP_INSTNORM over the same view in the same loop (same traffic shape, existing
     kernel); the two ops alternate, twice each
  3. a ResNet-50-nl pass (non-local blocks behind blocks 2, 3 of layer2 and 3, 4, 5 of layer3: fast-reid's WITH_NL) beside the
     plain ResNet-50 pass of profiles/reid_resnet.txt (256 x 128 crops) at batch 16 and 50: the two networks are created in
     turn, four times each, ten samples per turn

    python scripts/reid_nonlocal_timing.py [--parent-tree DIR] [--out profiles/reid_nonlocal.txt]"""
import argparse
import statistics
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(HERE))
sys.path.insert(1, str(HERE / 'tests'))
sys.path.insert(2, str(HERE / 'scripts'))

import numpy as np  # noqa: E402

from reid_ibn_timing import HBM, SAMPLES, network_passes, one_layer_times  # noqa: E402


def nonlocal_alone(ctx, batches, lines):
    import nonlocal_ref as NL
    from fastmot_amd.models import graph as G
    rng = np.random.default_rng(3)
    for label, c, hw in (('layer2 of a 256 x 128 crop', 512, (32, 16)), ('layer3 of a 256 x 128 crop', 1024, (16, 8))):
        x = rng.normal(0, 1, (max(batches),) + hw + (c,)).astype(np.float16)
        res = {}
        for turn in range(2):       # (nonlocal, instnorm, and again: alternating)
            g, _ = NL.make_case(1, hw[0], hw[1], c)
            for b, t in one_layer_times(ctx, g, 0, x, batches, samples=SAMPLES // 2).items():
                res.setdefault(('FM_OP_NONLOCAL', b), []).append(t)
            g = G.Graph(None, hw, c)
            dst = g.instnorm('in', g.input, rng.uniform(0.5, 1.5, c), rng.normal(0, 0.3, c), 1e-5, 'linear')
            g.outputs = [dst]
            for b, t in one_layer_times(ctx, g, 0, x, batches, samples=SAMPLES // 2).items():
                res.setdefault(('FM_OP_INSTNORM', b), []).append(t)
        for b in batches:
            nbytes = 2.0 * b * hw[0] * hw[1] * c * 2
            floor = nbytes / HBM * 1e6
            nl, inorm = (statistics.mean(res[k, b]) for k in ('FM_OP_NONLOCAL', 'FM_OP_INSTNORM'))
            lines.append(f'non-local block alone, {label}, C {c} over {hw[0]} x {hw[1]}, batch {b}: {nl:.2f} us for {nbytes / 1e6:.2f} MB '
                         f'({floor:.2f} us at 6.3 TB/s: x{nl / floor:.1f}, {nbytes / nl / 1e6:.2f} TB/s; {b} samples, at most 4 workgroups '
                         f'each, on 256 CUs); FM_OP_INSTNORM over the same view: {inorm:.2f} us (x{nl / inorm:.2f})')


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
    lines.append('# scripts/reid_nonlocal_timing.py: fast-reid non-local blocks (FM_OP_NONLOCAL), 256 x 128 crops; one MI355X, one call')
    ok = True
    if args.parent_tree:       # (first, in fresh processes: this process has not touched the GPU yet)
        ok = bench_ab(args.parent_tree, args.steps, args.warmup, args.rounds, lines)
    else:
        lines.append('bench.py default against the parent: not measured (no --parent-tree)')
    import nonlocal_ref as NL
    import resnet_ref as R
    from fastmot_amd.runtime import get_context
    ctx = get_context()
    batches = (16, 50)
    nonlocal_alone(ctx, batches, lines)
    files = {'ResNet-50': R.export(R.resnet50(head='bnneck'), hw=(256, 128)),
             'ResNet-50-nl': NL.export(NL.resnet50_nl(head='bnneck'), hw=(256, 128))}
    network_passes(ctx, files, batches, lines)
    ctx.feat_configure(512)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
