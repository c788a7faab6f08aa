"""Detector look-ahead: frames/s of the config[1] workload with MOT(detector_lookahead=1) and =2, alternating in one
process, and the stand-alone detector pass at batch 1 and 2 (fm_net_profile), total and per frame.

Uses bench.py's workload as it is (tracker_cfg, build_mot, the InjectedYOLODetector of tests/synthetic.py).  The
look-ahead run hands each step its next two frames (MOT.step(frame, next_frames=...)); the default run hands the next
frame (next_frame=..., the bench's pipelined mode).  The stand-alone figures are fm_net_profile's per-pass sums of
launch times (every layer synchronised), the batch-2 pass with the batch-1 reduction-order choices it runs with.

    python scripts/lookahead_rate.py [--steps 300] [--rounds 3] [--out profiles/lookahead_rate.txt]"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(1, str(ROOT / 'tests'))

import bench  # noqa: E402


def build(cfg, video, lookahead):
    import fastmot_amd.mot as mot_mod
    orig = mot_mod.MOT

    def mot_with_lookahead(*a, **kw):
        return orig(*a, detector_lookahead=lookahead, **kw)
    mot_mod.MOT = mot_with_lookahead
    try:
        return bench.build_mot(cfg, video)
    finally:
        mot_mod.MOT = orig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--warmup', type=int, default=60)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from fastmot_amd import Track, models
    from fastmot_amd.runtime import get_context
    from synthetic import SyntheticVideo
    models.allow_random_weights()
    ctx = get_context()
    cfg = bench.CONFIGS[1]
    size = cfg['size']
    video = SyntheticVideo(size, n_ids=cfg['n_dets'], n_frames=bench.RING, seed=100)
    ctx.frame_configure(size[0], size[1], bench.RING)
    host = ctx.pinned_frames(bench.RING)
    for i, fr in enumerate(video.frames):
        host[i] = fr
    frames = [host[i] for i in range(bench.RING)]
    lines = [f'# scripts/lookahead_rate.py, {cfg["name"]}: {cfg["desc"]}; pinned host frames, {args.steps} timed steps '
             f'after {args.warmup}, {args.rounds} alternating rounds']

    def run(mot, k, n, start):
        for s in range(start, start + n):
            i = bench.ping_pong(s, bench.RING)
            mot.detector._frame_idx = i
            nxt = [frames[bench.ping_pong(s + j, bench.RING)] for j in range(1, k + 1)]
            if k > 1:
                mot.step(frames[i], next_frames=nxt)
            else:
                mot.step(frames[i], next_frame=nxt[0])

    rates = {1: [], 2: []}
    for r in range(args.rounds):
        for k in (1, 2):
            mot = build(cfg, video, k)
            Track._count = 0
            mot.reset(1 / 30.)
            run(mot, k, args.warmup, 0)
            ctx.synchronize()
            t0 = time.perf_counter()
            run(mot, k, args.steps, args.warmup)
            ctx.synchronize()
            dt = time.perf_counter() - t0
            rates[k].append(args.steps / dt)
            lines.append(f'round {r} detector_lookahead={k}: {args.steps / dt:.1f} frames/s')
            mot.tracker._clear_tracks()
            del mot
    for k in (1, 2):
        lines.append(f'detector_lookahead={k}: median {sorted(rates[k])[len(rates[k]) // 2]:.1f} frames/s '
                     f'(runs {", ".join(f"{x:.1f}" for x in rates[k])})')
    # stand-alone detector pass (fm_net_profile: the layer sequence alone, every launch synchronised)
    mot = build(cfg, video, 2)
    net = mot.detector.backend
    for b in (1, 2):
        p = [net.profile(b, iters=20) for _ in range(3)]
        ms = sorted(q['conv_ms'] + q['other_ms'] for q in p)[1]
        lines.append(f'stand-alone detector pass batch {b}: {ms:.3f} ms ({ms / b:.3f} ms per frame; '
                     f'{p[0]["n_conv"] + p[0]["n_other"]} launches; median of 3 x 20)')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    print(json.dumps({'fps_lookahead1': rates[1], 'fps_lookahead2': rates[2]}))
    if args.out:
        Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
