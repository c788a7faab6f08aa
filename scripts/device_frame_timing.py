"""Ingest of frames that already lie in GPU memory (DeviceArrayFrame) against the host uploads beside it, on one 1920x1080
frame in one process, three alternating rounds of `--iters` with medians: frame_upload_ahead(1, frame) +
frame_promote_next() + a device synchronise for host BGR and host NV12 from page-locked memory (the yardsticks) and for
torch tensors on the device as BGR-HWC uint8, RGB-CHW uint8, RGB-CHW float16 and NV12 -- host-visible time (host clock
around the three calls), HIP-event time of the work on the look-ahead slot's stream (the library's trace marks
30 .. 31) and the conversion kernel alone (marks 36 .. 31 for host NV12; 59 .. 60 for the device kinds, whose
source-consumed event is recorded between 60 and 31).  The device frames are handed over as a pipeline would (not
`ready`: an event is recorded on the producer's stream, the null stream here, and waited for unless it is complete
already); BGR-HWC is also timed with `ready=True`.  No byte of a device frame crosses PCIe and no host copy is made.

    python scripts/device_frame_timing.py [--iters 100] [--rounds 3] [--out profiles/device_ingest.txt]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch          # before the library is loaded: one HIP runtime in the process (see DeviceArrayFrame)

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SIZE = (1920, 1080)
# bytes per pixel the conversion kernel reads; the host kinds cross PCIe with as many
BYTES_PER_PIXEL = {'host BGR': 3, 'host NV12': 1.5, 'device BGR-HWC': 3, 'device BGR-HWC ready': 3, 'device RGB-CHW u8': 3,
                   'device RGB-CHW f16': 6, 'device NV12': 1.5}
KERNEL_MARK = {'host NV12': (36, 31), 'device BGR-HWC': (59, 60), 'device BGR-HWC ready': (59, 60), 'device RGB-CHW u8': (59, 60),
               'device RGB-CHW f16': (59, 60), 'device NV12': (59, 60)}


def med(x):
    return float(np.median(x)) if len(x) else float('nan')


def rounds(x, scale=1., fmt='.3f'):
    return ', '.join(format(v * scale, fmt) for v in x)


def intervals(tags, ms, a, b):
    """Durations from each mark `a` to the next mark `b`."""
    out, t0 = [], None
    for t, m in zip(tags, ms):
        if t == a:
            t0 = m
        elif t == b and t0 is not None:
            out.append(m - t0)
            t0 = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from fastmot_amd import DeviceArrayFrame
    from fastmot_amd.runtime import get_context
    from fastmot_amd.utils import devarray
    if not torch.cuda.is_available():
        raise RuntimeError('no GPU: this script measures, it does not estimate')
    ctx = get_context()
    dev = torch.device('cuda', ctx.device)
    w, h = SIZE
    rng = np.random.default_rng(0)
    ctx.frame_configure(w, h, 0)
    bgr = ctx.pinned_frames(2)
    bgr[...] = rng.integers(0, 256, bgr.shape, dtype=np.uint8)
    nv = ctx.pinned_nv12_frames(2)
    for f in nv:
        f.y[...] = rng.integers(0, 256, f.y.shape, dtype=np.uint8)
        f.uv[...] = rng.integers(0, 256, f.uv.shape, dtype=np.uint8)
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    chw = [np.ascontiguousarray(f[..., ::-1].transpose(2, 0, 1)) for f in bgr]
    f16 = [(c / 255.).astype(np.float16) for c in chw]
    host_of = {'device BGR-HWC': [(f, dict(order='bgr')) for f in bgr], 'device RGB-CHW u8': [(c, dict(order='rgb')) for c in chw],
               'device RGB-CHW f16': [(c, dict(order='rgb')) for c in f16]}
    sources = {'host BGR': [bgr[0], bgr[1]], 'host NV12': nv}
    for kind, pairs in host_of.items():
        sources[kind] = [DeviceArrayFrame(put(a), **kw) for a, kw in pairs]
    sources['device BGR-HWC ready'] = [DeviceArrayFrame(f.array, 'bgr', ready=True) for f in sources['device BGR-HWC']]
    sources['device NV12'] = [DeviceArrayFrame.nv12(put(f.y), put(f.uv)) for f in nv]
    torch.cuda.synchronize(dev)
    res = {k: {'host': [], 'event': [], 'kernel': []} for k in sources}
    for _ in range(args.rounds):
        for kind, frames in sources.items():
            for i in range(20):                                # warm-up: first launch, events
                ctx.frame_upload_ahead(1, frames[i & 1])
                ctx.frame_promote_next()
            ctx.synchronize()
            ctx.trace_start(5 * args.iters + 16)
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
            if kind in KERNEL_MARK:
                res[kind]['kernel'].append(med(intervals(tags, ms, *KERNEL_MARK[kind])))
    # what was timed is the conversion the tests pin
    for kind, pairs in host_of.items():
        ctx.frame_upload_ahead(1, sources[kind][0])
        ctx.frame_promote_next()
        assert np.array_equal(ctx.frame_read(), devarray.to_bgr(pairs[0][0], **pairs[0][1])), kind
    ctx.frame_upload_ahead(1, sources['device NV12'][0])
    ctx.frame_promote_next()
    assert np.array_equal(ctx.frame_read(), devarray.to_bgr((nv[0].y, nv[0].uv)))
    assert ctx.pending_device_frames() == []
    lines = [f'# scripts/device_frame_timing.py: {ctx.device_info()["arch"]}; {w}x{h}, host sources page-locked, device sources contiguous torch '
             f'tensors, medians of {args.iters} per round, {args.rounds} alternating rounds']
    for kind, r in res.items():
        pcie = w * h * BYTES_PER_PIXEL[kind] if kind.startswith('host') else 0
        lines.append(f'{kind:21s} upload_ahead + promote + synchronise: host-visible {med(r["host"]):.3f} ms (rounds {rounds(r["host"])}); '
                     f'slot-stream events {med(r["event"]):.3f} ms (rounds {rounds(r["event"])}); {pcie / 1e6:.2f} MB over PCIe')
    for kind in KERNEL_MARK:
        k = res[kind]['kernel']
        moved = (BYTES_PER_PIXEL[kind] + 3) * w * h
        lines.append(f'{kind:21s} conversion kernel alone (events {KERNEL_MARK[kind][0]} .. {KERNEL_MARK[kind][1]}): {med(k) * 1e3:.1f} us (rounds {rounds(k, 1e3, ".1f")}); '
                     f'{BYTES_PER_PIXEL[kind] + 3:g} B/px = {moved / 1e6:.2f} MB -> {moved / 1e9 / (med(k) * 1e-3):.0f} GB/s '
                     '(event pairs around one short kernel also time the launch gap)')
    lines.append("(a trace mark is a timed event on the stream it marks: the 30 .. 31 interval of a device kind holds two of its own, 59 and 60, host NV12's one, host BGR's none)")
    # the detour a device frame took before: device -> host, then the host upload above
    t = sources['device BGR-HWC'][0].array
    down = []
    for _ in range(20):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        t.cpu()
        down.append((time.perf_counter() - t0) * 1e3)
    lines.append(f'host, per frame, without this path: `tensor.cpu()` of the BGR-HWC frame {med(down):.3f} ms (pageable destination), then the host BGR '
                 'upload above')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    print(json.dumps({kind: {m: med(v) for m, v in r.items() if v} for kind, r in res.items()}))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
