"""Shapes of the conv-engine unit tests, shared by tests/test_conv_gpu.py (the device) and tests/test_layer_bound_host.py
(CPU: the per-element bound has to bite at exactly these shapes), and `table`: the one-layer network of a case as the GPU
test builds it, with the same seeds."""
import numpy as np
import torch

from fastmot_amd.models.graph import Graph, RandomWeights, RES_BEFORE_ACT

# test_single_conv: (cin, cout, k, stride, act, h, w, n)
SINGLE_CONV = [
    (8, 32, 3, 1, 'mish', 20, 24, 1),       # stem-like
    (64, 64, 1, 1, 'leaky', 19, 19, 1),
    (32, 64, 3, 2, 'mish', 38, 38, 1),      # downsample
    (128, 255, 1, 1, 'linear', 13, 13, 1),  # head-like, ragged cout
    (256, 512, 3, 1, 'leaky', 19, 19, 1),   # big K
    (16, 16, 1, 1, 'relu', 64, 32, 5),      # OSNet x0.25 pointwise, batch
    (24, 96, 1, 1, 'relu', 16, 8, 7),
    (8, 16, 7, 2, 'relu', 64, 32, 3),       # OSNet conv1 (7x7 s2 p3)
    (512, 128, 1, 1, 'swish', 9, 11, 2),
    (64, 128, 3, 2, 'mish', 37, 51, 2),     # stride 2 over an odd map: no padding tap on the far border
    (8, 16, 7, 2, 'relu', 63, 31, 2),
]

# test_streamed_conv: (cin, cout, k, stride, act, h, w, n, extra)
STREAMED_CONV = [
    (512, 1024, 3, 1, 'leaky', 19, 19, 1, ''),      # 2 cout tiles per workgroup, 8 waves
    (1024, 255, 1, 1, 'linear', 19, 19, 2, 'f32'),  # YOLO head: ragged cout, fp32 output, batch
    (256, 512, 3, 2, 'leaky', 38, 38, 1, ''),       # stride-2 downsample into the 19 x 19 level
    (512, 512, 1, 1, 'mish', 19, 19, 1, 'res'),     # shortcut after the activation
    (512, 256, 1, 1, 'leaky', 19, 19, 1, 'up'),     # fused nearest x2 upsample into a concat slice
    (128, 64, 3, 1, 'relu', 7, 5, 3, 'res'),        # 1 cout tile per workgroup, ragged pixel tile, batch
    (64, 40, 3, 1, 'swish', 9, 9, 1, ''),           # 4 waves (K = 576: 9 chunks), cout padded to 64
    (2048, 512, 1, 1, 'leaky', 19, 19, 1, ''),
    (64, 128, 3, 2, 'mish', 37, 51, 2, ''),         # stride 2 over an odd map
]

# test_stem_conv: (cin, cout, k, stride, act, h, w, n)
STEM_CONV = [
    (3, 32, 3, 1, 'mish', 40, 37, 1),        # YOLOv4 layer 0
    (3, 16, 7, 2, 'relu', 64, 32, 3),        # OSNet conv1
    (3, 64, 7, 2, 'relu', 32, 16, 1),        # OSNet x1.0 conv1: cout > 32 -> generic kernel
    (4, 24, 3, 2, 'leaky', 33, 18, 2),
    (1, 8, 3, 1, 'linear', 16, 16, 1),
]

# test_convd_conv: (cin, cout, k, stride, act, h, w, n, extra)
CONVD_SHAPES = [
    (64, 128, 1, 1, 'mish', 76, 76, 1, ''),            # CSP stage entry
    (64, 64, 1, 1, 'mish', 48, 40, 1, 'slice'),        # reads a channel slice, writes a concat slice
    (128, 64, 1, 1, 'mish', 35, 35, 1, ''),            # ragged last pixel tile
    (128, 128, 1, 1, 'leaky', 32, 32, 2, ''),          # batch 2
    (256, 255, 1, 1, 'linear', 38, 38, 1, 'f32'),      # head: ragged cout, fp32 output
    (128, 255, 1, 1, 'logistic', 20, 20, 1, 'f32'),    # NEW_COORDS head
    (512, 256, 1, 1, 'leaky', 19, 19, 1, 'up'),        # fused nearest x2 upsample into a concat slice
    (512, 512, 1, 1, 'mish', 19, 19, 1, 'res'),        # shortcut after the activation
    (2048, 512, 1, 1, 'leaky', 19, 19, 1, ''),         # 32 K steps
    (128, 256, 3, 1, 'leaky', 38, 38, 1, ''),          # 3x3, padding on every border
    (64, 128, 3, 2, 'mish', 76, 76, 1, ''),            # stride-2 downsample, 9 K steps (odd: two steps per barrier repeat one)
    (256, 512, 3, 2, 'leaky', 38, 38, 1, ''),
    (512, 1024, 3, 1, 'leaky', 19, 19, 1, ''),         # 72 K steps
    (128, 64, 3, 1, 'relu', 7, 5, 3, 'res'),           # tiny maps, batch, shortcut
    (64, 40, 3, 1, 'swish', 9, 9, 1, ''),              # cout padded to 64
    (192, 96, 3, 1, 'relu', 16, 8, 4, 'resb'),         # cin = 3 * 64: a tap is three K steps; shortcut BEFORE the activation
    (16, 64, 1, 1, 'relu', 64, 32, 5, ''),             # OSNet x0.25 pointwise convs: cin % 64 != 0 (K zero-padded to a step,
    (96, 24, 1, 1, 'relu', 16, 8, 7, 'resb'),          #   chunks beyond the pixel's channels not fetched), batch
    (24, 96, 1, 1, 'linear', 32, 16, 3, 'slice'),
    (64, 128, 3, 2, 'mish', 37, 51, 2, ''),            # stride 2 over an odd map, batch 2
]
# forced configurations (bm, bn, K groups, ring slots, loader waves, steps per barrier); every shape runs the launcher's own
# choice and three of them (a different three per shape: every pairing of a shape class with a code path occurs)
CONVD_CFGS = [(128, 128, 1, 0, 1), (128, 64, 2, 0, 1), (128, 64, 1, 2, 0), (64, 64, 4), (64, 64, 1, 3, 1), (64, 64, 2, 0, 0),
              (128, 128, 2, 2, 1), (64, 64, 2, 2, 1, 2), (128, 64, 1, 3, 1, 2), (64, 64, 1, 0, 0, 2)]

PLAIN_CASES = ([('single', c) for c in SINGLE_CONV] + [('streamed', c) for c in STREAMED_CONV] +
               [('stem', c) for c in STEM_CONV] + [('convd', c) for c in CONVD_SHAPES])


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).transpose(0, 3, 1, 2)))


def table(kind, case):
    """-> (graph, fp16 NHWC input, index of the conv under test) of one PLAIN_CASES entry.  Which of the conv kernels the
    table selects is left at the builder's default: they share one reference (torch_ref.run_layer)."""
    cin, cout, k, stride, act, h, w, n = case[:8]
    extra = case[8] if len(case) > 8 else ''
    if kind == 'single':
        x = np.random.default_rng(cin * 1000 + cout).normal(0, 1, (n, h, w, cin)).astype(np.float16)
        g = Graph(RandomWeights(seed=cin + cout + k), (h, w), cin)
        g.conv('c', g.input, cout, k, stride, act, pad=3 if k == 7 else None)
    elif kind == 'stem':
        x = np.random.default_rng(cin + cout).normal(0, 1, (n, h, w, cin)).astype(np.float16)
        g = Graph(RandomWeights(seed=k + cout), (h, w), cin)
        g.conv('c', g.input, cout, k, stride, act, pad=3 if k == 7 else None)
    else:
        sl, guard = extra == 'slice', 16 if kind == 'streamed' else 64
        x = np.random.default_rng(cin + cout + (h if kind == 'convd' else 0)).normal(0, 1, (n, h, w, cin + (64 if sl else 0))).astype(np.float16)
        g = Graph(RandomWeights(seed=cin + 3 * cout + k), (h, w), x.shape[-1])
        src = g.input.slice(64, cin) if sl else g.input
        ho = (h + 2 * (k // 2) - k) // stride + 1
        wo = (w + 2 * (k // 2) - k) // stride + 1
        up = 2 if extra == 'up' else 1
        wide = g.new(ho * up, wo * up, cout + guard, f32=extra == 'f32')
        res = g.conv('r', src, cout, 1, stride, 'linear') if extra in ('res', 'resb') else None
        g.conv('c', src, cout, k, stride, act, dst=wide.slice(guard, cout), res=res, up=up, f32_out=extra == 'f32',
               res_mode=RES_BEFORE_ACT if extra == 'resb' else 1, bn=kind == 'streamed' or extra != 'f32')
    return g, x, len(g.layers) - 1
