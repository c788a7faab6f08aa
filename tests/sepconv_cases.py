"""Shapes and inputs shared by tests/test_sepconv_host.py (CPU) and tests/test_sepconv_gpu.py."""
import numpy as np
import torch

from fastmot_amd.models.graph import Graph, RandomWeights

# (N, H, W, cin, cout, stride)
SHAPES = [
    (1, 5, 7, 32, 64, 1),          # map smaller than a tile
    (1, 6, 8, 64, 128, 2),         # pad (0, 1)
    (1, 7, 5, 128, 128, 2),        # pad (1, 1)
    (3, 5, 5, 32, 64, 1),          # tile across samples
    (1, 9, 9, 24, 48, 1),          # cin % 32 != 0
    (1, 19, 19, 512, 512, 1),
    (1, 19, 19, 512, 1024, 2),
    (1, 3, 3, 1024, 1024, 1),
    (1, 150, 150, 32, 64, 1),
]
IDS = ['x'.join(map(str, s)) for s in SHAPES]


def build(shape, fused):
    """-> (graph, output view) of a one-block network with seeded parameters (the same in both forms)."""
    n, h, w, cin, cout, stride = shape
    g = Graph(RandomWeights(seed=cin + 7 * cout + stride), (h, w), cin)
    g.use_sepconv = fused
    y = g.sepconv('dw', 'pw', g.input, cout, stride)
    return g, y


def block_input(shape):
    """fp16 NHWC input, scaled (sigma 8) so that the depthwise stage leaves ReLU6's linear range on both sides."""
    n, h, w, cin, cout, stride = shape
    rng = np.random.default_rng(1000 * cin + cout + h)
    return rng.normal(0, 8, (n, h, w, cin)).astype(np.float16)


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).transpose(0, 3, 1, 2)))


def assert_leaves_linear_range(pre):
    """pre: the depthwise stage BEFORE its activation, on the reference alone."""
    hi, lo = float((pre > 6).double().mean()), float((pre < 0).double().mean())
    assert hi >= 0.10 and lo >= 0.10, (hi, lo)


def max_order_flips(numel, k):
    """How many of `numel` fp16 outputs two CORRECT evaluations of a K-term fp32 reduction may differ in when they sum in
    different orders -- the fused kernel walks K in 16-wide steps in one accumulator, the unfused
    pointwise conv of the large-K shapes splits K across wave groups.  The two fp32 sums differ by about sqrt(K) u32 |y|
    (u32 = 2^-24, a random walk of K roundings); the fp16 rounding flips when a rounding boundary (spacing 2^-10 |y|) lies
    between them: a fraction of about sqrt(K) 2^-14 of the outputs.  Four times that is allowed: sqrt(K) 2^-12 (0.55 % at
    K = 512, 0.78 % at 1024).  A depthwise intermediate that is not rounded to fp16, or rounded differently, changes about
    15 % of the outputs (tests/test_sepconv_host.py asserts that on the host stand-in)."""
    return numel * (k ** 0.5) * 2.0 ** -12
