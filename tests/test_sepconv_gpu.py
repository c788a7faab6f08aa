"""GPU: FM_OP_DWCONV (ops.hip) and FM_OP_SEPCONV (sepconv.hip) as one-layer networks against the float64 restatement of
tests/ssd_ref.py fed the device's fp16 inputs, under the per-element bound of DESIGN.md section 7 (for the fused op
composed from its two stages), and fused against unfused on the same input.  Shapes: tests/sepconv_cases.py."""
import numpy as np
import pytest
import torch

import ssd_ref
import torch_ref as T
from fastmot_amd.engine import HipNet, NET_DETECTOR
from fastmot_amd.models import graph as G
from sepconv_cases import IDS, SHAPES, assert_leaves_linear_range, block_input, build, max_order_flips, nchw

pytestmark = pytest.mark.gpu


def _run(ctx, g, x, views):
    net = HipNet(ctx, NET_DETECTOR, g, x.shape[0])
    net.write(g.input, x)
    net.run(x.shape[0])
    outs = [nchw(net.read(v, x.shape[0])) for v in views]
    net.close()
    return outs


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_dwconv_and_sepconv(ctx, shape):
    x = block_input(shape)
    xt = nchw(x)
    gf, yf = build(shape, True)
    gu, yu = build(shape, False)
    assert [d['op'] for d in gf.layers] == [G.OP_SEPCONV] and gu.layers[0]['op'] == G.OP_DWCONV and len(gu.layers) == 2
    d = gf.layers[0]
    wd, bd, a1, wp, bp = d['sep_ref']
    ref, bound, _ = ssd_ref.sep_block(xt, d['sep_ref'], d['act'], d['stride'])
    assert_leaves_linear_range(ssd_ref.conv_stage(xt.double(), 0.0, wd, bd, 0, 3, d['stride'], groups=xt.shape[1], track=False)[0])

    (fused,) = _run(ctx, gf, x, [yf])
    t_dev, unfused = _run(ctx, gu, x, [gu.layers[0]['out'], yu])

    # the unfused yardstick, layer by layer: FM_OP_DWCONV from the input, the pointwise conv from the device's depthwise tensor
    tref, tbound = ssd_ref.dw_layer(xt, wd, bd, a1, d['stride'])
    r_dw = T.check_layer(t_dev, tref, tbound, f'FM_OP_DWCONV {shape}')
    ref2, bound2 = ssd_ref.pw_layer(t_dev, wp, bp, d['act'])
    r_pw = T.check_layer(unfused, ref2, bound2, f'pointwise conv behind FM_OP_DWCONV {shape}')
    # the fused op under the bound composed from its two stages; the unfused pair's result under the same bound
    r_f = T.check_layer(fused, ref, bound, f'FM_OP_SEPCONV {shape}')
    r_u = T.check_layer(unfused, ref, bound, f'FM_OP_DWCONV + conv against the composed bound {shape}')
    # ... and under the second stage's bound alone, fed the depthwise tensor the unfused launch stored: holds when the fused
    # kernel rounds the same depthwise values to fp16 (what sees an unrounded intermediate, tests/test_sepconv_host.py)
    r_f2 = T.check_layer(fused, ref2, bound2, f'FM_OP_SEPCONV, second stage from the stored depthwise tensor {shape}')
    equal = bool(torch.equal(fused, unfused))
    diff = float((fused - unfused).abs().max())
    print(f'{shape}: err / bound dw {r_dw:.3g}, pw {r_pw:.3g}, fused {r_f:.3g} (second stage {r_f2:.3g}), unfused {r_u:.3g}; '
          f'fused == unfused: {equal} (max |diff| {diff:.3g}, {int((fused != unfused).sum())} of {fused.numel()} elements)')
    # fused against unfused on the same input, under the same bound
    T.check_layer(fused, unfused, bound, f'FM_OP_SEPCONV against FM_OP_DWCONV + conv {shape}')
    cin = shape[3]
    if cin <= 128:
        # one K chunk and one accumulator per output in both kernels, the same fmaf chain in the depthwise stage: bit for
        # bit -- the sharpest check that the LDS intermediate is rounded exactly as the unfused pair stores it (a wrong
        # rounding or another tap order fails here at once)
        assert equal, f'{shape}: {int((fused != unfused).sum())} of {fused.numel()} elements differ, max |diff| {diff:.3g}'
    else:
        # the pair's pointwise conv splits K across wave groups: another fp32 summation order, which may flip the fp16
        # rounding of a few outputs (sepconv_cases.max_order_flips); an unrounded intermediate changes ~15 %.  How far a
        # differing pair may lie apart is the bound asserted above: one fp16 ulp where the output is large, the two sums'
        # own difference where ReLU6 follows a sum that nearly cancels (a tiny output, whose ulp is smaller than that)
        differ = fused != unfused
        n_diff, cap = int(differ.sum()), max_order_flips(fused.numel(), cin)
        assert n_diff <= cap, f'{shape}: {n_diff} elements differ, more than two summation orders explain ({cap:.0f})'
        assert diff <= 2.0 ** -8, diff            # (one fp16 ulp of the top binade of ReLU6's range, [4, 6])
