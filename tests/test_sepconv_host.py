"""CPU: the separable block's layer-table entries, the kernel's shape predicate, and planted mistakes.

A torch restatement of one separable block (tests/ssd_ref.sep_block) in fp32 with fp16-rounded storage stands in for the
device.  Clean, it stays within the DESIGN section 7 per-element bound composed from the block's two stages; given one
of the mistakes a kernel author makes here -- symmetric padding at an even input, ReLU instead of ReLU6, the depthwise
result left unrounded in fp32 -- it must exceed the bound at the shapes tests/test_sepconv_gpu.py runs: the GPU test
can see those faults.

The unrounded intermediate is the one fault the COMPOSED bound cannot see at any shape: the float64 reference does not
round the intermediate either, so leaving it unrounded moves the result towards the reference (measured err / bound
0.07 .. 0.43, below the clean stand-in's 0.08 .. 0.58).  It is therefore judged against the second stage alone: the
reference W_pw . t + b_pw fed the fp16 intermediate t "exactly as the unfused pair would store it", with the one-stage
bound (d_in = 0).  The fault then adds W_pw . (t32 - fp16(t32)), about sqrt(K) u16 |w t|, to an allowance of about
K^2 u32 |w t| + u16 |y|: it is outside the bound for K = cin <= 128 (measured 3.4 .. 34 times) and asserted there; for
cin = 512 and 1024 it is inside ANY bound that allows a correct fp32 accumulation (measured 0.68, 0.73, 0.32 against a
clean 0.54, 0.54, 0.25), which is printed.  What is asserted at every shape, those three included, is the check
tests/test_sepconv_gpu.py makes of the fused launch against the unfused pair on the same input: bit-equal for cin <= 128,
and for cin >= 512 at most sepconv_cases.max_order_flips outputs differing, within the composed bound (what two fp32 summation
orders explain: 0.55 % / 0.78 % of the outputs; measured on the device 0.04 %, 0.03 %, 0.08 %).  The unrounded
intermediate changes about 15 % of the outputs at every shape -- asserted here, on the stand-in, to be more than four
times the cap.  tests/test_sepconv_gpu.py also applies the second-stage check to the device, fed the depthwise tensor
the unfused FM_OP_DWCONV launch stored."""
import numpy as np
import pytest
import torch

import ssd_ref
import torch_ref as T
from fastmot_amd.models import graph as G
from fastmot_amd.models.graph import Graph, RandomWeights
from sepconv_cases import IDS, SHAPES, assert_leaves_linear_range, block_input, build, max_order_flips, nchw


def test_relu6_is_activation_6():
    assert G.ACT['relu6'] == 6 and (G.OP_DWCONV, G.OP_SEPCONV) == (21, 22)


def test_predicate_agrees_with_the_kernel():
    from fastmot_amd import _lib
    lib = _lib.load()
    for cin in (0, 4, 8, 12, 16, 24, 32, 36, 64, 96, 512, 1024, 2048, 2056, 4096):
        for cout in (0, 8, 20, 32, 48, 64, 255, 256, 1024, 2048, 2056):
            for stride in (0, 1, 2, 3):
                assert Graph.sepconv_supported(cin, cout, stride) == bool(lib.fm_sepconv_supported(cin, cout, stride)), (cin, cout, stride)


def test_fused_and_unfused_tables(monkeypatch):
    g1, y1 = build(SHAPES[1], True)
    g2, y2 = build(SHAPES[1], False)
    assert [d['op'] for d in g1.layers] == [G.OP_SEPCONV]
    assert [d['op'] for d in g2.layers][0] == G.OP_DWCONV and len(g2.layers) == 2 and g2.layers[1]['op'] in G.CONV_OPS
    assert (y1.h, y1.w, y1.c) == (y2.h, y2.w, y2.c) == (3, 4, 128)
    wd, bd, a1, wp, bp = g1.layers[0]['sep_ref']
    (_, wd2, bd2), (_, wp2, bp2) = g2.conv_params
    for a, b in ((wd, wd2), (bd, bd2), (wp, wp2), (bp, bp2)):
        assert np.array_equal(a, b)                      # both forms draw the same parameters in the same order
    assert g1.layers[0]['act'] == g1.layers[0]['gates'][0] == a1 == 6
    monkeypatch.setenv('FASTMOT_SEPCONV', '0')
    assert not Graph(RandomWeights(0), (4, 4), 8).use_sepconv
    # a shape the kernel does not run falls back to the pair
    g = Graph(RandomWeights(0), (4, 4), 12)
    g.sepconv('dw', 'pw', g.input, 16)
    assert [d['op'] for d in g.layers][0] == G.OP_DWCONV


def test_conv_same_padding():
    g = Graph(RandomWeights(0), (6, 8), 16)
    y = g.conv('a', g.input, 32, 3, 2, 'relu6', same=True)           # even: pad (0, 1) as pad 0 with ceil(in / 2) outputs
    assert (y.h, y.w, g.layers[-1]['pad']) == (3, 4, 0) and g.layers[-1]['op'] != G.OP_CONVD
    g = Graph(RandomWeights(0), (7, 5), 16)
    y = g.conv('a', g.input, 32, 3, 2, 'relu6', same=True)           # odd: (1, 1), the symmetric default
    assert (y.h, y.w, g.layers[-1]['pad']) == (4, 3, 1)
    g = Graph(RandomWeights(0), (6, 5), 16)                          # one axis each: the column padding travels in gates[0]
    y = g.conv('a', g.input, 32, 3, 2, 'relu6', same=True)
    assert (y.h, y.w, g.layers[-1]['pad'], g.layers[-1]['gates']) == (3, 3, 0, [1]) and g.layers[-1]['op'] in (G.OP_CONV, G.OP_CONVS)
    g = Graph(RandomWeights(0), (6, 8), 16)
    with pytest.raises(ValueError):                                  # (2, 3) padding of a 5x5 stride-2 window: not implemented
        g.conv('a', g.input, 32, 5, 2, 'relu6', same=True)
    assert g.conv('b', g.input, 32, 5, 1, 'relu6', same=True).h == 6
    g = Graph(RandomWeights(0), (6, 8), 16)
    assert g.conv('a', g.input, 32, 3, 2).h == 3 and g.layers[-1]['pad'] == 1      # the default is unchanged
    assert ssd_ref.same_pad(300, 3, 2) == (0, 1) and ssd_ref.same_pad(75, 3, 2) == (1, 1) and ssd_ref.same_pad(19, 3, 1) == (1, 1)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_clean_stand_in_within_bound_and_planted_mistakes_outside(shape):
    g, _ = build(shape, True)
    d = g.layers[0]
    x = nchw(block_input(shape))
    ref, bound, _ = ssd_ref.sep_block(x, d['sep_ref'], d['act'], d['stride'])
    pre = ssd_ref.conv_stage(x.double(), 0.0, d['sep_ref'][0], d['sep_ref'][1], 0, 3, d['stride'], groups=x.shape[1], track=False)[0]
    assert_leaves_linear_range(pre)
    clean = ssd_ref.sep_block(x, d['sep_ref'], d['act'], d['stride'], dt=torch.float32)[0]
    r = T.check_layer(clean, ref, bound, f'clean stand-in {shape}')
    print(f'{shape}: clean err / bound {r:.3g}')
    variants = ['relu'] + (['symmetric'] if shape[5] == 2 and shape[1] % 2 == 0 else [])
    for variant in variants:
        bad = ssd_ref.sep_block(x, d['sep_ref'], d['act'], d['stride'], variant=variant, dt=torch.float32)[0]
        with pytest.raises(AssertionError):
            T.check_layer(bad, ref, bound, f'{variant} {shape}')
    # the unrounded intermediate: second stage alone, fed the fp16 intermediate (module docstring)
    t16 = ssd_ref.sep_block(x, d['sep_ref'], d['act'], d['stride'], dt=torch.float32)[2].double()
    ref2, bound2 = ssd_ref.pw_layer(t16, d['sep_ref'][3], d['sep_ref'][4], d['act'])
    T.check_layer(clean, ref2, bound2, f'clean stand-in, second stage {shape}')
    bad = ssd_ref.sep_block(x, d['sep_ref'], d['act'], d['stride'], variant='unrounded', dt=torch.float32)[0].double()
    ratio = float(((bad - ref2).abs() / bound2).max())
    print(f'{shape}: unrounded intermediate, err / second-stage bound {ratio:.3g}')
    if shape[3] <= 128:
        assert ratio > 1.0, ratio
    # ... and at EVERY shape through the check the GPU test makes of the fused launch against the unfused pair: equal bit
    # for bit at cin <= 128, at most max_order_flips differing outputs above.  The fault changes far more than that
    n_diff = int((bad != clean.double()).sum())
    cap = max_order_flips(clean.numel(), shape[3])
    print(f'{shape}: unrounded intermediate changes {n_diff} of {clean.numel()} outputs; two summation orders explain {cap:.0f}')
    assert n_diff > 4 * cap and n_diff > 0.05 * clean.numel()
    # (the cap is not vacuous the other way: another summation order of the clean stand-in stays far below it)
    other = ssd_ref.sep_block(x.contiguous(memory_format=torch.channels_last), d['sep_ref'], d['act'], d['stride'], dt=torch.float32)[0]
    assert int((other != clean).sum()) <= cap
