"""FM_OP_CONVIN (csrc/convin.hip) without a device: the one support rule on both sides of the library boundary, and the derived
bound of tests/convin_ref.py against a float32 host stand-in of the fused op -- the correct stand-in stays inside it at every
shape the device test runs, and each planted mistake leaves it at the shapes where the arithmetic says it must show."""
import ctypes

import numpy as np
import pytest
import torch

import convin_ref as C
import ibn_ref
from fastmot_amd import _lib
from fastmot_amd.models import graph as G
from fastmot_amd.models.graph import Graph


def test_convin_supported_agrees_with_the_library():
    lib = _lib.load()
    lib.fm_convin_supported.restype = ctypes.c_int
    lib.fm_convin_supported.argtypes = [ctypes.c_int] * 3
    for K in (0, 4, 8, 12, 16, 24, 64, 352, 4096, 4104):
        for cout in (0, 8, 20, 32, 40, 384, 4096, 4104):
            for hw in (0, 1, 32, 33, 2047, 2048, 2049, 8192):
                assert Graph.convin_supported(K, cout, hw) == bool(lib.fm_convin_supported(K, cout, hw)), (K, cout, hw)
    assert G.CONVIN_MAX_HW == 2048


def test_unsupported_shapes_hold_the_unfused_pair():
    """A map above the capacity, and FASTMOT_CONVIN=0, leave a linear conv + FM_OP_INSTNORM in the table (the residual in the
    conv for BEFORE_NORM, on the norm for AFTER_NORM); the parameters and the reference tuple are the same."""
    for hw, use in (((64, 64), True), ((16, 8), False)):
        for mode in (G.RES_BEFORE_NORM, G.RES_AFTER_NORM):
            g = Graph(None, hw, 16)
            g.use_convin = use
            res = g.new(hw[0], hw[1], 24)
            w, b = np.ones((24, 16, 1, 1), np.float32), np.zeros(24, np.float32)
            g.convin('tail', g.input, 24, (np.ones(24), np.zeros(24)), res=res, res_mode=mode, wb=(w, b))
            conv, norm = g.layers
            assert conv['op'] in G.CONV_OPS and conv['act'] == G.ACT['linear'] and norm['op'] == G.OP_INSTNORM
            assert norm['act'] == G.ACT['relu'] and norm['hid'] == 24 and norm['ins'][0].tid == conv['out'].tid
            if mode == G.RES_BEFORE_NORM:
                assert conv['res'] is res and conv['res_mode'] == G.RES_BEFORE_ACT and norm['res'] is None
            else:
                assert conv['res'] is None and norm['res'] is res and norm['res_mode'] == G.RES_BEFORE_ACT
    g = Graph(None, (16, 8), 16)
    g.use_convin = True
    g.convin('tail', g.input, 24, (np.ones(24), np.zeros(24)), wb=(w, b))
    assert [d['op'] for d in g.layers] == [G.OP_CONVIN] and g.layers[0]['res_mode'] == G.RES_NONE


def test_the_default_form_is_the_one_that_measured_faster(monkeypatch):
    """profiles/reid_ain.txt: the fused pass was slower, so the unfused pair is the default and FASTMOT_CONVIN=1 the switch."""
    monkeypatch.delenv('FASTMOT_CONVIN', raising=False)
    assert Graph(None, (4, 4), 8).use_convin is False
    monkeypatch.setenv('FASTMOT_CONVIN', '1')
    assert Graph(None, (4, 4), 8).use_convin is True


def stand_in(g, bufs, batch, mistake=None):
    d = g.layers[0]
    x = bufs[g.input.tid][:batch, d['ins'][0].coff:d['ins'][0].coff + d['ins'][0].c]
    res = bufs[d['res'].tid][:batch, d['res'].coff:d['res'].coff + d['res'].c] if d['res'] is not None else None
    y, _ = C.convin(x, d['convin_ref'], d['act'], res, d['res_mode'], dtype=torch.float32, track=False, mistake=mistake)
    return y.half().float()


@pytest.mark.parametrize('K,cout,hw,mode', C.CASES)
def test_correct_stand_in_stays_inside_the_bound(K, cout, hw, mode):
    g, _, x, r = C.make_case(K, cout, hw, mode)
    bufs, ref, bound = C.reference(g, x, r)
    for batch in (1, C.NMAX):
        worst = ibn_ref.check_layer(stand_in(g, bufs, batch), ref[:batch], bound[:batch], f'stand-in {K} {cout} {hw} mode {mode}')
        print(f'stand-in K={K} cout={cout} hw={hw} mode={mode} batch={batch}: worst err / bound = {worst:.3f}')


# where each mistake must show (reasoning, not observation):
#   unbiased      a factor sqrt(HW / (HW - 1)) on every normalised value: 1.5 % at 33 pixels, 0.4 % at 128 -- above the fp16
#                 store's 2^-11; at 2048 pixels it is 2^-12 and hides in the store, at one pixel both variances are 0
#   no_eps        the constant channel (all-zero weights, variance 0): 0 * inf, at every shape
#   batch_stats   every shape at batch 3 (at one pixel the batch gives the channel a variance it does not have)
#   ex2           the channel that copies the mean-100 input: one rounding of mean^2 = 10^4 is 6e-4, 6 % of its variance 0.01
#                 (HW > 1).  Not at 64 x 32: this stand-in sums with torch's pairwise fp32 reduction, which averages the
#                 roundings of 2048 squares out where a sequential device sum would not, and the defect it shows there is of
#                 the size of the bound's own allowance for that channel (K u 100 per value against a deviation of 0.1)
#   res_side      every shape, either mode
#   padded        33 pixels: 31 padding lanes that hold the bias alone
MISTAKES = [('unbiased', [c for c in C.CASES if c[2] in ((3, 11), (16, 8))]),
            ('no_eps', C.CASES),
            ('batch_stats', C.CASES),
            ('ex2', [c for c in C.CASES if c[2] not in ((1, 1), (64, 32))]),
            ('res_side', C.CASES),
            ('padded', [c for c in C.CASES if c[2] == (3, 11)])]


@pytest.mark.parametrize('mistake,cases', MISTAKES, ids=[m for m, _ in MISTAKES])
def test_planted_mistakes_leave_the_bound(mistake, cases):
    assert cases
    for K, cout, hw, mode in cases:
        g, _, x, r = C.make_case(K, cout, hw, mode)
        bufs, ref, bound = C.reference(g, x, r)
        with pytest.raises(AssertionError, match='bound'):
            ibn_ref.check_layer(stand_in(g, bufs, C.NMAX, mistake), ref, bound, f'{mistake} {K} {cout} {hw} mode {mode}')


def test_instnorm_residual_reference_reduces_to_ibn_ref():
    """With a zero residual the extended reference and bound are ibn_ref's (plus the add's own rounding term)."""
    rng = np.random.default_rng(5)
    x = torch.from_numpy(C.make_input(rng, 2, 16, (3, 11)).astype(np.float32)).permute(0, 3, 1, 2)
    ref = (rng.uniform(0.5, 1.5, 8).astype(np.float32), rng.normal(0, 0.3, 8).astype(np.float32), 1e-5)
    a, ea = ibn_ref.instnorm(x, ref, 8, G.ACT['relu'])
    b, eb = C.instnorm_res(x, ref, 8, G.ACT['relu'], torch.zeros_like(x))
    assert torch.equal(a, b)
    pre = C.instnorm_res(x, ref, 8, G.ACT['linear'], torch.zeros_like(x))[0]
    assert torch.allclose(eb, ea + C.U32 * pre.abs(), rtol=1e-12, atol=0)
