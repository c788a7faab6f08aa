"""FM_OP_CONVIN (csrc/convin.hip) and FM_OP_INSTNORM with its residual view as one-layer networks on the device against
tests/convin_ref.py in float64, fed the same fp16 inputs, under the elementwise bound that module derives -- no tuned
constant.  Shapes (K, cout, H x W): one pixel (variance 0: the output is act(beta (+ res)), exactly), K % 16 == 8 with a ragged
channel tile and 33 pixels, four whole pixel tiles, exactly the capacity of 2048 pixels, the concat form of an IBN block, and
channel views at offsets inside wider tensors.  Every case holds a constant output channel and one that copies the mean-100
input channel; batches 1 and 3; bytes outside the output view and samples beyond the batch keep their values; sample 0 does
not depend on the batch."""
import numpy as np
import pytest
import torch

import convin_ref as C
import ibn_ref
from fastmot_amd.engine import HipNet, NET_EXTRACTOR
from fastmot_amd.models import graph as G
from fastmot_amd.models.graph import View

pytestmark = pytest.mark.gpu
NMAX = C.NMAX


@pytest.fixture(scope='module', autouse=True)
def restore_feature_width(ctx):
    yield
    ctx.feat_configure(512)


def run_one_layer(ctx, g, x, r, what, exact=None):
    """Runs the one-layer graph at batches 1 and NMAX; -> worst err / bound."""
    d = g.layers[0]
    o, hw = d['out'], (d['out'].h, d['out'].w)
    out_c = g.tensors[o.tid][2]
    rng = np.random.default_rng(99)
    fill = rng.normal(0, 1, (NMAX,) + hw + (out_c,)).astype(np.float16)
    _, ref, bound = C.reference(g, x, r)
    eng = HipNet(ctx, NET_EXTRACTOR, g, NMAX)
    worst, first = 0.0, None
    try:
        for batch in (1, NMAX):
            eng.write(g.input, x)
            if d['res'] is not None:
                eng.write(View(d['res'].tid, 0, g.tensors[d['res'].tid][2], *hw), r)
            eng.write(View(o.tid, 0, out_c, *hw), fill)
            eng.run(batch)
            full = eng.read(View(o.tid, 0, out_c, *hw), NMAX)
            got = torch.from_numpy(full[:batch, ..., o.coff:o.coff + o.c]).permute(0, 3, 1, 2)
            ratio = ibn_ref.check_layer(got, ref[:batch], bound[:batch], f'{what} batch={batch}')
            print(f'{what} batch={batch}: worst err / bound = {ratio:.3f}')
            worst = max(worst, ratio)
            keep = np.ones(out_c, bool)
            keep[o.coff:o.coff + o.c] = False
            assert np.array_equal(full[:batch][..., keep], fill[:batch][..., keep].astype(np.float32))
            assert np.array_equal(full[batch:], fill[batch:].astype(np.float32))
            if first is None:
                first = full[0].copy()
            assert np.array_equal(full[0], first), 'sample 0 depends on the batch'
            if exact is not None:
                assert np.array_equal(full[:batch, ..., o.coff:o.coff + o.c], exact[:batch])
    finally:
        eng.close()
    return worst


@pytest.mark.parametrize('K,cout,hw,mode', C.CASES)
def test_convin_layer(ctx, K, cout, hw, mode):
    g, res, x, r = C.make_case(K, cout, hw, mode)
    exact = None
    if hw == (1, 1):                # variance 0: act(beta (+ res behind the norm)), rounded once
        beta = np.asarray(g.layers[0]['convin_ref'][3], np.float32)
        pre = beta[None, None, None, :] + (r.astype(np.float32) if mode == G.RES_AFTER_NORM else np.float32(0))
        exact = np.maximum(np.broadcast_to(pre, (NMAX, 1, 1, cout)), 0).astype(np.float16).astype(np.float32)
    run_one_layer(ctx, g, x, r, f'convin K={K} cout={cout} hw={hw} res_mode={mode}', exact)


@pytest.mark.parametrize('mode', [G.RES_BEFORE_NORM, G.RES_AFTER_NORM])
def test_convin_on_channel_views(ctx, mode):
    """Input channels [8, 32) of a 48-channel tensor -> output channels [16, 56) of a 64-channel tensor, the residual at
    [8, 48) of a 56-channel tensor; linear activation."""
    g, res, x, r = C.make_case(24, 40, (3, 11), mode, in_off=8, in_c=48, out_off=16, out_c=64, res_off=8, res_c=56, act='linear')
    d = g.layers[0]
    assert (d['ins'][0].coff, d['out'].coff, d['res'].coff) == (8, 16, 8)
    run_one_layer(ctx, g, x, r, f'convin on views res_mode={mode}')


def test_convin_without_residual(ctx):
    g, res, x, r = C.make_case(16, 8, (5, 7), G.RES_NONE)
    assert res is None
    run_one_layer(ctx, g, x, r, 'convin without residual')


@pytest.mark.parametrize('C_,cn,hw', [(16, 8, (3, 11)), (16, 16, (3, 11)), (64, 64, (16, 8))])
def test_instnorm_with_residual(ctx, C_, cn, hw):
    rng = np.random.default_rng(C_ + cn + hw[0])
    g = G.Graph(None, hw, C_)
    res = g.new(hw[0], hw[1], C_ + 8).slice(8, C_)
    gamma, beta = rng.uniform(0.5, 1.5, cn).astype(np.float32), rng.normal(0, 0.3, cn).astype(np.float32)
    dst = g.instnorm('in', g.input, gamma, beta, 1e-5, 'relu', res=res)
    g.outputs = [dst]
    assert g.layers[0]['res_mode'] == G.RES_BEFORE_ACT
    x = C.make_input(rng, NMAX, C_, hw)
    r = rng.normal(0, 1, (NMAX,) + hw + (C_ + 8,)).astype(np.float16)
    run_one_layer(ctx, g, x, r, f'instnorm + residual C={C_} cn={cn} hw={hw}')


def test_convin_refuses_tables_that_lie(ctx, monkeypatch):
    """A map above the capacity forced into the op, K beyond the input view, an output in place, a residual view that leaves
    its tensor: `bad argument` before any launch."""
    def table(mutate, hw=(4, 4)):
        g = G.Graph(None, hw, 16)
        g.use_convin = True
        res = g.new(hw[0], hw[1], 16)
        dst = g.convin('tail', g.input, 16, (np.ones(16), np.zeros(16)), res=res, res_mode=G.RES_AFTER_NORM,
                       wb=(np.zeros((16, 16, 1, 1), np.float32), np.zeros(16, np.float32)))
        g.outputs = [dst]
        assert g.layers[0]['op'] == G.OP_CONVIN
        mutate(g.layers[0], g)
        return g

    def lie_k(d, g):
        d['cin'] = 24

    def in_place(d, g):
        d['out'] = d['ins'][0]

    def lie_res(d, g):
        d['res'] = View(d['res'].tid, 8, 16, 4, 4)

    def lie_res_mode(d, g):
        d['res_mode'] = G.RES_AFTER_ACT

    def lie_blob(d, g):
        d['w2_off'] = len(g.blob) + 4096
    tables = [table(m) for m in (lie_k, in_place, lie_res, lie_res_mode, lie_blob)]
    monkeypatch.setattr(G.Graph, 'convin_supported', staticmethod(lambda K, cout, hw: True))
    tables.append(table(lambda d, g: None, hw=(64, 64)))            # 4096 pixels
    monkeypatch.undo()
    for g in tables:
        made = []
        try:
            with pytest.raises(Exception, match='bad argument'):
                made.append(HipNet(ctx, NET_EXTRACTOR, g, 1))
                made[0].run(1)
        finally:
            for eng in made:
                eng.close()
