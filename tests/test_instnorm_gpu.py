"""FM_OP_INSTNORM (csrc/instnorm.hip) and the GeM mode of FM_OP_POOLHEAD (csrc/reidhead_gem.hip) as one-layer networks on
the device against tests/ibn_ref.py in float64, fed the same fp16 input, under the elementwise bounds that module derives
from the number formats -- no tuned constant.  Shapes (C, cn, H x W): one pixel (variance 0: the output is beta), fewer
pixels than a wavefront with a pass-through half, three channel groups (a ragged last workgroup), exactly the register
path's capacity of 4096 pixels and a few above it, the 128 x 64 stem of an IBN-b model on the re-read path, and channel
views at an offset inside wider tensors."""
import numpy as np
import pytest
import torch

import ibn_ref
import torch_ref
from fastmot_amd.engine import HipNet, NET_EXTRACTOR
from fastmot_amd.models import graph as G
from fastmot_amd.models.graph import View

pytestmark = pytest.mark.gpu

REG_PIXELS = 4096                       # instnorm.hip: IN_T * IN_R pixels with one channel group per workgroup
SHAPES = [(8, 8, (1, 1)), (16, 8, (3, 11)), (64, 32, (16, 8)), (24, 24, (64, 32)), (8, 8, (64, 64)), (8, 8, (17, 241)), (16, 8, (128, 64)),
          (4096, 2048, (2, 3))]        # (the last: 8 channel groups per workgroup at batch 3, 4 at batch 1; the others run 1 or 2)
NMAX = 3


@pytest.fixture(scope='module', autouse=True)
def restore_feature_width(ctx):
    yield
    ctx.feat_configure(512)


def make_input(rng, n, c, hw):
    """Per-channel scales from 1e-2 to 30; channel 1: a large mean (100, std 0.1); channel 2: constant."""
    x = rng.normal(0, 1, (n,) + hw + (c,)) * np.geomspace(1e-2, 30, c) + rng.normal(0, 0.5, c)
    x[..., 1] = 100 + 0.1 * rng.normal(0, 1, (n,) + hw)
    x[..., 2] = 0.75
    return x.astype(np.float16)


def run_case(ctx, C, cn, hw, act, in_off=0, in_c=None, out_off=0, out_c=None, seed=0):
    assert hw[0] * hw[1] != REG_PIXELS or C == 8
    rng = np.random.default_rng(seed + C + 3 * cn + hw[0] * hw[1])
    in_c, out_c = in_c or C, out_c or C
    g = G.Graph(None, hw, in_c)
    src = g.input.slice(in_off, C)
    dst = g.new(hw[0], hw[1], out_c).slice(out_off, C)
    gamma, beta = rng.uniform(0.5, 1.5, cn).astype(np.float32), rng.normal(0, 0.3, cn).astype(np.float32)
    g.instnorm('in', src, gamma, beta, 1e-5, act, dst=dst)
    g.outputs = [dst]
    x = make_input(rng, NMAX, in_c, hw)
    fill = rng.normal(0, 1, (NMAX,) + hw + (out_c,)).astype(np.float16)
    eng = HipNet(ctx, NET_EXTRACTOR, g, NMAX)
    worst = 0.0
    try:
        d = g.layers[0]
        xin = torch.from_numpy(x.astype(np.float32)).permute(0, 3, 1, 2)
        kind, ref, bound = ibn_ref.run_layer(g, 0, {g.input.tid: xin})
        for batch in (1, NMAX):
            eng.write(g.input, x)
            eng.write(View(dst.tid, 0, out_c, *hw), fill)
            eng.run(batch)
            full = eng.read(View(dst.tid, 0, out_c, *hw), NMAX)
            got = torch.from_numpy(full[:batch, ..., out_off:out_off + C]).permute(0, 3, 1, 2)
            what = f'instnorm C={C} cn={cn} hw={hw} act={act} in {in_off}/{in_c} out {out_off}/{out_c} batch={batch}'
            r = ibn_ref.check_layer(got, ref[:batch], bound[:batch], what)
            print(f'{what}: worst err / bound = {r:.3f}')
            worst = max(worst, r)
            # channels outside the output view, and samples beyond the batch, keep their bytes
            keep = np.ones(out_c, bool)
            keep[out_off:out_off + C] = False
            assert np.array_equal(full[:batch][..., keep], fill[:batch][..., keep].astype(np.float32))
            assert np.array_equal(full[batch:], fill[batch:].astype(np.float32))
            if hw == (1, 1):        # variance 0: the output is act(beta), rounded once
                exp = np.float32(beta) if act == 'linear' else np.maximum(beta, 0)
                assert np.array_equal(full[:batch, 0, 0, out_off:out_off + cn], np.broadcast_to(exp.astype(np.float16).astype(np.float32), (batch, cn)))
        assert d['hid'] == cn
    finally:
        eng.close()
    return worst


@pytest.mark.parametrize('act', ['relu', 'linear'])
@pytest.mark.parametrize('C,cn,hw', SHAPES)
def test_instnorm_layer(ctx, C, cn, hw, act):
    run_case(ctx, C, cn, hw, act)


@pytest.mark.parametrize('act', ['relu', 'linear'])
def test_instnorm_on_channel_views(ctx, act):
    """Input channels [8, 40) of a 64-channel tensor -> output channels [16, 48) of a 56-channel tensor."""
    run_case(ctx, 32, 16, (16, 8), act, in_off=8, in_c=64, out_off=16, out_c=56)


def test_instnorm_refuses_tables_that_lie(ctx):
    """cn above the view, a view that leaves its tensor, an output in place: `bad argument` before any launch."""
    def table(mutate):
        g = G.Graph(None, (4, 4), 16)
        dst = g.instnorm('in', g.input, np.ones(8, np.float32), np.zeros(8, np.float32))
        g.outputs = [dst]
        mutate(g.layers[0], g)
        return g

    def lie_cn(d, g):
        d['hid'] = 24

    def lie_view(d, g):
        d['cin'] = d['cout'] = 24

    def lie_offset(d, g):
        d['out'] = View(d['out'].tid, 8, 16, 4, 4)

    def in_place(d, g):
        d['out'] = d['ins'][0]

    def lie_blob(d, g):
        d['w_off'] = len(g.blob) + 4096
    for mutate in (lie_cn, lie_view, lie_offset, in_place, lie_blob):
        g = table(mutate)
        made = []
        try:
            with pytest.raises(Exception, match='bad argument'):      # (offsets outside the blob: when the network is created)
                made.append(HipNet(ctx, NET_EXTRACTOR, g, 1))
                made[0].run(1)
        finally:
            for eng in made:
                eng.close()


GEM_SHAPES = [(32, (1, 1), None), (520, (8, 4), None), (2048, (16, 8), None), (64, (8, 4), 24)]
GEM_CASES = [(c, hw, d, neck, p) for c, hw, d in GEM_SHAPES for neck in (False, True) for p in (3.0, 2.6)]


@pytest.mark.parametrize('C,hw,D,neck,p', GEM_CASES)
def test_gem_head_layer(ctx, C, hw, D, neck, p):
    rng = np.random.default_rng(C + 7 * (D or 0) + neck + int(10 * p))
    nmax = 5
    x = rng.normal(0.3, 1.0, (nmax,) + hw + (C,)).astype(np.float16)        # (negative values too: the clamp matters)
    g = G.Graph(None, hw, C)
    scale = rng.uniform(0.5, 1.5, C).astype(np.float32)
    shift = rng.normal(0, 0.3, C).astype(np.float32)
    fc = (rng.normal(0, (1.0 / C) ** 0.5, (D, C)).astype(np.float32), rng.normal(0, 0.1, D).astype(np.float32)) if D else None
    g.poolhead('head', g.input, neck=(scale, shift) if neck else None, fc=fc, relu=bool(D), gem=(p, 1e-6))
    g.outputs = [g.input]
    dim = D or C
    ctx.feat_configure(dim)
    eng = HipNet(ctx, NET_EXTRACTOR, g, nmax)
    try:
        eng.write(g.input, x)
        d = g.layers[0]
        ref, bound = ibn_ref.poolhead(torch.from_numpy(x.astype(np.float32)).permute(0, 3, 1, 2), d['poolhead_ref'], d['gem_ref'])
        for batch in (1, 5):
            eng.run(batch)
            emb = eng.read_embeddings(batch)
            mirror = eng.read_embeddings_mirror(batch)
            what = f'GeM head C={C} HW={hw} D={D} neck={neck} p={p} batch={batch}'
            worst = ibn_ref.check_layer(emb, ref[:batch], bound[:batch], what)
            print(f'{what}: worst err / bound = {worst:.3f}')
            assert emb.shape == (batch, dim)
            assert np.array_equal(emb.view(np.uint32), mirror.view(np.uint32))             # the mirror row IS the device row
            norms = np.linalg.norm(emb.astype(np.float64), axis=1)
            assert np.abs(norms - 1).max() <= (dim + 4) * torch_ref.U32, norms
    finally:
        eng.close()


def test_gem_head_refuses_an_exponent_out_of_range(ctx):
    g = G.Graph(None, (2, 2), 16)
    g.poolhead('head', g.input, gem=(3.0, 1e-6))
    g.layers[0]['gates'][2] = G.f32_bits(32.0)
    g.outputs = [g.input]
    ctx.feat_configure(16)
    eng = HipNet(ctx, NET_EXTRACTOR, g, 1)
    try:
        with pytest.raises(Exception, match='bad argument'):
            eng.run(1)
    finally:
        eng.close()
