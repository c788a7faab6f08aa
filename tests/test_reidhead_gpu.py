"""FM_OP_POOLHEAD (csrc/reidhead.hip) as a one-layer network on the device against tests/reid_ref.py in float64, fed the
same fp16 input, under the elementwise bound reid_ref derives from the number formats (fp32 accumulation over HW and over
C) -- no tuned constant.  Shapes: the smallest head (one pixel, one wavefront's worth of channels),
a channel count that is no multiple of the workgroup size, ResNet-50's 2048 channels over the largest map a 256 x 128
crop leaves at stride 16, and the two FC forms (a small one, and 2048 -> 512 of resnet50_fc512)."""
import numpy as np
import pytest
import torch

import reid_ref
import torch_ref
from fastmot_amd.engine import HipNet, NET_EXTRACTOR
from fastmot_amd.models import graph as G

pytestmark = pytest.mark.gpu

SHAPES = [(32, (1, 1), None), (520, (8, 4), None), (2048, (16, 8), None), (64, (8, 4), 24), (2048, (8, 4), 512)]
CASES = [(c, hw, d, neck, relu) for c, hw, d in SHAPES for neck in (False, True) for relu in ((False, True) if d else (False,))]


@pytest.fixture(scope='module', autouse=True)
def restore_feature_width(ctx):
    yield
    ctx.feat_configure(512)


@pytest.mark.parametrize('C,hw,D,neck,relu', CASES)
def test_poolhead_layer(ctx, C, hw, D, neck, relu):
    rng = np.random.default_rng(C + 7 * (D or 0) + neck + 2 * relu)
    nmax = 5
    x = rng.normal(0.3, 1.0, (nmax,) + hw + (C,)).astype(np.float16)
    g = G.Graph(None, hw, C)
    scale = rng.uniform(0.5, 1.5, C).astype(np.float32)
    shift = rng.normal(0, 0.3, C).astype(np.float32)
    fc = (rng.normal(0, (1.0 / C) ** 0.5, (D, C)).astype(np.float32), rng.normal(0, 0.1, D).astype(np.float32)) if D else None
    g.poolhead('head', g.input, neck=(scale, shift) if neck else None, fc=fc, relu=relu)
    g.outputs = [g.input]
    dim = D or C
    ctx.feat_configure(dim)
    eng = HipNet(ctx, NET_EXTRACTOR, g, nmax)
    try:
        eng.write(g.input, x)
        ref, bound = reid_ref.poolhead(torch.from_numpy(x.astype(np.float32)).permute(0, 3, 1, 2), g.layers[0]['poolhead_ref'])
        for batch in (1, 5):
            eng.run(batch)
            emb = eng.read_embeddings(batch)
            mirror = eng.read_embeddings_mirror(batch)
            worst = torch_ref.check_layer(emb, ref[:batch], bound[:batch], f'poolhead C={C} HW={hw} D={D} neck={neck} relu={relu} batch={batch}')
            print(f'C={C} hw={hw} D={D} neck={neck} relu={relu} batch={batch}: worst err / bound = {worst:.3f}')
            assert emb.shape == (batch, dim) and np.isfinite(emb).all()
            assert np.array_equal(emb.view(np.uint32), mirror.view(np.uint32))             # the mirror row IS the device row
            norms = np.linalg.norm(emb.astype(np.float64), axis=1)
            assert np.abs(norms - 1).max() <= (dim + 4) * torch_ref.U32, norms
    finally:
        eng.close()


def test_poolhead_refuses_what_does_not_fit(ctx):
    """C above 4096 never reaches the device: Graph.poolhead refuses it, and so does the launch (LDS sized from C and D)."""
    g = G.Graph(None, (1, 1), 4104)
    with pytest.raises(ValueError, match='4096'):
        g.poolhead('head', g.input)
    g = G.Graph(None, (1, 1), 64)
    g.poolhead('head', g.input)
    g.layers[0]['cin'] = g.layers[0]['cout'] = 72                # a table that lies about its tensor
    g.outputs = [g.input]
    ctx.feat_configure(72)
    eng = HipNet(ctx, NET_EXTRACTOR, g, 1)
    try:
        with pytest.raises(Exception, match='bad argument'):
            eng.run(1)
    finally:
        eng.close()
