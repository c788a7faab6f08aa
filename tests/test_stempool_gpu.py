"""FM_OP_STEMPOOL (csrc/stempool.hip): the ResNet stem -- 7x7 stride-2 conv, ReLU -- with its 3x3 stride-2 max pool in one
launch, against the unfused pair on the same input and both against tests/reid_ref.py in float64 under the conv's own
bound (the pool only selects).  Shapes: 32 x 16 (one partial tile), 70 x 38 (conv map 35 x 19, pooled 18 x 10: clipped
windows on both axes, several tiles), 256 x 128 at batch 2; cout 32 and 64; both pool forms; from the input tensor and from
a frame crop.

cout <= 32: the unfused conv is FM_OP_STEMCONV, whose K order and MFMA sequence the fused kernel repeats: bit-identical.
cout 64: the unfused conv is the generic FM_OP_CONV over the 8-channel padded pixel (K = 392 in 64-wide steps, another
summation order than 13 steps of 16 over K = 196): the results are NOT bit-identical; asserted instead, as
tests/sepconv_cases.max_order_flips does: every difference is one fp16 rounding of a value both hold within the bound, and
at most sqrt(K) 2^-12 of the outputs differ."""
import numpy as np
import pytest
import torch

import reid_ref
import torch_ref
from fastmot_amd.engine import HipNet, NET_EXTRACTOR
from fastmot_amd.models import graph as G
from sepconv_cases import max_order_flips

pytestmark = pytest.mark.gpu


def build(hw, cout, ppad, fused, seed=0):
    rng = np.random.default_rng(seed)
    w = rng.normal(0, (2.0 / 147) ** 0.5, (cout, 3, 7, 7)).astype(np.float32)
    b = rng.normal(0, 0.2, cout).astype(np.float32)
    g = G.Graph(None, hw, 3)
    if fused:
        y = g.stempool('stem', g.input, cout, (w, b), pool_pad=ppad)
    else:
        y = g.pool(g.conv('stem', g.input, cout, 7, 2, 'relu', pad=3, wb=(w, b)), 3, 2, ppad, pad_end=1)
    g.outputs = [y]
    return g, y


def run(ctx, g, y, x):
    net = HipNet(ctx, NET_EXTRACTOR, g, len(x))
    try:
        net.write(g.input, x)
        net.run(len(x))
        return net.read(y, len(x)).transpose(0, 3, 1, 2)
    finally:
        net.close()


@pytest.mark.parametrize('ppad', [1, 0])
@pytest.mark.parametrize('cout', [32, 64])
@pytest.mark.parametrize('hw,batch', [((32, 16), 1), ((70, 38), 3), ((256, 128), 2)])
def test_fused_stem_against_the_pair_and_the_reference(ctx, hw, batch, cout, ppad):
    x = np.random.default_rng(hw[0] + cout + ppad).normal(0, 1, (batch,) + hw + (3,)).astype(np.float16)
    gf, yf = build(hw, cout, ppad, True)
    gu, yu = build(hw, cout, ppad, False)
    assert [d['op'] for d in gf.layers] == [G.OP_STEMPOOL] and len(gu.layers) == 2 and (yf.h, yf.w) == (yu.h, yu.w)
    fused, pair = run(ctx, gf, yf, x), run(ctx, gu, yu, x)
    ref, bound = reid_ref.stempool(torch.from_numpy(x.astype(np.float32)).permute(0, 3, 1, 2), gf.layers[0]['stempool_ref'])
    assert tuple(ref.shape) == fused.shape == pair.shape
    rf = torch_ref.check_layer(fused, ref, bound, f'fused stem {hw} cout {cout} pool pad {ppad}')
    ru = torch_ref.check_layer(pair, ref, bound, f'unfused stem {hw} cout {cout} pool pad {ppad}')
    diff = int((fused != pair).sum())
    print(f'stempool {hw} x{batch} cout {cout} ppad {ppad}: worst err / bound fused {rf:.3f}, pair {ru:.3f}; {diff} of {fused.size} differ')
    if cout <= 32:
        assert diff == 0                                   # same K order in both kernels
    else:
        assert diff <= max_order_flips(fused.size, 147)
        # (both lie within `bound` of the same reference; a differing pair is one fp16 rounding apart)
        assert float(np.abs(fused - pair).max()) <= 2 * float(bound.max())


@pytest.mark.parametrize('stem,pool', [(32, 'pad1'), (64, 'ceil')])
def test_fused_stem_from_a_frame_crop(ctx, tmp_path, monkeypatch, stem, pool):
    """The extractor front end treats the op like FM_OP_STEMCONV: no crop kernel, no input tensor.  Against the unfused
    table (FASTMOT_STEMPOOL=0: crop kernel or FM_OP_STEMCONV from the frame, then the pool) through FeatureExtractor: the
    same crops and, for 32 stem channels, the same embeddings bit for bit; for 64, inside the measured bar."""
    import resnet_ref as R
    from fastmot_amd.feature_extractor import FeatureExtractor
    from fastmot_amd.models import ReID
    net = R.seeded(R.ResNet('basic', (1, 1, 1, 1), (stem, 32, 32, 32), stem=stem, pool=pool, head='none'), seed=stem)
    path = tmp_path / f'stem{stem}.onnx'
    path.write_bytes(R.export(net))
    name = f'StemPoolCrop{stem}'
    ReID.from_onnx(path, name=name)
    size = (640, 360)
    rng = np.random.default_rng(stem)
    frame = rng.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)
    boxes = np.array([[10.7, 20.2, 70.9, 200.1], [-5., -8., 40., 90.], [600., 300., 700., 400.], [100., 50., 131., 113.],
                      [300., 10., 555., 355.]])
    out = {}
    try:
        for fused in ('1', '0'):
            monkeypatch.setenv('FASTMOT_STEMPOOL', fused)
            ext = FeatureExtractor(name, batch_size=8, size=size, reuse_buffers=False)
            assert (ext.graph.layers[0]['op'] == G.OP_STEMPOOL) == (fused == '1')
            emb = np.asarray(ext(frame, boxes), np.float32).copy()
            out[fused] = (emb, ctx.extract_read_input(5, 32, 64), ext.graph)
    finally:
        ctx.feat_configure(512)
    np.testing.assert_array_equal(out['1'][1], out['0'][1])
    if stem <= 32:
        assert np.array_equal(out['1'][0].view(np.uint32), out['0'][0].view(np.uint32))
    x = np.ascontiguousarray(out['1'][1].transpose(0, 3, 1, 2)).astype(np.float32)
    expect, bar_abs, bar_cos = reid_ref.measured_bar(net, out['1'][2], x)
    for fused in ('1', '0'):
        reid_ref.check_embeddings(out[fused][0], expect, bar_abs, bar_cos, f'stem {stem} FASTMOT_STEMPOOL={fused}')
