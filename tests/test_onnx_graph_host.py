"""General ONNX lowering for classification-style ReID backbones (fastmot_amd/models/onnx_graph.py) and its dispatch
(models/reid.py): CPU tests.  The networks are the plain-torch ResNets of tests/resnet_ref.py, exported by torch's own
ONNX serializer in both exporter forms; FM_OP_POOLHEAD's reference is tests/reid_ref.py."""
import functools
import hashlib

import numpy as np
import pytest
import torch

import onnx_writer as ow
import reid_ref
import resnet_ref as R
import torch_ref
from fastmot_amd.models import ReID, graph as G, onnx_graph
from fastmot_amd.models.onnx_reader import OnnxModel

CONVS = G.CONV_OPS + (G.OP_STEMCONV,)
HEADS = [('none', 'pad1'), ('bnneck', 'ceil'), ('fc512', 'pad1')]


@functools.lru_cache(maxsize=None)
def tiny_file(block, pool, head, folded=True):
    return R.export(R.tiny(block, pool, head), folded=folded)


def signature(g):
    return [(d['op'], d['cin'], d['cout'], d['k'], d['stride'], d['pad'], d['act'], d['res_mode'], d['out'].tid, d['out'].coff,
             tuple((v.tid, v.coff) for v in d['ins']), None if d['res'] is None else (d['res'].tid, d['res'].coff)) for d in g.layers]


# ------------------------------------------------------------------------------------------------ topology
@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('head,pool', HEADS)
@pytest.mark.parametrize('block', ['bottleneck', 'basic'])
def test_tiny_tables(block, head, pool, fused, monkeypatch):
    monkeypatch.setenv('FASTMOT_STEMPOOL', '1' if fused else '0')
    g, out = onnx_graph.lower(tiny_file(block, pool, head))
    ops = [d['op'] for d in g.layers]
    per_block = 3 if block == 'bottleneck' else 2
    # stem + max pool (ONE launch, or two with FASTMOT_STEMPOOL=0), four blocks with a downsample conv each, the head: one
    # launch per Conv node, ONE for everything behind the last block
    li = 1 if fused else 2
    assert len(g.layers) == li + 4 * (per_block + 1) + 1 and ops[-1] == G.OP_POOLHEAD
    assert all(op in G.CONV_OPS for op in ops[li:-1])
    stem, mp = g.layers[0], g.layers[li - 1]
    assert (stem['k'], stem['stride'], stem['pad'], stem['cout'], stem['act']) == (7, 2, 3, 16, G.ACT['relu'])
    assert stem['ins'][0].tid == g.input.tid and (mp['out'].h, mp['out'].w, mp['out'].c) == (16, 8, 16)
    if fused:
        assert ops[0] == G.OP_STEMPOOL and stem['gates'] == [1 if pool == 'pad1' else 0]
        assert len(g.tensors) == len(g.layers)                  # the conv's 32 x 16 output tensor does not exist
    else:
        assert ops[:2] == [G.OP_STEMCONV, G.OP_MAXPOOL] and (stem['out'].h, stem['out'].w) == (32, 16)
        assert (mp['k'], mp['stride'], mp['pad'], mp['pad_end']) == ((3, 2, 1, 1) if pool == 'pad1' else (3, 2, 0, 1))
    exp = 4 if block == 'bottleneck' else 1
    x = mp['out']
    for stage, mid in enumerate((8, 16, 32, 64)):
        blk = g.layers[li:li + per_block + 1]
        li += per_block + 1
        stride = 1 if stage == 0 else 2
        down = [d for d in blk if d['k'] == 1 and d['act'] == G.ACT['linear']]
        last = blk[-1]
        # the downsample path: a pointwise conv carrying the stage's stride, emitted BEFORE the conv whose epilogue reads it
        assert len(down) == 1 and down[0] is blk[-2] and down[0]['stride'] == stride and down[0]['ins'][0].tid == x.tid
        assert down[0]['cout'] == mid * exp and down[0]['res'] is None
        assert (down[0]['out'].h, down[0]['out'].w) == (x.h // stride, x.w // stride)
        # residual sum + ReLU = the epilogue of the block's last conv
        assert last['res_mode'] == G.RES_BEFORE_ACT and last['res'].tid == down[0]['out'].tid and last['act'] == G.ACT['relu']
        assert last['cout'] == mid * exp and blk[0]['ins'][0].tid == x.tid
        body = [d for d in blk if d is not down[0]]
        assert [d['k'] for d in body] == ([1, 3, 1] if block == 'bottleneck' else [3, 3])
        assert [d['stride'] for d in body] == ([1, stride, 1] if block == 'bottleneck' else [stride, 1])      # (v1.5: the 3x3 strides)
        assert all(d['act'] == G.ACT['relu'] and d['res'] is None for d in body[:-1])
        x = last['out']
    assert (x.h, x.w, x.c) == (2, 1, 64 * exp)
    hd = g.layers[-1]
    scale, shift, w, b, relu = hd['poolhead_ref']
    assert hd['ins'][0].tid == x.tid and hd['cin'] == 64 * exp
    assert (scale is not None) == (head == 'bnneck') and (w is not None) == (head == 'fc512') and relu == (head == 'fc512')
    assert hd['cout'] == (24 if head == 'fc512' else 64 * exp) and hd['gates'] == [int(head == 'bnneck'), int(head == 'fc512')]
    g.tables(max_batch=3, reuse=True)        # plan_arena / the C tables take the new op


@pytest.mark.parametrize('head,pool', HEADS)
@pytest.mark.parametrize('block', ['bottleneck', 'basic'])
def test_folded_and_unfolded_exports_give_equal_tables(block, head, pool):
    m0, m1 = OnnxModel(tiny_file(block, pool, head, True)), OnnxModel(tiny_file(block, pool, head, False))
    n_bn = [sum(n.op == 'BatchNormalization' for n in m.nodes) for m in (m0, m1)]
    assert n_bn[0] <= 1 and n_bn[1] >= 4 * 3 + 1              # the two exporter forms really differ
    g0, _ = onnx_graph.lower(m0)
    g1, _ = onnx_graph.lower(m1)
    assert signature(g0) == signature(g1)
    # BatchNorm folded by the exporter in float32 against folded here in float64: the last bit of an fp16 weight may differ
    for (l0, w0, b0), (l1, w1, b1) in zip(g0.conv_params, g1.conv_params):
        assert l0 == l1
        np.testing.assert_allclose(w0, w1, rtol=2e-3, atol=1e-6)
        np.testing.assert_allclose(b0, b1, rtol=1e-4, atol=1e-5)
    assert g0.layers[0]['op'] == G.OP_STEMPOOL
    np.testing.assert_allclose(g0.layers[0]['stempool_ref'][0], g1.layers[0]['stempool_ref'][0], rtol=2e-3, atol=1e-6)
    np.testing.assert_allclose(g0.layers[0]['stempool_ref'][1], g1.layers[0]['stempool_ref'][1], rtol=1e-4, atol=1e-5)
    for a, b in zip(g0.layers[-1]['poolhead_ref'][:4], g1.layers[-1]['poolhead_ref'][:4]):
        assert (a is None) == (b is None)
        if a is not None:
            np.testing.assert_allclose(a, b, rtol=2e-3, atol=1e-5)


# ------------------------------------------------------------------------------------------------ refusals
def hand_graph(extra=(), conv2=None, outputs=('emb',), unused=False):
    """input [1, 3, 32, 16] -> Conv c1 (8) -> Relu -> Conv c2 (8) -> Relu -> [extra nodes: 'r2' -> 'x'] -> GlobalAveragePool
    -> Flatten -> 'emb'."""
    rng = np.random.default_rng(0)
    c2 = dict(kernel_shape=[3, 3], pads=[1, 1, 1, 1], strides=[1, 1])
    c2.update(conv2 or {})
    cin2 = 8 // c2.get('group', 1)
    init = [ow.make_tensor('w1', 1, [8, 3, 3, 3], rng.normal(0, 0.3, 8 * 27)), ow.make_tensor('b1', 1, [8], rng.normal(0, 0.1, 8)),
            ow.make_tensor('w2', 1, [8, cin2, 3, 3], rng.normal(0, 0.2, 8 * cin2 * 9)), ow.make_tensor('b2', 1, [8], rng.normal(0, 0.1, 8)),
            ]
    if any('v8' in repr(n.data) for n in extra):
        init.append(ow.make_tensor('v8', 1, [8], rng.uniform(0.5, 1.5, 8)))
    if unused:
        init.append(ow.make_tensor('classifier.weight', 1, [4, 8], np.zeros(32)))
    nodes = [ow.make_node('Conv', ['input', 'w1', 'b1'], ['t1'], name='c1', kernel_shape=[3, 3], pads=[1, 1, 1, 1], strides=[2, 2]),
             ow.make_node('Relu', ['t1'], ['r1'], name='relu1'),
             ow.make_node('Conv', ['r1', 'w2', 'b2'], ['t2'], name='c2', **c2),
             ow.make_node('Relu', ['t2'], ['r2'], name='relu2')]
    nodes += list(extra) or [ow.make_node('Identity', ['r2'], ['x'], name='id')]
    nodes += [ow.make_node('GlobalAveragePool', ['x'], ['p'], name='gap'), ow.make_node('Flatten', ['p'], ['emb'], name='flat', axis=1)]
    outs = [ow.make_tensor_value_info(o, 1, [1, 8]) for o in outputs]
    g = ow.make_graph(nodes, 'hand', [ow.make_tensor_value_info('input', 1, [1, 3, 32, 16])], outs, init)
    return ow.make_model(g).data


def test_hand_graph_lowers():
    g, _ = onnx_graph.lower(hand_graph())
    assert [d['op'] for d in g.layers] == [G.OP_STEMCONV, G.OP_CONV, G.OP_POOLHEAD] and g.layers[-1]['cout'] == 8


REFUSED = {
    'ibn': dict(extra=[ow.make_node('InstanceNormalization', ['r2', 'v8', 'v8'], ['x'], name='ibn_a', epsilon=1e-5)], op='InstanceNormalization', node='ibn_a'),
    'gem': dict(extra=[ow.make_node('Pow', ['r2', 'v8'], ['x'], name='gem_pow')], op='Pow', node='gem_pow'),
    'sigmoid': dict(extra=[ow.make_node('Sigmoid', ['r2'], ['x'], name='se_sigmoid')], op='Sigmoid', node='se_sigmoid'),
    'mul': dict(extra=[ow.make_node('Mul', ['r2', 'r2'], ['x'], name='se_scale')], op='Mul', node='se_scale'),
    'grouped': dict(conv2=dict(group=2), op='Conv', node='c2', what='group'),
    'dilated': dict(conv2=dict(dilations=[2, 2], pads=[2, 2, 2, 2]), op='Conv', node='c2', what='dilations'),
    'asymmetric': dict(conv2=dict(pads=[0, 0, 1, 1]), op='Conv', node='c2', what='pads'),
}


@pytest.mark.parametrize('case', sorted(REFUSED))
def test_unsupported_nodes_are_refused_by_name(case):
    spec = REFUSED[case]
    with pytest.raises(NotImplementedError) as e:
        onnx_graph.lower(hand_graph(extra=spec.get('extra', ()), conv2=spec.get('conv2')))
    msg = str(e.value)
    assert repr(spec['node']) in msg and f'({spec["op"]})' in msg and spec.get('what', '') in msg
    assert 'Supported: Conv (groups 1' in msg and 'GlobalAveragePool' in msg


def test_second_output_is_refused():
    with pytest.raises(NotImplementedError, match='2 graph outputs'):
        onnx_graph.lower(hand_graph(outputs=('emb', 'p')))


def test_unused_initializer_raises():
    with pytest.raises(ValueError, match=r"parameters not used.*classifier\.weight"):
        onnx_graph.lower(hand_graph(unused=True))


# ------------------------------------------------------------------------------------------------ dispatch
def test_descriptor_without_channels_builds_from_its_onnx_file(tmp_path):
    """Fails on the parent commit: ReID.build_graph unpacked CHANNELS = None and called osnet_graph unconditionally."""
    path = tmp_path / 'tiny_r.onnx'
    path.write_bytes(tiny_file('bottleneck', 'pad1', 'none'))

    class TinyR(ReID):
        MODEL_PATH = path
        INPUT_SHAPE = (3, 64, 32)
        OUTPUT_LAYOUT = 256
        METRIC = 'euclidean'
    assert TinyR.CHANNELS is None and ReID.get_model('TinyR') is TinyR
    g, out = TinyR.build_graph()
    assert g.layers[-1]['op'] == G.OP_POOLHEAD and g.layers[-1]['cout'] == 256 and len(g.layers) == 18
    # an explicit source: path or bytes
    for src in (path, str(path), path.read_bytes()):
        g2, _ = TinyR.build_graph(src)
        assert bytes(g2.blob) == bytes(g.blob)
    with pytest.raises(TypeError, match='ONNX'):
        TinyR.build_graph(G.RandomWeights(1))
    # the checks against the descriptor
    with pytest.raises(ValueError, match='INPUT_SHAPE'):
        type('TinyRShape', (TinyR,), dict(INPUT_SHAPE=(3, 128, 64))).build_graph()
    with pytest.raises(ValueError, match='OUTPUT_LAYOUT'):
        type('TinyRDim', (TinyR,), dict(OUTPUT_LAYOUT=512)).build_graph()
    # a missing file is an error even where random weights are opted into: there is no topology to fill with them
    path.unlink()
    with pytest.raises(FileNotFoundError):
        TinyR.build_graph()


def test_from_onnx_registers_a_descriptor(tmp_path):
    path = tmp_path / 'my-reid.fc.onnx'
    path.write_bytes(tiny_file('basic', 'pad1', 'fc512'))
    desc = ReID.from_onnx(path, metric='cosine')
    assert desc.__name__ == 'my_reid_fc' and ReID.get_model('my_reid_fc') is desc and issubclass(desc, ReID)
    assert (desc.INPUT_SHAPE, desc.OUTPUT_LAYOUT, desc.METRIC, desc.CHANNELS) == ((3, 64, 32), 24, 'cosine', None)
    g, _ = desc.build_graph()
    assert g.layers[-1]['cout'] == 24
    named = ReID.from_onnx(path, name='PedestrianR18')
    assert ReID.get_model('PedestrianR18') is named and named.METRIC == 'euclidean'
    with pytest.raises(FileNotFoundError):
        ReID.from_onnx(tmp_path / 'nope.onnx')


# sha256 of repr(layer signature) of OSNet025's table, recorded on the commit before this lowering existed
OSNET025_SIGNATURE = 'e122569369c9b9b5f52d34c0a61e296e2e152f24e94e139743b5048ebe5810db'


def osnet_signature(g):
    sig = [(d['op'], d.get('name'), d['cin'], d['cout'], d['k'], d['stride'], d['act'], d['up'], d['out'].tid, d['out'].coff,
            tuple((v.tid, v.coff) for v in d['ins'])) for d in g.layers]
    return hashlib.sha256((repr(sig) + hashlib.sha256(bytes(g.blob)).hexdigest()).encode()).hexdigest()


def test_osnet_descriptors_keep_their_path():
    """A descriptor WITH CHANNELS goes the way it went: same layer table and parameter blob (seeded weights) as before."""
    desc = ReID.get_model('OSNet025')
    g, _ = desc.build_graph(G.RandomWeights(seed=1))
    assert g.layers[-1]['op'] == G.OP_OSTAIL and all(d['op'] != G.OP_POOLHEAD for d in g.layers)
    assert osnet_signature(g) == OSNET025_SIGNATURE
    # ... strict walker included: a ResNet file is not an OSNet
    with pytest.raises(ValueError, match='does not walk like torchreid OSNet'):
        desc.build_graph(tiny_file('bottleneck', 'pad1', 'none'))


# ------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize('head,pool', HEADS)
@pytest.mark.parametrize('block', ['bottleneck', 'basic'])
def test_table_on_the_cpu_interpreter_equals_the_module(block, head, pool):
    """torch module -> ONNX -> layer table -> tests/torch_ref.py + reid_ref.py in fp32 == the module.  The table holds
    fp16-rounded weights: the bar is the one tests/test_onnx_reader.py uses for OSNet on the same interpreter."""
    net = R.tiny(block, pool, head)
    g, _ = onnx_graph.lower(tiny_file(block, pool, head))
    x = R.random_input(3, (64, 32), seed=5)
    expect = R.embed(net, x)
    _, emb = reid_ref.run_graph(g, torch.from_numpy(x), emulate_fp16_storage=False)
    emb = emb.numpy()
    assert emb.shape == expect.shape
    assert np.abs(emb - expect).max() < 5e-3 and (np.sum(emb * expect, axis=1) > 0.9999).all()


@functools.lru_cache(maxsize=None)
def resnet50_file(pool='pad1', head='none'):
    return R.export(R.resnet50(pool, head), hw=(256, 128))


@pytest.mark.parametrize('fused', [True, False])
def test_resnet50_table_at_full_size(fused, monkeypatch):
    monkeypatch.setenv('FASTMOT_STEMPOOL', '1' if fused else '0')
    g = onnx_graph.lower(resnet50_file(), (3, 256, 128), 2048)[0]
    ops = [d['op'] for d in g.layers]
    first = 1 if fused else 2
    # stem + pool (1 launch fused, 2 unfused) + 16 bottlenecks x 3 convs + 4 downsample convs + 1 head
    assert len(g.layers) == first + 48 + 4 + 1 and ops[-1] == G.OP_POOLHEAD and all(op in G.CONV_OPS for op in ops[first:-1])
    if fused:
        assert ops[0] == G.OP_STEMPOOL and g.layers[0]['cout'] == 64 and g.layers[0]['gates'] == [1]
        assert all((h, w) != (128, 64) for h, w, _, _ in g.tensors)                  # the 128 x 64 x 64 conv output is never stored
    else:
        assert ops[:2] == [G.OP_CONV, G.OP_MAXPOOL]                                  # (64 output channels: not the <= 32 stem kernel)
        assert (g.layers[0]['out'].h, g.layers[0]['out'].w, g.layers[0]['out'].c) == (128, 64, 64)
    sizes = []
    for d in g.layers[first - 1:-1]:
        s = (d['out'].h, d['out'].w)
        if not sizes or sizes[-1] != s:
            sizes.append(s)
    assert sizes == [(64, 32), (32, 16), (16, 8), (8, 4)]
    # the strided pointwise convs of the downsample paths and the widths the family brings: cin / cout 1024 and 2048, a
    # 2048-channel residual operand
    body = g.layers[first:-1]
    down = [d for d in body if d['k'] == 1 and d['act'] == G.ACT['linear']]
    assert [(d['cin'], d['cout'], d['stride']) for d in down] == [(64, 256, 1), (256, 512, 2), (512, 1024, 2), (1024, 2048, 2)]
    # (the DMA-fed kernel at the large maps, the streamed one at 16 x 8 and 8 x 4: both address the input with the stride --
    # tests/test_reid_onnx_gpu.py checks every one of these layers on the device)
    assert [d['op'] for d in down] == [G.OP_CONVD, G.OP_CONVD, G.OP_CONVS, G.OP_CONVS]
    assert max(d['cin'] for d in body) == 2048 and max(d['cout'] for d in body) == 2048
    assert sum(d['res'] is not None and d['res'].c == 2048 for d in g.layers) == 3
    hd = g.layers[-1]
    assert (hd['cin'], hd['cout'], hd['ins'][0].h, hd['ins'][0].w) == (2048, 2048, 8, 4)
    assert g.conv_flops() == pytest.approx(2 * 2.7e9, rel=0.05)                       # ~2.7 GMAC per 256 x 128 crop
    _, _, blob = g.tables(max_batch=16, reuse=True)
    assert len(blob) > 2 * 23e6
    if fused:           # (with buffer reuse the arena's peak lies in stage 1, 3 x 64 x 32 x 256: it does not grow)
        monkeypatch.setenv('FASTMOT_STEMPOOL', '0')
        gu = onnx_graph.lower(resnet50_file())[0]
        gu.tables(max_batch=16, reuse=True)
        assert g.arena_bytes <= gu.arena_bytes


# ------------------------------------------------------------------------------------------------ the bound
def head_case(C, HW, D, neck, relu, n=3, seed=0):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(np.abs(rng.normal(0, 1, (n, C, HW, 1))).astype(np.float16).astype(np.float32))
    scale = rng.uniform(0.5, 1.5, C).astype(np.float32) if neck else None
    shift = rng.normal(0, 0.3, C).astype(np.float32) if neck else None
    w = rng.normal(0, (1.0 / C) ** 0.5, (D, C)).astype(np.float16).astype(np.float32) if D else None
    b = rng.normal(0, 0.1, D).astype(np.float32) if D else None
    return x, (scale, shift, w, b, relu)


@pytest.mark.parametrize('C,HW,D,neck,relu', [(64, 32, 0, False, False), (64, 32, 0, True, False), (64, 32, 64, True, False),
                                              (256, 8, 24, True, True), (2048, 32, 512, False, True)])
def test_poolhead_bound_holds_for_a_clean_fp32_stand_in(C, HW, D, neck, relu):
    """The same head in float32 (another summation order than the device's, the same number formats) stays inside the
    float64 reference's bound -- and not by orders of magnitude: the bound is not vacuous."""
    x, ref = head_case(C, HW, D, neck, relu)
    ref64, bound = reid_ref.poolhead(x, ref)
    got, _ = reid_ref.poolhead(x, ref, dtype=torch.float32, track=False)
    worst = torch_ref.check_layer(got, ref64, bound, 'fp32 stand-in')
    assert worst <= 1
    assert float(bound.max()) < 0.05 * float(ref64.abs().max())
    np.testing.assert_allclose(ref64.norm(dim=1).numpy(), 1.0, atol=1e-12)


@pytest.mark.parametrize('mistake,C,HW,D', [('mean_hw1', 64, 32, 24), ('mean_hw1', 2048, 32, 512), ('neck_after_fc', 64, 32, 64)])
def test_poolhead_bound_catches_planted_mistakes(mistake, C, HW, D):
    """(a mean over HW + 1 only rescales a head WITHOUT bias or neck -- the L2 normalisation removes it -- so the cases
    have an FC bias; the neck behind the FC instead of in front of it needs D == C to be expressible)"""
    x, ref = head_case(C, HW, D, neck=True, relu=False)
    ref64, bound = reid_ref.poolhead(x, ref)
    bad, _ = reid_ref.poolhead(x, ref, dtype=torch.float32, track=False, mistake=mistake)
    with pytest.raises(AssertionError, match='over the bound'):
        torch_ref.check_layer(bad, ref64, bound, mistake)


# ---- the fused stem
def stem_case(hw=(38, 22), cout=16, ppad=1, n=2, seed=0):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.normal(0, 1, (n, 3) + hw).astype(np.float16).astype(np.float32))
    w = rng.normal(0, (2.0 / 147) ** 0.5, (cout, 3, 7, 7)).astype(np.float16).astype(np.float32)
    return x, (w, rng.normal(0, 0.2, cout).astype(np.float32), ppad)


@pytest.mark.parametrize('ppad', [1, 0])
def test_stempool_bound_and_what_it_can_see(ppad):
    """A float32 stand-in with fp16 storage stays inside the bound.  Of the mistakes one might plant, two are INVISIBLE by
    construction and asserted to be so: ReLU and the fp16 rounding are monotone, so they commute with the maximum --
    padding the pool with 0 BEFORE the ReLU gives relu(max(0, a_i)) = max_i relu(a_i), and an intermediate left unrounded
    gives round(max a_i) = max round(a_i) once the pooled value is stored as fp16.  Neither is an error of the fused
    kernel's result.  A visible one -- the other padding form, i.e. windows shifted by one -- is far outside the bound."""
    x, ref = stem_case(ppad=ppad)
    ref64, bound = reid_ref.stempool(x, ref)
    clean, _ = reid_ref.stempool(x, ref, dtype=torch.float32, track=False)
    assert torch_ref.check_layer(clean, ref64, bound, 'fp32 stand-in') <= 1
    assert float((bound / ref64.abs().clamp_min(1.0)).max()) < 2e-3
    for mistake in ('pool_pad_zero', 'unrounded'):
        bad, _ = reid_ref.stempool(x, ref, dtype=torch.float32, track=False, mistake=mistake)
        assert torch.equal(bad.half(), clean.half()), mistake
    other, _ = reid_ref.stempool(x, (ref[0], ref[1], 1 - ppad), dtype=torch.float32, track=False)
    if other.shape == clean.shape:
        with pytest.raises(AssertionError, match='over the bound'):
            torch_ref.check_layer(other, ref64, bound, 'other padding form')
    else:
        assert ppad == 0 or other.shape != clean.shape
    # against plain torch: conv -> relu -> fp16 -> MaxPool2d in the exporter's two forms
    y = torch.relu(torch.nn.functional.conv2d(x.double(), torch.from_numpy(ref[0]).double(), torch.from_numpy(ref[1]).double(), 2, 3))
    mp = torch.nn.MaxPool2d(3, 2, 1) if ppad else torch.nn.MaxPool2d(3, 2, 0, ceil_mode=True)
    assert torch_ref.check_layer(mp(y), ref64, bound, 'torch MaxPool2d') <= 1
