"""IBN-Net ReID models through the ONNX lowering (models/onnx_graph.py: FM_OP_INSTNORM, GeM in FM_OP_POOLHEAD): CPU tests.
The networks are the plain-torch models of tests/ibn_ref.py, exported by torch's own serializer in both exporter forms;
the references and bounds of the two device stages are restated there."""
import functools

import numpy as np
import pytest
import torch

import ibn_ref
import onnx_writer as ow
import resnet_ref as R
import torch_ref
from fastmot_amd.models import ReID, graph as G, onnx_graph

KINDS = {'ibn_a': dict(ibn='a'), 'ibn_b': dict(ibn='b'), 'gem': dict(pool='gem'), 'gem_learned': dict(pool='gem', p=2.6, learn_p=True, head='bnneck'),
         'ibn_a_gem': dict(ibn='a', pool='gem', head='bnneck')}


def tiny_net(kind):
    return ibn_ref.tiny(**KINDS[kind])


@functools.lru_cache(maxsize=None)
def tiny_file(kind, folded=True):
    return R.export(tiny_net(kind), folded=folded)


def norms(g):
    return [(i, d) for i, d in enumerate(g.layers) if d['op'] == G.OP_INSTNORM]


# ------------------------------------------------------------------------------------------------ topology
@pytest.mark.parametrize('folded', [True, False])
def test_ibn_a_table(folded):
    net = tiny_net('ibn_a')
    g, _ = onnx_graph.lower(tiny_file('ibn_a', folded))
    ins = norms(g)
    # one conv + one OP_INSTNORM per IBN layer (stages 1-3; mid widths 16, 16, 32), the stem still ONE launch
    assert g.layers[0]['op'] == G.OP_STEMPOOL and [d['hid'] for _, d in ins] == [8, 8, 16]
    mods = [b.bn1 for b in net.blocks][:3]
    for (i, d), mod in zip(ins, mods):
        conv = g.layers[i - 1]
        assert conv['op'] in G.CONV_OPS and conv['act'] == G.ACT['linear'] and conv['res'] is None and conv['k'] == 1
        assert d['ins'][0].tid == conv['out'].tid and d['out'].tid != conv['out'].tid
        assert d['cin'] == d['cout'] == conv['cout'] == 2 * d['hid'] and d['act'] == G.ACT['relu']
        assert (d['out'].h, d['out'].w, d['out'].c) == (conv['out'].h, conv['out'].w, conv['cout'])
        gamma, beta, eps = d['instnorm_ref']
        np.testing.assert_array_equal(gamma, mod.IN.weight.detach().numpy())
        np.testing.assert_array_equal(beta, mod.IN.bias.detach().numpy())
        assert eps == float(np.float32(1e-5)) and d['gates'] == [G.f32_bits(1e-5)] == [0x3727C5AC]
        assert g.layers[i + 1]['ins'][0].tid == d['out'].tid                     # the 3x3 conv reads the normalised map
        # the BatchNorm half went into rows [h:] of the conv; rows [:h] are the file's
        _, w, b = next(p for p in g.conv_params if p[0] == i - 1)
        h = d['hid']
        assert np.all(b[:h] == 0) and np.any(b[h:] != 0)
    assert g.layers[-1]['op'] == G.OP_POOLHEAD and 'gem_ref' not in g.layers[-1] and g.layers[-1]['gates'] == [0, 0]
    g.tables(max_batch=3, reuse=True)


@pytest.mark.parametrize('folded', [True, False])
def test_ibn_b_table(folded):
    g, _ = onnx_graph.lower(tiny_file('ibn_b', folded))
    ins = norms(g)
    # the stem: conv + instnorm + pool (FM_OP_STEMPOOL is not used); the last block of stages 1-2: conv with the residual, no
    # activation, then instnorm over all channels with the ReLU
    assert [d['op'] for d in g.layers[:3]] == [G.OP_STEMCONV, G.OP_INSTNORM, G.OP_MAXPOOL]
    assert [(d['hid'], d['cin']) for _, d in ins] == [(16, 16), (64, 64), (64, 64)]
    assert g.layers[0]['act'] == G.ACT['linear'] and (g.layers[0]['out'].h, g.layers[0]['out'].w) == (32, 16)
    for i, d in ins:
        assert d['act'] == G.ACT['relu'] and d['ins'][0].tid == g.layers[i - 1]['out'].tid
    for i, d in ins[1:]:
        conv = g.layers[i - 1]
        assert conv['res_mode'] == G.RES_BEFORE_ACT and conv['res'] is not None and conv['act'] == G.ACT['linear']
    assert all(d['op'] != G.OP_ADD for d in g.layers)
    g.tables(max_batch=3, reuse=True)


@pytest.mark.parametrize('kind,p,neck', [('gem', 3.0, False), ('gem_learned', 2.6, True), ('ibn_a_gem', 3.0, True)])
@pytest.mark.parametrize('folded', [True, False])
def test_gem_head_table(kind, p, neck, folded):
    g, _ = onnx_graph.lower(tiny_file(kind, folded))
    hd = g.layers[-1]
    assert hd['op'] == G.OP_POOLHEAD and hd['gem_ref'] == (float(np.float32(p)), float(np.float32(1e-6)))
    assert hd['gates'] == [int(neck), 0, G.f32_bits(p), G.f32_bits(1e-6)] and len(hd['poolhead_ref']) == 5
    assert (hd['poolhead_ref'][0] is not None) == neck
    _, ls, _ = g.tables(max_batch=2, reuse=True)
    assert list(ls[len(g.layers) - 1].gate) == hd['gates']


def test_plain_head_keeps_its_fields():
    g = G.Graph(None, (4, 2), 16)
    g.poolhead('head', g.input)
    assert g.layers[0]['gates'] == [0, 0] and 'gem_ref' not in g.layers[0]
    with pytest.raises(ValueError, match='GeM'):
        G.Graph(None, (4, 2), 16).poolhead('head', G.Graph(None, (4, 2), 16).input, gem=(0.25, 1e-6))
    with pytest.raises(ValueError, match='multiples of 8'):
        g2 = G.Graph(None, (4, 2), 16)
        g2.instnorm('in', g2.input, np.ones(4), np.zeros(4))


@pytest.mark.parametrize('kind', ['ibn_a', 'ibn_b', 'ibn_a_gem'])
def test_folded_and_unfolded_exports_give_equal_tables(kind):
    def sig(g):
        return [(d['op'], d['cin'], d['cout'], d['hid'] if d['op'] == G.OP_INSTNORM else 0, d['k'], d['stride'], d['act'], d['res_mode'],
                 d['out'].tid, tuple(v.tid for v in d['ins'])) for d in g.layers]
    g0, g1 = (onnx_graph.lower(tiny_file(kind, f))[0] for f in (True, False))
    assert sig(g0) == sig(g1)
    for (l0, w0, b0), (l1, w1, b1) in zip(g0.conv_params, g1.conv_params):
        np.testing.assert_allclose(w0, w1, rtol=2e-3, atol=1e-6)
        np.testing.assert_allclose(b0, b1, rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize('folded', [True, False])
@pytest.mark.parametrize('kind', sorted(KINDS))
def test_table_on_the_cpu_interpreter_equals_the_module(kind, folded):
    """torch module -> ONNX -> layer table -> the fp32 interpreter of tests/ibn_ref.py == the module, within what the
    resnet_ref-based host tests use (tests/test_onnx_graph_host.py: fp16-rounded weights in the table)."""
    net = tiny_net(kind)
    g, _ = onnx_graph.lower(tiny_file(kind, folded))
    x = R.random_input(3, (64, 32), seed=5)
    expect = R.embed(net, x)
    _, emb = ibn_ref.run_graph(g, torch.from_numpy(x), emulate_fp16_storage=False)
    emb = emb.numpy()
    assert emb.shape == expect.shape
    assert np.abs(emb - expect).max() < 5e-3 and (np.sum(emb * expect, axis=1) > 0.9999).all()


def test_surfaces_reach_the_new_path(tmp_path):
    path = tmp_path / 'r-ibn.onnx'
    path.write_bytes(tiny_file('ibn_a_gem'))
    desc = ReID.from_onnx(path, metric='cosine')
    g, _ = desc.build_graph()
    assert (desc.INPUT_SHAPE, desc.OUTPUT_LAYOUT) == ((3, 64, 32), 256) and len(norms(g)) == 3 and 'gem_ref' in g.layers[-1]

    class TinyIBNb(ReID):
        MODEL_PATH = tmp_path / 'b.onnx'
        INPUT_SHAPE = (3, 64, 32)
        OUTPUT_LAYOUT = 256
        METRIC = 'euclidean'
    TinyIBNb.MODEL_PATH.write_bytes(tiny_file('ibn_b'))
    assert len(norms(TinyIBNb.build_graph()[0])) == 3


# ------------------------------------------------------------------------------------------------ refusals
def hand_graph(extra, conv2_out=16):
    """input [1, 3, 32, 16] -> Conv c1 (8) -> Relu r1 -> Conv c2 (16) 't2' -> [extra nodes: 't2' -> 'emb']."""
    rng = np.random.default_rng(0)
    init = [ow.make_tensor('w1', 1, [8, 3, 3, 3], rng.normal(0, 0.3, 8 * 27)), ow.make_tensor('b1', 1, [8], rng.normal(0, 0.1, 8)),
            ow.make_tensor('w2', 1, [conv2_out, 8, 3, 3], rng.normal(0, 0.2, conv2_out * 72)),
            ow.make_tensor('b2', 1, [conv2_out], rng.normal(0, 0.1, conv2_out))]
    for n in (4, 8, 12, 16):
        if any(f'v{n}' in repr(nd.data) for nd in extra):
            init.append(ow.make_tensor(f'v{n}', 1, [n], rng.uniform(0.5, 1.5, n)))
    for name, val in (('gem_eps', 1e-6), ('gem_three', 3.0), ('gem_third', 1.0 / 3), ('gem_half', 0.5)):
        if any(name.encode() in nd.data for nd in extra):
            init.append(ow.make_tensor(name, 1, [], [val]))
    nodes = [ow.make_node('Conv', ['input', 'w1', 'b1'], ['t1'], name='c1', kernel_shape=[3, 3], pads=[1, 1, 1, 1], strides=[2, 2]),
             ow.make_node('Relu', ['t1'], ['r1'], name='relu1'),
             ow.make_node('Conv', ['r1', 'w2', 'b2'], ['t2'], name='c2', kernel_shape=[3, 3], pads=[1, 1, 1, 1], strides=[1, 1])]
    nodes += list(extra)
    g = ow.make_graph(nodes, 'hand', [ow.make_tensor_value_info('input', 1, [1, 3, 32, 16])],
                      [ow.make_tensor_value_info('emb', 1, [1, conv2_out])], init)
    return ow.make_model(g).data


def ibn(parts, first='in', cat=('ni', 'nb')):
    a, b = parts
    ops = {'in': lambda src, dst, n: ow.make_node('InstanceNormalization', [src, f'v{n}', f'v{n}'], [dst], name='ibn_in', epsilon=1e-5),
           'bn': lambda src, dst, n: ow.make_node('BatchNormalization', [src, f'v{n}', f'v{n}', f'v{n}', f'v{n}'], [dst], name='ibn_bn', epsilon=1e-5)}
    second = 'bn' if first == 'in' else 'in'
    return [ow.make_node('Split', ['t2'], ['s0', 's1'], name='ibn_split', axis=1, split=[a, b]),
            ops[first]('s0', 'ni' if first == 'in' else 'nb', a), ops[second]('s1', 'nb' if first == 'in' else 'ni', b),
            ow.make_node('Concat', list(cat), ['cc'], name='ibn_cat', axis=1), ow.make_node('Relu', ['cc'], ['x'], name='ibn_relu')]


TAIL = [ow.make_node('GlobalAveragePool', ['x'], ['p'], name='gap'), ow.make_node('Flatten', ['p'], ['emb'], name='flat', axis=1)]


def gem(root='gem_third', clip=True, exponent='gem_three'):
    nodes = [ow.make_node('Relu', ['t2'], ['r2'], name='relu2')]
    nodes += [ow.make_node('Clip', ['r2', 'gem_eps', ''], ['cl'], name='gem_clip')] if clip else [ow.make_node('Identity', ['r2'], ['cl'], name='id')]
    nodes += [ow.make_node('Pow', ['cl', exponent], ['pw'], name='gem_pow'), ow.make_node('GlobalAveragePool', ['pw'], ['p'], name='gap')]
    if root:
        return nodes + [ow.make_node('Flatten', ['p'], ['f'], name='flat', axis=1), ow.make_node('Pow', ['f', root], ['emb'], name='gem_root')]
    return nodes + [ow.make_node('Flatten', ['p'], ['emb'], name='flat', axis=1)]


def test_hand_graphs_lower():
    g, _ = onnx_graph.lower(hand_graph(ibn((8, 8)) + TAIL))
    assert [d['op'] for d in g.layers] == [G.OP_STEMCONV, G.OP_CONV, G.OP_INSTNORM, G.OP_POOLHEAD] and g.layers[2]['hid'] == 8
    g, _ = onnx_graph.lower(hand_graph(gem()))
    assert g.layers[-1]['gem_ref'] == (3.0, float(np.float32(1e-6)))


REFUSED = {
    'split_not_8': dict(extra=ibn((4, 12)) + TAIL, op='Split', node='ibn_split', what='multiple of 8'),
    'in_trailing': dict(extra=ibn((8, 8), first='bn', cat=('nb', 'ni')) + TAIL, op='BatchNormalization', node='ibn_bn', what='must lead'),
    'parts_do_not_tile': dict(extra=ibn((8, 4)) + TAIL, op='Split', node='ibn_split', what='tile'),
    'part_read_elsewhere': dict(extra=ibn((8, 8))[:1] + [ow.make_node('Relu', ['s0'], ['x'], name='stray_relu')] + TAIL, op='Relu', node='stray_relu'),
    'gem_no_root': dict(extra=gem(root=None), op='GlobalAveragePool', node='gap', what='without its root'),
    'gem_wrong_root': dict(extra=gem(root='gem_half'), op='Pow', node='gem_root', what='does not match'),
    'gem_no_clip': dict(extra=gem(clip=False), op='Pow', node='gem_pow'),
    'gem_per_channel': dict(extra=gem(exponent='v16'), op='Pow', node='gem_pow', what='per-channel'),
    # the two hand graphs of tests/test_onnx_graph_host.py, restated: a normalisation of a stored, activated map; a bare Pow
    'old_ibn': dict(extra=[ow.make_node('Relu', ['t2'], ['r2'], name='relu2'),
                           ow.make_node('InstanceNormalization', ['r2', 'v16', 'v16'], ['x'], name='ibn_a', epsilon=1e-5)] + TAIL,
                    op='InstanceNormalization', node='ibn_a'),
    'old_gem': dict(extra=[ow.make_node('Relu', ['t2'], ['r2'], name='relu2'), ow.make_node('Pow', ['r2', 'v16'], ['x'], name='gem_pow')] + TAIL,
                    op='Pow', node='gem_pow'),
    'mul_of_maps': dict(extra=[ow.make_node('Relu', ['t2'], ['r2'], name='relu2'), ow.make_node('Mul', ['r2', 'r2'], ['x'], name='se_scale')] + TAIL,
                        op='Mul', node='se_scale'),
}


@pytest.mark.parametrize('case', sorted(REFUSED))
def test_new_forms_are_refused_by_name(case):
    spec = REFUSED[case]
    with pytest.raises(NotImplementedError) as e:
        onnx_graph.lower(hand_graph(spec['extra']))
    msg = str(e.value)
    assert repr(spec['node']) in msg and f'({spec["op"]})' in msg and spec.get('what', '') in msg
    assert 'Supported: Conv (groups 1' in msg and 'GlobalAveragePool' in msg and 'InstanceNormalization' in msg


# ------------------------------------------------------------------------------------------------ the bounds
def norm_case(n=3, c=24, cn=16, hw=(16, 8), seed=0):
    """Per-channel scales from 1e-2 to 30; channel 1: mean 100, std 0.1; channel 2: constant; pass-through channels of both signs."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (n, c) + hw) * np.geomspace(1e-2, 30, c)[None, :, None, None] + rng.normal(0, 0.5, (1, c, 1, 1))
    x[:, 1] = 100 + 0.1 * rng.normal(0, 1, (n,) + hw)
    x[:, 2] = 0.75
    x = torch.from_numpy(x.astype(np.float16).astype(np.float32))
    return x, (rng.uniform(0.5, 1.5, cn).astype(np.float32), rng.normal(0, 0.3, cn).astype(np.float32), float(np.float32(1e-5))), cn


def store(v):
    return v.half().to(torch.float64)


@pytest.mark.parametrize('act', ['relu', 'linear'])
@pytest.mark.parametrize('hw', [(1, 1), (3, 11), (16, 8), (64, 32)])
def test_instnorm_bound_holds_for_a_clean_fp32_stand_in(hw, act):
    x, ref, cn = norm_case(hw=hw)
    it = torch_ref._Interp(None, None, torch.float64, emulate=False, track=True)
    ref64, bound = it.store16(ibn_ref.instnorm(x, ref, cn, G.ACT[act]))
    got, _ = ibn_ref.instnorm(x, ref, cn, G.ACT[act], dtype=torch.float32, track=False)
    worst = torch_ref.check_layer(store(got), ref64, bound, 'fp32 stand-in')
    assert worst <= 1
    # not vacuous: away from the large-mean and the constant channel the typical bound stays below a percent of the value
    # even at 2048 pixels, where every centred value pays (HW + 1) u |mean| and the variance (HW + 1) u of itself
    if hw[0] * hw[1] >= 128:
        rel = (bound / ref64.abs().clamp_min(0.1))[:, 3:cn]
        assert float(rel.median()) < 1e-2, float(rel.median())
    if hw == (1, 1):            # (torch refuses to normalise one pixel; the result is beta)
        return
    # against torch's own operator
    y = torch.nn.functional.instance_norm(x[:, :cn].double(), weight=torch.from_numpy(ref[0]).double(), bias=torch.from_numpy(ref[1]).double(),
                                          eps=ref[2])
    if act == 'relu':
        y = torch.relu(y)
    np.testing.assert_allclose(ref64[:, :cn].numpy(), y.numpy(), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize('mistake,channel', [('unbiased', None), ('no_eps', 2), ('batch_stats', None), ('ex2', 1), ('pass_raw', None)])
def test_instnorm_bound_catches_planted_mistakes(mistake, channel):
    x, ref, cn = norm_case()
    it = torch_ref._Interp(None, None, torch.float64, emulate=False, track=True)
    ref64, bound = it.store16(ibn_ref.instnorm(x, ref, cn, G.ACT['relu']))
    # (no_eps: 0 * (1 / sqrt(0)) on the constant channel is not a number, which torch_ref.check_layer's comparison passes:
    # ibn_ref.check_layer refuses non-finite results first)
    bad, _ = ibn_ref.instnorm(x, ref, cn, G.ACT['relu'], dtype=torch.float32, track=False, mistake=mistake)
    sel = slice(None) if channel is None else slice(channel, channel + 1)
    with pytest.raises(AssertionError, match='over the bound'):
        ibn_ref.check_layer(store(bad)[:, sel], ref64[:, sel], bound[:, sel], mistake)


def gem_case(C=64, hw=(8, 4), neck=True, D=24, n=3, seed=0, negative=True):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.3, 1.0, (n, C) + hw)          # (op-level input WITH negative values: the clamp matters)
    x = torch.from_numpy((x if negative else np.abs(x)).astype(np.float16).astype(np.float32))
    scale = rng.uniform(0.5, 1.5, C).astype(np.float32) if neck else None
    shift = rng.normal(0, 0.3, C).astype(np.float32) if neck else None
    w = rng.normal(0, (1.0 / C) ** 0.5, (D, C)).astype(np.float16).astype(np.float32) if D else None
    b = rng.normal(0, 0.1, D).astype(np.float32) if D else None
    return x, (scale, shift, w, b, False)


@pytest.mark.parametrize('p', [3.0, 2.6, 0.5, 16.0])
@pytest.mark.parametrize('C,hw,neck,D', [(64, (8, 4), True, 24), (32, (1, 1), False, 0), (2048, (16, 8), True, 0)])
def test_gem_bound_holds_for_a_clean_fp32_stand_in(C, hw, neck, D, p):
    x, ref = gem_case(C, hw, neck, D)
    gem = (p, float(np.float32(1e-6)))
    ref64, bound = ibn_ref.poolhead(x, ref, gem)
    got, _ = ibn_ref.poolhead(x, ref, gem, dtype=torch.float32, track=False)
    assert torch_ref.check_layer(got, ref64, bound, 'fp32 stand-in') <= 1
    assert float(bound.max()) < 0.05 * float(ref64.abs().max())
    # against the module's expression
    v = torch.flatten(torch.nn.functional.adaptive_avg_pool2d(x.double().clamp(min=gem[1]).pow(p), 1), 1).pow(1.0 / p)
    pooled, _ = ibn_ref.gem_pool(x, gem)
    np.testing.assert_allclose(pooled[:, :, 0, 0].numpy(), v.numpy(), rtol=1e-9)


@pytest.mark.parametrize('p', [3.0, 2.6])
@pytest.mark.parametrize('mistake', ['no_clamp', 'no_root', 'pow_of_mean'])
def test_gem_bound_catches_planted_mistakes(mistake, p):
    x, ref = gem_case()
    gem = (p, float(np.float32(1e-6)))
    ref64, bound = ibn_ref.poolhead(x, ref, gem)
    bad, _ = ibn_ref.poolhead(x, ref, gem, dtype=torch.float32, track=False, mistake=mistake)
    with pytest.raises(AssertionError, match='over the bound'):
        ibn_ref.check_layer(bad, ref64, bound, mistake)


# ------------------------------------------------------------------------------------------------ full size
def test_resnet50_ibn_a_gem_table_at_full_size():
    g = onnx_graph.lower(R.export(ibn_ref.resnet50_ibn_a(), hw=(256, 128)), (3, 256, 128), 2048)[0]
    ins = norms(g)
    assert [d['hid'] for _, d in ins] == [32] * 3 + [64] * 4 + [128] * 6
    assert [(d['out'].h, d['out'].w) for _, d in ins] == [(64, 32)] * 4 + [(32, 16)] * 4 + [(16, 8)] * 5      # (v1.5: a stage's first 1x1 runs before the stride)
    assert g.layers[0]['op'] == G.OP_STEMPOOL and len(g.layers) == 1 + 48 + 4 + 13 + 1
    hd = g.layers[-1]
    assert hd['gem_ref'][0] == 3.0 and hd['gates'][:2] == [1, 0] and (hd['cin'], hd['cout']) == (2048, 2048)
    g.plan_arena(16, True)
    ts, ls, blob = g.tables(max_batch=16, reuse=True)
    i, d = ins[0]
    assert (ls[i].op, ls[i].hid, ls[i].cin, ls[i].act, ls[i].gate[0]) == (25, 32, 64, G.ACT['relu'], 0x3727C5AC)
    assert torch_ref.OP_NAMES[25] == 'OP_INSTNORM'
