"""fast-reid's non-local blocks without a device: the lowering of both exporter forms (models/onnx_graph.py -> FM_OP_NONLOCAL),
its refusals by node name, the one support rule on both sides of the library boundary, and the derived bound of
tests/nonlocal_ref.py against a float32 host stand-in -- three summation orders stay inside it at every shape the device test
runs, and each planted mistake leaves it at the shapes where the arithmetic says it must show."""
import ctypes

import numpy as np
import pytest
import torch

import ibn_ref
import nonlocal_ref as NL
import onnx_writer as ow
import resnet_ref as R
from fastmot_amd import _lib
from fastmot_amd.models import ReID, graph as G, onnx_graph
from fastmot_amd.models.graph import Graph
from fastmot_amd.models.onnx_reader import OnnxModel

# (what, the net, [(channels, h, w) of its non-local blocks])
NETS = {'resnet-nl': (NL.tiny, [(64, 8, 4), (128, 4, 2)]),
        'nl in front of the pool': (lambda: NL.tiny(nl_after={4: [0]}), [(256, 2, 1)]),
        'sbs': (NL.tiny_sbs, [(64, 8, 4), (128, 4, 2)])}


def signature(g):
    return [(d['op'], d['cin'], d['cout'], d['k'], d['stride'], d['pad'], d['act'], d['hid'], d['res_mode'], d['out'].tid, d['out'].c,
             d['out'].h, d['out'].w) for d in g.layers]


# ------------------------------------------------------------------------------------------------ lowering
@pytest.mark.parametrize('kind', sorted(NETS))
def test_both_exporter_forms_lower_to_the_same_table(kind):
    make, where = NETS[kind]
    net = make()
    files = [NL.export(net, folded=f) for f in (True, False)]
    ops = [{n.op for n in OnnxModel(f).nodes} for f in files]
    assert 'Unsqueeze' not in ops[0] and {'Unsqueeze', 'Concat', 'BatchNormalization'} <= ops[1]     # the two forms really differ
    g0, g1 = (onnx_graph.lower(f)[0] for f in files)
    assert signature(g0) == signature(g1)
    mods = [m for m in net.modules() if isinstance(m, NL.NonLocal)]
    for g in (g0, g1):
        at = [i for i, d in enumerate(g.layers) if d['op'] == G.OP_NONLOCAL]
        assert len(at) == len(mods) == len(where)
        for i, m, (c, h, w) in zip(at, mods, where):
            d, prev = g.layers[i], g.layers[i - 1]
            # behind the block it follows: it reads that block's output (conv + residual + ReLU) and writes a new tensor
            assert d['ins'][0].tid == prev['out'].tid and prev['act'] == G.ACT['relu'] and prev['res_mode'] == G.RES_BEFORE_ACT
            assert (d['cin'], d['cout'], d['out'].h, d['out'].w) == (c, c, h, w) and d['out'].tid != d['ins'][0].tid and d['res'] is None
            assert g.layers[i + 1]['ins'][0].tid == d['out'].tid
            # the module's parameters, W + BatchNorm folded in float64 (the exporter folds in float32)
            want = NL.folded_params(m)
            for got, ref in zip(d['nl_ref'][:5], want[:5]):
                np.testing.assert_allclose(got, ref, rtol=2e-3, atol=1e-6)
            np.testing.assert_allclose(d['nl_ref'][5], want[5], rtol=1e-4, atol=1e-5)
            assert all(a.dtype == np.float32 for a in d['nl_ref'])
    for d0, d1 in zip(g0.layers, g1.layers):
        if d0['op'] == G.OP_NONLOCAL:
            for a, b in zip(d0['nl_ref'], d1['nl_ref']):
                np.testing.assert_allclose(a, b, rtol=2e-3, atol=1e-6)
    if kind == 'sbs':
        assert sum(d['op'] == G.OP_INSTNORM for d in g0.layers) == 3 and 'gem_ref' in g0.layers[-1]
    g0.tables(max_batch=3, reuse=True)            # plan_arena / the C tables take the new op
    # the table computes what the module computes (fp32 interpretation on the host, no fp16 storage)
    x = R.random_input(3, (64, 32), seed=5)
    expect = R.embed(net, x)
    _, emb = NL.run_graph(g0, torch.from_numpy(x), emulate_fp16_storage=False)
    emb = emb.numpy()
    assert np.abs(emb - expect).max() < 5e-3 and (np.sum(emb * expect, axis=1) > 0.9999).all()


def test_surfaces_reach_the_new_path(tmp_path):
    path = tmp_path / 'sbs.onnx'
    path.write_bytes(NL.export(NL.tiny_sbs()))
    desc = ReID.from_onnx(path, metric='cosine')
    g, _ = desc.build_graph()
    assert (desc.INPUT_SHAPE, desc.OUTPUT_LAYOUT) == ((3, 64, 32), 256) and sum(d['op'] == G.OP_NONLOCAL for d in g.layers) == 2


def test_graph_nonlocal_checks_its_arguments():
    g = Graph(None, (4, 4), 16)
    v = [np.ones(16, np.float32)] * 3
    with pytest.raises(ValueError, match='five vectors'):
        g.nonlocal_('nl', g.input, *v, [0, 0, 0], np.ones(8), np.ones(16))
    with pytest.raises(ValueError, match='multiple of 8'):
        g12 = Graph(None, (4, 4), 12)
        g12.nonlocal_('nl', g12.input, *v, [0, 0, 0], np.ones(16), np.ones(16))
    with pytest.raises(ValueError, match='4096 pixels'):
        big = Graph(None, (128, 64), 16)
        big.nonlocal_('nl', big.input, *v, [0, 0, 0], np.ones(16), np.ones(16))


# ------------------------------------------------------------------------------------------------ refusals
def hand_block(c=8, inter=1, divisor=128.0, mul=False, other='r1', stray=None, softmax=False, x_from='r1'):
    """input [1, 3, 32, 16] -> Conv c1 (c, stride 2) -> Relu r1 [c, 16, 8] -> Conv c2 (c) -> Relu r2 -> the non-local block over
    `x_from`, hand-written as the exporter's folded form, summed with `other` -> 'x' -> GlobalAveragePool -> Flatten -> 'emb'."""
    rng = np.random.default_rng(0)
    f = lambda name, shape, scale=0.3: ow.make_tensor(name, 1, list(shape), rng.normal(0, scale, int(np.prod(shape))))
    init = [f('w1', (c, 3, 3, 3)), f('b1', (c,)), f('w2', (c, c, 3, 3)), f('b2', (c,)), f('wW', (c, inter, 1, 1)), f('bW', (c,)),
            ow.make_tensor('flat', 7, [3], [1, inter, -1]), ow.make_tensor('map', 7, [4], [1, inter, 16, 8]),
            ow.make_tensor('div', 1, [], [1.0 / divisor if mul else divisor])]
    for r in ('g', 'theta', 'phi'):
        init += [f(f'w{r}', (inter, c, 1, 1)), f(f'b{r}', (inter,))]
    pw = dict(kernel_shape=[1, 1], pads=[0, 0, 0, 0], strides=[1, 1])
    nodes = [ow.make_node('Conv', ['input', 'w1', 'b1'], ['t1'], name='c1', kernel_shape=[3, 3], pads=[1, 1, 1, 1], strides=[2, 2]),
             ow.make_node('Relu', ['t1'], ['r1'], name='relu1'),
             ow.make_node('Conv', ['r1', 'w2', 'b2'], ['t2'], name='c2', kernel_shape=[3, 3], pads=[1, 1, 1, 1], strides=[1, 1]),
             ow.make_node('Relu', ['t2'], ['r2'], name='relu2')]
    for r in ('g', 'theta', 'phi'):
        nodes += [ow.make_node('Conv', [x_from, f'w{r}', f'b{r}'], [f'{r}0'], name=f'nl_{r}', **pw),
                  ow.make_node('Reshape', [f'{r}0', 'flat'], [f'{r}1'], name=f'nl_{r}_flat')]
        if r != 'phi':
            nodes.append(ow.make_node('Transpose', [f'{r}1'], [f'{r}2'], name=f'nl_{r}_t', perm=[0, 2, 1]))
    nodes.append(ow.make_node('MatMul', ['theta2', 'phi1'], ['f'], name='nl_f'))
    if softmax:
        nodes.append(ow.make_node('Softmax', ['f'], ['fn'], name='nl_softmax', axis=2))
    else:
        nodes.append(ow.make_node('Mul' if mul else 'Div', ['f', 'div'], ['fn'], name='nl_div'))
    if stray:
        nodes.append(ow.make_node('Relu', [stray], ['stray_out'], name='stray_relu'))
    nodes += [ow.make_node('MatMul', ['fn', 'g2'], ['y0'], name='nl_y'),
              ow.make_node('Transpose', ['y0'], ['y1'], name='nl_y_t', perm=[0, 2, 1]),
              ow.make_node('Reshape', ['y1', 'map'], ['y2'], name='nl_y_map'),
              ow.make_node('Conv', ['y2', 'wW', 'bW'], ['wy'], name='nl_W', **pw),
              ow.make_node('Add', ['wy', other], ['x'], name='nl_add'),
              ow.make_node('GlobalAveragePool', ['x'], ['p'], name='gap'), ow.make_node('Flatten', ['p'], ['emb'], name='flat_emb', axis=1)]
    g = ow.make_graph(nodes, 'hand', [ow.make_tensor_value_info('input', 1, [1, 3, 32, 16])], [ow.make_tensor_value_info('emb', 1, [1, c])], init)
    return ow.make_model(g).data


def test_hand_block_lowers_with_div_and_with_mul():
    for kw in (dict(), dict(mul=True), dict(x_from='r2', other='r2')):
        g, _ = onnx_graph.lower(hand_block(**kw))
        assert [d['op'] for d in g.layers] == [G.OP_STEMCONV, G.OP_CONV, G.OP_NONLOCAL, G.OP_POOLHEAD]
        d = g.layers[2]
        assert d['cin'] == 8 and (d['out'].h, d['out'].w) == (16, 8) and d['ins'][0].tid == g.layers[0 if 'x_from' not in kw else 1]['out'].tid


REFUSED = {
    'inter_2': dict(kw=dict(inter=2), op='Reshape', node='nl_g_flat', what='inter channels 2: only the one-channel form fast-reid\'s Non_local builds'),
    'div_by_c': dict(kw=dict(divisor=8.0), op='Div', node='nl_div', what='does not match'),
    'mul_by_wrong': dict(kw=dict(divisor=127.0, mul=True), op='Mul', node='nl_div', what='does not match'),
    'softmax': dict(kw=dict(softmax=True), op='Softmax', node='nl_softmax', what='embedded-Gaussian'),
    'add_other': dict(kw=dict(x_from='r2', other='r1'), op='Add', node='nl_add', what='not the block\'s own input'),
    'stray_reader': dict(kw=dict(stray='fn'), op='Relu', node='stray_relu'),
    # (a stray reader sorted behind the block's own node: that node finds two readers)
    'stray_reader_of_theta': dict(kw=dict(stray='theta2'), op='MatMul', node='nl_f', what='something else reads'),
    'unsupported_channels': dict(kw=dict(c=12), op='Add', node='nl_add', what='8 <= C <= 2048'),
}


@pytest.mark.parametrize('case', sorted(REFUSED))
def test_variants_are_refused_by_name(case):
    spec = REFUSED[case]
    with pytest.raises(NotImplementedError) as e:
        onnx_graph.lower(hand_block(**spec['kw']))
    msg = str(e.value)
    assert repr(spec['node']) in msg and f'({spec["op"]})' in msg and spec.get('what', '') in msg
    assert 'Supported: Conv (groups 1' in msg and 'GlobalAveragePool' in msg and 'non-local' in msg


@pytest.mark.parametrize('nl_kw,op,what', [(dict(inter=2), 'Reshape', 'inter channels 2'), (dict(div='C'), 'Div', 'does not match'),
                                           (dict(softmax=True), 'Softmax', 'embedded-Gaussian')])
@pytest.mark.parametrize('folded', [True, False])
def test_edited_modules_are_refused(nl_kw, op, what, folded):
    """The same three through the exporter: the module with two inner channels, with f / C, with a softmax."""
    net = NL.tiny(nl_after={2: [0]}, nl_kw=nl_kw)
    with pytest.raises(NotImplementedError) as e:
        onnx_graph.lower(NL.export(net, folded=folded))
    assert f'({op})' in str(e.value) and what in str(e.value) and '/blocks/blocks.1/blocks.1.1/' in str(e.value)


def test_a_stray_reader_later_in_the_file_is_refused_too():
    """The stray node sorted BEHIND the block's own reader: the block's node finds two readers."""
    data = hand_block(stray='fn')
    m = OnnxModel(data)
    order = [n.name for n in m.nodes]
    assert order.index('stray_relu') < order.index('nl_y')
    i, j = order.index('stray_relu'), order.index('nl_y')
    m.nodes[i], m.nodes[j] = m.nodes[j], m.nodes[i]
    with pytest.raises(NotImplementedError, match=r"'nl_y' \(MatMul\).*something else reads"):
        onnx_graph.lower(m)


def test_unused_block_parameters_are_reported():
    """The "every initialiser must be used" check covers the block: its parameters count as used only through the block."""
    low = onnx_graph._Lowering(OnnxModel(hand_block()), None, None, 'hand')
    low.run()
    assert {'wg', 'bg', 'wtheta', 'btheta', 'wphi', 'bphi', 'wW', 'bW'} <= low.used
    # a block that stops in front of its sum leaves a graph without an embedding: its parameters are not silently dropped
    with pytest.raises(NotImplementedError):
        onnx_graph.lower(hand_block(other='missing'))


# ------------------------------------------------------------------------------------------------ the support rule
def test_nonlocal_supported_agrees_with_the_library():
    lib = _lib.load()
    lib.fm_nonlocal_supported.restype = ctypes.c_int
    lib.fm_nonlocal_supported.argtypes = [ctypes.c_int] * 2
    for c in (-8, 0, 4, 8, 12, 16, 24, 512, 520, 1024, 2040, 2048, 2056, 4096):
        for hw in (-1, 0, 1, 15, 128, 192, 512, 768, 4095, 4096, 4097, 8192):
            assert Graph.nonlocal_supported(c, hw) == bool(lib.fm_nonlocal_supported(c, hw)), (c, hw)
    for hw in (32 * 16, 16 * 8, 48 * 16, 24 * 8):          # the maps of 256 x 128 and 384 x 128 crops
        assert Graph.nonlocal_supported(512, hw) and Graph.nonlocal_supported(1024, hw)
    assert (G.NONLOCAL_MAX_HW, G.NONLOCAL_MAX_C) == (4096, 2048)


# ------------------------------------------------------------------------------------------------ the bound
def case(n, h, w, c):
    g, x = NL.make_case(n, h, w, c)
    bufs, ref, bound = NL.case_reference(g, x)
    return g.layers[0], bufs[g.input.tid], ref, bound


def test_closed_form_is_the_literal_module():
    """The issue's float64 check: the closed form against the module's own text, at its shapes and the test shapes."""
    for c, h, w in [(512, 32, 16), (1024, 16, 8), (24, 5, 3), (8, 1, 1), (2048, 7, 5)]:
        m = NL.seeded(NL.NonLocal(c), c).double()
        x = torch.randn(2, c, h, w, dtype=torch.float64, generator=torch.Generator().manual_seed(c))
        with torch.no_grad():
            want = m(x)
        ref = NL.folded_params(m)
        lit = NL.literal(x, ref)
        closed, _ = NL.nonlocal_(x, ref, track=False)
        assert float((lit - want).abs().max()) <= 1e-13 and float((closed - want).abs().max()) <= 1e-13


@pytest.mark.parametrize('n,h,w,c', NL.CASES)
def test_stand_ins_stay_inside_the_bound(n, h, w, c):
    d, x, ref, bound = case(n, h, w, c)
    s = NL.term(x, d['nl_ref'])[1]
    assert float(s.abs().min()) >= 0.1, s                  # the seeding's promise: |s_n| is O(0.1) or more at every test shape
    for order in ('closed', 'literal', 'reversed'):
        y, _ = NL.nonlocal_(x, d['nl_ref'], dtype=torch.float32, track=False, order=order)
        worst = ibn_ref.check_layer(y.half().float(), ref, bound, f'stand-in {order} {(n, h, w, c)}')
        print(f'stand-in {order:8s} N={n} {h}x{w} C={c}: worst err / bound = {worst:.3f}')


# where each mistake must show (reasoning, not observation):
#   div_c       s scaled by N / C, a term that is hundreds of bounds (the reference's condition) -- except where C == N, and the
#               32 x 16 map of 512 channels is such a shape: there f / C IS f / N
#   batch_s     batches of more than one sample: the samples' s differ by what their own pixels add to the product of the biases,
#               a few per cent of that term
#   swap        theta and phi exchanged: another per-pixel factor (phi's bias is 0.9, theta's a seeded 0.1) and another scalar;
#               not at one pixel, where theta mean(phi g) = theta phi g is symmetric in the two
#   no_w_bias, no_shift   b changes by a seeded value of order 0.1 on every channel, against a bound of 2^-11 |z|
#   theta16     an error of up to 2^-11 |a theta s|.  The bound allows theta (C + 1) u32 sum|w||x|, which grows like C sqrt(C)
#               against |theta|: past a few dozen channels it is more than fp16's 2^-11 |theta|, so the bound cannot tell (and
#               need not: the device's own dot product may be that far off).  It must show wherever the defect itself, computed
#               in float64, exceeds twice the element's bound (one bound may be eaten by the fp16 store's own rounding): that is
#               asserted to happen at C = 24, and checked wherever it happens
MISTAKES = [('div_c', [k for k in NL.CASES if k[3] != k[1] * k[2]]), ('batch_s', [k for k in NL.CASES if k[0] > 1]),
            ('swap', [k for k in NL.CASES if k[1] * k[2] > 1]), ('no_w_bias', NL.CASES), ('no_shift', NL.CASES)]


@pytest.mark.parametrize('mistake,cases', MISTAKES, ids=[m for m, _ in MISTAKES])
def test_planted_mistakes_leave_the_bound(mistake, cases):
    assert len(cases) >= 4
    for n, h, w, c in cases:
        d, x, ref, bound = case(n, h, w, c)
        y, _ = NL.nonlocal_(x, d['nl_ref'], dtype=torch.float32, track=False, mistake=mistake, parts=d['b_parts'])
        with pytest.raises(AssertionError, match='bound'):
            ibn_ref.check_layer(y.half().float(), ref, bound, f'{mistake} {(n, h, w, c)}')


def test_theta_rounded_to_fp16_leaves_the_bound_where_its_size_says_so():
    shown = []
    for n, h, w, c in NL.CASES:
        d, x, ref, bound = case(n, h, w, c)
        wt, bias, a = (torch.from_numpy(np.asarray(d['nl_ref'][i], np.float64)) for i in (0, 3, 4))
        theta = torch.nn.functional.conv2d(x.double(), wt.reshape(1, -1, 1, 1), bias[:1])
        s = NL.term(x, d['nl_ref'])[1].reshape(-1, 1, 1, 1)
        defect = (a.reshape(1, -1, 1, 1) * s * (theta - theta.half().double())).abs()
        if bool((defect > 2 * bound).any()):
            shown.append(c)
            y, _ = NL.nonlocal_(x, d['nl_ref'], dtype=torch.float32, track=False, mistake='theta16')
            with pytest.raises(AssertionError, match='bound'):
                ibn_ref.check_layer(y.half().float(), ref, bound, f'theta16 {(n, h, w, c)}')
    assert 24 in shown, shown
