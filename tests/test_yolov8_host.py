"""CPU: YOLOv8 from ONNX -- the lowering (models/onnx_detector.py), the closed form of the decode and its bound
(tests/yolov8_ref.py), the descriptors.  oracle=restated: Ultralytics' modules in plain torch (yolov8_ref)."""
import copy

import numpy as np
import pytest
import torch

import onnx_writer as W
import torch_ref
import yolov8_ref as R
from fastmot_amd import models
from fastmot_amd.models import graph as G
from fastmot_amd.models import onnx_detector as D
from fastmot_amd.models.onnx_reader import OnnxModel

HW = R.TINY_HW
STRIDES = [8, 16, 32]


@pytest.fixture(scope='module')
def net():
    return R.tiny(nc=3)


@pytest.fixture(scope='module')
def x():
    return np.random.default_rng(0).uniform(0, 1, (1, 3) + HW).astype(np.float32)


@pytest.fixture(scope='module')
def folded(net):
    return R.export(net, HW, folded=True)


# ------------------------------------------------------------------------------------------------ a third exporter form
def _module_shapes(m):
    """(c, h, w) of every map of a FOLDED torch export of a yolov8_ref module, from what the module is known to do and not
    from the lowering under test: convs pad k // 2 (output ceil(in / stride)), `chunk(2, 1)` halves its input (the Slice
    nodes of one parent, in order), `Upsample` doubles, everything else keeps or adds channels.  -> (shape, view_of: slice
    output -> (parent, offset, channels), users: value -> [op of each reader])."""
    shape, view_of, users = {'input': (3,) + HW}, {}, {}
    for nd in m.nodes:
        for t in nd.inputs:
            users.setdefault(t, []).append(nd.op)
    for nd in m.nodes:
        ins = [t for t in nd.inputs if t in shape]
        if not ins or ins[0] != nd.inputs[0]:
            continue
        c, h, w = shape[ins[0]]
        out = nd.outputs[0]
        if nd.op == 'Conv':
            st = nd.attrs['strides'][0]
            shape[out] = (m.tensor(nd.inputs[1]).shape[0], -(-h // st), -(-w // st))
        elif nd.op in ('Sigmoid', 'MaxPool'):
            shape[out] = (c, h, w)
        elif nd.op in ('Mul', 'Add') and len(ins) == 2:
            shape[out] = (c, h, w)
        elif nd.op == 'Concat' and len(ins) == len(nd.inputs):
            shape[out] = (sum(shape[t][0] for t in ins), h, w)
        elif nd.op == 'Resize':
            shape[out] = (c, 2 * h, 2 * w)
        elif nd.op == 'Slice':
            k = sum(1 for p, _, _ in view_of.values() if p == ins[0])
            shape[out] = (c // 2, h, w)
            view_of[out] = (ins[0], k * (c // 2), c // 2)
    return shape, view_of, users


def simplified(source, nc=3, softmax=True, dfl_weights=None, offset=0.5, strides=None, reg_max=16, extra_init=False,
               group_of=None, matmul=False, second_output=False):
    """The network of a torch export rewritten as a simplifier leaves it, with tests/onnx_writer.py: every constant an
    initialiser, `Split` instead of the Slice pairs, no shape arithmetic, the anchors and strides as one constant each.
    The keyword arguments plant the defects the lowering has to refuse."""
    m = OnnxModel(source)
    nodes, inits, alias = [], [], {}
    const = lambda name, a, t=W.TensorProto.FLOAT: inits.append(W.make_tensor(name, t, list(np.shape(a)), np.asarray(a).reshape(-1)))  # noqa: E731
    shape, view_of, users = _module_shapes(m)
    heads, n_split = [], 0
    keep = ('Conv', 'Sigmoid', 'Mul', 'Add', 'Concat', 'MaxPool', 'Resize')
    for nd in m.nodes:
        if nd.outputs[0] not in shape:
            continue
        ins = [alias.get(t, t) for t in nd.inputs]
        if nd.op in ('Slice', 'Split'):
            parent = nd.inputs[0]
            views = sorted((v for v, (p, _, _) in view_of.items() if p == parent), key=lambda v: view_of[v][1])
            if nd.outputs[0] == views[0]:
                n_split += 1
                nodes.append(W.make_node('Split', [alias.get(parent, parent)], views, name=f'split{n_split}', axis=1,
                                         split=[view_of[v][2] for v in views]))
            continue
        if nd.op not in keep:
            continue
        at = {k: v for k, v in nd.attrs.items()}
        if nd.op == 'Conv':
            for t in ins[1:]:
                const(t, m.tensor(t))
            if group_of == nd.name:
                at['group'] = 2
            us = users.get(nd.outputs[0], [])
            if 'Sigmoid' not in us:
                heads.append(nd.outputs[0])
        if nd.op == 'Resize':
            const(nd.outputs[0] + '_scales', [1, 1, 2, 2])
            ins = [ins[0], '', nd.outputs[0] + '_scales']
        if nd.op == 'Concat' and all(t in heads for t in nd.inputs):
            continue                                        # (the tail is written below)
        nodes.append(W.make_node(nd.op, ins, nd.outputs, name=nd.name, **at))
        if matmul and nd.name == '/b1/Mul':                 # (an attention-style product of an activated map)
            const('mm_w', np.eye(shape[nd.outputs[0]][2], dtype=np.float32))
            nodes.append(W.make_node('MatMul', [nd.outputs[0], 'mm_w'], ['mm_out'], name='attn_matmul'))
    levels = [(heads[i], heads[i + 1]) for i in range(0, len(heads), 2)]
    strides = strides or STRIDES[:len(levels)]
    flat, pts, st = [], [], []
    for i, ((box, cls), s) in enumerate(zip(levels, strides)):
        _, gh, gw = shape[cls]
        nodes.append(W.make_node('Concat', [box, cls], [f'lv{i}'], name=f'cat_lv{i}', axis=1))
        const(f'shape_lv{i}', [1, 4 * reg_max + nc, gh * gw], W.TensorProto.INT64)
        nodes.append(W.make_node('Reshape', [f'lv{i}', f'shape_lv{i}'], [f'flat{i}'], name=f'reshape_lv{i}'))
        flat.append(f'flat{i}')
        cell = np.arange(gh * gw)
        pts.append(np.stack([cell % gw + offset, cell // gw + offset]))
        st.append(np.full(gh * gw, float(s)))
    A = sum(len(v) for v in st)
    const('anchors', np.concatenate(pts, 1)[None])
    const('strides', np.concatenate(st)[None])
    const('dfl_w', np.arange(reg_max, dtype=np.float32).reshape(1, reg_max, 1, 1) if dfl_weights is None else dfl_weights)
    const('shape_dfl', [1, 4, reg_max, A], W.TensorProto.INT64)
    const('shape_d', [1, 4, A], W.TensorProto.INT64)
    const('two', [2.0])
    n = lambda *a, **k: nodes.append(W.make_node(*a, **k))            # noqa: E731
    n('Concat', flat, ['x_cat'], name='cat_levels', axis=2)
    n('Split', ['x_cat'], ['box', 'cls'], name='split_box_cls', axis=1, split=[4 * reg_max, nc])
    n('Reshape', ['box', 'shape_dfl'], ['b4'], name='dfl_reshape')
    n('Transpose', ['b4'], ['b4t'], name='dfl_t0', perm=[0, 1, 3, 2])
    if softmax:
        n('Softmax', ['b4t'], ['sm'], name='dfl_softmax', axis=3)
    n('Transpose', ['sm' if softmax else 'b4t'], ['smt'], name='dfl_t1', perm=[0, 3, 1, 2])
    n('Conv', ['smt', 'dfl_w'], ['dexp'], name='dfl_conv', kernel_shape=[1, 1])
    n('Reshape', ['dexp', 'shape_d'], ['d'], name='dfl_out')
    n('Split', ['d'], ['lt', 'rb'], name='split_lt_rb', axis=1, split=[2, 2])
    n('Sub', ['anchors', 'lt'], ['x1y1'], name='sub_lt')
    n('Add', ['anchors', 'rb'], ['x2y2'], name='add_rb')
    n('Add', ['x1y1', 'x2y2'], ['csum'], name='add_c')
    n('Div', ['csum', 'two'], ['cxy'], name='div_c')
    n('Sub', ['x2y2', 'x1y1'], ['wh'], name='sub_wh')
    n('Concat', ['cxy', 'wh'], ['dbox'], name='cat_box', axis=1)
    n('Mul', ['dbox', 'strides'], ['dbox_s'], name='mul_strides')
    n('Sigmoid', ['cls'], ['prob'], name='cls_sigmoid')
    n('Concat', ['dbox_s', 'prob'], ['output'], name='cat_out', axis=1)
    if extra_init:
        const('left_over', [1.0, 2.0])
    outs = [W.make_tensor_value_info('output', W.TensorProto.FLOAT, [1, 4 + nc, A])]
    if second_output:
        outs.append(W.make_tensor_value_info('prob', W.TensorProto.FLOAT, [1, nc, A]))
    graph = W.make_graph(nodes, 'v8', [W.make_tensor_value_info('input', W.TensorProto.FLOAT, [1, 3, HW[0], HW[1]])], outs, inits)
    return W.make_model(graph).SerializeToString()


def _table(g):
    """What makes two tables the same network: every layer's op, geometry and wiring."""
    view = lambda v: None if v is None else (v.tid, v.coff, v.c, v.h, v.w)      # noqa: E731
    return ([(d['op'], d['cin'], d['cout'], d['k'], d['stride'], d['pad'], d['act'], d['up'], d['res_mode'],
              [view(v) for v in d['ins']], view(d['out']), view(d['res'])) for d in g.layers], list(g.tensors))


def _head_arrays(g, info, bufs):
    return [(bufs[b.tid][0, b.coff:b.coff + b.c].numpy(), bufs[c.tid][0, c.coff:c.coff + c.c].numpy()) for b, c in info.levels]


# ------------------------------------------------------------------------------------------------ closed form
def test_closed_form_is_the_modules_own_tail(net, x):
    net64 = copy.deepcopy(net).double()
    with torch.no_grad():
        y = net64(torch.as_tensor(x, dtype=torch.float64)).numpy()[0]
    heads = [(b[0].numpy(), c[0].numpy()) for b, c in net64.detect.heads]
    dec = R.dfl_decode(heads, STRIDES, HW)
    mine = R.ultralytics_output(dec, heads)
    assert mine.shape == y.shape == (7, 126)
    np.testing.assert_allclose(mine, y, rtol=1e-12, atol=1e-11)
    np.testing.assert_allclose(D.closed_form([(b[None], c[None]) for b, c in heads], STRIDES, HW)[0], y, rtol=1e-12, atol=1e-11)
    # level-major numbering: anchor 96 is cell (0, 0) of the 4 x 6 level
    assert abs((dec['x1'][96] + dec['x2'][96]) / 2 - mine[0, 96]) < 1e-9 and mine.shape[1] == 96 + 24 + 6


def test_three_exporter_forms_give_one_table(net, x, folded):
    tables, heads = [], []
    for src in (folded, R.export(net, HW, folded=False), simplified(folded)):
        g, info = D.lower(src)
        assert info.strides == STRIDES and info.num_classes == 3 and info.in_hw == HW
        tables.append(_table(g))
        bufs, _ = torch_ref.run_graph(g, torch.from_numpy(x))
        heads.append(_head_arrays(g, info, bufs))
        ops = [d['op'] for d in g.layers]
        assert ops[0] == G.OP_STEMCONV and ops.count(G.OP_SPP) == 1 and ops.count(G.OP_UPSAMPLE2) == 2
        assert G.OP_COPY not in ops and G.OP_MAXPOOL not in ops and G.OP_ADD not in ops
        assert sum(d['res'] is not None for d in g.layers) == 4            # the backbone's four shortcut bottlenecks
    assert tables[0] == tables[1] == tables[2]
    _, want = R.module_heads(net, x)
    for got in heads:
        for (gb, gc), (wb, wc) in zip(got, want):
            for a, b in ((gb, wb[0]), (gc, wc[0])):
                assert np.abs(a - b).max() <= 2e-2 * np.abs(b).max() + 2e-3      # (fp16 storage against fp32: the project's bar)
    for a, b in zip(heads[0], heads[2]):            # the same initialisers, read through two writers: the same bits
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_sppf_as_one_spp_launch_equals_three_pools(x, folded):
    g1, i1 = D.lower(folded)
    g3, i3 = D.lower(folded, sppf_as_spp=False)
    assert [d['op'] for d in g3.layers].count(G.OP_MAXPOOL) == 3 and len(g1.layers) == len(g3.layers) - 2
    b1, _ = torch_ref.run_graph(g1, torch.from_numpy(x))
    b3, _ = torch_ref.run_graph(g3, torch.from_numpy(x))
    for (a, b), (c, d) in zip(_head_arrays(g1, i1, b1), _head_arrays(g3, i3, b3)):
        assert np.array_equal(a, c) and np.array_equal(b, d)


def test_two_levels_and_other_class_counts():
    for nc, levels in ((1, 2), (80, 3)):
        g, info = D.lower(R.export(R.tiny(nc=nc, levels=levels), HW))
        assert info.num_classes == nc and info.strides == STRIDES[:levels] and len(g.outputs) == 2 * levels
        assert all(g.tensors[v.tid][3] == 1 for v in g.outputs)            # fp32 head tensors


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize('kw,match', [
    (dict(softmax=False), "output 'output'"),
    (dict(dfl_weights=np.arange(16, dtype=np.float32)[::-1].reshape(1, 16, 1, 1).copy()), "output 'output'"),
    (dict(offset=0.0), "output 'output'"),
    (dict(strides=[8, 16, 16]), "output 'output'"),
    (dict(group_of='/b1/conv/Conv'), '/b1/conv/Conv.*group'),
    (dict(matmul=True), 'attn_matmul'),
    (dict(second_output=True), "second graph output 'prob'"),
    (dict(extra_init=True), 'left_over'),
])
def test_refusals_name_the_node(folded, kw, match):
    with pytest.raises((NotImplementedError, ValueError), match=match):
        D.lower(simplified(folded, **kw))


def test_reg_max_8_is_refused():
    net = R.seeded_v8(R.YOLOv8((16, 16, 16, 32, 32), (1, 1, 1, 1), 3), 5)
    net.detect = R.Detect(3, (16, 32, 32), (8, 16, 32), reg_max=8)
    R.seeded_v8(net, 5)
    with pytest.raises(NotImplementedError, match='reg_max = 8'):
        D.lower(R.export(net, HW))


def test_dynamic_input_is_refused(folded):
    m = OnnxModel(folded)
    m.inputs[0] = ('input', [None, 3, 64, 96])
    m.data_inputs = [m.inputs[0]]
    with pytest.raises(NotImplementedError, match='dynamic'):
        D.lower(m)


def test_descriptor_shape_mismatch(tmp_path, folded):
    path = tmp_path / 'tiny.onnx'
    path.write_bytes(folded)

    class WrongShapeV8(models.YOLO):
        MODEL_PATH, HEAD, INPUT_SHAPE, NUM_CLASSES = path, 'dfl', (3, 64, 64), 3

    class WrongClassesV8(models.YOLO):
        MODEL_PATH, HEAD, INPUT_SHAPE, NUM_CLASSES = path, 'dfl', (3, 64, 96), 80

    class RightV8(models.YOLO):
        MODEL_PATH, HEAD, INPUT_SHAPE, NUM_CLASSES = path, 'dfl', (3, 64, 96), 3
    with pytest.raises(ValueError, match='INPUT_SHAPE'):
        WrongShapeV8.build_graph()
    with pytest.raises(ValueError, match='NUM_CLASSES'):
        WrongClassesV8.build_graph()
    g, info = RightV8.build_graph()
    assert info.strides == STRIDES


# ------------------------------------------------------------------------------------------------ the decode bound
def _bound_case():
    rng = np.random.default_rng(7)
    heads = []
    for gh, gw in ((8, 12), (4, 6), (2, 3)):
        box = rng.normal(0, 3, (64, gh, gw)).astype(np.float32)
        cls = np.round(rng.normal(0, 2, (5, gh, gw))).astype(np.float32)       # rounded: ties between classes
        box[5] += 30
        box[37] -= 30
        heads.append((box, cls))
    return heads


@pytest.mark.parametrize('mistake', [None, 'offset', 'lt', 'grid', 'last', 'nomax'])
def test_bound_passes_the_decode_and_fails_planted_mistakes(mistake):
    heads = _bound_case()
    if mistake == 'nomax':
        heads = [(b + np.float32(80), c) for b, c in heads]          # exp(110) overflows fp32 without the subtraction
    size, offset = (1920.0, 1280.0), (0.0, 100.0)
    dec = R.dfl_decode(heads, STRIDES, HW)
    rows, bound = R.dfl_rows(dec, HW, size, offset)
    got = R.dfl_rows_fp32(heads, STRIDES, HW, size, offset, mistake)
    ok = (np.abs(got - rows) <= bound).all()
    assert ok == (mistake is None)
    if mistake is None:
        assert (bound[:, :4] < 0.05).all() and (bound[:, 6] < 1e-6).all()      # (pixels of a 1920-wide frame: the mistakes move boxes by >= 4 px)


# ------------------------------------------------------------------------------------------------ descriptors
def test_from_onnx_registers_a_descriptor(tmp_path, folded):
    path = tmp_path / 'my-v8.onnx'
    path.write_bytes(folded)
    M = models.YOLO.from_onnx(path)
    assert M.__name__ == 'my_v8' and models.YOLO.get_model('my_v8') is M
    assert (M.HEAD, M.TOPOLOGY, M.INPUT_SHAPE, M.NUM_CLASSES, M.LAYER_FACTORS, M.LETTERBOX, M.FRONT_LAYERS) == \
        ('dfl', 'onnx', (3, 64, 96), 3, STRIDES, True, 0)
    assert models.YOLO.from_onnx(path, name='V8NoBox', letterbox=False).LETTERBOX is False
    g, info = M.build_graph()
    assert len(info.levels) == 3
    with pytest.raises(TypeError, match='weights='):
        M.build_graph(weights=G.RandomWeights(0))
    with pytest.raises(FileNotFoundError):
        models.YOLO.from_onnx(tmp_path / 'missing.onnx')


def test_shipped_descriptors_need_their_file():
    for name in ('YOLOv8n', 'YOLOv8s', 'YOLOv8m', 'YOLOv8l', 'YOLOv8x'):
        M = models.YOLO.get_model(name)
        assert (M.HEAD, M.INPUT_SHAPE, M.NUM_CLASSES, M.LETTERBOX) == ('dfl', (3, 640, 640), 80, True)
        assert M.MODEL_PATH.name == name.lower() + '.onnx'
        if not M.MODEL_PATH.is_file():
            with pytest.raises(FileNotFoundError):          # (also with random weights allowed: there is no built-in topology)
                M.build_graph()
