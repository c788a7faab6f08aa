"""CPU: SSD-MobileNetV1's anchors, layer table and weight sources (fastmot_amd/models/ssd.py, tf_graph_reader.py)."""
import math

import numpy as np
import pytest

import pb_writer as W
import ssd_ref
from fastmot_amd.models import SSD
from fastmot_amd.models import graph as G
from fastmot_amd.models.graph import RandomWeights
from fastmot_amd.models.ssd import SSDMobileNetV1
from fastmot_amd.models.tf_graph_reader import read_constants


class TinySSD(SSDMobileNetV1):
    """Small enough for the tests, and awkward on purpose: not square, maps 10x8, 5x4, 3x2, 2x1, 1x1, 1x1 (both TF SAME
    cases, also one per axis), depth multiplier 0.5."""
    MODEL_PATH = None
    INPUT_SHAPE = (3, 160, 128)
    NUM_CLASSES = 5
    DEPTH_MULTIPLIER = 0.5
    TOPK = 20


def test_anchor_table_300():
    a = SSDMobileNetV1.anchors()
    assert a.shape == (1917, 4) and a.dtype == np.float32
    np.testing.assert_allclose(a[0], [0.5 / 19, 0.5 / 19, 0.1, 0.1], rtol=1e-7)
    np.testing.assert_allclose(a[-1], [0.5, 0.5, math.sqrt(0.95), math.sqrt(0.95)], rtol=1e-7)


@pytest.mark.parametrize('model', [SSDMobileNetV1, TinySSD])
def test_anchor_table_against_the_formulas(model):
    """Direct float64 evaluation, one anchor at a time, of create_ssd_anchors(reduce_boxes_in_lowest_layer=True)."""
    shapes = model.feature_map_shapes()
    lo, hi, n = model.ANCHOR_MIN_SCALE, model.ANCHOR_MAX_SCALE, len(shapes)
    scale = [lo + (hi - lo) * i / (n - 1) for i in range(n)] + [1.0]
    rows = []
    for k, (fh, fw) in enumerate(shapes):
        if k == 0:
            spec = [(0.1, 1.0), (scale[0], 2.0), (scale[0], 0.5)]
        else:
            spec = [(scale[k], r) for r in model.ASPECT_RATIOS] + [(math.sqrt(scale[k] * scale[k + 1]), 1.0)]
        for y in range(fh):
            for x in range(fw):
                for s, r in spec:
                    rows.append(((y + 0.5) / fh, (x + 0.5) / fw, s / math.sqrt(r), s * math.sqrt(r)))
    got = model.anchors()
    assert got.shape == (len(rows), 4)
    np.testing.assert_allclose(got.astype(np.float64), np.array(rows), rtol=2 ** -23, atol=0)
    assert sum(fh * fw * model.anchors_per_cell(k) for k, (fh, fw) in enumerate(shapes)) == len(rows)


def _maps(g):
    out = []
    for d in g.layers:
        hw = g.tensors[d['out'].tid][0]
        if not out or out[-1] != hw:
            out.append(hw)
    return out


def test_full_size_table(monkeypatch):
    g, heads = SSDMobileNetV1.build_graph(RandomWeights(seed=1))
    assert [g.tensors[d['out'].tid][0] for d in g.layers if not g.tensors[d['out'].tid][3]][0] == 150
    sizes = sorted({g.tensors[d['out'].tid][0] for d in g.layers}, reverse=True)
    assert sizes == [150, 75, 38, 19, 10, 5, 3, 2, 1]
    assert SSDMobileNetV1.feature_map_shapes() == [(19, 19), (10, 10), (5, 5), (3, 3), (2, 2), (1, 1)]
    assert [v.c for v in heads] == [3 * 95] + [6 * 95] * 5 and all(g.tensors[v.tid][3] for v in heads)
    assert [(v.h, v.w) for v in heads] == SSDMobileNetV1.feature_map_shapes()
    assert g.layers[0]['op'] == G.OP_STEMCONV and g.layers[0]['pad'] == 0            # 300 is even: TF SAME (0, 1)
    ops = [d['op'] for d in g.layers]
    assert ops.count(G.OP_SEPCONV) == 13 and G.OP_DWCONV not in ops and len(ops) == 1 + 13 + 8 + 6
    assert [d['act'] for d in g.layers[:22]] == [G.ACT['relu6']] * 22 and [d['act'] for d in g.layers[22:]] == [0] * 6
    monkeypatch.setenv('FASTMOT_SEPCONV', '0')
    g2, _ = SSDMobileNetV1.build_graph(RandomWeights(seed=1))
    ops2 = [d['op'] for d in g2.layers]
    assert ops2.count(G.OP_DWCONV) == 13 and G.OP_SEPCONV not in ops2 and len(ops2) == len(ops) + 13
    # the 3x3 stride-2 convs with TF SAME (0, 1) padding are kept off the DMA kernel
    for d in g.layers + g2.layers:
        if d['op'] == G.OP_CONVD:
            assert d['stride'] == 1 or d['pad'] == 1


def test_tiny_table_hits_both_padding_cases():
    g, heads = TinySSD.build_graph(RandomWeights(seed=2))
    assert [(v.h, v.w) for v in heads] == [(10, 8), (5, 4), (3, 2), (2, 1), (1, 1), (1, 1)]
    assert [v.c for v in heads] == [3 * 9] + [6 * 9] * 5
    extra = [d for d in g.layers if d['k'] == 3 and d['op'] in G.CONV_OPS]
    assert [(d['pad'], d['gates']) for d in extra] == [(1, [0]), (1, [0]), (0, [1]), (1, [])]    # 5x4, 3x2, 2x1, 1x1
    assert TinySSD.depth(32) == 16 and TinySSD.depth(1024) == 512 and len(TinySSD.anchors()) == 10 * 8 * 3 + (20 + 6 + 2 + 1 + 1) * 6
    assert SSD.get_model('TinySSD') is TinySSD


def test_other_ssd_models_still_raise():
    for name in ('SSDMobileNetV2', 'SSDInceptionV2'):
        with pytest.raises(NotImplementedError):
            SSD.get_model(name).build_graph()


# ------------------------------------------------------------------------------------------- tf_graph_reader
def test_reader_round_trip():
    rng = np.random.default_rng(0)
    a = rng.normal(size=(3, 3, 4, 5)).astype(np.float32)
    b = rng.normal(size=(7,)).astype(np.float32)
    i = np.array([[1, -2, 300], [4, 5, -70000]], np.int32)
    pb = W.graph_def([W.const_node('a/weights', a), W.op_node('a/weights/read', 'Identity', ['a/weights']),
                      W.const_node('b', b, form='float_val'), W.const_node('ones', np.float32([1.5]), form='scalar', dims=[2, 3]),
                      W.const_node('i', i, form='int_val'), W.const_node('i0', np.int32([7]), form='scalar', dims=[4]),
                      W.const_node('ic', i), W.op_node('relu', 'Relu6', ['a/weights/read'])])
    c = read_constants(pb)
    assert sorted(c) == ['a/weights', 'b', 'i', 'i0', 'ic', 'ones']                 # the non-Const nodes are skipped
    assert np.array_equal(c['a/weights'], a) and c['a/weights'].dtype == np.float32
    assert np.array_equal(c['b'], b) and np.array_equal(c['i'], i) and np.array_equal(c['ic'], i) and c['i'].dtype == np.int32
    assert np.array_equal(c['ones'], np.full((2, 3), 1.5, np.float32)) and np.array_equal(c['i0'], np.full(4, 7, np.int32))


def test_reader_refuses_truncated_input(tmp_path):
    a = np.arange(60, dtype=np.float32).reshape(3, 4, 5)
    pb = W.graph_def([W.const_node('a', a), W.const_node('b', a, form='float_val')])
    full = read_constants(pb)
    assert len(full) == 2
    refused = 0
    for cut in range(1, len(pb)):
        try:
            got = read_constants(pb[:cut])
        except ValueError:
            refused += 1
        else:                           # a cut between two top-level fields is a shorter, valid GraphDef
            assert all(np.array_equal(v, full[k]) for k, v in got.items()) and len(got) < 2 or cut >= len(pb) - 4
    assert refused >= len(pb) - 8
    path = tmp_path / 'cut.pb'
    path.write_bytes(pb[:len(pb) // 2])
    with pytest.raises(ValueError):
        read_constants(path)


def test_frozen_graph_and_mapping_give_the_same_network(tmp_path):
    arrays = ssd_ref.random_variables(TinySSD, seed=3)
    assert set(arrays) == set(TinySSD.variable_shapes())
    pb = W.frozen_graph(arrays)
    g_map, _ = TinySSD.build_graph(arrays)
    g_pb, _ = TinySSD.build_graph(pb)
    (tmp_path / 'tiny.pb').write_bytes(pb)
    np.savez(tmp_path / 'tiny.npz', **arrays)
    g_file, _ = TinySSD.build_graph(tmp_path / 'tiny.pb')
    g_npz, _ = TinySSD.build_graph(tmp_path / 'tiny.npz')
    assert len(g_map.blob) > 100000
    assert bytes(g_map.blob) == bytes(g_pb.blob) == bytes(g_file.blob) == bytes(g_npz.blob)
    bad = dict(arrays)
    del bad['BoxPredictor_3/ClassPredictor/biases']
    with pytest.raises(KeyError):
        TinySSD.build_graph(bad)
    bad = dict(arrays, **{'FeatureExtractor/MobilenetV1/Conv2d_0/weights': np.zeros((3, 3, 3, 8), np.float32)})
    with pytest.raises(ValueError):
        TinySSD.build_graph(bad)
    # BatchNorm is folded with eps 1e-3
    sc = TinySSD.scopes()['stem']
    w = arrays[sc + '/weights'].transpose(3, 2, 0, 1)
    scale = arrays[sc + '/BatchNorm/gamma'] / np.sqrt(arrays[sc + '/BatchNorm/moving_variance'] + 1e-3)
    _, wref, bref = g_map.conv_params[0]
    assert np.array_equal(wref, (w * scale[:, None, None, None]).astype(np.float16).astype(np.float32))
    np.testing.assert_allclose(bref, arrays[sc + '/BatchNorm/beta'] - arrays[sc + '/BatchNorm/moving_mean'] * scale, rtol=1e-6)


def test_missing_model_file_is_an_error(monkeypatch):
    from fastmot_amd.models import graph as graph_mod
    monkeypatch.setattr(graph_mod, '_ALLOW_RANDOM', [False])
    with pytest.raises(FileNotFoundError):
        SSDMobileNetV1.build_graph()
