"""torchreid's OSNet-AIN / OSNet-IBN without a device: the restated modules carry torchreid's parameter names, the layer tables
hold the ops the variants need (fused and with FASTMOT_CONVIN=0), the checkpoint loader and the ONNX walker give the same
blob and refuse the wrong variant by name, and the table computes what the module computes.  OSNet's own tables are pinned
byte for byte."""
import hashlib

import numpy as np
import pytest
import torch

import convin_ref
import resnet_ref
import torchreid_osnet as T0
import torchreid_osnet_ain as T
from fastmot_amd import models
from fastmot_amd.models import ReID, graph as G, onnx_reader
from fastmot_amd.models.graph import RandomWeights
from fastmot_amd.models.torchreid_weights import TorchreidWeights

X025, TinyIBN025, small, sd_of = T.X025, T.TinyIBN025, T.small, T.sd_of


def ops(g):
    return [d['op'] for d in g.layers]


def same(a, b, ga, gb):
    """View a of table gb and view b of table ga are the same slice of the tensor that the same block writes (tensor ids
    differ between the tables: the unfused one holds the conv3 tensors)."""
    def writer(g, v):
        d = [d for d in g.layers if d['out'].tid == v.tid][0]
        return '.'.join(d['name'].split('.')[:2]) if d.get('name') else d['op']
    return (a.coff, a.c, a.h, a.w) == (b.coff, b.c, b.h, b.w) and writer(gb, a) == writer(ga, b)


# ------------------------------------------------------------------------------------------------------------ the modules
def test_state_dict_names_are_torchreids():
    ain = set(T.OSNetVariant(X025, 'ain').state_dict())
    ibn = set(T.OSNetVariant(X025, 'ibn').state_dict())
    for keys in (ain, ibn):
        assert {'conv1.conv.weight', 'conv1.bn.weight', 'conv1.bn.bias'} <= keys
        assert not {'conv1.bn.running_mean', 'conv1.bn.running_var', 'conv1.conv.bias'} & keys
    # osnet_ain.py: LightConvStream streams, pool2 / pool3 transitions, OSBlockINin without a conv3 batch norm
    assert {'pool2.0.conv.weight', 'pool2.0.bn.running_var', 'pool3.0.conv.weight', 'conv2.0.conv2.3.layers.3.bn.running_var',
            'conv2.0.conv2.0.layers.0.conv1.weight', 'conv2.0.conv2.3.layers.3.conv2.weight', 'conv2.0.IN.weight',
            'conv2.0.IN.bias', 'conv2.0.conv3.conv.weight', 'conv2.0.downsample.bn.running_mean', 'conv3.0.conv3.bn.weight'} <= ain
    for blk, inin in (('conv2.0', True), ('conv2.1', True), ('conv3.0', False), ('conv3.1', True), ('conv4.0', True), ('conv4.1', False)):
        assert (f'{blk}.IN.weight' in ain) == inin and (f'{blk}.conv3.bn.weight' in ain) == (not inin)
        assert f'{blk}.IN.running_mean' not in ain and f'{blk}.conv3.conv.bias' not in ain
    assert not any(k.startswith(('conv2.2.', 'conv3.2.')) or '.conv2a.' in k for k in ain)
    # osnet.py with IN=True: OSNet's names plus .IN in conv2 / conv3
    plain = set(T0.OSNet(X025).state_dict())
    extra = {f'{b}.IN.{p}' for b in ('conv2.0', 'conv2.1', 'conv3.0', 'conv3.1') for p in ('weight', 'bias')}
    assert ibn == (plain - {'conv1.bn.running_mean', 'conv1.bn.running_var', 'conv1.bn.num_batches_tracked'}) | extra


# ------------------------------------------------------------------------------------------------------------ the tables
def build(name_or_desc, monkeypatch, convin=True, weights=None):
    monkeypatch.setenv('FASTMOT_CONVIN', '1' if convin else '0')
    desc = ReID.get_model(name_or_desc) if isinstance(name_or_desc, str) else name_or_desc
    g, _ = desc.build_graph(weights if weights is not None else RandomWeights(seed=1))
    return g


@pytest.mark.parametrize('name,n_layers', [('OSNetAIN10', 53), ('OSNetIBN10', 51), ('OSNetAIN025', 35)])
def test_tables_hold_the_variants_ops(name, n_layers, monkeypatch):
    g = build(name, monkeypatch)
    desc = ReID.get_model(name)
    o = ops(g)
    assert len(o) == n_layers and o.count(G.OP_CONVIN) == 4 and o.count(G.OP_INSTNORM) == 1 and o[1] == G.OP_INSTNORM
    assert o[0] in G.CONV_OPS + (G.OP_STEMCONV,) and g.layers[0]['act'] == G.ACT['linear'] and o[2] == G.OP_MAXPOOL
    assert g.layers[1]['act'] == G.ACT['relu'] and g.layers[1]['hid'] == desc.CHANNELS[0] and G.OP_OSTAIL not in o
    tails = [d for d in g.layers if d['op'] == G.OP_CONVIN]
    if desc.VARIANT == 'ain':
        assert [d['name'] for d in tails] == ['conv2.0.conv3', 'conv2.1.conv3', 'conv3.1.conv3', 'conv4.0.conv3']
        assert all(d['res_mode'] == G.RES_AFTER_NORM and d['res'] is not None and d['act'] == G.ACT['relu'] for d in tails)
        assert all(not np.any(d['convin_ref'][1]) for d in tails)                       # Conv1x1Linear(bn=False): no bias
        # INin down blocks: `down` is a linear conv into its own tensor, the tail reads x2 alone (no concat tensor)
        for d in (tails[0], tails[3]):
            assert d['cin'] == d['cout'] // 4 and g.tensors[d['ins'][0].tid][2] == d['cin']
            down = [e for e in g.layers if e.get('name') == d['name'].replace('conv3', 'down')][0]
            assert down['act'] == G.ACT['linear'] and down['out'].tid == d['res'].tid and down['op'] in G.CONV_OPS
        # the plain down block conv3.0 keeps OSNet's concat form
        assert any(e.get('name') == 'conv3.0.conv3+down' and e['op'] in G.CONV_OPS for e in g.layers)
    else:
        c0, c1, c2, _ = desc.CHANNELS
        assert [(d['name'], d['cin']) for d in tails] == [('conv2.0.conv3+down', c1 // 4 + c0), ('conv2.1.conv3', c1 // 4),
                                                          ('conv3.0.conv3+down', c2 // 4 + c1), ('conv3.1.conv3', c2 // 4)]
        assert [d['res_mode'] for d in tails] == [G.RES_NONE, G.RES_BEFORE_NORM, G.RES_NONE, G.RES_BEFORE_NORM]
    g.tables(4, reuse=True)


def test_ostail_fuses_ibn_at_quarter_width_and_never_ain(monkeypatch):
    g = build(TinyIBN025, monkeypatch)
    assert g.layers[-1]['op'] == G.OP_OSTAIL and ops(g).count(G.OP_CONVIN) == 4
    g = build('OSNetAIN025', monkeypatch)
    assert G.OP_OSTAIL not in ops(g) and g.layers[-1]['op'] == G.OP_HEAD
    assert g.fuse_ostail(len(g.layers) - 11) is False


class Recording(RandomWeights):
    def __init__(self, seed):
        super().__init__(seed)
        self.drawn = []

    def conv(self, name, *a, **kw):
        self.drawn.append(name)
        return super().conv(name, *a, **kw)

    def instnorm(self, name, c):
        self.drawn.append(name)
        return super().instnorm(name, c)


@pytest.mark.parametrize('name', ['OSNetAIN10', 'OSNetIBN10', 'OSNetAIN025'])
def test_unfused_table_has_one_layer_more_per_in_block(name, monkeypatch):
    wf, wu = Recording(3), Recording(3)
    fused, unfused = build(name, monkeypatch, True, wf), build(name, monkeypatch, False, wu)
    assert wf.drawn == wu.drawn and len(wf.drawn) == len(set(wf.drawn))            # equal parameter draw order
    assert len(unfused.layers) == len(fused.layers) + 4 and G.OP_CONVIN not in ops(unfused)
    assert ops(unfused).count(G.OP_INSTNORM) == 5
    it = iter(unfused.layers)
    for d in fused.layers:
        e = next(it)
        if d['op'] != G.OP_CONVIN:
            assert e['op'] == d['op'] and e.get('name') == d.get('name')
            continue
        n = next(it)
        assert e['op'] in G.CONV_OPS and e['act'] == G.ACT['linear'] and n['op'] == G.OP_INSTNORM and n['act'] == G.ACT['relu']
        w, b, gamma, beta, eps = d['convin_ref']
        cw, cb = {i: (w_, b_) for i, w_, b_ in unfused.conv_params}[unfused.layers.index(e)]
        assert np.array_equal(cw, w) and np.array_equal(cb, b)
        assert np.array_equal(n['instnorm_ref'][0], gamma) and np.array_equal(n['instnorm_ref'][1], beta) and n['instnorm_ref'][2] == eps
        if d['res_mode'] == G.RES_AFTER_NORM:
            assert same(n['res'], d['res'], fused, unfused) and e['res'] is None
        elif d['res_mode'] == G.RES_BEFORE_NORM:
            assert same(e['res'], d['res'], fused, unfused) and e['res_mode'] == G.RES_BEFORE_ACT and n['res'] is None


# hashed once on the parent commit: sha256 of the blob and of the fm_layer table (max_batch 4, reuse) with RandomWeights(seed=1)
PARENT = {'OSNet025': ('a225a0b8bbf08a2f13a341ecf31ab8622742a4d040de87721961ead03bb73a09',
                       '598d11456000fc6ab7de4b1c7b3a4150602e3123ecd9e7992586b0048d3b3e60', 22),
          'OSNet10': ('3da75d947a3845b7dfab5791fa14dcd5adde431dc21c1b6c392333d06d5a11ea',
                      'c1be56cdd72b2c12e6ac745fff74c1c2802d6b8c334b8531e15f6985d89fb1de', 50)}


@pytest.mark.parametrize('name', sorted(PARENT))
def test_osnet_tables_are_the_parents_byte_for_byte(name, monkeypatch):
    monkeypatch.delenv('FASTMOT_CONVIN', raising=False)
    g, _ = ReID.get_model(name).build_graph(RandomWeights(seed=1))
    _, ls, blob = g.tables(4, reuse=True)
    assert (hashlib.sha256(blob).hexdigest(), hashlib.sha256(bytes(ls)).hexdigest(), len(g.layers)) == PARENT[name]


# ------------------------------------------------------------------------------------------------------------ the loaders
VARIANTS = [('ain', 'OSNetAIN025'), ('ibn', TinyIBN025)]


@pytest.mark.parametrize('variant,desc', VARIANTS, ids=['ain', 'ibn'])
def test_state_dict_pth_and_onnx_give_the_same_blob(variant, desc, tmp_path, monkeypatch):
    monkeypatch.delenv('FASTMOT_CONVIN', raising=False)
    desc = small(ReID.get_model(desc) if isinstance(desc, str) else desc)
    net = T.random_variant(X025, variant, seed=4)
    w0 = TorchreidWeights(sd_of(net), variant)
    g0, _ = desc.build_graph(w0)
    assert w0.unused() == []                                            # every parameter is used (the classifier is expected)
    pth = tmp_path / 'model.pth.tar'
    torch.save({'state_dict': {'module.' + k: v for k, v in net.state_dict().items()}}, pth)
    w1 = TorchreidWeights(pth, variant)
    g1, _ = desc.build_graph(w1)
    assert bytes(g1.blob) == bytes(g0.blob) and w1.unused() == []
    data = resnet_ref.export_with_torch(net, torch.randn(1, 3, 64, 32), training=torch.onnx.TrainingMode.PRESERVE,
                                        do_constant_folding=False, keep_initializers_as_inputs=True)
    m = onnx_reader.OnnxModel(data)
    assert sum(n.op == 'InstanceNormalization' for n in m.nodes) == 5
    sd = onnx_reader.torchreid_state_dict_from_onnx(m, X025, 512, variant)
    assert set(sd) == {k for k in sd_of(net) if not k.startswith('classifier') and not k.endswith('num_batches_tracked')}
    w2 = TorchreidWeights(sd, variant)
    g2, _ = desc.build_graph(w2)
    assert bytes(g2.blob) == bytes(g0.blob) and ops(g2) == ops(g0) and w2.unused() == []
    # the exporter's default (BatchNorm folded into the convs) walks too, and through the descriptor's MODEL_PATH
    path = tmp_path / 'model.onnx'
    path.write_bytes(resnet_ref.export_with_torch(net, torch.randn(1, 3, 64, 32)))
    monkeypatch.setattr(desc, 'MODEL_PATH', path)
    g3, _ = desc.build_graph()
    assert ops(g3) == ops(g0) and len(g3.blob) == len(g0.blob)


def test_wrong_variant_fails_by_name():
    nets = {v: T.random_variant(X025, v, seed=4) for v in ('ain', 'ibn')}
    nets['osnet'] = T0.random_osnet(X025, seed=4)
    descs = {'ain': small(ReID.get_model('OSNetAIN025')), 'ibn': small(TinyIBN025), 'osnet': small(ReID.get_model('OSNet025'))}
    expect = {('osnet', 'ain'): 'conv1.bn.running_mean', ('osnet', 'ibn'): 'conv1.bn.running_mean',
              ('ibn', 'ain'): 'conv2.0.conv2.0.layers.0.conv1.weight', ('ain', 'ibn'): 'conv2.0.conv2a.conv1.weight',
              ('ain', 'osnet'): 'conv1.bn.running_mean', ('ibn', 'osnet'): 'conv1.bn.running_mean'}
    for (have, want), key in expect.items():
        with pytest.raises(KeyError, match=key.replace('.', r'\.')):
            descs[want].build_graph(TorchreidWeights(sd_of(nets[have]), want))
    exports = {v: resnet_ref.export_with_torch(n, torch.randn(1, 3, 64, 32)) for v, n in nets.items()}
    for have in exports:
        for want in exports:
            if have == want:
                onnx_reader.torchreid_state_dict_from_onnx(exports[have], X025, 512, want)
                continue
            with pytest.raises(ValueError, match=f"variant '{want}'"):
                onnx_reader.torchreid_state_dict_from_onnx(exports[have], X025, 512, want)
    with pytest.raises(ValueError, match='variant'):
        TorchreidWeights({}, 'osnet_ain')


@pytest.mark.parametrize('variant,desc', VARIANTS, ids=['ain', 'ibn'])
@pytest.mark.parametrize('convin', [True, False])
def test_table_computes_what_the_module_computes(variant, desc, convin, monkeypatch):
    """torch module -> state_dict -> layer table -> the CPU interpreter in fp32 == the module's own embeddings."""
    monkeypatch.setenv('FASTMOT_CONVIN', '1' if convin else '0')
    desc = small(ReID.get_model(desc) if isinstance(desc, str) else desc)
    net = T.random_variant(X025, variant, seed=2)
    x = resnet_ref.random_input(3, (64, 32), seed=1)
    expect = resnet_ref.embed(net, x)
    g, _ = desc.build_graph(TorchreidWeights(sd_of(net), variant))
    assert (G.OP_CONVIN in ops(g)) == convin
    _, emb = convin_ref.run_graph(g, torch.from_numpy(x), emulate_fp16_storage=False)
    emb = emb.numpy()
    assert np.abs(emb - expect).max() < 5e-3 and (np.sum(emb * expect, axis=1) > 0.9999).all()


def test_registry_and_files():
    for name, stem, ch in (('OSNetAIN10', 'osnet_ain_x1_0', (64, 256, 384, 512)), ('OSNetIBN10', 'osnet_ibn_x1_0', (64, 256, 384, 512)),
                           ('OSNetAIN025', 'osnet_ain_x0_25', X025)):
        d = ReID.get_model(name)
        assert d.MODEL_PATH.name == stem + '.onnx' and d.CHANNELS == ch and d.METRIC == 'cosine' and d.OUTPUT_LAYOUT == 512
    assert ReID.get_model('OSNet10').VARIANT == 'osnet' and models.ReID is ReID
