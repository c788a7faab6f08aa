"""GPU: the SSD-MobileNetV1 layer table (models/ssd.py) on the conv engine.

Every head tensor against the fp32 torch restatement of the table (tests/ssd_ref.run_table: TF SAME padding, ReLU6,
activations rounded to fp16 where the engine stores them) with the whole-tensor bar of tests/test_fullsize_gpu.py, and
every layer on its own, fed the tensors the device produced, under the per-element bound of DESIGN.md section 7
(tests/ssd_ref.layer_ref).  A sample of a batch-4 pass must equal the batch-1 pass on it within the same bound."""
import numpy as np
import pytest
import torch

import ssd_ref
import torch_ref as T
from fastmot_amd.engine import HipNet, NET_DETECTOR
from fastmot_amd.models import graph as G
from fastmot_amd.models.graph import RandomWeights
from fastmot_amd.models.ssd import SSDMobileNetV1
from test_fullsize_gpu import check_tensor
from test_ssd_topology import TinySSD

pytestmark = pytest.mark.gpu


def _input(model, n, seed):
    _, h, w = model.INPUT_SHAPE
    return np.random.default_rng(seed).uniform(-1, 1, (n, h, w, 3)).astype(np.float16)      # the range normalize() produces


def _device_run(ctx, g, x):
    """-> {tid: [N, cpad, h, w] torch tensor of what the device holds}"""
    n = x.shape[0]
    net = HipNet(ctx, NET_DETECTOR, g, n, reuse_buffers=False)
    net.write(g.input, x)
    net.run(n)
    out = {}
    for tid, (h, w, c, f32) in enumerate(g.tensors):
        a = net.read(G.View(tid, 0, c, h, w), n)
        out[tid] = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2)))
    net.close()
    return out


def _check(ctx, model, n, seed, x=None):
    g, heads = model.build_graph(RandomWeights(seed=seed), max_batch=n)
    x = _input(model, n, seed) if x is None else x
    dev = _device_run(ctx, g, x)
    ref = ssd_ref.run_table(g, torch.from_numpy(np.ascontiguousarray(x.astype(np.float32).transpose(0, 3, 1, 2))))
    for k, hd in enumerate(heads):
        rel, rms = check_tensor(dev[hd.tid][:, :hd.c].numpy(), ref[hd.tid][:, :hd.c].numpy(), f'{model.__name__} head {k}')
        print(f'{model.__name__} batch {n} head {k} {tuple(dev[hd.tid].shape)}: max err / max|ref| {rel:.3g}, rms err / rms {rms:.3g}')
    worst = {}
    for i, d in enumerate(g.layers):
        r, b = ssd_ref.layer_ref(g, i, dev)
        o = d['out']
        ratio = T.check_layer(dev[o.tid][:, o.coff:o.coff + o.c], r, b, f'{model.__name__} layer {i} {T.OP_NAMES[d["op"]]} {d.get("name")}')
        worst[T.OP_NAMES[d['op']]] = max(worst.get(T.OP_NAMES[d['op']], 0.0), ratio)
    print(f'{model.__name__} batch {n}: worst err / bound per op class {worst}')
    return g, heads, x, dev


def test_tiny_ssd_batch_1_and_4(ctx):
    g4, heads, x4, dev4 = _check(ctx, TinySSD, 4, seed=11)
    assert [d['op'] for d in g4.layers].count(G.OP_SEPCONV) == 13
    # sample 2 of the batch-4 pass against the batch-1 pass on it: layer by layer, wherever both passes fed the layer the
    # same input, the batch-4 output lies within the layer's bound around the float64 reference of the batch-1 pass
    g1, _, _, dev1 = _check(ctx, TinySSD, 1, seed=11, x=x4[2:3])
    equal, checked = True, 0
    for i, d in enumerate(g1.layers):
        o, v = d['out'], d['ins'][0]
        got4 = dev4[o.tid][2:3, o.coff:o.coff + o.c]
        equal = equal and torch.equal(got4, dev1[o.tid][:, o.coff:o.coff + o.c])
        if torch.equal(dev4[v.tid][2:3], dev1[v.tid]):
            r, b = ssd_ref.layer_ref(g1, i, dev1)
            T.check_layer(got4, r, b, f'batch-4 sample against the batch-1 reference, layer {i}')
            checked += 1
    print(f'batch-4 sample == batch-1 pass bit for bit: {equal}; {checked} of {len(g1.layers)} layers saw identical inputs')
    assert checked >= 14            # the stem and the 13 separable blocks at the least (no summation order depends on the batch there)
    for hd in heads:                # and the heads, whatever their inputs: the whole-tensor bar
        check_tensor(dev4[hd.tid][2:3, :hd.c].numpy(), dev1[hd.tid][:, :hd.c].numpy(), 'batch-4 sample against the batch-1 pass')


def test_tiny_ssd_unfused(ctx, monkeypatch):
    monkeypatch.setenv('FASTMOT_SEPCONV', '0')
    g, _, _, _ = _check(ctx, TinySSD, 2, seed=12)
    assert [d['op'] for d in g.layers].count(G.OP_DWCONV) == 13


def test_ssd_mobilenet_v1_300_batch_2(ctx):
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    g, heads, _, _ = _check(ctx, SSDMobileNetV1, 2, seed=13)
    assert sum(v.h * v.w * SSDMobileNetV1.anchors_per_cell(k) for k, v in enumerate(heads)) == 1917
