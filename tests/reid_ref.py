"""TEST INFRASTRUCTURE: float64 restatements of FM_OP_POOLHEAD (csrc/reidhead.hip, Graph.poolhead) and FM_OP_STEMPOOL
(csrc/stempool.hip, Graph.stempool) with their elementwise bounds, and `run_graph` / `run_layer` for layer tables that
hold them.  Every other op goes to
tests/torch_ref.py by import; the bound is built from that module's stages:

    pooled mean over HW pixels, fp32 on the device (HW adds and one division):   d_m = (HW + 1) u32 mean|x|
    BN neck  y = m * s + t  (one multiply, one add, fp32):                       d_y = |s| d_m + 2 u32 (|m s| + |t|)
    FC  f = act(W y + b), fp16 weights held exactly, K = C fp32 accumulations:   d_f = L (|W| d_y + C u32 (|W||y| + |b|))
    L2 normalisation  e = f / n:   d_e = d_f / n' + |f| d_n / (n n') + (2 u32 + 5e-6) |e|,
                                   d_n <= ||d_f||_2 + (D + 2) u32 n,  n' >= n - d_n            (as torch_ref's OP_HEAD)

FM_OP_STEMPOOL is two stages of torch_ref: the conv stage (K = 147, bias, ReLU) whose result the device ROUNDS TO FP16
(store16: d (1 + u16) + u16 |ref| + 2^-24), then a max pool, which only selects: |max a_i - max b_i| <= max |a_i - b_i|, so
the bound of a pooled value is the largest bound in its window; taps outside the conv map do not take part.

`mistake` plants one defect (tests/test_onnx_graph_host.py checks that the bound catches it):
    'mean_hw1'        the mean divides by HW + 1
    'neck_after_fc'   the BN neck is applied to the FC's output instead of its input (needs D == C)
    'pool_pad_zero'   (stempool) the pool pads the conv map with 0 BEFORE the ReLU is applied, i.e. the padding takes part
                      in the maximum of the pre-activation values
    'unrounded'       (stempool) the conv result is not rounded to fp16 before the pool
"""
import copy

import numpy as np
import torch
import torch.nn.functional as F

import resnet_ref
import torch_ref
from fastmot_amd.models import graph as G
from torch_ref import FAST_EXP, U32


def poolhead(x, ref, dtype=torch.float64, track=True, mistake=None):
    """x: [N, C, H, W] (the values the device read: exact fp16 numbers); ref: the layer's poolhead_ref = (scale, shift,
    weight [D, C], bias, relu), None where a stage is absent.  -> (embeddings [N, D], bound or None)."""
    scale, shift, w, b, relu = ref
    it = torch_ref._Interp(None, None, dtype, emulate=not track, track=track)
    x = torch.as_tensor(x).to(dtype)
    hw = x.shape[2] * x.shape[3]
    m, em = it.mean_stage((x, 0.0 if track else None))
    if mistake == 'mean_hw1':
        m = m * hw / (hw + 1)

    def neck(v, e):
        s, t = (torch_ref._t(a, dtype).reshape(1, -1, 1, 1) for a in (scale, shift))
        y = v * s + t
        return y, (s.abs() * e + 2 * U32 * ((v * s).abs() + t.abs()) if track else None)
    if scale is not None and mistake != 'neck_after_fc':
        m, em = neck(m, em)
    if w is not None:
        m, em = it.conv_stage((m, em), np.asarray(w)[:, :, None, None], b, G.ACT['relu'] if relu else G.ACT['linear'])
    if scale is not None and mistake == 'neck_after_fc':
        m, em = neck(m, em)
    fv = m[:, :, 0, 0]
    n = fv.norm(dim=1, keepdim=True)
    ev = fv / n
    if not track:
        return ev, None
    fe = em[:, :, 0, 0]
    dn = fe.norm(dim=1, keepdim=True) + (fv.shape[1] + 2) * U32 * n
    nlo = (n - dn).clamp_min(1e-30)
    return ev, fe / nlo + fv.abs() * dn / (n * nlo) + (2 * U32 + FAST_EXP) * ev.abs()


def stempool(x, ref, dtype=torch.float64, track=True, mistake=None):
    """x: [N, c, H, W] network input; ref: the layer's stempool_ref = (weight [cout, c, 7, 7], bias, pool_pad).
    -> (pooled tensor [N, cout, hp, wp], bound or None)."""
    w, b, ppad = ref
    it = torch_ref._Interp(None, None, dtype, emulate=not track, track=track)
    x = torch.as_tensor(x).to(dtype)[:, :np.asarray(w).shape[1]]
    pads = (ppad, 1, ppad, 1)          # (left, right, top, bottom): pads 1, or pads 0 + ceil_mode = one clipped row / column

    def pool(t, neutral):
        hp, wp = (t.shape[2] + ppad + 1 - 3) // 2 + 1, (t.shape[3] + ppad + 1 - 3) // 2 + 1
        return F.max_pool2d(F.pad(t, pads, value=neutral), 3, 2, 0)[:, :, :hp, :wp]
    if mistake == 'pool_pad_zero':
        pre = it.conv_stage((x, 0.0 if track else None), w, b, G.ACT['linear'], stride=2, padding=3)[0]
        return F.relu(pool(pre, 0.0)).half().to(dtype), None
    y = it.conv_stage((x, 0.0 if track else None), w, b, G.ACT['relu'], stride=2, padding=3)
    v, e = y if mistake == 'unrounded' else it.store16(y)
    return pool(v, float('-inf')), (pool(e, 0.0) if track else None)


def _in_view(d, bufs, dtype):
    v = d['ins'][0]
    return bufs[v.tid][:, v.coff:v.coff + v.c].to(dtype)


def run_layer(graph, idx, bufs, **kw):
    """torch_ref.run_layer for tables that may end in OP_POOLHEAD (kind 'emb')."""
    d = graph.layers[idx]
    if d['op'] == G.OP_STEMPOOL:
        v, e = stempool(_in_view(d, bufs, torch.float64), d['stempool_ref'])
        return 'tensor', v, e
    if d['op'] != G.OP_POOLHEAD:
        return torch_ref.run_layer(graph, idx, bufs, **kw)
    emb, bound = poolhead(_in_view(d, bufs, torch.float64), d['poolhead_ref'])
    return 'emb', emb, bound


def run_graph(graph, x_nchw, emulate_fp16_storage=True):
    """torch_ref.run_graph for tables that end in OP_POOLHEAD: -> (bufs, embeddings)."""
    d = graph.layers[-1]
    first = graph.layers[0]
    head, stem = d['op'] == G.OP_POOLHEAD, first['op'] == G.OP_STEMPOOL
    if not head and not stem:
        return torch_ref.run_graph(graph, x_nchw, emulate_fp16_storage)
    body = copy.copy(graph)
    body.layers = graph.layers[1 if stem else 0:-1 if head else None]
    body.conv_params = [(i - (1 if stem else 0), w, b) for i, w, b in graph.conv_params]

    def around(idx, bufs):
        if stem and idx == 0:       # the fused stem in front of the body's first layer
            y, _ = stempool(_in_view(first, bufs, torch.float32), first['stempool_ref'], dtype=torch.float32, track=False,
                            mistake=None if emulate_fp16_storage else 'unrounded')
            o = first['out']
            bufs[o.tid][:, o.coff:o.coff + o.c] = y
    bufs, emb = torch_ref.run_graph(body, x_nchw, emulate_fp16_storage, around=around)
    if not head:
        return bufs, emb
    emb, _ = poolhead(_in_view(d, bufs, torch.float32), d['poolhead_ref'], dtype=torch.float32, track=False)
    return bufs, emb


def measured_bar(net, g, x):
    """The embedding bar, measured and not guessed: on the CPU, the distance between the fp32 torch module and the
    fp16-STORAGE interpretation of the same table (no code under test involved); the device may differ from the module
    by 4x that -- the margin is for the accumulation order over K (up to 2048 * 9 at ResNet-50).
    -> (module embeddings, 4 x max |delta| per component, 4 x (1 - cosine))."""
    expect = resnet_ref.embed(net, x)
    _, emu = run_graph(g, torch.from_numpy(x), emulate_fp16_storage=True)
    emu = emu.numpy()
    d_abs = float(np.abs(emu - expect).max())
    d_cos = float((1 - np.sum(emu.astype(np.float64) * expect, axis=1)).max())
    return expect, 4 * d_abs, 4 * max(d_cos, 1e-7)          # (1e-7: fp32 rounding of a cosine of two unit vectors)


def check_embeddings(emb, expect, bar_abs, bar_cos, label):
    err = float(np.abs(emb - expect).max())
    cos = float((1 - np.sum(emb.astype(np.float64) * expect, axis=1)).max())
    print(f'EMBEDDING {label}: max |delta| {err:.3g} (bar {bar_abs:.3g}), 1 - cos {cos:.3g} (bar {bar_cos:.3g}); '
          f'OSNet bars (4e-3, 0.99999) {"hold" if err <= 4e-3 and cos <= 1e-5 else "do not hold"}')
    assert err <= bar_abs and cos <= bar_cos, (err, bar_abs, cos, bar_cos)
