"""TEST INFRASTRUCTURE for fast-reid's non-local blocks (models/onnx_graph.py, FM_OP_NONLOCAL in csrc/nonlocal.hip): the
`Non_local` module of fastreid/layers/non_local.py (the text of the AGW authors' ReID-Survey code) restated in plain torch,
a ResNet with such blocks on top of tests/resnet_ref.py / tests/ibn_ref.py, its ONNX export in both exporter forms, the
float64 reference of the device op with its elementwise bound, and `run_layer` / `run_graph` / `measured_bar` for layer
tables that hold it (every other op goes to tests/ibn_ref.py, tests/reid_ref.py and tests/torch_ref.py).

The module, literally (inter = reduc_ratio // reduc_ratio == 1: the published quirk; g, theta, phi are C -> 1 convs with bias):
    g_x     = g(x).view(B, inter, -1).permute(0, 2, 1)            [B, N, 1]   N = H * W
    theta_x = theta(x).view(B, inter, -1).permute(0, 2, 1)        [B, N, 1]
    phi_x   = phi(x).view(B, inter, -1)                           [B, 1, N]
    f       = matmul(theta_x, phi_x) / N                          [B, N, N]   dot-product form: no softmax
    y       = matmul(f, g_x).permute(0, 2, 1).view(B, inter, H, W)
    z       = BatchNorm(W(y)) + x                                 W: 1 -> C conv with bias; no activation behind the sum
The device computes the same thing without the N x N matrix:  s_n = mean_j(phi_j g_j),  y_i = theta_i s_n,
z[i, c] = x[i, c] + (a[c] y_i + b[c]) with a, b = W and its BatchNorm folded.  THE REFERENCE IS THE LITERAL FORM in float64.

The bound is DERIVED, nothing in it is tuned (u = u32 = 2^-23 per fp32 operation as in torch_ref, the
inputs are the exact fp16 numbers the device read, the parameters the exact fp32 numbers it holds):
    dot products  theta_i, phi_i, g_i = w . x_i + bias:       d_t, d_p, d_g = (C + 1) u (sum|w||x_i| + |bias|)
    products  q_i = phi_i g_i:                                 d_q = |phi| d_g + |g| d_p + d_p d_g + u (|phi| + d_p)(|g| + d_g)
    mean  s = sum(q) / N, N adds and a divide:                 d_s = mean(d_q) + (N + 2) u mean(|q| + d_q)
    y_i = theta_i s:                                           d_y = |theta| d_s + |s| d_t + d_t d_s + u (|theta| + d_t)(|s| + d_s)
    r = fma(a, y, b):                                          d_r = |a| d_y + u (|a| (|y| + d_y) + |b|)
    z = x + r:                                                 d_z = d_r + u (|x| + |r| + d_r)
    ONE fp16 store: torch_ref's store16.

`mistake` plants one defect in the float32 host stand-in (tests/test_nonlocal_host.py checks that the bound catches each):
    'div_c' (f / C instead of f / N: the source's own variable is called f_div_C), 'batch_s' (s over the whole batch),
    'swap' (theta and phi exchanged), 'no_w_bias' (the bias of W dropped from b), 'no_shift' (the BatchNorm's shift dropped
    from b), 'theta16' (theta rounded to fp16 before use).
`order` gives the stand-in three summation orders: 'closed' (the closed form, torch's pairwise fp32 sums), 'literal' (the N x N
matmuls in fp32), 'reversed' (channels and pixels walked backwards, one running fp32 sum each)."""
import copy

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import ibn_ref
import reid_ref
import resnet_ref
import torch_ref
from fastmot_amd.models import graph as G
from torch_ref import U32


# ---------------------------------------------------------------------------------------------------------------- models
class NonLocal(nn.Module):
    """fast-reid's Non_local.  inter / div / softmax: None / 'N' / False are the published block; other values build the
    variants the lowering must refuse (two inner channels, f / C, the embedded-Gaussian softmax)."""

    def __init__(self, c, reduc_ratio=2, inter=None, div='N', softmax=False):
        super().__init__()
        self.c, self.div, self.softmax = c, div, softmax
        self.inter = reduc_ratio // reduc_ratio if inter is None else inter
        self.g = nn.Conv2d(c, self.inter, 1)
        self.W = nn.Sequential(nn.Conv2d(self.inter, c, 1), nn.BatchNorm2d(c))
        self.theta = nn.Conv2d(c, self.inter, 1)
        self.phi = nn.Conv2d(c, self.inter, 1)

    def forward(self, x):
        B = x.size(0)
        g_x = self.g(x).view(B, self.inter, -1).permute(0, 2, 1)
        theta_x = self.theta(x).view(B, self.inter, -1).permute(0, 2, 1)
        phi_x = self.phi(x).view(B, self.inter, -1)
        f = torch.matmul(theta_x, phi_x)
        if self.softmax:
            f_div_C = F.softmax(f, dim=-1)
        else:
            f_div_C = f / (f.size(-1) if self.div == 'N' else self.c)
        y = torch.matmul(f_div_C, g_x).permute(0, 2, 1).contiguous().view(B, self.inter, *x.size()[2:])
        return self.W(y) + x


# biases of phi and g behind resnet_ref.seeded: s = mean(phi g) is then their product plus what the weights add -- O(0.1) or
# more at every test shape (plain seeded biases of 0.1 left s at 0.01 for C = 24)
PHI_BIAS, G_BIAS = 0.9, -0.8


def seeded(net, seed):
    """ibn_ref.seeded (the W BatchNorm's gamma is then non-zero: fast-reid initialises it to 0, which makes the block the
    identity), and the phi / g biases above, a little apart from block to block (the exporter shares equal initialisers
    between nodes through Identity nodes, which trained weights never make it do)."""
    ibn_ref.seeded(net, seed)
    with torch.no_grad():
        for k, m in enumerate(m for m in net.modules() if isinstance(m, NonLocal)):
            m.phi.bias.fill_(PHI_BIAS + 0.05 * k)
            m.g.bias.fill_(G_BIAS - 0.05 * k)
    return net.eval()


class NLResNet(ibn_ref.IBNResNet):
    """resnet_ref / ibn_ref's ResNet with a non-local block behind the listed blocks: nl_after = {stage: [block indices]},
    stages numbered as torchvision's layer1 .. layer4 (fast-reid's R50 with WITH_NL: {2: [2, 3], 3: [3, 4, 5]})."""

    def __init__(self, block='bottleneck', layers=(3, 4, 6, 3), widths=(64, 128, 256, 512), nl_after=None, nl_kw=None, **kw):
        super().__init__(block, layers, widths, **kw)
        exp = {'basic': 1, 'bottleneck': 4}[block]
        blocks, bi = list(self.blocks), 0
        for si, (n, mid) in enumerate(zip(layers, widths)):
            for j in range(n):
                if j in (nl_after or {}).get(si + 1, ()):
                    blocks[bi] = nn.Sequential(blocks[bi], NonLocal(mid * exp, **(nl_kw or {})))
                bi += 1
        self.blocks = nn.Sequential(*blocks)


def tiny(nl_after=None, seed=5, nl_kw=None, **kw):
    """ibn_ref.tiny's net (one block per stage, outputs 64 / 64 / 128 / 256 channels on 16 x 8 .. 2 x 1 maps of a 64 x 32
    input) with non-local blocks behind stages 2 and 3 unless told otherwise.  kw: ibn, pool ('gem'), p, head, block."""
    pool, p = kw.pop('pool', 'avg'), kw.pop('p', 3.0)
    nl_after = {2: [0], 3: [0]} if nl_after is None else nl_after
    return seeded(NLResNet(kw.pop('block', 'bottleneck'), (1, 1, 1, 1), (16, 16, 32, 64), stem=16, nl_after=nl_after, nl_kw=nl_kw,
                           gem=(p, 1e-6) if pool == 'gem' else None, fc_dim=24, **kw), seed)


def tiny_sbs(seed=6):
    """The shape of fast-reid's SBS / AGW R50-ibn in small: IBN-a blocks, non-local blocks, GeM pooling, BN neck."""
    return tiny(seed=seed, ibn='a', pool='gem', head='bnneck')


def resnet50_nl(seed=9, **kw):
    """fast-reid's R50 with WITH_NL: non-local blocks behind blocks 2, 3 of layer2 and 3, 4, 5 of layer3."""
    return seeded(NLResNet('bottleneck', (3, 4, 6, 3), (64, 128, 256, 512), stem=64, nl_after={2: [2, 3], 3: [3, 4, 5]}, **kw), seed)


def export(net, hw=(64, 32), folded=True):
    """resnet_ref.export: the exporter's default form, or (folded=False) training=PRESERVE without constant folding."""
    return resnet_ref.export(net, hw, folded)


def folded_params(m):
    """-> the layer's nl_ref from the module, W + BatchNorm folded in float64: (wtheta, wphi, wg, biases [3], a, b)."""
    conv, bn = m.W
    d = lambda t: t.detach().double().numpy().reshape(-1)
    scale = d(bn.weight) / np.sqrt(d(bn.running_var) + bn.eps)
    return (d(m.theta.weight), d(m.phi.weight), d(m.g.weight), np.concatenate([d(m.theta.bias), d(m.phi.bias), d(m.g.bias)]),
            d(conv.weight) * scale, d(conv.bias) * scale + d(bn.bias) - d(bn.running_mean) * scale)


def b_parts(m):
    """-> (the bias of W through the BatchNorm's scale, the BatchNorm's own shift): the two summands of b."""
    conv, bn = m.W
    d = lambda t: t.detach().double().numpy().reshape(-1)
    scale = d(bn.weight) / np.sqrt(d(bn.running_var) + bn.eps)
    return d(conv.bias) * scale, d(bn.bias) - d(bn.running_mean) * scale


# ---------------------------------------------------------------------------------------------------- float64 restatements
def _p(a, dtype):
    """A parameter array as a tensor, without a detour through fp32 (nl_ref holds fp32 arrays; folded_params float64 ones)."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype)


def literal(x, ref, dtype=torch.float64):
    """The module's own text on x [N, C, H, W] with the folded parameters `ref` = nl_ref: the N x N form."""
    wt, wp, wg, bias, a, b = (_p(v, dtype) for v in ref)
    x = torch.as_tensor(x).to(dtype)
    B, C, H, W = x.shape
    conv = lambda w, i: F.conv2d(x, w.reshape(1, C, 1, 1), bias[i:i + 1])
    g_x = conv(wg, 2).view(B, 1, -1).permute(0, 2, 1)
    theta_x = conv(wt, 0).view(B, 1, -1).permute(0, 2, 1)
    phi_x = conv(wp, 1).view(B, 1, -1)
    f = torch.matmul(theta_x, phi_x)
    y = torch.matmul(f / f.size(-1), g_x).permute(0, 2, 1).contiguous().view(B, 1, H, W)
    return F.conv2d(y, a.reshape(C, 1, 1, 1), b) + x


def _dots(x, w, bias, order):
    """w . x_i + bias per pixel -> [N, 1, H, W]; 'reversed': one running sum over the channels, last channel first."""
    if order == 'reversed':
        return (torch.cumsum((x * w.reshape(1, -1, 1, 1)).flip(1), dim=1)[:, -1:] + bias)
    return F.conv2d(x, w.reshape(1, -1, 1, 1), bias.reshape(1))


def nonlocal_(x, ref, dtype=torch.float64, track=True, mistake=None, order='closed', parts=None):
    """x: [N, C, H, W] (exact fp16 numbers), ref = the layer's nl_ref.  -> (values BEFORE the fp16 store, bound or None).
    track=True: the literal form's values with the bound of the module docstring.  track=False, dtype=float32: a host
    stand-in for the device, in one of three summation orders and optionally with one planted mistake.  parts = b_parts(m):
    what the bias of W and the BatchNorm's shift each contribute to b (the mistakes that drop one of them)."""
    wt, wp, wg, bias, a, b = (_p(v, dtype) for v in ref)
    x = torch.as_tensor(x).to(dtype)
    n, c, h, w = x.shape
    hw = h * w
    if track:
        assert mistake is None and order == 'closed'
    elif order == 'literal' and mistake is None:
        return literal(x, ref, dtype), None
    if mistake == 'swap':
        wt, wp, bias = wp, wt, torch.stack([bias[1], bias[0], bias[2]])
    theta, phi, g = (_dots(x, wv, bias[i], order) for i, wv in enumerate((wt, wp, wg)))
    if mistake == 'theta16':
        theta = theta.half().to(dtype)
    q = phi * g
    dims = (0, 2, 3) if mistake == 'batch_s' else (2, 3)
    if order == 'reversed':
        s = torch.cumsum(q.reshape(n, -1).flip(1), dim=1)[:, -1].reshape(n, 1, 1, 1) / hw
        if mistake == 'batch_s':
            s = s.mean(dim=0, keepdim=True).expand(n, 1, 1, 1)
    else:
        s = q.mean(dim=dims, keepdim=True)
    if mistake == 'div_c':
        s = s * hw / c
    y = theta * s
    if mistake in ('no_w_bias', 'no_shift'):
        b = b - _p(parts[0 if mistake == 'no_w_bias' else 1], dtype)
    av, bv = a.reshape(1, -1, 1, 1), b.reshape(1, -1, 1, 1)
    r = av * y + bv
    z = x + r
    if not track:
        return z, None
    u = U32
    ax = x.abs()
    d_t, d_p, d_g = ((c + 1) * u * (F.conv2d(ax, wv.abs().reshape(1, -1, 1, 1)) + bias[i].abs()) for i, wv in enumerate((wt, wp, wg)))
    d_q = phi.abs() * d_g + g.abs() * d_p + d_p * d_g + u * (phi.abs() + d_p) * (g.abs() + d_g)
    d_s = d_q.mean(dim=(2, 3), keepdim=True) + (hw + 2) * u * (q.abs() + d_q).mean(dim=(2, 3), keepdim=True)
    d_y = theta.abs() * d_s + s.abs() * d_t + d_t * d_s + u * (theta.abs() + d_t) * (s.abs() + d_s)
    d_r = av.abs() * d_y + u * (av.abs() * (y.abs() + d_y) + bv.abs())
    d_z = d_r + u * (ax + r.abs() + d_r)
    return literal(x, ref, dtype), d_z


def term(x, ref):
    """|a[c] theta_i s_n|, the data-dependent part of the output, in float64: [N, C, H, W]."""
    wt, wp, wg, bias, a, b = (_p(v, torch.float64) for v in ref)
    x = torch.as_tensor(x).double()
    theta, phi, g = (F.conv2d(x, wv.reshape(1, -1, 1, 1), bias[i:i + 1]) for i, wv in enumerate((wt, wp, wg)))
    s = (phi * g).mean(dim=(2, 3), keepdim=True)
    return (a.reshape(1, -1, 1, 1) * theta * s).abs(), s.reshape(-1)


def reference(x, ref):
    """-> (float64 reference, bound) of the STORED fp16 tensor, and the condition every test shape must meet, asserted on the
    reference alone: the data-dependent term exceeds 16 x the element's bound on at least half the elements (otherwise a
    kernel that drops the term passes)."""
    it = torch_ref._Interp(None, None, torch.float64, emulate=False, track=True)
    v, e = it.store16(nonlocal_(x, ref))
    t, s = term(x, ref)
    share = float((t > 16 * e).double().mean())
    assert share >= 0.5, f'vacuous case: term > 16 x bound on {share:.2f} of the elements, s = {s.tolist()}'
    return v, e


# -------------------------------------------------------------------------------------------------------------- layer tables
def _in_view(d, bufs, dtype):
    v = d['ins'][0]
    return bufs[v.tid][:, v.coff:v.coff + v.c].to(dtype)


def run_layer(graph, idx, bufs, **kw):
    """ibn_ref.run_layer for tables that hold OP_NONLOCAL."""
    d = graph.layers[idx]
    if d['op'] != G.OP_NONLOCAL:
        return ibn_ref.run_layer(graph, idx, bufs, **kw)
    v, e = reference(_in_view(d, bufs, torch.float64), d['nl_ref'])
    return 'tensor', v, e


def run_graph(graph, x_nchw, emulate_fp16_storage=True):
    """ibn_ref.run_graph (fp32, optionally fp16 storage) for such tables: -> (bufs, embeddings).  As there, torch_ref sees the
    ops it does not know as copies, and `around` overwrites each copy with the real thing."""
    last, first = graph.layers[-1], graph.layers[0]
    head, stem = last['op'] == G.OP_POOLHEAD, first['op'] == G.OP_STEMPOOL
    lo, hi = (1 if stem else 0), (len(graph.layers) - 1 if head else len(graph.layers))
    own = (G.OP_INSTNORM, G.OP_NONLOCAL)
    body = copy.copy(graph)
    body.layers = [dict(d, op=G.OP_COPY) if d['op'] in own else d for d in graph.layers[lo:hi]]
    body.conv_params = [(i - lo, w, b) for i, w, b in graph.conv_params]

    def put(d, bufs):
        x = _in_view(d, bufs, torch.float32)
        if d['op'] == G.OP_NONLOCAL:
            y = nonlocal_(x, d['nl_ref'], dtype=torch.float32, track=False)[0]
        else:
            y = ibn_ref.instnorm(x, d['instnorm_ref'], d['hid'], d['act'], dtype=torch.float32, track=False)[0]
        o = d['out']
        bufs[o.tid][:, o.coff:o.coff + o.c] = y.half().float() if emulate_fp16_storage else y

    def around(idx, bufs):
        if stem and idx == 0:
            y, _ = reid_ref.stempool(_in_view(first, bufs, torch.float32), first['stempool_ref'], dtype=torch.float32, track=False,
                                     mistake=None if emulate_fp16_storage else 'unrounded')
            o = first['out']
            bufs[o.tid][:, o.coff:o.coff + o.c] = y
        d = graph.layers[lo + idx]
        if d['op'] in own:
            return lambda b, emb: put(d, b)
    bufs, emb = torch_ref.run_graph(body, x_nchw, emulate_fp16_storage, around=around)
    if not head:
        return bufs, emb
    x = _in_view(last, bufs, torch.float32)
    if 'gem_ref' in last:
        emb, _ = ibn_ref.poolhead(x, last['poolhead_ref'], last['gem_ref'], dtype=torch.float32, track=False)
    else:
        emb, _ = reid_ref.poolhead(x, last['poolhead_ref'], dtype=torch.float32, track=False)
    return bufs, emb


def measured_bar(net, g, x):
    """ibn_ref.measured_bar's rule over this module's run_graph: the fp32 torch module against the fp16-STORAGE interpretation
    of the table on the CPU (no code under test involved), times the project's factor 4.
    -> (module embeddings, 4 x max |delta| per component, 4 x (1 - cosine))."""
    expect = resnet_ref.embed(net, x)
    _, emu = run_graph(g, torch.from_numpy(x), emulate_fp16_storage=True)
    emu = emu.numpy()
    d_abs = float(np.abs(emu - expect).max())
    d_cos = float((1 - np.sum(emu.astype(np.float64) * expect, axis=1)).max())
    return expect, 4 * d_abs, 4 * max(d_cos, 1e-7)


# ------------------------------------------------------------------------------------------------- one-layer cases (GPU + host)
NMAX = 3
# (N, H, W, C) of tests/test_nonlocal_gpu.py: one pixel; fewer pixels than waves with C / 8 = 3; two loads per pixel; exactly
# one pixel per wave load; several pixels per load; four loads per pixel on an odd map
CASES = [(1, 1, 1, 8), (3, 5, 3, 24), (2, 16, 8, 1024), (2, 32, 16, 512), (1, 24, 8, 256), (2, 7, 5, 2048)]


def make_case(n, h, w, c, in_off=0, in_c=None, out_off=0, out_c=None, seed=0):
    """-> (graph with ONE FM_OP_NONLOCAL layer over channels [in_off, in_off + c) of an in_c-channel input, written to channels
    [out_off, out_off + c) of an out_c-channel tensor; x [n, h, w, in_c] fp16).  Seeded as the models are: weights of variance
    1.6 / fan, the W BatchNorm away from the identity, the phi / g biases of this module."""
    m = seeded(NonLocal(c), seed + c + h * w)
    in_c, out_c = in_c or c, out_c or c
    g = G.Graph(None, (h, w), in_c)
    dst = g.new(h, w, out_c).slice(out_off, c)
    g.nonlocal_('nl', g.input.slice(in_off, c), *folded_params(m), dst=dst)
    g.layers[0]['b_parts'] = b_parts(m)
    g.outputs = [dst]
    x = np.random.default_rng(seed + 7 * c + h).normal(0, 1, (n, h, w, in_c)).astype(np.float16)
    return g, x


def case_reference(g, x):
    """The float64 reference and bound of make_case's one-layer graph: -> (bufs, ref, bound)."""
    bufs = {g.input.tid: torch.from_numpy(x.astype(np.float32)).permute(0, 3, 1, 2)}
    _, ref, bound = run_layer(g, 0, bufs)
    return bufs, ref, bound
