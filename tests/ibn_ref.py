"""TEST INFRASTRUCTURE for IBN-Net ReID models (models/onnx_graph.py, FM_OP_INSTNORM in csrc/instnorm.hip, the GeM mode of
FM_OP_POOLHEAD in csrc/reidhead.hip): the models in plain torch on top of tests/resnet_ref.py, float64 restatements of the
two device stages with their elementwise bounds, and `run_layer` / `run_graph` / `measured_bar` for layer tables that hold
them (every other op goes to tests/reid_ref.py and tests/torch_ref.py).

Models (IBN-Net, Pan et al. 2018; fast-reid's R50-ibn, torchreid's resnet50_ibn_a / _b; GeM: fast-reid's
GeneralizedMeanPooling / GeneralizedMeanPoolingP):
    ibn='a'   the IBN module -- InstanceNorm2d(affine) on the first half of the channels, BatchNorm2d on the rest, concatenated
              -- in place of `bn1` in every block of stages 1-3
    ibn='b'   InstanceNorm2d(affine) after the residual sum (before the ReLU) of the last block of stages 1-2, and in place of
              the stem's BatchNorm
    pool='gem'  mean(clamp(x, min=eps)^p)^(1/p) in place of the average pool; p a float, or (learn_p) a Parameter of shape [1]

Bounds (u = u32 = 2^-23 stands for one fp32 operation as in torch_ref, inputs are exact fp16 numbers):

  instnorm, per sample and channel over HW pixels
    mean  m = sum / HW, HW adds and a divide:                 d_m = (HW + 1) u mean|x|
    centred values  c = x - m':                               d_c = d_m + u |c|
    squares  c^2:                                             d_q = 2 |c| d_c + d_c^2 + u (|c| + d_c)^2
    variance  v = sum(q) / HW, HW adds and a divide:          d_v = mean(d_q) + (HW + 1) u mean((|c| + d_c)^2)
    s = v + eps:                                              d_s = d_v + u s
    r = sqrt(s) (IEEE):                                       d_r = d_s / (2 sqrt(s - d_s)) + u r
    rstd = 1 / r (IEEE):                                      d_rstd = d_r / (r (r - d_r)) + u rstd
                                                              (about d_s rstd^3 / 2: a near-constant channel, s ~ eps, is expensive)
    t = c * rstd:                                             d_t = d_c (rstd + d_rstd) + |c| d_rstd + u |t|
    a = t * gamma, y = a + beta:                              d_y = |gamma| d_t + u |a| + u (|a| + |beta|)
    activation (linear or ReLU, slope <= 1), ONE fp16 store:  torch_ref's store16
    pass-through channels: act(x), exact in fp32, the same store (which is then exact too)

  GeM, every term positive, so the errors are RELATIVE and compose as products of (1 + delta):
    g = max(x, eps)^p:   p == 3: two multiplies, 2 u;  otherwise powf: K_POW u
    mean over HW:        (HW + 1) u
    root  m^(1/p):       the mean's relative error / p, + cbrtf: K_CBRT u  or  powf: K_POW u + |ln m| u / p (the exponent
                         1 / p itself is rounded to fp32)
    d = value * expm1(sum of the above) + ((m + FLT_MIN)^(1/p) - m^(1/p)): powers below the smallest normal fp32 number
    (2^-126; eps^p for a large p) may be flushed;  then the neck, the FC and the L2 normalisation as tests/reid_ref.py.
  K_POW = 16, K_CBRT = 2: the OpenCL conformance limits for pow and cbrt in ulp.  HIP's own table of maximum ulp errors is a
  page of its documentation, which is not installed with the ROCm tree these tests run against, so the OpenCL limits it is
  to stay within are used; they are not tuned.

`mistake` plants one defect (tests/test_ibn_host.py checks that the bounds catch each):
    instnorm: 'unbiased' (variance / (HW - 1)), 'no_eps', 'batch_stats' (statistics over N x HW), 'ex2' (E[x^2] - mean^2 in
              fp32), 'pass_raw' (pass-through channels not activated)
    gem:      'no_clamp', 'no_root', 'pow_of_mean' (the power applied to the mean instead of the mean of the powers)
"""
import copy

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import reid_ref
import resnet_ref
import torch_ref
from fastmot_amd.models import graph as G
from torch_ref import FAST_EXP, U32

K_POW, K_CBRT = 16, 2
FLT_MIN = 2.0 ** -126


# ---------------------------------------------------------------------------------------------------------------- models
class IBN(nn.Module):
    def __init__(self, planes):
        super().__init__()
        self.half = planes // 2
        self.IN = nn.InstanceNorm2d(self.half, affine=True)
        self.BN = nn.BatchNorm2d(planes - self.half)

    def forward(self, x):
        a, b = torch.split(x, self.half, 1)
        return torch.cat((self.IN(a.contiguous()), self.BN(b.contiguous())), 1)


class INAfterSum(nn.Module):
    """A resnet_ref block with InstanceNorm2d between the residual sum and the ReLU (IBN-b)."""

    def __init__(self, blk, c):
        super().__init__()
        self.blk, self.IN = blk, nn.InstanceNorm2d(c, affine=True)

    def forward(self, x):
        b = self.blk
        out = F.relu(b.bn1(b.conv1(x)))
        if hasattr(b, 'conv3'):
            out = b.bn3(b.conv3(F.relu(b.bn2(b.conv2(out)))))
        else:
            out = b.bn2(b.conv2(out))
        return F.relu(self.IN(out + (x if b.downsample is None else b.downsample(x))))


class IBNResNet(resnet_ref.ResNet):
    def __init__(self, block='bottleneck', layers=(3, 4, 6, 3), widths=(64, 128, 256, 512), stem=64, ibn=None, gem=None,
                 learn_p=False, **kw):
        super().__init__(block, layers, widths, stem=stem, **kw)
        exp = {'basic': 1, 'bottleneck': 4}[block]
        blocks, bi = list(self.blocks), 0
        for si, (n, mid) in enumerate(zip(layers, widths)):
            for j in range(n):
                if ibn == 'a' and si < 3:
                    blocks[bi].bn1 = IBN(mid)
                if ibn == 'b' and si < 2 and j == n - 1:
                    blocks[bi] = INAfterSum(blocks[bi], mid * exp)
                bi += 1
        self.blocks = nn.Sequential(*blocks)
        if ibn == 'b':
            self.bn1 = nn.InstanceNorm2d(stem, affine=True)
        self.gem = gem
        if gem is not None:
            p, self.gem_eps = gem
            self.p = nn.Parameter(torch.ones(1) * p) if learn_p else float(p)

    def forward(self, x):
        x = self.blocks(self.maxpool(F.relu(self.bn1(self.conv1(x)))))
        if self.gem is not None:
            v = torch.flatten(F.adaptive_avg_pool2d(x.clamp(min=self.gem_eps).pow(self.p), 1), 1).pow(1.0 / self.p)
        else:
            v = torch.flatten(F.adaptive_avg_pool2d(x, 1), 1)
        if self.head == 'bnneck':
            v = self.neck(v)
        elif self.head == 'fc512':
            v = F.relu(self.fc_bn(self.fc(v)))
        return v


def seeded(net, seed):
    """resnet_ref.seeded, and InstanceNorm parameters away from the identity."""
    resnet_ref.seeded(net, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.InstanceNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) * 1.0 + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.3)
    return net.eval()


def tiny(ibn=None, pool='avg', p=3.0, learn_p=False, head='none', block='bottleneck', seed=5, gem_eps=1e-6):
    """One block per stage, mid widths 16 / 16 / 32 / 64 (every IN half a multiple of 8), stem 16, fc 24."""
    return seeded(IBNResNet(block, (1, 1, 1, 1), (16, 16, 32, 64), stem=16, ibn=ibn, gem=(p, gem_eps) if pool == 'gem' else None,
                            learn_p=learn_p, head=head, fc_dim=24), seed)


def resnet50_ibn_a(p=3.0, head='bnneck', seed=9):
    """fast-reid's R50-ibn shape: IBN-a, GeM, BN neck."""
    return seeded(IBNResNet('bottleneck', (3, 4, 6, 3), (64, 128, 256, 512), stem=64, ibn='a', gem=(p, 1e-6), head=head), seed)


# ---------------------------------------------------------------------------------------------------- float64 restatements
def instnorm(x, ref, cn, act, dtype=torch.float64, track=True, mistake=None):
    """x: [N, C, H, W] (exact fp16 numbers); ref = the layer's instnorm_ref (gamma [cn], beta [cn], eps).
    -> (values BEFORE the fp16 store, bound or None).  track=False, dtype=float32: a host stand-in for the device."""
    gamma, beta, eps = ref
    x = torch.as_tensor(x).to(dtype)
    n, c, h, w = x.shape
    hw = h * w
    ga, be = (torch_ref._t(a, dtype).reshape(1, -1, 1, 1) for a in (gamma, beta))
    xn = x[:, :cn]
    dims = (0, 2, 3) if mistake == 'batch_stats' else (2, 3)
    m = xn.mean(dim=dims, keepdim=True)
    cen = xn - m
    if mistake == 'ex2':
        var = ((xn * xn).mean(dim=dims, keepdim=True) - m * m).clamp_min(0)
    else:
        var = (cen * cen).mean(dim=dims, keepdim=True)
    if mistake == 'unbiased':
        var = var * hw / max(hw - 1, 1)
    s = var + (0.0 if mistake == 'no_eps' else eps)
    r = s.sqrt()
    rstd = 1.0 / r
    t = cen * rstd
    a = t * ga
    y = a + be
    rest = x[:, cn:]
    out = torch.cat([y, rest], dim=1)
    if act == G.ACT['relu']:
        out = torch.cat([F.relu(y), rest if mistake == 'pass_raw' else F.relu(rest)], dim=1)
    if not track:
        return out, None
    u = U32
    d_m = (hw + 1) * u * xn.abs().mean(dim=(2, 3), keepdim=True)
    d_c = d_m + u * cen.abs()
    hi = cen.abs() + d_c
    d_q = 2 * cen.abs() * d_c + d_c * d_c + u * hi * hi
    d_v = d_q.mean(dim=(2, 3), keepdim=True) + (hw + 1) * u * (hi * hi).mean(dim=(2, 3), keepdim=True)
    d_s = d_v + u * s
    d_r = d_s / (2 * (s - d_s).clamp_min(1e-300).sqrt()) + u * r
    d_rstd = d_r / (r * (r - d_r).clamp_min(1e-300)) + u * rstd
    d_t = d_c * (rstd + d_rstd) + cen.abs() * d_rstd + u * t.abs()
    d_y = ga.abs() * d_t + u * a.abs() + u * (a.abs() + be.abs())
    return out, torch.cat([d_y, torch.zeros_like(rest)], dim=1)


def _tail(it, m, em, ref, track):
    """What reid_ref.poolhead does behind its pool: neck, FC, L2 normalisation, from the pooled vector [N, C, 1, 1]."""
    scale, shift, w, b, relu = ref
    if scale is not None:
        s, t = (torch_ref._t(a, m.dtype).reshape(1, -1, 1, 1) for a in (scale, shift))
        em = s.abs() * em + 2 * U32 * ((m * s).abs() + t.abs()) if track else None
        m = m * s + t
    if w is not None:
        m, em = it.conv_stage((m, em), np.asarray(w)[:, :, None, None], b, G.ACT['relu'] if relu else G.ACT['linear'])
    fv = m[:, :, 0, 0]
    n = fv.norm(dim=1, keepdim=True)
    ev = fv / n
    if not track:
        return ev, None
    fe = em[:, :, 0, 0]
    dn = fe.norm(dim=1, keepdim=True) + (fv.shape[1] + 2) * U32 * n
    nlo = (n - dn).clamp_min(1e-30)
    return ev, fe / nlo + fv.abs() * dn / (n * nlo) + (2 * U32 + FAST_EXP) * ev.abs()


def gem_pool(x, gem, dtype=torch.float64, track=True, mistake=None):
    """The pooled GeM vector [N, C, 1, 1] of x [N, C, H, W] and its bound."""
    p, eps = gem
    x = torch.as_tensor(x).to(dtype)
    hw = x.shape[2] * x.shape[3]
    v = x if mistake == 'no_clamp' else x.clamp_min(eps)
    cube = float(p) == 3.0
    if mistake == 'pow_of_mean':
        return v.mean(dim=(2, 3), keepdim=True), None
    if mistake == 'no_clamp':       # (a negative base: odd p keeps the sign, any other p is not a number -- taken as |x|^p)
        g = v * v * v if cube else v.abs().pow(p)
    else:
        g = v * v * v if cube else v.pow(p)
    m = g.mean(dim=(2, 3), keepdim=True)
    if mistake == 'no_root':
        return m, None
    root = m.sign() * m.abs().pow(1.0 / p)
    if not track:
        return root, None
    rel = ((2 if cube else K_POW) + hw + 1) * U32 / p + (K_CBRT * U32 if cube else K_POW * U32 + m.log().abs() * U32 / p)
    # a power below the smallest normal fp32 number may be flushed or lose its digits: an ABSOLUTE FLT_MIN on the mean
    under = (m + FLT_MIN).pow(1.0 / p) - root
    return root, root * torch.expm1(torch.as_tensor(rel, dtype=dtype)) + under


def poolhead(x, ref, gem, dtype=torch.float64, track=True, mistake=None):
    """reid_ref.poolhead with GeM pooling: -> (embeddings [N, D], bound or None)."""
    it = torch_ref._Interp(None, None, dtype, emulate=not track, track=track)
    m, em = gem_pool(x, gem, dtype, track and mistake is None, mistake)
    if em is None and track:
        em = torch.zeros_like(m)
    return _tail(it, m, em, ref, track)


def check_layer(got, ref, bound, what):
    """torch_ref.check_layer, which compares with `err > 0` and so lets a NaN through: non-finite results are refused first
    (an epsilon left out of a constant channel gives 0 * inf)."""
    got = torch.as_tensor(got)
    bad = int((~torch.isfinite(got)).sum())
    assert bad == 0, f'{what}: {bad} non-finite results, over the bound'
    return torch_ref.check_layer(got, ref, bound, what)


# -------------------------------------------------------------------------------------------------------------- layer tables
def _in_view(d, bufs, dtype):
    v = d['ins'][0]
    return bufs[v.tid][:, v.coff:v.coff + v.c].to(dtype)


def run_layer(graph, idx, bufs, **kw):
    """reid_ref.run_layer for tables that hold OP_INSTNORM or a GeM head."""
    d = graph.layers[idx]
    if d['op'] == G.OP_INSTNORM:
        it = torch_ref._Interp(None, None, torch.float64, emulate=False, track=True)
        v, e = it.store16(instnorm(_in_view(d, bufs, torch.float64), d['instnorm_ref'], d['hid'], d['act']))
        return 'tensor', v, e
    if d['op'] == G.OP_POOLHEAD and 'gem_ref' in d:
        emb, bound = poolhead(_in_view(d, bufs, torch.float64), d['poolhead_ref'], d['gem_ref'])
        return 'emb', emb, bound
    return reid_ref.run_layer(graph, idx, bufs, **kw)


def run_graph(graph, x_nchw, emulate_fp16_storage=True):
    """reid_ref.run_graph (fp32, optionally fp16 storage) for such tables: -> (bufs, embeddings)."""
    last, first = graph.layers[-1], graph.layers[0]
    head, stem = last['op'] == G.OP_POOLHEAD, first['op'] == G.OP_STEMPOOL
    lo, hi = (1 if stem else 0), (len(graph.layers) - 1 if head else len(graph.layers))
    body = copy.copy(graph)
    # (torch_ref does not know OP_INSTNORM: it copies the view, and `around` overwrites the copy with the real thing)
    body.layers = [dict(d, op=G.OP_COPY) if d['op'] == G.OP_INSTNORM else d for d in graph.layers[lo:hi]]
    body.conv_params = [(i - lo, w, b) for i, w, b in graph.conv_params]

    def put(d, bufs, y):
        o = d['out']
        bufs[o.tid][:, o.coff:o.coff + o.c] = y.half().float() if emulate_fp16_storage else y

    def around(idx, bufs):
        if stem and idx == 0:
            y, _ = reid_ref.stempool(_in_view(first, bufs, torch.float32), first['stempool_ref'], dtype=torch.float32, track=False,
                                     mistake=None if emulate_fp16_storage else 'unrounded')
            o = first['out']
            bufs[o.tid][:, o.coff:o.coff + o.c] = y
        d = graph.layers[lo + idx]
        if d['op'] == G.OP_INSTNORM:
            return lambda b, emb: put(d, b, instnorm(_in_view(d, b, torch.float32), d['instnorm_ref'], d['hid'], d['act'],
                                                     dtype=torch.float32, track=False)[0])
    bufs, emb = torch_ref.run_graph(body, x_nchw, emulate_fp16_storage, around=around)
    if not head:
        return bufs, emb
    x = _in_view(last, bufs, torch.float32)
    if 'gem_ref' in last:
        emb, _ = poolhead(x, last['poolhead_ref'], last['gem_ref'], dtype=torch.float32, track=False)
    else:
        emb, _ = reid_ref.poolhead(x, last['poolhead_ref'], dtype=torch.float32, track=False)
    return bufs, emb


def measured_bar(net, g, x):
    """reid_ref.measured_bar over this module's run_graph: the fp32 torch module against the fp16-STORAGE interpretation
    of the table on the CPU (no code under test involved), times the project's factor 4.
    -> (module embeddings, 4 x max |delta| per component, 4 x (1 - cosine))."""
    expect = resnet_ref.embed(net, x)
    _, emu = run_graph(g, torch.from_numpy(x), emulate_fp16_storage=True)
    emu = emu.numpy()
    d_abs = float(np.abs(emu - expect).max())
    d_cos = float((1 - np.sum(emu.astype(np.float64) * expect, axis=1)).max())
    return expect, 4 * d_abs, 4 * max(d_cos, 1e-7)
