"""TEST INFRASTRUCTURE for the OSNet-IBN / OSNet-AIN block tail: float64 restatements, with elementwise bounds, of FM_OP_CONVIN
(csrc/convin.hip: pointwise conv, instance normalisation, residual, activation in one launch) and of FM_OP_INSTNORM with its
residual view, and `run_layer` / `run_graph` / `measured_bar` for layer tables that hold them (every other op goes to
tests/ibn_ref.py, tests/reid_ref.py and tests/torch_ref.py).

The bound is DERIVED, nothing in it is tuned (u = u32 = 2^-23 per fp32 operation, as in torch_ref; the inputs are the exact
fp16 numbers the device read; the reference is float64):

  conv stage (torch_ref._Interp.conv_stage), kept in fp32 and never stored:
      v = W x + b (+ res, RES_BEFORE_NORM),  S = |W| |x| + |b| (+ |res|),  K' = K (+ 1 with the residual)
      d_x = K' u S                                       the project's conv accumulation bound, here the norm's INPUT error
  the instance normalisation of tests/ibn_ref.py's docstring, which assumes exact inputs, with d_x carried through:
      mean  m = sum / HW:                                d_m = mean(d_x) + (HW + 1) u mean|v|
      centred values  c = v - m':                        d_c = d_x + d_m + u |c|
      squares  c^2:                                      d_q = 2 |c| d_c + d_c^2 + u (|c| + d_c)^2
      variance  sum(q) / HW:                             d_v = mean(d_q) + (HW + 1) u mean((|c| + d_c)^2)
      s = v + eps, r = sqrt(s), rstd = 1 / r:            d_s, d_r, d_rstd as ibn_ref
      t = c * rstd:                                      d_t = d_c (rstd + d_rstd) + |c| d_rstd + u |t|
      a = t * gamma, y = a + beta:                       d_y = |gamma| d_t + u |a| + u (|a| + |beta|)
  residual behind the affine (RES_AFTER_NORM), exact fp16 numbers added in fp32:   d_y += u |y + res|
  activation (linear or ReLU: slope <= 1), ONE fp16 store: torch_ref's store16.
  FM_OP_INSTNORM with a residual: ibn_ref's chain (d_x = 0) on the normalised channels, the same residual term on all.

`mistake` plants one defect in the float32 host stand-in (tests/test_convin_host.py checks that the bound catches each):
    'unbiased' (variance / (HW - 1)), 'no_eps', 'batch_stats' (statistics over N x HW), 'ex2' (E[v^2] - mean^2 in fp32),
    'res_side' (the residual on the other side of the norm), 'padded' (the 32-pixel tiles' padding lanes, which hold the
    bias alone, counted in both sums)."""
import numpy as np
import torch
import torch.nn.functional as F

import ibn_ref
import resnet_ref
import torch_ref
from fastmot_amd.models import graph as G
from torch_ref import U32


def norm_chain(v, d_x, gamma, beta, eps, track=True, mistake=None, pad_value=None):
    """Instance normalisation of v [N, C, H, W] whose elements carry the error d_x (tensor or 0.0) -> (y, d_y or None)."""
    n, c, h, w = v.shape
    hw = h * w
    ga, be = (torch_ref._t(a, v.dtype).reshape(1, -1, 1, 1) for a in (gamma, beta))
    dims = (0, 2, 3) if mistake == 'batch_stats' else (2, 3)
    if mistake == 'padded':          # lanes beyond HW in the last 32-pixel tile hold pad_value (the bias): counted, divisor HW
        extra = (-hw) % 32
        m = (v.sum(dim=dims, keepdim=True) + extra * pad_value) / hw
    else:
        m = v.mean(dim=dims, keepdim=True)
    cen = v - m
    if mistake == 'ex2':
        var = ((v * v).mean(dim=dims, keepdim=True) - m * m).clamp_min(0)
    elif mistake == 'padded':
        var = ((cen * cen).sum(dim=dims, keepdim=True) + extra * (pad_value - m) ** 2) / hw
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
    if not track:
        return y, None
    u = U32
    d_x = d_x if torch.is_tensor(d_x) else torch.full_like(v, d_x)
    d_m = d_x.mean(dim=(2, 3), keepdim=True) + (hw + 1) * u * v.abs().mean(dim=(2, 3), keepdim=True)
    d_c = d_x + d_m + u * cen.abs()
    hi = cen.abs() + d_c
    d_q = 2 * cen.abs() * d_c + d_c * d_c + u * hi * hi
    d_v = d_q.mean(dim=(2, 3), keepdim=True) + (hw + 1) * u * (hi * hi).mean(dim=(2, 3), keepdim=True)
    d_s = d_v + u * s
    d_r = d_s / (2 * (s - d_s).clamp_min(1e-300).sqrt()) + u * r
    d_rstd = d_r / (r * (r - d_r).clamp_min(1e-300)) + u * rstd
    d_t = d_c * (rstd + d_rstd) + cen.abs() * d_rstd + u * t.abs()
    d_y = ga.abs() * d_t + u * a.abs() + u * (a.abs() + be.abs())
    # where the variance's own error reaches s = var + eps (one pixel behind a long accumulation: var = 0, d_c^2 >= eps) the
    # chain bounds nothing -- 1 / sqrt(s - d_s) has no upper limit -- and says so with +inf instead of 0 * inf
    return y, torch.nan_to_num(d_y, nan=float('inf'))


def convin(x, ref, act, res=None, res_mode=G.RES_NONE, dtype=torch.float64, track=True, mistake=None):
    """x: [N, K, H, W], res: [N, cout, H, W] or None (exact fp16 numbers); ref = the layer's convin_ref (fp16-rounded weight
    [cout, K, 1, 1] as fp32, bias, gamma, beta, eps).  -> (values BEFORE the fp16 store, bound or None).
    track=False, dtype=float32: a host stand-in for the device."""
    w, b, gamma, beta, eps = ref
    x = torch.as_tensor(x).to(dtype)
    w, b = torch_ref._t(w, dtype), torch_ref._t(b, dtype)
    res = torch.as_tensor(res).to(dtype) if res is not None else None
    if mistake == 'res_side' and res_mode != G.RES_NONE:
        res_mode = G.RES_AFTER_NORM if res_mode == G.RES_BEFORE_NORM else G.RES_BEFORE_NORM
    v = F.conv2d(x, w, b)
    K = w[0].numel()
    S = F.conv2d(x.abs(), w.abs(), b.abs()) if track else None
    if res_mode == G.RES_BEFORE_NORM:
        v = v + res
        if track:
            K, S = K + 1, S + res.abs()
    y, d_y = norm_chain(v, K * U32 * S if track else 0.0, gamma, beta, eps, track, mistake, pad_value=b.reshape(1, -1, 1, 1))
    if res_mode == G.RES_AFTER_NORM:
        y = y + res
        if track:
            d_y = d_y + U32 * y.abs()
    if act == G.ACT['relu']:
        y = F.relu(y)
    return y, d_y


def instnorm_res(x, ref, cn, act, res, dtype=torch.float64, track=True):
    """FM_OP_INSTNORM with its residual view: ibn_ref.instnorm's normalisation of the first cn channels, `res` added to every
    channel behind the affine, then the activation."""
    gamma, beta, eps = ref
    x = torch.as_tensor(x).to(dtype)
    res = torch.as_tensor(res).to(dtype)
    y, d_y = norm_chain(x[:, :cn], 0.0, gamma, beta, eps, track)
    out = torch.cat([y, x[:, cn:]], dim=1) + res
    if act == G.ACT['relu']:
        out = F.relu(out)
    if not track:
        return out, None
    return out, torch.cat([d_y, torch.zeros_like(x[:, cn:])], dim=1) + U32 * (torch.cat([y, x[:, cn:]], dim=1) + res).abs()


# -------------------------------------------------------------------------------------------------------------- layer tables
def _view(v, bufs, dtype):
    return bufs[v.tid][:, v.coff:v.coff + v.c].to(dtype)


def _own(d):
    return d['op'] == G.OP_CONVIN or (d['op'] == G.OP_INSTNORM and d['res'] is not None)


def _eval(d, bufs, dtype, track):
    x = _view(d['ins'][0], bufs, dtype)
    res = _view(d['res'], bufs, dtype) if d['res'] is not None else None
    if d['op'] == G.OP_CONVIN:
        return convin(x, d['convin_ref'], d['act'], res, d['res_mode'], dtype, track)
    return instnorm_res(x, d['instnorm_ref'], d['hid'], d['act'], res, dtype, track)


def run_layer(graph, idx, bufs, **kw):
    """ibn_ref.run_layer for tables that hold OP_CONVIN or an OP_INSTNORM with a residual."""
    d = graph.layers[idx]
    if not _own(d):
        return ibn_ref.run_layer(graph, idx, bufs, **kw)
    it = torch_ref._Interp(None, None, torch.float64, emulate=False, track=True)
    v, e = it.store16(_eval(d, bufs, torch.float64, True))
    return 'tensor', v, e


def run_graph(graph, x_nchw, emulate_fp16_storage=True):
    """torch_ref.run_graph (fp32, optionally fp16 storage) for such tables: -> (bufs, embeddings)."""
    n = x_nchw.shape[0]
    bufs = {tid: torch.zeros(n, c, h, w) for tid, (h, w, c, f32) in enumerate(graph.tensors)}
    x = x_nchw.float()
    if emulate_fp16_storage:
        x = x.half().float()
    bufs[graph.input.tid][:, :x.shape[1]] = x
    params = {idx: (w, b) for idx, w, b in graph.conv_params}
    it = torch_ref._Interp(graph, bufs, torch.float32, emulate_fp16_storage)
    for idx, d in enumerate(graph.layers):
        if _own(d) or d['op'] == G.OP_INSTNORM:
            if d['op'] == G.OP_INSTNORM and d['res'] is None:
                y, _ = ibn_ref.instnorm(_view(d['ins'][0], bufs, torch.float32), d['instnorm_ref'], d['hid'], d['act'],
                                        dtype=torch.float32, track=False)
            else:
                y, _ = _eval(d, bufs, torch.float32, False)
            o = d['out']
            bufs[o.tid][:, o.coff:o.coff + o.c] = y.half().float() if emulate_fp16_storage else y
        else:
            it.step(d, params.get(idx))
    return bufs, (it.emb[0] if it.emb is not None else None)


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
# (K, cout, (H, W), residual mode): the shapes of tests/test_convin_gpu.py
CASES = [(K, cout, hw, mode) for K, cout, hw in [(8, 8, (1, 1)), (24, 40, (3, 11)), (128, 64, (16, 8)), (64, 32, (64, 32))]
         for mode in (G.RES_BEFORE_NORM, G.RES_AFTER_NORM)] + [(352, 384, (8, 4), G.RES_BEFORE_NORM)]


def make_input(rng, n, c, hw):
    """tests/test_instnorm_gpu.py make_input: per-channel scales from 1e-2 to 30; channel 1: a large mean (100, std 0.1);
    channel 2: constant."""
    x = rng.normal(0, 1, (n,) + hw + (c,)) * np.geomspace(1e-2, 30, c) + rng.normal(0, 0.5, c)
    x[..., 1] = 100 + 0.1 * rng.normal(0, 1, (n,) + hw)
    x[..., 2] = 0.75
    return x.astype(np.float16)


def make_case(K, cout, hw, mode, in_off=0, in_c=None, out_off=0, out_c=None, res_off=0, res_c=None, act='relu', seed=0):
    """-> (graph with ONE FM_OP_CONVIN layer, residual view or None, x [NMAX, h, w, in_c] fp16, r [NMAX, h, w, res_c] fp16).
    Output channel 0 has all-zero weights and a constant residual (a constant channel: variance 0); output channel 1 copies
    input channel 1 (mean 100, std 0.1: E[v^2] - mean^2 in fp32 loses its variance)."""
    rng = np.random.default_rng(seed + K + 3 * cout + hw[0] * hw[1] + mode)
    in_c, out_c, res_c = in_c or K, out_c or cout, res_c or cout
    g = G.Graph(None, hw, in_c)
    g.use_convin = True
    src = g.input.slice(in_off, K)
    dst = g.new(hw[0], hw[1], out_c).slice(out_off, cout)
    res = g.new(hw[0], hw[1], res_c).slice(res_off, cout) if mode != G.RES_NONE else None
    w = rng.normal(0, np.sqrt(1.0 / K), (cout, K, 1, 1)).astype(np.float32) / np.geomspace(1e-2, 30, K).reshape(1, K, 1, 1).astype(np.float32)
    w[0] = 0
    w[1] = 0
    w[1, 1] = 1
    b = rng.normal(0, 0.1, cout).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, cout).astype(np.float32), rng.normal(0, 0.3, cout).astype(np.float32)
    g.convin('tail', src, cout, (gamma, beta), 1e-5, act, res=res, res_mode=mode, wb=(w, b), dst=dst)
    g.outputs = [dst]
    assert len(g.layers) == 1 and g.layers[0]['op'] == G.OP_CONVIN
    x = make_input(rng, NMAX, in_c, hw)
    r = rng.normal(0, 1, (NMAX,) + hw + (res_c,)).astype(np.float16)
    r[..., res_off] = 0.5            # (the constant channel stays constant with the residual inside the norm)
    return g, res, x, r


def reference(g, x, r):
    """The float64 reference and bound of the one-layer graph of make_case for all NMAX samples."""
    d = g.layers[0]
    bufs = {g.input.tid: torch.from_numpy(x.astype(np.float32)).permute(0, 3, 1, 2)}
    if d['res'] is not None:
        bufs[d['res'].tid] = torch.from_numpy(r.astype(np.float32)).permute(0, 3, 1, 2)
    _, ref, bound = run_layer(g, 0, bufs)
    return bufs, ref, bound
