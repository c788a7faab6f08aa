"""TEST INFRASTRUCTURE for the MobileNet separable block and the SSD-MobileNetV1 tables (fastmot_amd/models/ssd.py):
plain PyTorch restatements written from the TensorFlow semantics, not from the kernels.

  * `same_pad` / `pad_same`: TF "SAME" padding.  out = ceil(in / s), total = max((out - 1) * s + k - in, 0),
    before = total // 2, after = total - before: an even map at stride 2 pads (0, 1), an odd one (1, 1).
  * `sep_block`: act(W_pw . act(dw3x3(x) + b_dw) + b_pw) in float64 from given (fp16-valued) inputs with the
    per-element bound of DESIGN.md section 7 composed from its two stages exactly as tests/torch_ref.py composes the
    stages of the other fused ops: stage bound d_pre = |W| (*) d_in + K u32 S, the fp16 intermediate
    d = L d_pre (1 + u16) + u16 |t| + 2^-24 feeding the next stage, the stored output rounded once more.
    (torch_ref's L = 1.1 covers ReLU6, whose slope is at most 1.)
    `variant` plants one of the mistakes a kernel author makes here (tests/test_sepconv_host.py).
  * `layer_ref`: one layer of a table built from the ops of an SSD network (stem / plain convs with TF SAME padding,
    FM_OP_DWCONV, FM_OP_SEPCONV) from the tensors the device produced ("teacher forcing") -> (reference, bound).
"""
import numpy as np
import torch
import torch.nn.functional as F

import torch_ref as T
from fastmot_amd.models import graph as G

RELU6 = G.ACT['relu6']


def act_fn(x, act):
    return x.clamp(0, 6) if act == RELU6 else T.act_fn(x, act)


def same_pad(n, k, stride):
    out = -(-n // stride)
    total = max((out - 1) * stride + k - n, 0)
    return total // 2, total - total // 2


def pad_same(x, k, stride, symmetric=False):
    """x [N, C, H, W] zero-padded for a k x k window at `stride`; symmetric=True is the planted mistake (k // 2 on every side)."""
    if symmetric:
        return F.pad(x, (k // 2,) * 4)
    (t, b), (l, r) = same_pad(x.shape[2], k, stride), same_pad(x.shape[3], k, stride)
    return F.pad(x, (l, r, t, b))


def _t(a, dt=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to(dt)


def conv_stage(x, xe, w, b, act, k, stride, groups=1, symmetric=False, dt=torch.float64, track=True):
    """One stage act(conv_SAME(x) + b) -> (value, bound before storage); xe: bound on x (tensor or 0.0)."""
    w, b = _t(w, dt), _t(b, dt)
    kw = dict(stride=stride, groups=groups)
    xp = pad_same(x, k, stride, symmetric)
    y = F.conv2d(xp, w, b, **kw)
    e = None
    if track:
        K = w[0].numel()
        S = F.conv2d(xp.abs(), w.abs(), b.abs(), **kw)
        e = K * T.U32 * S
        if torch.is_tensor(xe):
            e = e + F.conv2d(pad_same(xe, k, stride), w.abs(), None, **kw)
        e = T.L_ACT * e
    return act_fn(y, act), e


def store16(v, e):
    return e * (1 + T.U16) + T.U16 * v.abs() + T.SUB16


def dw_layer(x, w, b, act, stride):
    """FM_OP_DWCONV from exact inputs x [N, C, H, W] -> (ref, bound of the stored fp16 tensor)."""
    x = x.to(torch.float64)
    v, e = conv_stage(x, 0.0, w, b, act, 3, stride, groups=x.shape[1])
    return v, store16(v, e)


def pw_layer(t, w, b, act):
    """The pointwise stage alone from an exact (fp16-valued) intermediate t -> (ref, bound of the stored fp16 tensor)."""
    v, e = conv_stage(t.to(torch.float64), 0.0, w, b, act, 1, 1)
    return v, store16(v, e)


def sep_block(x, sep_ref, act2, stride, variant=None, dt=torch.float64):
    """x [N, C, H, W] (values the device holds in fp16).  dt float64, variant None: -> (ref, bound, depthwise ref).
    dt float32: a host stand-in for the device (the intermediate and the result rounded to fp16, no bound)."""
    wd, bd, act1, wp, bp = sep_ref
    x = x.to(dt)
    track = dt == torch.float64 and variant is None
    a1 = G.ACT['relu'] if variant == 'relu' else act1
    a2 = G.ACT['relu'] if variant == 'relu' else act2
    t, te = conv_stage(x, 0.0, wd, bd, a1, 3, stride, groups=x.shape[1], symmetric=variant == 'symmetric', dt=dt, track=track)
    if variant == 'symmetric' and t.shape[2:] != (-(-x.shape[2] // stride), -(-x.shape[3] // stride)):
        t = t[:, :, :-(-x.shape[2] // stride), :-(-x.shape[3] // stride)]
    if track:
        te = store16(t, te)
    elif variant != 'unrounded':
        t = t.half().to(dt)
    y, ye = conv_stage(t, te, wp, bp, a2, 1, 1, dt=dt, track=track)
    if track:
        return y, store16(y, ye), t
    return y.half().to(dt), None, t


def layer_ref(graph, idx, bufs):
    """Layer `idx` of an SSD table from the device's own input tensor bufs[tid] ([N, cpad, h, w]) -> (ref, bound) for the
    channels of its output view."""
    d = graph.layers[idx]
    v = d['ins'][0]
    x = bufs[v.tid][:, v.coff:v.coff + v.c].to(torch.float64)
    f32 = bool(graph.tensors[d['out'].tid][3])
    if d['op'] == G.OP_SEPCONV:
        y, e, _ = sep_block(x, d['sep_ref'], d['act'], d['stride'])
        return y, e
    params = {i: (w, b) for i, w, b in graph.conv_params}
    w, b = params[idx]
    if d['op'] == G.OP_DWCONV:
        return dw_layer(x, w, b, d['act'], d['stride'])
    assert d['op'] in G.CONV_OPS + (G.OP_STEMCONV,) and d['res'] is None and d['up'] == 1, d['op']
    y, e = conv_stage(x, 0.0, w, b, d['act'], d['k'], d['stride'])
    return y, (e + T.FAST_EXP * y.abs() if f32 else store16(y, e))


def run_table(graph, x, dt=torch.float32):
    """The whole table in fp32 from the network input x [N, C, H, W], every stored activation rounded to fp16 where the
    engine rounds it (the separable block's intermediate included): the stand-in for tests/torch_ref.run_graph on SSD
    tables, for the whole-tensor bar of tests/test_fullsize_gpu.py.  -> {tid: [N, cpad, h, w]}"""
    n = x.shape[0]
    bufs = {tid: torch.zeros(n, c, h, w, dtype=dt) for tid, (h, w, c, f32) in enumerate(graph.tensors)}
    bufs[graph.input.tid][:, :x.shape[1]] = x.to(dt).half().to(dt)
    params = {i: (w, b) for i, w, b in graph.conv_params}
    for idx, d in enumerate(graph.layers):
        v, o = d['ins'][0], d['out']
        xin = bufs[v.tid][:, v.coff:v.coff + v.c]
        if d['op'] == G.OP_SEPCONV:
            y = sep_block(xin, d['sep_ref'], d['act'], d['stride'], dt=dt, variant='stand-in')[0]
        else:
            w, b = params[idx]
            groups = xin.shape[1] if d['op'] == G.OP_DWCONV else 1
            y = conv_stage(xin, 0.0, w, b, d['act'], d['k'], d['stride'], groups=groups, dt=dt, track=False)[0]
            if not graph.tensors[o.tid][3]:
                y = y.half().to(dt)
        bufs[o.tid][:, o.coff:o.coff + o.c] = y
    return bufs


def random_variables(model, seed=0):
    """{TF variable name: float32 array} for every variable of model.variable_shapes(): variance-preserving kernels,
    BatchNorm statistics around the identity -- what a frozen graph of the model would hold, with made-up values."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in model.variable_shapes().items():
        leaf = name.rsplit('/', 1)[1]
        if leaf == 'weights':
            a = rng.normal(0, np.sqrt(1.0 / (shape[0] * shape[1] * shape[2])), shape)
        elif leaf == 'depthwise_weights':
            a = rng.normal(0, np.sqrt(1.0 / 9), shape)
        elif leaf in ('gamma', 'moving_variance'):
            a = rng.uniform(0.8, 1.2, shape)
        else:
            a = rng.normal(0, 0.1, shape)
        out[name] = a.astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------- decode + NMS + top-K
# A float64 restatement of NMS_TRT as the reference configures it (reference models/ssd.py:136-150: shareLocation,
# backgroundLabelId 0, confidenceThreshold 1e-8, topK = keepTopK, confSigmoid, isNormalized, TF-centre box coding), written
# from those semantics: per tile and anchor the box and the per-class sigmoid scores; per (tile, class != 0) the topk
# highest scores above 1e-8 and greedy NMS among them (IoU without +1, dropped when > thresh against a kept higher-scored
# box); per tile the topk highest-scored survivors over all classes, descending; ties by (class, anchor) ascending.
def split_heads(heads, anchors_per_cell, num_classes):
    """heads[k] [n_tiles, cells, A * (4 + C)] -> (loc [n_tiles, n_anchors, 4], logits [n_tiles, n_anchors, C]) in anchor order."""
    loc, logit = [], []
    for h, a in zip(heads, anchors_per_cell):
        h = np.asarray(h, np.float64)
        n, cells, _ = h.shape
        loc.append(h[:, :, :a * 4].reshape(n, cells * a, 4))
        logit.append(h[:, :, a * 4:a * (4 + num_classes)].reshape(n, cells * a, num_classes))
    return np.concatenate(loc, 1), np.concatenate(logit, 1)


def decode(loc, logits, anchors, box_scales):
    """-> (boxes [n_tiles, n_anchors, 4] as (xmin, ymin, xmax, ymax), scores [n_tiles, n_anchors, C]), float64"""
    an = np.asarray(anchors, np.float64)
    t = loc / np.asarray(box_scales, np.float64)
    cy, cx = t[..., 0] * an[:, 2] + an[:, 0], t[..., 1] * an[:, 3] + an[:, 1]
    h, w = np.exp(t[..., 2]) * an[:, 2], np.exp(t[..., 3]) * an[:, 3]
    boxes = np.clip(np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1), 0., 1.)
    return boxes, 1. / (1. + np.exp(-logits))


def iou(a, b):
    iw, ih = min(a[2], b[2]) - max(a[0], b[0]), min(a[3], b[3]) - max(a[1], b[1])
    if iw <= 0 or ih <= 0:
        return 0.
    inter = iw * ih
    union = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
    return inter / union if union > 0 else 0.


def nms_topk(boxes, scores, topk, thresh, stats=None):
    """-> rows float64 [n_tiles * topk, 7] (tile, label, conf, xmin, ymin, xmax, ymax), padding rows (tile, -1, 0, 0, 0, 0, 0),
    and the anchor index of every row (-1 for padding).  stats (a dict): max candidates per class, max survivors per tile,
    the IoUs that were compared."""
    n_tiles, n_anchors, n_classes = scores.shape
    rows = np.zeros((n_tiles, topk, 7))
    which = np.full((n_tiles, topk), -1, int)
    ious, max_cand, max_surv = [], 0, 0
    for t in range(n_tiles):
        survivors = []
        for c in range(1, n_classes):
            s = scores[t, :, c]
            cand = [a for a in range(n_anchors) if s[a] > 1e-8]
            max_cand = max(max_cand, len(cand))
            cand.sort(key=lambda a: (-s[a], a))
            kept = []
            for a in cand[:topk]:
                ok = True
                for b in kept:
                    v = iou(boxes[t, b], boxes[t, a])
                    ious.append(v)
                    if v > thresh:
                        ok = False
                        break
                if ok:
                    kept.append(a)
            survivors += [(-s[a], c, a) for a in kept]
        max_surv = max(max_surv, len(survivors))
        survivors.sort()
        rows[t, :, 0], rows[t, :, 1] = t, -1
        for r, (neg, c, a) in enumerate(survivors[:topk]):
            rows[t, r, 1:] = [c, -neg, *boxes[t, a]]
            which[t, r] = a
    if stats is not None:
        stats.update(max_candidates=max_cand, max_survivors=max_surv, ious=np.array(ious))
    return rows.reshape(-1, 7), which.reshape(-1)


def postprocess(heads, model, topk=None, thresh=None, stats=None):
    loc, logits = split_heads(heads, [model.anchors_per_cell(k) for k in range(len(heads))], model.NUM_CLASSES)
    boxes, scores = decode(loc, logits, model.anchors(), model.BOX_SCALES)
    return nms_topk(boxes, scores, model.TOPK if topk is None else topk, model.NMS_THRESH if thresh is None else thresh, stats)
