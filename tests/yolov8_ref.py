"""TEST INFRASTRUCTURE: Ultralytics YOLOv8 restated in plain torch from the published source (ultralytics/nn/modules:
Conv, Bottleneck, C2f, SPPF, DFL, Detect; cfg/models/v8/yolov8.yaml for the assembly; the package is not available
here), with seeded parameters, its ONNX export in both exporter forms, the decode's closed form in float64 and the
per-row error bound of the device decode (csrc/dfl_decode.h).

The closed form, for a level of stride s with a gh x gw grid, cell (row, col), box logits b[side][k], sides l, t, r, b:
    d_side = sum_k k softmax(b[side])_k,   ax = col + 0.5, ay = row + 0.5
    x1 = (ax - d_l) s, y1 = (ay - d_t) s, x2 = (ax + d_r) s, y2 = (ay + d_b) s
    Ultralytics' output column: (cx, cy, w, h) = ((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1), then sigmoid(class logits)
    the tracker's candidate row: x1 / in_w, y1 / in_h, (x2 - x1) / in_w, (y2 - y1) / in_h, 1, first argmax, sigmoid(max), index
with the anchors numbered level-major, row-major inside a level.

THE BOUND (dfl_row_bound).  The device evaluates the closed form in fp32, u = 2^-24, every operation rounded once
(-ffp-contract=off), on the SAME fp32 head tensors the float64 reference reads, so the inputs carry no error.
  * x_k = b_k - m (m the side's maximum, exact selection): one rounding, |dx_k| <= u |x_k|.
  * e_k = __expf(x_k) = v_exp_f32(x_k * log2(e)): the product is rounded (relative u) and the constant log2(e) is itself
    rounded (relative u): the base-2 exponent is off by at most 2 u |x_k| log2(e), i.e. a relative error 2 u |x_k| of the
    result; with dx_k that is 3 u |x_k|.  v_exp_f32 is specified to 1 ulp = 2 u; we allow 2 ulp.  So
        |de_k| <= e_k eps_k,  eps_k = 4 u + 3 u |x_k|       (+ 2^-126 absolute where the result is flushed to zero)
    The term of the maximum is exact (x = 0, 2^0 = 1), hence D = sum e_k >= 1: no cancellation anywhere, all terms >= 0.
  * N = sum_k k e_k and D = sum_k e_k: 16 products and 15 additions of non-negative terms, each rounded:
        dN <= sum_k k e_k eps_k + 17 u N,   dD <= sum_k e_k eps_k + 16 u D
  * d = N / D (IEEE division): dd <= (dN + d dD) / (D - dD) + u d.
  * corner: x1 = (ax - d_l) s: ax exact (col + 0.5 < 2^23), subtraction and product rounded; s a power of two or not,
    we charge both: |dx1| <= s (dd_l + 2 u (ax + d_l)).  Likewise the others.
  * row: x = x1 / in_w (one rounding), w = (x2 - x1) / in_w (two); emit_candidate then scales in double and rounds to
    fp32 twice (the product, the offset subtraction).  In frame pixels, S = size / in_w:
        |dX| <= S (|dx1| + u |x1|) + u (|X + off| + |X|)
        |dW| <= S (|dx1| + |dx2| + 2 u (|x1| + |x2|)) + u |W|
  * cls_prob = 1 / (1 + __expf(-z)): the exponential as above with x = -z, one addition, one division:
        |dp| <= p (1 - p) (4 u + 3 u |z|) + 2 u p
  * box_conf (1), the class and the index are exact.
An absolute 1e-37 covers results flushed to zero.  Everything is first order in u with the constants rounded up; the
planted mistakes of tests/test_yolov8_host.py (anchor offset 0, swapped sides, swapped grid axes, no maximum
subtraction, last maximum) miss it by orders of magnitude or change the class."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from resnet_ref import export_with_torch, seeded

REG_MAX = 16
U = 2.0 ** -24


def _autopad(k):
    return k // 2


class Conv(nn.Module):
    """Conv2d(bias=False) + BatchNorm2d + SiLU."""

    def __init__(self, c1, c2, k=1, s=1):
        super().__init__()
        self.conv = nn.Conv2d(c1, c2, k, s, _autopad(k), bias=False)
        self.bn = nn.BatchNorm2d(c2, eps=1e-3, momentum=0.03)

    def forward(self, x):
        return F.silu(self.bn(self.conv(x)))


class Bottleneck(nn.Module):
    def __init__(self, c1, c2, shortcut=True, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1, self.cv2 = Conv(c1, c_, 3, 1), Conv(c_, c2, 3, 1)
        self.add = shortcut and c1 == c2

    def forward(self, x):
        return x + self.cv2(self.cv1(x)) if self.add else self.cv2(self.cv1(x))


class C2f(nn.Module):
    def __init__(self, c1, c2, n=1, shortcut=False, e=0.5):
        super().__init__()
        self.c = int(c2 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv((2 + n) * self.c, c2, 1)
        self.m = nn.ModuleList(Bottleneck(self.c, self.c, shortcut, e=1.0) for _ in range(n))

    def forward(self, x):
        y = list(self.cv1(x).chunk(2, 1))
        y.extend(m(y[-1]) for m in self.m)
        return self.cv2(torch.cat(y, 1))


class SPPF(nn.Module):
    def __init__(self, c1, c2, k=5):
        super().__init__()
        c_ = c1 // 2
        self.cv1, self.cv2 = Conv(c1, c_, 1, 1), Conv(c_ * 4, c2, 1, 1)
        self.m = nn.MaxPool2d(kernel_size=k, stride=1, padding=k // 2)

    def forward(self, x):
        y = [self.cv1(x)]
        y.extend(self.m(y[-1]) for _ in range(3))
        return self.cv2(torch.cat(y, 1))


class DFL(nn.Module):
    def __init__(self, c1=REG_MAX):
        super().__init__()
        self.conv = nn.Conv2d(c1, 1, 1, bias=False).requires_grad_(False)
        self.conv.weight.data[:] = torch.arange(c1, dtype=torch.float).view(1, c1, 1, 1)
        self.c1 = c1

    def forward(self, x):
        b, _, a = x.shape
        return self.conv(x.view(b, 4, self.c1, a).transpose(2, 1).softmax(1)).view(b, 4, a)


def make_anchors(feats, strides, offset=0.5):
    pts, st = [], []
    for f, s in zip(feats, strides):
        h, w = f.shape[2:]
        sx = torch.arange(end=w, dtype=f.dtype) + offset
        sy = torch.arange(end=h, dtype=f.dtype) + offset
        sy, sx = torch.meshgrid(sy, sx, indexing='ij')
        pts.append(torch.stack((sx, sy), -1).view(-1, 2))
        st.append(torch.full((h * w, 1), float(s), dtype=f.dtype))
    return torch.cat(pts), torch.cat(st)


def dist2bbox(distance, anchor_points, dim=1):
    lt, rb = distance.chunk(2, dim)
    x1y1, x2y2 = anchor_points - lt, anchor_points + rb
    return torch.cat(((x1y1 + x2y2) / 2, x2y2 - x1y1), dim)


class Detect(nn.Module):
    def __init__(self, nc, ch, strides, reg_max=REG_MAX):
        super().__init__()
        self.nc, self.reg_max, self.no = nc, reg_max, nc + reg_max * 4
        self.stride = list(strides)
        c2, c3 = max(16, ch[0] // 4, reg_max * 4), max(ch[0], min(nc, 100))
        self.cv2 = nn.ModuleList(nn.Sequential(Conv(x, c2, 3), Conv(c2, c2, 3), nn.Conv2d(c2, 4 * reg_max, 1)) for x in ch)
        self.cv3 = nn.ModuleList(nn.Sequential(Conv(x, c3, 3), Conv(c3, c3, 3), nn.Conv2d(c3, nc, 1)) for x in ch)
        self.dfl = DFL(reg_max)
        self.anchor_offset = 0.5
        self.heads = None                       # the last forward's per-level (box, cls) head tensors

    def forward(self, x):
        self.heads = [(self.cv2[i](x[i]), self.cv3[i](x[i])) for i in range(len(x))]
        x = [torch.cat(h, 1) for h in self.heads]
        shape = x[0].shape
        x_cat = torch.cat([xi.view(shape[0], self.no, -1) for xi in x], 2)
        anchors, strides = (t.transpose(0, 1) for t in make_anchors(x, self.stride, self.anchor_offset))
        box, cls = x_cat.split((self.reg_max * 4, self.nc), 1)
        dbox = dist2bbox(self.dfl(box), anchors.unsqueeze(0), dim=1) * strides
        return torch.cat((dbox, cls.sigmoid()), 1)


class YOLOv8(nn.Module):
    """yolov8.yaml with channel widths w = (P1 .. P5) and depths d = (C2f repeats of the four backbone stages); the head's
    C2f blocks repeat d[0] times.  levels: 3 (P3, P4, P5) or 2 (P3, P4: the P5 branch of the head is left out)."""

    def __init__(self, w=(16, 32, 64, 128, 256), d=(1, 2, 2, 1), nc=80, levels=3):
        super().__init__()
        w1, w2, w3, w4, w5 = w
        n = d[0]
        self.b0, self.b1, self.b2 = Conv(3, w1, 3, 2), Conv(w1, w2, 3, 2), C2f(w2, w2, d[0], True)
        self.b3, self.b4 = Conv(w2, w3, 3, 2), C2f(w3, w3, d[1], True)
        self.b5, self.b6 = Conv(w3, w4, 3, 2), C2f(w4, w4, d[2], True)
        self.b7, self.b8, self.b9 = Conv(w4, w5, 3, 2), C2f(w5, w5, d[3], True), SPPF(w5, w5, 5)
        self.h12, self.h15 = C2f(w5 + w4, w4, n), C2f(w4 + w3, w3, n)
        self.h16, self.h18 = Conv(w3, w3, 3, 2), C2f(w3 + w4, w4, n)
        self.levels = levels
        if levels == 3:
            self.h19, self.h21 = Conv(w4, w4, 3, 2), C2f(w4 + w5, w5, n)
        self.detect = Detect(nc, (w3, w4, w5)[:levels], (8, 16, 32)[:levels])

    def forward(self, x):
        x = self.b2(self.b1(self.b0(x)))
        p3 = self.b4(self.b3(x))
        p4 = self.b6(self.b5(p3))
        p5 = self.b9(self.b8(self.b7(p4)))
        up = lambda t: F.interpolate(t, scale_factor=2.0, mode='nearest')          # noqa: E731
        n4 = self.h12(torch.cat([up(p5), p4], 1))
        o3 = self.h15(torch.cat([up(n4), p3], 1))
        o4 = self.h18(torch.cat([self.h16(o3), n4], 1))
        outs = [o3, o4]
        if self.levels == 3:
            outs.append(self.h21(torch.cat([self.h19(o4), p5], 1)))
        return self.detect(outs)


def seeded_v8(net, seed, cls_bias=None):
    """resnet_ref.seeded (variance-preserving convs, non-trivial BatchNorm statistics) with the DFL weights put back.
    cls_bias: added to the bias of every class-branch head conv (sets the fraction of cells over a threshold)."""
    seeded(net, seed)
    with torch.no_grad():
        c1 = net.detect.dfl.c1
        net.detect.dfl.conv.weight.copy_(torch.arange(c1, dtype=torch.float).view(1, c1, 1, 1))
        if cls_bias is not None:
            for seq in net.detect.cv3:
                seq[-1].bias.add_(float(cls_bias))
    return net


TINY_HW = (64, 96)


def tiny(nc=3, levels=3, seed=5, cls_bias=None):
    """Width 16 / 32, one repeat everywhere; at 64 x 96 the grids are 8 x 12, 4 x 6 and 2 x 3."""
    return seeded_v8(YOLOv8((16, 16, 16, 32, 32), (1, 1, 1, 1), nc, levels), seed, cls_bias)


def yolov8n(nc=80, seed=11, cls_bias=None):
    return seeded_v8(YOLOv8((16, 32, 64, 128, 256), (1, 2, 2, 1), nc), seed, cls_bias)


def yolov8s(nc=80, seed=12):
    return seeded_v8(YOLOv8((32, 64, 128, 256, 512), (1, 2, 2, 1), nc), seed)


def export(net, hw=TINY_HW, folded=True):
    """-> bytes of the ONNX file.  folded: the exporter's default (BatchNorm folded into the convs, constants folded: the
    anchors and strides arrive as initialisers); otherwise explicit BatchNormalization nodes, the module's parameter
    names and every shape computation as nodes (`chunk` as Shape / Gather / Add / Div / Mul / Slice)."""
    x = torch.zeros(1, 3, *hw)
    if folded:
        return export_with_torch(net, x)
    return export_with_torch(net, x, training=torch.onnx.TrainingMode.PRESERVE, do_constant_folding=False,
                             keep_initializers_as_inputs=True)


def module_heads(net, x):
    """-> (the module's output [N, 4 + nc, A] float64, [(box [N, 64, gh, gw], cls [N, nc, gh, gw])] per level, float32)."""
    with torch.no_grad():
        y = net(torch.as_tensor(x, dtype=torch.float32))
    return y.double().numpy(), [(b.numpy(), c.numpy()) for b, c in net.detect.heads]


# ------------------------------------------------------------------------------------------------ closed form
def dfl_expectation(box):
    """box [..., 4, 16] -> (d [..., 4] float64, the bound dd of the fp32 evaluation, see the module docstring)."""
    b = np.asarray(box, np.float64)
    x = b - b.max(-1, keepdims=True)
    e = np.exp(x)
    k = np.arange(b.shape[-1], dtype=np.float64)
    eps = 4 * U + 3 * U * np.abs(x)
    N, D = (k * e).sum(-1), e.sum(-1)
    d = N / D
    dN = (k * e * eps).sum(-1) + 17 * U * N + 16 * 15 * 2.0 ** -126
    dD = (e * eps).sum(-1) + 16 * U * D + 16 * 2.0 ** -126
    return d, (dN + d * dD) / (D - dD) + U * d


def dfl_decode(heads, strides, in_hw, offset=0.5):
    """heads: [(box [64, gh, gw], cls [nc, gh, gw])] per level (one image) -> dict of float64 arrays over the anchors in
    level-major order: x1, y1, x2, y2 (input pixels) with their bounds dx1 .., cls (first maximum), logit, prob, dprob."""
    out = {k: [] for k in ('x1', 'y1', 'x2', 'y2', 'dx1', 'dy1', 'dx2', 'dy2', 'cls', 'logit')}
    for (box, cls), s in zip(heads, strides):
        _, gh, gw = box.shape
        b = np.asarray(box, np.float64).reshape(4, REG_MAX, gh * gw).transpose(2, 0, 1)
        d, dd = dfl_expectation(b)
        cell = np.arange(gh * gw)
        ax, ay = cell % gw + offset, cell // gw + offset
        s = float(s)
        for name, a, sign, i in (('x1', ax, -1, 0), ('y1', ay, -1, 1), ('x2', ax, 1, 2), ('y2', ay, 1, 3)):
            out[name].append((a + sign * d[:, i]) * s)
            out['d' + name].append(s * (dd[:, i] + 2 * U * (a + d[:, i])))
        logits = np.asarray(cls, np.float64).reshape(cls.shape[0], gh * gw)
        c = logits.argmax(0)                     # (numpy: the first maximum)
        out['cls'].append(c)
        out['logit'].append(logits[c, cell])
    out = {k: np.concatenate(v) for k, v in out.items()}
    z = out['logit']
    p = 1.0 / (1.0 + np.exp(-z))
    out['prob'] = p
    out['dprob'] = p * (1 - p) * (4 * U + 3 * U * np.abs(z)) + 2 * U * p + 1e-37
    return out


def ultralytics_output(dec, heads):
    """The module's own output [4 + nc, A] from the closed form: (cx, cy, w, h), then the class sigmoids."""
    probs = np.concatenate([1.0 / (1.0 + np.exp(-np.asarray(c, np.float64).reshape(c.shape[0], -1))) for _, c in heads], 1)
    x1, y1, x2, y2 = (dec[k] for k in ('x1', 'y1', 'x2', 'y2'))
    return np.concatenate([np.stack([(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1]), probs])


def dfl_rows(dec, in_hw, size, offset):
    """The tracker's candidate rows of every anchor, float64, and their bound: [A, 8] each, columns x, y, w, h (frame
    pixels: fractions of the input scaled by `size`, minus `offset`), box_conf, class, cls_prob, index."""
    in_h, in_w = in_hw
    A = len(dec['x1'])
    rows, bound = np.zeros((A, 8)), np.zeros((A, 8))
    for col, (lo, hi, n, sz, off) in enumerate((('x1', 'x2', in_w, size[0], offset[0]), ('y1', 'y2', in_h, size[1], offset[1]))):
        S = sz / n
        a, b, da, db = dec[lo], dec[hi], dec['d' + lo], dec['d' + hi]
        X = a * S - off
        W = (b - a) * S
        rows[:, col], rows[:, 2 + col] = X, W
        bound[:, col] = S * (da + U * np.abs(a)) + U * (np.abs(X + off) + np.abs(X)) + 1e-37
        bound[:, 2 + col] = S * (da + db + 2 * U * (np.abs(a) + np.abs(b))) + U * np.abs(W) + 1e-37
    rows[:, 4], rows[:, 5], rows[:, 6], rows[:, 7] = 1.0, dec['cls'], dec['prob'], np.arange(A)
    bound[:, 6] = dec['dprob']
    return rows, bound


# fp32 evaluation of the closed form in the device's order: the host stand-in tests/test_yolov8_host.py plants mistakes in
def dfl_rows_fp32(heads, strides, in_hw, size, offset, mistake=None):
    f = np.float32
    in_h, in_w = in_hw
    rows = []
    base = 0
    for (box, cls), s in zip(heads, strides):
        _, gh, gw = box.shape
        if mistake == 'grid':
            gh, gw = gw, gh
        b = np.asarray(box, f).reshape(4, REG_MAX, -1).transpose(2, 0, 1)
        if mistake == 'lt':
            b = b[:, [1, 0, 2, 3]]
        m = b.max(-1, keepdims=True) if mistake != 'nomax' else np.zeros_like(b[..., :1])
        with np.errstate(over='ignore', invalid='ignore'):
            e = np.exp((b - m).astype(f)).astype(f)
            k = np.arange(REG_MAX, dtype=f)
            d = ((k * e).astype(f).sum(-1, dtype=f) / e.sum(-1, dtype=f)).astype(f)
        cell = np.arange(b.shape[0])
        off = f(0.0 if mistake == 'offset' else 0.5)
        ax, ay = (cell % gw).astype(f) + off, (cell // gw).astype(f) + off
        x1, y1 = (ax - d[:, 0]) * f(s), (ay - d[:, 1]) * f(s)
        x2, y2 = (ax + d[:, 2]) * f(s), (ay + d[:, 3]) * f(s)
        logits = np.asarray(cls, f).reshape(cls.shape[0], -1)
        c = logits.argmax(0) if mistake != 'last' else logits.shape[0] - 1 - logits[::-1].argmax(0)
        z = logits[c, cell]
        p = (f(1) / (f(1) + np.exp(-z).astype(f))).astype(f)
        r = np.zeros((len(cell), 8))
        r[:, 0] = ((x1 / f(in_w)).astype(f).astype(np.float64) * size[0]).astype(f).astype(np.float64) - offset[0]
        r[:, 1] = ((y1 / f(in_h)).astype(f).astype(np.float64) * size[1]).astype(f).astype(np.float64) - offset[1]
        r[:, 2] = (((x2 - x1) / f(in_w)).astype(f).astype(np.float64) * size[0])
        r[:, 3] = (((y2 - y1) / f(in_h)).astype(f).astype(np.float64) * size[1])
        r[:, :4] = r[:, :4].astype(f)
        r[:, 4], r[:, 5], r[:, 6], r[:, 7] = 1, c, p, base + cell
        rows.append(r)
        base += len(cell)
    return np.concatenate(rows)
