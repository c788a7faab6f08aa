"""ONNX exports of anchor-free detectors with a DFL head (Ultralytics YOLOv8, `yolo export format=onnx`) -> layer
tables of the HIP conv engine plus the description of their heads for csrc/dfl_decode.h.

A general walker over the file's own node list (ONNX nodes are topologically sorted), in three steps.

1. Folding.  Every node whose inputs are constants is evaluated with a small numpy interpreter (`_np_op`), `Shape` of a
   map included: the `Shape / Gather / Add / Div / Mul / Slice` chains that `chunk(2, 1)` exports to, the `Concat` of
   scales in front of a `Resize`, the anchor grid of the head (`Expand`, `Unsqueeze`, `Reshape`, ...) all become constants.
2. The network, up to the head convolutions:
     Conv                 group 1, dilation 1, symmetric pads k // 2, k in {1, 3}, stride in {1, 2}; the 3-channel stem goes
                          to FM_OP_STEMCONV (Graph.conv decides)
     BatchNormalization   behind a conv and read by nothing else: folded with the node's epsilon
     Sigmoid + Mul        of the same value: act='swish' of the producing conv
     Add                  of a conv's activated output, read by the Add alone, with a stored value: `res=`, RES_AFTER_ACT
                          (any other Add of two stored values: FM_OP_ADD)
     Concat (axis 1)      ONE tensor; the producers write their slices in place (`dst=`), a value with several readers
                          stays readable as the slice.  A conv output whose channel views (Split / Slice) enter the concat
                          in order is written there whole (C2f: cv1's two halves).  A value that already lives elsewhere --
                          in an earlier concat, or a view of a value with other readers -- is copied in (FM_OP_COPY).  Slice
                          offsets are multiples of 8 channels, or the node is refused
     Split / Slice (axis 1)   channel views
     MaxPool              5x5 stride 1 pads 2.  SPPF -- three chained pools, each read by the next pool and the concat only,
                          [x | p1 | p2 | p3] -> Conv -- is ONE FM_OP_SPP launch: chained 5x5 maxima ARE the 5x5, 9x9 and 13x13
                          maxima of x (max is exact and associative), the op writes [13 | 9 | 5] in front of x, and the
                          input-channel blocks of the conv behind the concat are reordered to match
     Resize               nearest, scales (1, 1, 2, 2), asymmetric / floor: folded into a producing 1x1 conv that nothing else
                          reads (`up=2`), otherwise FM_OP_UPSAMPLE2
     Identity, Constant
3. The head.  A Conv without activation ends the network: its output is an fp32 head tensor.  Ultralytics' `Detect` has
   two per level, joined by a 2-input Concat (box logits first, 4 * reg_max channels; class logits second).  Everything
   behind them -- the embedded decode -- is NOT trusted and NOT executed on the device: it is evaluated here in float64
   with `_np_op` on seeded head tensors (ties and logits of +-30 included) and compared with the closed form that
   csrc/dfl_decode.h implements (`closed_form`): reg_max = 16, anchor point (col + 0.5, row + 0.5), stride = input / grid,
   output (cx, cy, w, h) in input pixels followed by the class sigmoids, anchors level-major.  A tail that computes
   anything else is refused naming the graph output.

Refused with the node's name, before anything touches the device: grouped / depthwise / dilated convs, asymmetric
pads, MatMul and every other operator not listed (attention blocks, NonMaxSuppression / TopK of end-to-end exports), a
dynamic batch or spatial dimension, a batch other than 1, a second graph output (segmentation, pose, OBB), reg_max != 16,
more than FM_MAX_HEADS levels, more than 128 classes, strides that are not input / grid, an initialiser nothing reads.

The graph forms were derived from the published Ultralytics source restated in torch and the torch exporter at hand
(tests/yolov8_ref.py) plus a hand-written "simplified" form; they are not pinned against a real Ultralytics file.
"""
import numpy as np

from .graph import Graph, RES_AFTER_ACT, SPP_MAX_HW
from .onnx_reader import OnnxModel

REG_MAX = 16
MAX_LEVELS = 4            # FM_MAX_HEADS
MAX_CLASSES = 128


class Unsupported(NotImplementedError):
    pass


def _fail(node, what):
    raise Unsupported(f'node {node.name or node.outputs[0]!r} ({node.op}): {what}')


# ------------------------------------------------------------------------------------------------ numpy interpreter
def _softmax(x, axis, opset):
    axis %= x.ndim
    if opset is not None and opset < 13 and axis != x.ndim - 1:      # (before opset 13: over the flattened trailing dimensions)
        flat = x.reshape(int(np.prod(x.shape[:axis], dtype=np.int64)), -1)
        return _softmax(flat, 1, 13).reshape(x.shape)
    e = np.exp(x - x.max(axis, keepdims=True))
    return e / e.sum(axis, keepdims=True)


def _np_op(node, a, opset):
    """One node on numpy arrays `a` (None for an omitted optional input) -> list of outputs.  Floats are float64."""
    op, at = node.op, node.attrs
    isint = lambda v: np.issubdtype(np.asarray(v).dtype, np.integer)         # noqa: E731
    if op == 'Identity':
        return [a[0]]
    if op == 'Shape':
        return [np.array(a[0].shape, np.int64)]
    if op == 'Gather':
        return [np.take(a[0], np.asarray(a[1], np.int64), axis=at.get('axis', 0))]
    if op in ('Add', 'Sub', 'Mul'):
        return [{'Add': np.add, 'Sub': np.subtract, 'Mul': np.multiply}[op](a[0], a[1])]
    if op == 'Div':
        if isint(a[0]) and isint(a[1]):
            return [(np.sign(a[0]) * np.sign(a[1]) * (np.abs(a[0]) // np.abs(a[1]))).astype(np.int64)]     # (truncating)
        return [np.divide(a[0], a[1])]
    if op == 'Cast':
        to = {1: np.float64, 11: np.float64, 10: np.float64, 6: np.int64, 7: np.int64, 9: np.bool_}.get(at.get('to'))
        if to is None:
            _fail(node, f'cast to ONNX type {at.get("to")}')
        return [np.asarray(a[0]).astype(to)]
    if op == 'Concat':
        return [np.concatenate([np.atleast_1d(v) for v in a], axis=at['axis'])]
    if op in ('Unsqueeze', 'Squeeze'):
        axes = at.get('axes') if at.get('axes') is not None else (None if len(a) < 2 or a[1] is None else [int(v) for v in a[1]])
        x = np.asarray(a[0])
        if op == 'Squeeze':
            return [np.squeeze(x, axis=None if axes is None else tuple(axes))]
        for ax in sorted(ax % (x.ndim + len(axes)) for ax in axes):
            x = np.expand_dims(x, ax)
        return [x]
    if op == 'Reshape':
        x, shape = np.asarray(a[0]), [int(v) for v in a[1]]
        shape = [x.shape[i] if s == 0 else s for i, s in enumerate(shape)]
        return [x.reshape(shape)]
    if op == 'Transpose':
        return [np.transpose(a[0], at.get('perm'))]
    if op == 'Expand':
        x, shape = np.asarray(a[0]), [int(v) for v in a[1]]
        return [x * np.ones(shape, x.dtype)]
    if op == 'Slice':
        x = np.asarray(a[0])
        if len(a) == 1:
            starts, ends, axes, steps = at['starts'], at['ends'], at.get('axes'), None
        else:
            starts, ends = a[1], a[2]
            axes = a[3] if len(a) > 3 else None
            steps = a[4] if len(a) > 4 else None
        starts, ends = [int(v) for v in np.atleast_1d(starts)], [int(v) for v in np.atleast_1d(ends)]
        axes = list(range(len(starts))) if axes is None else [int(v) for v in np.atleast_1d(axes)]
        steps = [1] * len(starts) if steps is None else [int(v) for v in np.atleast_1d(steps)]
        idx = [slice(None)] * x.ndim
        for s, e, ax, st in zip(starts, ends, axes, steps):
            idx[ax] = slice(s, e, st)            # (python clamps as ONNX does)
        return [x[tuple(idx)]]
    if op == 'Split':
        x, axis = np.asarray(a[0]), at.get('axis', 0)
        split = at.get('split') if at.get('split') is not None else (None if len(a) < 2 or a[1] is None else [int(v) for v in a[1]])
        if split is None:
            split = [x.shape[axis] // len(node.outputs)] * len(node.outputs)
        return np.split(x, np.cumsum(split)[:-1], axis=axis)
    if op == 'Softmax':
        return [_softmax(np.asarray(a[0], np.float64), at.get('axis', -1 if opset and opset >= 13 else 1), opset)]
    if op == 'Sigmoid':
        return [1.0 / (1.0 + np.exp(-np.asarray(a[0], np.float64)))]
    if op == 'Range':
        return [np.arange(a[0], a[1], a[2])]
    if op == 'ConstantOfShape':
        v = at['value'].array().reshape(-1)[0] if at.get('value') is not None else 0.0
        return [np.full([int(s) for s in a[0]], v)]
    if op == 'Conv':        # (the DFL expectation: a pointwise conv)
        x, w = np.asarray(a[0], np.float64), np.asarray(a[1], np.float64)
        if (w.ndim != 4 or w.shape[2:] != (1, 1) or at.get('group', 1) != 1 or any(at.get('pads', [0])) or
                any(s != 1 for s in at.get('strides', [1]))):
            _fail(node, 'only a pointwise convolution is expected behind the head tensors')
        y = np.einsum('oc,nchw->nohw', w[:, :, 0, 0], x)
        return [y if len(a) < 3 or a[2] is None else y + np.asarray(a[2], np.float64).reshape(1, -1, 1, 1)]
    _fail(node, 'operator not supported (see fastmot_amd/models/onnx_detector.py for the list)')


def closed_form(heads, strides, in_hw):
    """heads: [(box [1, 64, gh, gw], cls [1, nc, gh, gw])] per level -> [1, 4 + nc, A] float64: what csrc/dfl_decode.h
    computes before the tracker's own row convention, in Ultralytics' output layout (cx, cy, w, h, class sigmoids)."""
    cols = []
    for (box, cls), s in zip(heads, strides):
        _, _, gh, gw = box.shape
        b = np.asarray(box, np.float64).reshape(4, REG_MAX, gh * gw)
        e = np.exp(b - b.max(1, keepdims=True))
        d = (e * np.arange(REG_MAX)[None, :, None]).sum(1) / e.sum(1)
        cell = np.arange(gh * gw)
        ax, ay = cell % gw + 0.5, cell // gw + 0.5
        x1, y1, x2, y2 = (ax - d[0]) * s, (ay - d[1]) * s, (ax + d[2]) * s, (ay + d[3]) * s
        p = 1.0 / (1.0 + np.exp(-np.asarray(cls, np.float64).reshape(cls.shape[1], gh * gw)))
        cols.append(np.concatenate([np.stack([(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1]), p]))
    return np.concatenate(cols, 1)[None]


# ------------------------------------------------------------------------------------------------ the walker
class DflHeadsInfo:
    """What the decode needs to know: per level the (box, class) head views and the stride."""

    def __init__(self, levels, strides, num_classes, in_hw):
        self.levels, self.strides, self.num_classes, self.in_hw = levels, strides, num_classes, in_hw


class _Walk:
    def __init__(self, model, where, sppf_as_spp=True):
        self.m, self.where, self.sppf_as_spp = model, where, sppf_as_spp
        self.nodes = model.nodes
        self.readers = {}
        for i, nd in enumerate(self.nodes):
            for t in nd.inputs:
                if t:
                    self.readers.setdefault(t, []).append(i)
        self.const = {}          # value name -> numpy array
        self.shape = {}          # map value name -> (c, h, w)
        self.view_of = {}        # channel view name -> (parent name, offset, channels)
        self.done = set()        # node indices that are accounted for
        self.from_const_node = {nd.outputs[0] for nd in self.nodes if nd.op == 'Constant'}

    # ---------------------------------------------------------------- constants
    def cget(self, name):
        if name == '':
            return None
        if name in self.const:
            return self.const[name]
        if self.m.has(name):
            a = self.m.tensor(name)
            a = a.astype(np.float64) if np.issubdtype(a.dtype, np.floating) else a.astype(np.int64)
            self.const[name] = a
            return a
        raise KeyError(name)

    def is_const(self, name):
        return name == '' or name in self.const or self.m.has(name)

    def users(self, name):
        return [self.nodes[i] for i in self.readers.get(name, [])]

    def sole(self, name, op):
        u = self.users(name)
        return u[0] if len(u) == 1 and u[0].op == op else None

    # ---------------------------------------------------------------- step 1: fold constants, infer the maps' shapes
    def fold(self):
        (in_name, in_shape), = self.m.data_inputs[:1] or [(None, None)]
        if len(self.m.data_inputs) != 1:
            raise Unsupported(f'{self.where}: {len(self.m.data_inputs)} data inputs, expected one image tensor')
        if in_shape is None or len(in_shape) != 4 or any(d is None or d <= 0 for d in in_shape):
            raise Unsupported(f'{self.where}: input {in_name!r} has a dynamic batch or spatial dimension {in_shape}: export with '
                              'fixed sizes (dynamic=False)')
        if in_shape[0] != 1:
            raise Unsupported(f'{self.where}: input {in_name!r} has batch {in_shape[0]}: export at batch 1 (the engine batches itself)')
        if len(self.m.outputs) != 1:
            raise Unsupported(f'{self.where}: second graph output {self.m.outputs[1][0]!r}: segmentation, pose and OBB heads '
                              'are not supported')
        self.input = in_name
        self.shape[in_name] = tuple(in_shape[1:])
        for i, nd in enumerate(self.nodes):
            if nd.op == 'Constant':
                self.done.add(i)
                continue
            if nd.op == 'Shape' and nd.inputs[0] in self.shape:
                self.const[nd.outputs[0]] = np.array((1,) + self.shape[nd.inputs[0]], np.int64)
                self.done.add(i)
                continue
            if all(self.is_const(t) for t in nd.inputs):
                outs = _np_op(nd, [self.cget(t) for t in nd.inputs], self.m.opset)
                for name, v in zip(nd.outputs, outs):
                    self.const[name] = np.asarray(v)
                self.done.add(i)
                continue
            self.infer(nd)

    def infer(self, nd):
        """Shape of a map-valued node's outputs; nodes behind the head tensors have none (shape[...] stays unset)."""
        x = nd.inputs[0]
        if x not in self.shape and not (nd.op in ('Concat', 'Add', 'Mul') and any(t in self.shape for t in nd.inputs)):
            return
        op, at = nd.op, nd.attrs
        if op == 'Conv':
            w = self.m._tensors.get(nd.inputs[1])
            if w is None:
                _fail(nd, 'weights are not an initialiser')
            c, h, wd = self.shape[x]
            k, s, p = at.get('kernel_shape', w.dims[2:]), at.get('strides', [1, 1]), at.get('pads', [0, 0, 0, 0])
            self.shape[nd.outputs[0]] = (w.dims[0], (h + p[0] + p[2] - k[0]) // s[0] + 1, (wd + p[1] + p[3] - k[1]) // s[1] + 1)
        elif op in ('BatchNormalization', 'Sigmoid', 'Identity', 'MaxPool'):
            if op == 'MaxPool' and (at.get('kernel_shape') != [5, 5] or at.get('strides', [1, 1]) != [1, 1] or
                                    at.get('pads', [0] * 4) != [2, 2, 2, 2] or at.get('ceil_mode', 0) or
                                    any(d != 1 for d in at.get('dilations', [1, 1]))):
                _fail(nd, 'only MaxPool 5x5 stride 1 pads 2 is supported')
            self.shape[nd.outputs[0]] = self.shape[x]
        elif op in ('Mul', 'Add'):
            shapes = [self.shape[t] for t in nd.inputs if t in self.shape]
            if len(shapes) != 2:
                return                      # (no map: emit() names the node unless it lies behind the head tensors)
            if shapes[0] != shapes[1]:
                _fail(nd, 'an elementwise op of two maps of different shapes')
            self.shape[nd.outputs[0]] = shapes[0]
        elif op == 'Concat':
            if not all(t in self.shape for t in nd.inputs):
                return
            if at.get('axis') != 1:
                _fail(nd, 'only a Concat of maps on axis 1 is supported')
            hw = {self.shape[t][1:] for t in nd.inputs}
            if len(hw) != 1:
                _fail(nd, 'Concat of maps of different sizes')
            self.shape[nd.outputs[0]] = (sum(self.shape[t][0] for t in nd.inputs),) + hw.pop()
        elif op == 'Resize':
            scales = self.cget(nd.inputs[2]) if len(nd.inputs) > 2 and nd.inputs[2] and self.is_const(nd.inputs[2]) else None
            c, h, w = self.shape[x]
            if scales is None or len(scales) == 0:
                sizes = self.cget(nd.inputs[3]) if len(nd.inputs) > 3 and self.is_const(nd.inputs[3]) else None
                scales = None if sizes is None else np.asarray(sizes, np.float64) / np.array([1, c, h, w])
            mode, ctm, nm = (at.get(k, d) for k, d in (('mode', b'nearest'), ('coordinate_transformation_mode', b'half_pixel'),
                                                       ('nearest_mode', b'round_prefer_floor')))
            if scales is None or list(scales) != [1, 1, 2, 2] or mode != b'nearest' or ctm != b'asymmetric' or nm != b'floor':
                _fail(nd, 'only Resize nearest x2 (asymmetric, floor) is supported')
            self.shape[nd.outputs[0]] = (c, 2 * h, 2 * w)
        elif op in ('Split', 'Slice'):
            c, h, w = self.shape[x]
            probe = np.arange(c).reshape(1, c, 1, 1)
            if not all(self.is_const(t) for t in nd.inputs[1:]):
                _fail(nd, 'channel ranges that are not constants')
            outs = _np_op(nd, [probe] + [self.cget(t) for t in nd.inputs[1:]], self.m.opset)
            for name, o in zip(nd.outputs, outs):
                ch = o.reshape(-1)
                if o.shape != (1, len(ch), 1, 1) or len(ch) == 0 or list(ch) != list(range(ch[0], ch[0] + len(ch))):
                    _fail(nd, 'only channel ranges (axis 1, step 1) are supported')
                self.shape[name] = (len(ch), h, w)
                self.view_of[name] = (x, int(ch[0]), len(ch))
        # (anything else has no map shape: emit() refuses it by name unless it lies behind the head tensors)

    # ---------------------------------------------------------------- step 2: emit the layers
    def conv_chain(self, i):
        """The Conv at node i with what the table folds into it -> dict(result name, w, b, act, res name, up, nodes)."""
        nd = self.nodes[i]
        at = nd.attrs
        w = self.cget(nd.inputs[1]).astype(np.float32)
        if at.get('group', 1) != 1:
            _fail(nd, f'grouped / depthwise convolution (group {at["group"]}) is not supported')
        if any(d != 1 for d in at.get('dilations', [1, 1])):
            _fail(nd, 'dilated convolution is not supported')
        k, s, p = at.get('kernel_shape', list(w.shape[2:])), at.get('strides', [1, 1]), at.get('pads', [0, 0, 0, 0])
        if k[0] != k[1] or k[0] not in (1, 3) or s[0] != s[1] or s[0] not in (1, 2):
            _fail(nd, f'kernel {k} stride {s}: only k in (1, 3) and stride in (1, 2)')
        if len(set(p)) != 1 or p[0] != k[0] // 2:
            _fail(nd, f'pads {p}: only symmetric pads of k // 2')
        b = self.cget(nd.inputs[2]).astype(np.float32) if len(nd.inputs) > 2 and nd.inputs[2] else np.zeros(w.shape[0], np.float32)
        used, y = [i], nd.outputs[0]
        bn = self.sole(y, 'BatchNormalization')
        if bn is not None:
            gamma, beta, mean, var = (self.cget(t).astype(np.float64) for t in bn.inputs[1:5])
            scale = gamma / np.sqrt(var + bn.attrs.get('epsilon', 1e-5))
            w = (w * scale.reshape(-1, 1, 1, 1)).astype(np.float32)
            b = (beta + (b - mean) * scale).astype(np.float32)
            used.append(self.nodes.index(bn))
            y = bn.outputs[0]
        act = 'linear'
        us = self.users(y)
        sig = [u for u in us if u.op == 'Sigmoid']
        if sig:
            mul = self.sole(sig[0].outputs[0], 'Mul')
            if len(us) != 2 or mul is None or mul not in us or sorted(mul.inputs) != sorted([y, sig[0].outputs[0]]):
                _fail(sig[0], 'a Sigmoid that is not the x * sigmoid(x) of a convolution')
            act = 'swish'
            used += [self.nodes.index(sig[0]), self.nodes.index(mul)]
            y = mul.outputs[0]
        out = dict(node=nd, x=nd.inputs[0], y=y, w=w, b=b, k=k[0], stride=s[0], act=act, res=None, up=1, used=used)
        if act == 'linear':
            return out
        add = self.sole(y, 'Add')
        if add is not None:
            other = [t for t in add.inputs if t != y]
            if len(other) == 1 and other[0] in self.val:
                out.update(res=other[0], y=add.outputs[0])
                used.append(self.nodes.index(add))
                return out
        rs = self.sole(y, 'Resize')
        if rs is not None and k[0] == 1 and s[0] == 1:
            out.update(up=2, y=rs.outputs[0])
            used.append(self.nodes.index(rs))
        return out

    def plan_concats(self):
        """slot[value] = (concat node index, channel offset) for the values their producers write in place."""
        self.slot, self.cat_perm, self.spp = {}, {}, {}
        for i, nd in enumerate(self.nodes):
            if nd.op != 'Concat' or i in self.done or nd.outputs[0] not in self.shape:
                continue
            ins, off, offs = nd.inputs, 0, []
            for t in ins:
                offs.append(off)
                off += self.shape[t][0]
            if any(o % 8 for o in offs):
                _fail(nd, f'slice offsets {offs} are not multiples of 8 channels')
            j = 0
            while j < len(ins):
                t = ins[j]
                if t in self.view_of:
                    # consecutive views that cover their parent, which nothing else reads: the parent is written here whole
                    p, _, _ = self.view_of[t]
                    views = [v for v in ins[j:] if self.view_of.get(v, (None,))[0] == p]
                    run = ins[j:j + len(views)]
                    want, ok = 0, p not in self.slot and p != self.input
                    for v in run:
                        ok = ok and self.view_of.get(v, (None,))[0] == p and self.view_of[v][1] == want
                        want += self.shape[v][0]
                    ok = ok and want == self.shape[p][0] and all(u.op in ('Split', 'Slice', 'Shape') for u in self.users(p))
                    if ok:
                        self.slot[p] = (i, offs[j])
                        j += len(run)
                        continue
                elif t not in self.slot and t != self.input:
                    self.slot[t] = (i, offs[j])
                j += 1
            self.plan_sppf(i, nd, offs)

    def plan_sppf(self, i, nd, offs):
        ins = nd.inputs
        if not (self.sppf_as_spp and len(ins) == 4 and len({self.shape[t] for t in ins}) == 1):
            return
        x, pools = ins[0], ins[1:]
        c, h, w = self.shape[x]
        prod = {n.outputs[0]: n for n in self.nodes if n.op == 'MaxPool'}
        chain = [x] + list(pools)
        for a, b in zip(chain, chain[1:]):
            if b not in prod or prod[b].inputs[0] != a:
                return
        for k, p in enumerate(pools):
            want = {id(nd)} | ({id(prod[pools[k + 1]])} if k < 2 else set())
            if {id(u) for u in self.users(p)} != want or len(self.users(p)) != len(want):
                return
        reader = self.sole(nd.outputs[0], 'Conv')
        if reader is None or c % 8 or h * w > SPP_MAX_HW or any(self.slot.get(t) != (i, o) for t, o in zip(ins, offs)):
            return
        # the op's layout [13 | 9 | 5 | x]: p3, p2, p1, x
        for t, o in zip((pools[2], pools[1], pools[0], x), range(0, 4 * c, c)):
            self.slot[t] = (i, o)
        self.spp[pools[0]] = (i, x)
        for p in pools[1:]:
            self.spp[p] = None
        self.cat_perm[i] = np.concatenate([np.arange(3 * c, 4 * c), np.arange(2 * c, 3 * c), np.arange(c, 2 * c), np.arange(0, c)])

    def cat_tensor(self, i):
        if i not in self.cats:
            c, h, w = self.shape[self.nodes[i].outputs[0]]
            self.cats[i] = self.g.new(h, w, c)
        return self.cats[i]

    def dst_of(self, name):
        if name not in self.slot:
            return None
        i, off = self.slot[name]
        return self.cat_tensor(i).slice(off, self.shape[name][0])

    def emit(self):
        c, h, w = self.shape[self.input]
        self.g = g = Graph(None, (h, w), c)
        g.use_resblock = False
        self.val = {self.input: g.input}
        self.cats, self.heads = {}, {}
        self.plan_concats()
        n_conv = 0
        for i, nd in enumerate(self.nodes):
            if i in self.done:
                continue
            op = nd.op
            if any(t in self.tail for t in nd.inputs):            # behind the head tensors: step 3
                self.tail.update(nd.outputs)
                self.tail_nodes.append(i)
                continue
            if nd.outputs[0] not in self.shape:
                _fail(nd, 'operator not supported here (see fastmot_amd/models/onnx_detector.py for the list)')
            if op == 'Conv':
                ch = self.conv_chain(i)
                x = self.val[ch['x']]
                wgt = ch['w']
                if x.coff == 0 and x.c == self.g.tensors[x.tid][2]:
                    for ci, t in self.cats.items():
                        if t.tid == x.tid and ci in self.cat_perm:
                            # (read back in the tensor's channel order: the op's [13 | 9 | 5 | x])
                            inv = self.cat_perm[ci]
                            wgt = wgt[:, inv]
                if wgt.shape[1] != x.c:
                    _fail(nd, f'weights for {wgt.shape[1]} input channels on a value of {x.c}')
                n_conv += 1
                head = ch['act'] == 'linear'
                if head and not all(u.op == 'Concat' for u in self.users(ch['y'])):
                    _fail(nd, 'a convolution without activation that is not a head output (only x * sigmoid(x) convs are '
                              'supported inside the network)')
                res = self.val[ch['res']] if ch['res'] is not None else None
                y = g.conv(nd.name or f'conv{n_conv}', x, wgt.shape[0], ch['k'], ch['stride'], ch['act'], bn=False,
                           dst=None if head else self.dst_of(ch['y']), res=res, res_mode=RES_AFTER_ACT, f32_out=head,
                           up=ch['up'], wb=(wgt, ch['b']))
                self.done.update(ch['used'])
                self.val[ch['y']] = y
                if head:
                    self.heads[ch['y']] = y
                    self.tail.add(ch['y'])
            elif op in ('Split', 'Slice'):
                for name in nd.outputs:
                    p, off, cn = self.view_of[name]
                    if off % 8:
                        _fail(nd, f'channel view at offset {off}: not a multiple of 8')
                    self.val[name] = self.val[p].slice(off, cn)
            elif op == 'Identity':
                self.val[nd.outputs[0]] = self.val[nd.inputs[0]]
            elif op == 'MaxPool':
                name = nd.outputs[0]
                if name in self.spp:
                    if self.spp[name] is not None:
                        ci, x = self.spp[name]
                        cn = self.shape[x][0]
                        g.spp(self.val[x], self.cat_tensor(ci).slice(0, 3 * cn))
                    self.val[name] = self.dst_of(name)
                else:
                    self.val[name] = g.pool(self.val[nd.inputs[0]], 5, 1, 2, dst=self.dst_of(name))
            elif op == 'Resize':
                self.val[nd.outputs[0]] = g.upsample2(self.val[nd.inputs[0]], dst=self.dst_of(nd.outputs[0]))
            elif op == 'Add':
                a, b = (self.val[t] for t in nd.inputs)
                self.val[nd.outputs[0]] = g.add(a, b, dst=self.dst_of(nd.outputs[0]))
            elif op == 'Concat':
                cat, off = self.cat_tensor(i), 0
                for t in nd.inputs:
                    cn = self.shape[t][0]
                    v = self.val[t]
                    at = self.slot[t][1] if self.slot.get(t, (None,))[0] == i else off      # (SPPF: the op's order)
                    if not (v.tid == cat.tid and v.coff == at):
                        g.copy(v, cat.slice(off, cn))             # (a value that lives elsewhere)
                    off += cn
                self.val[nd.outputs[0]] = cat
            else:
                _fail(nd, 'operator not supported (see fastmot_amd/models/onnx_detector.py for the list)')
            self.done.add(i)

    # ---------------------------------------------------------------- step 3: the head and its embedded decode
    def head_levels(self):
        levels = []
        for i in self.tail_nodes:
            nd = self.nodes[i]
            if nd.op == 'Concat' and any(t in self.heads for t in nd.inputs):
                if len(nd.inputs) != 2 or not all(t in self.heads for t in nd.inputs) or nd.attrs.get('axis') != 1:
                    _fail(nd, 'expected the Concat of a level\'s box and class head tensors')
                levels.append(tuple(nd.inputs))
        paired = {t for lv in levels for t in lv}
        for t in self.heads:
            if t not in paired:
                raise Unsupported(f'{self.where}: head tensor {t!r} is not one of a (box, class) pair')
        out_name = self.m.outputs[0][0]
        if not levels:
            raise Unsupported(f'{self.where}: no head convolutions found in front of output {out_name!r}')
        if len(levels) > MAX_LEVELS:
            raise Unsupported(f'{self.where}: {len(levels)} detection levels, at most {MAX_LEVELS} (FM_MAX_HEADS)')
        _, in_h, in_w = self.shape[self.input]
        strides, nc = [], self.shape[levels[0][1]][0]
        for box, cls in levels:
            cb, gh, gw = self.shape[box]
            if cb != 4 * REG_MAX:
                raise Unsupported(f'{self.where}: box head {box!r} has {cb} channels: reg_max = {cb / 4:g}, only reg_max = '
                                  f'{REG_MAX} is supported')
            if self.shape[cls] != (nc, gh, gw):
                raise Unsupported(f'{self.where}: class head {cls!r} is {self.shape[cls]}, expected {(nc, gh, gw)}')
            if in_h % gh or in_w % gw or in_h // gh != in_w // gw:
                raise Unsupported(f'{self.where}: level {box!r}: grid {gh} x {gw} is no integer stride of the input {in_h} x {in_w}')
            strides.append(in_h // gh)
        if nc > MAX_CLASSES:
            raise Unsupported(f'{self.where}: {nc} classes, at most {MAX_CLASSES}')
        self.verify_tail(levels, strides, nc, out_name)
        return DflHeadsInfo([(self.heads[b], self.heads[c]) for b, c in levels], strides, nc, (in_h, in_w))

    def verify_tail(self, levels, strides, nc, out_name):
        rng = np.random.default_rng(20240229)
        for trial in range(3):
            env, heads = {}, []
            for box, cls in levels:
                _, gh, gw = self.shape[box]
                b = rng.normal(0, 2.5, (1, 4 * REG_MAX, gh, gw))
                c = rng.normal(-1, 2.0, (1, nc, gh, gw))
                if trial == 1:          # ties, and logits of +-30
                    b[:, ::7] = 30.0
                    b[:, 3::11] = -30.0
                    b[:, 16:32] = 1.25
                    c[:, :, ::2] = 30.0
                    c[:, :, 1::3] = -30.0
                if trial == 2:
                    b = np.round(b)
                    c = np.round(c)
                env[box], env[cls] = b, c
                heads.append((b, c))
            for i in self.tail_nodes:
                nd = self.nodes[i]
                for t in nd.inputs:
                    if t not in env and not self.is_const(t):
                        _fail(nd, f'reads {t!r}, which is neither a head tensor nor a constant: only the decode of the head '
                                  'tensors may lie behind them')
                args = [env[t] if t in env else self.cget(t) for t in nd.inputs]
                for name, v in zip(nd.outputs, _np_op(nd, args, self.m.opset)):
                    env[name] = np.asarray(v)
            got = env.get(out_name)
            want = closed_form(heads, strides, self.shape[self.input][1:])
            if got is None or got.shape != want.shape:
                raise Unsupported(f'{self.where}: output {out_name!r} has shape {None if got is None else got.shape}, the decode of '
                                  f'these heads gives {want.shape} (4 + classes, anchors)')
            err = np.abs(got - want) / (1.0 + np.abs(want))
            if not np.isfinite(got).all() or err.max() > 1e-6:
                r, a = np.unravel_index(int(np.nanargmax(np.where(np.isfinite(err), err, np.inf))), err.shape[1:])
                raise Unsupported(
                    f'{self.where}: output {out_name!r} is not the DFL decode this engine implements (softmax expectation over '
                    f'{REG_MAX} bins, anchor offset 0.5, strides {strides}, xywh centres, class sigmoids): row {r}, anchor {a}: '
                    f'file {got[0, r, a]:.6g}, closed form {want[0, r, a]:.6g}')

    def run(self):
        self.fold()
        self.tail, self.tail_nodes = set(), []
        self.emit()
        info = self.head_levels()
        self.done.update(self.tail_nodes)
        left = [nd for i, nd in enumerate(self.nodes) if i not in self.done]
        if left:
            _fail(left[0], 'node was not consumed by the lowering')
        live = {t for i in self.done for t in self.nodes[i].inputs}
        unused = [n for n in self.m.initializer_names() if n not in self.from_const_node and n not in live]
        if unused:
            raise ValueError(f'{self.where}: initialisers nothing reads: {unused[:5]}{" ..." if len(unused) > 5 else ""}')
        self.g.outputs = [v for pair in info.levels for v in pair]
        return self.g, info


def lower(source, input_shape=None, num_classes=None, where=None, sppf_as_spp=True):
    """source: path, bytes or OnnxModel -> (Graph, DflHeadsInfo).  input_shape (c, h, w) / num_classes: a descriptor's
    declared values, checked against the file.  sppf_as_spp=False keeps SPPF as three FM_OP_MAXPOOL layers."""
    model = source if isinstance(source, OnnxModel) else OnnxModel(source)
    where = where or (str(source) if not isinstance(source, (bytes, bytearray, memoryview, OnnxModel)) else 'ONNX model')
    g, info = _Walk(model, where, sppf_as_spp).run()
    h, w, _, _ = g.tensors[g.input.tid]
    if input_shape is not None and tuple(input_shape) != (g.input.c, h, w):
        raise ValueError(f'{where}: input {(g.input.c, h, w)} != declared INPUT_SHAPE {tuple(input_shape)}')
    if num_classes is not None and num_classes != info.num_classes:
        raise ValueError(f'{where}: {info.num_classes} classes != declared NUM_CLASSES {num_classes}')
    return g, info
