"""ONNX files of classification-style ReID backbones -> layer tables of the HIP conv engine ("Add custom ReID" of the
reference's README: train with fast-reid / torchreid, export to ONNX, subclass models.ReID).

`onnx_reader._OSNetWalk` knows ONE topology and names its weights; this lowering knows OPERATORS and follows the node
list (ONNX nodes are topologically sorted) from the data input to the single output.  It covers the ResNet family both
toolkits default to -- BasicBlock and Bottleneck stages, torchreid's `resnet50` / `resnet50_fc512`, fast-reid's
bag-of-tricks R50 with a BN neck -- in both exporter forms: BatchNorm folded into the Conv (weights + bias), or an
explicit BatchNormalization node behind the Conv, folded here with the node's own epsilon.

Backbone operators
    Conv                groups 1, square k in {1, 3, 7}, stride 1 or 2, symmetric pads, dilation 1 (+ BatchNormalization)
    Relu                the activation of the conv (or of the conv + residual sum) in front of it
    Add                 the residual sum: with a Relu behind it, the `res=` / RES_BEFORE_ACT epilogue of the conv that
                        produces one operand; otherwise Graph.add
    MaxPool             3x3 stride 2, pads 1 (torchvision, torchreid) or pads 0 with ceil_mode = 1 (fast-reid); directly behind
                        the 7x7 stride-2 stem with at most 64 channels, stem and pool are ONE launch (FM_OP_STEMPOOL;
                        FASTMOT_STEMPOOL=0, more channels or another stem: the conv and the pool as two layers)
    Identity, Dropout   skipped
Head operators (the suffix of the graph; one FM_OP_POOLHEAD launch, Graph.poolhead)
    GlobalAveragePool | ReduceMean over axes (2, 3) | AveragePool whose kernel is the whole map
    Flatten, Reshape, Squeeze
    BatchNormalization on the pooled vector ([N, C] or [N, C, 1, 1]): the BN neck
    Gemm | MatMul + Add, then optionally BatchNormalization and Relu (`resnet50_fc512`, OSNet-style `fc`)
The tracker L2-normalises whatever comes out (feature_extractor.py of the reference): the head op does.

Anything else raises NotImplementedError naming the node: InstanceNormalization (IBN), Pow (GeM pooling), Sigmoid / Mul
(SE, non-local), grouped or dilated convs, asymmetric pads, a second graph output.  Those models need kernels this
engine does not have; silently approximating them would give embeddings that look plausible and match nothing.
"""
import numpy as np

from .graph import ACT, Graph, OP_CONV, OP_STEMCONV, RES_BEFORE_ACT
from .onnx_reader import OnnxModel

SUPPORTED = ('Conv (groups 1, square k in {1, 3, 7}, stride 1 or 2, symmetric pads, dilation 1), BatchNormalization behind a '
             'Conv, Relu, Add, MaxPool 3x3 stride 2 (pads 1, or pads 0 with ceil_mode 1), Identity, Dropout; as the head: '
             'GlobalAveragePool / ReduceMean over (2, 3) / whole-map AveragePool, Flatten / Reshape / Squeeze, '
             'BatchNormalization on the pooled vector, Gemm or MatMul + Add, BatchNormalization, Relu')


class _Conv:
    """A Conv (+ BatchNormalization) whose epilogue is not known yet: emitted when its Relu / Add / reader arrives."""

    def __init__(self, node, x, w, b, k, stride, pad):
        self.node, self.x, self.w, self.b, self.k, self.stride, self.pad = node, x, w, b, k, stride, pad


class _Sum:
    """conv + other, waiting for the Relu that makes it one launch."""

    def __init__(self, conv, other):
        self.conv, self.other = conv, other


class _Vec:
    """The pooled vector and what the head has applied to it so far."""

    def __init__(self, x):
        self.x, self.c = x, x.c
        self.neck = None            # (scale, shift) fp32
        self.fc = None              # [weight [D, C], bias [D]]
        self.bias_open = False      # a MatMul whose Add has not arrived
        self.bn_done = self.relu = False

    @property
    def width(self):
        return self.fc[0].shape[0] if self.fc is not None else self.c


def _bn_affine(m, node, use):
    g, b, mean, var = (np.asarray(m.tensor(use(t)), np.float64).reshape(-1) for t in node.inputs[1:5])
    scale = g / np.sqrt(var + float(node.attrs.get('epsilon', 1e-5)))
    return scale, b - mean * scale


class _Lowering:
    def __init__(self, model, input_shape, output_dim, where):
        self.m, self.where = model, where
        consts = {nd.outputs[0] for nd in model.nodes if nd.op == 'Constant'}
        self.inits = [n for n in model.initializer_names() if n not in consts]
        self.used = set()
        self.readers = {}
        for nd in model.nodes:
            for t in nd.inputs:
                self.readers[t] = self.readers.get(t, 0) + 1
        if len(model.outputs) != 1:
            raise NotImplementedError(f'{where}: {len(model.outputs)} graph outputs {[n for n, _ in model.outputs]}: a ReID model '
                                      f'has one (the embedding).  Supported: {SUPPORTED}')
        if len(model.data_inputs) != 1 or model.data_inputs[0][1] is None or len(model.data_inputs[0][1]) != 4:
            raise ValueError(f'{where}: expected one NCHW data input, found {model.data_inputs}')
        self.in_name, shape = model.data_inputs[0]
        chw = tuple(shape[1:])
        if not all(isinstance(v, int) and v > 0 for v in chw):
            raise ValueError(f'{where}: input {self.in_name!r} has symbolic or unknown dimensions {shape}')
        if input_shape is not None and chw != tuple(input_shape):
            raise ValueError(f'{where}: the file\'s input is {chw}, INPUT_SHAPE is {tuple(input_shape)}')
        self.input_shape, self.output_dim = chw, output_dim
        self.g = Graph(None, chw[1:], chw[0])
        self.env = {self.in_name: self.g.input}

    # ------------------------------------------------------------------------------------------ helpers
    def refuse(self, nd, what):
        raise NotImplementedError(f'{self.where}: node {nd.name or nd.outputs[0]!r} ({nd.op}): {what}.  Supported: {SUPPORTED}')

    def use(self, name):
        self.used.add(name)
        return name

    def const(self, nd, i):
        if len(nd.inputs) <= i or not self.m.has(nd.inputs[i]):
            self.refuse(nd, f'input {i} is not a constant of the file')
        return np.asarray(self.m.tensor(self.use(nd.inputs[i])))

    def name_of(self, nd):
        return nd.name or nd.outputs[0]

    def emit(self, c, act, res=None):
        return self.g.conv(self.name_of(c.node), c.x, c.w.shape[0], c.k, c.stride, act, pad=c.pad, res=res,
                           res_mode=RES_BEFORE_ACT, wb=(c.w, c.b))

    def view(self, name, nd):
        """The tensor `name` as a stored map (a pending conv is emitted without activation)."""
        v = self.env.get(name)
        if v is None:
            self.refuse(nd, f'input {name!r} is not produced by a supported node')
        if isinstance(v, _Conv):
            v = self.emit(v, 'linear')
        elif isinstance(v, _Sum):
            v = self.g.add(self.emit(v.conv, 'linear'), v.other)
        elif isinstance(v, _Vec):
            self.refuse(nd, 'reads the pooled vector: only head operators may follow the global pool')
        self.env[name] = v
        return v

    def sole(self, name):
        return self.readers.get(name, 0) == 1 and name != self.m.outputs[0][0]

    # ------------------------------------------------------------------------------------------ operators
    def conv(self, nd):
        a = nd.attrs
        w = self.const(nd, 1).astype(np.float32)
        if w.ndim != 4:
            self.refuse(nd, f'weights of shape {w.shape}')
        if a.get('group', 1) != 1:
            self.refuse(nd, f'grouped convolution (group = {a["group"]})')
        if any(d != 1 for d in a.get('dilations', [1, 1])):
            self.refuse(nd, f'dilations {a["dilations"]}')
        if a.get('auto_pad', b'NOTSET') not in (b'NOTSET', 'NOTSET'):
            self.refuse(nd, f'auto_pad {a["auto_pad"]}')
        k = w.shape[2]
        if w.shape[3] != k or k not in (1, 3, 7) or list(a.get('kernel_shape', [k, k])) != [k, k]:
            self.refuse(nd, f'kernel {w.shape[2]} x {w.shape[3]}')
        strides, pads = list(a.get('strides', [1, 1])), list(a.get('pads', [0, 0, 0, 0]))
        if strides[0] != strides[1] or strides[0] not in (1, 2):
            self.refuse(nd, f'strides {strides}')
        if len(set(pads)) != 1 or pads[0] > k // 2:
            self.refuse(nd, f'asymmetric or oversized pads {pads}')
        x = self.view(nd.inputs[0], nd)
        if w.shape[1] != x.c:
            self.refuse(nd, f'weights {w.shape} over a {x.c}-channel input')
        b = self.const(nd, 2).astype(np.float32).reshape(-1) if len(nd.inputs) > 2 and nd.inputs[2] else np.zeros(w.shape[0], np.float32)
        self.env[nd.outputs[0]] = _Conv(nd, x, w, b, k, strides[0], pads[0])

    def batchnorm(self, nd):
        v = self.env.get(nd.inputs[0])
        if isinstance(v, _Conv) and self.sole(nd.inputs[0]):
            scale, shift = _bn_affine(self.m, nd, self.use)
            if scale.shape != (v.w.shape[0],):
                self.refuse(nd, f'{scale.shape[0]} channels behind a conv of {v.w.shape[0]}')
            w = (v.w.astype(np.float64) * scale[:, None, None, None]).astype(np.float32)
            b = (v.b.astype(np.float64) * scale + shift).astype(np.float32)
            self.env[nd.outputs[0]] = _Conv(v.node, v.x, w, b, v.k, v.stride, v.pad)
        elif isinstance(v, _Vec) and not v.relu and not v.bias_open:
            scale, shift = _bn_affine(self.m, nd, self.use)
            if scale.shape != (v.width,):
                self.refuse(nd, f'{scale.shape[0]} channels on a vector of {v.width}')
            if v.fc is None and v.neck is None:
                v.neck = (scale.astype(np.float32), shift.astype(np.float32))
            elif v.fc is not None and not v.bn_done:
                v.fc = [(v.fc[0].astype(np.float64) * scale[:, None]).astype(np.float32),
                        (v.fc[1].astype(np.float64) * scale + shift).astype(np.float32)]
                v.bn_done = True
            else:
                self.refuse(nd, 'a second BatchNormalization at this place of the head')
            self.env[nd.outputs[0]] = v
        else:
            self.refuse(nd, 'BatchNormalization that follows neither a Conv (read by it alone) nor the pooled vector')

    def relu(self, nd):
        v = self.env.get(nd.inputs[0])
        if isinstance(v, _Conv) and self.sole(nd.inputs[0]):
            self.env[nd.outputs[0]] = self.emit(v, 'relu')
        elif isinstance(v, _Sum) and self.sole(nd.inputs[0]):
            self.env[nd.outputs[0]] = self.emit(v.conv, 'relu', res=v.other)
        elif isinstance(v, _Vec) and v.fc is not None and not v.relu and not v.bias_open:
            v.relu = True
            self.env[nd.outputs[0]] = v
        else:
            self.refuse(nd, 'Relu that follows neither a Conv, a Conv + residual Add (read by it alone) nor the head\'s FC')

    def add(self, nd):
        a, b = (self.env.get(t) for t in nd.inputs)
        if isinstance(a, _Vec) or isinstance(b, _Vec):
            v, other = (a, 1) if isinstance(a, _Vec) else (b, 0)
            if not (v.bias_open and self.m.has(nd.inputs[other])):
                self.refuse(nd, 'Add on the pooled vector that is not the bias of a MatMul')
            bias = self.const(nd, other).astype(np.float32).reshape(-1)
            if bias.shape != (v.width,):
                self.refuse(nd, f'bias of {bias.shape[0]} on a vector of {v.width}')
            v.fc[1] = bias
            v.bias_open = False
            self.env[nd.outputs[0]] = v
            return
        for i, (p, q) in enumerate(((a, b), (b, a))):
            if isinstance(p, _Conv) and self.sole(nd.inputs[i]) and p.w.shape[0] % 8 == 0:
                other = self.view(nd.inputs[1 - i], nd)
                ho = (p.x.h + 2 * p.pad - p.k) // p.stride + 1
                wo = (p.x.w + 2 * p.pad - p.k) // p.stride + 1
                if (other.c, other.h, other.w) != (p.w.shape[0], ho, wo):
                    self.refuse(nd, f'operands of different shapes ({(p.w.shape[0], ho, wo)} and {(other.c, other.h, other.w)})')
                self.env[nd.outputs[0]] = _Sum(p, other)
                return
        x, y = self.view(nd.inputs[0], nd), self.view(nd.inputs[1], nd)
        if (x.c, x.h, x.w) != (y.c, y.h, y.w):
            self.refuse(nd, f'operands of different shapes ({(x.c, x.h, x.w)} and {(y.c, y.h, y.w)})')
        self.env[nd.outputs[0]] = self.g.add(x, y)

    def maxpool(self, nd):
        a = nd.attrs
        pads, ceil = list(a.get('pads', [0, 0, 0, 0])), a.get('ceil_mode', 0)
        if (list(a.get('kernel_shape', [])) != [3, 3] or list(a.get('strides', [1, 1])) != [2, 2] or
                any(d != 1 for d in a.get('dilations', [1, 1])) or len(nd.outputs) != 1 or
                not (pads == [1, 1, 1, 1] or (pads == [0, 0, 0, 0] and ceil == 1))):
            self.refuse(nd, f'MaxPool kernel {a.get("kernel_shape")} strides {a.get("strides")} pads {pads} ceil_mode {ceil}')
        x = self.view(nd.inputs[0], nd)
        stem = self.g.layers[-1] if len(self.g.layers) == 1 else None
        if (stem is not None and self.g.use_stempool and stem['op'] in (OP_STEMCONV, OP_CONV) and stem['out'].tid == x.tid and
                stem['ins'][0].tid == self.g.input.tid and (stem['k'], stem['stride'], stem['pad']) == (7, 2, 3) and
                stem['act'] == ACT['relu'] and stem['res'] is None and self.sole(nd.inputs[0]) and x.tid == len(self.g.tensors) - 1 and
                Graph.stempool_supported(stem['cout'], pads[0]) and not (pads[0] == 1 and ceil)):
            # the stem conv and this pool as ONE launch (FM_OP_STEMPOOL): the conv's output tensor never exists
            self.g.layers.pop()
            _, w, b = self.g.conv_params.pop()
            self.g.tensors.pop()
            self.env[nd.outputs[0]] = self.g.stempool(stem['name'], self.g.input, stem['cout'], (w, b), pool_pad=pads[0])
            del self.env[nd.inputs[0]]
            return
        if pads[0] == 1:        # (ceil_mode with pads 1 could start a window in the padding: PyTorch drops it, so does floor)
            if ceil and ((x.h - 1) % 2 or (x.w - 1) % 2):
                self.refuse(nd, 'MaxPool pads 1 with ceil_mode 1 over this map size')
            self.env[nd.outputs[0]] = self.g.pool(x, 3, 2, 1)
        else:
            self.env[nd.outputs[0]] = self.g.pool(x, 3, 2, 0, pad_end=1)

    def global_pool(self, nd):
        x = self.view(nd.inputs[0], nd)
        a = nd.attrs
        if nd.op == 'ReduceMean':
            axes = a.get('axes')
            if axes is None and len(nd.inputs) > 1:
                axes = self.const(nd, 1).reshape(-1).tolist()
            if axes is None or sorted(ax % 4 for ax in axes) != [2, 3]:
                self.refuse(nd, f'ReduceMean over axes {axes}')
        elif nd.op == 'AveragePool':
            if (list(a.get('kernel_shape', [])) != [x.h, x.w] or any(a.get('pads', [0, 0, 0, 0])) or
                    a.get('auto_pad', b'NOTSET') not in (b'NOTSET', 'NOTSET')):
                self.refuse(nd, f'AveragePool kernel {a.get("kernel_shape")} pads {a.get("pads")} over a {x.h} x {x.w} map '
                                '(only the whole map)')
        if x.c % 8 or x.coff % 8 or x.c > Graph.POOLHEAD_MAX:
            self.refuse(nd, f'global pool over {x.c} channels (a multiple of 8, at most {Graph.POOLHEAD_MAX})')
        self.env[nd.outputs[0]] = _Vec(x)

    def reshape(self, nd):
        v = self.env.get(nd.inputs[0])
        if not isinstance(v, _Vec):
            self.refuse(nd, f'{nd.op} in front of the global pool')
        for t in nd.inputs[1:]:          # (the target shape / axes: constants of the file)
            if t and self.m.has(t):
                self.use(t)
            elif t:
                self.refuse(nd, f'computed shape input {t!r}')
        self.env[nd.outputs[0]] = v

    def fc(self, nd):
        v = self.env.get(nd.inputs[0])
        if not isinstance(v, _Vec) or v.fc is not None:
            self.refuse(nd, f'{nd.op} that does not read the pooled vector (or a second FC)')
        w = self.const(nd, 1).astype(np.float32)
        a = nd.attrs
        if nd.op == 'Gemm':
            if a.get('alpha', 1.0) != 1.0 or a.get('beta', 1.0) != 1.0 or a.get('transA', 0):
                self.refuse(nd, f'Gemm alpha {a.get("alpha")} beta {a.get("beta")} transA {a.get("transA")}')
            if not a.get('transB', 0):
                w = w.T
        else:
            w = w.T                      # MatMul: stored [in, out]
        if w.ndim != 2 or w.shape[1] != v.c:
            self.refuse(nd, f'weights {w.shape} on a vector of {v.c}')
        bias = np.zeros(w.shape[0], np.float32)
        if nd.op == 'Gemm' and len(nd.inputs) > 2 and nd.inputs[2]:
            bias = self.const(nd, 2).astype(np.float32).reshape(-1)
            if bias.shape != (w.shape[0],):
                self.refuse(nd, f'bias {bias.shape}')
        v.fc = [np.ascontiguousarray(w), bias]
        # (a MatMul may be followed by the Add of its bias -- or by nothing: bias=False)
        v.bias_open = nd.op == 'MatMul'
        self.env[nd.outputs[0]] = v

    def skip(self, nd):
        if nd.inputs[0] not in self.env:
            self.refuse(nd, f'input {nd.inputs[0]!r} is not produced by a supported node')
        for t in nd.inputs[1:]:
            if t and self.m.has(t):
                self.use(t)
        self.env[nd.outputs[0]] = self.env[nd.inputs[0]]
        self.readers[nd.outputs[0]] = self.readers.get(nd.outputs[0], 0) + self.readers.get(nd.inputs[0], 1) - 1

    HANDLERS = {'Conv': conv, 'BatchNormalization': batchnorm, 'Relu': relu, 'Add': add, 'MaxPool': maxpool,
                'GlobalAveragePool': global_pool, 'ReduceMean': global_pool, 'AveragePool': global_pool,
                'Flatten': reshape, 'Reshape': reshape, 'Squeeze': reshape, 'Gemm': fc, 'MatMul': fc,
                'Identity': skip, 'Dropout': skip}

    def run(self):
        for nd in self.m.nodes:
            if nd.op == 'Constant':
                continue
            h = self.HANDLERS.get(nd.op)
            if h is None:
                self.refuse(nd, 'operator not supported')
            h(self, nd)
        out_name = self.m.outputs[0][0]
        v = self.env.get(out_name)
        if not isinstance(v, _Vec):
            raise NotImplementedError(f'{self.where}: the output {out_name!r} is not a pooled embedding vector (a global pool '
                                      f'and the head operators must end the graph).  Supported: {SUPPORTED}')
        v.bias_open = False
        if self.output_dim is not None and v.width != self.output_dim:
            raise ValueError(f'{self.where}: the file\'s embedding has {v.width} components, OUTPUT_LAYOUT is {self.output_dim}')
        unused = [n for n in self.inits if n not in self.used]
        if unused:
            raise ValueError(f'{self.where}: parameters not used by the lowering: {unused[:5]} ...')
        out = self.g.poolhead('head', v.x, neck=v.neck, fc=tuple(v.fc) if v.fc is not None else None, relu=v.relu)
        self.g.outputs = [v.x]
        return self.g, out


def lower(source, input_shape=None, output_dim=None, where=None):
    """-> (Graph, output view).  source: an OnnxModel, a path or the bytes of a file.  input_shape (c, h, w) / output_dim:
    the descriptor's INPUT_SHAPE / OUTPUT_LAYOUT, checked against the file (ValueError); None: taken from the file."""
    model = source if isinstance(source, OnnxModel) else OnnxModel(source)
    where = where or (str(source) if not isinstance(source, (OnnxModel, bytes, bytearray, memoryview)) else 'ONNX model')
    return _Lowering(model, input_shape, output_dim, where).run()
