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
IBN-Net layers (one FM_OP_INSTNORM launch each, Graph.instnorm, csrc/instnorm.hip)
    IBN-a               Conv (read by the Split alone) -> Split(axis 1, [h, c - h]; opset 13: `split` as a constant input) ->
                        InstanceNormalization on part 0, BatchNormalization on part 1 -> Concat(axis 1) in that order -> Relu:
                        the BatchNorm is folded into rows [h:] of the conv, which is emitted without activation, then
                        instnorm(cn = h, relu) normalises the first h channels and applies the ReLU to all of them.  h % 8 == 0
    IBN-b, IN stem      InstanceNormalization that reads a pending Conv, or a pending Conv + Add sum, alone: the conv (with
                        `res=` for the sum) without activation, then instnorm(cn = c); a Relu behind it becomes the op's
                        activation.  A 7x7 stem followed by InstanceNormalization is conv + instnorm + pool: the normalisation
                        needs the whole conv map before the pool may start, so FM_OP_STEMPOOL is not used there
fast-reid's non-local blocks (AGW, SBS: `Non_local` with WITH_NL; one FM_OP_NONLOCAL launch each, Graph.nonlocal_, csrc/nonlocal.hip)
    three Conv (1x1, ONE output channel, with bias) that read the same stored map X -> Reshape [B, 1, -1 | N] each ->
    Transpose(0, 2, 1) on two of them -> MatMul(theta^T, phi) -> Div by N = H * W (or Mul by 1 / N) -> MatMul(., g^T) ->
    Transpose(0, 2, 1) -> Reshape [B, 1, H, W] -> Conv 1 -> C (+ BatchNormalization, folded here) -> Add(., X).  Roles come
    from the wiring: theta is the left operand of the first MatMul, phi its right one (no Transpose), g the right operand of
    the second.  With one inner channel the N x N matrix never exists on the device: s = mean(phi g) per sample, z = X +
    a theta s + b.  The shape operands are constants, or the exporter's unfolded Concat(axis 0) of Unsqueeze(axes [0]) of
    scalar constants: that small integer subgraph is folded here whatever its nodes are called
Head operators (the suffix of the graph; one FM_OP_POOLHEAD launch, Graph.poolhead)
    GlobalAveragePool | ReduceMean over axes (2, 3) | AveragePool whose kernel is the whole map
    GeM pooling: Clip(min = a positive scalar constant, no max) -> Pow(scalar constant or initialiser p, 0.5 .. 16) -> one of
                        the pools above -> Pow(q) on the pooled vector with |q p - 1| <= 1e-4.  A learned p arrives with its
                        root as Reciprocal / Mul / Cast of scalars: those few scalar nodes are folded here
    Flatten, Reshape, Squeeze
    BatchNormalization on the pooled vector ([N, C] or [N, C, 1, 1]): the BN neck
    Gemm | MatMul + Add, then optionally BatchNormalization and Relu (`resnet50_fc512`, OSNet-style `fc`)
The tracker L2-normalises whatever comes out (feature_extractor.py of the reference): the head op does.

Anything else raises NotImplementedError naming the node: an InstanceNormalization of a map that is already stored and
activated (OSNet-IBN / OSNet-AIN keep theirs inside the fused OSNet operators), a Split whose IN part is no multiple of 8 or
does not lead, a Pow without its Clip, with a per-channel exponent or without the matching root, Sigmoid / Mul (SE), a
non-local block with more than one inner channel, a Softmax (the embedded-Gaussian form), a divisor other than H * W or a
sum with anything but its own input, grouped or dilated convs, asymmetric pads, a second graph output.  Those models need
kernels this engine does not have; silently approximating them would give embeddings that look plausible and match nothing.
"""
import numpy as np

from .graph import ACT, Graph, OP_CONV, OP_STEMCONV, RES_BEFORE_ACT
from .onnx_reader import OnnxModel

SUPPORTED = ('Conv (groups 1, square k in {1, 3, 7}, stride 1 or 2, symmetric pads, dilation 1), BatchNormalization behind a '
             'Conv, Relu, Add, MaxPool 3x3 stride 2 (pads 1, or pads 0 with ceil_mode 1), Identity, Dropout; IBN-a: Conv -> '
             'Split(axis 1, [h, c - h], h % 8 == 0) -> InstanceNormalization on part 0 + BatchNormalization on part 1 -> Concat '
             '-> Relu; IBN-b: InstanceNormalization (+ Relu) behind a Conv or a Conv + Add read by it alone; as the head: '
             'GlobalAveragePool / ReduceMean over (2, 3) / whole-map AveragePool, optionally as GeM (Clip(min > 0) -> Pow(scalar '
             'p) -> pool -> Pow(1 / p)), Flatten / Reshape / Squeeze, BatchNormalization on the pooled vector, Gemm or '
             'MatMul + Add, BatchNormalization, Relu; fast-reid non-local block: three Conv 1x1 -> 1 channel of one stored map X -> '
             'Reshape [B, 1, N] (+ Transpose(0, 2, 1) on theta and g) -> MatMul(theta, phi) -> Div by H * W (or Mul by its '
             'reciprocal) -> MatMul(., g) -> Transpose -> Reshape [B, 1, H, W] -> Conv 1x1 1 -> C (+ BatchNormalization) -> '
             'Add(., X), with 8 <= C <= 2048, C % 8 == 0, H * W <= 4096; shape operands as constants or Concat / Unsqueeze '
             'of integer constants')


class _Conv:
    """A Conv (+ BatchNormalization) whose epilogue is not known yet: emitted when its Relu / Add / reader arrives."""

    def __init__(self, node, x, w, b, k, stride, pad):
        self.node, self.x, self.w, self.b, self.k, self.stride, self.pad = node, x, w, b, k, stride, pad


class _Sum:
    """conv + other, waiting for the Relu that makes it one launch."""

    def __init__(self, conv, other):
        self.conv, self.other = conv, other


class _Normed:
    """conv (+ other) -> instance normalisation of the first cn channels, waiting for its Relu."""

    def __init__(self, conv, other, gamma, beta, eps, node):
        self.conv, self.other, self.gamma, self.beta, self.eps, self.node = conv, other, gamma, beta, eps, node


class _Only:
    """A value only certain nodes may read: a part of an IBN Split, the clamped / powered map of GeM, a folded scalar."""
    what = ''


class _Split:
    def __init__(self, conv, parts, node):
        self.conv, self.parts, self.node = conv, parts, node
        self.inorm = self.bn = None          # (gamma, beta, eps, output name) / (scale, shift, output name)


class _Part(_Only):
    what = 'a part of a Split: only the InstanceNormalization (part 0) and BatchNormalization (part 1) of an IBN layer may'

    def __init__(self, split, index, done=False):
        self.split, self.index, self.done = split, index, done


class _Gem(_Only):
    what = 'the clamped / powered map of GeM pooling: only its Pow and its global pool may'

    def __init__(self, x, eps, p=None):
        self.x, self.eps, self.p = x, eps, p


class _Scalar(_Only):
    what = 'a folded scalar: only the exponent of a GeM root may'

    def __init__(self, value):
        self.value = value


class _Ints(_Only):
    what = 'a folded integer constant: only a shape operand may'

    def __init__(self, values):
        self.values = values


class _NLVec(_Only):
    """theta, phi or g of a non-local block as [B, 1, N] (t: transposed to [B, N, 1]); conv: the pending 1x1 Conv behind it."""
    what = 'an intermediate value of a non-local block: only the nodes of that block may'

    def __init__(self, conv, t=False):
        self.conv, self.t = conv, t


class _NLF(_NLVec):
    """matmul(theta, phi), [B, N, N]; div: already divided by N."""

    def __init__(self, theta, phi, div=False):
        self.theta, self.phi, self.div = theta, phi, div


class _NLY(_NLVec):
    """matmul(f / N, g): stage 0 as [B, N, 1], 1 transposed, 2 reshaped to the map [B, 1, H, W]; then W (a, b: float64)."""

    def __init__(self, f, g, stage=0, a=None, b=None, bn=False):
        self.f, self.g, self.stage, self.a, self.b, self.bn = f, g, stage, a, b, bn


class _Vec:
    """The pooled vector and what the head has applied to it so far."""

    def __init__(self, x, gem=None, gem_node=None):
        self.x, self.c = x, x.c
        self.gem, self.gem_node = gem, gem_node    # (p, eps); the root is still missing while gem_node is set
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
        elif isinstance(v, _Normed):
            v = self.emit_normed(v, 'linear')
        elif isinstance(v, _Only):
            self.refuse(nd, f'reads {v.what}')
        elif isinstance(v, _Vec):
            self.refuse(nd, 'reads the pooled vector: only head operators may follow the global pool')
        self.env[name] = v
        return v

    def sole(self, name):
        return self.readers.get(name, 0) == 1 and name != self.m.outputs[0][0]

    def emit_normed(self, n, act):
        y = self.emit(n.conv, 'linear', res=n.other)
        return self.g.instnorm(self.name_of(n.node), y, n.gamma, n.beta, n.eps, act)

    def scalar(self, name):
        """The value of a one-element constant, initialiser or folded scalar; None for anything else."""
        v = self.env.get(name)
        if isinstance(v, _Scalar):
            return v.value
        if name and self.m.has(name):
            a = np.asarray(self.m.tensor(name))
            if a.size == 1:
                self.use(name)
                return float(a.reshape(-1)[0])
        return None

    def ints(self, name):
        """The integers of a constant of the file or of a folded Unsqueeze / Concat of such; None for anything else."""
        v = self.env.get(name)
        if isinstance(v, _Ints):
            return v.values
        if name and self.m.has(name):
            a = np.asarray(self.m.tensor(name))
            if a.dtype.kind in 'iu' and a.size <= 8:
                self.use(name)
                return [int(q) for q in a.reshape(-1)]
        return None

    def only(self, nd, i):
        if not self.sole(nd.inputs[i]):
            self.refuse(nd, f'input {nd.inputs[i]!r} is a value of a non-local block that something else reads as well')

    def open_root(self, v, nd):
        if v.gem_node is not None:
            self.refuse(nd, f'follows GeM pooling ({self.name_of(v.gem_node)!r}) whose root Pow(1 / p) has not been applied')

    # ------------------------------------------------------------------------------------------ operators
    def conv(self, nd):
        a = nd.attrs
        if isinstance(self.env.get(nd.inputs[0]), _NLY):
            return self.nl_w(nd)
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
        elif isinstance(v, _NLY) and v.a is not None and not v.bn:
            self.only(nd, 0)
            scale, shift = _bn_affine(self.m, nd, self.use)
            if scale.shape != v.a.shape:
                self.refuse(nd, f'{scale.shape[0]} channels behind the W conv of a non-local block over {v.a.shape[0]}')
            self.env[nd.outputs[0]] = _NLY(v.f, v.g, 2, v.a * scale, v.b * scale + shift, bn=True)
        elif isinstance(v, _Part) and not v.done:
            sp = v.split
            if v.index != 1 or not self.sole(nd.inputs[0]):
                self.refuse(nd, 'BatchNormalization on the leading part of a Split: the InstanceNormalization half of an IBN '
                                'layer must lead (IBN-a), the BatchNormalization half trail')
            scale, shift = _bn_affine(self.m, nd, self.use)
            if scale.shape != (sp.parts[1],):
                self.refuse(nd, f'{scale.shape[0]} channels on a part of {sp.parts[1]}')
            sp.bn = (scale, shift)
            self.env[nd.outputs[0]] = _Part(sp, 1, done=True)
        elif isinstance(v, _Vec) and not v.relu and not v.bias_open:
            self.open_root(v, nd)
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
        elif isinstance(v, _Normed) and self.sole(nd.inputs[0]):
            self.env[nd.outputs[0]] = self.emit_normed(v, 'relu')
        elif isinstance(v, _Vec) and v.fc is not None and not v.relu and not v.bias_open:
            v.relu = True
            self.env[nd.outputs[0]] = v
        else:
            self.refuse(nd, 'Relu that follows neither a Conv, a Conv + residual Add, an IBN layer (read by it alone) nor the head\'s FC')

    def add(self, nd):
        a, b = (self.env.get(t) for t in nd.inputs)
        if isinstance(a, _NLVec) or isinstance(b, _NLVec):
            return self.nl_sum(nd, 0 if isinstance(a, _NLVec) else 1)
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

    # ---- IBN-Net
    def split(self, nd):
        v = self.env.get(nd.inputs[0])
        if not (isinstance(v, _Conv) and self.sole(nd.inputs[0])):
            self.refuse(nd, 'Split that does not read a Conv alone (the Split of an IBN-a layer does)')
        parts = nd.attrs.get('split')
        if parts is None and len(nd.inputs) > 1:
            parts = self.const(nd, 1).reshape(-1).tolist()
        c = v.w.shape[0]
        if nd.attrs.get('axis', 0) != 1 or parts is None or len(parts) != 2 or len(nd.outputs) != 2 or sum(parts) != c or min(parts) < 1:
            self.refuse(nd, f'Split axis {nd.attrs.get("axis", 0)} into {parts}: two parts along the channels that tile the '
                            f'{c} channels of the conv')
        if parts[0] % 8:
            self.refuse(nd, f'IBN layer whose InstanceNormalization part has {parts[0]} channels: a multiple of 8')
        sp = _Split(v, [int(q) for q in parts], nd)
        for i, name in enumerate(nd.outputs):
            self.env[name] = _Part(sp, i)

    def instnorm(self, nd):
        v = self.env.get(nd.inputs[0])
        eps = float(nd.attrs.get('epsilon', 1e-5))
        if isinstance(v, _Part) and not v.done:
            sp = v.split
            if v.index != 0:
                self.refuse(nd, 'InstanceNormalization on the trailing part of a Split: the IN half of an IBN layer must lead '
                                '(channels [0, h)), as in IBN-a')
            if not self.sole(nd.inputs[0]):
                self.refuse(nd, 'a part of a Split that something else reads as well')
            gamma, beta = (self.const(nd, i).astype(np.float32).reshape(-1) for i in (1, 2))
            if gamma.shape != (sp.parts[0],) or beta.shape != gamma.shape:
                self.refuse(nd, f'{gamma.shape[0]} channels on a part of {sp.parts[0]}')
            sp.inorm = (gamma, beta, eps, nd)
            self.env[nd.outputs[0]] = _Part(sp, 0, done=True)
            return
        if isinstance(v, (_Conv, _Sum)) and self.sole(nd.inputs[0]):
            conv, other = (v, None) if isinstance(v, _Conv) else (v.conv, v.other)
            c = conv.w.shape[0]
            gamma, beta = (self.const(nd, i).astype(np.float32).reshape(-1) for i in (1, 2))
            if c % 8 or gamma.shape != (c,) or beta.shape != (c,):
                self.refuse(nd, f'{gamma.shape[0]} channels behind a conv of {c} (a multiple of 8)')
            self.env[nd.outputs[0]] = _Normed(conv, other, gamma, beta, eps, nd)
            return
        self.refuse(nd, 'InstanceNormalization that reads neither part 0 of an IBN Split nor a Conv or Conv + Add alone (a map '
                        'that is already stored and activated would need a normalisation this lowering does not place)')

    def concat(self, nd):
        vs = [self.env.get(t) for t in nd.inputs]
        if not (len(vs) == 2 and all(isinstance(v, _Part) and v.done for v in vs) and vs[0].split is vs[1].split and
                nd.attrs.get('axis') == 1 and all(self.sole(t) for t in nd.inputs)):
            self.refuse(nd, 'Concat that does not join the two halves of one IBN layer along the channels')
        if (vs[0].index, vs[1].index) != (0, 1):
            self.refuse(nd, 'Concat of an IBN layer with its parts out of order')
        sp = vs[0].split
        scale, shift = sp.bn
        gamma, beta, eps, node = sp.inorm
        h, c = sp.parts[0], sp.conv
        w, b = c.w.astype(np.float64), c.b.astype(np.float64)
        w[h:] *= scale[:, None, None, None]
        b[h:] = b[h:] * scale + shift
        self.env[nd.outputs[0]] = _Normed(_Conv(c.node, c.x, w.astype(np.float32), b.astype(np.float32), c.k, c.stride, c.pad),
                                          None, gamma, beta, eps, node)

    # ---- GeM
    def clip(self, nd):
        lo = self.scalar(nd.inputs[1]) if len(nd.inputs) > 1 and nd.inputs[1] else nd.attrs.get('min')
        has_max = (len(nd.inputs) > 2 and nd.inputs[2]) or 'max' in nd.attrs
        if lo is None or has_max or not 0 < lo <= 1:
            self.refuse(nd, 'Clip that is not the clamp of GeM pooling (min = a scalar constant in (0, 1], no max)')
        x = self.view(nd.inputs[0], nd)
        if not self.sole(nd.outputs[0]):
            self.refuse(nd, 'the clamp of GeM pooling read by more than its Pow')
        self.env[nd.outputs[0]] = _Gem(x, float(lo))

    def pow(self, nd):
        v = self.env.get(nd.inputs[0])
        e = self.scalar(nd.inputs[1]) if len(nd.inputs) > 1 else None
        if isinstance(v, _Gem) and v.p is None:
            if e is None or not 0.5 <= e <= 16:
                self.refuse(nd, 'GeM pooling whose exponent is not one scalar constant in [0.5, 16] (a per-channel p is not supported)')
            if not self.sole(nd.outputs[0]):
                self.refuse(nd, 'the powered map of GeM pooling read by more than its global pool')
            self.env[nd.outputs[0]] = _Gem(v.x, v.eps, float(e))
        elif isinstance(v, _Vec) and v.gem_node is not None and v.neck is None and v.fc is None:
            if e is None or abs(e * v.gem[0] - 1) > 1e-4:
                self.refuse(nd, f'the root of GeM pooling with exponent {e}: it does not match 1 / p of {self.name_of(v.gem_node)!r} '
                                f'(p = {v.gem[0]:g})')
            v.gem_node = None
            self.env[nd.outputs[0]] = v
        else:
            self.refuse(nd, 'Pow that is neither the power of GeM pooling (behind its Clip, scalar exponent) nor its root')

    def fold_scalar(self, nd):
        for i, t in enumerate(nd.inputs[:2]):
            if nd.op == 'Mul' and len(nd.inputs) == 2 and isinstance(self.env.get(t), _NLF):
                return self.nl_div(nd, i)
        vals = [self.scalar(t) for t in nd.inputs]
        if not vals or any(v is None for v in vals):
            self.refuse(nd, 'operator not supported')
        if nd.op == 'Cast':
            if nd.attrs.get('to') not in (1, 11):
                self.refuse(nd, f'Cast of a scalar to type {nd.attrs.get("to")}')
            out = vals[0]
        elif nd.op == 'Reciprocal':
            out = 1.0 / vals[0]
        else:
            out = vals[0] * vals[1]
        self.env[nd.outputs[0]] = _Scalar(float(out))

    def global_pool(self, nd):
        v = self.env.get(nd.inputs[0])
        gem = None
        if isinstance(v, _Gem):
            if v.p is None:
                self.refuse(nd, 'global pool of a clamped map without the Pow of GeM pooling')
            x, gem = v.x, (v.p, v.eps)
        else:
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
        self.env[nd.outputs[0]] = _Vec(x, gem, nd if gem is not None else None)

    def reshape(self, nd):
        v = self.env.get(nd.inputs[0])
        if nd.op == 'Reshape' and len(nd.inputs) > 1 and isinstance(v, (_NLY, _Conv)):
            shape = self.ints(nd.inputs[1])
            # (a pending conv flattened to [B, k, N]: theta, phi or g of a non-local block; its product back to a map)
            if isinstance(v, _NLY) or (shape is not None and len(shape) == 3):
                return self.nl_reshape(nd, v)
        if not isinstance(v, _Vec):
            self.refuse(nd, f'{nd.op} in front of the global pool')
        for t in nd.inputs[1:]:          # (the target shape / axes: constants of the file)
            if t and self.m.has(t):
                self.use(t)
            elif t:
                self.refuse(nd, f'computed shape input {t!r}')
        self.env[nd.outputs[0]] = v

    def fc(self, nd):
        if nd.op == 'MatMul' and any(isinstance(self.env.get(t), _NLVec) for t in nd.inputs):
            return self.nl_matmul(nd)
        v = self.env.get(nd.inputs[0])
        if not isinstance(v, _Vec) or v.fc is not None:
            self.refuse(nd, f'{nd.op} that does not read the pooled vector (or a second FC)')
        self.open_root(v, nd)
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

    # ---- fast-reid's non-local block
    def fold_ints(self, nd):
        """Unsqueeze(axes [0]) of an integer constant, Concat(axis 0) of such: the exporter's unfolded shape operands."""
        if nd.op == 'Concat':
            vals, axes = [self.ints(t) for t in nd.inputs], [nd.attrs.get('axis')]
            if not vals or any(v is None for v in vals):
                return self.concat(nd)                # (the Concat of an IBN layer, or one that is refused there)
        else:
            vals, axes = [self.ints(nd.inputs[0])], nd.attrs.get('axes')
            if axes is None and len(nd.inputs) > 1:   # (opset 13: the axes as an input)
                axes = self.ints(nd.inputs[1])
            if vals[0] is None or len(vals[0]) != 1:
                self.refuse(nd, 'operator not supported')
        if list(axes or []) != [0]:
            self.refuse(nd, f'{nd.op} of integer constants along axes {axes}')
        self.env[nd.outputs[0]] = _Ints([q for v in vals for q in v])

    def nl_reshape(self, nd, v):
        shape = self.ints(nd.inputs[1])
        if shape is None:
            self.refuse(nd, f'computed shape input {nd.inputs[1]!r}')
        self.only(nd, 0)
        if isinstance(v, _Conv):                      # theta, phi or g: [B, inter, H, W] -> [B, inter, N]
            k, x = v.w.shape[0], v.x
            if shape[1] != k or (v.k, v.stride, v.pad) != (1, 1, 0):
                self.refuse(nd, f'{nd.op} in front of the global pool')
            if k != 1:
                self.refuse(nd, f'non-local block with inter channels {k}: only the one-channel form fast-reid\'s Non_local builds')
            if shape[2] not in (-1, x.h * x.w):
                self.refuse(nd, f'shape {shape} of a non-local block over a {x.h} x {x.w} map')
            self.env[nd.outputs[0]] = _NLVec(v)
            return
        x = v.g.x
        if v.stage != 1 or v.a is not None or len(shape) != 4 or shape[1:] != [1, x.h, x.w]:
            self.refuse(nd, f'shape {shape} behind the products of a non-local block over a {x.h} x {x.w} map ([B, 1, H, W] behind '
                            'the Transpose)')
        self.env[nd.outputs[0]] = _NLY(v.f, v.g, 2)

    def transpose(self, nd):
        v = self.env.get(nd.inputs[0])
        ok = type(v) is _NLVec and not v.t or (isinstance(v, _NLY) and v.stage == 0)
        if not ok or list(nd.attrs.get('perm', [])) != [0, 2, 1]:
            self.refuse(nd, 'Transpose that is not the (0, 2, 1) of a non-local block\'s theta, g or product')
        self.only(nd, 0)
        self.env[nd.outputs[0]] = _NLVec(v.conv, t=True) if type(v) is _NLVec else _NLY(v.f, v.g, 1)

    def nl_matmul(self, nd):
        a, b = (self.env.get(t) for t in nd.inputs[:2])
        self.only(nd, 0)
        self.only(nd, 1)
        if type(a) is _NLVec and a.t and type(b) is _NLVec and not b.t and a.conv.x is b.conv.x:
            self.env[nd.outputs[0]] = _NLF(a.conv, b.conv)            # theta: the left operand; phi: the right one, no transpose
        elif isinstance(a, _NLF) and type(b) is _NLVec and b.t and b.conv.x is a.theta.x:
            if not a.div:
                self.refuse(nd, 'the second product of a non-local block without the division by N = H * W in front of it')
            self.env[nd.outputs[0]] = _NLY(a, b.conv)
        else:
            self.refuse(nd, 'MatMul of non-local block values that is neither matmul(theta^T, phi) nor matmul(f / N, g^T) over '
                            'one input map')

    def nl_div(self, nd, i=0):
        v = self.env.get(nd.inputs[i])
        if not (isinstance(v, _NLF) and len(nd.inputs) == 2 and (i == 0 or nd.op == 'Mul')):
            self.refuse(nd, 'operator not supported')
        c, n = self.scalar(nd.inputs[1 - i]), v.theta.x.h * v.theta.x.w
        if v.div or c is None:
            self.refuse(nd, f'{nd.op} of the product of a non-local block that is not its one division by a constant')
        if (nd.op == 'Div' and c != n) or (nd.op == 'Mul' and abs(c * n - 1) > 1e-6):
            self.refuse(nd, f'the divisor {c if nd.op == "Div" else 1 / c if c else c:g} of a non-local block does not match N = H * W = '
                            f'{n} of its map (f / C, the source\'s variable name, is not what it computes)')
        self.only(nd, i)
        self.env[nd.outputs[0]] = _NLF(v.theta, v.phi, div=True)

    def softmax(self, nd):
        if isinstance(self.env.get(nd.inputs[0]), _NLF):
            self.refuse(nd, 'Softmax between the products of a non-local block (the embedded-Gaussian variant): only the '
                            'dot-product form, f / N, is supported')
        self.refuse(nd, 'operator not supported')

    def nl_w(self, nd):
        v, a = self.env[nd.inputs[0]], nd.attrs
        x = v.g.x
        w = self.const(nd, 1).astype(np.float64)
        if (v.stage != 2 or v.a is not None or w.shape != (x.c, 1, 1, 1) or a.get('group', 1) != 1 or
                any(q != 1 for q in a.get('strides', [1, 1])) or any(a.get('pads', [0, 0, 0, 0])) or any(q != 1 for q in a.get('dilations', [1, 1]))):
            self.refuse(nd, f'weights {w.shape} behind the products of a non-local block over {x.c} channels (W: a 1x1 conv 1 -> C '
                            'behind the Reshape to [B, 1, H, W])')
        self.only(nd, 0)
        b = self.const(nd, 2).astype(np.float64).reshape(-1) if len(nd.inputs) > 2 and nd.inputs[2] else np.zeros(x.c)
        self.env[nd.outputs[0]] = _NLY(v.f, v.g, 2, w.reshape(-1), b)

    def nl_sum(self, nd, i):
        v, other = self.env[nd.inputs[i]], self.env.get(nd.inputs[1 - i])
        if not (isinstance(v, _NLY) and v.a is not None):
            self.refuse(nd, f'reads {v.what}')
        x = v.g.x
        if other is not x:
            self.refuse(nd, f'Add of a non-local block whose other operand {nd.inputs[1 - i]!r} is not the block\'s own input (z = '
                            'W(y) + x)')
        self.only(nd, i)
        if x.coff % 8 or not Graph.nonlocal_supported(x.c, x.h * x.w):
            self.refuse(nd, f'non-local block over {x.c} channels on a {x.h} x {x.w} map: FM_OP_NONLOCAL runs 8 <= C <= 2048 with '
                            'C % 8 == 0 on at most 4096 pixels')
        theta, phi, g = v.f.theta, v.f.phi, v.g
        self.env[nd.outputs[0]] = self.g.nonlocal_(self.name_of(nd), x, theta.w, phi.w, g.w, [theta.b[0], phi.b[0], g.b[0]], v.a, v.b)

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
                'Identity': skip, 'Dropout': skip, 'Split': split, 'InstanceNormalization': instnorm, 'Concat': fold_ints,
                'Unsqueeze': fold_ints, 'Transpose': transpose, 'Div': nl_div, 'Softmax': softmax,
                'Clip': clip, 'Pow': pow, 'Cast': fold_scalar, 'Reciprocal': fold_scalar, 'Mul': fold_scalar}

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
        if v.gem_node is not None:
            self.refuse(v.gem_node, 'GeM pooling without its root: the pooled vector must go through Pow(1 / p)')
        if self.output_dim is not None and v.width != self.output_dim:
            raise ValueError(f'{self.where}: the file\'s embedding has {v.width} components, OUTPUT_LAYOUT is {self.output_dim}')
        unused = [n for n in self.inits if n not in self.used]
        if unused:
            raise ValueError(f'{self.where}: parameters not used by the lowering: {unused[:5]} ...')
        out = self.g.poolhead('head', v.x, neck=v.neck, fc=tuple(v.fc) if v.fc is not None else None, relu=v.relu, gem=v.gem)
        self.g.outputs = [v.x]
        return self.g, out


def lower(source, input_shape=None, output_dim=None, where=None):
    """-> (Graph, output view).  source: an OnnxModel, a path or the bytes of a file.  input_shape (c, h, w) / output_dim:
    the descriptor's INPUT_SHAPE / OUTPUT_LAYOUT, checked against the file (ValueError); None: taken from the file."""
    model = source if isinstance(source, OnnxModel) else OnnxModel(source)
    where = where or (str(source) if not isinstance(source, (OnnxModel, bytes, bytearray, memoryview)) else 'ONNX model')
    return _Lowering(model, input_shape, output_dim, where).run()
