"""torchreid OSNet checkpoint -> parameter source of the OSNet layer table (models/reid.py).

The reference converts the torchreid model to ONNX offline and builds a TensorRT engine from it
(fastmot/models/reid.py:48-92, README model zoo: osnet_x0_25_msmt17 / osnet_x1_0_msdc); here the
checkpoint's state_dict is read directly.  The mapping below follows torchreid/models/osnet.py:

    conv1                      ConvLayer        conv1.conv / conv1.bn
    conv{2,3,4}.{0,1}          OSBlock          .conv1 (Conv1x1: conv, bn)
                                                .conv2a | .conv2b.{0,1} | .conv2c.{0,1,2} | .conv2d.{0..3}
                                                    LightConv3x3: conv1 (1x1), conv2 (depthwise 3x3), bn
                                                .gate.fc1 / .gate.fc2 (1x1 convs with bias)
                                                .conv3 (Conv1x1Linear: conv, bn), .downsample (same)
    conv{2,3}.2.0              Conv1x1          transition before the 2x2 average pool
    conv5                      Conv1x1
    fc.0 / fc.1                Linear + BatchNorm1d

Two more variants share the loader (VARIANT of the descriptor, models/reid.py):

    'ibn'   osnet_ibn_x1_0 (osnet.py with IN=True): the names above; conv1.bn is an InstanceNorm2d(affine) -- weight and bias,
            no running statistics -- and every block of conv2 / conv3 has .IN (InstanceNorm2d(affine))
    'ain'   osnet_ain_x* (osnet_ain.py): streams  .conv2.{0..3}.layers.{i} (LightConvStream; LightConv3x3 as above),
            transitions  pool2.0 / pool3.0 (Conv1x1 in front of the average pool), conv1.bn an InstanceNorm2d as for 'ibn',
            OSBlockINin blocks (conv2.0, conv2.1, conv3.1, conv4.0) with .IN and a .conv3 WITHOUT batch norm and bias
These names are derived from the published torchreid sources, not checked against a checkpoint.

PyTorch is used for unpickling only (`torch.load`); a plain dict of arrays works as well -- that is how the
reference's ONNX export of the same model arrives (models/onnx_reader.torchreid_state_dict_from_onnx).
"""
import numpy as np

_STREAM = {1: 'conv2a', 2: 'conv2b', 3: 'conv2c', 4: 'conv2d'}


VARIANTS = ('osnet', 'ibn', 'ain')


def _key(name, variant='osnet'):
    """Layer-table parameter name (models/reid.py) -> (state_dict prefix of the conv / linear, prefix of the
    batch norm or None).  variant 'ain': the module names of osnet_ain.py where they differ."""
    parts = name.split('.')
    if name == 'conv1' or name == 'conv5':
        return f'{name}.conv', f'{name}.bn'
    if name == 'fc':
        return 'fc.0', 'fc.1'
    stage = parts[0]                                   # conv2 / conv3 / conv4
    if parts[1] == 't':
        if variant == 'ain':
            return f'pool{stage[4:]}.0.conv', f'pool{stage[4:]}.0.bn'
        return f'{stage}.2.0.conv', f'{stage}.2.0.bn'
    block = f'{stage}.{parts[1]}'
    tail = parts[2:]
    if tail == ['conv1']:
        return f'{block}.conv1.conv', f'{block}.conv1.bn'
    if tail == ['conv3']:
        return f'{block}.conv3.conv', f'{block}.conv3.bn'
    if tail == ['down']:
        return f'{block}.downsample.conv', f'{block}.downsample.bn'
    if tail[0] == 'gate':
        return f'{block}.gate.{tail[1]}', None
    if tail[0].startswith('s') and tail[-1] in ('pw', 'dw'):
        t, i = int(tail[0][1:]), int(tail[1])
        if variant == 'ain':
            lc = f'{block}.conv2.{t - 1}.layers.{i}'
            return (f'{lc}.conv1', None) if tail[-1] == 'pw' else (f'{lc}.conv2', f'{lc}.bn')
        lc = f'{block}.{_STREAM[t]}' if t == 1 else f'{block}.{_STREAM[t]}.{i}'
        return (f'{lc}.conv1', None) if tail[-1] == 'pw' else (f'{lc}.conv2', f'{lc}.bn')
    raise KeyError(f'no torchreid parameter for layer {name!r}')


def _in_key(name):
    """Layer-table name of an instance normalisation -> state_dict prefix: the stem's is the module torchreid still calls
    `bn` (ConvLayer(IN=True)), a block's is `IN`."""
    if name == 'conv1.IN':
        return 'conv1.bn'
    parts = name.split('.')
    if len(parts) == 3 and parts[2] == 'IN':
        return name
    raise KeyError(f'no torchreid instance normalisation for layer {name!r}')


class TorchreidWeights:
    def __init__(self, source, variant='osnet'):
        if variant not in VARIANTS:
            raise ValueError(f'variant {variant!r}: expected one of {VARIANTS}')
        self.variant = variant
        if isinstance(source, dict):
            sd = source
        else:
            import torch
            sd = torch.load(source, map_location='cpu')
        if 'state_dict' in sd and not any(k.endswith('.weight') for k in sd):
            sd = sd['state_dict']
        self.sd = {(k[7:] if k.startswith('module.') else k): np.asarray(getattr(v, 'numpy', lambda: v)(), np.float32)
                   for k, v in sd.items() if not k.endswith('num_batches_tracked')}
        self.used = set()

    def _get(self, key, shape=None):
        if key not in self.sd:
            raise KeyError(f'checkpoint has no parameter {key!r}')
        self.used.add(key)
        a = self.sd[key]
        if shape is not None and tuple(a.shape) != tuple(shape):
            raise ValueError(f'{key}: checkpoint shape {tuple(a.shape)} != expected {tuple(shape)}')
        return a

    def _bn(self, prefix, c):
        return dict(gamma=self._get(prefix + '.weight', (c,)), beta=self._get(prefix + '.bias', (c,)),
                    mean=self._get(prefix + '.running_mean', (c,)), var=self._get(prefix + '.running_var', (c,)))

    def conv(self, name, cout, cin, k, bn=True, gain=1.0, groups=1):
        ck, bk = _key(name, self.variant)
        p = dict(w=self._get(ck + '.weight', (cout, cin // groups, k, k)))
        if ck + '.bias' in self.sd:
            p['bias'] = self._get(ck + '.bias', (cout,))
        elif not bn:
            p['bias'] = np.zeros(cout, np.float32)
        if bn:
            if bk is None:
                raise KeyError(f'layer {name!r} has no batch norm in torchreid')
            if bk + '.weight' in self.sd:
                p.update(self._bn(bk, cout))
            elif ck + '.bias' not in self.sd:
                # (a source whose exporter folded BatchNorm into the conv -- ONNX, models/onnx_reader.py -- carries
                # the folded bias instead of the four BatchNorm vectors)
                raise KeyError(f'checkpoint has neither {bk}.* nor a folded {ck}.bias')
        return p

    def linear(self, name, cout, cin, bn=False):
        ck, bk = _key(name, self.variant)
        p = dict(w=self._get(ck + '.weight', (cout, cin)))
        if ck + '.bias' in self.sd:
            p['bias'] = self._get(ck + '.bias', (cout,))
        if bn and (bk + '.weight' in self.sd or ck + '.bias' not in self.sd):
            p.update(self._bn(bk, cout))
        return p

    def instnorm(self, name, c):
        """-> (gamma, beta) of an InstanceNorm2d(c, affine=True).  It has no running statistics: a module that carries
        them is a BatchNorm2d -- the checkpoint of another variant -- and is refused by name."""
        prefix = _in_key(name)
        if prefix + '.running_mean' in self.sd:
            raise KeyError(f'checkpoint has running statistics {prefix + ".running_mean"!r}: a BatchNorm2d where the '
                           f'{self.variant!r} variant has an InstanceNorm2d')
        return self._get(prefix + '.weight', (c,)), self._get(prefix + '.bias', (c,))

    def unused(self):
        """Checkpoint entries the layer table did not consume (the classifier is expected)."""
        return sorted(k for k in self.sd if k not in self.used and not k.startswith('classifier'))
