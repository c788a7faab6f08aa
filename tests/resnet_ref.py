"""TEST INFRASTRUCTURE: the ResNet family of torchvision / torchreid / fast-reid restated in plain torch (neither
package is available here), with seeded random parameters, and its ONNX export in both exporter forms.

  block   'basic' (two 3x3 convs, expansion 1) or 'bottleneck' (v1.5: 1x1, 3x3 carrying the stride, 1x1; expansion 4);
          the first block of a stage has a 1x1 downsample conv (stride 1 in stage 1, 2 afterwards) + BatchNorm
  pool    'pad1' (MaxPool2d(3, 2, 1): torchvision, torchreid) or 'ceil' (MaxPool2d(3, 2, 0, ceil_mode=True): fast-reid)
  head    'none' (the pooled vector), 'bnneck' (BatchNorm1d on it: fast-reid's bag of tricks) or 'fc512'
          (Linear -> BatchNorm1d -> ReLU: torchreid's resnet50_fc512; its width is `fc_dim`)
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F



def export_with_torch(module, x, **kw):
    """The recipe of tests/test_onnx_reader.py: torch.onnx.export (TorchScript exporter) without the `onnx` package -- only
    its last step, looking for onnxscript functions in the finished proto, imports it, and is skipped."""
    import io
    import warnings
    from torch.onnx._internal.torchscript_exporter import onnx_proto_utils
    orig = onnx_proto_utils._add_onnxscript_fn
    onnx_proto_utils._add_onnxscript_fn = lambda proto, custom_opsets: proto
    buf = io.BytesIO()
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            torch.onnx.export(module, x, buf, dynamo=False, opset_version=11, input_names=['input'],
                              output_names=['output'], **kw)
    finally:
        onnx_proto_utils._add_onnxscript_fn = orig
    return buf.getvalue()


def _bn(c):
    return nn.BatchNorm2d(c)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, cin, mid, stride, down):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(cin, mid, 3, stride, 1, bias=False), _bn(mid)
        self.conv2, self.bn2 = nn.Conv2d(mid, mid, 3, 1, 1, bias=False), _bn(mid)
        self.downsample = nn.Sequential(nn.Conv2d(cin, mid, 1, stride, bias=False), _bn(mid)) if down else None

    def forward(self, x):
        out = F.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return F.relu(out + (x if self.downsample is None else self.downsample(x)))


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, cin, mid, stride, down):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(cin, mid, 1, bias=False), _bn(mid)
        self.conv2, self.bn2 = nn.Conv2d(mid, mid, 3, stride, 1, bias=False), _bn(mid)
        self.conv3, self.bn3 = nn.Conv2d(mid, mid * 4, 1, bias=False), _bn(mid * 4)
        self.downsample = nn.Sequential(nn.Conv2d(cin, mid * 4, 1, stride, bias=False), _bn(mid * 4)) if down else None

    def forward(self, x):
        out = F.relu(self.bn1(self.conv1(x)))
        out = F.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return F.relu(out + (x if self.downsample is None else self.downsample(x)))


class ResNet(nn.Module):
    def __init__(self, block='bottleneck', layers=(3, 4, 6, 3), widths=(64, 128, 256, 512), stem=64, pool='pad1',
                 head='none', fc_dim=512, last_stride=2):
        super().__init__()
        B = {'basic': BasicBlock, 'bottleneck': Bottleneck}[block]
        self.conv1, self.bn1 = nn.Conv2d(3, stem, 7, 2, 3, bias=False), _bn(stem)
        self.maxpool = nn.MaxPool2d(3, 2, 1) if pool == 'pad1' else nn.MaxPool2d(3, 2, 0, ceil_mode=True)
        blocks, cin = [], stem
        for si, (n, mid) in enumerate(zip(layers, widths)):
            stride = 1 if si == 0 else (last_stride if si == 3 else 2)
            for bi in range(n):
                blocks.append(B(cin, mid, stride if bi == 0 else 1, down=bi == 0 and (stride != 1 or cin != mid * B.expansion)))
                cin = mid * B.expansion
        self.blocks = nn.Sequential(*blocks)
        self.head, self.feat = head, cin
        if head == 'bnneck':
            self.neck = nn.BatchNorm1d(cin)
        elif head == 'fc512':
            self.fc, self.fc_bn = nn.Linear(cin, fc_dim), nn.BatchNorm1d(fc_dim)
        self.out_dim = fc_dim if head == 'fc512' else cin

    def forward(self, x):
        x = self.maxpool(F.relu(self.bn1(self.conv1(x))))
        x = self.blocks(x)
        v = torch.flatten(F.adaptive_avg_pool2d(x, 1), 1)
        if self.head == 'bnneck':
            v = self.neck(v)
        elif self.head == 'fc512':
            v = F.relu(self.fc_bn(self.fc(v)))
        return v


def seeded(net, seed):
    """Variance-preserving conv weights and non-trivial BatchNorm statistics (a fresh BatchNorm is the identity: folding
    mistakes would not show)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                fan = m.weight[0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (1.6 / fan) ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
            elif isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) * 0.4 + 0.6)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.bias.shape, generator=g) * 0.4 + 0.8)
    return net.eval()


def tiny(block='bottleneck', pool='pad1', head='none', seed=3):
    """One block per stage, mid widths 8 / 16 / 32 / 64 (bottleneck outputs 32 ... 256), stem 16, fc 24."""
    return seeded(ResNet(block, (1, 1, 1, 1), (8, 16, 32, 64), stem=16, pool=pool, head=head, fc_dim=24), seed)


def resnet50(pool='pad1', head='none', seed=7):
    return seeded(ResNet('bottleneck', (3, 4, 6, 3), (64, 128, 256, 512), stem=64, pool=pool, head=head), seed)


def export(net, hw=(64, 32), folded=True):
    """-> bytes of the ONNX file.  folded: the exporter's default (eval mode: BatchNorm folded into the convs, anonymous
    initialisers); otherwise explicit BatchNormalization nodes and the module's parameter names."""
    x = torch.zeros(1, 3, *hw)
    if folded:
        return export_with_torch(net, x)
    return export_with_torch(net, x, training=torch.onnx.TrainingMode.PRESERVE, do_constant_folding=False,
                             keep_initializers_as_inputs=True)


def embed(net, x):
    """The module's L2-normalised output, fp32 numpy."""
    with torch.no_grad():
        v = net(torch.as_tensor(x, dtype=torch.float32))
    return (v / v.norm(dim=1, keepdim=True)).numpy()


def random_input(n, hw, seed=1):
    return np.random.default_rng(seed).normal(0, 1, (n, 3) + tuple(hw)).astype(np.float32)
