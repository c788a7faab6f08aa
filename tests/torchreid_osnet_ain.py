"""TEST INFRASTRUCTURE: torchreid's two OSNet variants for unseen domains in plain PyTorch, with torchreid's module structure
so that `state_dict()` carries the names a torchreid checkpoint would -- written from the published sources
(torchreid/models/osnet.py with IN=True: osnet_ibn_x1_0; torchreid/models/osnet_ain.py: osnet_ain_x1_0 / _x0_75 / _x0_5 /
_x0_25).  No checkpoint of either was at hand: the names are derived, not pinned.

    both      conv1 = ConvLayer(IN=True): conv, InstanceNorm2d(affine) -- the module is still called `bn` --, ReLU
    'ibn'     OSBlock(IN=True) in conv2 and conv3: relu(IN(conv3(x2) + identity)); everything else is tests/torchreid_osnet.py
    'ain'     streams conv2 = ModuleList(LightConvStream(mid, mid, t)), transitions pool2 / pool3 = Sequential(Conv1x1,
              AvgPool2d); blocks [[INin, INin], [OSBlock, INin], [INin, OSBlock]]; OSBlockINin: conv3 = Conv1x1Linear(bn=False),
              relu(IN(conv3(x2)) + identity)
"""
import torch
from torch import nn
from torch.nn import functional as F

from fastmot_amd.models import ReID
from torchreid_osnet import ChannelGate, Conv1x1, Conv1x1Linear, LightConv3x3, OSBlock

X025 = (16, 64, 96, 128)


class TinyIBN025(ReID):
    """osnet_ibn at x0.25 widths (torchreid ships only x1.0): the small widths of the IBN tail, and the ostail pattern."""
    INPUT_SHAPE = (3, 256, 128)
    OUTPUT_LAYOUT = 512
    METRIC = 'cosine'
    CHANNELS = X025
    VARIANT = 'ibn'


def small(desc, hw=(64, 32)):
    """The descriptor at a smaller input."""
    return type('Small' + desc.__name__, (desc,), dict(INPUT_SHAPE=(3,) + tuple(hw)))


def sd_of(net):
    return {k: v.numpy() for k, v in net.state_dict().items()}


class ConvLayerIN(nn.Module):
    def __init__(self, cin, cout, k, stride=1, padding=0):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, stride=stride, padding=padding, bias=False)
        self.bn = nn.InstanceNorm2d(cout, affine=True)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)))


class OSBlockIBN(OSBlock):
    """osnet.py OSBlock(IN=True)"""

    def __init__(self, cin, cout):
        super().__init__(cin, cout)
        self.IN = nn.InstanceNorm2d(cout, affine=True)

    def forward(self, x):
        x1 = self.conv1(x)
        x2 = self.gate(self.conv2a(x1)) + self.gate(self.conv2b(x1)) + self.gate(self.conv2c(x1)) + self.gate(self.conv2d(x1))
        ident = self.downsample(x) if self.downsample is not None else x
        return F.relu(self.IN(self.conv3(x2) + ident))


class Conv1x1LinearNoBN(nn.Module):
    """osnet_ain.py Conv1x1Linear(bn=False)"""

    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, 1, bias=False)

    def forward(self, x):
        return self.conv(x)


class LightConvStream(nn.Module):
    def __init__(self, cin, cout, depth):
        super().__init__()
        self.layers = nn.Sequential(*[LightConv3x3(cin if i == 0 else cout, cout) for i in range(depth)])

    def forward(self, x):
        return self.layers(x)


class OSBlockAIN(nn.Module):
    """osnet_ain.py OSBlock (inin=False) and OSBlockINin (inin=True)"""

    def __init__(self, cin, cout, inin):
        super().__init__()
        mid = cout // 4
        self.conv1 = Conv1x1(cin, mid)
        self.conv2 = nn.ModuleList([LightConvStream(mid, mid, t) for t in range(1, 5)])
        self.gate = ChannelGate(mid)
        self.conv3 = Conv1x1LinearNoBN(mid, cout) if inin else Conv1x1Linear(mid, cout)
        self.downsample = Conv1x1Linear(cin, cout) if cin != cout else None
        if inin:
            self.IN = nn.InstanceNorm2d(cout, affine=True)
        self.inin = inin

    def forward(self, x):
        x1 = self.conv1(x)
        x2 = 0
        for s in self.conv2:
            x2 = x2 + self.gate(s(x1))
        x3 = self.conv3(x2)
        if self.inin:
            x3 = self.IN(x3)
        ident = self.downsample(x) if self.downsample is not None else x
        return F.relu(x3 + ident)


class OSNetVariant(nn.Module):
    def __init__(self, channels, variant, feature_dim=512, num_classes=10):
        super().__init__()
        assert variant in ('ibn', 'ain')
        c0, c1, c2, c3 = channels
        self.variant = variant
        self.conv1 = ConvLayerIN(3, c0, 7, stride=2, padding=3)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)

        def transition(c):
            return nn.Sequential(Conv1x1(c, c), nn.AvgPool2d(2, stride=2))
        if variant == 'ibn':
            self.conv2 = nn.Sequential(OSBlockIBN(c0, c1), OSBlockIBN(c1, c1), transition(c1))
            self.conv3 = nn.Sequential(OSBlockIBN(c1, c2), OSBlockIBN(c2, c2), transition(c2))
            self.conv4 = nn.Sequential(OSBlock(c2, c3), OSBlock(c3, c3))
        else:
            self.conv2 = nn.Sequential(OSBlockAIN(c0, c1, True), OSBlockAIN(c1, c1, True))
            self.pool2 = transition(c1)
            self.conv3 = nn.Sequential(OSBlockAIN(c1, c2, False), OSBlockAIN(c2, c2, True))
            self.pool3 = transition(c2)
            self.conv4 = nn.Sequential(OSBlockAIN(c2, c3, True), OSBlockAIN(c3, c3, False))
        self.conv5 = Conv1x1(c3, c3)
        self.fc = nn.Sequential(nn.Linear(c3, feature_dim), nn.BatchNorm1d(feature_dim), nn.ReLU(inplace=True))
        self.classifier = nn.Linear(feature_dim, num_classes)

    def forward(self, x):
        x = self.maxpool(self.conv1(x))
        if self.variant == 'ibn':
            x = self.conv4(self.conv3(self.conv2(x)))
        else:
            x = self.conv4(self.pool3(self.conv3(self.pool2(self.conv2(x)))))
        x = self.conv5(x)
        return self.fc(F.adaptive_avg_pool2d(x, 1).flatten(1))      # eval mode: the feature vector


def random_variant(channels, variant, seed=0, feature_dim=512):
    """Seeded parameters with BatchNorm statistics and InstanceNorm affines away from the identity."""
    torch.manual_seed(seed)
    m = OSNetVariant(channels, variant, feature_dim)
    for mod in m.modules():
        if isinstance(mod, (nn.BatchNorm2d, nn.BatchNorm1d)):
            mod.weight.data.uniform_(0.8, 1.2)
            mod.bias.data.normal_(0, 0.1)
            mod.running_mean.normal_(0, 0.1)
            mod.running_var.uniform_(0.8, 1.2)
        elif isinstance(mod, nn.InstanceNorm2d):
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.normal_(0, 0.3)
    return m.eval()
