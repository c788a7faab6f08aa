"""ReID model descriptors (registry + attributes of fastmot/models/reid.py:10-45,95-109) and the
OSNet layer table for the HIP conv engine (torchreid osnet_x1_0 / osnet_x0_25 topology,
SURVEY.md appendix A: 978.9 / 82.3 MMAC per 256x128 crop)."""
from pathlib import Path

import numpy as np

from .graph import Graph, RES_AFTER_NORM, RES_BEFORE_ACT, RES_BEFORE_NORM, fold_bn, missing_weights


class ReID:
    """Base class for ReID models.

    ENGINE_PATH / MODEL_PATH : cache / checkpoint locations; INPUT_SHAPE (c, h, w);
    OUTPUT_LAYOUT : feature dimension; METRIC : {'euclidean', 'cosine'}.
    """
    __registry = {}

    PLUGIN_PATH = None
    ENGINE_PATH = None
    MODEL_PATH = None
    INPUT_SHAPE = None
    OUTPUT_LAYOUT = None
    METRIC = None
    CHANNELS = None
    VARIANT = 'osnet'       # which torchreid OSNet a descriptor with CHANNELS is: 'osnet', 'ibn' (osnet_ibn_*), 'ain' (osnet_ain_*)

    def __init_subclass__(cls, **kwargs):
        super().__init_subclass__(**kwargs)
        cls.__registry[cls.__name__] = cls

    @classmethod
    def get_model(cls, name):
        return cls.__registry[name]

    @classmethod
    def weight_file(cls):
        """MODEL_PATH if it exists, else the same stem as a torchreid checkpoint (.pth, .pth.tar); None."""
        if cls.MODEL_PATH is None:
            return None
        base = Path(cls.MODEL_PATH)
        for cand in (base, base.with_suffix('.pth'), base.with_suffix('.pth.tar')):
            if cand.is_file():
                return cand
        return None

    @classmethod
    def build_graph(cls, weights=None, fuse_lightconv=True):
        """Weights: the explicit source, else the model file at MODEL_PATH -- the reference's ONNX export
        (models/onnx_reader.py; fastmot/models/reid.py:97,106) or, next to it with the suffix .pth / .pth.tar, the
        torchreid checkpoint it was exported from (models/torchreid_weights.py); a missing file raises
        FileNotFoundError unless seeded random parameters were opted into (models.allow_random_weights()).

        A descriptor with CHANNELS set is an OSNet: its topology is built here (osnet_graph) and the file only supplies
        the parameters.  A descriptor with CHANNELS = None (the reference's "Add custom ReID": MODEL_PATH, INPUT_SHAPE,
        OUTPUT_LAYOUT, METRIC) takes topology AND parameters from its ONNX file (models/onnx_graph.py); `weights` may
        then be the path or the bytes of such a file."""
        onnx_src = weights if isinstance(weights, (str, Path, bytes, bytearray, memoryview)) else None
        if cls.CHANNELS is None:
            from .onnx_graph import lower
            from .onnx_reader import OnnxModel
            if weights is not None and onnx_src is None and not isinstance(weights, OnnxModel):
                raise TypeError(f'{cls.__name__} has no CHANNELS: its topology comes from an ONNX file; weights= must be the '
                                f'path or the bytes of one, not {type(weights).__name__}')
            src = weights
            if src is None:
                src = cls.weight_file()
                if src is None or src.suffix != '.onnx':
                    raise FileNotFoundError(
                        f'{cls.__name__}: ONNX file {cls.MODEL_PATH} not found.  A ReID descriptor without CHANNELS takes its '
                        'topology from that file: put it there or pass weights=<path or bytes of the .onnx>')
            return lower(src, cls.INPUT_SHAPE, cls.OUTPUT_LAYOUT, where=f'{cls.__name__} ({cls.MODEL_PATH if weights is None else "weights="})')
        ckpt = None
        if onnx_src is not None:
            from .onnx_reader import torchreid_state_dict_from_onnx
            from .torchreid_weights import TorchreidWeights
            weights = ckpt = TorchreidWeights(torchreid_state_dict_from_onnx(onnx_src, cls.CHANNELS, cls.OUTPUT_LAYOUT, cls.VARIANT), cls.VARIANT)
        if weights is None:
            path = cls.weight_file()
            if path is not None:
                from .torchreid_weights import TorchreidWeights
                if path.suffix == '.onnx':
                    from .onnx_reader import torchreid_state_dict_from_onnx
                    weights = ckpt = TorchreidWeights(torchreid_state_dict_from_onnx(path, cls.CHANNELS, cls.OUTPUT_LAYOUT,
                                                                                     cls.VARIANT), cls.VARIANT)
                else:
                    weights = ckpt = TorchreidWeights(path, cls.VARIANT)
            else:
                weights = missing_weights(cls, seed=1)
        out = osnet_graph(cls, weights, fuse_lightconv)
        if ckpt is not None and ckpt.unused():
            raise ValueError(f'{cls.MODEL_PATH}: parameters not used by {cls.__name__}: {ckpt.unused()[:5]} ...')
        return out

    @classmethod
    def from_onnx(cls, path, metric='euclidean', name=None):
        """Creates and registers a descriptor for an ONNX file (models/onnx_graph.py lists what it may contain):
        INPUT_SHAPE and OUTPUT_LAYOUT are read from the file.  The returned class's name -- `name`, by default the
        file's stem with every other character than letters, digits and '_' replaced by '_' -- then works as
        feature_extractor_cfgs[].model."""
        import re
        from .onnx_graph import lower
        path = Path(path)
        if not path.is_file():
            raise FileNotFoundError(f'ReID.from_onnx: {path} not found')
        if metric not in ('euclidean', 'cosine'):
            raise ValueError(f'metric {metric!r}: expected euclidean or cosine')
        g, _ = lower(path)
        h, w, _, _ = g.tensors[g.input.tid]
        name = name or re.sub(r'\W', '_', path.stem)
        if not name.isidentifier():
            raise ValueError(f'{name!r} is not a usable model name: pass name=')
        return type(name, (cls,), dict(MODEL_PATH=path, ENGINE_PATH=path.with_suffix('.hipnet'), INPUT_SHAPE=(g.input.c, h, w),
                                       OUTPUT_LAYOUT=g.layers[-1]['cout'], METRIC=metric, CHANNELS=None,
                                       __doc__=f'ReID model read from {path.name}'))


# the instance normalisation in the tail of a block, per variant and block (None: OSNet's plain block)
#   'ibn'  osnet.py, IN=True:   relu(IN(conv3(x2) + identity)) in every block of conv2 and conv3
#   'ain'  osnet_ain.py:        OSBlockINin, relu(IN(conv3(x2)) + identity) with a conv3 that has neither batch norm nor bias;
#                               blocks [[INin, INin], [OSBlock, INin], [INin, OSBlock]]
_BLOCK_IN = {'osnet': {},
             'ibn': {b: 'ibn' for b in ('conv2.0', 'conv2.1', 'conv3.0', 'conv3.1')},
             'ain': {b: 'ain' for b in ('conv2.0', 'conv2.1', 'conv3.1', 'conv4.0')}}


def osnet_graph(model, weights, fuse_lightconv=True):
    _, H, W = model.INPUT_SHAPE
    c0, c1, c2, c3 = model.CHANNELS
    variant = getattr(model, 'VARIANT', 'osnet')
    block_in = _BLOCK_IN[variant]
    g = Graph(weights, (H, W), 3)

    def osblock(name, x, cout, cat=None):
        """cat: [mid + x.c]-channel tensor whose upper slice already is x (the producer wrote it there):
        the gated sum goes to the lower slice and the block tail relu(conv3(x2) + downsample(x)) becomes
        ONE 1x1 conv over the concatenated channels with weights [W3 | Wd], bias b3 + bd."""
        mid = cout // 4
        x1 = g.conv(name + '.conv1', x, mid, 1, 1, 'relu')
        hid = max(mid // 16, 1)
        if fuse_lightconv and mid % 8 == 0 and mid <= 128:
            # stream t (1..4) is a chain of t LightConv3x3; the chains are independent: all of them run as
            # ONE launch when two halo tiles fit in LDS (litechain.hip), otherwise depth i of all streams that
            # reach it as one grouped launch (4, 3, 2, 1 groups); the four gates + the gated sum are one more.
            params = {(t, i): g.lightconv_params(f'{name}.s{t}.{i}', mid) for t in range(1, 5) for i in range(t)}
            streams, parts, prev = [], [], None
            chain = g.use_lightchain and g.lightchain_fits(mid, x1.h, x1.w)
            if chain:                    # all four chains in one launch: 2 launches per block tail
                y = g.lightchain(f'{name}.streams', x1, [params[(t, i)] for t in range(1, 5) for i in range(t)], 'relu')
                streams = [y.slice(t * mid, mid) for t in range(4)]
                parts = g.last_gap_slots
            for i in range(0 if chain else 4):
                ts = list(range(i + 1, 5))                       # streams alive at depth i
                xs = [x1] * len(ts) if i == 0 else [prev.slice((t - i) * mid, mid) for t in ts]
                prev = g.lightconv_group(f'{name}.depth{i}', xs, [params[(t, i)] for t in ts], 'relu', gap_slot=True)
                streams.append(prev.slice(0, mid))               # stream i+1 ends at depth i (group 0)
                parts.append(g.last_gap_slot)
            x2 = g.gated_sum(name + '.gate', streams, hid, parts=parts,
                             dst=cat.slice(0, mid) if cat is not None else None)
        else:
            streams, gids = [], []
            gp = None
            for t in range(1, 5):
                s = x1
                for i in range(t):
                    s = g.lightconv(f'{name}.s{t}.{i}', s, mid, 'relu', fuse=False)
                streams.append(s)
            for s in streams:
                gid, gp = g.gate(name + '.gate', s, hid, gp)
                gids.append(gid)
            x2 = g.gate_sum(streams, gids)
        kind = block_in.get(name)
        if cat is not None:
            wd, bd = fold_bn(weights.conv(name + '.down', cout, x.c, 1, bn=True))
            w3, b3 = fold_bn(weights.conv(name + '.conv3', cout, mid, 1, bn=True))
            wb = (np.concatenate([w3, wd], axis=1), b3 + bd)
            if kind == 'ibn':       # conv3 + downsample is linear: the concat form holds, the norm and the ReLU follow it
                return g.convin(name + '.conv3+down', cat, cout, name + '.IN', act='relu', wb=wb)
            return g.conv(name + '.conv3+down', cat, cout, 1, 1, 'relu', wb=wb)
        if x.c != cout:
            ident = g.conv(name + '.down', x, cout, 1, 1, 'linear')
        else:
            ident = x
        if kind == 'ibn':
            return g.convin(name + '.conv3', x2, cout, name + '.IN', act='relu', res=ident, res_mode=RES_BEFORE_NORM)
        if kind == 'ain':           # only the conv3 half is normalised: no concat form; Conv1x1Linear(bn=False)
            return g.convin(name + '.conv3', x2, cout, name + '.IN', act='relu', res=ident, res_mode=RES_AFTER_NORM, bn=False, bias=False)
        return g.conv(name + '.conv3', x2, cout, 1, 1, 'relu', res=ident, res_mode=RES_BEFORE_ACT)

    def down_block(name, make_x, cin, cout, h, w):
        """First block of a stage (cin != cout).  make_x(dst) emits the layer producing the block input."""
        mid = cout // 4
        if fuse_lightconv and mid % 8 == 0 and mid <= 128 and block_in.get(name) != 'ain':
            cat = g.new(h, w, mid + cin)
            return osblock(name, make_x(cat.slice(mid, cin)), cout, cat=cat)
        return osblock(name, make_x(None), cout)

    if variant == 'osnet':
        s = g.conv('conv1', g.input, c0, 7, 2, 'relu', pad=3)
    else:       # ConvLayer(IN=True): conv (no bias), InstanceNorm2d(affine), ReLU -- the norm needs the whole map: conv + instnorm
        s = g.conv('conv1', g.input, c0, 7, 2, 'linear', pad=3, bn=False, bias=False)
        s = g.instnorm('conv1.IN', s, *weights.instnorm('conv1.IN', c0), 1e-5, 'relu')
    x = down_block('conv2.0', lambda dst: g.pool(s, 3, 2, 1, dst=dst), c0, c1, H // 4, W // 4)
    x = osblock('conv2.1', x, c1)
    t2 = g.conv('conv2.t', x, c1, 1, 1, 'relu')
    x = down_block('conv3.0', lambda dst: g.pool(t2, 2, 2, 0, avg=True, dst=dst), c1, c2, H // 8, W // 8)
    x = osblock('conv3.1', x, c2)
    t3 = g.conv('conv3.t', x, c2, 1, 1, 'relu')
    tail = len(g.layers)
    x = down_block('conv4.0', lambda dst: g.pool(t3, 2, 2, 0, avg=True, dst=dst), c2, c3, H // 16, W // 16)
    x = osblock('conv4.1', x, c3)
    x = g.conv('conv5', x, c3, 1, 1, 'relu')
    g.head('fc', x, model.OUTPUT_LAYOUT)
    g.outputs = [x]
    fused = g.fuse_ostail(tail)       # x0.25 widths: everything after the last transition conv as one launch (ostail.hip)
    assert not (fused and variant == 'ain')     # (its conv4.0 is an OSBlockINin: not the sequence that launch computes)
    return g, x


class OSNet025(ReID):
    ENGINE_PATH = Path(__file__).parent / 'osnet_x0_25_msmt17.hipnet'
    MODEL_PATH = Path(__file__).parent / 'osnet_x0_25_msmt17.onnx'
    INPUT_SHAPE = (3, 256, 128)
    OUTPUT_LAYOUT = 512
    METRIC = 'euclidean'
    CHANNELS = (16, 64, 96, 128)


class OSNet10(ReID):
    """Multi-source model trained on MSMT17, DukeMTMC, and CUHK03, not provided."""
    ENGINE_PATH = Path(__file__).parent / 'osnet_x1_0_msdc.hipnet'
    MODEL_PATH = Path(__file__).parent / 'osnet_x1_0_msdc.onnx'
    INPUT_SHAPE = (3, 256, 128)
    OUTPUT_LAYOUT = 512
    METRIC = 'cosine'
    CHANNELS = (64, 256, 384, 512)


class OSNetIBN10(ReID):
    """torchreid osnet_ibn_x1_0: OSNet with instance normalisation in the stem and behind the residual sum of the blocks
    of conv2 and conv3.  Not provided."""
    ENGINE_PATH = Path(__file__).parent / 'osnet_ibn_x1_0.hipnet'
    MODEL_PATH = Path(__file__).parent / 'osnet_ibn_x1_0.onnx'
    INPUT_SHAPE = (3, 256, 128)
    OUTPUT_LAYOUT = 512
    METRIC = 'cosine'
    CHANNELS = (64, 256, 384, 512)
    VARIANT = 'ibn'


class OSNetAIN10(ReID):
    """torchreid osnet_ain_x1_0 (the architecture found by OSNet-AIN's search: OSBlockINin blocks).  Not provided."""
    ENGINE_PATH = Path(__file__).parent / 'osnet_ain_x1_0.hipnet'
    MODEL_PATH = Path(__file__).parent / 'osnet_ain_x1_0.onnx'
    INPUT_SHAPE = (3, 256, 128)
    OUTPUT_LAYOUT = 512
    METRIC = 'cosine'
    CHANNELS = (64, 256, 384, 512)
    VARIANT = 'ain'


class OSNetAIN025(ReID):
    """torchreid osnet_ain_x0_25.  Not provided."""
    ENGINE_PATH = Path(__file__).parent / 'osnet_ain_x0_25.hipnet'
    MODEL_PATH = Path(__file__).parent / 'osnet_ain_x0_25.onnx'
    INPUT_SHAPE = (3, 256, 128)
    OUTPUT_LAYOUT = 512
    METRIC = 'cosine'
    CHANNELS = (16, 64, 96, 128)
    VARIANT = 'ain'
