"""SSD model descriptors (registry + class attributes of fastmot/models/ssd.py:9-49,99-107,197-205,294-301).

The reference builds these networks from TensorFlow frozen graphs through graphsurgeon + UFF + a TensorRT < 8
parser, with the anchors (GridAnchor_TRT) and the box decode + NMS (NMS_TRT) as plugins inside the engine.

`SSDMobileNetV1.build_graph` lowers the network itself to the HIP conv engine: TF-slim MobileNetV1 (stem conv +
13 separable blocks, one FM_OP_SEPCONV launch each) + the Object Detection API's SSD feature maps and box predictors,
TensorFlow "SAME" padding, BatchNorm (eps 1e-3) folded, ReLU6.  The anchors of `anchors()` are those of
`create_ssd_anchors(..., reduce_boxes_in_lowest_layer=True)` with the values the reference passes to GridAnchor_TRT
(reference models/ssd.py:125-134).  Weights come from a mapping of TF variable names, an .npz of one, or a frozen .pb
(models/tf_graph_reader.py); the variable names below are DERIVED from the slim / Object Detection API sources, not pinned
against a file -- neither TensorFlow nor the .pb exist where this was written.
SSDMobileNetV2 / SSDInceptionV2 have no lowering: their `build_graph` raises, and `SSDDetector` (detector.py) runs its
tiling / normalisation / filtering / merging stages around any inference callable (its `backend` argument).
"""
import math
from pathlib import Path

import numpy as np

from .graph import Graph, RandomWeights, fold_bn, missing_weights


class SSD:
    """Base class: subclasses register themselves by name (fastmot/models/ssd.py:36-44)."""
    _registry = {}

    ENGINE_PATH = None
    MODEL_PATH = None
    NUM_CLASSES = None
    INPUT_SHAPE = None      # (channel, height, width)
    OUTPUT_NAME = None
    NMS_THRESH = None
    TOPK = None             # detections per tile in the network output

    def __init_subclass__(cls, **kwargs):
        super().__init_subclass__(**kwargs)
        SSD._registry[cls.__name__] = cls

    @classmethod
    def get_model(cls, name):
        return SSD._registry[name]

    @classmethod
    def build_graph(cls, weights=None, max_batch=1):
        raise NotImplementedError(f'{cls.__name__}: no lowering of this network to the conv engine (SSDMobileNetV1 has one); '
                                  'pass an inference callable to SSDDetector(backend=...) or use SSDMobileNetV1 / '
                                  'detector_type YOLO / PUBLIC')


class TFWeights:
    """A mapping {TF variable name: array} (conv kernels HWIO, depthwise [3, 3, C, 1], as TensorFlow stores them)
    through the weight-source interface of Graph (`conv(name, cout, cin, k, bn, groups)`; `name` = the variable scope)."""

    def __init__(self, arrays):
        self.arrays = arrays

    def _get(self, name, shape):
        if name not in self.arrays:
            raise KeyError(f'no variable {name!r} in the weight source')
        a = np.asarray(self.arrays[name], np.float32)
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f'{name}: shape {tuple(a.shape)}, the topology needs {tuple(shape)}')
        return a

    def conv(self, name, cout, cin, k, bn=True, gain=1.0, groups=1):
        if groups == 1:
            w = self._get(name + '/weights', (k, k, cin, cout)).transpose(3, 2, 0, 1)
        else:
            assert groups == cin == cout
            w = self._get(name + '/depthwise_weights', (k, k, cin, 1)).transpose(2, 3, 0, 1)
        p = dict(w=np.ascontiguousarray(w))
        if bn:
            for key, var in (('gamma', 'gamma'), ('beta', 'beta'), ('mean', 'moving_mean'), ('var', 'moving_variance')):
                p[key] = self._get(f'{name}/BatchNorm/{var}', (cout,))
        else:
            p['bias'] = self._get(name + '/biases', (cout,))
        return p


class SSDMobileNetV1(SSD):
    ENGINE_PATH = Path(__file__).parent / 'ssd_mobilenet_v1_coco.hipnet'
    MODEL_PATH = Path(__file__).parent / 'ssd_mobilenet_v1_coco.pb'
    NUM_CLASSES = 91
    INPUT_SHAPE = (3, 300, 300)
    OUTPUT_NAME = 'NMS'
    NMS_THRESH = 0.5
    TOPK = 100
    # ssd_mobilenet_v1_coco.config / the plugin parameters of the reference (models/ssd.py:125-150)
    DEPTH_MULTIPLIER = 1.0
    MIN_DEPTH = 16
    ANCHOR_MIN_SCALE = 0.2
    ANCHOR_MAX_SCALE = 0.95
    ASPECT_RATIOS = (1.0, 2.0, 0.5, 3.0, 0.33)
    BOX_SCALES = (10., 10., 5., 5.)         # 1 / variance of GridAnchor_TRT: (y, x, h, w)
    BN_EPS = 1e-3

    FEATURE_EXTRACTOR = 'FeatureExtractor/MobilenetV1'
    BLOCKS = ((64, 1), (128, 2), (128, 1), (256, 2), (256, 1), (512, 2), (512, 1), (512, 1), (512, 1), (512, 1), (512, 1),
              (1024, 2), (1024, 1))          # (cout, stride) of Conv2d_1 .. Conv2d_13
    FEATURE_BLOCKS = (11, 13)                # Conv2d_11_pointwise, Conv2d_13_pointwise
    EXTRA_DEPTHS = (512, 256, 256, 128)      # Conv2d_13_pointwise_2_Conv2d_{2..5}_3x3_s2_{depth}; the 1x1 before it has depth / 2

    @classmethod
    def depth(cls, d):
        return max(int(d * cls.DEPTH_MULTIPLIER), cls.MIN_DEPTH)

    # ---- the one table of TF variable scopes
    @classmethod
    def scopes(cls):
        """-> dict(stem, blocks [(depthwise scope, pointwise scope)], extras [(1x1 scope, 3x3 scope)], predictors
        [(box scope, class scope)])"""
        fe = cls.FEATURE_EXTRACTOR
        extras = []
        for i, d in enumerate(cls.EXTRA_DEPTHS, start=2):
            extras.append((f'{fe}/Conv2d_13_pointwise_1_Conv2d_{i}_1x1_{cls.depth(d // 2)}',
                           f'{fe}/Conv2d_13_pointwise_2_Conv2d_{i}_3x3_s2_{cls.depth(d)}'))
        n_maps = len(cls.FEATURE_BLOCKS) + len(cls.EXTRA_DEPTHS)
        return dict(stem=f'{fe}/Conv2d_0',
                    blocks=[(f'{fe}/Conv2d_{i}_depthwise', f'{fe}/Conv2d_{i}_pointwise') for i in range(1, len(cls.BLOCKS) + 1)],
                    extras=extras,
                    predictors=[(f'BoxPredictor_{k}/BoxEncodingPredictor', f'BoxPredictor_{k}/ClassPredictor') for k in range(n_maps)])

    @classmethod
    def variable_shapes(cls):
        """{TF variable name: shape} of everything build_graph reads (the name table, spelled out)."""
        out = {}

        def conv(scope, k, cin, cout, bn=True, depthwise=False):
            out[scope + ('/depthwise_weights' if depthwise else '/weights')] = (k, k, cin, 1 if depthwise else cout)
            if bn:
                for v in ('gamma', 'beta', 'moving_mean', 'moving_variance'):
                    out[f'{scope}/BatchNorm/{v}'] = (cout,)
            else:
                out[scope + '/biases'] = (cout,)
        sc = cls.scopes()
        c = cls.depth(32)
        conv(sc['stem'], 3, cls.INPUT_SHAPE[0], c)
        feats = []
        for i, ((dw, pw), (cout, _)) in enumerate(zip(sc['blocks'], cls.BLOCKS), start=1):
            conv(dw, 3, c, c, depthwise=True)
            conv(pw, 1, c, cls.depth(cout))
            c = cls.depth(cout)
            if i in cls.FEATURE_BLOCKS:
                feats.append(c)
        for (s1, s3), d in zip(sc['extras'], cls.EXTRA_DEPTHS):
            conv(s1, 1, c, cls.depth(d // 2))
            conv(s3, 3, cls.depth(d // 2), cls.depth(d))
            c = cls.depth(d)
            feats.append(c)
        for k, ((box, cl), c) in enumerate(zip(sc['predictors'], feats)):
            conv(box, 1, c, cls.anchors_per_cell(k) * 4, bn=False)
            conv(cl, 1, c, cls.anchors_per_cell(k) * cls.NUM_CLASSES, bn=False)
        return out

    # ---- anchors
    @classmethod
    def anchors_per_cell(cls, k):
        return 3 if k == 0 else len(cls.ASPECT_RATIOS) + 1

    @classmethod
    def feature_map_shapes(cls):
        """[(h, w)] of the six feature maps: TF SAME arithmetic, ceil(in / 2) per stride-2 layer."""
        h, w = (-(-v // 2) for v in cls.INPUT_SHAPE[1:])
        shapes = []
        for i, (_, stride) in enumerate(cls.BLOCKS, start=1):
            h, w = -(-h // stride), -(-w // stride)
            if i in cls.FEATURE_BLOCKS:
                shapes.append((h, w))
        for _ in cls.EXTRA_DEPTHS:
            h, w = -(-h // 2), -(-w // 2)
            shapes.append((h, w))
        return shapes

    @classmethod
    def anchors(cls):
        """-> float32 [n, 4] (cy, cx, h, w) in image fractions, order (map, row, column, anchor): create_ssd_anchors with
        reduce_boxes_in_lowest_layer, evaluated in float64."""
        shapes = cls.feature_map_shapes()
        n = len(shapes)
        lo, hi = cls.ANCHOR_MIN_SCALE, cls.ANCHOR_MAX_SCALE
        scales = [lo + (hi - lo) * i / (n - 1) for i in range(n)] + [1.0]
        rows = []
        for k, (fh, fw) in enumerate(shapes):
            if k == 0:
                spec = [(0.1, 1.0), (scales[0], 2.0), (scales[0], 0.5)]
            else:
                spec = [(scales[k], r) for r in cls.ASPECT_RATIOS] + [(math.sqrt(scales[k] * scales[k + 1]), 1.0)]
            assert len(spec) == cls.anchors_per_cell(k)
            hw = np.array([(s / math.sqrt(r), s * math.sqrt(r)) for s, r in spec], np.float64)
            cy, cx = np.meshgrid((np.arange(fh) + 0.5) / fh, (np.arange(fw) + 0.5) / fw, indexing='ij')
            a = np.empty((fh, fw, len(spec), 4), np.float64)
            a[..., 0], a[..., 1] = cy[..., None], cx[..., None]
            a[..., 2:] = hw
            rows.append(a.reshape(-1, 4))
        return np.concatenate(rows).astype(np.float32)

    # ---- weights
    @classmethod
    def weight_source(cls, weights):
        """weights: a weight source object (has `.conv`), a mapping of TF variable names, a path to an .npz of one or to a
        frozen .pb; None: MODEL_PATH if it exists, else the seeded random source when that was opted into."""
        if weights is None:
            if cls.MODEL_PATH is not None and Path(cls.MODEL_PATH).is_file():
                weights = cls.MODEL_PATH
            else:
                return missing_weights(cls, seed=0)
        if hasattr(weights, 'conv'):
            return weights
        if isinstance(weights, (str, Path)):
            path = Path(weights)
            if path.suffix == '.npz':
                with np.load(path) as z:
                    weights = {k: z[k] for k in z.files}
            else:
                from .tf_graph_reader import read_constants
                weights = read_constants(path)
        elif isinstance(weights, (bytes, bytearray, memoryview)):
            from .tf_graph_reader import read_constants
            weights = read_constants(weights)
        return TFWeights(weights)

    @classmethod
    def build_graph(cls, weights=None, max_batch=1):
        """-> (Graph, [head views]): one fp32 head tensor per feature map, channels [A * 4 box | A * NUM_CLASSES class],
        anchor-major within each part (the order of `anchors()`).  max_batch: the batch the caller will instantiate the
        table at (the number of tiles; kept on the graph as `max_batch`)."""
        src = cls.weight_source(weights)
        sc = cls.scopes()
        g = Graph(src, cls.INPUT_SHAPE[1:], cls.INPUT_SHAPE[0])
        g.max_batch = max_batch

        def folded(scope, cout, cin, k, groups=1):
            return fold_bn(src.conv(scope, cout, cin, k, bn=True, groups=groups), eps=cls.BN_EPS)

        x = g.conv(sc['stem'], g.input, cls.depth(32), 3, 2, 'relu6', same=True, wb=folded(sc['stem'], cls.depth(32), cls.INPUT_SHAPE[0], 3))
        feats = []
        for i, ((dw, pw), (cout, stride)) in enumerate(zip(sc['blocks'], cls.BLOCKS), start=1):
            cout = cls.depth(cout)
            wb_dw = folded(dw, x.c, x.c, 3, groups=x.c)
            x = g.sepconv(dw, pw, x, cout, stride, 'relu6', wb_dw=wb_dw, wb_pw=folded(pw, cout, x.c, 1))
            if i in cls.FEATURE_BLOCKS:
                feats.append(x)
        for (s1, s3), d in zip(sc['extras'], cls.EXTRA_DEPTHS):
            mid, cout = cls.depth(d // 2), cls.depth(d)
            y = g.conv(s1, x, mid, 1, 1, 'relu6', wb=folded(s1, mid, x.c, 1))
            x = g.conv(s3, y, cout, 3, 2, 'relu6', same=True, wb=folded(s3, cout, mid, 3))
            feats.append(x)
        assert [(f.h, f.w) for f in feats] == cls.feature_map_shapes()
        heads = []
        for k, ((box, cl), f) in enumerate(zip(sc['predictors'], feats)):
            a = cls.anchors_per_cell(k)
            pb = src.conv(box, a * 4, f.c, 1, bn=False)
            pc = src.conv(cl, a * cls.NUM_CLASSES, f.c, 1, bn=False)
            w = np.concatenate([pb['w'], pc['w']]).astype(np.float32)
            b = np.concatenate([pb['bias'], pc['bias']]).astype(np.float32)
            heads.append(g.conv(f'BoxPredictor_{k}', f, w.shape[0], 1, 1, 'linear', f32_out=True, wb=(w, b)))
        g.outputs = list(heads)
        g.check_fusions()
        return g, heads


class SSDMobileNetV2(SSD):
    ENGINE_PATH = Path(__file__).parent / 'ssd_mobilenet_v2_coco.hipnet'
    MODEL_PATH = Path(__file__).parent / 'ssd_mobilenet_v2_coco.pb'
    NUM_CLASSES = 91
    INPUT_SHAPE = (3, 300, 300)
    OUTPUT_NAME = 'NMS'
    NMS_THRESH = 0.5
    TOPK = 100


class SSDInceptionV2(SSD):
    ENGINE_PATH = Path(__file__).parent / 'ssd_inception_v2_coco.hipnet'
    MODEL_PATH = Path(__file__).parent / 'ssd_inception_v2_coco.pb'
    NUM_CLASSES = 91
    INPUT_SHAPE = (3, 300, 300)
    OUTPUT_NAME = 'NMS'
    NMS_THRESH = 0.5
    TOPK = 100
