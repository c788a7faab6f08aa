"""TEST INFRASTRUCTURE: inputs for the tests of the anchor-head decode (decode_kernel, detect.hip) and of the candidate
sort (sort_key / rank_sort*_kernel, nms_core.h) -- importable without a GPU; tests/test_decode_cases_host.py proves on the
CPU references alone that the inputs have the properties the GPU tests rely on, tests/test_decode_gpu.py and
tests/test_detect_gpu.py assert them again on what the device holds.

Decode.  Tiny YOLOv4 graphs (3 x 96 x 128, strides 8 / 16 / 32, three anchors per head: 576 + 144 + 36 = 756 rows) for
every class count of CLASS_COUNTS in both head forms, with scripted head convolutions (DecodeHeadWeights):
  * the head convolutions draw from a random stream of their own, so the backbone -- and with it the tensors the heads
    read -- is the same for every class count: one CPU pass per form (head_inputs) is all the scripting needs;
  * every row of a head's weight is scaled so that its logit has a chosen spread over the cells, and centred;
  * class logits spread wide enough that for nc <= 7 every class is the maximum somewhere;
  * forced ties: on anchor a < len(tie_pairs(nc)) the classes of pair a share weight and bias, raised until the pair is
    the joint maximum in about a quarter of that anchor's cells -- pairs on both sides of every seam of the class scan
    (four logits per 16-byte load, then a scalar tail);
  * NEW_COORDS: +30 on classes 0 and nc - 1 of anchor 2 of the second head in front of the in-network logistic: both
    saturate to exactly 1.0f in all of its 48 rows, the tie this form produces by itself;
  * box sizes: anchor 1 gets boxes many times the frame (classic: w/h logits + 8; NEW_COORDS: + 6, the head then holds
    0.9975 and the box is four times its anchor), anchor 2 sub-pixel ones (- 8); |logit| stays below about 10."""
import functools

import numpy as np

import np_oracle as o
from fastmot_amd.models import YOLO
from fastmot_amd.models.graph import RandomWeights

SIZE = (320, 180)                   # the frame
CLASS_COUNTS = (1, 3, 4, 5, 6, 7, 80, 128)
FORMS = ('classic', 'new_coords')
N_ROWS = 756
MAX_AREA = 20000                    # (the detectors of the decode tests: ordinary boxes pass, anchor 1's do not)
SEED = 4
SAT_HEAD, SAT_ANCHOR = 1, 2         # where the NEW_COORDS form saturates two classes
# spread over the cells of the logits of a head row: x / y, w / h, objectness, classes
STD_XY, STD_WH, STD_OBJ, STD_CLS = 1.0, 0.4, 2.0, 3.0
OBJ_BIAS = (-1.0, -1.0, 1.0)       # per anchor (anchor 2's objectness runs low where its tied classes peak)
TIE_SHARE = 0.25


def synthetic_frame(w, h, seed=0):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3)).astype(np.uint8)
    frame = np.kron(base, np.ones((8, 8, 1), np.uint8))[:h, :w]
    noise = rng.integers(-20, 20, frame.shape)
    return np.clip(frame.astype(int) + noise, 0, 255).astype(np.uint8)


class DecodeClassic(YOLO):
    NUM_CLASSES = 3
    INPUT_SHAPE = (3, 96, 128)
    LAYER_FACTORS = [8, 16, 32]
    SCALES = [1.2, 1.1, 1.05]
    ANCHORS = [[4, 7, 8, 15, 12, 30], [18, 40, 25, 60, 30, 80], [40, 90, 60, 70, 80, 95]]


class DecodeNewCoords(DecodeClassic):
    LETTERBOX = True
    NEW_COORDS = True
    SCALES = [2.0, 2.0, 2.0]


@functools.lru_cache(maxsize=None)
def model(nc, form):
    """The descriptor of (class count, form), registered under its name: YOLODetector(model=model(nc, form).__name__)."""
    base = {'classic': DecodeClassic, 'new_coords': DecodeNewCoords}[form]
    return type(f'{base.__name__}{nc}', (base,), dict(NUM_CLASSES=nc))


def scan_shape(nc):
    """(iterations of the 4-wide vector loop, length of the scalar tail) of decode_kernel's class scan at nc classes."""
    return nc // 4, nc % 4


def tie_pairs(nc):
    """The forced ties of a class count, pair a on anchor a: within one 4-wide load (1, 2); in two different loads (3, 70);
    the last lane of a load against the first element of the tail (3, 4); inside the tail (4, 5) -- at nc = 3 (1, 2) lies
    in a tail that is the whole scan; the last two lanes of the last load (126, 127).  The second class of a pair is the
    one a comparison gone soft would pick: it sits in the third lane of a load for (1, 2) and (3, 70), in the fourth for
    (126, 127) and the saturated (0, nc - 1); (4, 9) and (7, 8) put it into the second and the first lane as well."""
    return {1: [], 3: [(1, 2)], 4: [(1, 2)], 5: [(1, 2), (3, 4)], 6: [(1, 2), (3, 4), (4, 5)], 7: [(1, 2), (3, 4), (4, 5)],
            80: [(1, 2), (3, 70), (4, 9)], 128: [(1, 2), (126, 127), (7, 8)]}[nc]


def saturated_pair(nc, form):
    return (0, nc - 1) if form == 'new_coords' and nc >= 2 else None


class DecodeHeadWeights(RandomWeights):
    """RandomWeights(seed) for every layer but the YOLO head convolutions (recognised as synthetic.ScriptedHeadWeights does);
    those come from a stream of their own and, given the tensors they read (`head_inputs`, [cells, cin] per head), are
    scripted as the module's docstring says."""

    def __init__(self, seed, nc, form, head_inputs=None):
        super().__init__(seed)
        self.seed, self.nc, self.form, self.head_inputs = seed, nc, form, head_inputs
        self._head = 0

    def conv(self, name, cout, cin, k, bn=True, gain=1.0, groups=1):
        rec = 5 + self.nc
        if bn or cout % rec != 0:
            return super().conv(name, cout, cin, k, bn=bn, gain=gain, groups=groups)
        h, self._head = self._head, self._head + 1
        rng = np.random.default_rng((self.seed, 1000 + h))
        w = rng.normal(0, 1, (cout, cin)).astype(np.float64)
        bias = np.zeros(cout)
        if self.head_inputs is not None:
            self._script(h, w.reshape(-1, rec, cin), bias.reshape(-1, rec), np.asarray(self.head_inputs[h], np.float64))
        return dict(w=w.reshape(cout, cin, 1, 1).astype(np.float32), bias=bias.astype(np.float32))

    def _script(self, h, w, b, x):
        nc, new = self.nc, self.form == 'new_coords'
        pairs = tie_pairs(nc)
        for a in range(len(w)):
            for k in range(w.shape[1]):
                t = x @ w[a, k]
                w[a, k] *= (STD_XY if k < 2 else STD_WH if k < 4 else STD_OBJ if k == 4 else STD_CLS) / t.std()
                b[a, k] = -(x @ w[a, k]).mean()
            b[a, 4] += OBJ_BIAS[a]
            if a == 1:
                b[a, 2:4] += 6.0 if new else 8.0
            if a == 2:
                b[a, 2:4] -= 8.0
            if a < len(pairs):
                i, j = pairs[a]
                w[a, 5 + j], b[a, 5 + j] = w[a, 5 + i], b[a, 5 + i]
                logits = x @ w[a, 5:].T + b[a, 5:]
                rest = np.delete(logits, [i, j], axis=1).max(1)
                b[a, [5 + i, 5 + j]] += np.quantile(rest - logits[:, i], TIE_SHARE)
            sat = saturated_pair(nc, self.form)
            if sat and h == SAT_HEAD and a == SAT_ANCHOR:
                b[a, [5 + sat[0], 5 + sat[1]]] += 30.0


def _roi(m):
    """YOLODetector._create_letterbox's ROI (x, y, w, h) inside the network input, None for a stretched frame."""
    if not m.LETTERBOX:
        return None
    dst, src = np.array(m.INPUT_SHAPE[:0:-1]), np.array(SIZE)
    s = min(dst / src)
    scaled = np.rint(src * s).astype(int)
    off = ((dst - scaled) / 2).astype(int)
    return int(off[0]), int(off[1]), int(scaled[0]), int(scaled[1])


def frame():
    return synthetic_frame(*SIZE, seed=1)


def _run_host(m, weights):
    """-> (graph, head views, tensors of a CPU pass of the frame through the graph with fp16 storage as on the device)"""
    import torch
    import torch_ref
    g, heads = m.build_graph(weights)
    x = o.yolo_preprocess(frame(), m.INPUT_SHAPE[1:], _roi(m))
    bufs, _ = torch_ref.run_graph(g, torch.from_numpy(np.ascontiguousarray(x, np.float32))[None])
    return g, heads, bufs


@functools.lru_cache(maxsize=None)
def head_inputs(form):
    """[cells, cin] per head: what the head convolutions of this form read for the frame (the same for every class count)."""
    m = model(1, form)
    g, heads, bufs = _run_host(m, DecodeHeadWeights(SEED, 1, form))
    out = []
    for hv in heads:
        d, = [d for d in g.layers if d['out'].tid == hv.tid]
        v, = d['ins']
        out.append(bufs[v.tid][0, v.coff:v.coff + v.c].numpy().reshape(v.c, -1).T.astype(np.float64))
    return out


def weights(nc, form):
    return DecodeHeadWeights(SEED, nc, form, head_inputs(form))


def host_heads(nc, form):
    """The head tensors [(5 + nc) * 3, gh, gw] of a CPU pass through the scripted graph."""
    m = model(nc, form)
    _, heads, bufs = _run_host(m, weights(nc, form))
    return [bufs[hv.tid][0, hv.coff:hv.coff + (5 + nc) * 3].numpy() for hv in heads]


def oracle_rows(heads, m):
    """np_oracle.yolo_decode of head tensors [(5 + nc) * 3, gh, gw] -> [756, 7], heads in order, (anchor, cell) inside."""
    return np.concatenate([o.yolo_decode(np.ascontiguousarray(t, np.float32), m.ANCHORS[i], m.NUM_CLASSES,
                                         (m.INPUT_SHAPE[2], m.INPUT_SHAPE[1]), m.SCALES[i], m.NEW_COORDS)
                           for i, t in enumerate(heads)])


def class_logits(heads, nc):
    """[756, nc] class logits (NEW_COORDS: what the head holds) in the row order of oracle_rows."""
    return np.concatenate([t.reshape(3, 5 + nc, -1)[:, 5:].transpose(0, 2, 1).reshape(-1, nc) for t in heads])


def row_anchor():
    """The anchor of each of the 756 rows."""
    return np.concatenate([np.repeat(np.arange(3), c) for c in (192, 48, 12)])


def tie_rows(heads, nc, pair):
    """Rows in which the two classes of `pair` hold equal logits, the maximum of the row, and no class before them does."""
    lg = class_logits(heads, nc)
    return np.flatnonzero((lg[:, pair[0]] == lg[:, pair[1]]) & (lg.argmax(1) == pair[0]))


def gap_threshold(scores, near=0.25):
    """The middle of the widest gap between neighbouring scores among the nine nearest to `near`, and the gap."""
    s = np.sort(np.asarray(scores, np.float64))
    s = s[np.sort(np.argsort(np.abs(s - near))[:9])]
    assert len(s) >= 2
    k = int(np.argmax(np.diff(s)))
    return float((s[k] + s[k + 1]) / 2), float(s[k + 1] - s[k])


SCORE_REL = 5e-6                    # the project's criterion for the decode's rows (oracle/detector_check.py)


def check_preconditions(heads, nc, form):
    """What the decode tests need of head tensors, asserted: -> (threshold in a gap, candidates over it).  Run on the CPU
    pass by the host test and on the device's own tensors by the GPU test."""
    m = model(nc, form)
    rows = oracle_rows(heads, m)
    assert rows.shape == (N_ROWS, 7)
    cls = rows[:, 5].astype(int)
    for a, pair in enumerate(tie_pairs(nc)):
        t = tie_rows(heads, nc, pair)
        assert (row_anchor()[t] == a).sum() >= 10, (nc, form, pair, len(t))
        assert (cls[t] == pair[0]).all()                         # (the oracle's argmax takes the first maximum)
    sat = saturated_pair(nc, form)
    if sat:
        t = tie_rows(heads, nc, sat)
        lg = class_logits(heads, nc)
        assert len(t) == 48 and (lg[t][:, list(sat)] == np.float32(1.0)).all() and (cls[t] == 0).all()
    if nc <= 7:
        assert sorted(set(cls.tolist())) == list(range(nc)), (nc, form, np.bincount(cls, minlength=nc))
    if not m.NEW_COORDS:                                         # (__expf's argument reduction is not strained)
        assert max(np.abs(t.reshape(3, 5 + nc, -1)[:, 2:4]).max() for t in heads) <= 10.0
    score = rows[:, 4] * rows[:, 6]
    thresh, gap = gap_threshold(score)
    assert gap / 2 > 10 * SCORE_REL * thresh, (nc, form, gap)
    over = score >= np.float32(thresh)
    k = int(over.sum())
    assert 20 <= k <= 700, (nc, form, k)
    for pair in tie_pairs(nc) + ([sat] if sat else []):         # tied rows are among the candidates
        assert over[tie_rows(heads, nc, pair)].sum() >= 3, (nc, form, pair)
    if nc >= 3:                                                  # (the class-mask check turns classes 0 and 1 off)
        assert 0 < (over & (cls >= 2)).sum() < k
    return thresh, k


# ------------------------------------------------------------------------------------------- candidate sort
SORT_SIZE = [1920, 1080]
SORT_NMS, SORT_MAX_AREA, SORT_MIN_AR = 0.45, 800000, 0.0
SORT_COUNTS = (1, 7, 8, 9, 255, 256, 257, 513)          # both sort kernels
SORT_COUNTS_LARGE = (4097, 16385, 16448)                # the chunked one alone (capacity 16448)
SORT_SURVIVOR_CAP = 200


@functools.lru_cache(maxsize=None)
def sort_rows(n):
    """n rows for fm_filter_dets at conf_thresh 0 (every row is a candidate): three classes, boxes in 8 tight clusters as
    test_detect_gpu._seam_case; box_conf a multiple of 1/16, so most values repeat within their class and the original
    index decides the order; one row in eight with box_conf < 0 and cls_prob < 0 (the product passes), one in sixteen
    with box_conf -0.0 or +0.0.  -> (rows [n, 7] float32, read-only)"""
    rng = np.random.default_rng(1000 + n)
    centres = rng.uniform(0.1, 0.8, (8, 2))
    pick = rng.integers(0, 8, n)
    conf = rng.integers(1, 17, n) / 16.0
    prob = rng.uniform(0.6, 1, n)
    kind = rng.integers(0, 16, n)
    neg = (kind == 1) | (kind == 2)
    conf[neg], prob[neg] = -conf[neg], -prob[neg]
    conf[kind == 3] = 0.0
    conf[(kind == 3) & (rng.integers(0, 2, n) == 1)] = -0.0
    if n >= 7:                              # (small counts: one of each kind for certain)
        conf[:4], prob[:4] = [-0.5, -0.0, 0.0, -0.5], [-0.7, 0.9, 0.8, -0.9]
    rows = np.stack([centres[pick, 0] + rng.normal(0, 0.004, n), centres[pick, 1] + rng.normal(0, 0.004, n),
                     rng.uniform(0.05, 0.08, n), rng.uniform(0.1, 0.16, n), conf,
                     rng.integers(0, 3, n), prob], 1).astype(np.float32)
    if n >= 7:
        rows[:4, 5] = 1                     # (the four of one class: -0.0 and +0.0 tie there, as do the two -0.5)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def sort_reference(n):
    """-> (candidate rows in sorted order [n, 7] float32, their original indices, oracle detections, NMS survivors)"""
    rows = sort_rows(n)
    d, idx = o.filter_scale(rows, SORT_SIZE, [0, 0], [True] * 3, 0.0)
    assert len(d) == n                      # every row is a candidate
    order = np.lexsort((idx, -d[:, 4], d[:, 5]))
    survivors = sum(len(o.diou_nms(d[d[:, 5] == c, :4], d[d[:, 5] == c, 4], SORT_NMS)) for c in np.unique(d[:, 5]))
    ref = o.nms_finalize(d, SORT_NMS, SORT_MAX_AREA, SORT_MIN_AR, tie_rank=idx)
    return d[order], idx[order], ref, survivors
