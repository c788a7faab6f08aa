"""The per-layer, per-element bound of tests/torch_ref.run_layer checked against itself on
the host: it has to hold for a correct implementation and it has to FAIL for the mistakes kernels actually make.

The stand-in for the device is torch_ref itself in fp32 with channels-last convolutions (another kernel and another
summation order than the float64 reference) and every activation rounded to fp16 where the engine rounds it.

  * clean: on the YOLOv4-CSP @ 640 table (full size), the YOLOv4-P6 table at 320 x 320 (three-stage stem, OP_CONV),
    OSNet-x0.25 and OSNet-x1.0 (batch 2) every layer of the stand-in stays within the bound, and every op class of
    the five full-size benchmark tables occurs in one of them.
    Head-room: the bound's store term is u16 = 2^-11, the worst relative error of ONE correctly rounded fp16 store,
    which a correct layer reaches at the bottom of a binade -- its ratio err / bound is therefore just below 1 on any
    large map (observed 0.87 .. 0.99) and cannot be asked to stay below 0.6.  What can: against the same bound with a
    store term of one whole fp16 ulp (2^-10) a plain conv layer has to stay <= 0.6 (observed 0.49: the half ulp), so
    that arithmetic terms which silently grew past the store term are noticed.
  * mutations, each planted in the stand-in of one layer of each conv-like op class and each required to exceed the
    bound: (a) the last 32 output channels lose 8 input channels of the bottom filter row; (b) zero padding replaced by
    edge replication on the top border; (c) the last output row computed from the row above; (d) the activation between
    two fused stages skipped on one intermediate channel; (e) a residual added on the other side of the activation;
    (f) SPP slices written in the order (5, 9, 13).  For (a) the factor by which the whole-tensor bar of
    test_fullsize_gpu.py (6e-3 * max|ref| + 2e-3) is exceeded is printed next to the per-element one.
  * at the shapes of the unit tests (tests/conv_cases.py, every plain conv table of tests/test_conv_gpu.py with the same
    seeds): the clean stand-in stays within the bound, and one 16-byte chunk of one tap lost by the last output channel
    exceeds it -- at the largest K of that file, 4608, by 1.5x, where that file's whole-tensor bar passes it at 0.39.
  * the sentinel check of tests/layer_check.py refuses a store past the written channels, one into the sample behind the
    batch and a non-finite value (host memory in place of the device's).

A kernel author who nearly made some other mistake adds it to MUTATIONS."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_cases
import layer_check
import torch_ref as T
from fastmot_amd.models import YOLO, ReID
from fastmot_amd.models import graph as G
from fastmot_amd.models.graph import RandomWeights

PLAIN = ('OP_CONV', 'OP_CONVS', 'OP_CONVD', 'OP_STEMCONV')
REL, ABS = 6e-3, 2e-3                    # the whole-tensor bar of tests/test_fullsize_gpu.py


def _op_class(d):
    name = T.OP_NAMES[d['op']]
    return name + '/3' if 'stem3_ref' in d else name


def _tables():
    """name -> (graph, input)"""
    rng = np.random.default_rng(5)
    out = {}
    g, _ = YOLO.get_model('YOLOv4CSP_640').build_graph(RandomWeights(seed=31))
    out['YOLOv4CSP_640'] = (g, torch.from_numpy(rng.uniform(0, 1, (1, 3, 640, 640)).astype(np.float32)))

    class Quarter(YOLO.get_model('YOLOv4P6_1280')):
        INPUT_SHAPE = (3, 320, 320)
        MODEL_PATH = None
    g, _ = Quarter.build_graph(RandomWeights(seed=32))
    out['YOLOv4P6 @ 320'] = (g, torch.from_numpy(rng.uniform(0, 1, (1, 3, 320, 320)).astype(np.float32)))
    for name in ('OSNet025', 'OSNet10'):
        g, _ = ReID.get_model(name).build_graph(RandomWeights(seed=41))
        out[name] = (g, torch.from_numpy(rng.normal(0, 1, (2, 3, 256, 128)).astype(np.float32)))
    return out


# ---------------------------------------------------------------------------------------------- mutations
def _stages(graph, idx, bufs):
    """Dry run of the stand-in: per conv stage (weight shape, padding, residual mode, activation is not the identity)."""
    rec = {}

    def mut(point, stage, *a):
        r = rec.setdefault(stage, {})
        if point == 'w':
            r['w'] = tuple(a[0].shape)
        elif point == 'x':
            r['pad'] = a[0][1]
        elif point == 'res_mode':
            r['res'] = a[0]
        elif point == 'act':
            r['act'] = not torch.equal(a[0], a[1])
        return a[0]
    T.run_layer(graph, idx, bufs, dtype=torch.float32, emulate_fp16_storage=True, channels_last=True, mut=mut)
    return [rec[s] for s in sorted(rec)]


def _at(stage, point, fn):
    def mut(p, s, *a):
        return fn(*a) if (p, s) == (point, stage) else a[0]
    return mut


def _drop_taps(w):
    w = w.clone()
    w[-32:, :8, -1, :] = 0
    return w


def _replicate_top(xp):
    x, p = xp
    x = F.pad(x, (p, p, 0, p))
    return torch.cat([x[:, :, :1]] * p + [x], dim=2), 0


def _last_row_from_above(y):
    y = y.clone()
    y[:, :, -1] = y[:, :, -2]
    return y


def _skip_act_on_channel0(post, pre):
    post = post.clone()
    post[:, 0] = pre[:, 0]
    return post


def _mutations(d, st):
    """{letter: mut} of the mutations that apply to this layer."""
    out = {}
    if d['op'] == G.OP_LITECHAIN:      # (b), (c) in the one-level stream: the bound of the deeper ones has widened stage by stage
        full, st = st, st[:2]
    last = len(st) - 1
    dense = [i for i, s in enumerate(st) if s['w'][1] >= 3]                  # (not the depthwise stages)
    if dense:
        a = max(dense, key=lambda i: int(np.prod(st[i]['w'][1:])))
        out['a'] = _at(a, 'w', _drop_taps)
    padded = [i for i, s in enumerate(st) if s['pad'] > 0]
    if padded:
        out['b'] = _at(padded[-1], 'x', _replicate_top)
    out['c'] = _at(last, 'y', _last_row_from_above)
    if d['op'] == G.OP_LITECHAIN:
        st = full
    inner = [i for i, s in enumerate(st[:-1]) if s['act'] and (d['op'] != G.OP_LITECHAIN or i == 3)]
    if inner and d['op'] in (G.OP_RESBLOCK, G.OP_PAIR11, G.OP_STEM2, G.OP_LITECHAIN):
        out['d'] = _at(inner[0], 'act', _skip_act_on_channel0)
    res = [i for i, s in enumerate(st) if s['res'] != G.RES_NONE]
    if res:
        out['e'] = _at(res[0], 'res_mode', lambda m: G.RES_BEFORE_ACT if m == G.RES_AFTER_ACT else G.RES_AFTER_ACT)
    return out


CONV_LIKE = PLAIN + ('OP_RESBLOCK', 'OP_PAIR11', 'OP_STEM2', 'OP_STEM2/3', 'OP_LITECONV', 'OP_LITECHAIN')
# what has to have been planted (and caught) by the end: every conv-like class with every mutation that exists for it
# (1x1-only ops have no padding; OP_LITECONV's only activation is the last one; residuals: the fused unit and the
# shortcut / OSNet block-tail epilogues of the two DMA-fed and streamed kernels)
MUTATIONS = {c: {'a', 'c'} for c in CONV_LIKE}
for _c in ('OP_CONV', 'OP_CONVS', 'OP_CONVD', 'OP_STEMCONV', 'OP_RESBLOCK', 'OP_STEM2', 'OP_STEM2/3', 'OP_LITECONV', 'OP_LITECHAIN'):
    MUTATIONS[_c].add('b')
for _c in ('OP_RESBLOCK', 'OP_PAIR11', 'OP_STEM2', 'OP_STEM2/3', 'OP_LITECHAIN'):
    MUTATIONS[_c].add('d')
for _c in ('OP_RESBLOCK', 'OP_CONVD', 'OP_CONVS'):
    MUTATIONS[_c].add('e')
MUTATIONS['OP_SPP'] = {'f'}


def _exceeds(got, ref, bound):
    err = (got.double() - ref).abs()
    return float(torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max())


@pytest.fixture(scope='module')
def walked():
    """One walk over the four tables: clean ratios per (table, op class) and the mutation results."""
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    clean, plain_ulp, planted, seen = {}, {}, {}, set()
    for tname, (g, x) in _tables().items():
        gates = {}

        def around(i, bufs, g=g, tname=tname, gates=gates):
            d = g.layers[i]
            cls = _op_class(d)
            seen.add(cls)
            kind, ref, bound = T.run_layer(g, i, bufs, gates=gates)
            if kind == 'gate':
                return None
            what = f'{tname} layer {i} {cls}'
            bound_ulp = T.run_layer(g, i, bufs, u16=2 * T.U16)[2] if cls in PLAIN else None
            todo = MUTATIONS.get(cls, set()) - set(planted.get(cls, {}))
            if todo and kind == 'tensor':
                muts = {'f': _at(0, 'spp_order', lambda o: o[::-1])} if cls == 'OP_SPP' else _mutations(d, _stages(g, i, bufs))
                base = None
                for letter in sorted(todo & set(muts)):
                    got = T.run_layer(g, i, bufs, dtype=torch.float32, emulate_fp16_storage=True, channels_last=True,
                                      mut=muts[letter])[1]
                    entry = dict(where=what, ratio=_exceeds(got, ref, bound))
                    if letter == 'a':
                        if base is None:
                            base = T.run_layer(g, i, bufs, dtype=torch.float32, emulate_fp16_storage=True, channels_last=True)[1]
                        entry['old_bar'] = float((got - base).abs().max() / (REL * base.abs().max() + ABS))
                    planted.setdefault(cls, {})[letter] = entry

            def after(bufs, emb):
                o = d['out']
                got = emb if kind == 'emb' else bufs[o.tid][:, o.coff:o.coff + o.c]
                r = T.check_layer(got, ref, bound, what)
                clean[(tname, cls)] = max(clean.get((tname, cls), 0.0), r)
                if bound_ulp is not None:
                    plain_ulp[(tname, cls)] = max(plain_ulp.get((tname, cls), 0.0), T.check_layer(got, ref, bound_ulp, what))
            return after
        T.run_graph(g, x, channels_last=True, around=around)
    return dict(clean=clean, plain_ulp=plain_ulp, planted=planted, seen=seen)


def test_every_op_class_of_the_benchmark_tables_is_walked(walked):
    need = set()
    for name in ('YOLOv4_608', 'YOLOv4CSP_640', 'YOLOv4P6_1280'):
        need |= {_op_class(d) for d in YOLO.get_model(name).build_graph(RandomWeights(seed=1))[0].layers}
    for name in ('OSNet025', 'OSNet10'):
        need |= {_op_class(d) for d in ReID.get_model(name).build_graph(RandomWeights(seed=1))[0].layers}
    assert need <= walked['seen'], need - walked['seen']


def test_clean_stand_in_stays_within_the_bound(walked):
    """(check_layer has already asserted ratio <= 1 for every layer of every table while walking.)"""
    for key, r in sorted(walked['clean'].items()):
        print(f'{key[0]:16s} {key[1]:14s} worst err / bound {r:.3g}')
        assert r <= 1.0
    for key, r in sorted(walked['plain_ulp'].items()):
        print(f'{key[0]:16s} {key[1]:14s} worst err / bound(store term 2^-10) {r:.3g}')
        assert r <= 0.6, key
    # the bound is not vacuous where it is meant to bite: a correctly rounded store alone reaches most of it
    assert min(r for (t, c), r in walked['clean'].items() if c in PLAIN) >= 0.5


def _lose_a_chunk(w):
    """The last output channel loses the first min(8, cin) input channels of the bottom-right tap: one 16-byte chunk of
    the weight image, what a DMA-fed kernel drops when it miscounts the chunks of a pixel."""
    w = w.clone()
    w[-1, :min(8, w.shape[1]), -1, -1] = 0
    return w


@pytest.mark.parametrize('kind,case', conv_cases.PLAIN_CASES, ids=[f'{k}-' + '-'.join(map(str, c)) for k, c in conv_cases.PLAIN_CASES])
def test_bound_bites_at_the_unit_test_shapes(kind, case):
    """Every plain conv shape of tests/test_conv_gpu.py (conv_cases: the same one-layer table, the same seeds): (a) the
    clean stand-in stays within the bound, (b) the stand-in with one lost chunk exceeds it.  Printed beside (b), recorded
    only: the same defect against that file's whole-tensor bar, max err / (2e-2 * max|ref| + 2e-3)."""
    g, x, idx = conv_cases.table(kind, case)
    seen = {}

    def around(i, bufs):
        if i != idx:
            return None
        _, ref, bound = T.run_layer(g, i, bufs)
        bad = T.run_layer(g, i, bufs, dtype=torch.float32, emulate_fp16_storage=True, channels_last=True, mut=_at(0, 'w', _lose_a_chunk))[1]
        seen.update(defect=_exceeds(bad, ref, bound),
                    close=float((bad.double() - ref).abs().max() / (2e-2 * ref.abs().max() + 2e-3)))

        def after(bufs, emb):
            o = g.layers[i]['out']
            seen['clean'] = T.check_layer(bufs[o.tid][:, o.coff:o.coff + o.c], ref, bound, f'clean stand-in, {kind} {case}')
        return after
    T.run_graph(g, conv_cases.nchw(x), channels_last=True, around=around)
    print(f"{kind} {case}: clean err / bound {seen['clean']:.3g}; one lost chunk: err / bound {seen['defect']:.4g}, "
          f"err / whole-tensor bar {seen['close']:.3g}")
    assert seen['clean'] <= 1.0, (kind, case, seen)
    assert seen['defect'] > 1.0, (kind, case, seen)
    assert np.isfinite(seen['close']), (kind, case, seen)


class _HostNet:
    """What layer_check's sentinel functions use of a HipNet, with host memory behind the library's raw tensor write."""

    def __init__(self, graph, max_batch):
        self.graph, self.max_batch, self.which, self.mem = graph, max_batch, 0, {}
        self.ctx = SimpleNamespace(handle=None, lib=self)

    def fm_net_tensor_write(self, handle, which, tid, host, nbytes):
        h, w, c, f32 = self.graph.tensors[tid.value]
        a = np.frombuffer(ctypes.string_at(host, nbytes.value), np.float32 if f32 else np.float16)
        self.mem[tid.value] = a.reshape(-1, h, w, c).copy()
        return 0

    def read(self, view, batch):
        return self.mem[view.tid][:batch, ..., view.coff:view.coff + view.c].astype(np.float32)


@pytest.mark.parametrize('f32', [False, True])
def test_sentinel_check_fails_for_the_overruns_it_is_there_for(f32):
    """20 channels written at offset 16 of a 48-channel tensor, batch 2 of 3: the ceil8 padding [36, 40) may be stored;
    a store one channel past it, a store into sample 2 and a non-finite value in the slice are each refused."""
    g = G.Graph(RandomWeights(seed=1), (4, 3), 16)
    wide = g.new(4, 3, 48, f32=f32)
    g.conv('c', g.input, 20, 1, 1, 'linear', dst=wide.slice(16, 20), f32_out=f32)
    net = _HostNet(g, 3)
    layer_check.fill_sentinel(net)
    filled = net.mem[wide.tid].copy()
    assert filled.shape == (3, 4, 3, 48) and np.isfinite(filled).all()
    with pytest.raises(AssertionError, match='outside the written channels'):
        net.mem[wide.tid][:2, ..., 16:40] = 1.0
        net.mem[wide.tid][1, 3, 2, 40] = 0.0
        layer_check.check_sentinel(net, 2, 'one channel too far')
    net.mem[wide.tid][1, 3, 2, 40] = filled[1, 3, 2, 40]
    layer_check.check_sentinel(net, 2, 'clean')
    net.mem[wide.tid][2, 0, 0, 16] = 1.0
    with pytest.raises(AssertionError, match='beyond batch 2'):
        layer_check.check_sentinel(net, 2, 'into the next sample')
    net.mem[wide.tid][2, 0, 0, 16] = filled[2, 0, 0, 16]
    net.mem[wide.tid][0, 0, 0, 17] = np.inf
    with pytest.raises(AssertionError, match='non-finite'):
        layer_check.check_sentinel(net, 2, 'overflow')


@pytest.mark.parametrize('cls,letter', sorted((c, m) for c, ms in MUTATIONS.items() for m in ms))
def test_mutation_exceeds_the_bound(walked, cls, letter):
    entry = walked['planted'].get(cls, {}).get(letter)
    assert entry is not None, f'mutation ({letter}) was never planted in an {cls} layer'
    print(f"({letter}) in {entry['where']}: err / bound {entry['ratio']:.4g}" +
          (f", whole-tensor bar exceeded {entry['old_bar']:.3g} times" if 'old_bar' in entry else ''))
    assert entry['ratio'] > 1.0, entry
    if 'old_bar' in entry:           # recorded, not required: how far over the whole-tensor bar the same fault lands
        assert np.isfinite(entry['old_bar']), entry
