"""Every layer of a finished device run against tests/torch_ref.run_layer (float64, teacher-forced: each layer is fed the
tensors THE DEVICE produced for its inputs) under the derived per-element bound of DESIGN.md section 7, and a sentinel
check that a run changes nothing outside the channels its layers write and nothing beyond its batch.

    fill_sentinel(net)                      # optional, before the first run
    net.write(...); net.run(batch)
    ratios = check_net(net, batch, label)   # {op class: worst err / bound}; asserts <= 1 for every element
    check_sentinel(net, batch, label)

Tables in which a layer overwrites channels an earlier one wrote (torch_ref.clobbers: the merged CSP stages) need the
state before the overwrite from runs of the table cut there, and those need the network slot: read_run(net) -> net.close()
-> clobber_snapshots(...) -> check_layers(...); run_and_check does all of it from (ctx, which, graph, batch, input).
The network has private buffers (reuse_buffers=False): every tensor is read back."""
import copy
import ctypes as C

import numpy as np
import torch

import torch_ref
from fastmot_amd import _lib
from fastmot_amd.engine import HipNet, NET_DETECTOR
from fastmot_amd.models.graph import View, ceil_to

# values no layer of a test network produces (inputs and weights are O(1)): fp16 bits 0xF5A5, and an fp32 number that
# no fp16 holds.  Finite, so that a layer which reads never-written channels under zero weights still gets 0.
SENT16 = np.uint16(0xF5A5).view(np.float16)      # -23120.0
SENT32 = np.float32(-23120.5)


def _whole(g, tid):
    """View of a whole tensor (all stored channels)."""
    h, w, c, _ = g.tensors[tid]
    return View(tid, 0, c, h, w)


def _device_tensors(net, g, batch, tids=None):
    """tid -> torch view [N, cpad, h, w] of what the device holds (fp16 tensors stay fp16: lossless, half the host memory)."""
    out = {}
    for tid, (h, w, c, f32) in enumerate(g.tensors):
        if tids is None or tid in tids:
            a = net.read(_whole(g, tid), batch)
            out[tid] = torch.from_numpy(a if f32 else a.astype(np.float16)).permute(0, 3, 1, 2)
    return out


class _Forced:
    """The tensors layer `i` of a finished run saw: the final state, except for tensors a later layer overwrote in place
    (torch_ref.clobbers: the merged CSP stages) -- those come from a run of the table cut before the overwriting layer."""

    def __init__(self, final, snaps):
        self.final, self.snaps, self.i = final, snaps, 0       # snaps: [(layer index L, tid, tensor before layer L ran)]

    def __getitem__(self, tid):
        later = [(L, t) for L, st, t in self.snaps if st == tid and L > self.i]
        return min(later, key=lambda p: p[0])[1] if later else self.final[tid]


def _has_emb(which, g):
    return which != NET_DETECTOR and any(d['op'] in (torch_ref.G.OP_HEAD, torch_ref.G.OP_OSTAIL) for d in g.layers)


def _assert_private(net):
    """No two tensors share bytes (Graph.plan_arena without reuse places them one behind the other)."""
    g = net.graph
    each = sum(ceil_to(net.max_batch * h * w * c * (4 if f32 else 2), 256) for h, w, c, f32 in g.tensors)
    assert g.arena_bytes == each, 'the network shares activation memory between tensors: create it with reuse_buffers=False'


def read_run(net, batch):
    """-> (every tensor of the finished run, its embeddings / None)."""
    g = net.graph
    _assert_private(net)
    return _device_tensors(net, g, batch), (net.read_embeddings(batch) if _has_emb(net.which, g) else None)


def clobber_snapshots(ctx, which, g, x, batch):
    """[(L, tid, tensor `tid` before layer L ran)] for torch_ref.clobbers(g), each from a run of the table cut before L
    (the network slot `which` must be free)."""
    snaps = []
    for L, tid in torch_ref.clobbers(g):
        cut = copy.copy(g)
        cut.layers = g.layers[:L]
        net = HipNet(ctx, which, cut, batch, reuse_buffers=False)
        net.write(g.input, x)
        net.run(batch)
        snaps.append((L, tid, _device_tensors(net, g, batch, {tid})[tid]))
        net.close()
    return snaps


def check_layers(g, final, snaps, emb, label, keep=None):
    """Layer by layer on the device's own inputs, per-element bound -> {op class: worst err / bound}.
    keep: a dict that receives {layer index: (ref, bound)}."""
    forced, gates, ratios = _Forced(final, snaps), {}, {}
    for i, d in enumerate(g.layers):
        forced.i = i
        kind, ref, bound = torch_ref.run_layer(g, i, forced, gates=gates)
        if kind == 'gate':
            continue
        o = d['out']
        got = emb if kind == 'emb' else forced[o.tid][:, o.coff:o.coff + o.c]
        op = torch_ref.OP_NAMES[d['op']] + ('/3' if 'stem3_ref' in d else '')
        r = torch_ref.check_layer(got, ref, bound, f'{label} layer {i} {op} {d.get("name", "")} k{d["k"]} s{d["stride"]} '
                                                   f'cin {d["cin"]} cout {d["cout"]}')
        ratios[op] = max(ratios.get(op, 0.0), r)
        if keep is not None:
            keep[i] = (ref, bound)
    for op, r in sorted(ratios.items()):
        print(f'LAYERBOUND {label:24s} {op:14s} worst err/bound {r:.3g}')
    return ratios


def check_net(net, batch, label, keep=None):
    """check_layers on an already-run HipNet whose table overwrites nothing in place.
    keep: also receives keep['final'], the device's tensors."""
    g = net.graph
    assert not torch_ref.clobbers(g), 'a layer overwrites an earlier one: read_run / clobber_snapshots / check_layers'
    final, emb = read_run(net, batch)
    if keep is not None:
        keep['final'] = final
    return check_layers(g, final, [], emb, label, keep)


def close_and_check(net, batch, x, label, sentinel=False):
    """check_layers on an already-run HipNet of ANY table: reads the run, closes the network (the snapshot runs of
    torch_ref.clobbers need its slot; x: the input it ran on) and checks every layer.
    sentinel: the network was prepared with fill_sentinel -- check_sentinel before it closes."""
    g = net.graph
    final, emb = read_run(net, batch)
    if sentinel:
        check_sentinel(net, batch, label)
    net.close()
    return check_layers(g, final, clobber_snapshots(net.ctx, net.which, g, x, batch), emb, label)


def run_and_check(ctx, which, g, batch, x, label):
    """A private-buffer network of `g` run on x ([batch, h, w, c] fp16): every layer checked, and the sentinel."""
    net = HipNet(ctx, which, g, batch, reuse_buffers=False)
    fill_sentinel(net)
    net.write(g.input, x)
    net.run(batch)
    return close_and_check(net, batch, x, label, sentinel=True)


# ------------------------------------------------------------------------------------------------ untouched memory
def write_raw(net, tid, full):
    """Whole samples of tensor `tid` as stored (NHWC, all padded channels, fp16 or fp32): HipNet.write zero-pads and refuses
    fp32 tensors; the library call copies bytes and checks only the size."""
    h, w, c, f32 = net.graph.tensors[tid]
    full = np.ascontiguousarray(full)
    assert full.shape[1:] == (h, w, c) and full.dtype == (np.float32 if f32 else np.float16) and full.shape[0] <= net.max_batch
    _lib.check(net.ctx.lib.fm_net_tensor_write(net.ctx.handle, C.c_int(net.which), C.c_int(tid),
                                               full.ctypes.data_as(C.c_void_p), C.c_size_t(full.nbytes)))


def _written(g):
    """tid -> channel mask of what the layers may store: the union of [coff, coff + ceil8(c)) over their `out` views (the
    conv kernels store ceil8(cout) channels, the padding ones from zero weights and zero bias)."""
    out = {}
    for d in g.layers:
        o = d.get('out')
        if o is not None and o.tid != g.input.tid:
            out.setdefault(o.tid, np.zeros(g.tensors[o.tid][2], bool))[o.coff:o.coff + ceil_to(o.c, 8)] = True
    return out


def fill_sentinel(net):
    """Before the first run: every tensor some layer writes (the input tensor is the test's), all max_batch samples and
    all stored channels, set to the sentinel."""
    for tid in _written(net.graph):
        h, w, c, f32 = net.graph.tensors[tid]
        write_raw(net, tid, np.full((net.max_batch, h, w, c), SENT32 if f32 else SENT16))


def check_sentinel(net, batch, label, also=()):
    """After the last run of a network prepared with fill_sentinel: outside the written channels of the first `batch`
    samples every element still is the sentinel, inside every element is finite.
    also: tids whose samples beyond the batch the test itself set to the sentinel (its input)."""
    g = net.graph
    masks = _written(g)
    for tid in list(masks) + list(also):
        h, w, c, f32 = g.tensors[tid]
        a = net.read(_whole(g, tid), net.max_batch)              # (fp16 -> fp32 is exact: equal values are equal bits)
        kept = a == np.float32(SENT32 if f32 else SENT16)
        what = f'{label} tensor {tid} ({h}x{w}x{c}{" fp32" if f32 else ""})'
        beyond = np.argwhere(~kept[batch:])
        assert not len(beyond), f'{what}: {len(beyond)} elements of the samples beyond batch {batch} changed, the first at ' \
                                f'(sample, y, x, channel) {tuple(int(v) for v in beyond[0] + (batch, 0, 0, 0))}'
        if tid not in masks:
            continue
        m = masks[tid]
        out = np.argwhere(~kept[:batch][..., ~m])
        assert not len(out), f'{what}: {len(out)} elements outside the written channels {_ranges(m)} changed, the first at ' \
                             f'(sample, y, x) {tuple(int(v) for v in out[0][:3])}, channel {int(np.flatnonzero(~m)[out[0][3]])}'
        inside = a[:batch][..., m]
        assert np.isfinite(inside).all(), f'{what}: non-finite values in the written channels'


def _ranges(mask):
    edges = np.flatnonzero(np.diff(np.concatenate([[0], mask.astype(np.int8), [0]])))
    return [(int(a), int(b)) for a, b in zip(edges[::2], edges[1::2])]


def check_pair(a, b, what):
    """a, b: (graph, the `keep` dict of its check_net, layer index) of two runs whose layers compute ONE function of
    bit-identical network inputs (read back and compared here).  Each result lies within its own bound of the same float64
    reference, so |a - b| <= bound_a + bound_b elementwise: the triangle inequality, nothing measured -> worst ratio."""
    (ga, ka, ia), (gb, kb, ib) = a, b
    assert torch.equal(ka['final'][ga.input.tid], kb['final'][gb.input.tid]), f'{what}: the two runs read different inputs'
    (ref_a, bound_a), (ref_b, bound_b) = ka[ia], kb[ib]
    gap = (ref_a - ref_b).abs()              # the same float64 arithmetic evaluated twice: 0, or its own summation order
    assert float(gap.max()) <= 1e-12 * float(ref_a.abs().max()), f'{what}: the two float64 references differ by {float(gap.max())}'
    oa, ob = ga.layers[ia]['out'], gb.layers[ib]['out']
    return torch_ref.check_layer(ka['final'][oa.tid][:, oa.coff:oa.coff + oa.c], kb['final'][ob.tid][:, ob.coff:ob.coff + ob.c],
                                 bound_a + bound_b + gap, what)
