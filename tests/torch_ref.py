"""TEST INFRASTRUCTURE: plain PyTorch (CPU, NCHW) interpreter of a models/graph.py layer table
-- the reference the conv-engine kernels are compared against (the reference's own conv arithmetic
is TensorRT's, which is neither available nor pinned).

Two entry points share ONE set of op bodies (`_Interp.step`):
  * `run_graph`: the whole table in fp32; `emulate_fp16_storage=True` rounds every layer output to fp16, as the
    engine stores activations.
  * `run_layer`: ONE layer of the table from given input tensors ("teacher forcing": the tensors the device itself
    produced), in float64 and without any fp16 rounding of its own, together with an ELEMENTWISE bound on
    |device - float64| derived from the number formats:
        u16 = 2^-11 (fp16 round to nearest), u32 = 2^-23 (one fp32 ulp: holds for a rounding or a truncating matrix
        pipe), K = cin / groups * kh * kw, L = 1.1 (largest slope of any activation of graph.ACT),
        S = |W| (*) |x| + |b| (the same convolution on absolute values);
        one stage (conv + bias + residual + activation) with input bound d_in:
            d_pre = |W| (*) d_in + K * u32 * S,   d_act = L * d_pre (+ d_res),
            stored as fp16:  d_out = d_act * (1 + u16) + u16 * |ref| + 2^-24      (2^-24: fp16 subnormal spacing)
            stored as fp32:  d_out = d_act + 5e-6 * |ref|                         (the device's fast-exp activations)
    Fused ops apply the rule stage by stage, the fp16 intermediate's d_out being the next stage's d_in.  Ops that only
    select (max pools, SPP, upsample, copy) have bound 0 on exact inputs: the comparison is then array_equal.
    The parameters are the ones the engine holds: graph.conv_params / *_ref keep the fp16-ROUNDED weights (as fp32
    arrays) and the fp32 biases that Graph packed into the blob, so no further rounding is applied here."""
import numpy as np
import torch
import torch.nn.functional as F

from fastmot_amd.models import graph as G

U16, U32, SUB16 = 2.0 ** -11, 2.0 ** -23, 2.0 ** -24
L_ACT = 1.1            # mish 1.089, swish 1.100, leaky / relu / linear 1, logistic 0.25
FAST_EXP = 5e-6        # relative error allowed for an fp32 result of the device's fast-exp activations (as the decode rows)

OP_NAMES = {v: k for k, v in vars(G).items() if k.startswith('OP_')}


def act_fn(x, act):
    if act == G.ACT['leaky']:
        return F.leaky_relu(x, 0.1)
    if act == G.ACT['mish']:
        return x * torch.tanh(F.softplus(x))
    if act == G.ACT['relu']:
        return F.relu(x)
    if act == G.ACT['logistic']:
        return torch.sigmoid(x)
    if act == G.ACT['swish']:
        return x * torch.sigmoid(x)
    return x


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to(dtype)


class _Interp:
    """Evaluates layers on values `v` and, when `track`, bounds `e` (None: not tracked; 0.0: exact).
    inplace=True (run_graph): results go into the caller's `bufs`.  inplace=False (run_layer): `bufs` is read only and
    results are kept as channel slices in `written`, which later (sub-)layers of the same call read back.
    `mut(point, stage, *tensors)` (tests/test_layer_bound_host.py only): lets a test plant one defect in one stage."""

    def __init__(self, graph, bufs, dtype, emulate, track=False, inplace=True, gates=None, s_dtype=None,
                 channels_last=False, mut=None, u16=U16):
        self.u16 = u16
        self.g, self.bufs, self.dt, self.emulate, self.track, self.inplace = graph, bufs, dtype, emulate, track, inplace
        self.gates = {} if gates is None else gates
        self.s_dt = s_dtype or dtype
        self.cl, self.mut = channels_last, mut
        self.written = {}
        self.emb = None
        self.stage = 0

    # ------------------------------------------------------------ storage
    def rd(self, v):
        if self.inplace:
            return self.bufs[v.tid][:, v.coff:v.coff + v.c], (0.0 if self.track else None)
        pieces = [p for p in self.written.get(v.tid, []) if p[0] < v.coff + v.c and v.coff < p[0] + p[1]]
        for coff, c, val, err in pieces:
            if coff <= v.coff and v.coff + v.c <= coff + c:
                s = slice(v.coff - coff, v.coff - coff + v.c)
                return val[:, s], (err[:, s] if torch.is_tensor(err) else err)
        val = self.bufs[v.tid][:, v.coff:v.coff + v.c].to(self.dt).contiguous()
        if not pieces:
            return val, (0.0 if self.track else None)
        val = val.clone()
        err = torch.zeros_like(val)
        for coff, c, pv, pe in pieces:
            lo, hi = max(coff, v.coff), min(coff + c, v.coff + v.c)
            val[:, lo - v.coff:hi - v.coff] = pv[:, lo - coff:hi - coff]
            if self.track:
                err[:, lo - v.coff:hi - v.coff] = pe[:, lo - coff:hi - coff] if torch.is_tensor(pe) else pe
        return val, (err if self.track else None)

    def store16(self, x):
        """A value the device rounds to fp16 (an activation tensor or an intermediate of a fused op)."""
        v, e = x
        if self.track:
            return v, e * (1 + self.u16) + self.u16 * v.abs() + SUB16
        return (v.half().to(self.dt) if self.emulate else v), None

    def wr(self, view, x, f32=False, exact=False):
        v, e = x
        if exact:                            # pure selection: nothing is rounded
            pass
        elif f32:
            e = e + FAST_EXP * v.abs() if self.track else None
        else:
            v, e = self.store16(x)
        if self.inplace:
            self.bufs[view.tid][:, view.coff:view.coff + view.c] = v
        else:
            self.written.setdefault(view.tid, []).insert(0, (view.coff, view.c, v, e))

    # ------------------------------------------------------------ building blocks
    def _m(self, point, *a):
        return self.mut(point, self.stage, *a) if self.mut is not None else a[0]

    def conv_stage(self, x, w, b, act, stride=1, padding=0, groups=1, res=None, res_mode=G.RES_NONE):
        """act(conv(x) + b [+ res]) [+ res] with its bound; every conv-like stage of every op goes through here."""
        xv, xe = x
        w = self._m('w', _t(w, self.dt))
        b = _t(b, self.dt) if b is not None else None
        xv, padding = self._m('x', (xv, padding))
        res_mode = self._m('res_mode', res_mode)
        if self.cl:
            xv, w = xv.contiguous(memory_format=torch.channels_last), w.contiguous(memory_format=torch.channels_last)
        kw = dict(stride=stride, padding=padding, groups=groups)
        y = F.conv2d(xv, w, b, **kw)
        e = None
        if self.track:
            K = w[0].numel() + (1 if res_mode == G.RES_BEFORE_ACT else 0)
            aw = w.abs()
            S = F.conv2d(xv.abs().to(self.s_dt), aw.to(self.s_dt), b.abs().to(self.s_dt) if b is not None else None, **kw).to(self.dt)
            if self.s_dt != self.dt:
                S = S * (1 + K * U32)        # S itself summed in fp32: its own rounding, second order
            if res_mode == G.RES_BEFORE_ACT:
                S = S + res[0].abs()
            e = K * U32 * S
            if torch.is_tensor(xe):
                e = e + F.conv2d(xe, aw, None, **kw)
        if res_mode == G.RES_BEFORE_ACT:
            y = y + res[0]
            if self.track:
                e = e + res[1]
        y = self._m('act', act_fn(y, act), y)
        if self.track:
            e = L_ACT * e
        if res_mode == G.RES_AFTER_ACT:
            y = y + res[0]
            if self.track:
                e = e + res[1] + U32 * y.abs()           # the add itself, in fp32
        y = self._m('y', y)
        self.stage += 1
        return y, e

    def mean_stage(self, x):
        """Global average pool, kept [N, C, 1, 1] in fp32 on the device (h * w adds and one scale)."""
        v, e = x
        m = v.mean(dim=(2, 3), keepdim=True)
        if not self.track:
            return m, None
        hw = v.shape[2] * v.shape[3]
        em = (hw + 1) * U32 * v.abs().mean(dim=(2, 3), keepdim=True)
        if torch.is_tensor(e):
            em = em + e.mean(dim=(2, 3), keepdim=True)
        return m, em

    def gate_of(self, x, ref):
        """OSNet ChannelGate of one stream: sigmoid(fc2(relu(fc1(GAP(x))))), fp32 on the device -> [N, C, 1, 1]."""
        w1, b1, w2, b2 = ref
        hid = self.conv_stage(self.mean_stage(x), np.asarray(w1)[:, :, None, None], b1, G.ACT['relu'])
        gv, ge = self.conv_stage(hid, np.asarray(w2)[:, :, None, None], b2, G.ACT['logistic'])
        return gv, (ge + FAST_EXP * gv.abs() if self.track else None)

    def gated_sum(self, terms):
        """sum_i x_i * g_i (fp32 fmaf chain on the device: one rounding per term)."""
        y, e, S = 0, 0.0, 0
        for (xv, xe), (gv, ge) in terms:
            y = y + xv * gv
            if self.track:
                S = S + xv.abs() * gv.abs()
                e = e + xv.abs() * ge + xe * (gv.abs() + ge)
        return y, (e + 2 * len(terms) * U32 * S if self.track else None)

    def select(self, x, fn):
        v, e = x
        return fn(v), (fn(e) if torch.is_tensor(e) else e)

    def is_exact(self, x):
        return self.track and not torch.is_tensor(x[1])

    # ------------------------------------------------------------ the ops
    def step(self, d, wb):
        op = d['op']
        g = self.g
        x = self.rd(d['ins'][0])
        if op == G.OP_OSTAIL:            # the layers the fused launch replaces, with their own references
            for sd, swb in d['sub']:
                self.step(sd, swb)
        elif op in G.CONV_OPS + (G.OP_STEMCONV,):
            w, b = wb
            res = self.rd(d['res']) if d['res_mode'] != G.RES_NONE else None
            y = self.conv_stage(x, w, b, d['act'], stride=d['stride'], padding=d['pad'], res=res, res_mode=d['res_mode'])
            if d['up'] == 2:
                y = self.select(y, lambda t: F.interpolate(t, scale_factor=2, mode='nearest'))
            self.wr(d['out'], y, f32=bool(g.tensors[d['out'].tid][3]))
        elif op == G.OP_RESBLOCK:
            w1, b1, w2, b2 = d['res_ref']
            y = self.store16(self.conv_stage(x, w1, b1, d['act']))
            self.wr(d['out'], self.conv_stage(y, w2, b2, d['act'], padding=1, res=x, res_mode=G.RES_AFTER_ACT))
        elif op == G.OP_PAIR11:
            w1, b1, act1, w2, b2 = d['pair_ref']
            tv, te = self.store16(self.conv_stage(x, w1, b1, act1))
            ov, oe = self.rd(d['ins'][1])
            cat = torch.cat([tv, ov], dim=1)
            ce = torch.cat([te, oe if torch.is_tensor(oe) else torch.zeros_like(ov)], dim=1) if self.track else None
            self.wr(d['out'], self.conv_stage((cat, ce), w2, b2, d['act']))
        elif op == G.OP_STEM2:
            w1, b1, act1, w2, b2 = d['stem2_ref']
            three = 'stem3_ref' in d
            y = self.store16(self.conv_stage(x, w1, b1, act1, padding=1))
            y = self.conv_stage(y, w2, b2, d['stem3_ref'][0] if three else d['act'], stride=2, padding=1)
            if three:
                _, w3, b3 = d['stem3_ref']
                y = self.conv_stage(self.store16(y), w3, b3, d['act'])
            self.wr(d['out'], y)
        elif op == G.OP_DWCONV3:
            w, b = wb
            self.wr(d['out'], self.conv_stage(x, w, b, d['act'], padding=1, groups=x[0].shape[1]))
        elif op == G.OP_LITECONV:
            c = d['cout']
            for gi, (v, (pw, wd, bd)) in enumerate(zip(d['ins'], d['lite_ref'])):
                y = self.store16(self.conv_stage(self.rd(v), pw, None, G.ACT['linear']))
                self.wr(d['out'].slice(gi * c, c), self.conv_stage(y, wd, bd, d['act'], padding=1, groups=c))
        elif op == G.OP_LITECHAIN:
            c = d['cout']
            refs = iter(d['lite_ref'])
            for t in range(4):
                y = x
                for lvl in range(t + 1):
                    pw, wd, bd = next(refs)
                    if lvl:
                        y = self.store16(y)
                    y = self.store16(self.conv_stage(y, pw, None, G.ACT['linear']))
                    y = self.conv_stage(y, wd, bd, d['act'], padding=1, groups=c)
                self.wr(d['out'].slice(t * c, c), y)
        elif op == G.OP_GATED_SUM:
            xs = [self.rd(v) for v in d['ins']]
            self.wr(d['out'], self.gated_sum([(xv, self.gate_of(xv, d['gate_ref'])) for xv in xs]))
        elif op == G.OP_SPP:
            c = d['cout']
            for i, k in enumerate(self._m('spp_order', (13, 9, 5))):
                self.wr(d['out'].slice(i * c, c), self.select(x, lambda t, k=k: F.max_pool2d(t, k, 1, k // 2)), exact=self.is_exact(x))
        elif op == G.OP_MAXPOOL:
            pe = d.get('pad_end', d['pad'])

            def pool(t, neutral=float('-inf')):
                return F.max_pool2d(F.pad(t, (d['pad'], pe, d['pad'], pe), value=neutral), d['k'], d['stride'], 0)
            v, e = x
            self.wr(d['out'], (pool(v), pool(e, 0.0) if torch.is_tensor(e) else e), exact=self.is_exact(x))
        elif op == G.OP_AVGPOOL:
            v, e = x

            def pool(t):
                return F.avg_pool2d(t, d['k'], d['stride'], d['pad'])
            ye = None
            if self.track:
                ye = (d['k'] * d['k'] + 1) * U32 * pool(v.abs()) + (pool(e) if torch.is_tensor(e) else 0.0)
            self.wr(d['out'], (pool(v), ye))
        elif op == G.OP_UPSAMPLE2:
            self.wr(d['out'], self.select(x, lambda t: F.interpolate(t, scale_factor=2, mode='nearest')), exact=self.is_exact(x))
        elif op == G.OP_ADD:
            ov, oe = self.rd(d['ins'][1])
            self.wr(d['out'], (x[0] + ov, (x[1] + oe + 2 * U32 * (x[0].abs() + ov.abs())) if self.track else None))
        elif op == G.OP_COPY:
            self.wr(d['out'], x, exact=self.is_exact(x))
        elif op == G.OP_GATE:
            self.gates[d['gates'][0]] = self.gate_of(x, d['gate_ref'])
        elif op == G.OP_GATE_SUM:
            self.wr(d['out'], self.gated_sum([(self.rd(v), self.gates[gid]) for v, gid in zip(d['ins'], d['gates'])]))
        elif op == G.OP_HEAD:
            w, b = d['head_ref']
            fv, fe = self.conv_stage(self.mean_stage(x), np.asarray(w)[:, :, None, None], b, G.ACT['relu'])
            fv, n = fv[:, :, 0, 0], fv[:, :, 0, 0].norm(dim=1, keepdim=True)
            ev = fv / n
            ee = None
            if self.track:       # |f/n - f'/n'| <= d_f / n' + |f| d_n / (n n'),  d_n <= ||d_f||_2 + (C + 2) u32 n,  n' >= n - d_n
                fe = fe[:, :, 0, 0]
                dn = fe.norm(dim=1, keepdim=True) + (fv.shape[1] + 2) * U32 * n
                nlo = (n - dn).clamp_min(1e-30)
                ee = fe / nlo + fv.abs() * dn / (n * nlo) + (2 * U32 + FAST_EXP) * ev.abs()
            self.emb = (ev, ee)
        else:
            raise ValueError(op)


def run_graph(graph, x_nchw, emulate_fp16_storage=True, channels_last=False, around=None):
    """x_nchw: float tensor [N, C, H, W].  Returns dict tid -> tensor [N, cpad, h, w] and the
    embedding matrix if the graph has a head.  channels_last: the convolutions run in the other memory format
    (another kernel, another summation order: the host stand-in for a device, tests/test_layer_bound_host.py).
    around(idx, bufs): called before layer idx runs; what it returns, if callable, is called as f(bufs, emb) after it."""
    n = x_nchw.shape[0]
    bufs = {}
    for tid, (h, w, c, f32) in enumerate(graph.tensors):
        bufs[tid] = torch.zeros(n, c, h, w)
    x = x_nchw.float()
    if emulate_fp16_storage:
        x = x.half().float()
    bufs[graph.input.tid][:, :x.shape[1]] = x
    params = {idx: (w, b) for idx, w, b in graph.conv_params}
    it = _Interp(graph, bufs, torch.float32, emulate_fp16_storage, channels_last=channels_last)
    for idx, d in enumerate(graph.layers):
        after = around(idx, bufs) if around is not None else None
        it.step(d, params.get(idx))
        if callable(after):
            after(bufs, it.emb[0] if it.emb is not None else None)
    return bufs, (it.emb[0] if it.emb is not None else None)


def run_layer(graph, idx, bufs, dtype=torch.float64, gates=None, s_dtype=None, emulate_fp16_storage=False,
              channels_last=False, mut=None, u16=U16):
    """Layer `idx` of the table from the tensors in `bufs` (tid -> [N, cpad, h, w], any float dtype; only the layer's
    inputs are needed and nothing is modified).  -> (kind, ref, bound):
      kind 'tensor': ref / bound [N, c, h, w] for the channels of the layer's `out` view;
      kind 'emb' (OP_HEAD, OP_OSTAIL): the [N, dim] embeddings;  kind 'gate' (OP_GATE): (None, None) -- the gate goes
      to the caller's `gates` dict (pass the same dict for every layer of a table, in layer order).
    With the defaults `ref` is float64 without fp16 rounding and `bound` the elementwise bound of the module docstring
    (0 where the op only selects).  s_dtype=torch.float32 evaluates S, the abs-value convolution, in fp32.
    dtype=float32, emulate_fp16_storage=True (and channels_last / mut) make the same call a host stand-in for the device:
    `bound` is then None.  u16: the relative size of one fp16 store in the bound (2^-11: round to nearest)."""
    d = graph.layers[idx]
    track = not emulate_fp16_storage
    params = {i: (w, b) for i, w, b in graph.conv_params}
    it = _Interp(graph, bufs, dtype, emulate_fp16_storage, track=track, inplace=False, gates=gates, s_dtype=s_dtype,
                 channels_last=channels_last, mut=mut, u16=u16)
    it.step(d, params.get(idx))
    if d['op'] in (G.OP_HEAD, G.OP_OSTAIL):
        return ('emb',) + it.emb
    if d['op'] == G.OP_GATE:
        return 'gate', None, None
    v, e = it.rd(d['out'])
    if track and not torch.is_tensor(e):
        e = torch.full_like(v, e)
    return 'tensor', v, e


def clobbers(graph):
    """Layers that overwrite channels an earlier layer wrote (the merged CSP stages reuse the first half of their
    concat tensor): [(layer index, tid)].  After a whole run such a tensor no longer holds what the layers before the
    overwrite read, so a teacher-forced check needs its state from a run of the table cut before that layer."""
    seen, out = {}, []
    for li, d in enumerate(graph.layers):
        if d['op'] in (G.OP_HEAD, G.OP_OSTAIL, G.OP_GATE):
            continue
        o = d['out']
        if any(lo < o.coff + o.c and o.coff < hi for lo, hi in seen.get(o.tid, [])):
            out.append((li, o.tid))
        seen.setdefault(o.tid, []).append((o.coff, o.coff + o.c))
    return out


def check_layer(got, ref, bound, what, tile=32):
    """Asserts |got - ref| <= bound elementwise ([N, c, h, w] or [N, dim]); -> worst err / bound (0 / 0 = 0).
    The message names the worst element, its ratio and, for maps, the 32-channel block and 32-pixel tile it lies in."""
    got, ref, bound = (torch.as_tensor(a).to(torch.float64) for a in (got, ref, bound))
    err = (got - ref).abs()
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    worst = float(ratio.max())
    if worst > 1 or not torch.isfinite(ratio).all():
        at = np.unravel_index(int(torch.nan_to_num(ratio, nan=float('inf')).argmax()), tuple(ratio.shape))
        where = f'element {tuple(int(i) for i in at)}'
        if ratio.dim() == 4:
            n, c, y, x = at
            where += f' (channel block {c // tile}, pixel tile {(y * ratio.shape[3] + x) // tile} of row-major {tile}-pixel tiles)'
        raise AssertionError(f'{what}, shape {tuple(ratio.shape)}: |got - ref64| = {float(err[at]):.6g} > bound {float(bound[at]):.6g} '
                             f'(ratio {float(ratio[at]):.4g}) at {where}; got {float(got[at]):.6g}, ref {float(ref[at]):.6g}; '
                             f'{int((ratio > 1).sum())} elements over the bound')
    return worst
