"""GPU parity: association kernels (assoc.hip) through the C ABI.
  * oracle=reference: tests/golden/assoc_kat.npz (cdist/iou/occluded/fuse+gate/LAP/greedy from the
    reference source)
  * oracle=restated : np_oracle + scipy.optimize.linear_sum_assignment on seeded inputs incl.
    tie-heavy, rectangular, gated (1e5) and degenerate matrices.  Index results must be IDENTICAL.
Off the defaults: the Mahalanobis term on evolved (non-diagonal) covariances under both parameter sets, the LDS chunk
loop and the I/O switch of find_occluded, fm_iou_dist, every way fm_assoc_cascade solves its stages, lap_kernel with its
work arrays in global memory and with more than 64 KiB of LDS, infeasible matrices, results returned by blit copy."""
import numpy as np
import pytest

import cascade_cases
import np_oracle as o
from fastmot_amd import _lib

pytestmark = pytest.mark.gpu

KF_DEFAULT = dict(std_factor_acc=2.25, std_offset_acc=78.5, std_factor_det=(0.08, 0.08),
                  std_factor_klt=(0.14, 0.14), min_std_det=(4.0, 4.0), min_std_klt=(5.0, 5.0),
                  init_pos_weight=5, init_vel_weight=12, vel_coupling=0.6, vel_half_life=2)
KF_OFFDEFAULT = dict(std_factor_acc=1.7, std_offset_acc=40.0, std_factor_det=(0.05, 0.11),
                     std_factor_klt=(0.2, 0.09), min_std_det=(3.0, 6.5), min_std_klt=(7.0, 4.0),
                     init_pos_weight=3, init_vel_weight=9, vel_coupling=0.35, vel_half_life=0.7)
KF_SETS = {'default': KF_DEFAULT, 'offdefault': KF_OFFDEFAULT}
CHI_SQ_INV_95 = 9.4877


class options:
    """Context options for the body; the session-wide context gets its defaults back."""
    DEFAULTS = dict(zero_copy_tracks=2048, host_lap_elems=262144)

    def __init__(self, ctx, **values):
        self.ctx, self.values = ctx, values

    def __enter__(self):
        for k, v in self.values.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.values:
            self.ctx.set_option(k, self.DEFAULTS[k])


def load_tracks(ctx, feats, counts=None):
    """Puts features into slots 1..n through the public feature path (first update = copy)."""
    n = len(feats)
    slots = np.arange(1, n + 1)
    ctx.feat_reset(slots)
    ctx.emb_upload(feats.astype(np.float32))
    ctx.feat_update(slots, np.arange(n))
    return slots


@pytest.mark.parametrize('tag', ['a', 'b', 'c', 'd'])
def test_golden_pairwise_and_stage(ctx, golden_dir, tag):
    g = np.load(golden_dir / 'assoc_kat.npz')
    ctx.kf_configure(1 / 30., **KF_DEFAULT)
    XA, XB = g[f'{tag}_XA'], g[f'{tag}_XB']
    ta, db = g[f'{tag}_ta'], g[f'{tag}_db']
    nt, nd = len(XA), len(XB)
    slots = load_tracks(ctx, XA)
    ctx.trk_create(slots, ta)
    occ = g[f'{tag}_occ']
    np.testing.assert_array_equal(ctx.find_occluded(db, 0.7), occ)
    np.testing.assert_array_equal(ctx.find_occluded(db, 0.3), g[f'{tag}_occ3'])
    for metric, key, tol in ((_lib.METRIC_COSINE, 'cos', 2e-7), (_lib.METRIC_EUCLIDEAN, 'euc', 1e-12)):
        ctx.emb_upload(XB)
        ctx.assoc_prepare(metric, slots, ta, g[f'{tag}_tlab'], db, g[f'{tag}_dlab'], occ)
        feat, maha, iou = ctx.assoc_get_pairwise(nt, nd)
        ref = g[f'{tag}_{key}']
        mask = g[f'{tag}_mask']
        np.testing.assert_allclose(feat[~mask], ref[~mask], rtol=0, atol=tol)
        np.testing.assert_array_equal(iou, g[f'{tag}_iou'])
        # restated oracle (Numba typing): tight tolerance
        exp = o.cdist(XA.astype(np.float64), XB, 'cosine' if key == 'cos' else 'euclidean')
        np.testing.assert_allclose(feat, exp, rtol=0, atol=1e-13)
        p = o.KFParams(1 / 30.)
        m, c = o.kf_create(p, ta)
        np.testing.assert_allclose(maha, o.kf_maha(p, m, c, db), rtol=1e-10)
    # IoU stage cost + LAP + greedy vs reference outputs
    rows, cols = np.arange(nt), np.arange(nd)
    m_rows, m_cols, gated, cost = ctx.assoc_stage(_lib.STAGE_IOU, _lib.SOLVER_GREEDY, rows, cols,
                                                  max_cost=0.8, want_cost=True)
    exp_cost = o.gate_cost(g[f'{tag}_iou'], g[f'{tag}_tlab'], g[f'{tag}_dlab'], 0.8)
    np.testing.assert_array_equal(cost, exp_cost)
    em, _, _ = o.greedy_match(exp_cost, 0.8)
    assert list(zip(m_rows.tolist(), m_cols.tolist())) == em
    # golden LAP on the reference's fused+gated cost matrix
    r, c = ctx.lap(g[f'{tag}_cost'])
    er, ec = o.lsa(g[f'{tag}_cost'])
    np.testing.assert_array_equal(r, er)
    np.testing.assert_array_equal(c, ec)
    m, ur, uc = o.assignment_matches(g[f'{tag}_cost'], r, c)
    assert [(100 + a, b) for a, b in m] == [tuple(x) for x in g[f'{tag}_lap_m'].tolist()]
    assert [100 + a for a in ur] == g[f'{tag}_lap_ut'].tolist() and uc == g[f'{tag}_lap_ud'].tolist()
    gr, gc = ctx.greedy(g[f'{tag}_iou'], 0.8)
    assert [(100 + a, b) for a, b in zip(gr.tolist(), gc.tolist())] == [tuple(x) for x in g[f'{tag}_gr_m'].tolist()]


def test_matching_stage_vs_oracle(ctx):
    rng = np.random.default_rng(42)
    dt = 1 / 30.
    ctx.kf_configure(dt, **KF_DEFAULT)
    p = o.KFParams(dt)
    for nt, nd, metric in ((50, 50, 'euclidean'), (7, 90, 'cosine'), (120, 33, 'cosine'), (300, 300, 'euclidean')):
        tl = rng.uniform(0, 1500, (nt, 2))
        tb = np.rint(np.concatenate([tl, tl + rng.uniform(30, 200, (nt, 2))], 1))
        sel = rng.integers(0, nt, nd)
        db = np.rint(tb[sel] + rng.normal(0, 8, (nd, 4)))
        XA = rng.normal(0, 1, (nt, 512)).astype(np.float32)
        XA /= np.linalg.norm(XA, axis=1, keepdims=True)
        XB = (XA[sel] + rng.normal(0, 0.03, (nd, 512))).astype(np.float32)
        XB /= np.linalg.norm(XB, axis=1, keepdims=True)
        slots = load_tracks(ctx, XA)
        nofeat = rng.random(nt) < 0.1
        ctx.feat_reset(slots[nofeat])
        ctx.trk_create(slots, tb)
        m, c = o.kf_create(p, tb)
        tlab, dlab = rng.integers(0, 2, nt), rng.integers(0, 2, nd)
        occ = o.find_occluded(db, 0.7)
        ctx.emb_upload(XB)
        mid = _lib.METRIC_COSINE if metric == 'cosine' else _lib.METRIC_EUCLIDEAN
        ctx.assoc_prepare(mid, slots, tb, tlab, db, dlab, occ)
        rows = rng.permutation(nt)[:max(1, nt // 2)]
        cols = rng.permutation(nd)[:max(1, (2 * nd) // 3)]
        m_rows, m_cols, gated, cost = ctx.assoc_stage(_lib.STAGE_MATCHING, _lib.SOLVER_LAP, rows, cols,
                                                      motion_weight=0.2, max_cost=0.8, fill_val=0.9,
                                                      want_cost=True)
        mask = nofeat[:, None] | occ[None, :]
        fd = o.cdist(XA.astype(np.float64), XB, metric, mask, 0.9)
        exp = o.matching_cost(fd, o.kf_maha(p, m, c, db), tlab, dlab, 0.2, 0.8)[np.ix_(rows, cols)]
        big = exp >= 1e5
        np.testing.assert_array_equal(cost >= 1e5, big)
        np.testing.assert_allclose(cost[~big], exp[~big], rtol=0, atol=1e-11)
        er, ec = o.lsa(cost)
        np.testing.assert_array_equal(m_rows, er)
        np.testing.assert_array_equal(m_cols, ec)
        np.testing.assert_array_equal(gated, cost[er, ec] >= 1e5)


@pytest.mark.parametrize('kf', ['default', 'offdefault'])
def test_matching_stage_evolved_tracks(ctx, kf):
    """The same stage on tracks two device steps old: S is a full matrix in pairwise_kernel's Cholesky and forward
    substitution (straight from trk_create it is diagonal and every off-diagonal product multiplies a zero)."""
    rng = np.random.default_rng(43)
    kf = KF_SETS[kf]
    dt = 1 / 30.
    ctx.kf_configure(dt, **kf)
    ctx.set_frame_rect([0., 0., 1919., 1079.])
    p = o.KFParams(dt, **kf)
    for nt, nd, metric in ((50, 50, 'euclidean'), (7, 90, 'cosine'), (120, 33, 'cosine'), (150, 140, 'euclidean')):
        tl = rng.uniform(0, 1500, (nt, 2))
        tb = np.rint(np.concatenate([tl, tl + rng.uniform(30, 200, (nt, 2))], 1))
        XA = rng.normal(0, 1, (nt, 512)).astype(np.float32)
        XA /= np.linalg.norm(XA, axis=1, keepdims=True)
        slots = load_tracks(ctx, XA)
        ctx.trk_create(slots, tb)
        H = np.eye(3) + rng.normal(0, 1e-2, (3, 3))
        H[:2, 2] = rng.normal(0, 8, 2); H[2, :2] = rng.normal(0, 1e-4, 2); H[2, 2] = 1.
        for it in range(2):
            m, _ = ctx.trk_get_state(slots)
            ctx.trk_step(slots, H, np.rint(m[:, :4] + rng.normal(0, 3, (nt, 4))), rng.random(nt) < 0.7,
                         rng.uniform(1, 6, nt))
        m, c = ctx.trk_get_state(slots)            # the oracle works on the state the device holds
        assert np.abs(c[:, 0, 2]).min() > 0 and np.abs(c[:, 1, 3]).min() > 0
        tb = np.rint(m[:, :4])
        sel = rng.integers(0, nt, nd)
        db = np.rint(tb[sel] + rng.normal(0, 8, (nd, 4)))
        XB = (XA[sel] + rng.normal(0, 0.03, (nd, 512))).astype(np.float32)
        XB /= np.linalg.norm(XB, axis=1, keepdims=True)
        nofeat = rng.random(nt) < 0.1
        ctx.feat_reset(slots[nofeat])
        tlab, dlab = rng.integers(0, 2, nt), rng.integers(0, 2, nd)
        occ = o.find_occluded(db, 0.7)
        ctx.emb_upload(XB)
        mid = _lib.METRIC_COSINE if metric == 'cosine' else _lib.METRIC_EUCLIDEAN
        ctx.assoc_prepare(mid, slots, tb, tlab, db, dlab, occ)
        rows = rng.permutation(nt)[:max(1, nt // 2)]
        cols = rng.permutation(nd)[:max(1, (2 * nd) // 3)]
        m_rows, m_cols, gated, cost = ctx.assoc_stage(_lib.STAGE_MATCHING, _lib.SOLVER_LAP, rows, cols,
                                                      motion_weight=0.2, max_cost=0.8, fill_val=0.9,
                                                      want_cost=True)
        mask = nofeat[:, None] | occ[None, :]
        fd = o.cdist(XA.astype(np.float64), XB, metric, mask, 0.9)
        maha = o.kf_maha(p, m, c, db)
        # no decision of this case hangs on the last bits: nothing sits on the chi-square gate or on max_cost
        fused = 0.8 * fd + 0.2 * (1. / CHI_SQ_INV_95) * maha
        assert np.abs(maha - CHI_SQ_INV_95).min() > 1e-6
        assert np.abs(fused[maha <= CHI_SQ_INV_95] - 0.8).min() > 1e-9
        assert (maha <= CHI_SQ_INV_95).any() and (maha > CHI_SQ_INV_95).any()
        exp = o.matching_cost(fd, maha, tlab, dlab, 0.2, 0.8)[np.ix_(rows, cols)]
        big = exp >= 1e5
        assert not big.all()
        np.testing.assert_array_equal(cost >= 1e5, big)
        np.testing.assert_allclose(cost[~big], exp[~big], rtol=0, atol=1e-11)
        er, ec = o.lsa(cost)
        np.testing.assert_array_equal(m_rows, er)
        np.testing.assert_array_equal(m_cols, ec)
        np.testing.assert_array_equal(gated, cost[er, ec] >= 1e5)


@pytest.mark.parametrize('fixture,tag,kf', [('kalman_kat', 'dt30', 'default'), ('kalman_kat', 'dt12', 'default'),
                                            ('kalman_kat_offdefault', 'od30', 'offdefault'),
                                            ('kalman_kat_offdefault', 'od7', 'offdefault')])
def test_golden_maha_on_evolved_covariances(ctx, golden_dir, fixture, tag, kf):
    """pairwise_kernel's Mahalanobis term against the reference's motion_distance on the covariances the reference
    itself evolved (rtol 1e-9: what tests/test_oracle_golden.py grants the oracle against these vectors) and against
    the oracle (rtol 1e-10)."""
    g = np.load(golden_dir / f'{fixture}.npz')
    dt = float(g[f'{tag}_dt'])
    ctx.kf_configure(dt, **KF_SETS[kf])
    m, c, det = g[f'{tag}_klt_m'], g[f'{tag}_klt_c'], g[f'{tag}_det']
    assert np.abs(c[:, 0, 2]).min() > 0 and np.abs(c[:, 1, 3]).min() > 0 and np.abs(c[:, 0, 1]).max() > 0
    n = len(m)
    slots = np.arange(3, 3 + n)
    ctx.trk_set_state(slots, m, c)
    ctx.emb_upload(np.zeros((n, ctx.feat_dim), np.float32))
    zeros = np.zeros(n, int)
    ctx.assoc_prepare(_lib.METRIC_EUCLIDEAN, slots, np.rint(m[:, :4]), zeros, det, zeros, np.zeros(n, bool))
    _, maha, iou = ctx.assoc_get_pairwise(n, n)
    np.testing.assert_allclose(maha, g[f'{tag}_maha'], rtol=1e-9)
    np.testing.assert_allclose(maha, o.kf_maha(o.KFParams(dt, **KF_SETS[kf]), m, c, det), rtol=1e-10)
    np.testing.assert_array_equal(iou, o.iou_dist(np.rint(m[:, :4]), det))


def _crowd(n):
    """n boxes spread so that a good part of them is occluded at either threshold and a good part is not."""
    if n == 2:
        return np.array([[0., 0., 99., 99.], [20., 10., 60., 50.]])      # the second lies inside the first
    rng = np.random.default_rng(900 + n)
    tl = rng.uniform(0, 80. * np.sqrt(n) + 40, (n, 2))
    return np.rint(np.concatenate([tl, tl + rng.uniform(10, 160, (n, 2))], 1))


@pytest.mark.parametrize('zero_copy_tracks', [2048, 0])
@pytest.mark.parametrize('n', [1, 2, 255, 256, 257, 600, 1025])
def test_find_occluded_vs_oracle(ctx, n, zero_copy_tracks):
    """occluded_kernel around its 256-box LDS chunk (255, 256, 257, several chunks) and on both sides of the
    n > zero_copy_tracks / 2 switch of fm_find_occluded (1025 at the default; everything at 0)."""
    boxes = _crowd(n)
    with options(ctx, zero_copy_tracks=zero_copy_tracks):
        for thresh in (0.3, 0.7):
            exp = o.find_occluded(boxes, thresh)
            if n >= 255:
                assert 0.1 * n <= exp.sum() <= 0.9 * n
            np.testing.assert_array_equal(ctx.find_occluded(boxes, thresh), exp)


def test_find_occluded_exact_threshold(ctx):
    boxes = np.array([[0., 0., 9., 9.], [3., 0., 20., 9.]])       # 70 of the first box's 100 px are covered
    assert o.find_occluded(boxes, 0.7).tolist() == [True, False] and o.find_occluded(boxes, 0.71).tolist() == [False, False]
    assert ctx.find_occluded(boxes, 0.7).tolist() == [True, False]
    assert ctx.find_occluded(boxes, 0.71).tolist() == [False, False]


@pytest.mark.parametrize('shape', [(1, 1), (3, 85), (16, 16), (257, 1), (50, 70)])
def test_iou_dist_equals_oracle(ctx, shape):
    """fm_iou_dist (the tracker's duplicate removal) is the oracle's iou_dist to the bit."""
    na, nb = shape
    rng = np.random.default_rng(na * 1000 + nb)
    tl = rng.uniform(0, 600, (na, 2))
    a = np.rint(np.concatenate([tl, tl + rng.uniform(10, 200, (na, 2))], 1))
    b = np.rint(a[rng.integers(0, na, nb)] + rng.normal(0, 25, (nb, 4)))
    big, small = (b, a) if nb >= na else (a, b)         # the special rows go where there is room for them
    ref = small[0].copy()
    x0, y0, x1, y1 = ref
    special = np.array([ref,                                        # identical: 0.0
                        [x1 + 1, y0, x1 + 1 + (x1 - x0), y1],       # horizontally adjacent, iw == 0: 1.0
                        [x1, y0, x1 + (x1 - x0), y1],               # one shared pixel column
                        [x0 + 2, y0 + 2, x1 - 2, y1 - 2]])          # fully nested
    k = min(len(special), len(big))
    big[:k] = special[:k]
    exp = o.iou_dist(a, b)
    col = (exp[0, :k] if nb >= na else exp[:k, 0]).tolist()
    w, h = x1 - x0 + 1, y1 - y0 + 1
    assert col == [0.0, 1.0, 1. - h / (2 * w * h - h), 1. - (w - 4) * (h - 4) / (w * h)][:k]
    np.testing.assert_array_equal(ctx.iou_dist(a, b), exp)


CASCADE_WAYS = {'mirror': (dict(), False),                                        # host fill, host solvers
                'device': (dict(host_lap_elems=0), False),                        # cost kernel, device LAP, device greedy
                'blit': (dict(host_lap_elems=0, zero_copy_tracks=0), False),      # the same through blit copies
                'per_stage': (dict(), True)}                 # cost kernel into pinned memory, host LAP, device greedy


@pytest.mark.parametrize('nT,nD', [(7, 90), (50, 50), (90, 7)])       # lap_kernel (> 64 columns), lap64_kernel, transposed
@pytest.mark.parametrize('way', list(CASCADE_WAYS))
def test_cascade_every_way_equals_host_cascade_on_device_terms(ctx, way, nT, nD):
    """Every way the one cascade (fm_assoc_cascade) can run gives fm_cascade_host's result on the three matrices read
    back from the device: on the page-locked mirror pairwise_kernel writes beside its device arrays, and stage by stage
    on the device terms.  A prepare on other detections goes first, so a term that failed to reach the mirror would be
    a stale one, not the right one by chance."""
    opts, per_stage = CASCADE_WAYS[way]
    rng = np.random.default_rng(74 + nT)
    ctx.kf_configure(1 / 30., **KF_DEFAULT)
    ctx.set_frame_rect([0., 0., 1919., 1079.])
    case = cascade_cases.make_case(rng, nT, nD, nT // 4, False)
    _, _, _, _, tlab, dlab, docc, groups, active, unconf, hist_rows, hist_labels, det_conf, p = case
    tl = rng.uniform(0, 1500, (nT, 2))
    tb = np.rint(np.concatenate([tl, tl + rng.uniform(30, 200, (nT, 2))], 1))
    XA = rng.normal(0, 1, (nT, 512)).astype(np.float32)
    XA /= np.linalg.norm(XA, axis=1, keepdims=True)
    slots = load_tracks(ctx, XA)
    ctx.feat_reset(slots[::5])
    ctx.trk_create(slots, tb)
    H = np.eye(3) + rng.normal(0, 1e-3, (3, 3))
    for it in range(2):
        m, _ = ctx.trk_get_state(slots)
        ctx.trk_step(slots, H, np.rint(m[:, :4] + rng.normal(0, 3, (nT, 4))), rng.random(nT) < 0.7, rng.uniform(1, 6, nT))
    tb = np.rint(ctx.trk_get_state(slots)[0][:, :4])
    sel = rng.integers(0, nT, nD)
    db = np.rint(tb[sel] + rng.normal(0, 6, (nD, 4)))
    XB = (XA[sel] + rng.normal(0, 0.03, (nD, 512))).astype(np.float32)
    XB /= np.linalg.norm(XB, axis=1, keepdims=True)
    mirror = 'host_lap_elems' not in opts
    flat = [r for g in groups for r in g]
    pack = ctx.cascade_pack([len(g) for g in groups], flat, [active[r] for r in flat], unconf, hist_rows, hist_labels,
                            det_conf, p['motion_weight'], p['max_assoc_cost'], p['fill_val'], p['max_iou_cost'],
                            p['conf_thresh'], p['max_reid_cost'], per_stage=per_stage)
    with options(ctx, **opts):
        ctx.emb_upload(np.roll(XB, 1, axis=0))
        assert ctx.assoc_prepare(_lib.METRIC_COSINE, slots, tb, tlab, db[::-1] + 300., dlab, docc) == mirror
        ctx.emb_upload(XB)
        assert ctx.assoc_prepare(_lib.METRIC_COSINE, slots, tb, tlab, db, dlab, docc) == mirror
        got = cascade_cases.unpack(ctx.assoc_cascade(pack))
    feat, maha, iou = ctx.assoc_get_pairwise(nT, nD)
    has_feat = ctx.feat_read(slots)[1] > 0
    assert not has_feat.all() and has_feat.any()
    ref = cascade_cases.run_host(feat, maha, iou, has_feat, tlab, dlab, docc, groups, active, unconf, hist_rows,
                                 hist_labels, det_conf, p)
    assert len(ref[0]) >= 3 and (maha <= CHI_SQ_INV_95).any() and (maha > CHI_SQ_INV_95).any()
    assert ref[2] and ref[3], 'the greedy re-identification must have something to match and something to leave'
    assert got[0] == ref[0], 'matches'
    assert got[1] == ref[1], 'unmatched track order'
    assert got[2] == ref[2], 're-identification'
    assert got[3] == ref[3], 'new-track detections order'


def test_reid_stage_f32_rows(ctx):
    rng = np.random.default_rng(8)
    ctx.kf_configure(1 / 30., **KF_DEFAULT)
    nt, nd = 20, 15
    XA = rng.normal(0, 1, (nt, 512)).astype(np.float32); XA /= np.linalg.norm(XA, axis=1, keepdims=True)
    XB = rng.normal(0, 1, (nd, 512)).astype(np.float32); XB /= np.linalg.norm(XB, axis=1, keepdims=True)
    XB[:5] = XA[3:8] + rng.normal(0, 0.01, (5, 512)).astype(np.float32)
    slots = load_tracks(ctx, XA)
    boxes = np.tile(np.array([10., 10., 60., 200.]), (nt, 1))
    ctx.trk_create(slots, boxes)
    for metric, mid in (('cosine', _lib.METRIC_COSINE), ('euclidean', _lib.METRIC_EUCLIDEAN)):
        ctx.emb_upload(XB)
        ctx.assoc_prepare(mid, slots, boxes, np.ones(nt, int), np.tile(boxes[0], (nd, 1)), np.ones(nd, int),
                          np.zeros(nd, bool), trk_feat_f32=np.ones(nt, bool))
        labels = np.ones(nt, int); labels[4] = 0
        m_rows, m_cols, _, cost = ctx.assoc_stage(_lib.STAGE_REID, _lib.SOLVER_GREEDY, np.arange(nt), np.arange(nd),
                                                  max_cost=0.6, row_labels=labels, want_cost=True)
        exp = o.gate_cost(o.cdist(XA, XB, metric), labels, np.ones(nd, int))
        np.testing.assert_allclose(cost, exp, rtol=0, atol=1e-13)
        em, _, _ = o.greedy_match(exp, 0.6)
        assert list(zip(m_rows.tolist(), m_cols.tolist())) == em


def _check_lap(ctx, cost):
    r, c = ctx.lap(cost)
    er, ec = o.lsa(cost)
    np.testing.assert_array_equal(r, er)
    np.testing.assert_array_equal(c, ec)


@pytest.mark.parametrize('host_lap_elems', [262144, 0])
def test_lap_matches_scipy_exactly(ctx, host_lap_elems):
    """Host solver for small matrices (default) and the device kernels (lap64_kernel: n <= 64 in
    registers, lap_kernel: LDS / global work arrays) all reproduce SciPy's (rows, cols) exactly."""
    ctx.set_option('host_lap_elems', host_lap_elems)
    try:
        _lap_cases(ctx)
    finally:
        ctx.set_option('host_lap_elems', 262144)


def _lap_cases(ctx):
    rng = np.random.default_rng(0)
    for trial in range(200):
        nr, nc = rng.integers(1, 40, 2)
        kind = trial % 4
        if kind == 0:
            cost = rng.uniform(0, 1, (nr, nc))
        elif kind == 1:
            cost = rng.integers(0, 4, (nr, nc)).astype(float)          # massive ties
        elif kind == 2:
            cost = np.round(rng.uniform(0, 1, (nr, nc)), 1)
            cost[rng.random((nr, nc)) < 0.5] = 1e5                       # gated entries
        else:
            cost = np.full((nr, nc), 1e5)                                # everything gated
            cost[rng.random((nr, nc)) < 0.1] = 0.3
        _check_lap(ctx, cost)
    # register-resident kernel boundary (n <= 64) with massive ties
    for shape in ((64, 64), (64, 30), (30, 64), (63, 64), (64, 65), (65, 64), (50, 50), (64, 1), (1, 64)):
        for ties in (False, True):
            cost = rng.integers(0, 3, shape).astype(float) if ties else rng.uniform(0, 1, shape)
            _check_lap(ctx, cost)
    for shape in ((1, 1), (1, 300), (300, 1), (128, 128), (300, 300), (150, 420), (420, 150), (700, 700)):
        cost = rng.uniform(0, 1, shape)
        cost[rng.random(shape) < 0.3] = 1e5
        _check_lap(ctx, cost)


def _gated_uniform(rng, shape):
    cost = rng.uniform(0, 1, shape)
    cost[rng.random(shape) < 0.3] = 1e5
    return cost


@pytest.mark.parametrize('shape', [(2, 5000), (5000, 3), (2, 3000), (8, 3000)])
def test_lap_kernel_large_modes(ctx, shape):
    """lap_kernel where 700 x 700 (work arrays in 33 KiB of LDS) does not take it: (2, 5000) and (5000, 3) need
    156 KiB of work arrays, which stay in global memory (lds_mode 0); (2, 3000) runs with 141 KiB of LDS, cost matrix
    included (mode 2), and (8, 3000) with 94 KiB of work arrays and the matrix in global memory (mode 1) -- both above
    the 64 KiB a kernel gets without hipFuncSetAttribute."""
    rng = np.random.default_rng(shape[0] + shape[1])
    with options(ctx, host_lap_elems=0):
        _check_lap(ctx, _gated_uniform(rng, shape))


def test_lap_and_greedy_results_by_blit(ctx):
    """zero_copy_tracks=0: run_lap / run_greedy write to device memory and the result comes back by a copy."""
    rng = np.random.default_rng(12)
    with options(ctx, host_lap_elems=0, zero_copy_tracks=0):
        for shape in ((64, 64), (65, 64), (128, 128), (150, 420)):
            _check_lap(ctx, _gated_uniform(rng, shape))
        cost = rng.uniform(0, 1, (300, 280))
        r, c = ctx.greedy(cost, 0.5)
        em, _, _ = o.greedy_match(cost, 0.5)
        assert list(zip(r.tolist(), c.tolist())) == em


@pytest.mark.parametrize('host_lap_elems', [262144, 0])
@pytest.mark.parametrize('shape', [(5, 7), (70, 80)])
def test_lap_infinite_costs(ctx, shape, host_lap_elems):
    """+inf entries on the host solver, lap64_kernel (5 x 7) and lap_kernel (70 x 80): a matrix that stays feasible is
    solved like SciPy solves it; one with a row of +inf only is refused, where SciPy raises ValueError."""
    rng = np.random.default_rng(shape[0])
    nr, nc = shape
    cost = rng.uniform(0, 1, shape)
    holes = rng.random(shape) < 0.4
    holes[np.arange(nr), rng.permutation(nc)[:nr]] = False       # an assignment without +inf exists
    cost[holes] = np.inf
    bad = cost.copy()
    bad[nr // 2] = np.inf
    with pytest.raises(ValueError):
        o.lsa(bad)
    with options(ctx, host_lap_elems=host_lap_elems):
        _check_lap(ctx, cost)
        with pytest.raises(_lib.FastMOTHipError, match='infeasible'):
            ctx.lap(bad)
        _check_lap(ctx, cost)                                     # and the refusal leaves nothing behind


def test_greedy_matches_reference_semantics(ctx):
    rng = np.random.default_rng(1)
    for trial in range(100):
        nr, nc = rng.integers(1, 30, 2)
        cost = np.round(rng.uniform(0, 1, (nr, nc)), 1 if trial % 2 else 6)
        thr = float(rng.uniform(0.1, 0.9))
        r, c = ctx.greedy(cost, thr)
        em, _, _ = o.greedy_match(cost, thr)
        assert list(zip(r.tolist(), c.tolist())) == em
    cost = rng.uniform(0, 1, (300, 280))
    r, c = ctx.greedy(cost, 0.5)
    em, _, _ = o.greedy_match(cost, 0.5)
    assert list(zip(r.tolist(), c.tolist())) == em


def test_average_feature_kernel(ctx):
    rng = np.random.default_rng(3)
    slots = np.array([5, 9, 2])
    ctx.feat_reset(slots)
    state = {int(s): None for s in slots}
    for step in range(1, 6):
        embs = rng.normal(0, 1, (3, 512)).astype(np.float32)
        embs /= np.linalg.norm(embs, axis=1, keepdims=True)
        ctx.emb_upload(embs)
        ctx.feat_update(slots, [2, 0, 1])
        for s, row in zip(slots, [2, 0, 1]):
            if state[int(s)] is None:
                state[int(s)] = (embs[row].copy(), embs[row].copy())
            else:
                state[int(s)] = o.average_feature(state[int(s)][0], embs[row], step)
            fsum, avg, cnt = ctx.feat_get(int(s))
            assert cnt == step
            np.testing.assert_allclose(fsum, state[int(s)][0], rtol=0, atol=1e-6)
            np.testing.assert_allclose(avg, state[int(s)][1], rtol=0, atol=1e-6)
    ctx.feat_merge(5, 9)
    fsum, avg, cnt = ctx.feat_get(5)
    s2, a2 = o.average_feature(state[5][0], state[9][0], 10)
    assert cnt == 10
    np.testing.assert_allclose(avg, a2, atol=1e-6)


def test_feature_update_by_blit(ctx):
    """fm_feat_update with its slot / row lists copied to the device (zero_copy_tracks=0); five tracks: the second
    block of feat_update_kernel has one live wave."""
    rng = np.random.default_rng(4)
    slots = np.array([7, 3, 12, 1, 9])
    embs = rng.normal(0, 1, (2, 5, 512)).astype(np.float32)
    embs /= np.linalg.norm(embs, axis=2, keepdims=True)
    rows = [[4, 2, 0, 1, 3], [1, 0, 3, 4, 2]]
    with options(ctx, zero_copy_tracks=0):
        ctx.feat_reset(slots)
        for e, r in zip(embs, rows):
            ctx.emb_upload(e)
            ctx.feat_update(slots, r)
        got = [ctx.feat_get(int(s)) for s in slots]
    for k, (fsum, avg, cnt) in enumerate(got):
        esum, eavg = o.average_feature(embs[0][rows[0][k]], embs[1][rows[1][k]], 2)
        assert cnt == 2
        np.testing.assert_allclose(fsum, esum, rtol=0, atol=1e-6)
        np.testing.assert_allclose(avg, eavg, rtol=0, atol=1e-6)
