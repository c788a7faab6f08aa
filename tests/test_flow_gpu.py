"""GPU parity of the KLT stage (flow.hip + flow_estimate.hip) against oracle=restated
(oracle/cv_oracle.py: OpenCV algorithms restated in numpy -- the reference delegates this stage
to OpenCV, which is not available, so parity here is pinned only between restatement and kernels;
SURVEY.md section 8c).  Integer image results must be IDENTICAL, and so must the LK points: the kernel
accumulates the 5x5 window sums in float32 in the same sequential (y, x) order as LKTrackerInvoker's scalar
loop and the restatement."""
import numpy as np
import pytest

import cv_oracle as cv
import scenes
from fastmot_amd import _lib
from fastmot_amd.flow import Flow
from fastmot_amd.detector import bind_frame

pytestmark = pytest.mark.gpu


def textured_frame(w, h, seed, shift=(0, 0)):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h // 6 + 8, w // 6 + 8, 3)).astype(np.uint8)
    big = np.kron(base, np.ones((6, 6, 1), np.uint8))
    big = np.clip(big.astype(int) + rng.integers(-12, 12, big.shape), 0, 255).astype(np.uint8)
    oy, ox = 12 + shift[1], 12 + shift[0]
    return np.ascontiguousarray(big[oy:oy + h, ox:ox + w])


class FakeTrack:
    def __init__(self, trk_id, tlbr, age=0):
        self.trk_id, self.age = trk_id, age
        self._tlbr = np.asarray(tlbr, float)
        self.keypoints = np.empty((0, 2), np.float32)
        self.prev_keypoints = np.empty((0, 2), np.float32)
        self.inlier_ratio = 1.

    @property
    def tlbr(self):
        return self._tlbr

    def __lt__(self, other):
        return (self.tlbr[-1], -self.age) < (other.tlbr[-1], -other.age)


def make_flow(size):
    kw = scenes.tracker_kwargs()['flow_cfg']
    return Flow(size, **vars(kw))


@pytest.mark.parametrize('bits', [14, 15])
def test_gray_both_opencv_generations(ctx, bits):
    """Flow(gray_coeff_bits=...): the gray image and everything derived from it follow the chosen OpenCV generation
    (14-bit coefficients = the default = the reference's pinned 4.1.1, 15-bit = later 4.x), both paths of the
    conversion (the fused gray + half-resolution kernel at an exact 2x scale, the plain kernel otherwise)."""
    for size, scale in (((640, 360), (0.5, 0.5)), ((600, 338), (0.4, 0.4))):
        f0 = textured_frame(*size, 5)
        kw = dict(vars(scenes.tracker_kwargs()['flow_cfg']))
        kw.update(opt_flow_scale_factor=scale, gray_coeff_bits=bits)
        flow = Flow(size, **kw)
        flow.init(f0)
        g0 = cv.bgr2gray(f0, bits)
        np.testing.assert_array_equal(ctx.flow_read_image(0), g0)
        small = cv.resize_linear_u8(g0, (round(scale[0] * size[0]), round(scale[1] * size[1])))
        np.testing.assert_array_equal(ctx.flow_read_image(2), small)
    assert (cv.bgr2gray(f0, 14) != cv.bgr2gray(f0, 15)).any()


def test_images_pyramid_lk(ctx):
    size = (640, 360)
    f0, f1 = textured_frame(*size, 1), textured_frame(*size, 1, shift=(4, 2))
    flow = make_flow(size)
    flow.init(f0)
    g0 = cv.bgr2gray(f0)
    np.testing.assert_array_equal(ctx.flow_read_image(0), g0)
    small0 = cv.resize_linear_u8(g0, (320, 180))
    np.testing.assert_array_equal(ctx.flow_read_image(2), small0)
    pyr = cv.build_pyramid(small0, 5, 5)
    for l, img in enumerate(pyr):
        np.testing.assert_array_equal(ctx.flow_read_image(2 + l), img)
    # LK on arbitrary points
    ctx.frame_upload(f1)
    ctx.flow_begin()
    ctx.flow_targets(np.zeros((0, 4)), np.zeros((0, 2), np.float32), np.zeros(1, np.int32))
    rng = np.random.default_rng(3)
    pts = np.stack([rng.uniform(-3, 323, 400), rng.uniform(-3, 183, 400)], 1).astype(np.float32)
    nxt, st, err = ctx.flow_lk(pts)
    small1 = cv.resize_linear_u8(cv.bgr2gray(f1), (320, 180))
    en, es, ee = cv.calc_optical_flow_pyr_lk(small0, small1, pts)
    np.testing.assert_array_equal(st, es)
    ok = es > 0
    # one lane per point, window sums in LKTrackerInvoker's scalar order: bit-identical to the restatement
    np.testing.assert_array_equal(nxt[ok], en[ok])
    np.testing.assert_array_equal(err[ok], ee[ok])
    assert ok.mean() > 0.7
    # the dominant motion is the shift (-4, -2)/2 in the half-resolution frame
    med = np.median((nxt - pts)[ok], axis=0)
    np.testing.assert_allclose(med, [-2, -1], atol=0.1)


def test_targets_gftt_fast(ctx):
    size = (640, 360)
    f0 = textured_frame(*size, 5)
    flow = make_flow(size)
    flow.init(f0)
    g0 = cv.bgr2gray(f0)
    rects = np.array([[100, 200, 180, 359], [150, 120, 230, 300], [400, 50, 460, 200], [0, 0, 50, 90]], float)
    kps = np.array([[120.4, 250.2], [160., 210.], [200., 150.], [155., 250.], [420.6, 60.5], [700., 10.]], np.float32)
    off = np.array([0, 2, 4, 6, 6], np.int32)
    area, keep = ctx.flow_targets(rects, kps, off)
    mask = np.full((360, 640), 255, np.uint8)
    exp_area, exp_keep = [], []
    for k, r in enumerate(rects.astype(int)):
        crop = mask[r[1]:r[3] + 1, r[0]:r[2] + 1]
        exp_area.append(int((crop != 0).sum()))
        for p in kps[off[k]:off[k + 1]]:
            x, y = int(np.rint(p[0])), int(np.rint(p[1]))
            inside = r[0] <= x <= r[2] and r[1] <= y <= r[3]
            exp_keep.append(bool(inside and mask[y, x] == 255))
        masks_k = crop.copy() if k == 1 else None
        if k == 1:
            mask1 = masks_k
        crop[:] = 0
    np.testing.assert_array_equal(area, exp_area)
    np.testing.assert_array_equal(keep, exp_keep)
    # GFTT on track 1 (partly occluded by track 0) and track 2
    pts, cnt = ctx.flow_detect([1, 2], rects[[1, 2]], [6, 5], cap=1000)
    for i, (k, md) in enumerate(((1, 6), (2, 5))):
        r = rects[k].astype(int)
        m = np.full((r[3] - r[1] + 1, r[2] - r[0] + 1), 255, np.uint8) if k == 2 else mask1
        exp = cv.good_features_to_track(g0[r[1]:r[3] + 1, r[0]:r[2] + 1], m, 1000, 0.06, md)
        exp = exp + np.array(r[:2], np.float32)
        c = (rects[k][:2] + rects[k][2:]) / 2
        ax = (rects[k][2:] - rects[k][:2] + 1) * 0.5
        exp = exp[(((exp - c) / ax) ** 2).sum(1) <= 1.]
        got = pts[i, :cnt[i]]
        assert len(got) == len(exp) and len(exp) > 3
        np.testing.assert_array_equal(got, exp)
    # background FAST keypoints under the final mask
    bg = ctx.flow_background()
    bg_img = cv.resize_linear_u8(g0, (64, 36))
    np.testing.assert_array_equal(ctx.flow_read_image(20), bg_img)
    kp = cv.fast_detect(bg_img, 10)
    mask_small = cv.resize_nearest(mask, (64, 36))
    kp = kp[[mask_small[int(p[1] + 0.5), int(p[0] + 0.5)] != 0 for p in kp]]
    np.testing.assert_array_equal(bg, kp)
    assert len(kp) > 10


def mask_bookkeeping(size, rects, kps, off):
    """The reference's foreground mask, zeroed rect by rect (flow.py:163-169): -> (area of every track = non-zero mask
    pixels of its crop, keep flag of every propagated keypoint = _rect_filter, the crops' masks, the final mask)."""
    mask = np.full((size[1], size[0]), 255, np.uint8)
    area, keep, masks = [], [], []
    for k, r in enumerate(np.asarray(rects).astype(int)):
        crop = mask[r[1]:r[3] + 1, r[0]:r[2] + 1]
        area.append(int((crop != 0).sum()))
        for p in kps[off[k]:off[k + 1]]:
            x, y = int(np.rint(p[0])), int(np.rint(p[1]))
            inside = r[0] <= x <= r[2] and r[1] <= y <= r[3]
            keep.append(bool(inside and mask[y, x] == 255))
        masks.append(crop.copy())
        crop[:] = 0
    return np.array(area), np.array(keep, bool), masks, mask


def edge_targets():
    """49 rects for the seams of the mask bookkeeping and the tiled corner kernel -> (rects, kps, kp_off, keep expected
    of the keypoints).  Rects 0 .. 39 overlap up to ten earlier ones each (prepare_kernel's 64-column words, one ragged
    word per row); rect 40 is overlapped by all 40 -- more than the OV_LDS = 32 rects the kernels keep in LDS: the
    per-pixel branch over the global overlap list, 181 x 151 pixels -- and it alone has propagated keypoints.  Then crops
    one, two and three pixels wide, exactly one 32 x 32 tile, one pixel more, the frame's corners, and 64 x 8.  (Rows of
    several words under a short list: the 81 and 201 pixel wide rects of test_prepare_matches_staged_calls and
    test_no_targets_after_targets.)"""
    small = [[300 + 3 * i, 200 + 2 * i, 330 + 3 * i, 240 + 2 * i] for i in range(40)]       # 40 rects crossing the big one
    rects = np.array(small + [
        [280, 180, 460, 330],       # 40: overlapped by all 40 above
        [10, 10, 10, 40],           # 41: one pixel wide
        [20, 10, 21, 12],           # 42: 2 x 3
        [40, 10, 42, 12],           # 43: 3 x 3 (one interior pixel)
        [60, 20, 91, 51],           # 44: exactly one tile
        [100, 20, 132, 52],         # 45: 33 x 33
        [0, 0, 70, 9],              # 46: frame corner, 71 x 10
        [560, 300, 639, 359],       # 47: bottom right corner of the frame
        [200, 20, 263, 27],         # 48: 64 x 8
    ], float)
    kps = np.array([
        [310.2, 210.7], [400.4, 280.3],     # under rect 0; under rects 24 .. 33
        [447., 318.], [300., 200.],         # the last pixel of rect 39, the first of rect 0
        [285., 185.], [455.6, 325.1],       # free: near the two far corners of rect 40
        [350., 190.], [299.4, 220.],        # free: above the band of small rects, one column left of rect 0
        [279.4, 250.], [460.6, 200.],       # outside rect 40 by one column on either side (279, 461)
        [336.5, 205.],                      # rintf -> 336 (even), the last column rect 2 covers in that row; 337 is free
        [290., 330.5],                      # rintf -> 330 (even), the last row of rect 40; 331 is outside
    ], np.float32)
    off = np.zeros(len(rects) + 1, np.int32)
    off[41:] = len(kps)
    exp_keep = [False, False, False, False, True, True, True, True, False, False, False, True]
    return rects, kps, off, exp_keep


def test_gftt_edge_crops(ctx):
    """Mask bookkeeping and corner detection on the crops the kernels have to get right at their seams (edge_targets):
    one or two pixels wide, exactly one 32 x 32 tile, one pixel more than a tile, a frame corner, a crop with a strong
    min-distance (few cells), and a track overlapped by 40 earlier ones (more than the 32 rects the kernels keep in
    LDS: the global overlap list).  Area and keep flags must equal the reference's mask walked in numpy, for all 49
    rects; every corner list must equal the restated goodFeaturesToTrack on the same crop and mask (bit-identical
    points, same order)."""
    size = (640, 360)
    f0 = textured_frame(*size, 11)
    flow = make_flow(size)
    flow.init(f0)
    g0 = cv.bgr2gray(f0)
    rects, kps, off, keep_by_hand = edge_targets()
    area, keep = ctx.flow_targets(rects, kps, off)
    exp_area, exp_keep, masks, _ = mask_bookkeeping(size, rects, kps, off)
    assert exp_keep.tolist() == keep_by_hand            # (the numpy statement says what the points were placed for)
    np.testing.assert_array_equal(area, exp_area)
    np.testing.assert_array_equal(keep, exp_keep)
    assert len(area) == 49 and 0 < exp_area[40] < 181 * 151 and (exp_area[41:] == [31, 6, 9, 1024, 1089, 710, 4800, 512]).all()
    idx = list(range(40, len(rects)))
    mds = [7, 1, 1, 1, 3, 4, 2, 25, 2]
    pts, cnt = ctx.flow_detect(idx, rects[idx], mds, cap=1000)
    seen = 0
    for i, (k, md) in enumerate(zip(idx, mds)):
        r = rects[k].astype(int)
        exp = cv.good_features_to_track(g0[r[1]:r[3] + 1, r[0]:r[2] + 1], masks[k], 1000, 0.06, md)
        exp = exp.reshape(-1, 2) + np.array(r[:2], np.float32)
        c = (rects[k][:2] + rects[k][2:]) / 2
        ax = (rects[k][2:] - rects[k][:2] + 1) * 0.5
        exp = exp[(((exp - c) / ax) ** 2).sum(1) <= 1.] if len(exp) else exp
        got = pts[i, :cnt[i]]
        assert len(got) == len(exp), (k, len(got), len(exp))
        np.testing.assert_array_equal(got, exp)
        seen += len(exp)
    assert masks[40].any() and not masks[40].all() and seen > 40


def test_fast_background_ragged_raster(ctx):
    """Background FAST keypoints on a raster whose size is not a multiple of the compaction's 256-pixel segments
    (65 x 37 = 2405), under a mask of three tracks: same keypoints, same raster order as the restatement."""
    size = (650, 370)
    f0 = textured_frame(*size, 21)
    flow = make_flow(size)
    flow.init(f0)
    g0 = cv.bgr2gray(f0)
    rects = np.array([[100, 100, 300, 300], [0, 0, 60, 369], [500, 20, 649, 120]], float)
    ctx.flow_targets(rects, np.empty((0, 2), np.float32), np.zeros(4, np.int32))
    mask = np.full((size[1], size[0]), 255, np.uint8)
    for r in rects.astype(int):
        mask[r[1]:r[3] + 1, r[0]:r[2] + 1] = 0
    bg = ctx.flow_background()
    bw, bh = int(size[0] * 0.1), int(size[1] * 0.1)
    assert (bw * bh) % 256 != 0
    bg_img = cv.resize_linear_u8(g0, (bw, bh))
    kp = cv.fast_detect(bg_img, 10)
    mask_small = cv.resize_nearest(mask, (bw, bh))
    kp = kp[[mask_small[int(p[1] + 0.5), int(p[0] + 0.5)] != 0 for p in kp]]
    np.testing.assert_array_equal(bg, kp)
    assert len(kp) > 10


def test_estimate_vs_oracle(ctx):
    rng = np.random.default_rng(9)
    size = (640, 360)
    Htrue = np.array([[1.002, 0.001, 3.0], [-0.0015, 0.999, -2.0], [1e-6, -2e-6, 1.]])
    n_bg = 150
    bgp = np.stack([rng.uniform(0, 640, n_bg), rng.uniform(0, 360, n_bg)], 1)
    q = np.c_[bgp, np.ones(n_bg)] @ Htrue.T
    bgc = q[:, :2] / q[:, 2:] + rng.normal(0, 0.3, (n_bg, 2))
    bgc[::7] += rng.normal(0, 25, bgc[::7].shape)           # outliers
    tracks = np.array([[100, 100, 160, 280], [140, 120, 200, 300], [400, 60, 450, 200], [300, 300, 340, 359]], float)
    prev, cur, begins, ends = [], [], [], []
    for k, t in enumerate(tracks):
        n = [40, 30, 25, 2][k]
        p = np.stack([rng.uniform(t[0], t[2], n), rng.uniform(t[1], t[3], n)], 1)
        c = p * 1.01 + np.array([5., -3.]) + rng.normal(0, 0.4, (n, 2))
        c[::6] += rng.normal(0, 15, c[::6].shape)
        begins.append(len(np.concatenate(prev)) if prev else 0)
        prev.append(p); cur.append(c)
        ends.append(begins[-1] + n)
    prev.append(bgp); cur.append(bgc)
    P = np.concatenate(prev).astype(np.float32); Cc = np.concatenate(cur).astype(np.float32)
    status = rng.random(len(P)) > 0.05
    args = (P, Cc, status, np.array(begins, np.int32), np.array(ends, np.int32), ends[-1], len(P) - 1, tracks,
            size, 500, 0.99, 4)
    H, res, est, nm, inl = ctx.flow_estimate(*args)
    eH, eres, eest, enm, einl = cv.flow_estimate(*args)
    assert H is not None and eH is not None
    np.testing.assert_array_equal(res, eres)
    np.testing.assert_array_equal(nm, enm)
    np.testing.assert_array_equal(inl, einl)
    np.testing.assert_array_equal(est, eest)
    np.testing.assert_allclose(H, eH, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(H, Htrue, atol=5e-2, rtol=5e-2)
    assert list(res) == [1, 1, 1, 0]


def test_flow_predict_moving_scene(ctx):
    """End to end: Flow.predict on a synthetic camera pan -> boxes follow the motion."""
    size = (640, 360)
    flow = make_flow(size)
    f0 = textured_frame(*size, 11)
    f1 = textured_frame(*size, 11, shift=(6, -4))      # content moves by (-6, +4) px
    flow.init(f0)
    tracks = [FakeTrack(1, [100, 100, 170, 300]), FakeTrack(2, [300, 50, 380, 330], age=1), FakeTrack(3, [500, 20, 560, 180])]
    boxes, H = flow.predict(f1, tracks)
    assert H is not None and len(boxes) == 3
    np.testing.assert_allclose(H, [[1, 0, -6], [0, 1, 4], [0, 0, 1]], atol=0.05)
    for t in tracks:
        np.testing.assert_allclose(boxes[t.trk_id], t.tlbr + np.array([-6, 4, -6, 4]), atol=1.01)
        assert len(t.keypoints) >= 4 and 0 < t.inlier_ratio <= 1
    # second call reuses propagated keypoints (no GFTT) and still tracks
    f2 = textured_frame(*size, 11, shift=(12, -8))
    for t in tracks:
        t._tlbr = boxes[t.trk_id]
    boxes2, H2 = flow.predict(f2, tracks)
    assert H2 is not None and len(boxes2) == 3
    np.testing.assert_allclose(H2, [[1, 0, -6], [0, 1, 4], [0, 0, 1]], atol=0.05)


def test_prepare_matches_staged_calls(ctx):
    """fm_flow_prepare (one round trip) == fm_flow_targets + fm_flow_detect + fm_flow_background.  Both run the same
    bookkeeping kernel, so area and keep flags are also held against the reference's mask walked in numpy -- for the
    four rects here and for the 49 of edge_targets."""
    size = (640, 360)
    f0 = textured_frame(*size, 21)
    flow = make_flow(size)
    flow.init(f0)
    rects = np.array([[100, 200, 180, 359], [150, 120, 230, 300], [400, 50, 460, 200], [0, 0, 50, 90]], float)
    rng = np.random.default_rng(4)
    kps, off = [], [0]
    for k, r in enumerate(rects):
        n = [0, 3, 120, 5][k]
        kps.append(np.stack([rng.uniform(r[0] - 5, r[2] + 5, n), rng.uniform(r[1] - 5, r[3] + 5, n)], 1))
        off.append(off[-1] + n)
    kps = np.concatenate(kps).astype(np.float32)
    off = np.array(off, np.int32)
    area0, keep0 = ctx.flow_targets(rects, kps, off)
    kept = [int(keep0[off[k]:off[k + 1]].sum()) for k in range(4)]
    needy0 = [kept[k] < 0.005 * area0[k] for k in range(4)]
    idx = [k for k in range(4) if needy0[k]]
    md = [max(round(np.sqrt(area0[k]) * 0.06), 1) for k in idx]
    pts0, cnt0 = ctx.flow_detect(idx, rects[idx], md, cap=1000)
    bg0 = ctx.flow_background()
    area, keep, needy, new_pts, new_off, new_cnt, bg = ctx.flow_prepare(rects, rects, kps, off, 0.005, 0.06)
    np.testing.assert_array_equal(area, area0)
    np.testing.assert_array_equal(keep, keep0)
    np.testing.assert_array_equal(needy, needy0)
    np.testing.assert_array_equal(bg, bg0)
    assert needy.tolist() == [True, True, False, True]
    for i, k in enumerate(idx):
        np.testing.assert_array_equal(new_pts[new_off[k]:new_off[k] + new_cnt[k]], pts0[i, :cnt0[i]])
    exp_area, exp_keep, _, _ = mask_bookkeeping(size, rects, kps, off)
    np.testing.assert_array_equal(area, exp_area)
    np.testing.assert_array_equal(keep, exp_keep)
    assert exp_keep.any() and not exp_keep.all() and exp_area[1] < 81 * 181      # (rect 1: two words per row under rect 0)
    # the seams: 49 rects, the keypoints of rect 40
    rects, kps, off, _ = edge_targets()
    area0, keep0 = ctx.flow_targets(rects, kps, off)
    area, keep, needy = ctx.flow_prepare(rects, rects, kps, off, 0.005, 0.06)[:3]
    exp_area, exp_keep, _, _ = mask_bookkeeping(size, rects, kps, off)
    np.testing.assert_array_equal(area, exp_area)
    np.testing.assert_array_equal(keep, exp_keep)
    np.testing.assert_array_equal(area0, exp_area)
    np.testing.assert_array_equal(keep0, exp_keep)
    kept = np.array([exp_keep[off[k]:off[k + 1]].sum() for k in range(len(rects))])
    np.testing.assert_array_equal(needy, kept < 0.005 * exp_area)


def test_many_small_targets_grow_the_buffers(ctx):
    """1000 non-overlapping 3 x 3 rects on an 8-pixel grid: more one-tile crops than the 4 * 640 * 360 / 1024 = 900 tiles
    the corner arena starts with, and an upload that outgrows the staging block's first size -- once through the staged
    calls, once through fm_flow_prepare, each on a freshly configured state.  Areas are 9, the two point lists are equal
    track by track and equal the restated goodFeaturesToTrack on every crop; an ordinary call afterwards shows that
    the grown state still works."""
    size = (640, 360)
    f0 = textured_frame(*size, 11)
    g0 = cv.bgr2gray(f0)
    n = 1000
    x0, y0 = 8 * (np.arange(n) % 80), 8 * (np.arange(n) // 80)
    rects = np.stack([x0, y0, x0 + 2, y0 + 2], 1).astype(float)
    assert rects[:, 3].max() < size[1]
    no_kps, off = np.empty((0, 2), np.float32), np.zeros(n + 1, np.int32)
    flow = make_flow(size)
    flow.init(f0)
    area0, _ = ctx.flow_targets(rects, no_kps, off)
    pts0, cnt0 = ctx.flow_detect(np.arange(n), rects, np.ones(n, np.int32), cap=4)
    flow = make_flow(size)                              # (fm_flow_configure: a new state, the arena at its first size)
    flow.init(f0)
    area, keep, needy, new_pts, new_off, new_cnt, bg = ctx.flow_prepare(rects, rects, no_kps, off, 1., 0.06)
    np.testing.assert_array_equal(area0, 9)
    np.testing.assert_array_equal(area, 9)
    assert needy.all()
    np.testing.assert_array_equal(new_cnt, cnt0)
    seen = 0
    full = np.full((3, 3), 255, np.uint8)
    for k in range(n):
        r = rects[k].astype(int)
        exp = cv.good_features_to_track(g0[r[1]:r[3] + 1, r[0]:r[2] + 1], full, 1000, 0.06, 1)
        exp = exp.reshape(-1, 2) + np.array(r[:2], np.float32)       # (a 3 x 3 crop's one candidate is its centre: inside the ellipse)
        np.testing.assert_array_equal(pts0[k, :cnt0[k]], exp, err_msg=f'staged, crop {k}')
        np.testing.assert_array_equal(new_pts[new_off[k]:new_off[k] + new_cnt[k]], exp, err_msg=f'prepare, crop {k}')
        seen += len(exp)
    assert seen > 0
    # an ordinary call on the grown state
    rects = np.array([[100, 200, 180, 359], [150, 120, 230, 300], [400, 50, 460, 200], [0, 0, 50, 90]], float)
    off = np.zeros(5, np.int32)
    area, keep, needy, new_pts, new_off, new_cnt, bg2 = ctx.flow_prepare(rects, rects, no_kps, off, 0.005, 0.06)
    exp_area, _, masks, _ = mask_bookkeeping(size, rects, no_kps, off)
    np.testing.assert_array_equal(area, exp_area)
    assert needy.all()
    for k in range(4):
        r = rects[k].astype(int)
        md = max(int(np.rint(np.sqrt(exp_area[k]) * 0.06)), 1)
        exp = cv.good_features_to_track(g0[r[1]:r[3] + 1, r[0]:r[2] + 1], masks[k], 1000, 0.06, md)
        exp = exp + np.array(r[:2], np.float32)
        c = (rects[k][:2] + rects[k][2:]) / 2
        ax = (rects[k][2:] - rects[k][:2] + 1) * 0.5
        exp = exp[(((exp - c) / ax) ** 2).sum(1) <= 1.]
        assert len(exp) > 3
        np.testing.assert_array_equal(new_pts[new_off[k]:new_off[k] + new_cnt[k]], exp)


def test_no_targets_after_targets(ctx):
    """fm_flow_targets and fm_flow_prepare with no tracks, after a call with tracks: the rects of the earlier call are
    gone from the mask, the background keypoints are the unmasked FAST keypoints of the restatement.  (The call with
    tracks has a 201 pixel wide rect under a short overlap list: four 64-column words per row, the last one ragged.)"""
    size = (640, 360)
    f0 = textured_frame(*size, 5)
    flow = make_flow(size)
    flow.init(f0)
    kp_all = cv.fast_detect(cv.resize_linear_u8(cv.bgr2gray(f0), (64, 36)), 10)
    rects = np.array([[100, 100, 300, 200], [50, 150, 250, 250], [240, 90, 400, 160], [420, 20, 620, 340]], float)
    no_kps, off = np.empty((0, 2), np.float32), np.zeros(5, np.int32)
    exp_area, _, _, mask = mask_bookkeeping(size, rects, no_kps, off)
    assert 0 < exp_area[1] < 201 * 101
    mask_small = cv.resize_nearest(mask, (64, 36))
    kp_masked = kp_all[[mask_small[int(p[1] + 0.5), int(p[0] + 0.5)] != 0 for p in kp_all]]
    assert 10 < len(kp_masked) < len(kp_all)
    none = np.zeros((0, 4)), no_kps, np.zeros(1, np.int32)
    area, _ = ctx.flow_targets(rects, no_kps, off)
    np.testing.assert_array_equal(area, exp_area)
    np.testing.assert_array_equal(ctx.flow_background(), kp_masked)
    area, _ = ctx.flow_targets(*none)
    assert len(area) == 0
    np.testing.assert_array_equal(ctx.flow_background(), kp_all)
    res = ctx.flow_prepare(rects, rects, no_kps, off, 0.005, 0.06)
    np.testing.assert_array_equal(res[0], exp_area)
    np.testing.assert_array_equal(res[6], kp_masked)
    res = ctx.flow_prepare(none[0], none[0], no_kps, none[2], 0.005, 0.06)
    assert len(res[0]) == 0
    np.testing.assert_array_equal(res[6], kp_all)
    np.testing.assert_array_equal(ctx.flow_background(), kp_all)


@pytest.mark.parametrize('hammer', ['liteconv', 'osnet'])
def test_lk_deterministic_while_other_streams_are_busy(ctx, hammer):
    """LK on constant inputs must reproduce its idle result bit for bit while another host thread keeps the CUs busy
    with the ReID network's kernels -- an ORDINARY launch (4-point workgroups, no whole-CU request, no ordering).

    History: rounds 1-2 saw single points change by 1e-5 .. 6 px in up to 70 % of such calls, traced it to the two
    fused LightConv kernels being resident on the same CU, and shipped isolation / ordering around an unknown cause.
    Round 3 captured disturbed calls (scripts/lk_bisect.py): the packed-fp32 form the compiler had chosen for the
    position update returned a wrong low half in lanes 48..63 (the head of csrc/lk_core.h, csrc/diag.hip); without
    packed fp32 in the KLT kernels 0 of 5.1 M iterations disagree under the same load."""
    import threading
    from fastmot_amd.detector import DeviceFrame
    from fastmot_amd.engine import HipNet, NET_EXTRACTOR
    from fastmot_amd.models import ReID
    from fastmot_amd.models.graph import Graph, RandomWeights
    from synthetic import SyntheticVideo
    size = (960, 540)
    video = SyntheticVideo(size, n_ids=6, n_frames=2, seed=4)
    ctx.frame_configure(size[0], size[1], 2)
    for i in range(2):
        ctx.frame_ring_store(i, video.frames[i])
    flow = Flow(size)
    flow.init(DeviceFrame(0))
    bind_frame(ctx, DeviceFrame(1), size)
    ctx.flow_begin()
    ctx.synchronize()
    ctx.feat_configure(512)
    if hammer == 'liteconv':
        g = Graph(RandomWeights(seed=1), (64, 32), 16)
        params = [g.lightconv_params(f'p{i}', 16) for i in range(4)]
        g.lightconv_group('l', [g.input] * 4, params)
    else:
        g, _ = ReID.get_model('OSNet025').build_graph(RandomWeights(seed=1))
    net = HipNet(ctx, NET_EXTRACTOR, g, 50, reuse_buffers=True)
    net.run(50)                                          # (graph capture happens here, not beside the copies below)
    ctx.synchronize()
    rng = np.random.default_rng(0)
    pts = np.stack([rng.uniform(20, size[0] / 2 - 20, 600), rng.uniform(20, size[1] / 2 - 20, 600)], 1).astype(np.float32)
    base = [ctx.flow_lk(pts), ctx.flow_lk(pts)]          # the second call tracks in the opposite direction
    stop = []

    def hammer_loop():
        ctx.bind_thread()
        while not stop:
            net.run(50)
            ctx.synchronize()
    th = threading.Thread(target=hammer_loop)
    th.start()
    try:
        bad = 0
        for r in range(100):
            for k in range(2):
                nxt, st, _ = ctx.flow_lk(pts)
                ok = np.array_equal(st, base[k][1]) and np.array_equal(nxt[st > 0], base[k][0][st > 0])
                bad += not ok
    finally:
        stop.append(1)
        th.join()
        net.close()
    assert bad == 0


def test_lk_beside_the_detector(ctx):
    """... and while the DETECTOR network -- every conv kernel variant YOLOv4@608 uses, the LDS-halo and two-pixel-tile
    streamed convs of late round 2 included (they were switched off then because this test failed with them) -- runs on
    another stream."""
    import threading
    from fastmot_amd.detector import DeviceFrame
    from fastmot_amd.engine import HipNet, NET_DETECTOR
    from fastmot_amd.models import YOLO
    from synthetic import SyntheticVideo
    size = (960, 540)
    video = SyntheticVideo(size, n_ids=6, n_frames=2, seed=4)
    ctx.frame_configure(size[0], size[1], 2)
    for i in range(2):
        ctx.frame_ring_store(i, video.frames[i])
    flow = Flow(size)
    flow.init(DeviceFrame(0))
    bind_frame(ctx, DeviceFrame(1), size)
    ctx.flow_begin()
    ctx.synchronize()
    g, _ = YOLO.get_model('YOLOv4_608').build_graph()
    net = HipNet(ctx, NET_DETECTOR, g, 1, reuse_buffers=True)
    net.run(1)                                           # (graph capture happens here, not beside the copies below)
    ctx.synchronize()
    rng = np.random.default_rng(0)
    pts = np.stack([rng.uniform(20, size[0] / 2 - 20, 600), rng.uniform(20, size[1] / 2 - 20, 600)], 1).astype(np.float32)
    stop = []

    def hammer_loop():
        ctx.bind_thread()
        while not stop:
            net.run(1)
            ctx.synchronize()
    try:
        base = [ctx.flow_lk(pts), ctx.flow_lk(pts)]      # the second call tracks in the opposite direction
        th = threading.Thread(target=hammer_loop)
        th.start()
        try:
            bad = 0
            for r in range(150):
                for k in range(2):
                    nxt, st, _ = ctx.flow_lk(pts)
                    ok = np.array_equal(st, base[k][1]) and np.array_equal(nxt[st > 0], base[k][0][st > 0])
                    bad += not ok
        finally:
            stop.append(1)
            th.join()
    finally:
        net.close()
    assert bad == 0, f'{bad} of 300 LK calls differ beside the detector network'
