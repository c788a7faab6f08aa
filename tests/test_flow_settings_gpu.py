"""The KLT stage (flow.hip + flow_estimate.hip) at the settings its defaults never reach: the other LK window and
pyramid depths, other termination criteria, the plain (not fused) pyramid path, blockSize 5, the three selection paths
of gftt_select_kernel and its limits, Flow.predict end to end at a non-default configuration.

Oracle: oracle/cv_oracle.py called with the same parameters.  The kernels claim bit-identity with it, so every
comparison is assert_array_equal (the homography of the end-to-end test: that test's own rtol 1e-6 for the host's double
arithmetic, as in tests/test_fullsize_gpu.py).  Floors that keep a degenerate input from passing are asserted on the
ORACLE's output, never on the kernel's."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import cpu_tracker
import cv_oracle as cv
import scenes
from fastmot_amd._lib import FastMOTHipError
from fastmot_amd.flow import Flow

pytestmark = pytest.mark.gpu

FM_ERR_ARG = -2
GFTT_MAX_CAND, GFTT_MAX_CELLS, GFTT_MAX_CORNERS = 4096, 1536, 1024      # csrc/flow.hip


# ---- helpers of tests/test_flow_gpu.py (copies)
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


def make_flow(size, scale=(0.5, 0.5), win=5, max_level=5, criteria=(3, 10, 0.03), block=3, max_corners=1000,
              quality=0.06, **over):
    kw = dict(vars(scenes.tracker_kwargs()['flow_cfg']))
    kw.update(opt_flow_scale_factor=scale,
              obj_feat_params=SimpleNamespace(maxCorners=max_corners, qualityLevel=quality, blockSize=block),
              opt_flow_params=SimpleNamespace(winSize=(win, win), maxLevel=max_level, criteria=criteria))
    kw.update(over)
    return Flow(size, **kw)


def small_size(size, scale):
    return round(scale[0] * size[0]), round(scale[1] * size[1])


@functools.lru_cache(maxsize=None)
def frame_pair(size, scale, seed, shift):
    """-> (f0, f1, small0, small1): two textured frames `shift` apart and their optical-flow images (oracle side)."""
    f0, f1 = textured_frame(*size, seed), textured_frame(*size, seed, shift=shift)
    sz = small_size(size, scale)
    out = f0, f1, cv.resize_linear_u8(cv.bgr2gray(f0), sz), cv.resize_linear_u8(cv.bgr2gray(f1), sz)
    for a in out:
        a.setflags(write=False)
    return out


def random_points(w, h, n, seed=3):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-3, w + 3, n), rng.uniform(-3, h + 3, n)], 1).astype(np.float32)


def seam_points(w, h, levels):
    """60 points placed where random ones do not fall: the columns around x = 256 at level 0 (the 256-thread block
    boundary of pyr_level_kernel; the image centre when the image is narrower), the first and last two
    rows and columns, the four corner pixels, and the centre of the coarsest level with its four neighbours there."""
    x0 = 254.5 if w > 260 else w / 2 - 1.5
    pts = [(x0 + 0.5 * i, y) for i in range(7) for y in (1.25, h * 0.3, h / 2 + 0.5, h * 0.8, h - 2.25)]
    pts += [(x, y) for x in (0, 1, w - 2, w - 1) for y in (h * 0.25, h * 0.6 + 0.5)]
    pts += [(x, y) for y in (0, 1, h - 2, h - 1) for x in (w * 0.25, w * 0.7 + 0.5)]
    pts += [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]
    step = float(1 << (levels - 1))
    pts += [(w / 2 + dx * step, h / 2 + dy * step) for dx, dy in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1))]
    assert len(pts) == 60
    return np.array(pts, np.float32)


def start_pair(ctx, flow, f0, f1):
    """Flow.init on f0, then the first half of Flow.predict on f1 with no tracks: both pyramids are on the device and
    fm_flow_lk tracks from f0 to f1 (and back on the next call: it swaps the two)."""
    flow.init(f0)
    ctx.frame_upload(f1)
    ctx.flow_begin()
    ctx.flow_targets(np.zeros((0, 4)), np.zeros((0, 2), np.float32), np.zeros(1, np.int32))


def check_levels(ctx, small, win, max_level):
    """Every pyramid level of the previous frame equals cv.build_pyramid; level `levels` does not exist.  -> levels"""
    pyr = cv.build_pyramid(small, win, max_level)
    for l, img in enumerate(pyr):
        np.testing.assert_array_equal(ctx.flow_read_image(2 + l), img, err_msg=f'level {l}')
    with pytest.raises(FastMOTHipError, match='unknown image id'):
        ctx.flow_read_image(2 + len(pyr))
    return len(pyr)


def check_lk(ctx, prev_small, next_small, pts, win, max_level, max_count, epsilon, floor=0.5):
    """One fm_flow_lk call against the restated calcOpticalFlowPyrLK: status, next points and error identical."""
    en, es, ee = cv.calc_optical_flow_pyr_lk(prev_small, next_small, pts, win, max_level, max_count, epsilon)
    if floor is not None:
        assert es.mean() > floor, es.mean()            # (the oracle's own success rate: the input is not degenerate)
    nxt, st, err = ctx.flow_lk(pts)
    ok = es > 0
    print(f'lk win {win} maxLevel {max_level} criteria ({max_count}, {epsilon}) n {len(pts)}: oracle tracks '
          f'{ok.mean():.3f}; status differs {int((st != es).sum())}, next differs {int((nxt[ok] != en[ok]).any(1).sum())} '
          f'tracked / {int((nxt[~ok] != en[~ok]).any(1).sum())} lost, err differs {int((err != ee).sum())}')
    np.testing.assert_array_equal(st, es)
    np.testing.assert_array_equal(nxt[ok], en[ok])
    np.testing.assert_array_equal(err[ok], ee[ok])
    np.testing.assert_array_equal(nxt, en)             # (lost points too: both sides leave the last estimate there)
    np.testing.assert_array_equal(err, ee)
    return en, es


# ------------------------------------------------------------------------------------------------------------------
# 1. LK instantiations and termination criteria
# ------------------------------------------------------------------------------------------------------------------
LK_CASES = {
    # name: (scale, win, maxLevel, criteria, (max_count, epsilon) the oracle gets, expected levels)
    'win3':            ((0.5, 0.5), 3, 5, (3, 10, 0.03), (10, 0.03), 6),
    'win5_7levels':    ((1, 1), 5, 7, (3, 10, 0.03), (10, 0.03), 7),
    'win3_7levels':    ((1, 1), 3, 7, (3, 10, 0.03), (10, 0.03), 7),
    'one_level':       ((0.5, 0.5), 5, 0, (3, 10, 0.03), (10, 0.03), 1),
    'three_levels':    ((0.5, 0.5), 5, 2, (3, 10, 0.03), (10, 0.03), 3),
    'count30_eps0.01': ((0.5, 0.5), 5, 5, (3, 30, 0.01), (30, 0.01), 6),
    'count1_eps0.5':   ((0.5, 0.5), 5, 5, (3, 1, 0.5), (1, 0.5), 6),
    'count_only':      ((0.5, 0.5), 5, 5, (1, 10, 0.7), (10, 0.01), 6),     # TermCriteria.COUNT: epsilon = 0.01
    'eps_only':        ((0.5, 0.5), 5, 5, (2, 3, 0.03), (30, 0.03), 6),     # TermCriteria.EPS: 30 iterations
}


@pytest.mark.parametrize('case', list(LK_CASES))
def test_lk_windows_levels_criteria(ctx, case):
    """fm_flow_lk at the window sizes, pyramid depths and termination criteria the default configuration never runs:
    `lk_pair_pre_kernel<3>` (winSize 3, at most LK_PRE = 6 levels), `lk_pair_kernel<5>` and
    `lk_pair_kernel<3>` (a pyramid deeper than LK_PRE: 7 levels of a 640 x 360 optical-flow image, scale 1, which
    also takes the plain pyramid path), one and three levels (`pyr_level_kernel` with has_next == false, no tail launch),
    the window-dependent pyramid depth (flow.hip: buildOpticalFlowPyramid's stop rule in fm_flow_configure), criteria
    with other counts / epsilons and with COUNT or EPS alone (Flow._configure: epsilon 0.01, 30 iterations).

    The 640 x 360 frame pair of test_images_pyramid_lk; three calls per case: 400 random points + 60 on the seams
    (forward), 399 points (backward: fm_flow_lk swaps the frames), 1 point (forward) -- with an odd count the last
    wavefront of the two-points-per-wavefront kernels carries one point."""
    scale, win, max_level, criteria, (max_count, eps), levels = LK_CASES[case]
    size = (640, 360)
    f0, f1, small0, small1 = frame_pair(size, scale, 1, (4, 2))
    h, w = small0.shape
    flow = make_flow(size, scale=scale, win=win, max_level=max_level, criteria=criteria)
    start_pair(ctx, flow, f0, f1)
    assert check_levels(ctx, small0, win, max_level) == levels
    pts = random_points(w, h, 400)
    # the oracle alone (100 points, scale 0.5): 0.77 of the points tracked with win 3, 0.92 - 0.94 otherwise
    check_lk(ctx, small0, small1, np.concatenate([pts, seam_points(w, h, levels)]), win, max_level, max_count, eps)
    check_lk(ctx, small1, small0, pts[:399], win, max_level, max_count, eps)
    check_lk(ctx, small0, small1, np.float32([[w * 0.4, h * 0.55]]), win, max_level, max_count, eps, floor=None)


LK_KERNEL_CASES = {
    # the four production instantiations: lk_pair_pre_kernel<5> / <3> (at most LK_PRE = 6 levels: the default configuration
    # and 'win3'), lk_pair_kernel<5> / <3> (7 levels)
    'win5': ((0.5, 0.5), 5, 5, (3, 10, 0.03), (10, 0.03), 6),
    **{name: LK_CASES[name] for name in ('win3', 'win5_7levels', 'win3_7levels')},
}


@pytest.mark.parametrize('case', list(LK_KERNEL_CASES))
def test_lk_point_counts(ctx, case):
    """Every production LK kernel with 1, 2, 3 and 65 points: two points share a wavefront, so an odd count leaves the
    second half of the last wavefront without a point (n = 1: of the first), and 65 points are 33 wavefronts, 8 per
    256-thread workgroup -- a ninth workgroup with one half-filled wavefront.

    The first points are chosen so that the small counts meet the branches a point can take: [0] an ordinary point,
    [1] one that lies inside the TOP level only (x = w + 3 half 2^(levels - 3): its window starts right of every finer
    level, `posok` false there, status 0 -- beside a point that iterates in the other half of the wavefront), [2] the
    corner pixel (0, 0), whose window starts outside level 0 at (-half, -half) (reflected samples, zero derivatives),
    [3], [4] points just right of / above the image that miss level 0 alone; then seam_points and random ones."""
    scale, win, max_level, criteria, (max_count, eps), levels = LK_KERNEL_CASES[case]
    size = (640, 360)
    f0, f1, small0, small1 = frame_pair(size, scale, 1, (4, 2))
    h, w = small0.shape
    flow = make_flow(size, scale=scale, win=win, max_level=max_level, criteria=criteria)
    start_pair(ctx, flow, f0, f1)
    assert check_levels(ctx, small0, win, max_level) == levels
    seams = seam_points(w, h, levels)
    assert tuple(seams[51]) == (0, 0)
    half = (win - 1) * 0.5
    top_only = w + half * 3 * (1 << (levels - 3))       # between where the two coarsest levels' windows may start
    special = np.float32([[w * 0.4, h * 0.55], [top_only, h * 0.5], seams[51], [w + half + 0.5, h * 0.3],
                          [w * 0.6, -3.5]])
    shapes = [img.shape for img in cv.build_pyramid(small0, win, max_level)]
    start_ok = [[-win <= np.floor(x / (1 << l) - half) < lw and -win <= np.floor(y / (1 << l) - half) < lh
                 for l, (lh, lw) in enumerate(shapes)] for x, y in special]
    assert all(start_ok[0]) and all(start_ok[2])
    assert start_ok[1] == [False] * (levels - 1) + [True]
    assert start_ok[3] == [False] + [True] * (levels - 1) and start_ok[4] == start_ok[3]
    pts = np.concatenate([special, seams[:51], seams[52:], random_points(w, h, 1, seed=5)])
    assert len(pts) == 65
    prev, nxt = small0, small1
    for n in (1, 2, 3, 65):
        en, es = check_lk(ctx, prev, nxt, pts[:n], win, max_level, max_count, eps, floor=None)
        prev, nxt = nxt, prev                          # (fm_flow_lk swaps the two frames)
        # (the oracle's own: the ordinary point is tracked, the ones that start outside level 0 are lost)
        assert es[0] == 1 and not es[[i for i in (1, 3, 4) if i < n]].any()
    # (60 of the 65 lie on borders and seams: the oracle tracks 0.78 / 0.68 of them with winSize 5, 0.58 / 0.48 with 3; the
    # floor only has to show that a good part of the points iterates to the end, as in test_pyramid_paths)
    assert es.mean() > 0.3, es.mean()


def test_lk_window_leaves_the_patch(ctx):
    """`LKPatch::sample`'s fallback to global loads (lk_core.h, both LK kernels): the kernel stages a patch of the next
    image around the start position and leaves it when the window travels more than LK_PR = 5 px inside one level.  With ONE
    level a point's displacement is its travel inside that level: the frames are (16, 8) apart, (8, 4) in the
    optical-flow image, and 30 iterations with epsilon 0.01 let the points get there."""
    size, scale = (640, 360), (0.5, 0.5)
    f0, f1, small0, small1 = frame_pair(size, scale, 1, (16, 8))
    h, w = small0.shape
    flow = make_flow(size, max_level=0, criteria=(3, 30, 0.01))
    start_pair(ctx, flow, f0, f1)
    assert check_levels(ctx, small0, 5, 0) == 1
    pts = random_points(w, h, 400)
    en, es = check_lk(ctx, small0, small1, pts, 5, 0, 30, 0.01, floor=None)
    far = (es > 0) & (np.hypot(*(en - pts).T) > 6.5)
    assert far.sum() >= 50, far.sum()                  # (the oracle alone: 110 of 300 tracked points)
    flow = make_flow(size, win=3, max_level=0, criteria=(3, 30, 0.01))      # ... and the 3 x 3 instance of the same code
    start_pair(ctx, flow, f0, f1)
    check_lk(ctx, small0, small1, pts, 3, 0, 30, 0.01, floor=None)


# ------------------------------------------------------------------------------------------------------------------
# 2. Pyramid construction off the default path
# ------------------------------------------------------------------------------------------------------------------
PYR_CASES = {
    # name: (size, scale, win, maxLevel)
    'plain_0.4':         ((600, 338), (0.4, 0.4), 5, 5),     # gray_kernel, resize_linear_kernel; one pyr_level_kernel launch + tail
    'plain_0.6':         ((802, 452), (0.6, 0.6), 5, 5),     # ... 481 x 271, 241 x 136 above 10 000 px (two launches), then the tail
    'plain_0.6_2levels': ((802, 452), (0.6, 0.6), 5, 1),     # ... pyr_level_kernel with and without a next level, no tail launch
    'tail_only_win5':    ((96, 56), (0.5, 0.5), 5, 5),       # every level <= 10 000 px: pyr_tail_kernel alone (tail == 0)
    'tail_only_win3':    ((96, 56), (0.5, 0.5), 3, 5),       # ... one level more: the depth depends on the window
    'single_level':      ((640, 360), (0.5, 0.5), 5, 0),     # pyr_level_kernel, has_next == false, no tail launch
    'odd_level_widths':  ((642, 360), (0.5, 0.5), 5, 5),     # fused path, 321 -> 161 -> 81 -> 41 -> 21 -> 11
    'odd_small_image':   ((638, 362), (0.5, 0.5), 5, 5),     # 319 x 181: still W == 2 * lw, the fused path
}


@pytest.mark.parametrize('case', list(PYR_CASES))
def test_pyramid_paths(ctx, case):
    """Gray image, every pyramid level and -- through one LK call, which reads the Scharr derivatives of every level --
    the derivative images, where build_pyramid (flow.hip) takes another way than for 1080p at scale 0.5: the plain path
    (`gray_kernel` + `resize_linear_kernel` make gray and level 0, then the level loop every path shares) at a scale
    other than 0.5 -- with one and with two levels above 10 000 px in front of the tail, and with two levels and no tail --,
    all levels inside `pyr_tail_kernel` (no level above 10 000 px), a single level (`pyr_level_kernel` without a next level and
    no tail), odd level widths early in the fused path, and the window-dependent depth (96 x 56: winSize 5 gives three
    levels, winSize 3 four)."""
    size, scale, win, max_level = PYR_CASES[case]
    f0, f1, small0, small1 = frame_pair(size, scale, 5, (2, 2))
    h, w = small0.shape
    flow = make_flow(size, scale=scale, win=win, max_level=max_level)
    start_pair(ctx, flow, f0, f1)
    np.testing.assert_array_equal(ctx.flow_read_image(0), cv.bgr2gray(f0))
    levels = check_levels(ctx, small0, win, max_level)
    if size == (96, 56):
        n5, n3 = len(cv.build_pyramid(small0, 5, 5)), len(cv.build_pyramid(small0, 3, 5))
        assert n5 != n3 and levels == (n5 if win == 5 else n3)
    if case == 'single_level':
        assert levels == 1
    for l, img in enumerate(cv.build_pyramid(small1, win, max_level)):          # the new frame's pyramid
        np.testing.assert_array_equal(ctx.flow_read_image(10 + l), img, err_msg=f'new frame, level {l}')
    pts = np.concatenate([random_points(w, h, 200, seed=8), seam_points(w, h, levels)])
    # (48 x 28: a fifth of the points start outside the image and winSize 3 loses more of the rest; the floor only has to
    # show that a good part of the ~260 points is tracked at all)
    floor = 0.3 if size == (96, 56) else 0.5
    check_lk(ctx, small0, small1, pts, win, max_level, 10, 0.03, floor=floor)
    check_lk(ctx, small1, small0, pts[:131], win, max_level, 10, 0.03, floor=floor)   # (derivatives of the other set)


# ------------------------------------------------------------------------------------------------------------------
# 3. Corner detection: block size 5, selection paths, limits
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gftt_frame():
    f0 = textured_frame(640, 360, 11)
    g0 = cv.bgr2gray(f0)
    f0.setflags(write=False)
    g0.setflags(write=False)
    return f0, g0


@functools.lru_cache(maxsize=None)
def sorted_candidates(rect, quality, block):
    """The candidates of goodFeaturesToTrack on the crop `rect` of gftt_frame() without a mask, strongest first (value
    descending, raster index descending: featureselect.cpp's greaterThanPtr): -> (values f32[n], raster indices)."""
    g0 = gftt_frame()[1]
    eig = cv.corner_min_eigen_val(g0[rect[1]:rect[3] + 1, rect[0]:rect[2] + 1], block)
    h, w = eig.shape
    thr = np.float32(eig.max() * np.float32(quality))
    inner = eig[1:-1, 1:-1]
    nb = np.max([eig[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    ys, xs = np.nonzero((inner > thr) & (inner != 0) & (inner >= nb))
    val, idx = inner[ys, xs], (ys + 1) * w + xs + 1
    order = np.lexsort((-idx, -val.astype(np.float64)))
    return val[order], idx[order]


def ellipse(pts, rect):
    rect = np.asarray(rect, float)
    c = (rect[:2] + rect[2:]) / 2
    ax = (rect[2:] - rect[:2] + 1) * 0.5
    return pts[(((pts - c) / ax) ** 2).sum(1) <= 1.] if len(pts) else pts


def expected_corners(g0, rect, mask, max_corners, quality, md, block):
    """goodFeaturesToTrack on the crop + the crop's offset + Flow's ellipse filter -> (list, corners before the filter)"""
    r = np.asarray(rect, int)
    raw = cv.good_features_to_track(g0[r[1]:r[3] + 1, r[0]:r[2] + 1], mask, max_corners, quality, md, block)
    raw = raw.reshape(-1, 2) + np.array(r[:2], np.float32)
    return ellipse(raw, rect), raw


def detect_one(ctx, rect, md, cap=1000):
    """fm_flow_targets + fm_flow_detect for one unmasked crop -> its corner list"""
    rects = np.array([rect], float)
    ctx.flow_targets(rects, np.empty((0, 2), np.float32), np.zeros(2, np.int32))
    pts, cnt = ctx.flow_detect([0], rects, [md], cap=cap)
    return pts[0, :cnt[0]]


def test_gftt_block_size_5_edge_crops(ctx):
    """`eig_cand_kernel<2>` (blockSize 5: a 5 x 5 box over the gradient products, two pixels of halo instead of one) on
    the nine crops of test_gftt_edge_crops, where the tiled kernel has its seams: one pixel wide, 2 x 3, 3 x 3, exactly
    one 32 x 32 tile, 33 x 33, both frame corners, 64 x 8, and a track overlapped by 40 earlier ones.  (cv_oracle is
    defined for all nine: BORDER_REFLECT_101 of a one- or two-pixel axis folds back into it, as cv::borderInterpolate
    does; none is dropped.)"""
    f0, g0 = gftt_frame()
    size = (640, 360)
    flow = make_flow(size, block=5)
    flow.init(f0)
    small = [[300 + 3 * i, 200 + 2 * i, 330 + 3 * i, 240 + 2 * i] for i in range(40)]
    rects = np.array(small + [[280, 180, 460, 330], [10, 10, 10, 40], [20, 10, 21, 12], [40, 10, 42, 12], [60, 20, 91, 51],
                              [100, 20, 132, 52], [0, 0, 70, 9], [560, 300, 639, 359], [200, 20, 263, 27]], float)
    ctx.flow_targets(rects, np.empty((0, 2), np.float32), np.zeros(len(rects) + 1, np.int32))
    mask = np.full((size[1], size[0]), 255, np.uint8)
    masks = []
    for r in rects.astype(int):
        masks.append(mask[r[1]:r[3] + 1, r[0]:r[2] + 1].copy())
        mask[r[1]:r[3] + 1, r[0]:r[2] + 1] = 0
    idx = list(range(40, len(rects)))
    mds = [7, 1, 1, 1, 3, 4, 2, 25, 2]
    pts, cnt = ctx.flow_detect(idx, rects[idx], mds, cap=1000)
    seen, differs_from_block3 = 0, False
    for i, (k, md) in enumerate(zip(idx, mds)):
        exp, _ = expected_corners(g0, rects[k], masks[k], 1000, 0.06, md, 5)
        got = pts[i, :cnt[i]]
        assert len(got) == len(exp), (k, len(got), len(exp))
        np.testing.assert_array_equal(got, exp, err_msg=f'crop {k}')
        seen += len(exp)
        exp3, _ = expected_corners(g0, rects[k], masks[k], 1000, 0.06, md, 3)
        differs_from_block3 |= len(exp3) != len(exp) or bool((exp3 != exp).any())
    assert masks[40].any() and not masks[40].all() and seen > 40 and differs_from_block3


BIG = (100, 80, 399, 279)          # 300 x 200
GFTT_CASES = {
    # name: (rect, minDistance, maxCorners, quality, blockSize)
    'bitonic':         (BIG, 4, 1000, 0.06, 3),
    'list_scan':       ((200, 100, 380, 250), 2, 1000, 0.01, 3),     # 181 x 151, cells of 2 px: 91 x 76 > 1536
    'list_scan_md3':   ((200, 100, 380, 250), 3, 1000, 0.01, 3),     # ... of 3 px: 61 x 51 > 1536
    'list_scan_md7':   ((100, 60, 399, 319), 7, 1000, 0.06, 3),      # 300 x 260, cells of 7 px: 43 x 38 > 1536
    'max_corners_50':  (BIG, 4, 50, 0.06, 3),
    'first_1000':      (BIG, 1, 1000, 0.06, 3),
    'first_1024':      (BIG, 1, 1024, 0.06, 3),
    'quality_0.3':     (BIG, 4, 1000, 0.3, 3),
    'quality_0.001':   (BIG, 4, 1000, 0.001, 3),
    'bitonic_block5':  (BIG, 4, 1000, 0.06, 5),
}


@pytest.mark.parametrize('case', list(GFTT_CASES))
def test_gftt_selection_paths(ctx, case):
    """gftt_select_kernel beyond the rank sort of a small crop.  `bitonic`: more than 1024 candidates above the
    threshold (the oracle counts 1457 on this 300 x 200 crop), so the bitonic network sorts them (n > 1024).
    `list_scan`, `list_scan_md3`, `list_scan_md7`: minDistance 2 / 3 on 181 x 151 gives 91 x 76 / 61 x 51 cells and
    minDistance 7 on 300 x 260 gives 43 x 38, more than GFTT_MAX_CELLS = 1536, so `use_grid == false` and the
    accepted-list scan decides.  (Two local maxima of a 3 x 3 neighbourhood are never closer than 2 px unless they tie,
    so minDistance 2 blocks nothing here; 3 blocks a few candidates, 7 most of them, after a bitonic sort.)  `max_corners_50`, `first_1000`, `first_1024`: the
    `limit = min(max_corners, 1024)` truncation, in the middle of a span, with every candidate accepted until the limit
    (minDistance 1), and at the largest maxCorners fm_flow_configure admits.  `quality_*`: other thresholds (few
    candidates / very many).  `bitonic_block5`: `eig_cand_kernel<2>` on a crop of 10 x 7 tiles."""
    rect, md, max_corners, quality, block = GFTT_CASES[case]
    f0, g0 = gftt_frame()
    w, h = rect[2] - rect[0] + 1, rect[3] - rect[1] + 1
    n_cand = len(sorted_candidates(rect, quality, block)[0])
    exp, raw = expected_corners(g0, rect, np.full((h, w), 255, np.uint8), max_corners, quality, md, block)
    print(f'{case}: {n_cand} candidates, {len(raw)} corners, {len(exp)} inside the ellipse')
    assert n_cand <= GFTT_MAX_CAND and len(exp) > 10
    if case in ('bitonic', 'bitonic_block5', 'max_corners_50', 'first_1000', 'first_1024'):
        assert n_cand > 1024
    if case.startswith('list_scan'):
        assert ((w + md - 1) // md) * ((h + md - 1) // md) > GFTT_MAX_CELLS and n_cand > 512
    if case == 'list_scan_md3':
        assert 64 < len(raw) < n_cand                   # (candidates are blocked: the scan has something to find)
    if case == 'list_scan_md7':
        assert 64 < len(raw) < n_cand // 2 and n_cand > 1024
    if case in ('max_corners_50', 'first_1000', 'first_1024'):
        assert len(raw) == max_corners
    if case == 'quality_0.3':
        assert n_cand < 1024
    flow = make_flow((640, 360), block=block, max_corners=max_corners, quality=quality)
    flow.init(f0)
    got = detect_one(ctx, rect, md, cap=1024)
    assert len(got) == len(exp), (len(got), len(exp))
    np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize('max_corners, rank_limit', [(200, 207), (1000, 1043)])
def test_gftt_candidate_overflow(ctx, max_corners, rank_limit):
    """gftt_select_kernel with `s_n > GFTT_MAX_CAND = 4096`: the whole 640 x 360 frame as one crop has 5412 candidates
    above the threshold.  The kernel keeps the 4096 strongest (it handed out the LDS slots in scheduling order before:
    a different subset from call to call); with minDistance 3 the oracle's selection ends within the 207 (maxCorners
    200) / 1043 (maxCorners 1000) strongest candidates, so the lists must be the oracle's, twice in a row.  (Only one
    pair of the candidates ties in value: the order is well defined.)"""
    rect, md = (0, 0, 639, 359), 3
    f0, g0 = gftt_frame()
    val, idx = sorted_candidates(rect, 0.06, 3)
    assert len(val) > GFTT_MAX_CAND
    exp, raw = expected_corners(g0, rect, np.full((360, 640), 255, np.uint8), max_corners, 0.06, md, 3)
    assert len(raw) == max_corners
    rank = {int(i): r for r, i in enumerate(idx)}
    worst = max(rank[int(p[1]) * 640 + int(p[0])] for p in raw)
    print(f'{len(val)} candidates, {len(raw)} corners, the last one is candidate {worst}; {int((np.diff(val) == 0).sum())} ties')
    assert worst < rank_limit < GFTT_MAX_CAND
    flow = make_flow((640, 360), max_corners=max_corners)
    flow.init(f0)
    for _ in range(2):
        got = detect_one(ctx, rect, md)
        assert len(got) == len(exp), (len(got), len(exp))
        np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize('max_corners', [0, -1, 1025, 5000])
def test_max_corners_outside_the_range_is_refused(ctx, max_corners):
    """`limit = min(max_corners, 1024)` (gftt_select_kernel): a maxCorners above 1024 used to be capped silently and
    `<= 0` -- OpenCV: no limit -- returned no corner.  fm_flow_configure refuses both and names the limit."""
    flow = make_flow((640, 360), max_corners=max_corners)
    with pytest.raises(FastMOTHipError, match=f'error {FM_ERR_ARG}: maxCorners {max_corners}: .*1 .. {GFTT_MAX_CORNERS}'):
        flow.init(gftt_frame()[0])


# ------------------------------------------------------------------------------------------------------------------
# 4. Flow.predict end to end at a non-default configuration
# ------------------------------------------------------------------------------------------------------------------
PREDICT_KW = dict(opt_flow_scale_factor=(0.6, 0.6), bg_feat_scale_factor=(0.2, 0.2), feat_density=0.01,
                  feat_dist_factor=0.03, max_error=60, inlier_thresh=3, ransac_max_iter=200, bg_feat_thresh=20)
PREDICT_SEED = 100


def predict_pair(size, **over):
    kw = dict(PREDICT_KW)
    kw.update(over)
    flow = make_flow(size, scale=kw.pop('opt_flow_scale_factor'), win=3, max_level=3, criteria=(3, 20, 0.02), block=5,
                     max_corners=300, quality=0.03, **kw)
    ora = cpu_tracker.OracleFlow(size, bg_scale=kw['bg_feat_scale_factor'], opt_scale=(0.6, 0.6),
                                 feat_density=kw['feat_density'], feat_dist_factor=kw['feat_dist_factor'],
                                 ransac_max_iter=kw['ransac_max_iter'], max_error=kw['max_error'],
                                 inlier_thresh=kw['inlier_thresh'], bg_feat_thresh=kw['bg_feat_thresh'],
                                 max_corners=300, quality_level=0.03, block_size=5, win=3, max_level=3, max_count=20,
                                 epsilon=0.02)
    return flow, ora


def test_flow_predict_non_default_configuration(ctx):
    """Flow.predict in one call per frame, as test_flow_predict_1080p_50_tracks, with every parameter off its default:
    optical-flow scale 0.6 (the plain pyramid path inside fm_flow_predict), background scale 0.2, feat_density 0.01,
    feat_dist_factor 0.03, winSize 3 / maxLevel 3 / criteria (3, 20, 0.02) (`lk_pair_pre_kernel<3>`), blockSize 5
    (`eig_cand_kernel<2>`), qualityLevel 0.03, maxCorners 300, max_error 60, inlier_thresh 3, 200 RANSAC iterations,
    FAST threshold 20.  Three consecutive frames of a 640 x 360 clip with 8 objects."""
    from synthetic import SyntheticVideo
    size = (640, 360)
    video = SyntheticVideo(size, n_ids=8, n_frames=4, seed=PREDICT_SEED)
    flow, ora = predict_pair(size)
    flow.init(video.frames[0])
    ora.init(video.frames[0])
    boxes0 = video.detections(0).tlbr
    a = [FakeTrack(i + 1, boxes0[i]) for i in range(8)]
    b = [FakeTrack(i + 1, boxes0[i]) for i in range(8)]
    for f in (1, 2, 3):
        gb, Hb = ora.predict(video.frames[f], b)
        assert Hb is not None and len(gb) >= 6                                # (the oracle's own result)
        ga, Ha = flow.predict(video.frames[f], a)
        assert Ha is not None
        assert [t.trk_id for t in a] == [t.trk_id for t in b]                 # same closest-first order
        assert list(ga.keys()) == list(gb.keys())
        for ta, tb in zip(a, b):
            assert len(ta.keypoints) == len(tb.keypoints), (f, ta.trk_id)
            np.testing.assert_array_equal(ta.prev_keypoints, tb.prev_keypoints)   # GFTT / propagated points
            np.testing.assert_array_equal(ta.keypoints, tb.keypoints)             # LK: bit-identical
            assert ta.inlier_ratio == tb.inlier_ratio
        np.testing.assert_array_equal(flow.prev_bg_keypoints, ora.prev_bg_keypoints)
        np.testing.assert_array_equal(flow.bg_keypoints, ora.bg_keypoints)
        assert sum(len(t.keypoints) for t in b) > 100 and len(ora.bg_keypoints) > 20
        for k in ga:
            np.testing.assert_array_equal(ga[k], gb[k])                           # rounded boxes
        np.testing.assert_allclose(Ha, Hb, rtol=1e-6, atol=1e-8)                  # host double arithmetic (Jacobi / LM)
        for ta, tb in zip(a, b):                                              # both sides continue from the same boxes
            if ta.trk_id in gb:
                ta._tlbr = tb._tlbr = np.rint(gb[ta.trk_id])


def test_flow_predict_without_background_keypoints(ctx):
    """The failure branch of the same configuration: a FAST threshold of 255 leaves no background keypoint, and both
    sides return ({}, None)."""
    from synthetic import SyntheticVideo
    size = (640, 360)
    video = SyntheticVideo(size, n_ids=8, n_frames=4, seed=PREDICT_SEED)
    flow, ora = predict_pair(size, bg_feat_thresh=255)
    flow.init(video.frames[0])
    ora.init(video.frames[0])
    boxes0 = video.detections(0).tlbr
    a = [FakeTrack(i + 1, boxes0[i]) for i in range(8)]
    b = [FakeTrack(i + 1, boxes0[i]) for i in range(8)]
    assert ora.predict(video.frames[1], b) == ({}, None)
    assert flow.predict(video.frames[1], a) == ({}, None)
    assert len(flow.bg_keypoints) == 0 and len(ora.bg_keypoints) == 0


# ------------------------------------------------------------------------------------------------------------------
# 5. fm_flow_configure's argument checks
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [dict(win=7), dict(block=7), dict(max_level=8)], ids=lambda kw: '_'.join(map(str, *kw.items())))
def test_configure_refuses_what_has_no_kernel(ctx, kw):
    """winSize 7, blockSize 7 and maxLevel 8 have no kernel instance / no room in the level tables: fm_flow_configure
    answers FM_ERR_ARG before it launches or allocates anything."""
    flow = make_flow((640, 360), **kw)
    with pytest.raises(FastMOTHipError, match=f'error {FM_ERR_ARG}: .*bad argument'):
        flow._configure()
    make_flow((640, 360)).init(gftt_frame()[0])        # (the context is usable afterwards)
