"""GPU parity: batched Kalman kernels (kalman.hip) through the C ABI
  * oracle=reference: golden vectors generated from /root/reference (tests/golden/kalman_kat.npz)
  * oracle=restated : oracle/np_oracle.py on seeded random inputs (sizes 1..300 tracks)
Tolerance: fp64 round-off (rtol 1e-9 on covariances, 1e-11 on means) -- the reference multiplies
8x8 matrices through BLAS with an unspecified summation order; rounded boxes must be identical.
Off the defaults: tests/golden/kalman_kat_offdefault.npz (oracle/make_golden.py golden_kalman_offdefault) and the
KF_OFFDEFAULT cases below -- width and height factors that differ, F_pos_self / F_pos_other away from 0.6 / 0.4, a
homography with a perspective row, fast tracks, partly filled last blocks and the blit I/O path (zero_copy_tracks=0)."""
import numpy as np
import pytest

import np_oracle as o

pytestmark = pytest.mark.gpu

KF_DEFAULT = dict(std_factor_acc=2.25, std_offset_acc=78.5, std_factor_det=(0.08, 0.08),
                  std_factor_klt=(0.14, 0.14), min_std_det=(4.0, 4.0), min_std_klt=(5.0, 5.0),
                  init_pos_weight=5, init_vel_weight=12, vel_coupling=0.6, vel_half_life=2)
KF_OFFDEFAULT = dict(std_factor_acc=1.7, std_offset_acc=40.0, std_factor_det=(0.05, 0.11),
                     std_factor_klt=(0.2, 0.09), min_std_det=(3.0, 6.5), min_std_klt=(7.0, 4.0),
                     init_pos_weight=3, init_vel_weight=9, vel_coupling=0.35, vel_half_life=0.7)
KF_SETS = {'default': KF_DEFAULT, 'offdefault': KF_OFFDEFAULT}
FRAME = np.array([0., 0., 1919., 1079.])


def configure(ctx, dt, kf=KF_DEFAULT):
    ctx.kf_configure(dt, **kf)
    ctx.set_frame_rect(FRAME)


class io_path:
    """zero_copy_tracks for the body: 2048 (the default: kernels read and write page-locked host memory) or 0 (inputs and
    results go through blit copies)."""

    def __init__(self, ctx, zero_copy_tracks):
        self.ctx, self.value = ctx, zero_copy_tracks

    def __enter__(self):
        self.ctx.set_option('zero_copy_tracks', self.value)

    def __exit__(self, *exc):
        self.ctx.set_option('zero_copy_tracks', 2048)


def perspective_H(rng):
    """A homography whose third row matters: h31, h32 ~ 1e-4 move the divisor by up to ~0.2 across a 1920 px frame."""
    H = np.eye(3) + rng.normal(0, 1e-2, (3, 3))
    H[:2, 2] = rng.normal(0, 8, 2)
    H[2, :2] = rng.normal(0, 1e-4, 2)
    H[2, 2] = 1.
    return H


@pytest.mark.parametrize('tag', ['dt30', 'dt12'])
def test_golden_chain(ctx, golden_dir, tag):
    _golden_chain(ctx, np.load(golden_dir / 'kalman_kat.npz'), tag, KF_DEFAULT)


@pytest.mark.parametrize('tag', ['od30', 'od7'])
def test_golden_chain_offdefault(ctx, golden_dir, tag):
    """n = 23: the last block of kf_step_kernel and kf_update_det_kernel has a dead wave."""
    _golden_chain(ctx, np.load(golden_dir / 'kalman_kat_offdefault.npz'), tag, KF_OFFDEFAULT)


def _golden_chain(ctx, g, tag, kf):
    configure(ctx, float(g[f'{tag}_dt']), kf)
    boxes, H = g[f'{tag}_boxes'], g[f'{tag}_H']
    n = len(boxes)
    slots = np.arange(10, 10 + n)
    ctx.trk_create(slots, boxes)
    m, c = ctx.trk_get_state(slots)
    np.testing.assert_array_equal(m, g[f'{tag}_create_m'])
    np.testing.assert_allclose(c, g[f'{tag}_create_c'], rtol=1e-15)
    # warp only
    ctx.trk_set_state(slots, g[f'{tag}_start_m'], g[f'{tag}_start_c'])
    zeros, ones = np.zeros((n, 4)), np.ones(n)
    ctx.trk_step_ops(1, slots, H, zeros, np.zeros(n, np.uint8), ones)
    m, c = ctx.trk_get_state(slots)
    np.testing.assert_allclose(m, g[f'{tag}_warp_m'], rtol=1e-12, atol=1e-10)
    np.testing.assert_allclose(c, g[f'{tag}_warp_c'], rtol=1e-9, atol=1e-9)
    # predict only
    ctx.trk_set_state(slots, g[f'{tag}_warp_m'], g[f'{tag}_warp_c'])
    ctx.trk_step_ops(2, slots, np.eye(3), zeros, np.zeros(n, np.uint8), ones)
    m, c = ctx.trk_get_state(slots)
    np.testing.assert_allclose(m, g[f'{tag}_pred_m'], rtol=1e-12, atol=1e-10)
    np.testing.assert_allclose(c, g[f'{tag}_pred_c'], rtol=1e-10, atol=1e-9)
    # KLT update only
    ctx.trk_set_state(slots, g[f'{tag}_pred_m'], g[f'{tag}_pred_c'])
    ctx.trk_step_ops(4, slots, np.eye(3), g[f'{tag}_klt'], np.ones(n, np.uint8), g[f'{tag}_mult'])
    m, c = ctx.trk_get_state(slots)
    np.testing.assert_allclose(m, g[f'{tag}_klt_m'], rtol=1e-11, atol=1e-9)
    np.testing.assert_allclose(c, g[f'{tag}_klt_c'], rtol=1e-9, atol=1e-8)
    # detector update
    ctx.trk_set_state(slots, g[f'{tag}_klt_m'], g[f'{tag}_klt_c'])
    tlbr, lost = ctx.trk_update_det(slots, g[f'{tag}_det'])
    m, c = ctx.trk_get_state(slots)
    np.testing.assert_allclose(m, g[f'{tag}_det_m'], rtol=1e-11, atol=1e-9)
    np.testing.assert_allclose(c, g[f'{tag}_det_c'], rtol=1e-9, atol=1e-8)
    np.testing.assert_array_equal(tlbr, np.rint(g[f'{tag}_det_m'][:, :4]))
    np.testing.assert_array_equal(lost, o.ios(np.rint(g[f'{tag}_det_m'][:, :4]), FRAME) < 0.5)


@pytest.mark.parametrize('n', [1, 3, 4, 5, 50, 300])
def test_fused_step_vs_oracle(ctx, n):
    def nearly_affine_H(rng):
        H = np.eye(3) + rng.normal(0, 1e-3, (3, 3)); H[:2, 2] += rng.normal(0, 3, 2)
        H[2, :2] = rng.normal(0, 1e-6, 2); H[2, 2] = 1.
        return H
    _fused_steps(ctx, np.random.default_rng(100 + n), n, KF_DEFAULT, nearly_affine_H, vel_std=0.)


@pytest.mark.parametrize('zero_copy_tracks', [2048, 0])
@pytest.mark.parametrize('kf', ['default', 'offdefault'])
def test_fused_step_perspective_fast_tracks(ctx, kf, zero_copy_tracks):
    """The fused step where the near-affine, slow default cases do not reach: h31, h32 ~ 1e-4 and velocities of ~120 px/s
    give the second-order term of the warp's Jacobian and its -(Hv h3^T + b H1)/a^2 block entries of the size of the
    others; both parameter sets; inputs and results through page-locked memory (2048) and through blit copies (0)."""
    with io_path(ctx, zero_copy_tracks):
        for n in (1, 5, 50):
            _fused_steps(ctx, np.random.default_rng(7000 + n), n, KF_SETS[kf], perspective_H, vel_std=120.)


def _fused_steps(ctx, rng, n, kf, make_H, vel_std):
    dt = 1 / 30.
    configure(ctx, dt, kf)
    p = o.KFParams(dt, **kf)
    tl = np.stack([rng.uniform(-50, 1800, n), rng.uniform(-50, 1000, n)], 1)
    boxes = np.rint(np.concatenate([tl, tl + rng.uniform(20, 300, (n, 2))], 1))
    slots = rng.permutation(np.arange(1, 2 * n + 1))[:n]
    ctx.trk_create(slots, boxes)
    m, c = o.kf_create(p, boxes)
    gm, gc = ctx.trk_get_state(slots)
    np.testing.assert_array_equal(gm, m)
    np.testing.assert_allclose(gc, c, rtol=1e-15)
    H = make_H(rng)
    if vel_std:
        m[:, 4:] = rng.normal(0, vel_std, (n, 4))
        ctx.trk_set_state(slots, m, c)
    for it in range(4):
        has = rng.random(n) < 0.7
        klt = np.rint(m[:, :4] + rng.normal(0, 3, (n, 4)))
        mult = rng.uniform(1, 6, n)
        tlbr, lost = ctx.trk_step(slots, H, klt, has, mult)
        m, c = o.kf_warp(m, c, H)
        m, c = o.kf_predict(p, m, c)
        mu, cu = o.kf_update(p, m, c, klt, 'flow', mult)
        m = np.where(has[:, None], mu, m)
        c = np.where(has[:, None, None], cu, c)
        gm, gc = ctx.trk_get_state(slots)
        np.testing.assert_allclose(gm, m, rtol=1e-11, atol=1e-9)
        np.testing.assert_allclose(gc, c, rtol=1e-9, atol=1e-8)
        np.testing.assert_array_equal(tlbr, np.rint(m[:, :4]))
        exp_lost = o.ios(np.rint(m[:, :4]), FRAME) < 0.5
        np.testing.assert_array_equal(lost, exp_lost)
        # continue from the device state so that round-off does not accumulate in the comparison
        m, c = gm, gc


@pytest.mark.parametrize('n,zero_copy_tracks', [(1, 2048), (2, 2048), (3, 2048), (5, 2048), (6, 2048), (7, 2048),
                                                (7, 0), (50, 2048)])
@pytest.mark.parametrize('kf', ['default', 'offdefault'])
def test_update_det_vs_oracle(ctx, kf, n, zero_copy_tracks):
    """kf_update_det_kernel on states two device steps old, at batch sizes that leave 3, 2, 1 and no waves of the last
    block dead.  A dead wave runs the update on slot 0 for the barriers' sake and must not write: slot 0 holds a state
    of its own here and is compared afterwards.  Every third track sits mostly outside the frame (lost)."""
    rng = np.random.default_rng(300 + n)
    dt = 1 / 30.
    configure(ctx, dt, KF_SETS[kf])
    p = o.KFParams(dt, **KF_SETS[kf])
    tl = np.stack([rng.uniform(100, 1600, n), rng.uniform(100, 800, n)], 1)
    boxes = np.rint(np.concatenate([tl, tl + rng.uniform(20, 250, (n, 2))], 1))
    out = np.arange(n) % 3 == 0
    boxes[out, 0::2] -= np.rint(boxes[out, 0] + 0.8 * (boxes[out, 2] - boxes[out, 0]))[:, None]   # 20% of the width inside
    slots = rng.permutation(np.arange(1, 2 * n + 1))[:n]
    with io_path(ctx, zero_copy_tracks):
        ctx.trk_create(np.append(slots, 0), np.vstack([boxes, [[300., 200., 380., 420.]]]))
        H = perspective_H(rng)
        for it in range(2):
            m, _ = ctx.trk_get_state(slots)
            ctx.trk_step(slots, H, np.rint(m[:, :4] + rng.normal(0, 3, (n, 4))), rng.random(n) < 0.7, rng.uniform(1, 6, n))
        ctx.trk_step([0], H, [[302., 203., 381., 424.]], [1], [2.])
        m, c = ctx.trk_get_state(slots)
        m0, c0 = ctx.trk_get_state([0])
        assert np.abs(c[:, 0, 2]).min() > 0 and np.abs(c[:, 1, 5]).min() > 0       # evolved: not diagonal
        det = np.rint(m[:, :4] + rng.normal(0, 6, (n, 4)))
        tlbr, lost = ctx.trk_update_det(slots, det)
        gm, gc = ctx.trk_get_state(slots)
        s0 = ctx.trk_get_state([0])
    em, ec = o.kf_update(p, m, c, det, 'detector')
    np.testing.assert_allclose(gm, em, rtol=1e-11, atol=1e-9)
    np.testing.assert_allclose(gc, ec, rtol=1e-9, atol=1e-8)
    np.testing.assert_array_equal(tlbr, np.rint(em[:, :4]))
    exp_lost = o.ios(np.rint(em[:, :4]), FRAME) < 0.5
    if n >= 5:
        assert exp_lost.any() and not exp_lost.all()
    np.testing.assert_array_equal(lost, exp_lost)
    np.testing.assert_array_equal(s0[0], m0)
    np.testing.assert_array_equal(s0[1], c0)


@pytest.mark.parametrize('zero_copy_tracks', [2048, 0])
def test_write_box_rounding_and_lost_flag(ctx, zero_copy_tracks):
    """trk_step_ops with no operation bit: the kernel only rounds the mean's box (half to even, like the reference's
    as_tlbr) and flags it lost when less than half of it lies inside the frame; the state comes back as it went in."""
    configure(ctx, 1 / 30.)
    rng = np.random.default_rng(5)
    box = np.array([[10.5, 11.5, 110.5, 211.5],        # halves go to the even neighbour ...
                    [-0.5, 2.5, 99.5, 101.5],          # ... -0.5 -> -0
                    [-50., 100., 49., 199.],           # exactly half inside: ios == 0.5 is not < 0.5
                    [-51., 100., 48., 199.],           # 49 of 100 columns inside
                    [2000., 100., 2100., 200.],        # entirely outside
                    [-99., 100., 0., 199.],            # one pixel column inside
                    [-50.5, 99.5, 49.5, 199.5]])       # rounds to [-50, 100, 50, 200]: 51 of 101 columns inside
    exp = np.array([[10., 12., 110., 212.], [-0., 2., 100., 102.], [-50., 100., 49., 199.], [-51., 100., 48., 199.],
                    [2000., 100., 2100., 200.], [-99., 100., 0., 199.], [-50., 100., 50., 200.]])
    exp_lost = np.array([False, False, False, True, True, True, False])
    np.testing.assert_array_equal(exp, np.rint(box))
    np.testing.assert_array_equal(exp_lost, o.ios(exp, FRAME) < 0.5)
    assert o.ios(exp, FRAME)[2] == 0.5
    n = len(box)
    mean = np.concatenate([box, rng.normal(0, 50, (n, 4))], 1)
    a = rng.normal(0, 10, (n, 8, 8))
    cov = a @ a.transpose(0, 2, 1)
    slots = np.array([4, 9, 2, 7, 11, 3, 6])
    with io_path(ctx, zero_copy_tracks):
        ctx.trk_set_state(slots, mean, cov)
        tlbr, lost = ctx.trk_step_ops(0, slots, np.eye(3), np.zeros((n, 4)), np.zeros(n, np.uint8), np.ones(n))
        gm, gc = ctx.trk_get_state(slots)
    np.testing.assert_array_equal(tlbr, exp)
    assert np.signbit(tlbr[1, 0]) and not np.signbit(tlbr[1, 1])
    np.testing.assert_array_equal(lost, exp_lost)
    np.testing.assert_array_equal(gm, mean)
    np.testing.assert_array_equal(gc, cov)


def test_copy_state(ctx):
    rng = np.random.default_rng(6)
    mean = rng.normal(0, 300, (3, 8))
    cov = rng.normal(0, 100, (3, 8, 8))
    src, dst, other = 12, 5, 13
    ctx.trk_set_state([src, dst, other], mean, cov)
    ctx.trk_copy_state(dst, src)
    gm, gc = ctx.trk_get_state([src, dst, other])
    np.testing.assert_array_equal(gm, mean[[0, 0, 2]])
    np.testing.assert_array_equal(gc, cov[[0, 0, 2]])


def test_empty_batch(ctx):
    configure(ctx, 1 / 30.)
    tlbr, lost = ctx.trk_step([], np.eye(3), np.zeros((0, 4)), [], [])
    assert tlbr.shape == (0, 4) and lost.shape == (0,)
    ctx.trk_create([], np.zeros((0, 4)))
