"""CPU: oracle restatement vs the reference's own functions, on seeded inputs.  What the reference computes on these
inputs is stored in tests/golden/oracle_vs_reference.npz (oracle/make_golden_refcheck.py runs the reference modules
under oracle/ref_shim.py, and its decode kernels through oracle/yolo_layer_ref.py, on the inputs built here)."""
import numpy as np
import pytest

import np_oracle as o

YOLO_CASES = [(80, False), (2, False), (1, False), (80, True), (3, True)]
YOLO_ANCHORS = [12, 16, 19, 36, 40, 28]
YOLO_SHAPES = (((19, 19), (608, 608)), ((20, 36), (1152, 640)), ((1, 1), (32, 32)))


@pytest.fixture(scope='module')
def ref(golden_dir):
    return np.load(golden_dir / 'oracle_vs_reference.npz')


def kalman_inputs():
    rng = np.random.default_rng(3)
    n = 24
    tl = rng.uniform(0, 1000, (n, 2))
    boxes = np.rint(np.concatenate([tl, tl + rng.uniform(20, 300, (n, 2))], 1))
    H = np.eye(3) + rng.normal(0, 1e-3, (3, 3)); H[2, 2] = 1; H[2, :2] *= 1e-3
    p = o.KFParams(1 / 25.)
    m, c = o.kf_create(p, boxes)
    m[:, 4:] = rng.normal(0, 20, (n, 4))
    return boxes, H, m, c


def lap_problems():
    rng = np.random.default_rng(5)
    for _ in range(30):
        nr, nc = rng.integers(1, 12, 2)
        cost = np.round(rng.uniform(0, 1, (nr, nc)), 1)    # many ties
        cost[rng.random((nr, nc)) < 0.3] = 1e5
        yield cost


def feature_inputs():
    rng = np.random.default_rng(9)
    for k in range(1, 6):
        v = rng.normal(0, 1, 512).astype(np.float32)
        v /= np.linalg.norm(v)
        yield v


def yolo_heads(num_classes, new_coords):
    rng = np.random.default_rng(num_classes + 7 * new_coords)
    for (H, W), in_wh in YOLO_SHAPES:
        head = (rng.uniform(0, 1, ((5 + num_classes) * 3, H, W)) if new_coords
                else rng.normal(0, 2.5, ((5 + num_classes) * 3, H, W))).astype(np.float32)
        if num_classes > 1:
            head[5 + 1, 0, 0] = head[5, 0, 0]          # a tie between two class logits: the first one wins
        yield head, in_wh


def test_kalman_random(ref):
    """kf.warp -> predict -> update(FLOW) of the reference's KalmanFilter, track by track."""
    boxes, H, m, c = kalman_inputs()
    p = o.KFParams(1 / 25.)
    m2, c2 = o.kf_warp(m, c, H)
    m2, c2 = o.kf_predict(p, m2, c2)
    m2, c2 = o.kf_update(p, m2, c2, boxes + 2, 'flow', 3.0)
    for i in range(len(boxes)):
        np.testing.assert_allclose(m2[i], ref['kalman_mean'][i], rtol=1e-11, atol=1e-9)
        np.testing.assert_allclose(c2[i], ref['kalman_cov'][i], rtol=1e-9, atol=1e-8)


def test_greedy_and_lap_random(ref):
    """matching.linear_assignment and matching.greedy_match of the reference, row ids offset by 10."""
    def pairs(key):
        return [(int(a), int(b)) for a, b in ref[key].reshape(-1, 2)]

    def ids(key):
        return [int(x) for x in ref[key]]
    for t, cost in enumerate(lap_problems()):
        r, c = o.lsa(cost)
        m2, ur2, uc2 = o.assignment_matches(cost, r, c)
        assert [(10 + a, b) for a, b in m2] == pairs(f'lap{t}_m')
        assert [10 + a for a in ur2] == ids(f'lap{t}_ur') and uc2 == ids(f'lap{t}_uc')
        m2, ur2, uc2 = o.greedy_match(cost, 0.5)
        assert [(10 + a, b) for a, b in m2] == pairs(f'greedy{t}_m')
        assert [10 + a for a in ur2] == ids(f'greedy{t}_ur') and uc2 == ids(f'greedy{t}_uc')


def test_average_feature(ref):
    """track.AverageFeature of the reference after each of five updates."""
    s = a = None
    for k, v in enumerate(feature_inputs(), 1):
        if s is None:
            s, a = v.copy(), v.copy()
        else:
            s, a = o.average_feature(s, v, k)
        np.testing.assert_allclose(a, ref['average_feature'][k - 1], rtol=2e-6, atol=1e-7)


@pytest.mark.parametrize('num_classes,new_coords', YOLO_CASES)
def test_yolo_decode_against_the_reference_kernels(ref, num_classes, new_coords):
    """np_oracle.yolo_decode against the reference's own CalDetection / CalDetection_NewCoords (plugins/yolo_layer.cu:
    127-230), compiled for the host from the reference file by oracle/yolo_layer_ref.py (CUDA's __expf becomes expf):
    row order, output layout and class arg-max identical, the NEW_COORDS variant (no exponential in it) bit for bit,
    the sigmoid variant to the last bits of exp()."""
    for k, (head, in_wh) in enumerate(yolo_heads(num_classes, new_coords)):
        H, W = head.shape[1:]
        got = o.yolo_decode(head, YOLO_ANCHORS, num_classes, in_wh, 1.05, new_coords)
        want = ref[f'yolo_{num_classes}_{int(new_coords)}_{k}']
        assert want.shape == got.shape == (3 * H * W, 7)
        np.testing.assert_array_equal(got[:, 5], want[:, 5])
        if new_coords:
            np.testing.assert_array_equal(got, want)
        else:
            np.testing.assert_allclose(got, want, rtol=1e-6, atol=2e-6)
