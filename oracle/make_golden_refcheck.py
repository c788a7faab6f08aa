"""TEST INFRASTRUCTURE -- what the reference computes on the seeded inputs of tests/test_oracle_vs_reference.py and
tests/test_motchallenge.py, stored as fixtures so that those tests need no reference tree.  Run where the reference
exists (build container only):

    python oracle/make_golden_refcheck.py
      -> tests/golden/oracle_vs_reference.npz   KalmanFilter, linear_assignment / greedy_match, AverageFeature,
                                                the YOLO decode kernels (oracle/yolo_layer_ref.py)
      -> tests/golden/public_detector_ref.npz   PublicDetector on the synthetic MOTChallenge sequence
      -> tests/golden/MOT20-01_head.txt         the first frames of the reference's eval/results/MOT20-01.txt
"""
import importlib.util
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / 'tests' / 'golden'
for p in (ROOT, ROOT / 'oracle', ROOT / 'tests'):
    sys.path.insert(0, str(p))
import ref_shim  # noqa: E402

MOT20_FRAMES = 110


def oracle_vs_reference(ns):
    import test_oracle_vs_reference as t
    import yolo_layer_ref
    out = {}
    boxes, H, m, c = t.kalman_inputs()
    kf = ns.kalman_filter.KalmanFilter()
    kf.reset_dt(1 / 25.)
    means, covs = [], []
    for i in range(len(boxes)):
        a, b = kf.warp(m[i], c[i], H)
        a, b = kf.predict(a, b)
        a, b = kf.update(a, b, boxes[i] + 2, ns.kalman_filter.MeasType.FLOW, 3.0)
        means.append(a)
        covs.append(b)
    out['kalman_mean'], out['kalman_cov'] = np.array(means), np.array(covs)
    for k, cost in enumerate(t.lap_problems()):
        nr, nc = cost.shape
        rid, cid = list(range(10, 10 + nr)), list(range(nc))
        before = cost.copy()
        for name, res in (('lap', ns.matching.linear_assignment(cost, rid, cid)),
                          ('greedy', ns.matching.greedy_match(cost.copy(), rid, cid, 0.5))):
            mt, ur, uc = res
            out[f'{name}{k}_m'] = np.array([(int(a), int(b)) for a, b in mt], np.int64).reshape(-1, 2)
            out[f'{name}{k}_ur'] = np.array([int(x) for x in ur], np.int64)
            out[f'{name}{k}_uc'] = np.array([int(x) for x in uc], np.int64)
        assert np.array_equal(cost, before, equal_nan=True), 'the reference changed the cost matrix it was given'
    af = ns.track.AverageFeature()
    avgs = []
    for v in t.feature_inputs():
        af.update(v)
        avgs.append(np.array(af.avg, np.float32))
    out['average_feature'] = np.array(avgs)
    for nc, new in t.YOLO_CASES:
        for k, (head, in_wh) in enumerate(t.yolo_heads(nc, new)):
            out[f'yolo_{nc}_{int(new)}_{k}'] = yolo_layer_ref.decode(head, t.YOLO_ANCHORS, nc, in_wh, 1.05, new)
    np.savez_compressed(GOLDEN / 'oracle_vs_reference.npz', **out)


def public_detector(ns):
    import test_motchallenge as t
    sys.modules['fastmot.utils'].TRTInference = object
    for mod, rel in (('utils.decoder', 'utils/decoder.py'), ('detector', 'detector.py')):
        spec = importlib.util.spec_from_file_location('fastmot.' + mod, ref_shim.REF_ROOT / 'fastmot' / rel)
        m = importlib.util.module_from_spec(spec)
        sys.modules['fastmot.' + mod] = m
        spec.loader.exec_module(m)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        t.make_sequence(Path(tmp) / 'seq')
        for size, frame_skip in t.PUBLIC_CASES:
            det = m.PublicDetector(size, (1,), frame_skip, sequence_path=str(Path(tmp) / 'seq'), max_area=400000)
            for step in range(t.PUBLIC_STEPS):
                det.detect_async(None)
                d = det.postprocess()
                key = f'{size[0]}x{size[1]}_skip{frame_skip}_{step}'
                out[key + '_tlbr'] = np.asarray(d.tlbr, np.float64).reshape(-1, 4)
                out[key + '_label'] = np.asarray(d.label, np.int64)
                out[key + '_conf'] = np.asarray(d.conf, np.float64)
    np.savez_compressed(GOLDEN / 'public_detector_ref.npz', **out)


def mot20_head():
    lines = (ref_shim.REF_ROOT / 'eval' / 'results' / 'MOT20-01.txt').read_text().splitlines()
    frames = sorted({int(line.split(',')[0]) for line in lines if line.strip()})[:MOT20_FRAMES]
    keep = [line for line in lines if line.strip() and int(line.split(',')[0]) <= frames[-1]]
    (GOLDEN / 'MOT20-01_head.txt').write_text('\n'.join(keep) + '\n')


if __name__ == '__main__':
    if not ref_shim.reference_available():
        raise SystemExit('the reference tree is not here')
    ns = ref_shim.load_reference()
    try:
        oracle_vs_reference(ns)
        public_detector(ns)
    finally:
        ref_shim.unload_reference(ns)
    mot20_head()
    for name in ('oracle_vs_reference.npz', 'public_detector_ref.npz', 'MOT20-01_head.txt'):
        print(name, (GOLDEN / name).stat().st_size, 'bytes')
