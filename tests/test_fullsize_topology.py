"""The FULL-SIZE layer tables of the detectors behind BASELINE configs [1], [2], [4] -- real channel widths, the
descriptors' own class counts, strides and head order -- against an interpreter that does not read the table
(VERDICT r4 item 9): tests/darknet_cases.torch_darknet walks the Darknet cfg text section by section in PyTorch;
tests/torch_ref.run_graph walks the lowered `graph.layers` (what tests/test_fullsize_gpu.py compares the engine with).
A topology error in models/yolo.py / darknet.py / graph.py that both the engine and torch_ref would share shows up
here.  Both sides read the same random Darknet `.weights` image; maps at ~1/4 of the descriptor's resolution (the
topology does not depend on it), CPU only, fp32."""
import numpy as np
import pytest
import torch

import darknet_cases as dc
import torch_ref
from fastmot_amd.models import YOLO, darknet, scaled_yolov4


def _cfg_text(name, w, h, classes):
    if name == 'YOLOv4_608':
        return dc.yolov4_cfg(w, h, classes=classes)            # the test suite's own yolov4.cfg (110 conv sections)
    gen = {'YOLOv4CSP_640': scaled_yolov4.yolov4_csp_cfg, 'YOLOv4P6_1280': scaled_yolov4.yolov4_p6_cfg}[name]
    return gen(w, h, classes)                                   # (parameter / FLOP totals pinned in test_scaled_yolov4.py)


@pytest.mark.parametrize('name,n_heads', [('YOLOv4_608', 3), ('YOLOv4CSP_640', 3), ('YOLOv4P6_1280', 4)])
def test_descriptor_table_equals_the_cfg_interpreter(name, n_heads):
    base = YOLO.get_model(name)
    _, H, W = base.INPUT_SHAPE
    h, w = (H // 4 + 31) // 32 * 32, (W // 4 + 31) // 32 * 32         # 160 x 160, 160 x 160, 320 x 320

    class Quarter(base):
        INPUT_SHAPE = (3, h, w)
        MODEL_PATH = None                                       # no model file: topology = the built-in table / generator

    text = _cfg_text(name, w, h, base.NUM_CLASSES)
    cfg = darknet.parse_cfg(text)
    blob = dc.random_weights_file(cfg, seed=11)
    weights = darknet.DarknetWeights(blob)
    g, heads = Quarter.build_graph(weights)
    assert weights.remaining() == 0                             # the table consumed every parameter, in Darknet order
    assert len(heads) == n_heads
    x = torch.from_numpy(np.random.default_rng(3).uniform(0, 1, (1, 3, h, w)).astype(np.float32))
    ref = dc.torch_darknet(cfg, blob, x)
    bufs, _ = torch_ref.run_graph(g, x, emulate_fp16_storage=False)
    assert len(ref) == n_heads
    na = len(base.ANCHORS[0]) // 2
    for hv, r, stride in zip(heads, ref, base.LAYER_FACTORS):
        assert (hv.h, hv.w, hv.c) == (h // stride, w // stride, (base.NUM_CLASSES + 5) * na)
        got = bufs[hv.tid][:, hv.coff:hv.coff + hv.c]
        assert got.shape == r.shape
        err = (got - r).abs().max().item()
        assert err <= 1e-2 * r.abs().max().item() + 1e-3, f'{name} stride {stride}: {err}'    # fp16-rounded weights only


def test_unmerged_csp_table_builds_and_equals_the_merged_one(monkeypatch):
    """FASTMOT_CSP_MERGE=0 (sibling 1x1 convs of a CSP stage as separate layers): the table passes Graph.tables() -- it did
    not while the first sibling was taken for the third stage of the stem launch, whose input the second one still reads --
    and computes what the merged table computes."""
    base = YOLO.get_model('YOLOv4_608')

    class Quarter(base):
        INPUT_SHAPE = (3, 160, 160)
        MODEL_PATH = None

    from fastmot_amd.models.graph import RandomWeights
    x = torch.from_numpy(np.random.default_rng(4).uniform(0, 1, (1, 3, 160, 160)).astype(np.float32))
    outs = []
    for merge in ('1', '0'):
        monkeypatch.setenv('FASTMOT_CSP_MERGE', merge)
        g, heads = Quarter.build_graph(RandomWeights(seed=9))
        g.tables()
        bufs, _ = torch_ref.run_graph(g, x, emulate_fp16_storage=False)
        outs.append((len(g.layers), [bufs[h.tid][:, h.coff:h.coff + h.c] for h in heads]))
    assert outs[1][0] == outs[0][0] + 6
    for a, b in zip(outs[0][1], outs[1][1]):
        assert (a - b).abs().max().item() <= 1e-4 * a.abs().max().item()
