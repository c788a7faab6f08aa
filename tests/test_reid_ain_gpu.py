"""torchreid's OSNet-AIN / OSNet-IBN on the device (models/reid.py VARIANT 'ain' / 'ibn' -> FM_OP_CONVIN, csrc/convin.hip, or with
FASTMOT_CONVIN=0 a linear conv + FM_OP_INSTNORM): every layer of the table on the tensors the device itself produced, under
the per-element bounds of DESIGN.md section 7 (tests/convin_ref.py for the block tails, tests/ibn_ref.py / torch_ref.py for
the rest); the embeddings against the torch module under the measured bar; and the way up through FeatureExtractor and
MOT.step."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import convin_ref
import ibn_ref
import reid_ref
import resnet_ref
import torch_ref
import torchreid_osnet_ain as T
from fastmot_amd.engine import HipNet, NET_EXTRACTOR
from fastmot_amd.models import ReID, graph as G
from fastmot_amd.models.graph import RandomWeights, View
from fastmot_amd.models.torchreid_weights import TorchreidWeights
from torchreid_osnet_ain import TinyIBN025, X025, sd_of, small

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def restore_feature_width(ctx):
    yield
    ctx.feat_configure(512)


def device_pass(ctx, g, x_nchw, batch):
    """-> (tid -> [N, cpad, h, w] torch tensor of what the device holds, embeddings [N, D])."""
    ctx.feat_configure(g.layers[-1]['cout'])
    net = HipNet(ctx, NET_EXTRACTOR, g, batch, reuse_buffers=False)
    try:
        net.write(g.input, np.ascontiguousarray(x_nchw.transpose(0, 2, 3, 1)).astype(np.float16))
        net.run(batch)
        final = {}
        for tid, (h, w, c, f32) in enumerate(g.tensors):
            final[tid] = torch.from_numpy(net.read(View(tid, 0, c, h, w), batch).astype(np.float16)).permute(0, 3, 1, 2)
        return final, net.read_embeddings(batch)
    finally:
        net.close()


def check_every_layer(g, final, emb, label):
    """Every layer from the tensors the DEVICE produced for its inputs (no layer of these tables writes in place)."""
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    ratios = {}
    for i, d in enumerate(g.layers):
        own = d['op'] in (G.OP_INSTNORM, G.OP_CONVIN)
        kind, ref, bound = convin_ref.run_layer(g, i, final) if own else convin_ref.run_layer(g, i, final, s_dtype=torch.float32)
        o = d['out']
        got = emb if kind == 'emb' else final[o.tid][:, o.coff:o.coff + o.c]
        op = torch_ref.OP_NAMES[d['op']]
        r = ibn_ref.check_layer(got, ref, bound, f'{label} layer {i} {op} {d.get("name", "")} cin {d["cin"]} cout {d["cout"]} hid {d["hid"]}')
        ratios[op] = max(ratios.get(op, 0.0), r)
    for op, r in sorted(ratios.items()):
        print(f'LAYERBOUND {label:28s} {op:16s} worst err/bound {r:.3g}')
    return ratios


@pytest.mark.parametrize('convin', [True, False], ids=['fused', 'FASTMOT_CONVIN=0'])
@pytest.mark.parametrize('variant,desc', [('ain', 'OSNetAIN025'), ('ibn', TinyIBN025)], ids=['ain', 'ibn'])
def test_quarter_width_models_every_layer_and_embeddings(ctx, variant, desc, convin, monkeypatch):
    monkeypatch.setenv('FASTMOT_CONVIN', '1' if convin else '0')
    desc = small(ReID.get_model(desc) if isinstance(desc, str) else desc)
    net = T.random_variant(X025, variant, seed=6)
    g, _ = desc.build_graph(TorchreidWeights(sd_of(net), variant))
    o = [d['op'] for d in g.layers]
    assert o.count(G.OP_CONVIN) == (4 if convin else 0) and o.count(G.OP_INSTNORM) == (1 if convin else 5)
    x = resnet_ref.random_input(3, (64, 32), seed=11)
    final, emb = device_pass(ctx, g, x, 3)
    ratios = check_every_layer(g, final, emb, f'{variant} x0.25 {"fused" if convin else "unfused"}')
    assert ('OP_CONVIN' in ratios) == convin and 'OP_INSTNORM' in ratios
    expect, bar_abs, bar_cos = convin_ref.measured_bar(net, g, x)
    reid_ref.check_embeddings(emb, expect, bar_abs, bar_cos, f'{variant} x0.25 {"fused" if convin else "unfused"}')
    np.testing.assert_allclose(np.linalg.norm(emb, axis=1), 1, atol=1e-5)


@pytest.mark.parametrize('name', ['OSNetAIN10', 'OSNetIBN10'])
def test_full_width_models_every_layer(ctx, name, monkeypatch):
    """x1.0 widths at 256 x 128, batch 2, seeded weights: the tails over 64 x 32 (the op's capacity) .. 16 x 8 maps, K up to
    352 (the IBN concat form)."""
    monkeypatch.setenv('FASTMOT_CONVIN', '1')
    g, _ = ReID.get_model(name).build_graph(RandomWeights(seed=1))
    tails = [d for d in g.layers if d['op'] == G.OP_CONVIN]
    assert len(tails) == 4 and max(d['out'].h * d['out'].w for d in tails) == G.CONVIN_MAX_HW
    x = resnet_ref.random_input(2, (256, 128), seed=12)
    final, emb = device_pass(ctx, g, x, 2)
    ratios = check_every_layer(g, final, emb, name)
    assert {'OP_CONVIN', 'OP_INSTNORM'} <= set(ratios)
    np.testing.assert_allclose(np.linalg.norm(emb, axis=1), 1, atol=1e-5)


def test_feature_extractor_with_osnet_ain(ctx):
    """FeatureExtractor with model "OSNetAIN10": more boxes than batch_size, unit norms, the mirror equal to the device
    matrix bit for bit, two passes consistent with one."""
    from fastmot_amd.feature_extractor import FeatureExtractor
    size = (640, 360)
    rng = np.random.default_rng(2)
    base = rng.integers(0, 256, (size[1] // 8 + 1, size[0] // 8 + 1, 3)).astype(np.uint8)
    frame = np.clip(np.kron(base, np.ones((8, 8, 1), np.uint8))[:size[1], :size[0]].astype(int) + rng.integers(-20, 20, (size[1], size[0], 3)),
                    0, 255).astype(np.uint8)
    ext = FeatureExtractor('OSNetAIN10', batch_size=4, size=size, reuse_buffers=False)
    assert ext.feature_dim == 512 and ext.metric.lower() == 'cosine'
    assert sum(d['op'] in (G.OP_CONVIN, G.OP_INSTNORM) for d in ext.graph.layers) >= 5
    boxes = np.array([[10.7, 20.2, 70.9, 200.1], [-5., -8., 40., 90.], [600., 300., 700., 400.], [100., 50., 131., 113.],
                      [300., 10., 555., 355.], [30., 40., 90., 160.]])
    emb = np.asarray(ext(frame, boxes[:4]), np.float32)
    assert emb.shape == (4, 512) and np.isfinite(emb).all()
    dev = ext.backend.read_embeddings(4)
    assert np.array_equal(emb.view(np.uint32), dev.view(np.uint32))
    emb6 = np.asarray(ext(frame, boxes), np.float32)                     # two network passes
    assert emb6.shape == (6, 512) and np.array_equal(emb6[:4].view(np.uint32), emb.view(np.uint32))
    np.testing.assert_allclose(np.linalg.norm(emb6, axis=1), 1, atol=1e-5)
    assert np.abs(emb6[:4] @ emb6[4:].T).max() < 0.9999                  # different crops, different embeddings


def test_mot_step_with_osnet_ain_equals_the_cpu_oracle(ctx):
    """A short MOT.step sequence with OSNetAIN10 as the ReID model: the same track ids, boxes and life cycles as the CPU
    oracle fed the embeddings the device produced (the recipe of tests/test_reid_ibn_gpu.py)."""
    import e2e_check
    import scenes
    import fastmot_amd.mot as mot_mod
    from fastmot_amd.detector import YOLODetector
    from fastmot_amd.models import YOLO
    from synthetic import InjectedYOLODetector, SyntheticVideo

    class AINMotTiny(YOLO):
        NUM_CLASSES = 2
        INPUT_SHAPE = (3, 160, 288)
        LAYER_FACTORS = [8, 16, 32]
        SCALES = [1.2, 1.1, 1.05]
        ANCHORS = [[4, 7, 8, 15, 12, 30], [18, 40, 25, 60, 30, 80], [40, 90, 60, 70, 80, 95]]
    size, n_frames = (960, 540), 10
    video = SyntheticVideo(size, n_ids=6, n_frames=n_frames, seed=21)
    kw = scenes.tracker_kwargs()
    mot_mod.YOLODetector = InjectedYOLODetector
    try:
        mot = mot_mod.MOT(size, detector_type='YOLO', detector_frame_skip=1, class_ids=(1,),
                          yolo_detector_cfg=SimpleNamespace(model='AINMotTiny', conf_thresh=0.25, nms_thresh=0.5,
                                                            max_area=800000, min_aspect_ratio=1.2),
                          feature_extractor_cfgs=(SimpleNamespace(model='OSNetAIN10', batch_size=16),),
                          tracker_cfg=SimpleNamespace(**kw))
    finally:
        mot_mod.YOLODetector = YOLODetector
    mot.detector.bind_video(video)
    assert mot.extractors[0].feature_dim == 512
    assert any(d['op'] in (G.OP_CONVIN, G.OP_INSTNORM) for d in mot.extractors[0].graph.layers)
    hip, emb = e2e_check.hip_pass(mot, video, n_frames, 2, prefetch=True)
    ora, _, _ = e2e_check.oracle_pass(size, mot.extractors[0].metric.lower(), kw, video, n_frames, 2, emb)
    summary = e2e_check.compare(hip, ora)
    mot.tracker._clear_tracks()
    print(summary)
    assert summary['frames'] == n_frames and summary['max_tracks'] >= 4
    assert summary['ids_identical'] and summary['all_identical'], summary['first_mismatch']
