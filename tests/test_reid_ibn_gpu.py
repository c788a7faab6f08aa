"""IBN-Net ReID models from their ONNX files on the device (models/onnx_graph.py -> FM_OP_INSTNORM, GeM in FM_OP_POOLHEAD):
every layer of the lowered table on the tensors the device itself produced, under the per-element bounds of DESIGN.md
section 7 (tests/ibn_ref.py for the two new stages, tests/reid_ref.py / tests/torch_ref.py for the rest); the embeddings
against the torch module under the measured bar; and the way up through ReID.from_onnx, FeatureExtractor and MOT.step."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ibn_ref
import reid_ref
import resnet_ref as R
import torch_ref
from fastmot_amd.engine import HipNet, NET_EXTRACTOR
from fastmot_amd.models import ReID, graph as G, onnx_graph
from fastmot_amd.models.graph import View

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
        own = d['op'] in (G.OP_INSTNORM, G.OP_POOLHEAD)
        kind, ref, bound = ibn_ref.run_layer(g, i, final) if own else ibn_ref.run_layer(g, i, final, s_dtype=torch.float32)
        o = d['out']
        got = emb if kind == 'emb' else final[o.tid][:, o.coff:o.coff + o.c]
        op = torch_ref.OP_NAMES[d['op']]
        r = ibn_ref.check_layer(got, ref, bound, f'{label} layer {i} {op} {d.get("name", "")} cin {d["cin"]} cout {d["cout"]} hid {d["hid"]}')
        ratios[op] = max(ratios.get(op, 0.0), r)
    for op, r in sorted(ratios.items()):
        print(f'LAYERBOUND {label:24s} {op:16s} worst err/bound {r:.3g}')
    return ratios


@pytest.mark.parametrize('kind,kw', [('IBN-a + GeM', dict(ibn='a', pool='gem', head='bnneck')), ('IBN-b', dict(ibn='b'))])
def test_tiny_files_every_layer_and_embeddings(ctx, kind, kw):
    net = ibn_ref.tiny(**kw)
    g, _ = onnx_graph.lower(R.export(net))
    x = R.random_input(3, (64, 32), seed=11)
    final, emb = device_pass(ctx, g, x, 3)
    ratios = check_every_layer(g, final, emb, f'tiny {kind}')
    assert {'OP_INSTNORM', 'OP_POOLHEAD'} <= set(ratios)
    assert ('gem_ref' in g.layers[-1]) == ('pool' in kw)
    expect, bar_abs, bar_cos = ibn_ref.measured_bar(net, g, x)
    reid_ref.check_embeddings(emb, expect, bar_abs, bar_cos, f'tiny {kind}')


def test_resnet50_ibn_a_gem_every_layer(ctx):
    """ResNet-50-IBN-a + GeM + BN neck at 256 x 128, batch 2, seeded weights: 13 instnorm layers with cn 32 / 64 / 128 over
    64 x 32 .. 16 x 8 maps behind linear 1x1 convs, the GeM head at C = 2048."""
    net = ibn_ref.resnet50_ibn_a()
    g, _ = onnx_graph.lower(R.export(net, hw=(256, 128)))
    assert sum(d['op'] == G.OP_INSTNORM for d in g.layers) == 13
    x = R.random_input(2, (256, 128), seed=12)
    final, emb = device_pass(ctx, g, x, 2)
    ratios = check_every_layer(g, final, emb, 'resnet50-ibn-a')
    assert {'OP_INSTNORM', 'OP_POOLHEAD', 'OP_STEMPOOL'} <= set(ratios)
    np.testing.assert_allclose(np.linalg.norm(emb, axis=1), 1, atol=1e-5)


def tiny_descriptor(tmp_path, name, **kw):
    net = ibn_ref.tiny(**kw)
    path = tmp_path / f'{name}.onnx'
    path.write_bytes(R.export(net))
    return ReID.from_onnx(path, name=name), net


def test_feature_extractor_with_an_ibn_descriptor(ctx, tmp_path):
    """FeatureExtractor over ReID.from_onnx of the IBN-a + GeM file: more boxes than batch_size, unit norms, the mirror
    equal to the device matrix bit for bit, the embeddings under the measured bar on the crops the device produced."""
    from fastmot_amd.feature_extractor import FeatureExtractor
    desc, net = tiny_descriptor(tmp_path, 'TinyIBNaGeM', ibn='a', pool='gem', head='bnneck')
    size = (640, 360)
    rng = np.random.default_rng(2)
    base = rng.integers(0, 256, (size[1] // 8 + 1, size[0] // 8 + 1, 3)).astype(np.uint8)
    frame = np.clip(np.kron(base, np.ones((8, 8, 1), np.uint8))[:size[1], :size[0]].astype(int) + rng.integers(-20, 20, (size[1], size[0], 3)),
                    0, 255).astype(np.uint8)
    ext = FeatureExtractor('TinyIBNaGeM', batch_size=4, size=size, reuse_buffers=False)
    assert ext.feature_dim == 256 and sum(d['op'] == G.OP_INSTNORM for d in ext.graph.layers) == 3 and 'gem_ref' in ext.graph.layers[-1]
    boxes = np.array([[10.7, 20.2, 70.9, 200.1], [-5., -8., 40., 90.], [600., 300., 700., 400.], [100., 50., 131., 113.],
                      [300., 10., 555., 355.], [30., 40., 90., 160.]])
    emb = np.asarray(ext(frame, boxes[:4]), np.float32)
    assert emb.shape == (4, 256) and np.isfinite(emb).all()
    dev = ext.backend.read_embeddings(4)
    assert np.array_equal(emb.view(np.uint32), dev.view(np.uint32))      # what postprocess() hands out is the mirror
    inp = ctx.extract_read_input(4, 32, 64)                              # [n, h, w, 3]: the crops as the network saw them
    x = np.ascontiguousarray(inp.transpose(0, 3, 1, 2)).astype(np.float32)
    expect, bar_abs, bar_cos = ibn_ref.measured_bar(net, ext.graph, x)
    reid_ref.check_embeddings(emb, expect, bar_abs, bar_cos, 'FeatureExtractor tiny IBN-a + GeM')
    emb6 = np.asarray(ext(frame, boxes), np.float32)                     # two network passes
    assert emb6.shape == (6, 256) and np.array_equal(emb6[:4].view(np.uint32), emb.view(np.uint32))
    np.testing.assert_allclose(np.linalg.norm(emb6, axis=1), 1, atol=1e-5)


def test_mot_step_with_an_ibn_reid_equals_the_cpu_oracle(ctx, tmp_path):
    """One MOT.step sequence with the IBN-b file as the ReID model: the same track ids, boxes and life cycles as the CPU
    oracle fed the embeddings the device produced (the recipe of tests/test_reid_onnx_gpu.py)."""
    import e2e_check
    import scenes
    import fastmot_amd.mot as mot_mod
    from fastmot_amd.detector import YOLODetector
    from fastmot_amd.models import YOLO
    from synthetic import InjectedYOLODetector, SyntheticVideo
    tiny_descriptor(tmp_path, 'TinyIBNb256', ibn='b', pool='gem')

    class IBNMotTiny(YOLO):
        NUM_CLASSES = 2
        INPUT_SHAPE = (3, 160, 288)
        LAYER_FACTORS = [8, 16, 32]
        SCALES = [1.2, 1.1, 1.05]
        ANCHORS = [[4, 7, 8, 15, 12, 30], [18, 40, 25, 60, 30, 80], [40, 90, 60, 70, 80, 95]]
    size, n_frames = (960, 540), 16
    video = SyntheticVideo(size, n_ids=8, n_frames=n_frames, seed=21)
    kw = scenes.tracker_kwargs()
    mot_mod.YOLODetector = InjectedYOLODetector
    try:
        mot = mot_mod.MOT(size, detector_type='YOLO', detector_frame_skip=1, class_ids=(1,),
                          yolo_detector_cfg=SimpleNamespace(model='IBNMotTiny', conf_thresh=0.25, nms_thresh=0.5,
                                                            max_area=800000, min_aspect_ratio=1.2),
                          feature_extractor_cfgs=(SimpleNamespace(model='TinyIBNb256', batch_size=16),),
                          tracker_cfg=SimpleNamespace(**kw))
    finally:
        mot_mod.YOLODetector = YOLODetector
    mot.detector.bind_video(video)
    assert mot.extractors[0].feature_dim == 256
    assert sum(d['op'] == G.OP_INSTNORM for d in mot.extractors[0].graph.layers) == 3
    hip, emb = e2e_check.hip_pass(mot, video, n_frames, 2, prefetch=True)
    ora, _, _ = e2e_check.oracle_pass(size, mot.extractors[0].metric.lower(), kw, video, n_frames, 2, emb)
    summary = e2e_check.compare(hip, ora)
    mot.tracker._clear_tracks()
    print(summary)
    assert summary['frames'] == n_frames and summary['max_tracks'] >= 6
    assert summary['ids_identical'] and summary['all_identical'], summary['first_mismatch']
