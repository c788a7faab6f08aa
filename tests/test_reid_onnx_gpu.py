"""ResNet-family ReID models from their ONNX files on the device (models/onnx_graph.py -> HIP conv engine):
every layer of the lowered table on the tensors the device itself produced, under the per-element bound of DESIGN.md
section 7 (tests/torch_ref.py for the existing ops, tests/reid_ref.py for FM_OP_POOLHEAD); the embeddings against the
torch module; and the way up through FeatureExtractor, MOT.step and the association at a 2048-wide feature."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

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
            a = net.read(View(tid, 0, c, h, w), batch)
            final[tid] = torch.from_numpy(a.astype(np.float16)).permute(0, 3, 1, 2)
        return final, net.read_embeddings(batch)
    finally:
        net.close()


def check_every_layer(g, final, emb, label):
    """Every layer from the tensors the DEVICE produced for its inputs (no layer of these tables writes in place).
    S, the abs-value convolution of the bound, in float32 (torch_ref.run_layer: its own rounding is second order)."""
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    ratios = {}
    for i, d in enumerate(g.layers):
        kind, ref, bound = reid_ref.run_layer(g, i, final, s_dtype=torch.float32) if d['op'] != G.OP_POOLHEAD else reid_ref.run_layer(g, i, final)
        o = d['out']
        got = emb if kind == 'emb' else final[o.tid][:, o.coff:o.coff + o.c]
        op = torch_ref.OP_NAMES[d['op']]
        r = torch_ref.check_layer(got, ref, bound, f'{label} layer {i} {op} {d.get("name", "")} k{d["k"]} s{d["stride"]} '
                                                   f'cin {d["cin"]} cout {d["cout"]}')
        key = op + (' 1x1 s2' if d['op'] in G.CONV_OPS and d['k'] == 1 and d['stride'] == 2 else '')
        ratios[key] = max(ratios.get(key, 0.0), r)
    for op, r in sorted(ratios.items()):
        print(f'LAYERBOUND {label:24s} {op:16s} worst err/bound {r:.3g}')
    return ratios


@pytest.mark.parametrize('block,pool,head', [('bottleneck', 'ceil', 'bnneck'), ('basic', 'pad1', 'fc512')])
def test_tiny_files_every_layer_and_embeddings(ctx, block, pool, head):
    net = R.tiny(block, pool, head)
    g, _ = onnx_graph.lower(R.export(net))
    x = R.random_input(3, (64, 32), seed=11)
    final, emb = device_pass(ctx, g, x, 3)
    ratios = check_every_layer(g, final, emb, f'tiny {block}')
    assert 'OP_POOLHEAD' in ratios and any(k.endswith('1x1 s2') for k in ratios)
    expect, bar_abs, bar_cos = reid_ref.measured_bar(net, g, x)
    reid_ref.check_embeddings(emb, expect, bar_abs, bar_cos, f'tiny {block} {head}')


def test_resnet50_every_layer_and_embeddings(ctx):
    """ResNet-50 at 256 x 128, batch 4, seeded weights: cin / cout 1024 and 2048 on the DMA-fed and the streamed kernel,
    the strided pointwise convs of the downsample paths on both, a 2048-channel residual operand, the 2048-wide head."""
    net = R.resnet50()
    g, _ = onnx_graph.lower(R.export(net, hw=(256, 128)))
    x = R.random_input(4, (256, 128), seed=12)
    final, emb = device_pass(ctx, g, x, 4)
    ratios = check_every_layer(g, final, emb, 'resnet50')
    assert {'OP_CONVD 1x1 s2', 'OP_CONVS 1x1 s2', 'OP_POOLHEAD', 'OP_STEMPOOL'} <= set(ratios)
    expect, bar_abs, bar_cos = reid_ref.measured_bar(net, g, x)
    reid_ref.check_embeddings(emb, expect, bar_abs, bar_cos, 'resnet50')


def tiny_descriptor(tmp_path, name, head='fc512', fc_dim=24):
    net = R.seeded(R.ResNet('bottleneck', (1, 1, 1, 1), (8, 16, 32, 64), stem=16, head=head, fc_dim=fc_dim), seed=9)
    path = tmp_path / f'{name}.onnx'
    path.write_bytes(R.export(net))
    return ReID.from_onnx(path, name=name), net


def test_feature_extractor_with_an_onnx_descriptor(ctx, tmp_path):
    """FeatureExtractor over a descriptor made by ReID.from_onnx: the reference's preprocessing (crop, resize to
    INPUT_SHAPE, BGR -> RGB, ImageNet mean / std) in front, the embeddings from the page-locked mirror the head wrote --
    equal to the interpreter on the crops the device produced, and to the device matrix bit for bit."""
    import cv_oracle
    from fastmot_amd.feature_extractor import FeatureExtractor
    desc, net = tiny_descriptor(tmp_path, 'TinyOnnxReID')
    size = (640, 360)
    rng = np.random.default_rng(2)
    base = rng.integers(0, 256, (size[1] // 8 + 1, size[0] // 8 + 1, 3)).astype(np.uint8)
    frame = np.clip(np.kron(base, np.ones((8, 8, 1), np.uint8))[:size[1], :size[0]].astype(int) + rng.integers(-20, 20, (size[1], size[0], 3)),
                    0, 255).astype(np.uint8)
    ext = FeatureExtractor('TinyOnnxReID', batch_size=4, size=size, reuse_buffers=False)
    assert ext.feature_dim == 24 and ext.metric == 'euclidean'
    boxes = np.array([[10.7, 20.2, 70.9, 200.1], [-5., -8., 40., 90.], [600., 300., 700., 400.], [100., 50., 131., 113.],
                      [300., 10., 555., 355.], [30., 40., 90., 160.]])
    emb = np.asarray(ext(frame, boxes[:4]), np.float32)
    assert emb.shape == (4, 24)
    dev = ext.backend.read_embeddings(4)
    assert np.array_equal(emb.view(np.uint32), dev.view(np.uint32))      # what postprocess() hands out is the mirror
    inp = ctx.extract_read_input(4, 32, 64)                              # [n, h, w, 3]: the crops as the network saw them
    exp = cv_oracle.reid_preprocess(frame, boxes[:4], in_wh=(32, 64)).transpose(0, 2, 3, 1)
    np.testing.assert_allclose(inp, exp, rtol=0, atol=2.5e-3)            # fp16 storage of values in [-2.2, 2.7]
    x = np.ascontiguousarray(inp.transpose(0, 3, 1, 2)).astype(np.float32)
    expect, bar_abs, bar_cos = reid_ref.measured_bar(net, ext.graph, x)
    reid_ref.check_embeddings(emb, expect, bar_abs, bar_cos, 'FeatureExtractor tiny')
    # more boxes than batch_size: two network passes, the rows of the first are the same bits
    emb6 = np.asarray(ext(frame, boxes), np.float32)
    assert emb6.shape == (6, 24) and np.array_equal(emb6[:4].view(np.uint32), emb.view(np.uint32))
    np.testing.assert_allclose(np.linalg.norm(emb6, axis=1), 1, atol=1e-5)


def test_mot_step_with_an_onnx_reid_equals_the_cpu_oracle(ctx, tmp_path):
    """One MOT.step sequence with a ResNet ReID (D = 256) named in feature_extractor_cfgs: the same track ids, boxes and
    life cycles as the CPU oracle fed the embeddings the device produced (tests/test_e2e_parity_gpu.py's recipe)."""
    import e2e_check
    import scenes
    import fastmot_amd.mot as mot_mod
    from fastmot_amd.detector import YOLODetector
    from fastmot_amd.models import YOLO
    from synthetic import InjectedYOLODetector, SyntheticVideo
    tiny_descriptor(tmp_path, 'TinyOnnxReID256', head='none')

    class OnnxMotTiny(YOLO):
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
                          yolo_detector_cfg=SimpleNamespace(model='OnnxMotTiny', conf_thresh=0.25, nms_thresh=0.5,
                                                            max_area=800000, min_aspect_ratio=1.2),
                          feature_extractor_cfgs=(SimpleNamespace(model='TinyOnnxReID256', batch_size=16),),
                          tracker_cfg=SimpleNamespace(**kw))
    finally:
        mot_mod.YOLODetector = YOLODetector
    mot.detector.bind_video(video)
    assert mot.extractors[0].feature_dim == 256
    hip, emb = e2e_check.hip_pass(mot, video, n_frames, 2, prefetch=True)
    ora, _, _ = e2e_check.oracle_pass(size, mot.extractors[0].metric.lower(), kw, video, n_frames, 2, emb)
    summary = e2e_check.compare(hip, ora)
    mot.tracker._clear_tracks()
    print(summary)
    assert summary['frames'] == n_frames and summary['max_tracks'] >= 6
    assert summary['ids_identical'] and summary['all_identical'], summary['first_mismatch']


def test_association_at_feature_width_2048(ctx):
    """ctx.feat_configure(2048): embedding matrix, running feature averages and the pairwise-cost kernel's dynamic LDS
    are sized by it -- 5 tracks x 5 detections equal the numpy cost."""
    import np_oracle as o
    from fastmot_amd import _lib
    rng = np.random.default_rng(5)
    kf = dict(std_factor_acc=2.25, std_offset_acc=78.5, std_factor_det=(0.08, 0.08), std_factor_klt=(0.14, 0.14),
              min_std_det=(4.0, 4.0), min_std_klt=(5.0, 5.0), init_pos_weight=5, init_vel_weight=12, vel_coupling=0.6, vel_half_life=2)
    ctx.feat_configure(2048)
    ctx.kf_configure(1 / 30., **kf)
    XA = rng.normal(0, 1, (5, 2048)).astype(np.float32)
    XA /= np.linalg.norm(XA, axis=1, keepdims=True)
    XB = (XA[::-1] + rng.normal(0, 0.01, (5, 2048))).astype(np.float32)
    XB /= np.linalg.norm(XB, axis=1, keepdims=True)
    tl = rng.uniform(0, 800, (5, 2))
    tb = np.rint(np.concatenate([tl, tl + rng.uniform(30, 200, (5, 2))], 1))
    slots = np.arange(1, 6)
    ctx.feat_reset(slots)
    ctx.emb_upload(XA)
    ctx.feat_update(slots, np.arange(5))           # (first update of a slot = copy)
    ctx.trk_create(slots, tb)
    _, avg, cnt = ctx.feat_get(int(slots[3]))
    np.testing.assert_allclose(avg, XA[3], rtol=0, atol=1e-6)
    assert cnt == 1
    for metric, mid, tol in (('cosine', _lib.METRIC_COSINE, 2e-7), ('euclidean', _lib.METRIC_EUCLIDEAN, 1e-12)):
        ctx.emb_upload(XB)
        ctx.assoc_prepare(mid, slots, tb, np.ones(5, int), tb[::-1].copy(), np.ones(5, int), np.zeros(5, bool))
        feat, _, _ = ctx.assoc_get_pairwise(5, 5)
        np.testing.assert_allclose(feat, o.cdist(XA.astype(np.float64), XB, metric), rtol=0, atol=1e-13)
        assert (feat.argmin(axis=1) == np.arange(5)[::-1]).all()
