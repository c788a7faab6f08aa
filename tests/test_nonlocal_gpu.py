"""FM_OP_NONLOCAL (csrc/nonlocal.hip) on the device: one-layer networks against tests/nonlocal_ref.py's float64 reference (the
literal N x N form) under the elementwise bound that module derives -- no tuned constant; a sample's independence of its
batch, bit for bit; then fast-reid-shaped ReID models with non-local blocks from their ONNX bytes in both exporter forms
(models/onnx_graph.py), every layer on the tensors the device itself produced, the embeddings against the torch module under
the measured bar; and the way up through ReID.from_onnx, FeatureExtractor and MOT.step.
Shapes (N, H, W, C): one pixel; fewer pixels than wavefronts with C / 8 = 3 on four lanes; C = 1024 (two loads per pixel);
C = 512 (exactly one pixel per wave load); C = 256 (two pixels per load); C = 2048 on an odd map (four loads per pixel,
the parameters in LDS); channel views at offsets inside wider tensors."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ibn_ref
import nonlocal_ref as NL
import reid_ref
import resnet_ref as R
import torch_ref
from fastmot_amd.engine import HipNet, NET_EXTRACTOR
from fastmot_amd.models import ReID, graph as G, onnx_graph
from fastmot_amd.models.graph import View
from test_reid_ibn_gpu import device_pass

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def restore_feature_width(ctx):
    yield
    ctx.feat_configure(512)


def run_one_layer(ctx, g, x, batches, what):
    """Runs the one-layer graph at each batch over the leading samples of x; -> {batch: the whole output tensor}.  Every run
    is held to the bound; bytes outside the output view and samples beyond the batch keep their values."""
    d = g.layers[0]
    o, hw = d['out'], (d['out'].h, d['out'].w)
    out_c, nmax = g.tensors[o.tid][2], x.shape[0]
    fill = np.random.default_rng(99).normal(0, 1, (nmax,) + hw + (out_c,)).astype(np.float16)
    _, ref, bound = NL.case_reference(g, x)
    eng = HipNet(ctx, NET_EXTRACTOR, g, nmax)
    outs = {}
    try:
        for batch in batches:
            eng.write(g.input, x)
            eng.write(View(o.tid, 0, out_c, *hw), fill)
            eng.run(batch)
            full = eng.read(View(o.tid, 0, out_c, *hw), nmax)
            got = torch.from_numpy(full[:batch, ..., o.coff:o.coff + o.c]).permute(0, 3, 1, 2)
            ratio = ibn_ref.check_layer(got, ref[:batch], bound[:batch], f'{what} batch={batch}')
            print(f'{what} batch={batch}: worst err / bound = {ratio:.3f}')
            keep = np.ones(out_c, bool)
            keep[o.coff:o.coff + o.c] = False
            assert np.array_equal(full[:batch][..., keep], fill[:batch][..., keep].astype(np.float32))
            assert np.array_equal(full[batch:], fill[batch:].astype(np.float32))
            outs[batch] = full
    finally:
        eng.close()
    return outs


@pytest.mark.parametrize('n,h,w,c', NL.CASES)
def test_nonlocal_layer(ctx, n, h, w, c):
    g, x = NL.make_case(n, h, w, c)
    assert [d['op'] for d in g.layers] == [G.OP_NONLOCAL]
    run_one_layer(ctx, g, x, [n], f'nonlocal N={n} {h}x{w} C={c}')


def test_nonlocal_on_channel_views(ctx):
    """Input channels [16, 40) of a 48-channel tensor -> output channels [8, 32) of a 40-channel tensor."""
    g, x = NL.make_case(3, 5, 3, 24, in_off=16, in_c=48, out_off=8, out_c=40)
    d = g.layers[0]
    assert (d['ins'][0].coff, d['out'].coff, g.tensors[d['out'].tid][2]) == (16, 8, 40)
    run_one_layer(ctx, g, x, [1, 3], 'nonlocal on views')


@pytest.mark.parametrize('h,w,c', [(5, 3, 24), (32, 16, 512)])
def test_a_sample_does_not_depend_on_its_batch(ctx, h, w, c):
    """Sample 1 of a batch-3 run is the batch-1 run on it, bit for bit: the order of summation depends on (C, HW) alone."""
    g, x = NL.make_case(3, h, w, c)
    in_batch = run_one_layer(ctx, g, x, [3], f'nonlocal {h}x{w} C={c} in a batch of 3')[3][1]
    alone = run_one_layer(ctx, g, np.ascontiguousarray(x[1:2]), [1], f'nonlocal {h}x{w} C={c} sample 1 alone')[1][0]
    assert np.array_equal(in_batch.view(np.uint32), alone.view(np.uint32))


def test_nonlocal_refuses_tables_that_lie(ctx, monkeypatch):
    """A map above the capacity forced into the op, more channels than the input view holds, an output in place, a parameter
    offset outside the blob: `bad argument` before any launch."""
    def table(mutate, hw=(4, 4)):
        g, _ = NL.make_case(1, hw[0], hw[1], 16)
        mutate(g.layers[0], g)
        return g

    def lie_c(d, g):
        d['cin'] = d['cout'] = 24

    def in_place(d, g):
        d['out'] = d['ins'][0]

    def lie_blob(d, g):
        d['w2_off'] = len(g.blob) + 4096
    tables = [table(m) for m in (lie_c, in_place, lie_blob)]
    monkeypatch.setattr(G.Graph, 'nonlocal_supported', staticmethod(lambda c, hw: True))
    tables.append(table(lambda d, g: None, hw=(128, 64)))           # 8192 pixels
    monkeypatch.undo()
    for g in tables:
        made = []
        try:
            with pytest.raises(Exception, match='bad argument'):
                made.append(HipNet(ctx, NET_EXTRACTOR, g, 1))
                made[0].run(1)
        finally:
            for eng in made:
                eng.close()


# ------------------------------------------------------------------------------------------------ whole networks
def check_every_layer(g, final, emb, label):
    """Every layer from the tensors the DEVICE produced for its inputs (tests/test_reid_ibn_gpu.py's walk, with the new op)."""
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    ratios = {}
    for i, d in enumerate(g.layers):
        own = d['op'] in (G.OP_INSTNORM, G.OP_POOLHEAD, G.OP_NONLOCAL)
        kind, ref, bound = NL.run_layer(g, i, final) if own else NL.run_layer(g, i, final, s_dtype=torch.float32)
        o = d['out']
        got = emb if kind == 'emb' else final[o.tid][:, o.coff:o.coff + o.c]
        op = torch_ref.OP_NAMES[d['op']]
        r = ibn_ref.check_layer(got, ref, bound, f'{label} layer {i} {op} {d.get("name", "")} cin {d["cin"]} cout {d["cout"]} hid {d["hid"]}')
        ratios[op] = max(ratios.get(op, 0.0), r)
    for op, r in sorted(ratios.items()):
        print(f'LAYERBOUND {label:24s} {op:16s} worst err/bound {r:.3g}')
    return ratios


NETS = {'resnet-nl': NL.tiny, 'sbs': NL.tiny_sbs}


@pytest.mark.parametrize('folded', [True, False], ids=['folded', 'unfolded'])
@pytest.mark.parametrize('kind', sorted(NETS))
def test_tiny_files_every_layer_and_embeddings(ctx, kind, folded):
    net = NETS[kind]()
    g, _ = onnx_graph.lower(NL.export(net, folded=folded))
    assert sum(d['op'] == G.OP_NONLOCAL for d in g.layers) == 2
    x = R.random_input(3, (64, 32), seed=11)
    final, emb = device_pass(ctx, g, x, 3)
    ratios = check_every_layer(g, final, emb, f'tiny {kind}')
    assert {'OP_NONLOCAL', 'OP_POOLHEAD'} <= set(ratios) and ('OP_INSTNORM' in ratios) == (kind == 'sbs')
    expect, bar_abs, bar_cos = NL.measured_bar(net, g, x)
    reid_ref.check_embeddings(emb, expect, bar_abs, bar_cos, f'tiny {kind}')


def tiny_descriptor(tmp_path, name):
    net = NL.tiny_sbs()
    path = tmp_path / f'{name}.onnx'
    path.write_bytes(NL.export(net))
    return ReID.from_onnx(path, name=name), net


def test_feature_extractor_with_a_nonlocal_descriptor(ctx, tmp_path):
    """FeatureExtractor over ReID.from_onnx of the SBS-shaped file: more boxes than batch_size, unit norms, the mirror equal to
    the device matrix bit for bit, the embeddings under the measured bar on the crops the device produced."""
    from fastmot_amd.feature_extractor import FeatureExtractor
    desc, net = tiny_descriptor(tmp_path, 'TinySBS')
    size = (640, 360)
    rng = np.random.default_rng(2)
    base = rng.integers(0, 256, (size[1] // 8 + 1, size[0] // 8 + 1, 3)).astype(np.uint8)
    frame = np.clip(np.kron(base, np.ones((8, 8, 1), np.uint8))[:size[1], :size[0]].astype(int) + rng.integers(-20, 20, (size[1], size[0], 3)),
                    0, 255).astype(np.uint8)
    ext = FeatureExtractor('TinySBS', batch_size=4, size=size, reuse_buffers=False)
    assert ext.feature_dim == 256 and sum(d['op'] == G.OP_NONLOCAL for d in ext.graph.layers) == 2 and 'gem_ref' in ext.graph.layers[-1]
    boxes = np.array([[10.7, 20.2, 70.9, 200.1], [-5., -8., 40., 90.], [600., 300., 700., 400.], [100., 50., 131., 113.],
                      [300., 10., 555., 355.], [30., 40., 90., 160.]])
    emb = np.asarray(ext(frame, boxes[:4]), np.float32)
    assert emb.shape == (4, 256) and np.isfinite(emb).all()
    dev = ext.backend.read_embeddings(4)
    assert np.array_equal(emb.view(np.uint32), dev.view(np.uint32))      # what postprocess() hands out is the mirror
    inp = ctx.extract_read_input(4, 32, 64)                              # [n, h, w, 3]: the crops as the network saw them
    x = np.ascontiguousarray(inp.transpose(0, 3, 1, 2)).astype(np.float32)
    expect, bar_abs, bar_cos = NL.measured_bar(net, ext.graph, x)
    reid_ref.check_embeddings(emb, expect, bar_abs, bar_cos, 'FeatureExtractor tiny SBS')
    emb6 = np.asarray(ext(frame, boxes), np.float32)                     # two network passes
    assert emb6.shape == (6, 256) and np.array_equal(emb6[:4].view(np.uint32), emb.view(np.uint32))
    np.testing.assert_allclose(np.linalg.norm(emb6, axis=1), 1, atol=1e-5)


def test_mot_step_with_a_nonlocal_reid_equals_the_cpu_oracle(ctx, tmp_path):
    """MOT.step with the SBS-shaped file as the ReID model: the same track ids, boxes and life cycles as the CPU oracle fed
    the embeddings the device produced (the recipe of tests/test_reid_ibn_gpu.py)."""
    import e2e_check
    import scenes
    import fastmot_amd.mot as mot_mod
    from fastmot_amd.detector import YOLODetector
    from fastmot_amd.models import YOLO
    from synthetic import InjectedYOLODetector, SyntheticVideo
    tiny_descriptor(tmp_path, 'TinySBSMot')

    class NLMotTiny(YOLO):
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
                          yolo_detector_cfg=SimpleNamespace(model='NLMotTiny', conf_thresh=0.25, nms_thresh=0.5,
                                                            max_area=800000, min_aspect_ratio=1.2),
                          feature_extractor_cfgs=(SimpleNamespace(model='TinySBSMot', batch_size=16),),
                          tracker_cfg=SimpleNamespace(**kw))
    finally:
        mot_mod.YOLODetector = YOLODetector
    mot.detector.bind_video(video)
    assert mot.extractors[0].feature_dim == 256
    assert sum(d['op'] == G.OP_NONLOCAL for d in mot.extractors[0].graph.layers) == 2
    hip, emb = e2e_check.hip_pass(mot, video, n_frames, 2, prefetch=True)
    ora, _, _ = e2e_check.oracle_pass(size, mot.extractors[0].metric.lower(), kw, video, n_frames, 2, emb)
    summary = e2e_check.compare(hip, ora)
    mot.tracker._clear_tracks()
    print(summary)
    assert summary['frames'] == n_frames and summary['max_tracks'] >= 6
    assert summary['ids_identical'] and summary['all_identical'], summary['first_mismatch']
