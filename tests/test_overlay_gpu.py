"""GPU: overlays on the device frame -- csrc/overlay.hip behind fm_frame_render_overlay / MOT(gpu_draw=True).

The judge is the library's host renderer (fm_overlay_render_host: csrc/overlay_pixel.h, the text the kernel is compiled
from, run on the CPU), which tests/test_overlay_host.py pins against the numpy statement and against Pillow.  Sizes:
67x35 (201 bytes per row: three rows in four start unaligned, both sides smaller than a tile or no multiple of it), 80x48,
200x40 (several tiles across)."""
import numpy as np
import pytest

import overlay_cases as cases
from fastmot_amd import _lib
from fastmot_amd.utils import jpeg as J

pytestmark = pytest.mark.gpu

SIZES = [(67, 35), (80, 48), (200, 40)]


def upload(ctx, w, h, seed):
    frame = cases.noise(w, h, seed)
    ctx.frame_configure(w, h, 0)
    ctx.frame_upload(frame)
    return frame


@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_render_equals_host_renderer(ctx, size):
    w, h = size
    frame = upload(ctx, w, h, 20)
    lists = dict(cases.primitive_lists(w, h))
    lists['scene'] = cases.scene_commands(w, h)
    lists['scene_no_flags'] = cases.scene_commands(w, h, {})
    for name, (cmds, masks) in lists.items():
        ctx.frame_render_overlay(cmds, masks)
        got = ctx.overlay_read()
        want = _lib.overlay_render_host(frame.copy(), cmds, masks)
        assert np.array_equal(got, want), name
        if name in ('empty', 'outside'):
            assert np.array_equal(got, frame), name
        else:
            assert (got != frame).any(), name
    assert ctx.overlay_stream_ms() > 0


@pytest.mark.parametrize('size', SIZES[:2], ids=lambda s: f'{s[0]}x{s[1]}')
def test_painters_order_across_binning_chunks(ctx, size):
    w, h = size
    frame = upload(ctx, w, h, 21)
    for name, (cmds, masks) in cases.painter_lists(w, h).items():
        assert len(cmds) >= 700                           # three chunks of 256 hit the same tile
        ctx.frame_render_overlay(cmds, masks)
        assert np.array_equal(ctx.overlay_read(), _lib.overlay_render_host(frame.copy(), cmds, masks)), name


def test_tracker_frame_is_untouched_and_bad_lists_are_refused(ctx):
    w, h = 67, 35
    frame = upload(ctx, w, h, 22)
    before = ctx.frame_read()
    cmds, masks = cases.scene_commands(w, h)
    ctx.frame_render_overlay(cmds, masks)
    drawn = ctx.overlay_read()
    assert np.array_equal(ctx.frame_read(), before) and np.array_equal(before, frame)
    assert (drawn != frame).any()
    bad = cmds.copy()
    bad['mask_off'][bad['kind'] == _lib.OVL_MASK] = len(masks)
    with pytest.raises(_lib.FastMOTHipError):
        ctx.frame_render_overlay(bad, masks)
    assert np.array_equal(ctx.overlay_read(), drawn)      # a refused list leaves the last picture
    # another frame size: the picture of the old one is gone until the next render
    ctx.frame_configure(80, 48, 0)
    ctx.frame_upload(cases.noise(80, 48, 23))
    with pytest.raises(_lib.FastMOTHipError):
        ctx.overlay_read()


@pytest.mark.parametrize('size', SIZES[:2], ids=lambda s: f'{s[0]}x{s[1]}')
def test_overlay_encode_equals_encode_of_the_read_back(ctx, size):
    w, h = size
    upload(ctx, w, h, 24)
    ctx.frame_render_overlay(*cases.scene_commands(w, h))
    drawn = ctx.overlay_read()
    assert ctx.overlay_encode_jpeg(75) == J.encode_bgr(drawn, 75, ctx)
    assert ctx.frame_encode_jpeg(75) != ctx.overlay_encode_jpeg(75)      # (the bare frame is still what frame_encode_jpeg codes)


def mot_frames(kind, video, size):
    """(frames handed to the gpu_draw run, the host pixels the tracker sees for them), as tests/test_jpegenc_gpu.py's
    test_mot_encode_frame makes them: a JPEG of every frame against Pillow's decode of it, a 2x upsampled source against
    its resize on the host."""
    import jpeg_cases as jc
    from fastmot_amd import JPEGFrame, SourceFrame
    from fastmot_amd.videoio import resize_bgr
    if kind == 'ndarray':
        return list(video.frames), list(video.frames)
    if kind == 'jpeg':
        files = [jc.encode(np.ascontiguousarray(f[:, :, ::-1]), '420', 90) for f in video.frames]
        return [JPEGFrame(d) for d in files], [jc.pillow_bgr(d) for d in files]
    big = [np.ascontiguousarray(np.repeat(np.repeat(f, 2, 0), 2, 1)) for f in video.frames]
    big[1][::2, ::2] ^= 0x40                                 # (not every 2 x 2 mean is one of its four pixels)
    return [SourceFrame(b) for b in big], [resize_bgr(b, size) for b in big]


@pytest.mark.parametrize('kind', ['ndarray', 'jpeg', 'source'])
def test_mot_gpu_draw_equals_host_draw(ctx, kind):
    """Six steps with every flag on, three ways: MOT(draw=True) on the host pixels, MOT(gpu_draw=True) on the frames as
    ndarray / JPEGFrame / SourceFrame, and a run on those frames that never renders.  Pictures, files and track rows are
    equal; the list is rendered once per step however often the picture is asked for, and never when it is not."""
    from synthetic import SyntheticVideo
    from fastmot_amd import Track
    from fastmot_amd.utils.visualization import Visualizer
    from test_mot_gpu import build_mot
    size = (960, 540)
    video = SyntheticVideo(size, n_ids=8, n_frames=6, seed=5)
    frames, pixels = mot_frames(kind, video, size)
    seen, renders = [], []

    def run(inputs, check=None, draw=False, gpu_draw=False):
        mot = build_mot(size, video, 1)
        mot.draw, mot.gpu_draw = draw, gpu_draw
        mot.visualizer = Visualizer(**cases.ALL_FLAGS)
        render = ctx.frame_render_overlay
        ctx.frame_render_overlay = lambda *a, **k: (renders.append(mot.frame_count), render(*a, **k))[1]
        try:
            Track._count = 0
            mot.reset(1 / 30.)
            rows = []
            for f in range(video.n_frames):
                mot.detector._frame_idx = f
                frame = inputs[f].copy() if draw else inputs[f]
                mot.step(frame, next_frame=inputs[f + 1] if f + 1 < video.n_frames else None)
                rows.append([(t.trk_id, tuple(t.tlbr), t.age, t.hits) for t in mot.tracker.tracks.values()])
                seen.append(len(list(mot.visible_tracks())))
                if check:
                    check(mot, f, frame)
            mot.tracker._clear_tracks()
        finally:
            del ctx.frame_render_overlay
        return rows

    host_drawn = []
    host_rows = run(pixels, lambda mot, f, frame: host_drawn.append(frame), draw=True)
    assert any((d != pixels[f]).any() for f, d in enumerate(host_drawn)) and max(seen) > 0      # boxes of visible tracks among them
    assert not renders

    def check_gpu(mot, f, frame):
        if kind == 'ndarray':
            assert np.array_equal(frame, video.frames[f])                # the caller's array is not drawn on
        assert mot.encode_frame(75, overlays=False) == J.encode_bgr(pixels[f], 75, ctx), f
        assert renders.count(f + 1) == 0                                 # nothing rendered until the picture is asked for
        got = mot.render_frame()
        assert np.array_equal(got, host_drawn[f]), f
        assert mot.encode_frame(75) == J.encode_bgr(host_drawn[f], 75, ctx), f
        assert np.array_equal(mot.render_frame(), host_drawn[f]), f
        assert renders.count(f + 1) == 1                                 # ... and once for all of these
        assert np.array_equal(ctx.frame_read(), pixels[f])               # the tracker's frame is as it was
    assert run(frames, check_gpu, gpu_draw=True) == host_rows
    assert len(renders) == video.n_frames
    assert run(frames, gpu_draw=True) == host_rows
    assert len(renders) == video.n_frames                                # a run that never asks renders nothing
