"""GPU: redaction inside the overlay pass -- csrc/redact.hip (cell means) and the tile pass of csrc/overlay.hip behind
fm_frame_render_redacted / MOT(redact=...).  The judge is the numpy statement tests/redact_ref.py (and tests/overlay_ref.py
for the commands drawn on top); every comparison is exact."""
import numpy as np
import pytest

import overlay_cases
import overlay_ref
import redact_cases as cases
import redact_ref as R
from fastmot_amd import _lib
from fastmot_amd.utils import jpeg as J
from fastmot_amd.utils.yuv import bgr_to_planar420

pytestmark = pytest.mark.gpu


def upload(ctx, w, h, seed):
    frame = cases.noise(w, h, seed)
    ctx.frame_configure(w, h, 0)
    ctx.frame_upload(frame)
    return frame


def redacted(ctx, regions, cmds=(), masks=b''):
    ctx.frame_render_redacted(R.as_array(regions), cmds, masks)
    return ctx.overlay_read()


def i420(bgr):
    return np.concatenate([p.ravel() for p in bgr_to_planar420(bgr)])


def test_cpu_cases(ctx):
    frame = upload(ctx, cases.W, cases.H, 31)
    for name, regions in cases.all_lists().items():
        assert np.array_equal(redacted(ctx, regions), R.render(frame, regions)), name
    assert ctx.redact_stream_ms() > 0 and ctx.overlay_stream_ms() > 0
    assert np.array_equal(ctx.frame_read(), frame)                       # the tracker's frame is only read


def test_exactly_one_tile(ctx):
    w, h = 64, 16
    frame = upload(ctx, w, h, 32)
    lists = {'whole': [R.region(0, 0, w - 1, h - 1, R.PIXELATE, R.RECT, 5)],
             'beyond': [R.region(-3, -3, 70, 20, R.SMOOTH, R.ELLIPSE, 7)],
             'many': cases.many(w, h, 9)}
    for name, regions in lists.items():
        got = redacted(ctx, regions)
        assert np.array_equal(got, R.render(frame, regions)), name
        assert (got != frame).any(), name


def test_regions_and_cells_straddling_tiles(ctx):
    w, h = 130, 50
    frame = upload(ctx, w, h, 33)
    for name, regions in cases.tiled_lists(w, h).items():
        got = redacted(ctx, regions)
        assert np.array_equal(got, R.render(frame, regions)), name
        assert (got != frame).any(), name
    # more regions than one binning chunk of 256 holds, all on the same tiles: the later chunk wins
    regions = [R.region(20 + k % 7, 5 + k % 5, 90 + k % 11, 40 + k % 3, cases.MODES[k % 3], cases.SHAPES[k % 2], 2 + k % 23, (k % 256, 3, 4))
               for k in range(300)]
    assert np.array_equal(redacted(ctx, regions), R.render(frame, regions))


def test_full_hd_fifty_regions(ctx):
    w, h = 1920, 1080
    frame = upload(ctx, w, h, 34)
    regions = cases.many(w, h, 50)
    assert {r['mode'] for r in regions} == set(cases.MODES) and {r['shape'] for r in regions} == set(cases.SHAPES)
    got = redacted(ctx, regions)
    assert np.array_equal(got, R.render(frame, regions))
    assert (got != frame).any(axis=2).mean() > 0.05


def test_commands_are_drawn_on_the_redacted_pixels(ctx):
    w, h = 130, 50
    frame = upload(ctx, w, h, 35)
    regions = cases.tiled_lists(w, h)['straddle']
    cmds, masks = overlay_cases.scene_commands(w, h)
    got = redacted(ctx, regions, cmds, masks)
    bare = R.render(frame, regions)
    want = overlay_ref.render(bare.copy(), cmds, masks)
    assert np.array_equal(got, want)
    assert (want != bare).any() and (want != overlay_ref.render(frame.copy(), cmds, masks)).any()
    # the same picture as a JPEG file and as planar 4:2:0, from the buffer as it stands
    assert ctx.overlay_encode_jpeg(75) == J.encode_bgr(want, 75, ctx)
    assert np.array_equal(ctx.overlay_export_i420(), i420(want))
    assert np.array_equal(ctx.frame_read(), frame)
    assert ctx.frame_encode_jpeg(75) == J.encode_bgr(frame, 75, ctx)     # the bare frame is still what frame_encode_jpeg codes


@pytest.mark.parametrize('size', [(67, 35), (130, 50)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_no_region_is_render_overlay(ctx, size):
    w, h = size
    frame = upload(ctx, w, h, 36)
    none = np.zeros(0, _lib.REDACT_REGION_DTYPE)
    for name, (cmds, masks) in {'no_commands': ((), b''), 'scene': overlay_cases.scene_commands(w, h)}.items():
        ctx.frame_render_overlay(cmds if len(cmds) else np.zeros(0, _lib.OVERLAY_CMD_DTYPE), masks)
        want = ctx.overlay_read()
        ctx.frame_render_redacted(none, cmds, masks)
        assert np.array_equal(ctx.overlay_read(), want), name
        if name == 'no_commands':
            assert np.array_equal(want, frame)


def test_a_refused_list_leaves_the_last_picture(ctx):
    w, h = 67, 35
    frame = upload(ctx, w, h, 37)
    regions = [R.region(5, 5, 40, 30, R.SMOOTH, R.ELLIPSE, 6)]
    drawn = redacted(ctx, regions)
    bad = R.as_array(regions)
    bad['cell'] = 1
    with pytest.raises(_lib.FastMOTHipError):
        ctx.frame_render_redacted(bad)
    bad_cmds, masks = overlay_cases.scene_commands(w, h)
    bad_cmds = bad_cmds.copy()
    bad_cmds['kind'][0] = 5
    with pytest.raises(_lib.FastMOTHipError):
        ctx.frame_render_redacted(R.as_array(regions), bad_cmds, masks)
    assert np.array_equal(ctx.overlay_read(), drawn) and np.array_equal(ctx.frame_read(), frame)


def test_mot_redact(ctx):
    """Five steps at 320 x 180 with the detector on every second frame, so that frames 1 and 3 are tracked by KLT alone:
    without `redact`, with it on the GPU (pixelate), and with it and draw=True on the host frame.  The tracks are the same;
    every picture the MOT hands out is the reference built from the step's own tracks and detections."""
    from synthetic import SyntheticVideo
    from fastmot_amd import Track
    from fastmot_amd.utils.overlay import build_commands
    from fastmot_amd.utils.redact import Redact, build_regions
    from test_mot_gpu import build_mot
    size = (320, 180)
    video = SyntheticVideo(size, n_ids=5, n_frames=5, seed=7)
    cfg = Redact(mode='pixelate', part='box', margin=0.1, cells=4)
    pictures = []

    def run(redact=None, draw=False, check=None):
        mot = build_mot(size, video, 2)
        mot.redact, mot.draw = redact, draw
        Track._count = 0
        mot.reset(1 / 30.)
        rows = []
        try:
            for f in range(video.n_frames):
                mot.detector._frame_idx = f
                frame = video.frames[f].copy()
                mot.step(frame)
                rows.append([(t.trk_id, tuple(t.tlbr), t.age, t.hits) for t in mot.tracker.tracks.values()])
                if check:
                    check(mot, f, frame)
        finally:
            mot.tracker._clear_tracks()
        return rows

    plain = run()
    klt_only = []

    def check_gpu(mot, f, frame):
        pixels = video.frames[f]
        assert np.array_equal(frame, pixels)                             # the caller's array is not written
        regions = build_regions(mot.tracker.tracks.values(), mot._last_detections, cfg, size)
        assert len(regions) > 0, f
        if len(mot._last_detections) == 0:
            klt_only.append(f)
        bare = R.render(pixels, regions)
        assert mot.encode_frame(75, overlays=False) == J.encode_bgr(bare, 75, ctx), f
        planes = mot.export_frame_i420(overlays=False).data
        assert np.array_equal(planes, i420(bare)), f
        visible = list(mot.visible_tracks())
        cmds, masks = build_commands(mot.visualizer, visible, mot._last_detections, mot.tracker.klt_bboxes.values(),
                                     mot.tracker.flow.prev_bg_keypoints, mot.tracker.flow.bg_keypoints, f'visible: {len(visible)}', size)
        want = overlay_ref.render(bare.copy(), cmds, masks)
        got = mot.render_frame()
        assert np.array_equal(got, want), f
        assert mot.encode_frame(75) == J.encode_bgr(bare, 75, ctx), f    # (gpu_draw is off: the default is the bare picture)
        assert mot.encode_frame(75, overlays=True) == J.encode_bgr(want, 75, ctx), f
        assert np.array_equal(ctx.frame_read(), pixels)                  # the tracker's frame is as it was
        assert np.array_equal(mot.redact_frame(pixels.copy()), bare), f  # the caller's own copy, on the CPU
        # pixelate: every cell of the last region (nothing lies over it) is one colour -- in the luma plane the GPU exported
        luma = planes[:size[0] * size[1]].reshape(size[1], size[0])
        r = regions[-1]
        c, cells = int(r['cell']), 0
        for y0 in range(int(r['y0']), int(r['y1']) + 1, c):
            for x0 in range(int(r['x0']), int(r['x1']) + 1, c):
                block = luma[max(y0, 0):max(min(y0 + c, int(r['y1']) + 1), 0), max(x0, 0):max(min(x0 + c, int(r['x1']) + 1), 0)]
                if block.size:
                    assert (block == block.flat[0]).all(), (f, x0, y0)
                    cells += 1
        assert cells > 1
        pictures.append(got)

    assert run(cfg, check=check_gpu) == plain
    assert klt_only and 0 not in klt_only                                # a frame the detector skipped was covered by its tracks
    assert any(len(row) for row in plain)

    def check_host(mot, f, frame):
        assert np.array_equal(frame, pictures[f]), f                     # redacted in place, then drawn on
    assert run(cfg, draw=True, check=check_host) == plain
