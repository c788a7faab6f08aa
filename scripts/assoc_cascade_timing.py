"""Wall time of MultiTracker.update on a scripted scene (tests/scenes.py), e.g. with every association stage solved the
device way:
    python scripts/assoc_cascade_timing.py s300_4k_multiclass host_lap_elems=0 [zero_copy_tracks=0]
Prints the mean / median / minimum over the scene's update calls of one warm-up run plus three timed runs (microseconds).
The library is the one FASTMOT_LIB_PATH names.  -> profiles/assoc_cascade_ab.txt"""
import os as _os
_os.environ.setdefault('FASTMOT_RANDOM_WEIGHTS', '1')
import sys, time
import numpy as np
sys.path[:0] = ['.', 'oracle', 'tests']
import scenes
from fastmot_amd import MultiTracker, Track
from fastmot_amd.runtime import get_context

name = sys.argv[1] if len(sys.argv) > 1 else 's300_4k_multiclass'
ctx = get_context()
for arg in sys.argv[2:]:
    key, value = arg.split('=')
    ctx.set_option(key, int(value))
scene = scenes.Scene(name)
times = []


class Timed(MultiTracker):
    def update(self, *args, **kw):
        t = time.perf_counter()
        super().update(*args, **kw)
        times.append(time.perf_counter() - t)


for run in range(4):
    Track._count = 0
    tracker = Timed(scene.size, scene.metric, **scenes.tracker_kwargs(name))
    scenes.run_scene(tracker, scene, record_states=False)
    tracker._clear_tracks()
    tracker.reset(1 / 30.)
    if run == 0:
        times.clear()
us = np.array(times) * 1e6
print(f'{name} {" ".join(sys.argv[2:]) or "defaults"}: update x {len(us)}  mean {us.mean():.1f} us  '
      f'median {np.median(us):.1f} us  min {us.min():.1f} us')
