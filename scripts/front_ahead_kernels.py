"""What the front of a pass and the tail of the previous pass cost each other (front-ahead): per detector kernel
(name, grid) the average duration in two rocprofv3 --kernel-trace runs of the bench command, front-ahead off and on.

    python scripts/front_ahead_kernels.py OFF.db ON.db [rows]

Kernels are listed in the order of a pass (first dispatch of each (name, grid) in the OFF run); both runs launch the layers
one by one (FASTMOT_GRAPHS=0: the profiler does not survive hipGraphLaunch in this pipeline), so the overlap is the one of a
host-bound pipeline, not the benchmark's."""
import sqlite3
import sys


def table(path):
    cur = sqlite3.connect(path).cursor()
    rows = cur.execute("select name, grid_x, grid_y, grid_z, workgroup_x, count(*), avg(duration), min(start) from kernels "
                       "group by name, grid_x, grid_y, grid_z").fetchall()
    return {(n, gx // max(wx, 1), gy, gz): (calls, avg / 1e3, first) for n, gx, gy, gz, wx, calls, avg, first in rows}


def main():
    off, on = table(sys.argv[1]), table(sys.argv[2])
    rows = int(sys.argv[3]) if len(sys.argv) > 3 else 200
    calls = sorted(c for c, _, _ in off.values())[len(off) // 2]           # (the median group: one launch per pass)
    keys = [k for k in off if k in on and off[k][0] >= calls * 3 // 4]    # (about once per pass or more: the networks' layers)
    keys.sort(key=lambda k: off[k][2])
    print(f'# {"kernel":<44} {"workgroups":>11} {"calls":>6} {"off us":>8} {"on us":>8} {"on - off":>9}')
    tot = [0., 0.]
    for k in keys[:rows]:
        name = k[0].replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0]
        name = name if len(name) <= 44 else name[:41] + '...'
        wg = k[1] * k[2] * k[3]
        per_pass = off[k][0] / calls
        tot[0] += off[k][1] * per_pass
        tot[1] += on[k][1] * on[k][0] / calls
        print(f'{name:<46} {wg:>11} {off[k][0]:>6} {off[k][1]:>8.2f} {on[k][1]:>8.2f} {on[k][1] - off[k][1]:>+9.2f}')
    print(f'# sum of the listed kernels, weighted by their calls per pass: off {tot[0]:.1f} us, on {tot[1]:.1f} us')


if __name__ == '__main__':
    main()
