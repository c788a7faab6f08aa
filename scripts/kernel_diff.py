"""Did a change to one source of the library change its device code?  Compiles the file as it is in the tree and as it
was at a commit (gfx950, the flags build.py gives that file), and compares every kernel's assembly instruction for
instruction, plus its register / scratch / LDS directives:
    python scripts/kernel_diff.py flow.hip HEAD^ > profiles/flow_prepare_regs.txt
Compared is the compiler's assembly (-S), where other symbols appear by name: a kernel that merely moved inside the code
object compares equal.  Local labels carry the function's number (.LBB12_3) and are renumbered.  hipcc cross-compiles
without a GPU."""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def kernels(src_text, name, td, tag):
    """{demangled kernel: (instructions, {directive: value})} of one version of the source"""
    sys.path.insert(0, str(ROOT))
    from fastmot_amd.build import FLAGS, FILE_FLAGS
    src = ROOT / 'fastmot_amd' / 'csrc' / f'_{tag}_{name}'          # (beside the headers it includes)
    src.write_text(src_text)
    try:
        flags = [f for f in FLAGS if f not in ('-shared', '-fPIC')] + FILE_FLAGS.get(name, [])
        subprocess.run(['/opt/rocm/bin/hipcc'] + flags + ['--cuda-device-only', '-S', str(src), '-o', f'{td}/{tag}.s'], check=True)
    finally:
        src.unlink()
    text = Path(f'{td}/{tag}.s').read_text()
    out = {}
    for m in re.finditer(r'^(\w+):\s*; @\1\n(.*?)^\s*\.amdhsa_kernel \1\n(.*?)\.end_amdhsa_kernel', text, re.S | re.M):
        body = [re.sub(r'\.L(BB|tmp|func_end|func_begin)\d+', r'.L\1', ln.split(';')[0].strip()) for ln in m[2].splitlines()]
        body = [ln for ln in body if ln and (not ln.startswith('.') or ln.startswith(('.LBB', '.long')))]   # (labels, jump tables)
        res = dict(re.findall(r'\.amdhsa_(\w+) (\S+)', m[3]))        # the whole kernel descriptor takes part
        dem = subprocess.run(['c++filt', m[1]], capture_output=True, text=True).stdout.strip()
        dem = re.sub(r'\(anonymous namespace\)::', '', dem).replace('void ', '')
        out[dem[:dem.find('(')] if '(' in dem else dem] = (body, res)
    return out


def main():
    name, rev = sys.argv[1], sys.argv[2]
    old_text = subprocess.run(['git', 'show', f'{rev}:fastmot_amd/csrc/{name}'], capture_output=True, text=True, check=True).stdout
    with tempfile.TemporaryDirectory() as td:
        old = kernels(old_text, name, td, 'old')
        new = kernels((ROOT / 'fastmot_amd' / 'csrc' / name).read_text(), name, td, 'new')
    print(f'{name}: device code of the tree against {rev} (gfx950; vgpr / sgpr / scratch / lds from the kernel descriptors)')
    print(f'{"kernel":<44} {"verdict":<10} {"instr":>6} {"vgpr":>5} {"sgpr":>5} {"scratch":>7} {"lds":>6}')
    bad = 0
    for k in sorted(set(old) | set(new)):
        if k not in new or k not in old:
            print(f'{k[:44]:<44} {"removed" if k in old else "added"}')
            continue
        same = old[k] == new[k]
        bad += not same
        b, r = new[k]
        print(f'{k[:44]:<44} {"identical" if same else "DIFFERS":<10} {len(b):>6} {r["next_free_vgpr"]:>5} {r["next_free_sgpr"]:>5} '
              f'{r["private_segment_fixed_size"]:>7} {r["group_segment_fixed_size"]:>6}')
        if not same:
            print(f'    before: {len(old[k][0])} instructions, descriptor fields that differ: '
                  f'{ {f: (v, r.get(f)) for f, v in old[k][1].items() if r.get(f) != v} }')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
