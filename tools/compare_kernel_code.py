#!/usr/bin/env python3
"""Registers, spills, scratch, LDS, occupancy and the instruction stream of every gfx950 kernel whose name contains one of the
given substrings, in two builds of the library side by side (developer tool; no GPU).
  python tools/compare_kernel_code.py PARENT.so TREE.so mcmc_ [more substrings] > profiles/.../resources.txt
"identical": the two disassemblies agree instruction for instruction (addresses and encodings' comments aside); "differs": they do
not, and the line gives the two instruction counts.  Occupancy: waves per SIMD from the unified register file (512 a lane)."""
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, __import__('os').path.dirname(__import__('os').path.abspath(__file__)))
from kernel_resources import READELF, code_objects  # noqa: E402

OBJDUMP = '/opt/rocm/lib/llvm/bin/llvm-objdump'
KEYS = ('vgpr_count', 'agpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size',
        'group_segment_fixed_size')


def kernels(path, pats):
    """name -> (resources, [instructions])"""
    out = {}
    for co in code_objects(open(path, 'rb').read()):
        with tempfile.NamedTemporaryFile(suffix='.co') as f:
            f.write(co)
            f.flush()
            notes = subprocess.run([READELF, '--notes', f.name], capture_output=True, text=True).stdout
            if not any(p in notes for p in pats):
                continue
            txt = subprocess.run([OBJDUMP, '-d', '--demangle', f.name], capture_output=True, text=True).stdout
        res = {}
        for blk in notes.split('- .agpr_count')[1:]:
            blk = '.agpr_count' + blk
            g = lambda k: (re.search(r'\.%s:\s+(\S+)' % k, blk) or [None, '?'])[1]
            res[g('name')] = tuple(g(k) for k in KEYS)
        names = subprocess.run(['c++filt'], input='\n'.join(res), capture_output=True, text=True).stdout.split('\n')
        res = {n.strip(): r for n, r in zip(names, res.values())}
        for m in re.finditer(r'^[0-9a-f]+ <(.*?)>:\n(.*?)(?=^\n|\Z)', txt, re.S | re.M):
            name, body = m.group(1), m.group(2)
            name = re.sub(r'^void ', '', name)
            key = next((n for n in res if re.sub(r'^void ', '', n) == name), None)
            if key is None or not any(p in name for p in pats):
                continue
            ins = [' '.join(l.split('//')[0].split()) for l in body.split('\n')]
            out[name] = (res[key], [i for i in ins if i and not i.startswith('<')])
    return out


def occupancy(vgpr):
    return min(8, 512 // max(8, (int(vgpr) + 7) // 8 * 8))


def main():
    parent, tree, pats = sys.argv[1], sys.argv[2], sys.argv[3:]
    a, b = kernels(parent, pats), kernels(tree, pats)
    print('per kernel: vgpr agpr sgpr vspill sspill scratch lds occupancy, parent | tree')
    same = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print('%-110s only in %s' % (name[:110], 'parent' if name in a else 'tree'))
            continue
        (ra, ia), (rb, ib) = a[name], b[name]
        verdict = 'identical' if ia == ib else 'differs (%d | %d instructions)' % (len(ia), len(ib))
        same += ia == ib
        print('%-110s %s %d | %s %d  %s' % (name[:110], ' '.join(ra), occupancy(ra[0]), ' '.join(rb), occupancy(rb[0]), verdict))
    print('%d kernels, %d identical' % (len(set(a) | set(b)), same))


if __name__ == '__main__':
    main()
