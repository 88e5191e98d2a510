#!/usr/bin/env python3
"""Compare, bit for bit, what two builds' K4 launches computed (developer tool).

Each build dumps its outputs with `python bench.py --bare --steps 3 --warmup 2 --dump-outputs DIR [variant flags]`, one
directory per variant; this script walks the variants of two such trees and requires every array of every pair to be
equal with numpy.array_equal (NaNs compared by their bits).  Exit status 0 only if all pairs are equal.

  python tools/compare_k4_outputs.py BEFORE_DIR AFTER_DIR [--out report.txt]

BEFORE_DIR / AFTER_DIR hold one sub-directory per variant (same names on both sides) with the .npy files of --dump-outputs."""
import os
import sys

import numpy as np


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if np.array_equal(a, b):
        return True
    return a.tobytes() == b.tobytes()   # (NaN payloads: equal bits count as equal)


def main():
    before, after = sys.argv[1], sys.argv[2]
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    lines, bad = [], 0
    variants = sorted(d for d in os.listdir(before) if os.path.isdir(os.path.join(before, d)))
    if not variants:
        lines.append('no variants under %s' % before)
        bad += 1
    for v in variants:
        da, db = os.path.join(before, v), os.path.join(after, v)
        names = sorted(f for f in os.listdir(da) if f.endswith('.npy'))
        if not os.path.isdir(db) or sorted(f for f in os.listdir(db) if f.endswith('.npy')) != names or not names:
            lines.append('%-28s MISSING or different file lists' % v)
            bad += 1
            continue
        for f in names:
            a, b = np.load(os.path.join(da, f)), np.load(os.path.join(db, f))
            ok = same_bits(a, b)
            bad += 0 if ok else 1
            extra = ''
            if not ok and a.shape == b.shape:
                ne = a != b
                extra = '  %d of %d differ, max |diff| %.3g' % (int(ne.sum()), a.size, float(np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64)))))
            lines.append('%-28s %-14s %-10s %-14s %s%s' % (v, f[:-4], a.dtype, 'x'.join(map(str, a.shape)), 'equal' if ok else 'DIFFERENT', extra))
    lines.append('%d arrays compared, %d different' % (sum(1 for l in lines if l.endswith('equal') or 'DIFFERENT' in l), bad))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if out:
        with open(out, 'w') as fh:
            fh.write(text)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
