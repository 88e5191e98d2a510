#!/usr/bin/env python3
"""Developer tool: cut one loop out of a kernel listing written by tools/disasm_kernel.py --dump, and compare two such loops up to register
names.  The loop is the body of the backward branch whose length is closest to --len (default 422: the solo K4 lagged-step loop).
  python tools/extract_loop.py KERNEL.s [--len N] [--out LOOP.s]          cut it out (comments and addresses dropped)
  python tools/extract_loop.py --diff A_LOOP.s B_LOOP.s                   same instruction sequence up to register names?  exit 0 / 1"""
import re
import sys


def instructions(path):
    out = []
    for l in open(path):
        l = l.split('//')[0].rstrip()
        if l.strip() and not l.lstrip().startswith(';'):
            out.append(l.strip())
    return out


def cut(path, want):
    rows = []
    for l in open(path):
        m = re.match(r'\s*(.*?)\s*//\s*([0-9A-Fa-f]+):', l)
        if m and m.group(1):
            rows.append((int(m.group(2), 16), m.group(1)))
    addr = {a: i for i, (a, _) in enumerate(rows)}
    best = None
    for i, (a, text) in enumerate(rows):
        m = re.match(r's_c?branch\S*\s+(\d+)', text)
        if not m:
            continue
        off = int(m.group(1))
        off -= 65536 if off >= 32768 else 0
        t = a + 4 + 4 * off
        if off < 0 and t in addr:
            n = i - addr[t] + 1
            if best is None or abs(n - want) < abs(best[0] - want):
                best = (n, addr[t], i)
    n, lo, hi = best
    return [t for _, t in rows[lo:hi + 1]]


def shape(ins):
    s = re.sub(r'\b([vsa])\[\d+:\d+\]', r'\1[R]', ins)
    s = re.sub(r'\b([vsa])\d+\b', r'\1R', s)
    return re.sub(r'(s_c?branch\S*)\s+\d+', r'\1 T', s)


def main():
    if sys.argv[1] == '--diff':
        a, b = instructions(sys.argv[2]), instructions(sys.argv[3])
        sa, sb = [shape(i) for i in a], [shape(i) for i in b]
        import difflib
        ops = [o for o in difflib.SequenceMatcher(None, sa, sb, autojunk=False).get_opcodes() if o[0] != 'equal']
        print('%d / %d instructions; %d places differ up to register names' % (len(a), len(b), len(ops)))
        for tag, i1, i2, j1, j2 in ops[:40]:
            print('  %s at %d / %d' % (tag, i1, j1))
            for k in range(i1, i2):
                print('      - ' + a[k])
            for k in range(j1, j2):
                print('      + ' + b[k])
        return 0 if not ops else 1
    want = int(sys.argv[sys.argv.index('--len') + 1]) if '--len' in sys.argv else 422
    body = cut(sys.argv[1], want)
    text = '\n'.join('\t' + t for t in body) + '\n'
    if '--out' in sys.argv:
        open(sys.argv[sys.argv.index('--out') + 1], 'w').write(text)
    print('%d instructions' % len(body))
    return 0


if __name__ == '__main__':
    sys.exit(main())
