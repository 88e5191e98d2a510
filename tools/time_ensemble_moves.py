"""Developer diagnostic: the ensemble sampler's move mixtures (nnest_ensemble_moves_steps) on the two configurations of
tools/time_ensemble.py -- ms per launch of `steps` steps, on the same flow, walkers and seeds:
   (a) fused, stretch 0.5 / DE 0.5      (b) fused, DE only      (c) the round route on the mixture of (a)
   (d) fused, the stretch move alone through the old entry (nnest_ensemble_steps)
One process, the variants ALTERNATED round by round after a warm-up launch of each, so drift hits them alike; per variant the mean,
the standard deviation and the standard error of the mean over the rounds.  Two statements are checked and printed: (a) is faster
than (c) by more than the spread of the two means; and, with --parent-tree DIR (a built checkout of the parent commit), (d) equals
the parent's build of the same entry within the spread of the two means -- timed in fresh child processes, this tree and the
parent's alternated (one library per process).  (a) / (d) is reported, not bounded.
   python tools/time_ensemble_moves.py [--rounds R] [--parent-tree DIR] [x_dim like_id walkers steps] ...
   (default: 50 0 1000 250 and 20 1 1000 250)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {0: 'rosenbrock', 1: 'gaussmix'}


def stats(ts):
    ts = np.asarray(ts, np.float64) * 1e3
    return dict(mean=float(ts.mean()), sd=float(ts.std(ddof=1)) if len(ts) > 1 else 0.0,
                se=float(ts.std(ddof=1) / np.sqrt(len(ts))) if len(ts) > 1 else 0.0, n=len(ts))


def spread(a, b):
    """the spread of the difference of two means: their standard errors in quadrature, times 3"""
    return 3.0 * float(np.hypot(a['se'], b['se']))


def timed(fn, seed):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(seed)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def setup(root, D, like_id, C):
    sys.path.insert(0, root)
    import torch
    from nnest_amd import flow
    nvp = flow.HipNVP(D, 16, 3, 1, seed=0)
    z0 = torch.from_numpy(np.random.RandomState(0).normal(size=(C, D)).astype(np.float32) * 0.5).cuda()
    kw = dict(t_std=np.full(D, 0.5), t_mean=np.zeros(D), lo=np.full(D, -5.0), hi=np.full(D, 5.0))
    return nvp, z0, kw


def child(root, D, like_id, C, S, rounds):
    """(d) alone in this process, from the tree `root`: one JSON line"""
    nvp, z0, kw = setup(root, D, like_id, C)
    fn = lambda seed: nvp.ensemble_steps(like_id, z0, S, seed=seed, **kw)
    timed(fn, 0)
    ts = [timed(fn, 1 + k)[0] for k in range(rounds)]
    print(json.dumps(dict(ts=ts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('cfg', nargs='*', type=int)
    a = ap.parse_args()
    cfg = a.cfg or [50, 0, 1000, 250, 20, 1, 1000, 250]
    if a.child:
        return child(a.child, *cfg[:4], rounds=a.rounds)
    for D, like_id, C, S in zip(*[iter(cfg)] * 4):
        nvp, z0, kw = setup(HERE, D, like_id, C)
        from nnest_amd.ensemble_rounds import ensemble_rounds
        mix, de = {'stretch': 0.5, 'de': 0.5}, {'de': 1.0}
        variants = [('a fused mix', lambda s: nvp.ensemble_steps(like_id, z0, S, seed=s, moves=mix, **kw)),
                    ('b fused de', lambda s: nvp.ensemble_steps(like_id, z0, S, seed=s, moves=de, **kw)),
                    ('c rounds mix', lambda s: ensemble_rounds(nvp, z0, S, like_id=like_id, seed=s, moves=mix, **kw)),
                    ('d fused stretch', lambda s: nvp.ensemble_steps(like_id, z0, S, seed=s, **kw))]
        print('x_dim %d, %s, %d walkers x %d steps (resident: %d walkers with a DE step, %d without)' % (
            D, NAMES.get(like_id, like_id), C, S, nvp.ensemble_max_walkers(like_id, moves=mix), nvp.ensemble_max_walkers(like_id)))
        ts, acc = {n: [] for n, _ in variants}, {}
        for n, fn in variants:   # warm-up
            timed(fn, 0)
        for k in range(a.rounds):
            for n, fn in variants:
                t, out = timed(fn, 1 + k)
                ts[n].append(t)
                n_acc = out['n_accept'] if isinstance(out, dict) else out[0].n_accept
                acc[n] = float(n_acc.sum()) / (C * S)
        st = {n: stats(v) for n, v in ts.items()}
        for n, _ in variants:
            s = st[n]
            print('  %-16s %9.3f ms per launch (mean of %d, sd %.3f, se %.3f), %8.2f us per step, acceptance %.3f' % (
                n, s['mean'], s['n'], s['sd'], s['se'], 1e3 * s['mean'] / S, acc[n]))
        A, Cc, Dd = st['a fused mix'], st['c rounds mix'], st['d fused stretch']
        print('  (c) - (a) = %.3f ms, spread of the two means %.3f ms: (a) faster than (c): %s;  (c) / (a) = %.2fx' % (
            Cc['mean'] - A['mean'], spread(A, Cc), Cc['mean'] - A['mean'] > spread(A, Cc), Cc['mean'] / A['mean']))
        print('  (a) / (d) = %.3f, (b) / (d) = %.3f (reported, not bounded)' % (A['mean'] / Dd['mean'], st['b fused de']['mean'] / Dd['mean']))
        if a.parent_tree:
            del nvp, z0
            both = {'this': [], 'parent': []}
            for k in range(3):   # fresh processes, alternated
                for name, root in (('this', HERE), ('parent', os.path.abspath(a.parent_tree))):
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', root, '--rounds', str(a.rounds),
                                          str(D), str(like_id), str(C), str(S)], capture_output=True, text=True, timeout=300, check=True)
                    both[name] += json.loads(out.stdout.strip().splitlines()[-1])['ts']
            t, p = stats(both['this']), stats(both['parent'])
            print('  (d) this tree %9.3f ms (n %d, sd %.3f, se %.3f);  parent %9.3f ms (n %d, sd %.3f, se %.3f)' % (
                t['mean'], t['n'], t['sd'], t['se'], p['mean'], p['n'], p['sd'], p['se']))
            print('  difference %.3f ms, spread of the two means %.3f ms: equal within it: %s' % (
                t['mean'] - p['mean'], spread(t, p), abs(t['mean'] - p['mean']) <= spread(t, p)))


if __name__ == '__main__':
    main()
