"""Developer diagnostic: what a solo K4 launch spends OUTSIDE its step loop -- cycle stamps around the phases of the prologue and the
epilogue of tile 0's first net wave and of its noise wave, from an NNEST_STAMP build (tools/build_stamp.sh):
   NNEST_HIP_LIB=tools/ab/lib_STAMP.so python tools/stamp_prologue.py [--launches N]
BASELINE config 2 (1000 walkers, x_dim 50, 250 steps), the product's batch rule and a fixed step; the median over the launches."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from nnest_amd import flow
N = int(sys.argv[sys.argv.index('--launches') + 1]) if '--launches' in sys.argv else 20
D, C, S = 50, 1000, 250
nvp = flow.HipNVP(D, 16, 3, 1, seed=0)
u0 = np.random.RandomState(0).uniform(-1, 1, size=(C, D))
z0, _ = nvp.forward(u0)
l0 = flow.loglike(0, u0, 5.0)
NET = ['staging', 'etab', 'barrier', 'weights', 'z+inverse', 'wait_P0', 'loop', 'epilogue', 'total']
NOISE = ['staging', 'etab', 'barrier', 'seed+draw0', 'wait_P0', 'rest', 'total']
for tag, kw in (('batch rule', dict(dynamic='batch')), ('fixed step', {})):
    rows = []
    for i in range(N + 2):
        z, l = z0.clone(), l0.clone()
        res = nvp.mh_steps(0, 5.0, z, l, float(l0.min()), 1 / np.sqrt(D), S, seed=1 + i, form='solo', **kw)
        rows.append(res['scale'].cpu().numpy()[:48].astype(np.float64))
    o = np.median(np.array(rows[2:]), axis=0)   # (the first launches: cold caches)
    for who, names, base in (('net wave 0', NET, 16), ('noise wave', NOISE, 32)):
        print('%-10s %-10s ' % (tag, who) + '  '.join('%s %d' % (n, round(o[base + k])) for k, n in enumerate(names)))
    net = dict(zip(NET, o[16:]))
    print('%-10s outside the loop: %d of %d cycles (%.1f %%); loop %.0f cycles per step' % (
        tag, round(net['total'] - net['loop']), round(net['total']), 100.0 * (net['total'] - net['loop']) / net['total'], net['loop'] / S))
