"""Developer diagnostic: per-step cycle stamps of the solo K4 kernel from an NNEST_STAMP + NNEST_STAMP_STEPS build (STEPS=1
tools/build_stamp.sh): propose (with the wait at the barrier), inverse, post (likelihood, decision, apply) of tile 0's first net wave,
and the inverse / post segments of its four net waves (one of them shares its SIMD with the noise wave).
   NNEST_HIP_LIB=tools/ab/lib_STAMP.so python tools/stamp_solo_steps.py [label]
BASELINE config 2 (1000 walkers, x_dim 50, 250 steps), a fixed step and the product's batch rule, three launches each (the format of
profiles/r09/k4_stamps.txt)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from nnest_amd import flow
label = sys.argv[1] if len(sys.argv) > 1 else 'build'
D, C, S = 50, 1000, 250
nvp = flow.HipNVP(D, 16, 3, 1, seed=0)
u0 = np.random.RandomState(0).uniform(-1, 1, size=(C, D))
z0, _ = nvp.forward(u0)
l0 = flow.loglike(0, u0, 5.0)
for tag, kw in (('fixed', {}), ('batch', dict(dynamic='batch'))):
    for rep in range(-2, 3):   # (two launches first: cold caches)
        z, l = z0.clone(), l0.clone()
        res = nvp.mh_steps(0, 5.0, z, l, float(l0.min()), 1 / np.sqrt(D), S, seed=1 + rep, form='solo', **kw)
        o = res['scale'].cpu().numpy()[:16].astype(np.float64) / S
        if rep >= 0:
            print('%-6s %-6s rep %d  cycles per step: total %7.1f  propose %6.1f  inverse %7.1f  post %6.1f   inverse of net waves 0..3: %s   post: %s' % (
                label, tag, rep, o[0], o[1], o[2], o[3], ' '.join('%.1f' % o[8 + 2 * j] for j in range(4)), ' '.join('%.1f' % o[9 + 2 * j] for j in range(4))))
