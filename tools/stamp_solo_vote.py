"""Developer diagnostic: the chain of an exact step's vote in the solo K4 kernel, segment by segment, from an NNEST_STAMP +
NNEST_STAMP_VOTE build (VOTE=1 tools/build_stamp.sh): s_memtime cycles of tile 0's relay wave and of its first net wave, averaged over the
exact steps of a launch.
   NNEST_HIP_LIB=tools/ab/lib_STAMP.so python tools/stamp_solo_vote.py [label]
BASELINE config 2 (1000 walkers, x_dim 50, 250 steps): a lag-0 launch (249 exact steps) and the product's rule (16 exact steps, then
lag 8); two launches first (cold caches), then three.

Relay wave, per exact step, in the order of the chain:
  A>post     barrier A passed .. the tile's accepts read from LDS and the post issued
  post>P     .. barrier P passed
  P>read     .. the first counter read issued
  read>hit   the first read issued .. the read that saw every arrival issued (0 if the first read was complete)
  hit>ret    that read issued .. returned
  ret>vote   .. the vote known
  rule       the rule's arithmetic between the vote and the LDS writes
  write>B    the LDS writes .. barrier B reached
  B wait     barrier B reached .. passed
  B>A        barrier B passed .. the next barrier A passed (the net waves' accept flags; the relay's next pair of outcomes)
  reads      counter reads per vote;  first saw: the arrivals the first read saw, of the tiles
First net wave: B>A reached, the wait at A, A passed .. both finish calls done, done .. B passed (the wait for the vote)."""
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
RELAY = ['A>post', 'post>P', 'P>read', 'read>hit', 'hit>ret', 'rule', 'write>B', 'B>A', 'ret>vote', 'B wait']
ORDER = [0, 1, 2, 3, 4, 8, 5, 6, 9, 7]
for tag, kw in (('lag0', dict(dynamic='batch', lag=0)), ('default', dict(dynamic='batch'))):
    for rep in range(-2, 3):
        z, l = z0.clone(), l0.clone()
        res = nvp.mh_steps(0, 5.0, z, l, float(l0.min()), 1 / np.sqrt(D), S, seed=1 + rep, form='solo', **kw)
        flow.HipNVP.check_sync(res)
        o = res['scale'].cpu().numpy().astype(np.float64)
        if rep < 0:
            continue
        n, tiles = o[52], o[53]
        r = o[40:50] / n
        r[7] = o[47] / max(n - 1, 1)
        w = o[54:58] / n
        w[0] = o[54] / max(n - 1, 1)
        chain = r[[0, 1, 2, 3, 4, 8, 5, 6, 9, 7]].sum()
        print('%-10s %-7s rep %d  %3d exact steps  relay: %s  | period %7.1f  reads %.2f  first saw %5.1f of %d' % (
            label, tag, rep, n, '  '.join('%s %6.1f' % (RELAY[i], r[i]) for i in ORDER), chain, o[50] / n, o[51] / n, tiles))
        print('%-10s %-7s rep %d  %3d exact steps  net 0: B>A %6.1f  A wait %6.1f  A>finished %7.1f  finished>B passed %7.1f  | period %7.1f' % (
            label, tag, rep, n, w[0], w[1], w[2], w[3], w.sum()))
