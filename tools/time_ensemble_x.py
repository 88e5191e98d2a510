"""Developer diagnostic: the x-space stretch run (nnest_ensemble_x_steps, ensemble_x_kernel) -- ms per launch of 250
steps of 1000 walkers at x_dim 50 Rosenbrock, x_dim 20 and x_dim 100 GaussianMix (U = 2, 1, 4), the stretch move alone and the
stretch / DE mixture: 7 launches behind a warm-up launch, each timed by a host clock around work that ends in a device synchronise.
   python tools/time_ensemble_x.py     (NNEST_HIP_LIB selects the library, nnest_amd/_lib.py)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnest_amd import flow  # noqa: E402

NAMES = {0: 'rosenbrock', 1: 'gaussmix'}


def main():
    for D, like_id in ((50, 0), (20, 1), (100, 1)):
        x0 = (np.random.RandomState(0).normal(size=(1000, D)) * 0.5).astype(np.float32)
        sd, mu = np.full(D, 0.5, np.float32), np.zeros(D, np.float32)
        print('x_dim %d, %s, x-space, 1000 walkers x 250 steps' % (D, NAMES[like_id]))
        for tag, moves in (('x stretch', None), ('x mix', {'stretch': 0.5, 'de': 0.5})):
            def fn(seed):
                return flow.ensemble_x_steps(like_id, x0, 250, t_std=sd, t_mean=mu, seed=seed, moves=moves)
            fn(0)
            torch.cuda.synchronize()
            ts = []
            for k in range(7):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(k + 1)
                torch.cuda.synchronize()
                ts.append(1e3 * (time.perf_counter() - t0))
            print('  %-12s %9.3f ms per launch (mean of %d; sd %.3f)' % (tag, np.mean(ts), len(ts), np.std(ts, ddof=1)))


if __name__ == '__main__':
    main()
