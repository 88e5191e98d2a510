"""K5 (NVP training) time per epoch at a BASELINE population, multi-CU kernel and single-workgroup kernel (developer diagnostic).
  python tools/time_train.py [x_dim] [n_live]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnest_amd import flow  # noqa: E402

D = int(sys.argv[1]) if len(sys.argv) > 1 else 50
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
rng = np.random.RandomState(0)
live = rng.uniform(-1, 1, size=(N, D))
nv = N // 10
E = 40
perms = torch.stack([torch.randperm(N - nv) for _ in range(E)]).int()
for name, one_cu in (('multi-CU (train_kernel_rows)', False), ('one CU   (train_kernel)', True)):
    nvp = flow.HipNVP(D, 16, 3, 1, seed=1)
    kw = dict(seed=1, jitter=0.01, batch=100, patience=1000, one_cu=one_cu)
    nvp.train_epochs(live[nv:], live[:nv], perms[:2], None, max_epochs=2, **kw)
    torch.cuda.synchronize()
    ts = []
    for k in range(3):
        t0 = time.perf_counter()
        res = nvp.train_epochs(live[nv:], live[:nv], perms, None, max_epochs=E, **kw)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / res['epochs_run'] * 1e3)
    print('x_dim %d, %d live points, %-32s %.3f ms per epoch (%d minibatches: %.1f us each)' % (
        D, N, name, min(ts), (N - nv + 99) // 100, min(ts) * 1e3 / ((N - nv + 99) // 100)))

if os.environ.get('NNEST_HIP_LIB', '').endswith('STAMP.so'):   # NNEST_STAMP build: cycles per phase of a minibatch (workgroup 0)
    nvp = flow.HipNVP(D, 16, 3, 1, seed=1)
    res = nvp.train_epochs(live[nv:], live[:nv], perms, None, max_epochs=E, seed=1, jitter=0.01, batch=100, patience=1000)
    ph = res['losses'].cpu().numpy().ravel()[:8] / (E * ((N - nv + 99) // 100))
    print('rows kernel, cycles per minibatch: forward %d  backward+staging %d  first grid barrier %d  weight-gradient jobs + Adam + publish %d  '
          'workgroup barrier %d  loss + image refresh (tag polls) %d  [first barrier: drain + workgroup barrier %d cycles, %.2f missed polls]' % tuple(ph[:8]))
