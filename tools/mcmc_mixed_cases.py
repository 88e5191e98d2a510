"""Developer tool, CPU only: chooses the cases of tests/test_gpu_mcmc_mixed.py with the numpy restatement (tests/mcmc_mixed_check.py)
through the oracle's flows on the initialisation the GPU test uses -- the flows' default_init needs no device.

  replay (test 2): per flow and width the first (box, start scale, seed) for which, at k = 2, C = 70, S = 6, the restatement alone has
    at most 0.25 % of its decisions within ten times the lp tolerance of the threshold (the test allows 1 %), proposals of each kind
    fall outside the box, and of the global proposals at least 15 % are accepted and at least 15 % refused (the test asks 10 %);
  corner (test 5): per flow, and per seed 31 .. 36 of the flow and T, the smallest S (a multiple of 10, <= 200) after which every one
    of the N = 2000 walkers started in one corner of the box has moved at k = 1, and the global acceptance over those S steps; the
    test takes seed 35, the one with the smallest S for both flows (60 and 70), and runs 100 steps.

Usage: python tools/mcmc_mixed_cases.py [replay|corner]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import oracle as orc   # noqa: E402
from tests import mcmc_mixed_check as mc   # noqa: E402

CORR = 0.5
SPL_TOL = 3e-5


def nvp_weights(D, seed):
    from nnest_amd.flow import HipNVP
    o = object.__new__(HipNVP)
    o.D, o.H, o.B, o.L, o.scale = D, 16, 3, 1, ''
    o.num_params = 2 * 3 * (16 * D + 16 + (16 * 16 + 16) + D * 16 + D)
    return o.default_init(seed)


def spline_oracle(D, seed, x0):
    """the oracle's spline on HipSpline's default_init(seed), its ActNorm layers set from x0 (the first forward); returns (o, z0)"""
    from nnest_amd.spline import HipSpline
    s = object.__new__(HipSpline)
    s.D, s.H, s.B, s.K = D, 16, 3, 8
    s.nu = D // 2
    s.nl = D - s.nu
    w, P = s.default_init(seed)
    o = orc.Spline(D, 16, 3, 8, 3.0, w, P)
    z0, _ = o.forward(np.asarray(x0, np.float32), data_init=True)
    return o, z0


def affine(D, seed):
    r = np.random.RandomState(seed)
    return r.uniform(0.5, 1.5, D).astype(np.float32), r.uniform(-0.3, 0.3, D).astype(np.float32)


def restated(o, sd, mu, half, beta=1.0):
    T = lambda x: (np.asarray(x, np.float32) * sd) + mu
    inb = lambda x: np.all(np.abs(np.asarray(T(x), np.float64)) <= half, axis=1)
    logl = lambda x: orc.loglike('gaussian', T(x), 1.0, params=[CORR])
    x_of_z = lambda q: o.inverse(np.asarray(q, np.float32))
    return mc.latent_target(x_of_z, logl, inb), x_of_z, inb


def replay_stats(lp_fn, x_of_z, inb, z0, seed, offset, S, k, step, tol):
    C, D = z0.shape
    eps, u = mc.mcmc_draws(seed, offset, C, 0, S, D)
    z, lp = z0, lp_fn(z0)
    border = 0
    out = {True: 0, False: 0}
    acc_g = n_g = 0
    for i in range(S):
        rec = {}
        g = mc.kind(i, k)
        lp_prev = lp
        z, lp = mc.mixed_step(i, k, z, lp, eps[i], u[i], step, lp_fn, record=rec)
        with np.errstate(invalid='ignore'):
            m = 10.0 * tol(np.maximum(np.abs(np.where(np.isfinite(rec['lp_q']), rec['lp_q'], 0.0)),
                                      np.abs(np.where(np.isfinite(lp_prev), lp_prev, 0.0))))
            border += int((np.abs(rec['margin']) < m).sum())
        out[g] += int((~inb(x_of_z(rec['q'])[0])).sum())
        if g:
            acc_g += int(rec['accept'].sum())
            n_g += C
    return border / float(C * S), out[False], out[True], acc_g / float(max(1, n_g))


def choose_replay():
    C, S, k = 70, 6, 2
    for name, D, offset in (('nvp', 5, 0), ('nvp', 50, 1000), ('nvp', 70, 0), ('nvp', 100, 0), ('spline', 5, 0), ('spline', 40, 0)):
        sd, mu = affine(D, D)
        # (x_dim > 50 has no recorded figure: the GPU test measures it; 1e-4 stands in for it here)
        tol = ((lambda v: 2e-5 + 1e-6 * np.abs(v)) if D <= 50 else (lambda v: 1e-4 + 0.0 * v)) if name == 'nvp' else (
            lambda v: SPL_TOL * (1.0 + np.abs(v)))
        found = None
        for half in (2.5, 3.0, 4.0, 5.0, 6.0, 8.0):
            for scale in (0.5, 1.0):
                for seed in range(6000 + D, 6000 + D + 5):
                    x0 = np.random.RandomState(D).normal(size=(C, D)).astype(np.float32) * scale
                    if name == 'nvp':
                        o, z0 = orc.NVP(D, 16, 3, 1, nvp_weights(D, D)), x0
                    else:
                        o, z0 = spline_oracle(D, D, x0)
                    lp_fn, x_of_z, inb = restated(o, sd, mu, half)
                    b, out_l, out_g, ag = replay_stats(lp_fn, x_of_z, inb, z0, seed, offset, S, k, 1.0 / np.sqrt(D), tol)
                    if b <= 0.0025 and out_l > 0 and out_g > 0 and 0.15 <= ag <= 0.85:
                        found = (half, scale, seed, b, out_l, out_g, ag)
                        break
                if found:
                    break
            if found:
                break
        print(name, D, offset, 'box %.1f scale %.1f seed %d: borderline %.4f, outside local %d global %d, global acceptance %.3f'
              % found if found else 'NOTHING FOUND')


def exact_gauss_box(rng, n, D):
    cov = (1 - CORR) * np.eye(D) + CORR * np.ones((D, D))
    out, have = [], 0
    while have < n:
        x = rng.multivariate_normal(np.zeros(D), cov, size=8 * n)
        x = x[np.all(np.abs(x) <= 1.0, axis=1)]
        out.append(x)
        have += len(x)
    return np.concatenate(out)[:n]


CORNER = np.array([0.9, -0.9, 0.9, -0.9, 0.9])   # (a corner of [-1, 1]^5 where the equicorrelated Gaussian is low)


def choose_corner():
    D, N = 5, 2000
    for name in ('nvp', 'spline'):
        for seed in range(31, 37):
            sd, mu = affine(D, seed)
            x0 = ((np.tile(CORNER, (N, 1)) - mu) / sd).astype(np.float32)
            if name == 'nvp':
                o = orc.NVP(D, 16, 3, 1, nvp_weights(D, seed))
            else:   # (the ActNorm layers are set from exact draws of the target, as the invariance test's are)
                tx = exact_gauss_box(np.random.RandomState(seed), N, D)
                o, _ = spline_oracle(D, seed, ((tx - mu) / sd).astype(np.float32))
            z0, _ = o.forward(x0)
            lp_fn, x_of_z, inb = restated(o, sd, mu, 1.0)
            z, lp = np.asarray(z0, np.float32), lp_fn(z0)
            moved = np.zeros(N, bool)
            acc = 0
            for S in range(1, 201):
                eps, u = mc.mcmc_draws(7, 0, N, S - 1, 1, D)
                rec = {}
                z, lp = mc.global_step(z, lp, eps[0], u[0], lp_fn, record=rec)
                moved |= rec['accept']
                acc += int(rec['accept'].sum())
                if S % 10 == 0 and moved.all():
                    break
            print(name, 'seed', seed, 'S', S, 'moved', int(moved.sum()), 'global acceptance %.3f' % (acc / float(N * S)))


if __name__ == '__main__':
    what = sys.argv[1] if len(sys.argv) > 1 else 'replay'
    choose_replay() if what == 'replay' else choose_corner()
