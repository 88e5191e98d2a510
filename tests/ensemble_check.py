"""A numpy restatement of the ensemble sampler's move (include/nnest_hip.h nnest_ensemble_steps): emcee's stretch move (a = 2, two
sets, a random split per step) on recorded draws -- the split `inds` [N] and the uniforms `u` [N, 3] of each step, as
nnest_ensemble_fill_noise exports them, or any other draws.  Proposals are float32 with every operation rounded (the kernels' fp
contract off), lnpdiff float64.

`stretch_step` records per half-step what the GPU replay compares: the moving walkers, their partners, the proposals, lnpdiff and
log u3.  `jacobian` (default D - 1) exists so that the CPU suite can check the invariance statistics reject a wrong move.
"""
import numpy as np

A = 2.0


def split_sets(inds):
    """set 0 and set 1 of a step, each in ascending walker order"""
    inds = np.asarray(inds)
    return np.flatnonzero(inds == 0), np.flatnonzero(inds == 1)


def stretch_step(z, lp, inds, u, lp_fn, jacobian=None, record=None):
    """one step of every walker.  z [N, D] float32, lp [N] float64 (updated copies are returned); u [N, 3] float32;
    lp_fn(q [n, D] float32) -> lp [n] float64.  record: a list that receives one dict per half-step."""
    z = np.array(z, dtype=np.float32)
    lp = np.array(lp, dtype=np.float64)
    N, D = z.shape
    jac = float(D - 1 if jacobian is None else jacobian)
    sets = split_sets(inds)
    for half in (0, 1):
        k, other = sets[half], sets[1 - half]
        u1, u2, u3 = (np.asarray(u[k, c], np.float32) for c in range(3))
        s = np.float32(A - 1.0) * u1 + np.float32(1.0)
        zz = (s * s) / np.float32(A)
        m2 = np.round(u2.astype(np.float64) * (1 << 24)).astype(np.int64)
        j = other[(m2 * len(other)) >> 24]
        q = z[j] - (z[j] - z[k]) * zz[:, None]
        lpq = np.asarray(lp_fn(q), np.float64)
        with np.errstate(invalid='ignore'):   # (-inf - -inf: NaN, never accepted, as in emcee)
            lnpdiff = jac * np.log(zz.astype(np.float64)) + lpq - lp[k]
        logu3 = np.log(u3.astype(np.float64))
        acc = lnpdiff > logu3
        if record is not None:
            record.append(dict(half=half, walkers=k, partners=j, q=q.copy(), lp_q=lpq, lnpdiff=lnpdiff, logu3=logu3, accept=acc))
        z[k[acc]] = q[acc]
        lp[k[acc]] = lpq[acc]
    return z, lp


def stretch_run(z, lp, draws, lp_fn, jacobian=None):
    """steps of stretch_step on draws = [(inds, u), ...]; returns z, lp and the history of z [N, S, D] and lp [N, S]"""
    hz, hl = [], []
    for inds, u in draws:
        z, lp = stretch_step(z, lp, inds, u, lp_fn, jacobian)
        hz.append(z)
        hl.append(lp)
    return z, lp, np.stack(hz, 1), np.stack(hl, 1)


def numpy_draws(rng, N, S):
    """draws with emcee's structure from a numpy generator: inds = arange(N) % 2 shuffled; u 24-bit uniforms"""
    out = []
    for _ in range(S):
        inds = np.arange(N) % 2
        rng.shuffle(inds)
        u = (np.floor(rng.uniform(size=(N, 3)) * (1 << 24)) / (1 << 24)).astype(np.float32)
        out.append((inds, u))
    return out


def latent_target(x_of_z, logl, in_prior, loglstar=None, logdet_sign=1.0):
    """lp(z) of sampler.py:674-689 for a flow given as x_of_z(q) -> (x, log|det dx/dz|): (logL + ld) + prior, or with loglstar
    -inf below it and ld + prior above.  logdet_sign = -1 states the move with the log-det's sign flipped (the CPU power test)."""
    def lp_fn(q):
        x, ld = x_of_z(q)
        ld = logdet_sign * np.asarray(ld, np.float64)
        ll = np.asarray(logl(x), np.float64)
        prior = np.where(in_prior(x), 0.0, -np.inf)
        if loglstar is None:
            return (ll + ld) + prior
        return np.where(ll < loglstar, -np.inf, ld + prior)
    return lp_fn


def borderline_prefix(record, margin=1e-5):
    """the half-steps that may be compared decision for decision: every one before the first whose replay has a decision within
    `margin` of its threshold (the ensemble couples the walkers, so after one the trajectories may part legitimately)"""
    for n, r in enumerate(record):
        if np.any(np.abs(r['lnpdiff'] - r['logu3']) < margin):
            return n
    return len(record)
