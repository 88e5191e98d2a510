"""A numpy restatement of the MIXED walk (include/nnest_hip.h nnest_mcmc_mixed_steps): nnest_mcmc_steps's random-walk Metropolis step
(tests/mcmc_walk_check.rw_step, unchanged) with a flow-independence ("global") step at every k-th step of the run, on recorded draws
-- the normals `eps` [N, D] and the uniform `u` [N] of each step, as nnest_mcmc_fill_noise exports them, or any other draws.  A draw
is used by exactly one kind of step.  The target is the ensemble sampler's (tests/ensemble_check.latent_target).

Global step: the proposal is q = eps (float32, as drawn); with lw(z) = lp(z) - (-1/2 zz(z) - D log sqrt(2 pi)), zz the float64 sum of
the squares of the float32 row, the walker moves iff lw(q) - lw(z) > log u (float64, rw_step's comparison).

`global_step` records what the GPU replay compares: the proposals, lp(q), the margin and the decision.
"""
import numpy as np

from tests.mcmc_walk_check import latent_target, mcmc_draws, rw_step   # noqa: F401  (re-exported for the tests)

LOG_SQRT_2PI = 0.91893853320467274178


def kind(t, k):
    """whether step t (global index) of a run with global_every = k is a global step"""
    return k > 0 and (int(t) + 1) % int(k) == 0


def logb(z):
    """the N(0, I) log density of the rows of z (float32), float64"""
    z = np.asarray(z, np.float32).astype(np.float64)
    return -0.5 * np.sum(z * z, axis=1) - z.shape[1] * LOG_SQRT_2PI


def global_step(z, lp, eps, u, lp_fn, record=None):
    """one global step of every walker.  z [N, D] float32, lp [N] float64 (updated copies are returned); eps [N, D] float32, u [N]
    float32; lp_fn(q [n, D] float32) -> lp [n] float64.  record: a dict that receives q, lp_q, margin and accept."""
    z = np.array(z, dtype=np.float32)
    lp = np.array(lp, dtype=np.float64)
    q = np.array(eps, dtype=np.float32)
    lpq = np.asarray(lp_fn(q), np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):   # (-inf - -inf: NaN, never accepted; log 0 = -inf)
        lnpdiff = 0.0 + (lpq - logb(q)) - (lp - logb(z))
        logu = np.log(np.asarray(u, np.float32).astype(np.float64))
        margin = lnpdiff - logu
    acc = lnpdiff > logu
    if record is not None:
        record.update(q=q.copy(), lp_q=lpq, margin=margin, accept=acc)
    z[acc] = q[acc]
    lp[acc] = lpq[acc]
    return z, lp


def mixed_step(t, k, z, lp, eps, u, step_size, lp_fn, record=None):
    """step t of the run: global_step where kind(t, k), rw_step otherwise"""
    if kind(t, k):
        return global_step(z, lp, eps, u, lp_fn, record=record)
    return rw_step(z, lp, eps, u, step_size, lp_fn, record=record)


def mixed_run(z, lp, draws, step_size, lp_fn, k, step0=0):
    """steps step0 .. of mixed_step on draws = [(eps, u), ...]; returns z, lp, the history of z [N, S, D] and lp [N, S], how often each
    walker moved [N], how often by a global step [N], and the number of global steps"""
    hz, hl = [], []
    n_acc, n_glob = np.zeros(len(z), np.int64), np.zeros(len(z), np.int64)
    n_g = 0
    for i, (eps, u) in enumerate(draws):
        rec = {}
        z, lp = mixed_step(step0 + i, k, z, lp, eps, u, step_size, lp_fn, record=rec)
        n_acc += rec['accept']
        if kind(step0 + i, k):
            n_glob += rec['accept']
            n_g += 1
        hz.append(z)
        hl.append(lp)
    return z, lp, np.stack(hz, 1), np.stack(hl, 1), n_acc, n_glob, n_g
