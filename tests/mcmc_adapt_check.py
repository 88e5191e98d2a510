"""A numpy restatement of the ADAPTIVE walk (include/nnest_hip.h nnest_mcmc_adapt_steps): the mixed walk
(tests/mcmc_mixed_check.mixed_step, unchanged) with the step of the local proposal a float64 `sigma` per walker.  A local step t
proposes q = z + float32(sigma) * eps and, iff t < adapt_steps, the decision moves sigma:

    g     = rate / sqrt(t + 1)
    sigma = sigma * (1 + g * (acc - target))
    sigma = min(max(sigma, STEP_MIN), STEP_MAX)

in float64, every operation rounded -- numpy's division, square root, product and sum are IEEE's, as the device's are, so the kernels'
sigma is reproduced to the bit from the decisions.  Global steps and steps t >= adapt_steps leave sigma alone.
"""
import numpy as np

from tests.mcmc_mixed_check import kind, latent_target, mcmc_draws, mixed_step   # noqa: F401  (re-exported for the tests)

STEP_MIN, STEP_MAX = 1e-8, 1e2


def clamp(sigma):
    """min(max(sigma, STEP_MIN), STEP_MAX) as the kernels write it: each keeps its bound where the comparison is false, so a NaN
    comes out as STEP_MIN (np.maximum would hand the NaN on)"""
    sigma = np.asarray(sigma, np.float64)
    with np.errstate(invalid='ignore'):
        lo = np.where(sigma > STEP_MIN, sigma, STEP_MIN)
        return np.where(lo < STEP_MAX, lo, STEP_MAX)


def step_f32(sigma):
    """the float32 step a local proposal multiplies the draw by"""
    return np.asarray(sigma, np.float64).astype(np.float32)


def adapt_factor(t, acc, rate, target):
    """1 + rate / sqrt(t + 1) * (acc - target), float64, each operation rounded"""
    g = np.float64(rate) / np.sqrt(np.float64(int(t)) + 1.0)
    return 1.0 + g * (np.where(acc, 1.0, 0.0) - np.float64(target))


def adapt_update(sigma, t, acc, rate, target):
    """sigma after the decision(s) `acc` of the local step t < adapt_steps (the caller's conditions)"""
    return clamp(np.asarray(sigma, np.float64) * adapt_factor(t, acc, rate, target))


def adapt_replay(sigma0, moved, k, adapt_steps, rate, target, step0=0):
    """the rule replayed from decisions: sigma0 [N] (as loaded: clamp it first where it came through step_in), moved [N, S] bool;
    returns sigma after each step [N, S]"""
    sigma = np.array(sigma0, np.float64)
    out = np.empty(moved.shape, np.float64)
    for i in range(moved.shape[1]):
        t = step0 + i
        if not kind(t, k) and t < adapt_steps:
            sigma = adapt_update(sigma, t, moved[:, i], rate, target)
        out[:, i] = sigma
    return out


def adapt_run(z, lp, draws, sigma0, lp_fn, k, adapt_steps, rate=1.0, target=0.234, step0=0, records=None):
    """steps step0 .. on draws = [(eps, u), ...] from the walkers' steps sigma0 (a scalar or [N]; as loaded); returns z, lp, the
    history of z [N, S, D], lp [N, S] and sigma [N, S], how often each walker moved [N], how often by a global step [N], and the
    decisions [N, S].  records: a list that receives every step's record (q, lp_q, margin, accept)"""
    z = np.array(z, np.float32)
    sigma = np.broadcast_to(np.asarray(sigma0, np.float64), (len(z),)).copy()
    hz, hl, hs, ha = [], [], [], []
    n_acc, n_glob = np.zeros(len(z), np.int64), np.zeros(len(z), np.int64)
    for i, (eps, u) in enumerate(draws):
        t = step0 + i
        rec = {}
        z, lp = mixed_step(t, k, z, lp, eps, u, step_f32(sigma)[:, None], lp_fn, record=rec)
        acc = rec['accept']
        n_acc += acc
        if kind(t, k):
            n_glob += acc
        elif t < adapt_steps:
            sigma = adapt_update(sigma, t, acc, rate, target)
        hz.append(z)
        hl.append(lp)
        hs.append(sigma.copy())
        ha.append(acc)
        if records is not None:
            records.append(rec)
    return z, lp, np.stack(hz, 1), np.stack(hl, 1), np.stack(hs, 1), n_acc, n_glob, np.stack(ha, 1)
