"""A numpy restatement of the importance-sampled evidence of a regression (include/nnest_hip.h nnest_importance_glm_evidence,
nnest_spline_importance_glm_evidence), by composition: the draws, the base density, the sums, their merge and the
result are tests/importance_check.py's; the likelihood, its bound B and its sensitivity are tests/glm_check.py's, with its restated
latent target under a box; the normal prior and the latent target under it are tests/gauss_prior_check.py's (RestatedPrior).

A sample m draws z_m from stream 7, x = f^-1(z) through the oracle's flow, t = T(x) in float32, and
    logw = ((logL(t) + log|det|) + prior) - logb(z)     float64
with prior = 0 inside the box +-half on t and -inf outside (no box: 0), or log pi(t) of the GaussianPrior and no box."""
import numpy as np

from tests import gauss_prior_check as gp
from tests import glm_check as gk
from tests import importance_check as ic
from tests.importance_check import importance_draws, is_live, logb, merge, result, sums   # noqa: F401  (re-exported for the tests)


def restated(o, data, sd, mu, half=None, prior=None):
    """the latent target of the kernels on the descriptor `data` through the oracle's flow `o` under T = (sd, mu): under the box
    +-half (None: no box) -- glm_check.Restated -- or under a GaussianPrior -- gauss_prior_check.RestatedPrior, no box"""
    if prior is not None:
        if half is not None:
            raise ValueError('a prior together with a box')
        return gp.RestatedPrior(o, data, prior, sd, mu, half=None, beta=1.0)
    return gk.Restated(o, data, sd, mu, np.inf if half is None else half)


def logw(rs, z):
    """logw [M] float64 of the draws z [M, D] float32 under the restated target"""
    return ic.logw_of(z, rs.lp)


def logprior(rs, x):
    """what the target adds to (logL + log|det|) at the rows x: log pi, or 0 / -inf by the box"""
    if hasattr(rs, 'logpi'):
        return rs.logpi(x)
    return np.where(rs.in_prior(x), 0.0, -np.inf)


def near_face(rs, x, m):
    """rows whose live / dead verdict hangs on a coordinate of T(x) within m of a face of the box: no coordinate is outside by
    more than m, and one is within m of a face.  No box: none"""
    half = getattr(rs, 'half', None)
    if half is None or not np.isfinite(half):
        return np.zeros(len(x), bool)
    t = np.abs(np.asarray(rs.T(x), np.float64)) - half
    return np.all(t <= m, axis=1) & np.any(np.abs(t) <= m, axis=1)


def estimate(lw, t_std=None):
    """the evidence from the log weights: importance_check.result on their sums, with logz = logz_x + sum log|t_std| (the convention
    of Sampler.importance_evidence for a prior on T(x))"""
    lw = np.asarray(lw, np.float64)
    r = dict(ic.result(*ic.sums(lw), len(lw)))
    const = 0.0 if t_std is None else float(np.sum(np.log(np.abs(np.asarray(t_std, np.float64)))))
    r['logz'] = r['logz_x'] + const
    return r
