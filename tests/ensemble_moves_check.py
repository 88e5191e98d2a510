"""A numpy restatement of the ensemble sampler's move mixtures (include/nnest_hip.h nnest_ensemble_moves_steps): per step either
emcee's stretch move (tests/ensemble_check.py stretch_step, unchanged) or emcee's differential-evolution (DE) move, on recorded
draws -- fill_noise's split `inds` [N] and uniforms `u` [N, 3], and fill_moves' move id, second partner `jb` [N] and scale `gamma`
[N] of each step -- or any other draws.  DE proposals are float32 with every operation rounded (the kernels' fp contract off),
lnpdiff float64 without a factor.

`de_step` takes a `wrong` variant so that the CPU suite can check the invariance statistics reject a wrong DE move.
"""
import numpy as np

from tests.ensemble_check import split_sets, stretch_step

STRETCH, DE = 0, 1
DE_SIGMA = 1e-5


def de_gamma0(D):
    """emcee's default DE scale"""
    return 2.38 / np.sqrt(2.0 * D)


def de_step(z, lp, inds, u, jb, gamma, lp_fn, record=None, wrong=None):
    """one DE step of every walker.  z [N, D] float32, lp [N] float64 (updated copies are returned); u [N, 3] float32 (u2: the
    first partner, by the stretch partner's rule; u3: the decision); jb [N]: the second partner as an index into the other set
    (already shifted past the first); gamma [N] float32.  wrong: None, 'pull' (q = z_k + gamma (z_b - z_k): not symmetric) or
    'factor' (a spurious Metropolis factor (D - 1) log(1 + gamma))."""
    z = np.array(z, dtype=np.float32)
    lp = np.array(lp, dtype=np.float64)
    N, D = z.shape
    jb, gamma = np.asarray(jb), np.asarray(gamma, np.float32)
    sets = split_sets(inds)
    for half in (0, 1):
        k, other = sets[half], sets[1 - half]
        u2, u3 = np.asarray(u[k, 1], np.float32), np.asarray(u[k, 2], np.float32)
        m2 = np.round(u2.astype(np.float64) * (1 << 24)).astype(np.int64)
        ja = (m2 * len(other)) >> 24
        assert np.all(jb[k] != ja) and np.all((jb[k] >= 0) & (jb[k] < len(other)))
        a, b = other[ja], other[jb[k]]
        g = gamma[k][:, None]
        if wrong == 'pull':
            q = z[k] + (z[b] - z[k]) * g
        else:
            q = z[k] + (z[b] - z[a]) * g
        assert q.dtype == np.float32
        lpq = np.asarray(lp_fn(q), np.float64)
        factor = (D - 1) * np.log1p(gamma[k].astype(np.float64)) if wrong == 'factor' else 0.0
        with np.errstate(invalid='ignore'):   # (-inf - -inf: NaN, never accepted, as in emcee)
            lnpdiff = factor + lpq - lp[k]
        logu3 = np.log(u3.astype(np.float64))
        acc = lnpdiff > logu3
        if record is not None:
            record.append(dict(half=half, move=DE, walkers=k, partners=a, partners_b=b, q=q.copy(), lp_q=lpq, lnpdiff=lnpdiff,
                               logu3=logu3, accept=acc))
        z[k[acc]] = q[acc]
        lp[k[acc]] = lpq[acc]
    return z, lp


def moves_step(z, lp, inds, u, move, jb, gamma, lp_fn, record=None):
    """one step of every walker: a stretch step through stretch_step, or a DE step"""
    if int(move) == STRETCH:
        rec = None if record is None else []
        out = stretch_step(z, lp, inds, u, lp_fn, record=rec)
        if record is not None:
            for r in rec:
                r['move'] = STRETCH
            record += rec
        return out
    return de_step(z, lp, inds, u, jb, gamma, lp_fn, record=record)


def moves_run(z, lp, draws, lp_fn, wrong=None):
    """steps on draws = [(inds, u, move, jb, gamma), ...]; returns z, lp and whether each walker ever moved"""
    z = np.array(z, dtype=np.float32)
    moved = np.zeros(len(z), bool)
    for inds, u, move, jb, gamma in draws:
        if move == DE and wrong is not None:
            z1, lp = de_step(z, lp, inds, u, jb, gamma, lp_fn, wrong=wrong)
        else:
            z1, lp = moves_step(z, lp, inds, u, move, jb, gamma, lp_fn)
        moved |= np.any(z1 != z, axis=1)
        z = z1
    return z, lp, moved


def numpy_moves_draws(rng, N, S, D, p_stretch, g0=None, sigma=DE_SIGMA):
    """draws with emcee's structure from a numpy generator: per step the split (arange(N) % 2 shuffled), 24-bit uniforms, the move
    (stretch with probability p_stretch), an ordered pair of distinct partners and gamma = g0 (1 + sigma n)"""
    g0 = de_gamma0(D) if g0 is None else g0
    out = []
    for _ in range(S):
        inds = np.arange(N) % 2
        rng.shuffle(inds)
        u = (np.floor(rng.uniform(size=(N, 3)) * (1 << 24)) / (1 << 24)).astype(np.float32)
        move = STRETCH if rng.uniform() < p_stretch else DE
        nc = np.where(inds == 0, np.sum(inds == 1), np.sum(inds == 0))   # the size of each walker's other set
        m2 = np.round(u[:, 1].astype(np.float64) * (1 << 24)).astype(np.int64)
        ja = (m2 * nc) >> 24
        mw = np.floor(rng.uniform(size=N) * (1 << 24)).astype(np.int64)
        jb = (mw * (nc - 1)) >> 24
        jb += jb >= ja
        gamma = (g0 * (1.0 + sigma * rng.standard_normal(N))).astype(np.float32)
        out.append((inds, u, move, jb, gamma))
    return out
