"""[UNPINNED] CPU checks of the checker of the build-defined slice proposal (oracle/oracle.py::slice_sample; the reference has no
slice proposal, nnest/sampler.py:310-316): the restatement keeps the invariants of a slice-sampling update under a hard constraint,
its uniforms are the Philox words the kernel draws (Random123's known-answer vector pins the generator), and it is a function of
its arguments."""
import numpy as np

from oracle import oracle as orc


def test_philox_known_answer_and_the_uniform_built_on_it():
    # Random123 kat_vectors: philox4x32-10, counter = key = 0 / all ones
    assert orc.philox4x32_10([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert orc.philox4x32_10([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    u = [float(orc.slice_uniform(7, w, k)) for w in range(3) for k in range(64, 70)]
    assert all(0.0 <= v < 1.0 for v in u) and len(set(u)) == len(u)
    assert orc.slice_uniform(7, 1, 64) == orc.slice_uniform(7, 1, 64) and orc.slice_uniform(7, 1, 64) != orc.slice_uniform(8, 1, 64)


def test_slice_sample_keeps_the_constraint_and_moves():
    D, C, S = 4, 12, 6
    rng = np.random.RandomState(0)
    nvp = orc.NVP(D, 16, 3, 1, (rng.uniform(-1, 1, size=orc.NVP(D, 16, 3, 1).n) * 0.3).astype(np.float32))
    u0 = rng.uniform(-0.5, 0.5, size=(C, D))
    l0 = orc.loglike('rosenbrock', u0, 5.0)
    star = float(np.sort(l0)[2])
    keep = l0 > star
    u0, l0 = u0[keep], l0[keep]
    z0, _ = nvp.forward(u0.astype(np.float32))
    dz = rng.standard_normal((S, u0.shape[0], D)).astype(np.float32)
    margins = np.empty((S, u0.shape[0]))
    a = orc.slice_sample(nvp, 'rosenbrock', 5.0, z0, l0, star, 0.7, dz, seed=3, walker_offset=10, margins=margins)
    assert np.all(np.abs(a['x'][:, -1]) <= 1.0) and np.all(a['logl'] > star)
    assert np.all(a['n_eval'] >= a['n_call']) and np.all(a['n_call'] >= a['n_move']) and a['n_move'].mean() > 0.9 * S
    np.testing.assert_allclose(a['logl'], orc.loglike('rosenbrock', a['x'][:, -1], 5.0), rtol=1e-6, atol=1e-6)
    xb, _ = nvp.inverse(a['z'])
    assert np.max(np.abs(xb - a['x'][:, -1])) < 1e-5
    b = orc.slice_sample(nvp, 'rosenbrock', 5.0, z0, l0, star, 0.7, dz, seed=3, walker_offset=10)
    assert np.array_equal(a['x'], b['x']) and np.array_equal(a['n_eval'], b['n_eval'])
    c = orc.slice_sample(nvp, 'rosenbrock', 5.0, z0, l0, star, 0.7, dz, seed=4, walker_offset=10)
    assert not np.array_equal(a['x'], c['x'])
    assert np.all(np.isfinite(margins)) and np.all(margins >= 0)


def test_exact_rosenbrock_evidence_by_transfer_quadrature():
    """oracle/rosenbrock_exact.py (the known answer the slice proposal's convergence is judged by): equals the 2-D closed
    form the nested tests use (-5.804), a brute-force 3-D grid sum of the oracle's own log-likelihood, and is converged in the grid step."""
    from oracle.rosenbrock_exact import log_evidence
    assert abs(log_evidence(2) + 5.804132) < 1e-5
    h = 0.04
    g = np.arange(-5 + h / 2, 5, h)                       # midpoint rule, 250^3 cells
    tot = 0.0
    for x1 in g:
        pts = np.stack(np.meshgrid([x1], g, g, indexing='ij'), axis=-1).reshape(-1, 3) / 5.0
        tot += np.exp(orc.loglike('rosenbrock', pts, 5.0)).sum()
    brute = np.log(tot * h ** 3) - 3 * np.log(10.0)
    assert abs(log_evidence(3) - brute) < 2e-3, (log_evidence(3), brute)
    assert abs(log_evidence(50, h=0.01) - log_evidence(50, h=0.005)) < 1e-6
    assert abs(log_evidence(50) + 231.9384) < 1e-3


def test_stepping_out_keeps_within_its_budget_and_splits_it_at_random():
    """stepping out goes left, then right, to the first grid point outside the slice on each side, if that takes at most
    B = 2 max_stepout expansions; otherwise it restarts and splits B by the update's uniform 63 (Neal 2003, sec. 4.1):
    J = min(B, floor(v (B + 1))) expansions at most to the left, K = B - J to the right.  An identity flow in the box (the slice is
    the chord of the box) with a width small against it, so small budgets are exceeded and large ones are not."""
    D, C, S, w = 2, 24, 4, 0.05
    nvp = orc.NVP(D, 16, 3, 1, np.zeros(orc.NVP(D, 16, 3, 1).n, np.float32))   # the identity flow
    rng = np.random.RandomState(5)
    u0 = rng.uniform(-0.9, 0.9, size=(C, D))
    l0 = orc.loglike('rosenbrock', u0, 5.0)
    dz = rng.standard_normal((S, C, D)).astype(np.float32)
    seed, off = 11, 7
    uni = np.array([[[float(orc.slice_uniform(seed, off + c, 64 * it + k)) for k in (0, 63)] for it in range(1, S + 1)]
                    for c in range(C)])
    for m in (0, 1, 3, 20):
        B = 2 * m
        a = orc.slice_sample(nvp, 'rosenbrock', 5.0, u0.astype(np.float32), l0, -1e30, w, dz, seed, walker_offset=off, max_stepout=m)
        J = np.array([[orc.slice_stepout_split(uni[c, it, 1], m)[0] for it in range(S)] for c in range(C)])
        assert np.array_equal(J, np.minimum(B, np.floor(uni[:, :, 1] * (B + 1))))
        nl, nr, sp = a['n_left'], a['n_right'], a['split']
        assert np.all(nl[sp] <= J[sp]) and np.all(nr[sp] <= B - J[sp])
        assert np.all(nl[~sp] + nr[~sp] <= B)
        for c, it in zip(*np.nonzero(~sp & (B > 0))):   # the full step-out: both ends are the first grid points outside the box
            x, e = a['x'][c, it].astype(np.float64), dz[it, c].astype(np.float64)
            for t_end, t_in in ((-uni[c, it, 0] - nl[c, it], -uni[c, it, 0] - nl[c, it] + 1),
                                (1 - uni[c, it, 0] + nr[c, it], 1 - uni[c, it, 0] + nr[c, it] - 1)):
                out, inn = np.max(np.abs(x + t_end * w * e)), np.max(np.abs(x + t_in * w * e))
                assert out > 1 - 1e-5 and (inn < 1 + 1e-5 or t_in * (t_in - t_end) < 0), (m, c, it, out, inn)
        if m == 0:
            assert not nl.any() and not nr.any() and not sp.any()
        elif m < 20:
            assert sp.mean() > 0.5                                      # the chords are ~30 brackets long
            assert np.any((nl == J) & (J > 0) & sp) and np.any((nr == B - J) & (J < B) & sp)   # the split binds on each side
        else:
            assert sp.mean() < 0.5 and np.any(~sp & (np.maximum(nl, nr) > m))   # beyond what a per-side cap of m would allow
        assert np.all(a['n_eval'] >= (nl + nr + 1).sum(1))             # every expansion is an evaluation, + one shrinkage draw
    assert orc.slice_stepout_split(np.float32(1.0 - 2.0 ** -24), 8) == (16, 0) and orc.slice_stepout_split(np.float32(0.0), 8) == (0, 16)
    assert orc.slice_stepout_split(np.float32(0.5), 8) == (8, 8)
