"""The 'choleksy' flow (SingleSpeedCholeksy, nnest/networks.py:162-239) restated with its closed-form training gradient, in numpy at
any precision: float64 is the yardstick of tests/test_gpu_cholesky.py, float32 the measure of what float32 reaches on an input.
tests/test_cholesky_check.py pins it to the reference's autograd gradients in tests/golden/cholesky_*.npz.

y = L x + b, L lower triangular with diag = softplus(unconstrained_diag) + 1e-3 (the reference adds the constant to a float32 tensor:
it is float32(1e-3)); log_probs = log p(y) + sum log diag; loss = -mean(log_probs).  With gy = dE/dy / M (E = -log p):

    d loss / d bias_i       = sum_rows gy[r, i]
    d loss / d lower[i, j]  = sum_rows gy[r, i] x[r, j]           (j < i; packed in np.tril_indices(D, -1) order)
    d loss / d u_i          = (sum_rows gy[r, i] x[r, i] - 1 / diag_i) sigmoid(u_i)

Weights: bias [D], lower_entries [D (D - 1) / 2], unconstrained_diag [D]."""
import math

import numpy as np

EPS = float(np.float32(1e-3))


def shapes(D):
    return [('flow.flows.0.bias', (D,)), ('flow.flows.0.lower_entries', (D * (D - 1) // 2,)), ('flow.flows.0.unconstrained_diag', (D,))]


def parts(w, D, dt=np.float64):
    """(L [D, D] with its diagonal, bias, diag, unconstrained_diag) in dtype dt"""
    nl = D * (D - 1) // 2
    w = np.asarray(w, np.float32)
    b, lo, ud = w[:D].astype(dt), w[D:D + nl].astype(dt), w[D + nl:].astype(dt)
    L = np.zeros((D, D), dt)
    L[np.tril_indices(D, -1)] = lo
    diag = (np.log1p(np.exp(ud)) + dt(EPS)).astype(dt)
    L[np.diag_indices(D)] = diag
    return L, b, diag, ud


def base(y, beta):
    """(log p(y) summed over the dimensions [N], dE/dy [N, D]) of N(0, I) (beta 0) or GeneralisedNormal(0, 1, beta)"""
    dt = y.dtype.type
    if beta == 0:
        return -dt(0.5) * np.sum(y * y, axis=1) - dt(y.shape[1] * 0.5 * math.log(2 * math.pi)), y
    cst = dt(math.log(beta) - math.log(2.0) - math.lgamma(1.0 / beta))
    a = np.abs(y)
    return np.sum(-a ** dt(beta) + cst, axis=1), dt(beta) * a ** dt(beta - 1) * np.sign(y)


def forward(w, X, D, dt=np.float64):
    L, b, diag, _ = parts(w, D, dt)
    X = np.atleast_2d(X).astype(dt)
    return X @ L.T + b, np.full(X.shape[0], np.sum(np.log(diag)), dt)


def inverse(w, Z, D):
    """float64 only: x = L^-1 (z - b)"""
    L, b, diag, _ = parts(w, D)
    Z = np.atleast_2d(Z).astype(np.float64)
    return np.linalg.solve(L, (Z - b).T).T, np.full(Z.shape[0], -np.sum(np.log(diag)))


def inverse32(w, Z, D):
    """the inverse the way a float32 kernel has to do it, forward substitution row by row (torch.triangular_solve, networks.py:210):
    what float32 reaches on an input, for the bounds that depend on the conditioning of L"""
    L, b, diag, _ = parts(w, D, np.float32)
    Z = np.atleast_2d(Z).astype(np.float32)
    out = np.zeros_like(Z)
    for i in range(D):
        out[:, i] = (Z[:, i] - b[i] - out[:, :i] @ L[i, :i]) / diag[i]
    return out


def log_probs(w, X, D, beta=0.0, dt=np.float64):
    y, ld = forward(w, X, D, dt)
    return base(y, beta)[0] + ld


def loss_grad(w, X, D, beta=0.0, dt=np.float64, terms=False):
    """(loss, gradient in packed order) from the closed form; terms=True appends sum_rows |gy[r, i] x[r, j]| for every lower entry:
    the size of what a float32 sum of that element's products can lose"""
    L, b, diag, ud = parts(w, D, dt)
    X = np.atleast_2d(X).astype(dt)
    M = X.shape[0]
    y = X @ L.T + b
    lp, dE = base(y, beta)
    loss = -np.mean(lp + np.sum(np.log(diag)))
    gy = dE / dt(M)
    G = gy.T @ X                                                     # [i, j] = sum_rows gy[r, i] x[r, j]
    gdiag = (np.diag(G) - dt(1) / diag) * (dt(1) / (dt(1) + np.exp(-ud)))
    grad = np.concatenate([gy.sum(axis=0), G[np.tril_indices(D, -1)], gdiag])
    if terms:
        return float(loss), grad.astype(np.float64), (np.abs(gy).T @ np.abs(X))[np.tril_indices(D, -1)].astype(np.float64)
    return float(loss), grad.astype(np.float64)


def case_weights(D, seed=0):
    """lower entries ~ U(-0.3, 0.3), unconstrained_diag from -3 to 25 (across the softplus switch at 20 from x_dim 2 on), bias ~ N(0, 1)"""
    rng = np.random.RandomState(1000 + D + seed)
    return np.concatenate([rng.randn(D), rng.uniform(-0.3, 0.3, D * (D - 1) // 2), np.linspace(-3.0, 25.0, D)]).astype(np.float32)



PASS_ROWS = (1, 63, 64, 65, 1000)
# inverse(forward(x)) in float32 (forward, then forward substitution) against x, relative to 1 + |x|, over pass_rows(128): rounding z
# alone moves x by ulp(z) / diag, diag down to softplus(-3) + 1e-3 = 0.05 under a bias of order 1.  At x_dim <= 33 it stays below 1e-5.
F32_ROUND_TRIP_128 = 1.3e-5
ROUND_TRIP_CAP = 10 * 2 * F32_ROUND_TRIP_128     # ten times the restatement's loss (nvp_vjp_check's rule), itself held within a factor 2


def pass_rows(D):
    """[(N, X [N, D] uniform on [-1, 1])] for the passes"""
    rng = np.random.RandomState(50 + D)
    return [(N, rng.uniform(-1, 1, size=(N, D)).astype(np.float32)) for N in PASS_ROWS]


def round_trip32(w, X, D):
    """max |inverse32(forward32(x)) - x| / (1 + |x|): what float32 loses on these rows"""
    X = np.atleast_2d(X)
    back = inverse32(w, forward(w, X, D, np.float32)[0], D).astype(np.float64)
    return float(np.max(np.abs(back - X) / (1.0 + np.abs(X))))
