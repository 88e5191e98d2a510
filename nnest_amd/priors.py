"""Priors with the reference's protocol (nnest/priors.py): callable on ONE row -> log density; .sample(n)."""
import numpy as np


class Prior(object):

    def __init__(self, x_dim):
        self.x_dim = x_dim

    def __call__(self, x):
        raise NotImplementedError

    def sample(self, num_samples):
        raise NotImplementedError


class UniformPrior(Prior):
    """Box prior (nnest/priors.py:25-47): 0 inside [minimum, maximum], -inf outside; NaN counts as inside
    because both comparisons are false -- the HIP kernels reproduce exactly that (flow_tile.h inbox_tile)."""

    def __init__(self, x_dim, minimum, maximum):
        self.minimum = np.array([minimum] * x_dim) if not hasattr(minimum, '__len__') else np.array(minimum)
        self.maximum = np.array([maximum] * x_dim) if not hasattr(maximum, '__len__') else np.array(maximum)
        assert len(self.minimum) == x_dim and len(self.maximum) == x_dim
        super(UniformPrior, self).__init__(x_dim)

    def __call__(self, x):
        if np.any(x < self.minimum) or np.any(x > self.maximum):
            return -np.inf
        return 0

    def log_prob_rows(self, x):
        """__call__ over the rows of x[N, D] at once (same comparisons, so NaN rows count as inside too)"""
        out_of_box = np.any(x < self.minimum, axis=1) | np.any(x > self.maximum, axis=1)
        return np.where(out_of_box, -np.inf, 0.0)

    def sample(self, num_samples):
        # numpy global RNG, one uniform block of (n, D) -- same stream consumption as priors.py:45-47
        return self.minimum + (self.maximum - self.minimum) * np.random.uniform(size=(num_samples, self.x_dim))

    def is_unit_box(self):
        return bool(np.all(self.minimum == -1) and np.all(self.maximum == 1))


class GaussianPrior(Prior):
    """Independent normal priors, one per coordinate (BUILD-DEFINED: the reference has the box only): mean and sigma scalars or
    length-x_dim sequences, every sigma finite and positive (ValueError otherwise).  The callable returns the NORMALISED log density
    in float64, -1/2 sum ((x - m) / sigma)^2 - sum log sigma - (D / 2) log 2 pi, so an evidence under it needs no correction.
    `hip_gauss_prior` carries what the fused Metropolis kernels of a GLMData take (include/nnest_hip.h nnest_gauss_prior_t): m
    float32 [D], r = float32(1 / sigma) [D] and logc = -sum log sigma - (D / 2) log 2 pi, a Python float."""

    def __init__(self, x_dim, mean, sigma):
        x_dim = int(x_dim)
        try:
            self.mean = np.broadcast_to(np.asarray(mean, np.float64), (x_dim,)).copy()
            self.sigma = np.broadcast_to(np.asarray(sigma, np.float64), (x_dim,)).copy()
        except ValueError:
            raise ValueError('GaussianPrior: mean and sigma must be scalars or sequences of length x_dim=%d' % x_dim)
        if not np.all(np.isfinite(self.mean)):
            raise ValueError('GaussianPrior: every mean must be finite')
        if not (np.all(np.isfinite(self.sigma)) and np.all(self.sigma > 0.0)):
            raise ValueError('GaussianPrior: every sigma must be finite and positive')
        super(GaussianPrior, self).__init__(x_dim)
        self.logc = float(-np.sum(np.log(self.sigma)) - 0.5 * x_dim * np.log(2.0 * np.pi))
        self.hip_gauss_prior = dict(m=self.mean.astype(np.float32), r=(1.0 / self.sigma).astype(np.float32), logc=self.logc)

    def __call__(self, x):
        u = (np.asarray(x, np.float64) - self.mean) / self.sigma
        return float(-0.5 * np.sum(u * u) + self.logc)

    def log_prob_rows(self, x):
        """__call__ over the rows of x[N, D] at once"""
        u = (np.asarray(x, np.float64) - self.mean) / self.sigma
        return -0.5 * np.sum(u * u, axis=1) + self.logc

    def sample(self, num_samples):
        # numpy global RNG, one normal block of (n, D), as UniformPrior.sample takes one uniform block
        return self.mean + self.sigma * np.random.standard_normal(size=(num_samples, self.x_dim))
