"""DeviceTarget: what the fused routes hand a kernel as the target -- the likelihood (an id the kernels know and its parameters, or
the descriptor of a Gaussian likelihood from user data: `like_data`, or of a regression likelihood of user data: `like_glm`, with
like_id None), the
affine T(x) = x * t_std + t_mean the likelihood sees, and the prior: a box [lo, hi] on T(x), or, beside a `like_glm`, the descriptor of
independent normal priors on T(x): `prior_gauss`.  `Sampler._device_target` decides it, once
per run; every launch of the run takes the same staged tensors (`launch_kwargs`)."""
import numpy as np

_FIXED = ('like_id', 'like_params', 't_std', 't_mean', 'lo', 'hi', 'like_data', 'like_glm', 'prior_gauss')


def affine_on_device(x, t_std, t_mean):
    """T(x) = x * t_std + t_mean on float32 device tensors: two roundings, as the fused kernels compute it"""
    return x * t_std + t_mean


class DeviceTarget(object):
    """like_id, like_params; t_std, t_mean: float32 [D] or both None (the identity); lo, hi: float32 [D] or both None (no prior).
    like_data: None, or the descriptor of a Gaussian likelihood from user data (likelihoods.GaussianData.hip_like_data: mu, R,
    logl0) -- like_id is then None, and the Metropolis bindings route on the `like_data` keyword.
    like_glm: None, or the descriptor of a regression likelihood of user data (likelihoods.GLMData.hip_like_glm: at, y, o, logl0, n,
    family) -- like_id and like_data are then None, and the Metropolis bindings route on the `like_glm` keyword.
    prior_gauss: None, or the descriptor of independent normal priors on T(x) (priors.GaussianPrior.hip_gauss_prior: m, r, logc) --
    only beside a like_glm and without a box (ValueError otherwise); the Metropolis bindings route on the `prior_gauss` keyword.
    The fields are fixed once set: another transform is another target (`with_transform`), so tensors staged for one (std, mean)
    never serve another."""

    def __init__(self, like_id, like_params=(), t_std=None, t_mean=None, lo=None, hi=None, like_data=None, like_glm=None,
                 prior_gauss=None):
        if (t_std is None) != (t_mean is None) or (lo is None) != (hi is None):
            raise ValueError('DeviceTarget: t_std and t_mean, and lo and hi: both or neither')
        vec = lambda v: None if v is None else np.array(v, np.float32).reshape(-1)   # (a copy, cast as the bindings cast)
        if (like_id is not None) + (like_data is not None) + (like_glm is not None) != 1:
            raise ValueError('DeviceTarget: a like_id, or like_id None with a like_data or with a like_glm')
        self.like_id, self.like_params = None if like_id is None else int(like_id), tuple(like_params or ())
        if like_data is not None:   # (copies, cast as the bindings cast)
            like_data = dict(mu=np.array(like_data['mu'], np.float32).reshape(-1), R=np.array(like_data['R'], np.float32),
                             logl0=float(like_data['logl0']))
            like_data['mu'].setflags(write=False)
            like_data['R'].setflags(write=False)
        self.like_data = like_data
        if like_glm is not None:   # (copies, cast as the bindings cast)
            like_glm = dict(at=np.array(like_glm['at'], np.float32), y=np.array(like_glm['y'], np.float32).reshape(-1),
                            o=np.array(like_glm['o'], np.float32).reshape(-1), logl0=float(like_glm['logl0']), n=int(like_glm['n']),
                            family=like_glm['family'])
            for k in ('at', 'y', 'o'):
                like_glm[k].setflags(write=False)
        self.like_glm = like_glm
        if prior_gauss is not None:   # (copies, cast as the bindings cast)
            if like_glm is None:
                raise ValueError('DeviceTarget: prior_gauss needs a like_glm (the kernels take a GaussianPrior beside a GLMData only)')
            if lo is not None:
                raise ValueError('DeviceTarget: prior_gauss goes with no box (lo and hi None)')
            prior_gauss = dict(m=np.array(prior_gauss['m'], np.float32).reshape(-1), r=np.array(prior_gauss['r'], np.float32).reshape(-1),
                               logc=float(prior_gauss['logc']))
            for k in ('m', 'r'):
                prior_gauss[k].setflags(write=False)
        self.prior_gauss = prior_gauss
        self.t_std, self.t_mean, self.lo, self.hi = vec(t_std), vec(t_mean), vec(lo), vec(hi)
        for v in (self.t_std, self.t_mean, self.lo, self.hi):
            if v is not None:
                v.setflags(write=False)
        self._staged = {}

    def __setattr__(self, name, value):
        if name in _FIXED and name in self.__dict__:
            raise AttributeError('DeviceTarget.%s is fixed: with_transform() makes the target under another T' % name)
        object.__setattr__(self, name, value)

    def with_transform(self, t_std, t_mean):
        """the same likelihood and prior under T(x) = x * t_std + t_mean: neither depends on T, so nothing is checked again"""
        return DeviceTarget(self.like_id, self.like_params, t_std, t_mean, self.lo, self.hi, self.like_data, self.like_glm, self.prior_gauss)

    def launch_kwargs(self, device):
        """the keywords the flow bindings take (t_std, t_mean, lo, hi as float32 tensors on `device`, and like_params; with a
        like_data, and only then, `like_data` with mu and R as float32 tensors on `device`; with a like_glm, and only then,
        `like_glm` with at, y and o likewise; with a prior_gauss, and only then, `prior_gauss` with m and r likewise): staged on the first call for a device,
        the same tensors after it"""
        from . import flow
        key = str(device)
        if key not in self._staged:
            vecs = flow.target_vectors('DeviceTarget', device, self.t_std, self.t_mean, self.lo, self.hi)
            self._staged[key] = dict(zip(('t_std', 't_mean', 'lo', 'hi'), vecs), like_params=self.like_params)
            if self.like_data is not None:
                _, (mu, R) = flow.gdata_spec(self.like_data, device)
                self._staged[key]['like_data'] = dict(mu=mu, R=R, logl0=self.like_data['logl0'])
            if self.like_glm is not None:
                _, (at, y, o) = flow.glm_spec(self.like_glm, device)
                self._staged[key]['like_glm'] = dict(self.like_glm, at=at, y=y, o=o)
            if self.prior_gauss is not None:
                _, (m, r) = flow.gauss_prior_spec(self.prior_gauss, device)
                self._staged[key]['prior_gauss'] = dict(m=m, r=r, logc=self.prior_gauss['logc'])
        return dict(self._staged[key])

    def transform(self, x):
        """T(x) of a float32 tensor on its own device"""
        if self.t_std is None:
            return x
        kw = self.launch_kwargs(x.device)
        return affine_on_device(x, kw['t_std'], kw['t_mean'])
