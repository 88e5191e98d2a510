"""HipCholesky: the reference's 'choleksy' flow (SingleSpeedCholeksy, nnest/networks.py:162-239) -- one linear map
y = L x + b with L lower triangular -- on the nnest_chol_* entry points.  No fused proposal kernel: the sampler drives it
through the host protocol."""
import ctypes

import numpy as np
import torch

from . import _lib
from .flow import _HipFlow, train_epochs_host


class HipCholesky(_HipFlow):

    def __init__(self, num_inputs, device=None, seed=None):
        if not torch.cuda.is_available():
            raise _lib.NnestHipError('HipCholesky needs an MI355X visible to PyTorch-ROCm; there is no CPU fallback')
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.D = self.num_inputs = int(num_inputs)
        self._lib = _lib.load()
        L = self._lib
        self._bind('nnest_chol')
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(L.nnest_chol_create(self.D, ctypes.byref(self._h)))
        # the library's vectors are the packed ones as they are: the identity form of flow._PaddedVectors' names
        self.num_params = self._native_params = L.nnest_chol_num_params(self._h)
        self.prior = torch.distributions.MultivariateNormal(torch.zeros(self.D, device=self.device),
                                                            torch.eye(self.D, device=self.device))
        self.load_packed(self.default_init())

    def _to_native_dev(self, t):
        return t

    _from_native_dev = _to_native_dev

    def layer_shapes(self):
        D = self.D
        return [('flow.flows.0.bias', (D,)), ('flow.flows.0.lower_entries', (D * (D - 1) // 2,)), ('flow.flows.0.unconstrained_diag', (D,))]

    def default_init(self):
        """identity_init (networks.py:183-189): bias 0, lower 0, unconstrained_diag = log(e^{1 - eps} - 1) so that diag = 1"""
        D = self.D
        w = np.zeros(self.num_params, np.float32)
        w[-D:] = np.log(np.exp(1 - 1e-3) - 1)
        return w

    def load_packed(self, packed):
        packed = np.ascontiguousarray(packed, dtype=np.float32)
        if packed.size != self.num_params:
            raise ValueError('expected %d packed weights, got %d' % (self.num_params, packed.size))
        with torch.cuda.device(self.device):
            _lib.check(self._lib.nnest_chol_load_weights(self._h, packed.ctypes.data_as(ctypes.c_void_p), _lib.current_stream(self.device)))

    def store_packed(self):
        out = np.empty(self.num_params, np.float32)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.nnest_chol_store_weights(self._h, out.ctypes.data_as(ctypes.c_void_p), _lib.current_stream(self.device)))
        return out

    def state_dict(self):
        packed, sd, off = self.store_packed(), {}, 0
        for name, shape in self.layer_shapes():
            n = int(np.prod(shape))
            sd[name] = torch.from_numpy(packed[off:off + n].reshape(shape).copy())
            off += n
        return sd

    def load_state_dict(self, sd):
        self.load_packed(np.concatenate([np.asarray(sd[n].detach().cpu().numpy() if torch.is_tensor(sd[n]) else sd[n], dtype=np.float32).ravel()
                                         for n, _ in self.layer_shapes()]))

    # the fused kernels do not know this flow: the sampler falls back to the host protocol
    mh_steps = None
    inverse_loglike = None

    epoch_chunk = 1 << 30

    def _train_epoch(self, rows, epoch, n_train, batch, lr, weight_decay):
        step_losses = []
        for b0 in range(0, n_train, batch):
            loss, grad = self.loss_grad(rows(epoch, b0, b0 + batch).contiguous())
            self.adam_step(grad, lr, weight_decay)
            step_losses.append(loss)
        return torch.stack(step_losses).sum()

    def train_epochs(self, xtrain, xvalid, perm, noise=None, seed=0, jitter=0.0, batch=100, max_epochs=1, patience=50,
                     lr=1e-3, weight_decay=1e-6, epoch_offset=0, resume=False, finalize=True, result=None):
        """Trainer.train's epoch loop (trainer.py:198-241), host-driven (flow.train_epochs_host); arguments and return value as
        HipNVP.train_epochs"""
        assert not resume and epoch_offset == 0
        return train_epochs_host(self, self._train_epoch, xtrain, xvalid, perm, noise, seed, jitter, batch, max_epochs, patience, lr,
                                 weight_decay)
