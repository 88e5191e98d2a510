"""HipMAF: a masked autoregressive flow resident on one MI355X, driven through the C ABI (nnest_maf_create; every other call
is the nnest_nvp_* entry point of the same name -- the handle is an nnest_nvp_t).

ABSENT FROM THE REFERENCE: nnest/trainer.py:83-100 builds 'choleksy', 'nvp' or 'spline' only.  BASELINE.json's north star and
its config 5 name a MAF, so this build defines one (nnest_amd/csrc/maf_tile.h) behind the reference's flow protocol
(nnest/networks.py:17-84: forward, inverse, log_probs, sample) and its Trainer seam (`Trainer(flow='maf')`):
B blocks of two MADE-masked nets with the shapes of the reference's coupling nets, order reversed between blocks; forward
(density / training) is one pass, inverse (sampling, MCMC proposals) runs group by group.  Parity is against a CPU
restatement of the same definition (tests/) and against self-consistency (round trip, log-det), as the reference tests its own flows
(tests/test_flows.py:27-30)."""
import ctypes

import torch

from . import _lib
from .flow import HipNVP, train_epochs_host


class HipMAF(HipNVP):
    """num_inputs=D, num_hidden=H (16), num_blocks=B, num_layers=L.  The state_dict has the keys and shapes of SingleSpeedNVP
    (scale_net / translate_net per block); masked entries are kept (they are zero in effect and take only Adam's weight-decay
    steps, like the entries RealNVP's mask never reaches)."""

    epoch_chunk = 1 << 30   # Trainer.train hands the whole run to train_epochs (flow.train_epochs_host keeps the early-stopping books)
    ensemble_fused_by_default = False   # (no fused ensemble kernel: `ensemble` is not bound below)

    def __init__(self, num_inputs, num_hidden=16, num_blocks=3, num_layers=1, device=None, seed=None):
        if not torch.cuda.is_available():
            raise _lib.NnestHipError('HipMAF needs an MI355X visible to PyTorch-ROCm (torch.cuda.is_available() is False); '
                                     'there is no CPU fallback')
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.D, self.H, self.B, self.L = int(num_inputs), int(num_hidden), int(num_blocks), int(num_layers)
        self.num_inputs = self.D
        self.scale = ''
        self._lib = _lib.load()
        L = self._lib
        self._bind('nnest_nvp', mh='nnest_mh_constrained_steps')   # the handle is an nnest_nvp_t: HipNVP's entry points (no `slice`:
        # there is no fused slice kernel for the MAF, the slice proposal runs through nnest_amd.slice_rounds)
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(L.nnest_maf_create(self.D, self.H, self.B, self.L, ctypes.byref(self._h)))
        self.num_params = L.nnest_nvp_num_params(self._h)
        self._set_pad_index(None, self.num_params)
        self.num_groups = L.nnest_maf_num_groups(self._h)   # passes of the nets per block in the sampling direction
        self.prior = torch.distributions.MultivariateNormal(torch.zeros(self.D, device=self.device),
                                                            torch.eye(self.D, device=self.device))
        self.load_packed(self.default_init(seed))

    def _train_epoch(self, rows, epoch, n_train, batch, lr, weight_decay):
        """the epoch's rows in minibatch order, jitter applied: one gather and one draw per epoch, and every minibatch of the epoch
        queued by one library call (nothing read back; a minibatch is a slice)"""
        rows_all = rows(epoch, 0, n_train).contiguous()
        tot = torch.zeros((), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.nnest_maf_train_epoch(self._h, _lib.ptr(rows_all), n_train, batch, ctypes.c_float(lr),
                                                       ctypes.c_float(weight_decay), _lib.ptr(tot), _lib.current_stream(self.device)))
        return tot

    def train_epochs(self, xtrain, xvalid, perm, noise=None, seed=0, jitter=0.0, batch=100, max_epochs=1, patience=50,
                     lr=1e-3, weight_decay=1e-6, epoch_offset=0, resume=False, finalize=True, result=None, one_cu=False):
        """Trainer.train's epoch loop (trainer.py:198-241) driven from the host (flow.train_epochs_host): per minibatch one gradient
        (nnest_nvp_loss_grad: two launches) and one Adam step + image rebuild, an epoch's minibatches queued by one call
        (nnest_maf_train_epoch); arguments and return value as HipNVP.train_epochs"""
        assert not resume and epoch_offset == 0

        def valid_sum(xvalid):
            # the validation set in pieces of `batch` rows: the SUM of each piece's mean (then / n_valid, as Trainer._validate divides,
            # trainer.py:405-418).  The reference and the other flows validate in ONE batch (valid_loader's batch_size is
            # X_valid.shape[0], trainer.py:190), i.e. one mean over the whole set: this differs from it by the number of pieces, and
            # in detail when the last one is ragged.  Kept as it is (the reported validation losses depend on it).
            return torch.stack([-c.mean() for c in self.log_probs(xvalid).split(int(batch))]).sum()

        return train_epochs_host(self, self._train_epoch, xtrain, xvalid, perm, noise, seed, jitter, batch, max_epochs, patience, lr,
                                 weight_decay, valid_sum=valid_sum)
