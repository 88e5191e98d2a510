"""The books of the one host-driven epoch loop (nnest_amd.flow.train_epochs_host), on the CPU with a stand-in net: what
Trainer.train keeps per epoch (reference nnest/trainer.py:198-241) -- best validation loss and its epoch, the patience counter, the
early stop, the restore of the best weights -- and the `rows` helper the flows' epoch bodies gather their minibatches through."""
import numpy as np
import pytest
import torch

from nnest_amd.flow import train_epochs_host, chunked_epoch

VALID = [5.0, 4.0, 4.5, 3.0, 3.5, 3.6, 3.7, 1.0]   # validation loss of epochs 1..8
N_TRAIN, N_VALID, D, BATCH, CHUNK = 10, 4, 3, 4, 3


class StandIn(object):
    """one weight, +1 per Adam step; log_probs scripted so that epoch e validates at VALID[e] (the loop divides -mean by n_valid)"""
    device = torch.device('cpu')

    def __init__(self):
        self.w = np.zeros(1, np.float32)
        self.adam_steps = self.validations = 0
        self.chunks = []

    def store_packed(self):
        return self.w.copy()

    def load_packed(self, w):
        self.w = np.array(w, dtype=np.float32)

    def loss_grad(self, x):
        self.chunks.append(x.shape[0])
        return torch.ones(1), torch.zeros(1)

    def adam_step(self, grad, lr, weight_decay):
        self.w = self.w + 1
        self.adam_steps += 1

    def log_probs(self, x):
        v = VALID[self.validations]
        self.validations += 1
        return torch.full((x.shape[0],), -v * x.shape[0])


def run(max_epochs, patience, net=None, body=None, noise=None, jitter=0.0, seed=0):
    net = StandIn() if net is None else net
    g = torch.Generator().manual_seed(1)
    xtrain, xvalid = torch.randn(N_TRAIN, D, generator=g), torch.randn(N_VALID, D, generator=g)
    perm = torch.stack([torch.randperm(N_TRAIN, generator=g) for _ in range(max(max_epochs, 1))])[:max_epochs].to(torch.int32)
    res = train_epochs_host(net, chunked_epoch(net, CHUNK) if body is None else body, xtrain, xvalid, perm.reshape(-1), noise, seed,
                            jitter, BATCH, max_epochs, patience, 1e-3, 1e-6)
    return net, res, xtrain, perm


def test_books_as_the_reference_keeps_them():
    """trainer.py:198-241 by hand for VALID and patience 2: best at epochs 1, 2, 4; counter 1, 1, 2, 1, 2, 3 -> stop after epoch 6"""
    net, res, _, _ = run(max_epochs=8, patience=2)
    assert res['epochs_run'] == 6 and res['best_epoch'] == 4 and res['best_validation_loss'] == 3.0
    assert res['counter'] == 3 and res['stopped'] is True and res['result'] is None
    assert net.adam_steps == 18                      # three minibatches x six epochs
    assert net.w.tolist() == [12.0]                  # the weights of epoch 4 restored: three minibatches x four epochs
    assert net.chunks == [3, 1, 3, 1, 2] * 6         # minibatches of 4, 4, 2 rows in chunks of at most 3
    losses = res['losses'].numpy()
    assert losses.shape == (8, 2) and losses.dtype == np.float32
    assert np.array_equal(losses[:6, 1], np.float32(VALID[:6]))
    assert np.array_equal(losses[:6, 0], np.full(6, np.float32(3.0 / N_TRAIN)))   # each minibatch's loss is 1: the sum / n_train
    assert np.array_equal(losses[6:], np.zeros((2, 2), np.float32))
    assert res['last_train_loss'] == float(np.float32(3.0 / N_TRAIN))


def test_patience_never_reached():
    net, res, _, _ = run(max_epochs=8, patience=50)
    assert res['stopped'] is False and res['epochs_run'] == 8
    assert res['best_epoch'] == 8 and res['best_validation_loss'] == 1.0 and res['counter'] == 1
    assert net.adam_steps == 24 and net.w.tolist() == [24.0]   # the last epoch is the best one: restored all the same
    net, res, _, _ = run(max_epochs=7, patience=50)            # ... and where it is not the last: epoch 4 of 7
    assert res['stopped'] is False and res['epochs_run'] == 7 and res['best_epoch'] == 4 and res['counter'] == 4
    assert net.adam_steps == 21 and net.w.tolist() == [12.0]


def test_no_epochs():
    net, res, _, _ = run(max_epochs=0, patience=2)
    assert res['epochs_run'] == 0 and res['best_epoch'] == 0 and res['best_validation_loss'] == float('inf')
    assert res['counter'] == 0 and res['stopped'] is False and res['last_train_loss'] == 0.0
    assert net.adam_steps == 0 and net.validations == 0 and net.w.tolist() == [0.0]
    assert np.array_equal(res['losses'].numpy(), np.zeros((1, 2), np.float32))


def test_restore_hands_back_P_where_the_flow_has_one():
    class WithP(StandIn):
        P = 'the permutations'

        def load_packed(self, w, P):
            self.loaded_P = P
            StandIn.load_packed(self, w)

    net, _, _, _ = run(max_epochs=8, patience=2, net=WithP())
    assert net.loaded_P == 'the permutations' and net.w.tolist() == [12.0]


def test_validation_rule_can_be_replaced():
    """the MAF's hook: what valid_sum returns is divided by n_valid and takes the place of -mean(log_probs)"""
    net = StandIn()
    g = torch.Generator().manual_seed(1)
    seen = []

    def valid_sum(xvalid):
        seen.append(tuple(xvalid.shape))
        return torch.tensor(2.0 * N_VALID * VALID[len(seen) - 1])

    res = train_epochs_host(net, chunked_epoch(net, CHUNK), torch.randn(N_TRAIN, D, generator=g), torch.randn(N_VALID, D, generator=g),
                            torch.arange(N_TRAIN).repeat(8), None, 0, 0.0, BATCH, 8, 2, 1e-3, 1e-6, valid_sum=valid_sum)
    assert seen == [(N_VALID, D)] * 6 and net.validations == 0
    assert res['best_validation_loss'] == 6.0 and res['best_epoch'] == 4 and res['epochs_run'] == 6


class Recorder(object):
    """an epoch body that keeps what `rows` hands it: the whole epoch at once (per_minibatch False) or minibatch by minibatch"""

    def __init__(self, per_minibatch):
        self.per_minibatch, self.epochs = per_minibatch, []

    def __call__(self, rows, epoch, n_train, batch, lr, weight_decay):
        if self.per_minibatch:
            got = torch.cat([rows(epoch, lo, lo + batch) for lo in range(0, n_train, batch)])
        else:
            got = rows(epoch, 0, n_train)
        self.epochs.append(got.clone())
        return 0.0                                   # (a float sum, as the fast/slow body returns)


@pytest.mark.parametrize('recorded', [True, False])
def test_rows_per_epoch_and_per_minibatch(recorded):
    """rows(e, 0, n) and the per-minibatch rows(e, lo, hi) gather the same rows in loader order, the last minibatch ragged; recorded
    noise adds the same jitter to both.  Without recorded noise nothing is added at jitter 0, and at jitter > 0 the draws come from one
    generator seeded from `seed` in the order asked for (the per-epoch draw is checked against that generator)."""
    E, jitter = 3, 0.25
    noise = torch.randn(E, N_TRAIN, D, generator=torch.Generator().manual_seed(2)) if recorded else None
    whole, parts = Recorder(False), Recorder(True)
    _, _, xtrain, perm = run(E, 50, body=whole, noise=noise, jitter=jitter if recorded else 0.0)
    run(E, 50, body=parts, noise=noise, jitter=jitter if recorded else 0.0)
    assert len(whole.epochs) == len(parts.epochs) == E
    for e in range(E):
        want = xtrain[perm[e].long()]
        if recorded:
            want = want + jitter * noise[e]
        assert whole.epochs[e].shape == (N_TRAIN, D)
        assert torch.equal(whole.epochs[e], want) and torch.equal(parts.epochs[e], want)
    if not recorded:
        drawn = Recorder(False)
        run(E, 50, body=drawn, noise=None, jitter=jitter, seed=(1 << 63) + 7)
        gen = torch.Generator().manual_seed(7)       # seed & 0x7FFF...
        for e in range(E):
            assert torch.equal(drawn.epochs[e], xtrain[perm[e].long()] + jitter * torch.randn(N_TRAIN, D, generator=gen))
