"""ORACLE -- TEST INFRASTRUCTURE ONLY (nnest_amd/ never imports it).

A differentiable float64 restatement of the RealNVP coupling stack, SingleSpeedNVP, and of the fast/slow hierarchy built on it
(FastSlowNVP / FastSlowSpline).  It follows oracle/nnest_oracle_impl.h step by step (the C oracle, pinned to the reference's passes
by tests/test_oracle_golden.py) but is written in torch on the CPU, so autograd gives the gradient of ANY scalar of the flow's
outputs with respect to the weights AND the inputs: the yardstick for nnest_nvp_vjp, whose contract (include/nnest_hip.h) is

    L = <gz, z(X)> + gld * sum_rows logdet(X)   ->   dL/dw (packed order), dL/dx [M, D]

Block b conditions on the dimensions with (d + b) odd; the scale net is tanh, the translate net relu, L hidden layers each;
scale='translate' drops the scale nets, scale='constant' follows every translate-only coupling with a ScaleLayer, y = x e^s, that
adds s (the scalar itself, not D s) to the log-determinant, as the reference and the C oracle do.

Weights are the float32 packed vector of the C ABI (scale-net slots kept in every mode, ScaleLayer scalars appended), upcast to
`dtype`: torch.float64 is the oracle; torch.float32 is the same definition in float32, the stand-in for a kernel on the CPU and the
measure of what float32 can reach on an input.  tests/test_nvp_vjp_check.py pins this module to the C oracle and to the reference's
autograd gradients in tests/golden/.
"""
import numpy as np
import torch

from oracle import spline_grad

COUPLING_HIDDEN = 64        # the fast/slow hierarchy's last coupling: hidden 64, one hidden layer (networks.py:112-120)


def net_size(D, H, L):
    return H * D + H + L * (H * H + H) + D * H + D


def num_params(D, H, B, L, scale=''):
    return 2 * B * net_size(D, H, L) + (B if scale == 'constant' else 0)


def _mlp(w, off, D, H, L, act, m):
    """Linear(D, H) act [Linear(H, H) act] x L Linear(H, D) from the packed vector at `off`"""
    dims = [(H, D)] + [(H, H)] * L + [(D, H)]
    h = m
    for i, (o, k) in enumerate(dims):
        W = w[off:off + o * k].reshape(o, k)
        off += o * k
        b = w[off:off + o]
        off += o
        h = h @ W.T + b
        if i < len(dims) - 1:
            h = act(h)
    return h


def _coupling(w, off, D, H, L, mask, z, scale_net=True):
    """CouplingLayer.forward (networks.py:289-298): scale net at `off`, translate net one net further; mask 1 = conditioning side"""
    m = z * mask
    t = _mlp(w, off + net_size(D, H, L), D, H, L, torch.relu, m) * (1 - mask)
    if not scale_net:
        return z + t, torch.zeros(z.shape[0], dtype=z.dtype)
    ls = _mlp(w, off, D, H, L, torch.tanh, m) * (1 - mask)
    return z * torch.exp(ls) + t, ls.sum(dim=1)


def forward(w, X, D, H, B, L, scale=''):
    """NormalizingFlow.forward on rows X [N, D] (tensors of one dtype; w the packed vector) -> z [N, D], logdet [N]"""
    assert w.numel() == num_params(D, H, B, L, scale), (w.numel(), num_params(D, H, B, L, scale))
    ns = net_size(D, H, L)
    z, ld = X, torch.zeros(X.shape[0], dtype=X.dtype)
    d = torch.arange(D)
    for b in range(B):
        mask = (((d + b) % 2) == 1).to(X.dtype)
        z, l = _coupling(w, 2 * b * ns, D, H, L, mask, z, scale_net=scale == '')
        ld = ld + l
        if scale == 'constant':
            s = w[2 * B * ns + b]
            z = z * torch.exp(s)
            ld = ld + s
    return z, ld


_w = spline_grad._w64          # float32 packed vector -> tensor of dtype (the float32 values, exactly)
_x = spline_grad._x64
base_logp = spline_grad.base_logp


def _np64(t):
    return t.detach().to(torch.float64).numpy()


def passes(w_packed, X, D, H, B, L, scale='', dtype=torch.float64):
    """(z, logdet) as float64 numpy arrays"""
    with torch.no_grad():
        z, ld = forward(_w(w_packed, False, dtype), _x(X, dtype), D, H, B, L, scale)
    return _np64(z), _np64(ld)


def log_probs(w_packed, X, D, H, B, L, scale='', base_beta=0.0, dtype=torch.float64):
    """NormalizingFlowModel.log_probs [N]"""
    with torch.no_grad():
        z, ld = forward(_w(w_packed, False, dtype), _x(X, dtype), D, H, B, L, scale)
        return _np64(base_logp(z, base_beta) + ld)


def vjp(w_packed, X, gz, gld, D, H, B, L, scale='', dtype=torch.float64):
    """(dL/dw [n], dL/dx [M, D]) for L = <gz, z(X)> + gld * sum_rows logdet(X): the contract of nnest_nvp_vjp.  The base
    distribution does not enter."""
    w = _w(w_packed, True, dtype)
    x = _x(X, dtype).requires_grad_(True)
    z, ld = forward(w, x, D, H, B, L, scale)
    gz = torch.as_tensor(np.asarray(gz, np.float64)).to(dtype)
    (((z * gz).sum()) + float(gld) * ld.sum()).backward()
    return _np64(w.grad), _np64(x.grad)


def base_denergy(z, base_beta=0.0):
    """dE/dz of E = -log p(z): z for N(0, I), beta |z|^(beta - 1) sign(z) for the generalised normal"""
    if base_beta == 0.0:
        return z
    return base_beta * np.abs(z) ** (base_beta - 1.0) * np.sign(z)


def loss_grad(w_packed, X, D, H, B, L, scale='', base_beta=0.0, dtype=torch.float64):
    """(loss = -mean(log_probs(X)), dloss/dw): vjp's special case gz = dE/dz / M, gld = -1 / M"""
    M = np.atleast_2d(X).shape[0]
    with torch.no_grad():
        z, ld = forward(_w(w_packed, False, dtype), _x(X, dtype), D, H, B, L, scale)
        loss = float(-(base_logp(z, base_beta) + ld).mean())
    gz = base_denergy(_np64(z), base_beta) / M
    return loss, vjp(w_packed, X, gz, -1.0 / M, D, H, B, L, scale, dtype)[0]


# ---- the fast/slow hierarchy (networks.py:86-150, :350-380, :718-731) ---------------------------------------------------------------
class FastSlow(object):
    """slow stage on x[:, :S], fast stage on x[:, S:], then one hidden-64, one-hidden-layer coupling whose mask is the slow block
    (slow conditions fast).  kind='nvp': both stages RealNVP(H, B, L); kind='spline': neural-spline stages (oracle/spline_grad.py),
    the fast one always with hidden width 16 (networks.py:722), P = {'fast': .., 'slow': ..} their permutations.  Parameters in the
    reference's state_dict order (fast_flow, slow_flow, flow), the order of HipFastSlowNVP.store_packed()."""

    def __init__(self, S, F, H=16, B=3, L=1, kind='nvp', P=None, K=8, tail=3.0):
        self.S, self.F, self.D, self.H, self.B, self.L = int(S), int(F), int(S) + int(F), int(H), int(B), int(L)
        self.kind, self.P, self.K, self.tail = kind, P, int(K), float(tail)
        if kind == 'nvp':
            self.n_fast, self.n_slow = num_params(self.F, H, B, L), num_params(self.S, H, B, L)
        else:
            self.n_fast, self.n_slow = spline_grad.num_params(self.F, 16, B, self.K), spline_grad.num_params(self.S, H, B, self.K)
        self.n_coupling = 2 * net_size(self.D, COUPLING_HIDDEN, 1)
        self.n = self.n_fast + self.n_slow + self.n_coupling

    def layer_shapes(self):
        """[(name, shape, offset)] of the concatenated state_dict"""
        out, off = [], 0
        if self.kind == 'nvp':
            fast, slow = _nvp_shapes(self.F, self.H, self.B, self.L), _nvp_shapes(self.S, self.H, self.B, self.L)
        else:
            fast = spline_grad.layer_shapes(self.F, 16, self.B, self.K)
            slow = spline_grad.layer_shapes(self.S, self.H, self.B, self.K)
        named = [(n.replace('flow.flows', 'fast_flow.flows', 1), s) for n, s in fast]
        named += [(n.replace('flow.flows', 'slow_flow.flows', 1), s) for n, s in slow]
        named += _nvp_shapes(self.D, COUPLING_HIDDEN, 1, 1)
        for n, s in named:
            out.append((n, s, off))
            off += int(np.prod(s))
        assert off == self.n
        return out

    def _stage(self, w, x, which):
        D = self.F if which == 'fast' else self.S
        if self.kind == 'nvp':
            return forward(w, x, D, self.H, self.B, self.L)
        return spline_grad.forward(w, self.P[which], x, D, 16 if which == 'fast' else self.H, self.B, self.K, self.tail)

    def stages(self, w, X):
        """(z [N, D], (logdet of the slow stage, of the fast stage, of the coupling))"""
        S = self.S
        zs, lds = self._stage(w[self.n_fast:self.n_fast + self.n_slow], X[:, :S], 'slow')
        zf, ldf = self._stage(w[:self.n_fast], X[:, S:], 'fast')
        mask = torch.cat([torch.ones(S), torch.zeros(self.F)]).to(X.dtype)
        z, ldc = _coupling(w, self.n_fast + self.n_slow, self.D, COUPLING_HIDDEN, 1, mask, torch.cat([zs, zf], dim=1))
        return z, (lds, ldf, ldc)

    def forward(self, w, X):
        z, lds = self.stages(w, X)
        return z, lds[0] + lds[1] + lds[2]

    def log_probs(self, w_packed, X, dtype=torch.float64, parts=False):
        """log_probs [N] (N(0, I) base); parts=True: also the three stages' log-determinants"""
        with torch.no_grad():
            z, lds = self.stages(_w(w_packed, False, dtype), _x(X, dtype))
            lp = base_logp(z) + lds[0] + lds[1] + lds[2]
        return (_np64(lp), [_np64(l) for l in lds]) if parts else _np64(lp)

    def loss_grad(self, w_packed, X, dtype=torch.float64):
        """(the training loss -mean(log_probs(X)), its gradient in store_packed() order) by autograd"""
        w = _w(w_packed, True, dtype)
        z, ld = self.forward(w, _x(X, dtype))
        loss = -(base_logp(z) + ld).mean()
        loss.backward()
        return float(loss.detach()), _np64(w.grad)


def _nvp_shapes(D, H, B, L):
    """[(name, shape)] of SingleSpeedNVP(scale='') in state_dict order"""
    out = []
    for b in range(B):
        for net in ('scale_net', 'translate_net'):
            for i, (o, k) in enumerate([(H, D)] + [(H, H)] * L + [(D, H)]):
                out += [('flow.flows.%d.%s.%d.weight' % (b, net, 2 * i), (o, k)), ('flow.flows.%d.%s.%d.bias' % (b, net, 2 * i), (o,))]
    return out
