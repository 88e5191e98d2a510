"""ORACLE -- TEST INFRASTRUCTURE ONLY (nnest_amd/ never imports it).

A differentiable float64 restatement of the neural-spline flow, SingleSpeedSpline: per block ActNorm -> LU-parametrised 1x1
convolution (Kingma & Dhariwal 2018) -> NSF_CL, two rational-quadratic spline couplings (Durkan et al. 2019) over the
contiguous halves of the vector.  It follows oracle/spline_oracle_impl.h step by step (the C oracle, pinned to the reference's
passes by tests/test_oracle_golden.py) but is written in torch float64 on the CPU, so autograd gives the float64 gradient of the
training loss at any shape: the yardstick for the hand-written backward passes of nnest_spline_rows.hip / nnest_spline_train.hip.

Weights are the float32 packed vector in state_dict order (layer_shapes below, = HipSpline.layer_shapes()), upcast to float64;
P [B, D, D] are the fixed permutations of the 1x1 convolutions.  tests/test_oracle_spline_grad.py pins this module to the C
oracle's float64 log_probs and to the reference's autograd gradients in tests/golden/spline_*.npz.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

MIN_BIN = 1e-3
MIN_DERIV = 1e-3
LOG_2PI_HALF = 0.91893853320467274178


def nlower(D):
    return D // 2 + (D & 1)


def layer_shapes(D, H, B, K):
    """[(name, shape)] in the reference's state_dict order (HipSpline.layer_shapes)"""
    out, nl, nu, Pn = [], nlower(D), D // 2, 3 * K - 1
    for b in range(B):
        out += [('flow.flows.%d.s' % (3 * b), (1, D)), ('flow.flows.%d.t' % (3 * b), (1, D)),
                ('flow.flows.%d.L' % (3 * b + 1), (D, D)), ('flow.flows.%d.S' % (3 * b + 1), (D,)),
                ('flow.flows.%d.U' % (3 * b + 1), (D, D))]
        for f, nin, nout in (('f1', nl, Pn * nu), ('f2', nu, Pn * nl)):
            for i, sh in enumerate(((H, nin), (H, H), (H, H), (nout, H))):
                out.append(('flow.flows.%d.%s.net.%d.weight' % (3 * b + 2, f, 2 * i), sh))
                out.append(('flow.flows.%d.%s.net.%d.bias' % (3 * b + 2, f, 2 * i), (sh[0],)))
    return out


def num_params(D, H, B, K):
    return sum(int(np.prod(sh)) for _, sh in layer_shapes(D, H, B, K))


def unpack(w, D, H, B, K):
    """packed vector (any dtype; a float64 tensor keeps its graph) -> {name: float64 tensor view}"""
    w = w if torch.is_tensor(w) else torch.from_numpy(np.asarray(w, dtype=np.float64))
    out, off = {}, 0
    for name, sh in layer_shapes(D, H, B, K):
        n = int(np.prod(sh))
        out[name] = w[off:off + n].reshape(sh)
        off += n
    assert off == w.numel(), (off, w.numel())
    return out


def _mlp(p, prefix, x):
    """Linear LReLU(.2) Linear LReLU Linear LReLU Linear"""
    for i in range(4):
        x = x @ p['%s.net.%d.weight' % (prefix, 2 * i)].T + p['%s.net.%d.bias' % (prefix, 2 * i)]
        if i < 3:
            x = F.leaky_relu(x, 0.2)
    return x


def _knots(raw, tail):
    """bin edges [.., K+1] and widths [.., K] from raw logits [.., K]: softmax, min-bin mixing, cumsum onto [-tail, tail]"""
    K = raw.shape[-1]
    p = MIN_BIN + (1 - MIN_BIN * K) * torch.softmax(raw, dim=-1)
    c = F.pad(torch.cumsum(p, dim=-1), (1, 0))
    c = 2 * tail * c - tail
    c = torch.cat([torch.full_like(c[..., :1], -tail), c[..., 1:-1], torch.full_like(c[..., :1], tail)], dim=-1)
    return c, c[..., 1:] - c[..., :-1]


def rqs(raw, x, K, tail):
    """NSF_CL's conditioner output [.., 3K-1] -> the forward rational-quadratic spline of x [..]: (y, log|dy/dx|, distance of x
    to the nearest knot of the searched edges, +inf outside [-tail, tail])"""
    inside = (x >= -tail) & (x <= tail)
    xi = torch.where(inside, x, torch.zeros_like(x))                  # keeps the untaken branch finite
    uw = 2 * tail * torch.softmax(raw[..., :K], dim=-1)               # softmax, scaled by 2 tail (NSF_CL) ...
    uh = 2 * tail * torch.softmax(raw[..., K:2 * K], dim=-1)
    const = math.log(math.exp(1 - MIN_DERIV) - 1)                     # end-knot derivatives 1
    ud = F.pad(F.softplus(raw[..., 2 * K:]), (1, 1), value=const)     # softplus (NSF_CL) ...
    cw, wd = _knots(uw, tail)                                         # ... and softmax again (RQS)
    ch, ht = _knots(uh, tail)
    dv = MIN_DERIV + F.softplus(ud)                                   # ... and softplus again
    edges = cw.detach().clone()
    edges[..., -1] += 1e-6
    bin_ = ((xi.detach()[..., None] >= edges).sum(dim=-1) - 1).clamp(0, K - 1)[..., None]
    margin = (xi.detach()[..., None] - cw.detach()).abs().min(dim=-1).values
    margin = torch.where(inside, margin, torch.full_like(margin, math.inf))
    g = lambda a: torch.gather(a, -1, bin_)[..., 0]                  # noqa: E731
    icw, ibw, ich, ih = g(cw), g(wd), g(ch), g(ht)
    d0, d1 = g(dv), torch.gather(dv, -1, bin_ + 1)[..., 0]
    delta = ih / ibw
    theta = (xi - icw) / ibw
    tomt = theta * (1 - theta)
    den = delta + (d0 + d1 - 2 * delta) * tomt
    y = ich + ih * (delta * theta * theta + d0 * tomt) / den
    num = delta * delta * (d1 * theta * theta + 2 * delta * tomt + d0 * (1 - theta) * (1 - theta))
    ld = torch.log(num) - 2 * torch.log(den)
    return torch.where(inside, y, x), torch.where(inside, ld, torch.zeros_like(ld)), margin


def forward(w, P, X, D, H, B, K, tail, margins=False, stats=None):
    """NormalizingFlow.forward on rows X [N, D] (float64 tensors; w a packed float64 tensor) -> z [N, D], logdet [N]
    (and, with margins=True, each row's smallest distance of a spline input to a knot of its bin search).  A dict `stats`
    receives the largest conditioner output ('max_logit') and the number of spline inputs outside [-tail, tail] ('n_tail')."""
    p = unpack(w, D, H, B, K)
    dt = w.dtype
    P = torch.as_tensor(np.asarray(P, dtype=np.float64)).reshape(B, D, D).to(dt)
    nl = nlower(D)
    z, ld = X, torch.zeros(X.shape[0], dtype=dt)
    marg = torch.full((X.shape[0],), math.inf, dtype=dt)
    eye = torch.eye(D, dtype=dt)
    for b in range(B):
        s, t = p['flow.flows.%d.s' % (3 * b)], p['flow.flows.%d.t' % (3 * b)]
        z = z * torch.exp(s) + t                                       # ActNorm
        ld = ld + s.sum()
        c = 'flow.flows.%d.' % (3 * b + 1)
        L, S, U = p[c + 'L'], p[c + 'S'], p[c + 'U']
        W = P[b] @ (torch.tril(L, -1) + eye) @ (torch.triu(U, 1) + torch.diag(S))
        z = z @ W                                                      # 1x1 convolution
        ld = ld + torch.log(torch.abs(S)).sum()
        n = 'flow.flows.%d.' % (3 * b + 2)
        lower, upper = z[:, :nl], z[:, nl:]
        for prefix, cond, tgt in (('f1', 'lower', 'upper'), ('f2', 'upper', 'lower')):
            xc = lower if cond == 'lower' else upper
            xt = upper if tgt == 'upper' else lower
            raw = _mlp(p, n + prefix, xc).reshape(X.shape[0], xt.shape[1], 3 * K - 1)
            y, l, m = rqs(raw, xt, K, tail)
            if stats is not None:
                stats['max_logit'] = max(stats.get('max_logit', -math.inf), float(raw.detach().max())) if raw.numel() else \
                    stats.get('max_logit', -math.inf)
                stats['n_tail'] = stats.get('n_tail', 0) + int((xt.detach().abs() > tail).sum())
            ld = ld + l.sum(dim=1)
            if m.shape[1]:
                marg = torch.minimum(marg, m.min(dim=1).values)
            if tgt == 'upper':
                upper = y
            else:
                lower = y
        z = torch.cat([lower, upper], dim=1)
    return (z, ld, marg) if margins else (z, ld)


def base_logp(z, base_beta=0.0):
    """N(0, I), or GeneralisedNormal(0, 1, beta) for base_beta > 0"""
    if base_beta == 0.0:
        return -0.5 * (z * z).sum(dim=1) - z.shape[1] * LOG_2PI_HALF
    cst = math.log(base_beta) - math.log(2.0) - math.lgamma(1.0 / base_beta)
    return (-torch.abs(z) ** base_beta + cst).sum(dim=1)


def _w64(w_packed, requires_grad=False, dtype=torch.float64):
    w = torch.tensor(np.asarray(w_packed, dtype=np.float32)).to(dtype)
    return w.requires_grad_(requires_grad)


def _x64(X, dtype=torch.float64):
    return torch.tensor(np.atleast_2d(np.asarray(X))).to(dtype)


def log_probs(w_packed, P, X, D, H, B, K=8, tail=3.0, base_beta=0.0, margins=False, stats=None):
    """NormalizingFlowModel.log_probs -> (log_probs [N] numpy float64, loss = -mean); margins=True appends each row's smallest
    distance to a knot"""
    with torch.no_grad():
        z, ld, m = forward(_w64(w_packed), P, _x64(X), D, H, B, K, tail, margins=True, stats=stats)
        lp = base_logp(z, base_beta) + ld
    out = (lp.numpy(), float(-lp.mean()))
    return out + (m.numpy(),) if margins else out


def loss_grad(w_packed, P, X, D, H, B, K=8, tail=3.0, base_beta=0.0, dtype=torch.float64):
    """(loss = -mean(log_probs(X)), dloss/dw in packed order) by autograd in float64 (dtype=torch.float32: the same definition
    evaluated in float32, as the reference evaluates it -- a yardstick for the float32 conditioning of a case)"""
    w = _w64(w_packed, True, dtype)
    z, ld = forward(w, P, _x64(X, dtype), D, H, B, K, tail)
    loss = -(base_logp(z, base_beta) + ld).mean()
    loss.backward()
    return float(loss.detach()), w.grad.numpy().astype(np.float64)


def vjp(w_packed, P, X, D, H, B, K, tail, gz, gld):
    """(dL/dw, dL/dx) for L = <gz, z(x)> + gld * sum_rows logdet(x): the contract of nnest_spline_vjp"""
    w = _w64(w_packed, True)
    x = _x64(X).requires_grad_(True)
    z, ld = forward(w, P, x, D, H, B, K, tail)
    L = (z * torch.as_tensor(np.asarray(gz, dtype=np.float64))).sum() + float(gld) * ld.sum()
    L.backward()
    return w.grad.numpy(), x.grad.numpy()


def adam(ws, grads, lr, wd, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam with coupled weight decay, in float64: the weights after len(grads) steps from zero moments, where
    grads[i] was taken at ws[i] (the weights before step i + 1; a single vector stands for ws[0] when there is one step).
    Step i + 1 starts from ws[i], so the prediction of the last step uses the caller's own weights before it."""
    ws = [np.asarray(ws, np.float64)] if np.ndim(ws) == 1 else [np.asarray(w, np.float64) for w in ws]
    assert len(ws) == len(grads), (len(ws), len(grads))
    b1, b2 = betas
    m = v = 0.0
    for i, (w, g) in enumerate(zip(ws, grads)):
        gi = np.asarray(g, np.float64) + wd * w
        m = b1 * m + (1 - b1) * gi
        v = b2 * v + (1 - b2) * gi * gi
        t = i + 1
        out = w - (lr / (1 - b1 ** t)) * m / (np.sqrt(v) / math.sqrt(1 - b2 ** t) + eps)
    return out
