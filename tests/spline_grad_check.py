"""Per-tensor comparison of a spline-flow gradient (packed, state_dict order) against its float64 oracle
(oracle/spline_grad.py), shared by tests/test_oracle_spline_grad.py (CPU) and tests/test_gpu_spline_grad.py (GPU).

For every state_dict tensor t:   max|g - g64|_t  <=  rtol_t * max|g64|_t  +  atol_floor * max|g64|_all.
A criterion over the whole vector (max|g - g64| <= tol * max|g64|_all) lets a tensor whose gradients are 100x smaller than the
largest be wrong by 100 % of its own scale; this one scales the bound to each tensor and keeps only a small floor for tensors
whose gradient is rounding noise of the others."""
import numpy as np


def per_tensor_ratios(g, g64, shapes, rtol_t, atol_floor, slack=None):
    """[(error / bound, name, index of the worst element within the tensor, g, g64)] for every tensor, in packed order.
    slack: optional {name: extra absolute allowance} (the float32 conditioning of an ill-conditioned case)"""
    g = np.asarray(g, np.float64).ravel()
    g64 = np.asarray(g64, np.float64).ravel()
    assert g.shape == g64.shape, (g.shape, g64.shape)
    floor = atol_floor * np.max(np.abs(g64))
    out, off = [], 0
    for name, sh in shapes:
        n = int(np.prod(sh))
        a, b = g[off:off + n], g64[off:off + n]
        err = np.abs(a - b)
        err[~np.isfinite(err)] = np.inf
        k = int(np.argmax(err))
        bound = rtol_t * np.max(np.abs(b)) + floor + (slack or {}).get(name, 0.0)
        out.append((float(err[k] / bound) if bound > 0 else (0.0 if err[k] == 0 else np.inf), name, k, float(a[k]), float(b[k])))
        off += n
    assert off == g.size, (off, g.size)
    return out


def float32_slack(g32, g64, shapes, factor):
    """{name: factor * max|g32 - g64|_t}: the error of the same definition evaluated in float32, scaled"""
    d = np.abs(np.asarray(g32, np.float64) - np.asarray(g64, np.float64))
    return {name: factor * float(np.max(d[s])) for name, s in tensor_slices(shapes).items()}


def assert_grad_close(g, g64, shapes, rtol_t, atol_floor, what='', slack=None):
    """raises AssertionError naming the first tensor (and its worst element) outside its bound; returns the worst ratio"""
    rows = per_tensor_ratios(g, g64, shapes, rtol_t, atol_floor, slack)
    for ratio, name, k, a, b in rows:
        assert ratio <= 1.0, '%s%s[%d]: %.9g vs float64 %.9g (error / bound %.3g; rtol_t %g, atol_floor %g)' % (
            what + ': ' if what else '', name, k, a, b, ratio, rtol_t, atol_floor)
    return max(r[0] for r in rows)


def whole_vector_ok(g, g64, tol=2e-4):
    """the criterion of test_loss_and_gradient_vs_reference_autograd: max|g - g64| < tol * (1e-3 + max|g64|)"""
    g, g64 = np.asarray(g, np.float64), np.asarray(g64, np.float64)
    return bool(np.max(np.abs(g - g64)) < tol * (1e-3 + np.max(np.abs(g64))))


def tensor_slices(shapes):
    """{name: slice into the packed vector}"""
    out, off = {}, 0
    for name, sh in shapes:
        n = int(np.prod(sh))
        out[name] = slice(off, off + n)
        off += n
    return out


# ---- the shapes the spline-training kernels are held to ------------------------------------------------------------------------
# One row per case: (D, H, B, M) and the instantiation it reaches, derived from the dispatch code:
#   rows form (nnest_spline_rows.hip): eligible for native hidden 16 (H <= 16), 2 <= D <= 64, M <= 128, B <= 4
#     (spline_rows_eligible).  nmax = ceil(D/2); NW = 1 / 2 / 4 waves for 8 nmax <= 64 / <= 128 / more (rows_waves);
#     ns = ceil(ceil(23 nmax / 16) / NW):  splr_grad_kernel<1,12> (NW 1), <2,8> (NW 2, ns <= 8), <2,12>, <4,9> (ns <= 9), <4,12>;
#     splr_update_kernel<26> for M <= 104, <32> above.
#   tile form (nnest_spline_train.hip, DISPATCH_SPLT): key = 10 NTh + NH, NTh = ceil(ceil(D/2) / 16), NH = native hidden / 16;
#     rows per tile 16 for NTh 1, 8 above (rows_per_tile).  M > 128 takes the host epoch loop (flow.train_epochs_host with
#     flow.chunked_epoch) over loss_grad.
# ROWS_TABLE runs the rows form in-process and the tile form (keys 11 / 21) in a child process with NNEST_SPL_ROWS=0.
ROWS_TABLE = [
    # D,  H, B,   M    rows form                     tile form (NNEST_SPL_ROWS=0)
    (2, 10, 1, 1),     # grad <1,12>, update <26>    key 11
    (16, 16, 4, 37),   # grad <1,12>, update <26>    key 11
    (17, 16, 3, 100),  # grad <2,8>,  update <26>    key 11   (nl 9 != nu 8)
    (22, 10, 1, 104),  # grad <2,8>,  update <26>    key 11
    (23, 16, 4, 105),  # grad <2,12>, update <32>    key 11
    (32, 16, 2, 128),  # grad <2,12>, update <32>    key 11
    (33, 16, 1, 37),   # grad <4,9>,  update <26>    key 21
    (50, 10, 3, 100),  # grad <4,9>,  update <26>    key 21
    (51, 16, 4, 128),  # grad <4,12>, update <32>    key 21
    (64, 16, 2, 1),    # grad <4,12>, update <26>    key 21
]
TILES_TABLE = [
    # D,  H, B,   M    tile form
    (65, 16, 2, 100),  # key 31 (NTh 3, NH 1), image rebuilt per minibatch
    (70, 16, 1, 129),  # key 31, host epoch loop (M > 128)
    (100, 16, 2, 37),  # key 41 (NTh 4, NH 1)
    (128, 16, 5, 64),  # key 41, B 5
    (8, 17, 2, 100),   # key 12 (NTh 1, NH 2: hidden 17 padded to 32)
    (8, 32, 5, 129),   # key 12, B 5, host epoch loop
    (40, 17, 1, 37),   # key 22 (NTh 2, NH 2)
    (40, 32, 2, 105),  # key 22
]
# one shape per tile key for nnest_spline_vjp (always the tile form): (D, H, B, M, key)
VJP_TABLE = [(16, 16, 2, 37, 11), (50, 16, 3, 100, 21), (70, 16, 1, 64, 31), (100, 16, 2, 37, 41), (8, 32, 2, 100, 12),
             (40, 17, 1, 37, 22)]


def tile_key(D, H):
    nh = {16: 1, 32: 2}[16 if H <= 16 else 32]
    return 10 * (-(-(D - D // 2) // 16)) + nh


def random_weights(D, H, B, K=8, seed=0):
    """the reference's construction of a fresh SingleSpeedSpline (HipSpline.default_init) on the CPU: ActNorm s, t ~ N(0,1), the
    1x1 convolutions from the LU decomposition of a random orthogonal matrix, Linear layers U(-1/sqrt(fan_in), 1/sqrt(fan_in))
    -> (packed float32 weights, P [B, D, D] float32)"""
    import torch
    from oracle import spline_grad as sg
    g = torch.Generator()
    g.manual_seed(int(seed))
    parts, Ps, lu = [], [], None
    for name, shape in sg.layer_shapes(D, H, B, K):
        leaf = name.split('.')[-1]
        if leaf in ('s', 't'):
            parts.append(torch.randn(D, generator=g))
        elif leaf == 'L':
            Q = torch.linalg.qr(torch.randn(D, D, generator=g, dtype=torch.float64))[0]
            P, L, U = torch.linalg.lu(Q)
            Ps.append(P.to(torch.float32))
            lu = U
            parts.append(L.to(torch.float32).reshape(-1))
        elif leaf == 'S':
            parts.append(torch.diagonal(lu).to(torch.float32))
        elif leaf == 'U':
            parts.append(torch.triu(lu, diagonal=1).to(torch.float32).reshape(-1))
        else:
            fan_in = shape[1] if len(shape) == 2 else fan_in
            parts.append((torch.rand(int(np.prod(shape)), generator=g) * 2 - 1) / np.sqrt(fan_in))
    return torch.cat(parts).numpy().astype(np.float32), torch.stack(Ps).numpy()


def saturate(w, shapes, factor=60.0):
    """scale the last layer (net.6) of every conditioner: spline logits beyond 20, past the softplus threshold, and saturated
    softmax bins"""
    w = np.array(w, np.float32)
    for name, sl in tensor_slices(shapes).items():
        if '.net.6.' in name:
            w[sl] *= np.float32(factor)
    return w


def make_rows(rng, n, D, outliers=0.05):
    """uniform rows on [-1, 1] with ~5 % of them scaled by 4: after the ActNorm initialisation those reach the linear tails"""
    X = rng.uniform(-1, 1, size=(n, D))
    X[rng.uniform(size=n) < outliers] *= 4
    return X.astype(np.float32)


# tolerances of the GPU kernels against the float64 oracle (tests/test_gpu_spline_grad.py)
GPU_RTOL_T, GPU_FLOOR = 1e-3, 2e-5
