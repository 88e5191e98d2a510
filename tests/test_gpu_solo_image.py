"""The solo lane image (nnest_amd/csrc/solo_tile.h: solo_image_kernel; built by launch_repack beside the fragment image) and the
launch prologue that reads it: the one-walker-per-wave kernels no longer gather their weights from the packed vector at every
launch, so (1) the image must never be older than the weights, by whichever route they changed; (2) every layout instantiation
(U = 1..4 slots per class, 4 / 8 / 12 walkers per workgroup, weights in registers or in LDS) must still run the chains of the
image-form kernel on the same noise; (3) the usable-chain flag, whose first x now waits in LDS, must still be the reference's test.
Every launch is 3 steps."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
S = 3


@pytest.fixture(scope='module')
def hip():
    from nnest_amd import flow
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return flow


def cpu(t):
    return t.detach().cpu().numpy()


def rel(a, b):
    return float(np.max(np.abs(a - b) / (1.0 + np.abs(b))))


# ---- (1) the image is never stale -------------------------------------------------------------------------------------------
D1, C1 = 50, 37


def every_route(nvp):
    """one launch of every kernel that stages the flow's weights, on inputs that do not depend on the weights: a tuple of tensors"""
    rng = np.random.RandomState(3)
    z0 = torch.from_numpy(rng.uniform(-0.5, 0.5, size=(C1, D1)).astype(np.float32)).cuda()
    out = []
    x, _, logl, _ = nvp.inverse_loglike(0, 5.0, z0)
    for dyn in (False, 'batch'):
        z, l = z0.clone(), logl.clone()
        res = nvp.mh_steps(0, 5.0, z, l, -1e300, 0.05, S, seed=5, dynamic=dyn)
        out += [z, l, res['x'], res['n_accept_word'], res['scale']]
    if nvp.supports_fused_slice(C1):
        z, l = z0.clone(), logl.clone()
        res = nvp.slice_steps(0, 5.0, z, l, -1e300, 0.3, S, seed=5)
        out += [z, l, res['x'], res['n_eval']]
    if nvp.ensemble_max_walkers(0) >= C1:
        res = nvp.ensemble_steps(0, z0, S, seed=5)
        out += [res['z'], res['x'], res['lp']]
        res = nvp.mcmc_steps(0, z0, S, 0.05, seed=5)
        out += [res['z'], res['x'], res['lp'], res['logl']]
    if nvp.importance_refusal(0) is None:
        res = nvp.importance_evidence(0, 256, seed=5, want_samples=True)
        out += [res['x'], res['logl'], res['logw'], res['sums']]
    return out


def reach_load(hip, nvp, w2):
    nvp.load_packed(w2)


def reach_train(hip, nvp, w2):
    """two epochs of the rows form (the launch's own repack behind it); the affine-scale-off flow trains in the one-workgroup form,
    which rebuilds the fragment image inside the kernel"""
    assert nvp.train_form_for(100)[0] == ('rows' if nvp.mh_form_for(C1) == 'solo' else 'single')
    rng = np.random.RandomState(11)
    xt, xv = rng.uniform(-1, 1, size=(200, D1)), rng.uniform(-1, 1, size=(50, D1))
    perm = torch.from_numpy(np.stack([rng.permutation(200) for _ in range(2)]).astype(np.int32))
    r = nvp.train_epochs(xt, xv, perm, seed=1, batch=100, max_epochs=2, lr=1e-2)
    assert r['epochs_run'] == 2


def reach_adam(hip, nvp, w2):
    x = torch.from_numpy(np.random.RandomState(12).uniform(-1, 1, size=(64, D1)).astype(np.float32)).cuda()
    _, grad = nvp.loss_grad(x)
    nvp.adam_step(grad, 1e-2, 0.0)


@pytest.mark.parametrize('scale', ['', 'translate'])
@pytest.mark.parametrize('reach', [reach_load, reach_train, reach_adam])
def test_lane_image_follows_the_weights(hip, reach, scale):
    """W1, a launch of every kernel, then W2 by one route, the same launches again: bit for bit what a fresh handle computes that only
    ever saw the stored W2.  scale='translate': the affine-scale-off flow, whose every weight change runs through zero-scale-nets (its
    populations run the image forms; the handle still carries a lane image)."""
    w1 = hip.HipNVP(D1, 16, 3, 1, seed=1).store_packed()
    w2 = hip.HipNVP(D1, 16, 3, 1, seed=2).store_packed()
    nvp = hip.HipNVP(D1, 16, 3, 1, scale=scale)
    nvp.load_packed(w1)
    first = every_route(nvp)
    reach(hip, nvp, w2)
    second = every_route(nvp)
    fresh = hip.HipNVP(D1, 16, 3, 1, scale=scale)
    fresh.load_packed(nvp.store_packed())
    want = every_route(fresh)
    assert len(second) == len(want) and len(want) >= 10
    for i, (a, b) in enumerate(zip(second, want)):
        assert torch.equal(a, b), (reach.__name__, scale, i)
    assert any(not torch.equal(a, b) for a, b in zip(first, second))   # (the weights did change what the launches compute)


# ---- (2) every layout instantiation against the image-form kernel -----------------------------------------------------------
_flows = {}


def flow_of(hip, D):
    if D not in _flows:
        nvp = hip.HipNVP(D, 16, 3, 1, seed=D)
        rng = np.random.RandomState(D)
        init = rng.uniform(-0.5, 0.5, size=(2100, D))
        z0, _ = nvp.forward(init)
        _flows[D] = (nvp, z0, hip.loglike(0, init, 5.0))
    return _flows[D]


@pytest.mark.parametrize('rule', ['fixed', 'product', 'lag0'])
@pytest.mark.parametrize('C', [5, 1030, 2100])
@pytest.mark.parametrize('D', [2, 50, 80, 128])
def test_every_layout_runs_the_image_forms_chains(hip, D, C, rule):
    """U = 1, 2, 3, 4; a ragged tile of 4 walkers per workgroup, 8 and 12 per workgroup; fixed step, the product's batch rule and lag 0.
    Solo against mh_kernel's image form on the same in-kernel noise, with the bounds tests/test_gpu_solo.py holds the solo form to
    against another form (test_solo_agrees_with_the_quad_form_and_shards): accept counts differ in at most 3 of 600 walkers
    (C // 200 here), the others agree to 2e-5.
    The product's schedule (16 exact steps in front of lag 8) exists in the solo form only; over a launch of 3 steps it is two exact
    steps and a third at the scale they end with -- the chains of lag 0, which is what the image form runs beside it (only the last
    step's vote, which lag 0 applies to the scale it reports and the product's schedule does not, sets the two apart)."""
    nvp, z0, l0 = flow_of(hip, D)
    kw = {'fixed': {}, 'product': dict(dynamic='batch'), 'lag0': dict(dynamic='batch', lag=0)}[rule]
    assert nvp.mh_form_for(C, **kw) == 'solo'
    if rule == 'product':
        assert nvp.default_lag(C) > S and nvp.default_warm(C, 'batch', nvp.default_lag(C)) >= S - 1
    star = float(np.median(cpu(l0[:C]))) - 50.0
    out = {}
    for form in ('solo', 'image'):
        z, l = z0[:C].clone(), l0[:C].clone()
        res = nvp.mh_steps(0, 5.0, z, l, star, 0.05, S, seed=21, form=form, **(kw if form == 'solo' or not kw else dict(dynamic='batch', lag=0)))
        if kw:
            nvp.check_sync(res)
        out[form] = (cpu(z), cpu(l), cpu(res['x']), cpu(res['n_accept']), cpu(res['scale']))
    zs, ls, xs, ns, ss = out['solo']
    zi, li, xi, ni, si = out['image']
    same = ns == ni
    assert np.sum(~same) <= C // 200
    assert rel(zs[same], zi[same]) < 2e-5 and rel(ls[same], li[same]) < 2e-5 and rel(xs[same], xi[same]) < 2e-5
    if rule != 'product':
        assert np.array_equal(ss, si) or rel(ss, si) < 1e-6
    assert int(ns.sum()) > 0


# ---- (3) the usable-chain flag, first x in LDS ------------------------------------------------------------------------------
@pytest.mark.parametrize('D,C', [(50, 5), (128, 1030)])
def test_moved_flag_is_the_launchs_own_history(hip, D, C):
    """nested.py:432 (tests/test_gpu_solo.py::test_usable_chain_flag_is_the_references_test) at proposal scales down to where an
    accepted move leaves float32 coordinates where they were.  The history build exists for 4 walkers per workgroup only, and a walker's
    chain does not depend on its workgroup's size, so the history of the 1030-walker launch (8 per workgroup, weights in LDS) is that
    of its shards of at most 1000 walkers: the production launch must end on the history's last x, bit for bit, and its flag must be
    the history's first-against-last test."""
    if D == 50:
        g = np.load(os.path.join(G, 'mcmc_rosen_d50.npz'))
        nvp = hip.HipNVP(50, 16, 3, 1)
        nvp.load_packed(g['w'])
        init = g['init'][np.random.RandomState(17).randint(0, g['init'].shape[0], size=C)]
    else:
        nvp = hip.HipNVP(D, 16, 3, 1, seed=D)
        init = np.random.RandomState(17).uniform(-0.5, 0.5, size=(C, D))
    z0, _ = nvp.forward(init)
    l0 = hip.loglike(0, init, 5.0)
    star = float(np.min(cpu(l0))) - 1e3
    parted = 0
    for step in (5e-2, 1e-5, 2e-7):
        z, l = z0.clone(), l0.clone()
        res = nvp.mh_steps(0, 5.0, z, l, star, step, S, seed=3, form='solo')
        hx = []
        for lo in range(0, C, 1000):
            hi = min(C, lo + 1000)
            zh, lh = z0[lo:hi].clone(), l0[lo:hi].clone()
            hx.append(cpu(nvp.mh_steps(0, 5.0, zh, lh, star, step, S, seed=3, walker_offset=lo, history=True, form='solo')['hist_x']))
        hx = np.concatenate(hx)
        na = cpu(res['n_accept'])
        assert np.array_equal(cpu(res['x']), hx[:, -1])
        assert np.all((na >= 0) & (na <= S))                                   # the flag does not leak into the count
        moved_ref = np.all(hx[:, 0] != hx[:, -1], axis=1)
        assert np.array_equal(cpu(res['moved']), moved_ref), (step, int(np.sum(cpu(res['moved']) != moved_ref)))
        assert not np.any(moved_ref & (na == 0))                               # no move without an accept
        parted += int(np.sum((na > 0) & ~moved_ref))
    if C > 1000:
        assert parted > 0                                                      # the small scales did separate the two notions
