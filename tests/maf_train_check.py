"""MAF training held to float64 optimizer step by optimizer step: the table, the mask and the evaluator that tests/nvp_train_check.py's
check_step needs for the masked autoregressive flow; shared by tests/test_maf_train_check.py (CPU: the float32 MAF oracle plays the
kernel) and tests/test_gpu_maf_train_oracle.py (GPU: maf_grad_kernel<NT,L> + maf_reduce_kernel + adam, and maf_grad_kernel<NT,L> +
maf_update_kernel behind nnest_maf_train_epoch).

The MAF has RealNVP's packed layout (HipMAF inherits layer_shapes and default_init), so check_step, step_inputs, jittered,
away_from_kinks, the loss checks and BOUNDS are nvp_train_check's own, unchanged; what differs is
  evaluator   orc.NVP(..., kind='maf', base_beta=...): oracle/maf_oracle_impl.h, whose float64 mode is the reference here
  masked      the oracle's own rule, orc_maf_param_live(D, H, L, block, index in the net) -- first-layer entries with
              deg(hidden) < deg(input), hidden entries with deg(out) < deg(in), last-layer entries with deg(output) <= deg(hidden)

Bounds: BOUNDS of nvp_train_check with the floor F = 10 x MAF_FLOOR_MEASURED.  The float32 MAF oracle run as the kernel over every
row of TRAIN_TABLE, four steps each, needs NO floor (re-measured by test_maf_train_check.py::test_float32_maf_oracle_needs_no_floor),
so the per-tensor gradient bound is purely relative to the tensor's own largest gradient, R max|g64|_t with
R = max(3e-5, 10 x the float32 oracle's worst per-tensor relative error on the same input).  No bound comes from a kernel's output.

Instantiations: launch_maf_loss_grad / launch_maf_train_minibatch dispatch maf_grad_kernel<NT,L> for NT 1..4 x L 0..2 on (FlowShape.NT,
FlowShape.L) alone; expected_instantiation restates the two limits a shape has to pass to get there (maf_shape_supported's image in
one CU's LDS, launch_maf_grad_t's LDS bound) and TRAIN_TABLE reaches all twelve with hidden 16 and B 3."""
import numpy as np

from tests import nvp_train_check as ntc

MAF_FLOOR_MEASURED = 0.0             # the smallest F the float32 MAF oracle needs over TRAIN_TABLE (see the header)
BOUNDS = dict(ntc.BOUNDS, floor=10.0 * MAF_FLOOR_MEASURED)
OLD_WHOLE_VECTOR_RULE = 2e-4         # test_gpu_maf.py's one gradient bound: max|g - go| < 2e-4 max|go|


def frag_net_floats(NT, NH, L):
    """flow_tile.h: the fragment image of one net over NT tiles"""
    return NH * NT * 256 + L * NH * NH * 256 + NT * NH * 256 + 16 * NH + L * 16 * NH + 16 * NT


def expected_instantiation(c):
    """(NT, L) of the maf_grad_kernel a case trains in from the library's own rules, restated; None where they refuse the shape"""
    return instantiation(c.D, c.H, c.B, c.L, c.M)


def instantiation(D, H, B, L, M=1):
    """(NT, L) of the maf_grad_kernel a shape trains in, None where the library refuses it: nnest_maf_create (hidden 16, x_dim 2..128,
    maf_shape_supported: the image of both parity classes + the group table within 150 KiB) and launch_maf_grad_t (its LDS: block inputs,
    both nets' activations, the exchange area and two waves' staging areas, within 160 KiB - 512)"""
    NT = ntc.tiles(D)
    if H != 16 or D < 2 or NT > 4 or L > 2 or not 1 <= M <= 128:
        return None
    image_floats = B * 2 * frag_net_floats(2 * NT, 1, L) + B * 32 * NT
    if image_floats * 4 > 150 * 1024:
        return None
    stage_count = 2 * (2 * NT) + 2 * (L + 1)                      # StageMap<2 NT, 1, L>::count
    lds = (B * 2 * NT * 64 + B * 2 * (L + 1) * 64 + 2 * 2 * NT * 64) * 16 + 2 * stage_count * 16 * 16 * 4
    return (NT, L) if lds <= 160 * 1024 - 512 else None


def case(D, NT, L, M, B=None, beta=0.0, ragged=False):
    """a table row, its NT written out (expected_instantiation must agree: tests/test_maf_train_check.py); B 3 unless the rule above
    refuses it (then 2); ragged: also run as the only minibatch of batch = 128 > M"""
    if B is None:
        B = 3 if instantiation(D, 16, 3, L, M) else 2
    return ntc.case(D, 16, B, L, M, ('maf', 10 * NT + L), beta=beta, batches=ntc.both(M) if ragged else None)


# x_dim from the tile edges (2 | 32 / 33 | 64 / 65 | 96 / 97 | 128), minibatches from the 16-row tiles and their ragged ends
TRAIN_TABLE = [
    case(2, 1, 0, 1), case(33, 2, 0, 37, ragged=True), case(96, 3, 0, 128), case(97, 4, 0, 100),
    case(32, 1, 1, 17), case(64, 2, 1, 101), case(65, 3, 1, 16, ragged=True), case(128, 4, 1, 128),
    case(5, 1, 2, 100), case(64, 2, 2, 17), case(70, 3, 2, 37), case(128, 4, 2, 101, ragged=True),
    case(5, 1, 1, 37, B=1), case(5, 1, 1, 16, B=5),
    case(50, 2, 1, 100, beta=8, ragged=True),
    case(100, 4, 1, 100),                                         # BASELINE config 5's shape
]
IDS = [ntc.case_id(c) for c in TRAIN_TABLE]


def row(**want):
    """the one table row with these fields (rows are named by what they are, never by their position in the table)"""
    hits = [c for c in TRAIN_TABLE if all(getattr(c, k) == v for k, v in want.items())]
    assert len(hits) == 1, (want, len(hits))
    return hits[0]


# one launch of three minibatches against three launches: (case, batch, n_train) at an NT = 3 row and an L = 0 row
EPOCH_CASES = [(row(D=70, L=2), 37, 2 * 37 + 30), (row(D=33, L=0), 100, 230)]
VALID_CASE = row(D=65, L=1, M=16)


_SHAPES = {}


def make_oracle(c, w=None):
    """the MAF oracle of the case at weights w; without weights one shared object per case (check_step reads its shape only)"""
    from oracle import oracle as orc
    if w is None:
        if c not in _SHAPES:
            _SHAPES[c] = orc.NVP(c.D, c.H, c.B, c.L, None, base_beta=c.beta, kind='maf')
        return _SHAPES[c]
    return orc.NVP(c.D, c.H, c.B, c.L, w, base_beta=c.beta, kind='maf')


def evaluator(c):
    return lambda w: make_oracle(c, w)


_MASKS = {}


def masked(c):
    """bool [num_params]: parameters whose gradient is zero by construction, from the oracle's own rule"""
    key = (c.D, c.H, c.B, c.L)
    if key not in _MASKS:
        from oracle import oracle as orc
        live = orc.lib().orc_maf_param_live
        ns = c.H * c.D + c.H + c.L * (c.H * c.H + c.H) + c.D * c.H + c.D
        net = [np.array([live(c.D, c.H, c.L, b, i) for i in range(ns)], dtype=bool) for b in range(c.B)]
        _MASKS[key] = ~np.concatenate([net[b] for b in range(c.B) for _ in range(2)])
    return _MASKS[key]


def away_from_kinks(c, w, s):
    return ntc.away_from_kinks(c, w, s, evaluator=evaluator(c))


def check_step(c, pre, post, data, layer_shapes, what=''):
    return ntc.check_step(pre, post, data, make_oracle(c), ntc.LR, ntc.WD, layer_shapes, bounds=BOUNDS, what=what, evaluator=evaluator(c),
                          masked=masked(c))


def check_gradient(c, w, data, loss, grad, layer_shapes, what=''):
    """a gradient the kernel returns (loss_grad), held directly to float64 at weights w: the loss, the whole vector, tensor by tensor
    (check_step's bounds), masked elements exactly 0.  Returns the error / bound ratios."""
    ev = make_oracle(c, w)
    l64, g64 = ev.loss_grad(data, f64=True)
    g32 = ev.loss_grad(data)[1]
    g = np.asarray(grad, np.float64)
    mask = masked(c)
    assert g.shape == g64.shape and np.all(np.isfinite(g)), what
    assert np.all(g[mask] == 0), '%s: %d masked elements with a gradient' % (what, int(np.count_nonzero(g[mask])))
    out = dict(train_loss=abs(float(loss) - l64) / (BOUNDS['loss'] * (1 + abs(l64))))
    assert out['train_loss'] < 1, '%s: loss %.9g vs float64 %.9g' % (what, float(loss), l64)
    err = np.abs(g - g64)
    whole = BOUNDS['whole'] * (1e-3 + float(np.max(np.abs(g64))))
    assert np.max(err) < whole, '%s: gradient element %d: %.9g vs float64 %.9g (whole-vector bound %.3g)' % (
        what, int(np.argmax(err)), g[np.argmax(err)], g64[np.argmax(err)], whole)
    out['grad_whole'] = float(np.max(err) / whole)
    rtol = ntc.gradient_rtol(g32, g64, layer_shapes, BOUNDS)
    out['grad_tensor'] = 0.0
    for name, s, bound in ntc.tensor_bounds(g64, rtol, layer_shapes, BOUNDS):
        k = int(np.argmax(err[s]))
        assert err[s][k] <= bound, '%s: gradient %s[%d]: %.9g vs float64 %.9g (error / per-tensor bound %.3g; R %.3g)' % (
            what, name, k, g[s][k], g64[s][k], err[s][k] / bound, rtol)
        out['grad_tensor'] = max(out['grad_tensor'], float(err[s][k] / bound))
    return out
