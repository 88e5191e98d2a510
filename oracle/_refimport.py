"""Import the upstream reference (adammoss/nnest v0.4.2, unmodified, read-only) for the fixture generators.

Test infrastructure: the checkout of the reference is named by the environment variable NNEST_REFERENCE (the directory that
holds its `nnest` package). The reference needs two logging-only modules the image lacks
(tensorboard, getdist); neither touches arithmetic, so they are replaced
by inert placeholders in sys.modules before `import nnest`. Nothing here is imported by
the product package, bench.py or the test suite: the suite reads what the generators stored under tests/golden/.
"""
import os
import sys
import types


def reference_root():
    root = os.environ.get('NNEST_REFERENCE', '')
    if not os.path.isdir(os.path.join(root, 'nnest')):
        raise SystemExit('NNEST_REFERENCE=%r: expected a checkout of adammoss/nnest v0.4.2 (the directory that holds nnest/)' % root)
    return os.path.abspath(root)


def import_reference():
    import matplotlib
    matplotlib.use('Agg')
    import torch
    import torch.utils  # noqa: F401

    if 'torch.utils.tensorboard' not in sys.modules:
        tb = types.ModuleType('torch.utils.tensorboard')

        class SummaryWriter(object):  # logging sink only
            def __init__(self, *a, **k):
                pass

            def add_scalar(self, *a, **k):
                pass

            def add_figure(self, *a, **k):
                pass

        tb.SummaryWriter = SummaryWriter
        sys.modules['torch.utils.tensorboard'] = tb
    if 'getdist' not in sys.modules:
        gd = types.ModuleType('getdist')
        gm = types.ModuleType('getdist.mcsamples')

        class MCSamples(object):
            pass

        gd.MCSamples = MCSamples
        gm.MCSamples = MCSamples
        gd.mcsamples = gm
        sys.modules['getdist'] = gd
        sys.modules['getdist.mcsamples'] = gm
    # on the path for the import only: the reference has a `tests` package of its own, and a path entry left behind would
    # shadow this repo's `tests` in every process spawned later (spawn hands the parent's sys.path to the child)
    root = reference_root()
    sys.path.insert(0, root)
    try:
        import nnest  # noqa: F401
        import nnest.nested, nnest.mcmc, nnest.sampler, nnest.trainer, nnest.networks  # noqa: F401,E401
    finally:
        sys.path.remove(root)
    return nnest
