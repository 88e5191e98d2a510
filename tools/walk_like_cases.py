"""Developer tool, CPU only: chooses the seeds of tests/test_gpu_walk_likes.py and tests/test_gpu_tile_data_likes.py with the numpy
restatement of the walk (tests/mcmc_adapt_check.py) through the oracle's flows on the initialisations the GPU tests use
(tests/tile_like_check.py analytic_case, data_case).  Per case the first seed from 9000 + x_dim on for which the restatement alone,
on the restated draws (tests/mcmc_walk_check.mcmc_draws), moves some but not all local steps under every configuration the case
runs and, under each with global steps, has among the walkers that start inside the box an accepted and a refused global proposal
whose walker's decisions up to there all lie further than ten times the tolerance in force from their thresholds
(tile_like_check.seed_is_fair).  Prints the two tables tile_like_check.WALK_SEEDS and DATA_SEEDS hold.

`prior` chooses the prior width and the seed of every case of tests/test_gpu_prior_tile.py the same way (tests/prior_tile_check.py
pick): widths 1, 2, 0.5, 0.25, each moved to the first base (1 + j / 4096) under which the float32 restatement of the prior term
leaves half of B_pi unused on the case's start, and sixty seeds from 9000 + x_dim on, four hundred where those hold no fair pair; the
first pair under which the restatement with the normal prior in the target, at tile_like_check.DATA_CONFIG, moves some but not all
local steps, accepts and refuses a global proposal, starts with more than C / 4 finite rows and has NO acceptance margin within ten
times the tolerance in force -- the flow's, plus B, plus B_pi.  It prints the tables prior_tile_check.PRIOR_SEEDS and
BORDER_EXCEPTIONS hold; a case without such a pair is printed with the fair pair that has the fewest borderline decisions.

Usage: python tools/walk_like_cases.py [walk|data|prior]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import tile_like_check as tl   # noqa: E402


def walk_cases():
    from tests.test_gpu_fused_likes import NVP_TABLE, SPLINE_TABLE
    return [('nvp',) + c for c in NVP_TABLE] + [('spline',) + c for c in SPLINE_TABLE]


def choose_walk():
    print('WALK_SEEDS = {')
    for case in walk_cases():
        target_of_beta, z0 = tl.analytic_case(*case)
        seed = tl.pick_seed(target_of_beta, z0, list(tl.CONFIGS.values()), 9000 + case[3])
        stats = [tl.walk_stats(target_of_beta(c[0]), z0, seed, c) for c in tl.CONFIGS.values()]
        print('    %r: %d,   # (accepted, refused, local moved, local) %s' % (case, seed, stats), flush=True)
    print('}')


def choose_data():
    print('DATA_SEEDS = {')
    cases = [('gdata', D, H) for D, H in tl.GDATA_CASES if D >= 2] + [('glm',) + c for c in tl.GLM_CASES]
    for case in cases:
        target_of_beta, z0, _ = tl.data_case(*case)
        seed = tl.pick_seed(target_of_beta, z0, [tl.DATA_CONFIG], 9000 + case[1])
        print('    %r: %d,   # %s' % (case, seed, tl.walk_stats(target_of_beta(tl.BETA_DATA), z0, seed, tl.DATA_CONFIG)), flush=True)
    print('}')


def _pick_prior(case):
    from tests import prior_tile_check as pt
    return (case,) + pt.pick(case)


def choose_prior():
    import multiprocessing
    from tests import prior_tile_check as pt
    exceptions = {}
    print('PRIOR_SEEDS = {')
    with multiprocessing.Pool(12) as pool:
        for case, width, seed, st, exact in pool.imap(_pick_prior, pt.CASES):
            print('    %r: (%r, %d),   # %s' % (case, width, seed, st), flush=True)
            if not exact:
                exceptions[case] = st['border']
    print('}')
    print('BORDER_EXCEPTIONS = %r' % (exceptions,))


if __name__ == '__main__':
    what = sys.argv[1] if len(sys.argv) > 1 else 'both'
    if what in ('walk', 'both'):
        choose_walk()
    if what in ('data', 'both'):
        choose_data()
    if what == 'prior':
        choose_prior()
