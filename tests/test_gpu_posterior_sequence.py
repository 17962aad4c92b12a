"""GPU tier of the stale-state sequences (tests/posterior_sequence.py): ONE context lives through a seeded schedule of some sixty calls
-- the fifteen posterior entry points added since tests/test_gpu_round3.py's sequence test (and predict) in the modes their registered
scalers allow, with masks, pending rows, both forms of loo and predict_cov, row counts on either side of the 256-row padding and scripted
visits of one, two and three chunks; set_params, X and y scaler changes, the training calls and option changes of that test, and
documented failing calls (a NaN found on the device, rows that are not in the fit, a host-side argument error) each followed directly by
a valid call of an entry point that shares its buffers.  Every posterior step is compared (a) bit for bit with a fresh context that
makes the same call once and (b) with the CPU reference under the bound of the entry point's own GPU test.  What a call leaves behind
in the buffers, flags and cached operands that live as long as the context (the padded chunk buffers, C / V, the typed Li and Fall^T,
the borrowed training scratch, the update / loo / forget work sets, the row feed) must never reach a later call."""
import time

import pytest

from tests import posterior_sequence as PS

pytestmark = pytest.mark.gpu

IDS = ['%d-%d-%d-%s' % (g + (dt,)) for g, dt in PS.CASES]


def _engine(D, S, M, dtype):
    from scfgp_amd.engine import HipEngine
    return HipEngine(D, S, M, dtype=dtype)


def test_geometries_cover_the_padding_and_the_rank_s_projection():
    """K < Kp and K = Kp are both in the set, and at least one geometry projects through the S columns (Sp < Dp: the rank-S buffer of
    the chunk pipeline is live)"""
    padded, lowrank = set(), set()
    for D, S, M in PS.GEOMETRIES:
        eng = _engine(D, S, M, 'f64')
        d = eng.dims()
        eng.close()
        assert d['K'] == 2 * (S + M) and d['Kp'] >= d['K'] and d['Kp'] % 128 == 0
        padded.add(d['K'] < d['Kp'])
        lowrank.add((S + 1 + 15) // 16 * 16 < d['Dp'])
        ref = PS.RefEngine(D, S, M).dims()
        assert (ref['Kp'], ref['Dp']) == (d['Kp'], d['Dp'])
    assert padded == {True, False} and True in lowrank


@pytest.mark.parametrize('ci', range(len(PS.CASES)), ids=IDS)
def test_one_context_through_a_schedule_of_posterior_calls(ci):
    steps = PS.make_schedule(ci)
    PS.check_schedule(steps, ci)
    t0 = time.time()
    run = PS.Runner(ci, _engine)
    try:
        counts = run.run(steps)                # an assertion carries the step number and the log of the steps so far
    finally:
        run.close()
    print('%s: %d steps, %d posterior steps against a twin, %d reference checks, %d failing calls, %.1f s' %
          (IDS[ci], len(steps), counts['twin'], counts['records'], counts['failing'], time.time() - t0))
    assert counts['twin'] == sum(st['op'] == 'post' for st in steps) and counts['failing'] == sum(st['op'] == 'fail' for st in steps)
