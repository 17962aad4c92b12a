"""GPU tier of the stale-state sequences (tests/posterior_sequence.py): ONE context lives through a seeded schedule of some sixty calls
-- the eighteen posterior entry points added since tests/test_gpu_round3.py's sequence test (and predict) in the modes their registered
scalers allow, with masks, pending rows, both forms of loo and predict_cov, row counts on either side of the 256-row padding and scripted
visits of one, two and three chunks (predict_gradcov: three of its own chunks of points); set_params, X and y scaler changes, the
training calls and option changes of that test, and documented failing calls (a NaN found on the device, rows that are not in the fit,
a host-side argument error) each followed directly by a valid call of an entry point that shares its buffers.  Every posterior step is compared (a) bit for bit with a fresh context that
makes the same call once and (b) with the CPU reference under the bound of the entry point's own GPU test.  What a call leaves behind
in the buffers, flags and cached operands that live as long as the context (the padded chunk buffers, C / V, the typed Li and Fall^T,
the borrowed training scratch, the update / loo / forget work sets, the row feed) must never reach a later call.

predict_gradcov, predict_pd and acquire_kg joined last.  Their steps are inserted between the older ones, which keep their arguments,
seeds and order (tests/test_posterior_sequence_ref.py pins them) and see the fit they saw, since none of the new steps moves it: each
at least twice per schedule with weights, output subsets, grids of 1, 9 and 64 values and reference rows drawn per step; predict_gradcov
at three of its own chunks (16 684 points with a D x D array each) and predict_pd at three row chunks with the ICE rows around the
boundaries; weights that sum to 0 refused before `loo`, a NaN in a weighted row found on the device before `sample`, and a NaN row
that predict_gradcov keeps inside its own point's outputs before predict_cov.  The log of a step drawn at run time names the draw that
was used and the options it ran with.  Measured on the device (MI355X), every step equal to its twin: largest error / bound of the three
against the CPU references under the bounds of their own GPU tests, and the seconds of the case (9 tests in 13 s):

    case           acquire_kg predict_gradcov predict_pd   seconds
    7-3-40-f64     0.17       1.7e-05         0.0001       1.6
    7-3-40-f32     0.19       0.043           0.057        2.3
    5-4-60-f64     0.095      3.3e-05         1.6e-05      0.7
    5-4-60-f32     0.19       0.027           0.052        0.8
    40-6-150-f64   0.016      2.3e-05         2.6e-05      1.5
    40-6-150-f32   0.14       0.023           0.065        1.8
    5-12-200-f64   0.037      9.9e-06         9.7e-06      1.7
    5-12-200-f32   0.26       0.039           0.052        1.7"""
import time

import pytest

from tests import posterior_sequence as PS

pytestmark = pytest.mark.gpu

IDS = ['%d-%d-%d-%s' % (g + (dt,)) for g, dt in PS.CASES]
NEWEST = PS.NEWEST                                             # the entry points that joined the sequences last: their ratios are printed


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
        # the chunk of predict_gradcov, which places the scripted three-chunk visit: the header's formula restated against the engine's
        eng = _engine(D, S, M, 'f32')
        for want_cov in (True, False):
            assert eng.gradcov_points_per_chunk(want_cov) == PS.gradcov_points_per_chunk(D, S, want_cov), ((D, S, M), want_cov)
        eng.close()
    assert PS.BIG_GRADCOV == 2 * PS.gradcov_points_per_chunk(*PS.GEOMETRIES[1][:2], True) + 300 == 16684
    assert padded == {True, False} and True in lowrank


@pytest.mark.parametrize('ci', range(len(PS.CASES)), ids=IDS)
def test_one_context_through_a_schedule_of_posterior_calls(ci):
    steps = PS.make_schedule(ci)
    PS.check_schedule(steps, ci)
    worst = {}

    def on_records(i, a, got, recs):
        if a['ep'] in NEWEST:
            for rec in recs:
                r = PS.ratio(rec)
                if r is not None:
                    worst[a['ep']] = max(worst.get(a['ep'], 0.0), r)

    t0 = time.time()
    run = PS.Runner(ci, _engine, on_records=on_records)
    try:
        counts = run.run(steps)                # an assertion carries the step number and the log of the steps so far
    finally:
        run.close()
        print('%s: largest error / bound: %s' % (IDS[ci], ' '.join('%s %.2g' % kv for kv in sorted(worst.items()))))
    print('%s: %d steps, %d posterior steps against a twin, %d reference checks, %d failing calls, %.1f s' %
          (IDS[ci], len(steps), counts['twin'], counts['records'], counts['failing'], time.time() - t0))
    assert counts['twin'] == sum(st['op'] == 'post' for st in steps) and counts['failing'] == sum(st['op'] == 'fail' for st in steps)
    assert set(worst) == set(NEWEST)
