"""GPU tier of the geometry sweep of the posterior entry points (tests/posterior_sequence.py: SWEEP_GEOMETRIES, sweep_schedule).  All
nineteen posterior entry points run on padded buffers whose kernels "need no edge code"; what a call launches depends on a few integer
classes of (D, S, M): the column plan of the apply products (64-wide tiles up to K = 256, 128-wide tiles and a 64-wide remainder above),
the padding of K to Kp and the Kp / 64 partial slots, Jp, Dp, Sp and whether the rank-S projection is live.  Each geometry of the set
sits in classes no other posterior test reaches (K = 8 and D = 1, M < S, three-tile small plans, K = 256 = Kp with J = Jp, K = 258 with
two live remainder columns and J one past Jp, a two-tile remainder, K = 384 with no remainder launch, D + 1 and S + 1 on and one past
the 16 boundary).  One context per (geometry, dtype) goes through the lean schedule: every entry point in every mode it has at T = 257
rows and then on row 0 of those rows alone, and is checked

  (b) against the CPU reference under the bound of the entry point's own GPU test;
  (c) bit for bit, row 0 alone against row 0 of the 257-row call, where include/scfgp_hip.h says a row's outputs depend on that row
      alone (PS.ROW_ALONE): a padding row or a tile tail that leaks into live rows is far below a reference tolerance at these sizes;
  (d) in the f32 case, bit for bit against an f16x3 context that makes the same calls, where the header says the two modes agree bit
      for bit (PS.F16X3_EQUAL); its split products run for K > 256 only.

Measured on the device (MI355X): 0.1 to 0.5 s per case, 21 tests in 9.7 s (8.9 s before predict_gradcov and predict_pd joined).  Largest
error / bound of each of the seventeen older entry points in f32 (every (c) and (d) record held exactly; each case prints its own line
of these):

    geometry   acquire acquire_kg condition forget loo predict predict_cov predict_grad predict_raw predict_y sample sample_argmax
               sample_grad sample_weights select select_iv select_qei
    1-2-2      0.22 0.23 0.19 0.27 0.21 0.21 0.076 0.25 0.2 2.2e-07 0.14 0.085 0.063 0.00012 0.055 0.75 0.091
    7-12-3     0.24 0.24 0.28 0.23 0.28 0.25 0.16 0.22 0.24 1.7e-07 0.16 0.15 0.096 0.00018 0.3 0.49 0.24
    70-5-60    0.17 0.11 0.042 0.027 0.047 0.049 0.092 0.042 0.032 0 0.2 0.16 0.029 0.0004 0.19 0.28 0.15
    15-15-60   0.13 0.35 0.058 0.041 0.059 0.044 0.1 0.037 0.038 0 0.29 0.16 0.035 0.0005 0.15 0.31 0.19
    16-16-70   0.39 0.44 0.22 0.14 0.22 0.12 0.088 0.15 0.11 2.1e-07 0.17 0.15 0.039 0.00035 0.2 0.35 0.14
    6-5-91     0.21 0.11 0.026 0.025 0.027 0.023 0.08 0.028 0.024 2.2e-07 0.089 0.1 0.024 0.00048 0.069 0.07 0.11
    9-8-120    0.16 0.083 0.048 0.045 0.058 0.042 0.072 0.048 0.039 2.1e-07 0.2 0.23 0.027 0.00051 0.12 0.19 0.19
    40-6-123   0.26 0.46 0.11 0.044 0.13 0.051 0.071 0.055 0.05 1.9e-07 0.18 0.18 0.042 0.00054 0.13 0.088 0.18
    33-3-158   0.11 0.088 0.038 0.028 0.035 0.033 0.068 0.037 0.028 2e-07 0.11 0.11 0.044 0.00062 0.079 0.12 0.22
    5-4-188    0.13 0.29 0.025 0.02 0.056 0.019 0.089 0.019 0.017 2e-07 0.24 0.46 0.05 0.00071 0.25 0.17 0.21

predict_gradcov and predict_pd, which joined last (four groups at the end of the schedule, on the fit that condition and forget have
moved): largest error / bound against the CPU closed forms under the bounds of their own GPU tests, per geometry and dtype, and the
seconds of the case.  Every (c) record (dvar, dcov, ice of row 0 alone), every (d) record (all eight outputs of the f16x3 context) and
every symmetry, diagonal, sign and subset record held exactly, at the three geometries with K > 256 as elsewhere:

    geometry   f32: predict_gradcov predict_pd   f64: predict_gradcov predict_pd   seconds f64 / f32
    1-2-2      0.019    0.04     4.4e-06  5.9e-06    0.2 / 0.1
    7-12-3     0.036    0.17     1.1e-05  5.3e-05    0.1 / 0.2
    70-5-60    0.015    0.094    2.6e-05  3.1e-05    0.3 / 0.4
    15-15-60   0.02     0.077    1e-05    5.5e-06    0.3 / 0.3
    16-16-70   0.035    0.14     1.3e-05  2.3e-05    0.3 / 0.3
    6-5-91     0.014    0.041    8e-06    1.1e-05    0.2 / 0.3
    9-8-120    0.016    0.08     8.5e-06  6.8e-06    0.3 / 0.3
    40-6-123   0.033    0.11     1.3e-05  1.7e-05    0.5 / 0.5
    33-3-158   0.0084   0.038    1.8e-05  1.3e-05    0.4 / 0.5
    5-4-188    0.02     0.034    1.4e-05  8.9e-06    0.4 / 0.4"""
import time

import pytest

from tests import posterior_sequence as PS

pytestmark = pytest.mark.gpu

GEOS = PS.SWEEP_GEOMETRIES
CASES = [(g, dt) for g in GEOS for dt in PS.DTYPES]
IDS = ['%d-%d-%d-%s' % (g + (dt,)) for g, dt in CASES]


def _engine(D, S, M, dtype):
    from scfgp_amd.engine import HipEngine
    return HipEngine(D, S, M, dtype=dtype)


def test_dims_of_every_geometry_of_the_set():
    """the context's own geometry against the Python restatement the CPU tier's class coverage rests on, and its points per chunk of
    predict_gradcov against the restatement of the header's formula"""
    for D, S, M in GEOS:
        ref = PS.RefEngine(D, S, M).dims()
        for dtype in PS.DTYPES + ('f16x3',):
            eng = _engine(D, S, M, dtype)
            d = eng.dims()
            for want_cov in (True, False):
                assert eng.gradcov_points_per_chunk(want_cov) == PS.gradcov_points_per_chunk(D, S, want_cov), ((D, S, M), want_cov)
            eng.close()
            assert {k: d[k] for k in ('K', 'Kp', 'Jp', 'Dp')} == {k: ref[k] for k in ('K', 'Kp', 'Jp', 'Dp')}, ((D, S, M), dtype, d, ref)


@pytest.mark.parametrize('g,dtype', CASES, ids=IDS)
def test_every_posterior_entry_point_at_this_geometry(g, dtype):
    steps = PS.sweep_schedule(*g)
    PS.check_sweep(steps)
    worst = {}

    def on_records(i, a, got, recs):
        for rec in recs:
            r = PS.ratio(rec)
            if r is not None:
                worst[a['ep']] = max(worst.get(a['ep'], 0.0), r)

    t0 = time.time()
    run = PS.Runner(g + (dtype,), _engine, twins=False, on_records=on_records, mirror='f16x3' if dtype == 'f32' else None)
    try:
        counts = run.run(steps)                # an assertion carries the step number and the log of the steps so far
    finally:
        run.close()
        print('%s: largest error / bound per entry point: %s' % (IDS[CASES.index((g, dtype))], ' '.join('%s %.2g' % kv for kv in sorted(worst.items()))))
    print('%s: %d steps, %d records (%d of row 0 alone, %d against the f16x3 context), %.1f s' %
          (IDS[CASES.index((g, dtype))], len(steps), counts['records'], counts['row0'], counts['mirror'], time.time() - t0))
    assert counts['records'] > 0 and counts['row0'] > 0 and (counts['mirror'] > 0) == (dtype == 'f32')
    assert set(worst) == set(PS.SWEEP_ENTRY_POINTS)
