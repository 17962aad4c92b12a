"""CPU tier of the geometry sweep of the posterior entry points (tests/posterior_sequence.py: SWEEP_GEOMETRIES, sweep_schedule): the set
covers every geometry class it is there for (the column plan of the apply products, the padding of K, J, D + 1 and S + 1, the rank-S
projection, M < S), restated in Python so that an edit of the list cannot drop one; the sweep schedule of every geometry runs through the
runner on the CPU references, with a second reference context in the f16x3 context's place; no check is vacuous (every bounded record
fails when moved by ten times its bound, every exact one by one ulp); every one of the seventeen entry points had a bounded record moved at
every geometry; and a correct fp32 evaluation of predict stays inside half the fp32 bound under the schedule's own parameters, rows and
scalers, so that a miss on the GPU means the kernel."""
import time

import numpy as np
import pytest

from oracle import scfgp_oracle as O
from tests import parity
from tests import posterior_sequence as PS

GEOS = PS.SWEEP_GEOMETRIES
IDS = ['%d-%d-%d' % g for g in GEOS]
MOVED = {}                  # geometry -> entry points of which an output was moved by ten times its bound


def test_the_set_covers_the_geometry_classes():
    table = {g: PS.geometry_classes(*g) for g in GEOS}
    # the rows of the table as the issue states them: K and Kp
    assert [(c['K'], c['Kp']) for c in table.values()] == [(8, 128), (30, 128), (130, 256), (150, 256), (172, 256), (192, 256), (256, 256),
                                                           (258, 384), (322, 384), (384, 384)]
    seen = {g: PS.classes_of(*g) for g in GEOS}
    for name in PS.SWEEP_CLASSES:
        assert any(name in s for s in seen.values()), 'no geometry of the set is in the class %r' % name
    # the plan restated: tile counts against ApplyPlan's rule, and the partial slots against what the tiles span
    for (D, S, M), c in table.items():
        assert c['K'] == 2 * (S + M) and c['Kp'] % 128 == 0 and c['Kp'] >= c['K'] and c['Kp'] - c['K'] < 128
        assert 128 * c['n128'] + 64 * c['n64'] >= c['K'] > 128 * c['n128'] + 64 * (c['n64'] - 1)
        assert (c['n128'] == 0) == (c['K'] <= 256) and c['n64'] <= (4 if c['small'] else 2)
        assert c['slots'] >= c['covered'] and c['Kp'] == 128 * (c['gfull'] + c['gstrip'])
        assert 0 <= c['jpad'] < 128 and 0 <= c['dpad'] < 16 and 0 <= c['spad'] < 16
        assert PS.RefEngine(D, S, M).dims() == {k: c[k] for k in ('K', 'Kp', 'Jp', 'Dp', 'Sp')}
    # geometries on either side of the f16x3 split products (they run for K > 256 only)
    assert sum(c['small'] for c in table.values()) == 7 and len(GEOS) == 10
    # the set is separate from the sequences' geometries, which keep their cases
    assert PS.GEOMETRIES == [(7, 3, 40), (5, 4, 60), (40, 6, 150), (5, 12, 200)] and not set(GEOS) & set(PS.GEOMETRIES)
    assert (1, 1, 1) not in GEOS and all(M > 1 for _, _, M in GEOS)


def test_sweep_schedules_hold_every_entry_point_in_every_mode():
    for g in GEOS:
        steps = PS.sweep_schedule(*g)
        info = PS.check_sweep(steps)
        assert len(PS.SWEEP_ENTRY_POINTS) == 17 and not any(st['op'] in ('fail', 'eval', 'rows', 'train', 'option') for st in steps)
        post = [st for st in steps if st['op'] == 'post']
        assert {st['m'] for st in post} == {5} and {st['T'] for st in post} == {1, 37, 257, 300}
        PS.sweep_schedule.cache_clear()
        assert PS.sweep_schedule(*g) == steps                     # a function of the geometry alone
    print('steps per geometry: %d, posterior steps: %d' % (info['steps'], info['posterior']))


@pytest.mark.parametrize('g', GEOS, ids=IDS)
def test_dry_run_on_the_references_and_no_check_is_vacuous(g):
    moved = {'bound': {}, 'exact': 0, 'row0': 0, 'mirror': 0, 'conditioned': 0}
    refs = {}
    holder = {}

    def on_records(i, a, got, recs):
        # a condition on the inputs: no norm-relative record of a step on row 0 alone is bounded relative to a cancellation
        refs[i] = {rec[0]: rec[3] for rec in recs if rec[1] == 'relnorm'}
        if 'row0_of' in steps[i]:
            for label, ref in refs[i].items():
                if label in refs[steps[i]['row0_of']]:
                    assert PS.conditioned_row0(ref, refs[steps[i]['row0_of']][label]) is not False, (i, a['ep'], label)
                    moved['conditioned'] += 1
            if a['ep'] == 'acquire_kg' and a['T'] == 257 and not (g[0] == 1 and a['R'] == 37):
                assert PS.kg_conditioning(a, holder['run'].fit) <= 1.0, (i, PS.kg_conditioning(a, holder['run'].fit))
            if a['ep'] == 'acquire' and 'grad' in a['want']:
                c = PS.acquire_grad_cancellation(a, holder['run'].fit)
                assert c <= PS.GRAD_CANCEL, (i, a['kind'], c)
        for rec in recs:
            PS.evaluate(rec)
            bad = PS.perturbed(rec)
            if bad is None:
                continue
            with pytest.raises(AssertionError):
                PS.evaluate(bad)
            if rec[0].startswith('(c)'):
                moved['row0'] += 1
            elif rec[0].startswith('(d)'):
                moved['mirror'] += 1
            elif rec[1] == 'exact':
                moved['exact'] += 1
            else:
                assert PS.ratio(rec) is not None and PS.ratio(rec) <= 1.0 and PS.ratio(bad) > 1.0, rec[0]
                moved['bound'][a['ep']] = moved['bound'].get(a['ep'], 0) + 1

    t0 = time.time()
    steps = PS.sweep_schedule(*g)
    run = PS.Runner(g + ('f64',), lambda D, S, M, dtype: PS.RefEngine(D, S, M, dtype), twins=False, on_records=on_records, mirror='f16x3')
    holder['run'] = run
    counts = run.run(steps)
    run.close()
    print('%s: %d steps, %s, moved %s, %.1f s' % (g, len(steps), counts, moved, time.time() - t0))
    assert counts['twin'] == 0 and counts['records'] > 0 and counts['row0'] > 0 and counts['mirror'] > 0
    assert moved['exact'] > 0 and moved['row0'] > 0 and moved['mirror'] > 0 and moved['conditioned'] > 0
    # every one of the seventeen entry points had a bounded record moved at this geometry
    assert set(moved['bound']) == set(PS.SWEEP_ENTRY_POINTS), sorted(set(PS.SWEEP_ENTRY_POINTS) - set(moved['bound']))
    assert len(run.min_pivot2) == 2 and min(run.min_pivot2) >= 0.25
    MOVED[g] = set(moved['bound'])


def test_every_entry_point_had_a_record_moved_in_every_geometry_class():
    """over the geometries that ran before this test in the session (all ten in a full run)"""
    if len(MOVED) == len(GEOS):
        for name in PS.SWEEP_CLASSES:
            there = [g for g in GEOS if name in PS.classes_of(*g)]
            assert there and all(MOVED[g] == set(PS.SWEEP_ENTRY_POINTS) for g in there), name


@pytest.mark.parametrize('g', GEOS, ids=IDS)
def test_a_correct_fp32_predict_stays_inside_half_the_fp32_bound(g):
    """parity.apply32_model of the oracle's Phi, alpha and Li (PS.new_params' docstring) under the sweep schedule's own parameters, rows
    and X / y scalers, at the 257 rows of the schedule's first predict step: a condition on the choice of inputs, not a tolerance"""
    D, S, M = g
    steps = PS.sweep_schedule(*g)
    fit = PS.Fit(D, S, M)
    fit.xs = PS.x_scaler(steps[0]['algo'], D); fit.ys = PS.y_scaler(steps[3]['algo'])
    fit.params = PS.new_params(np.random.default_rng(steps[1]['seed']), D, S, M)
    rng = np.random.default_rng(steps[2]['seed'])
    fit.Xraw = PS.raw_rows(rng, steps[2]['N'], D); fit.yraw = PS.raw_targets(rng, fit.Xraw)
    alpha, Li = fit.factors()
    st = next(s for s in steps if s['op'] == 'post')
    Xs = PS.materialise(st, fit)['X']
    assert Xs.shape == (257, D)
    mu0, sd0 = O.predict(Xs, alpha, Li, fit.params, S, M)
    Phi = O.feature_map(Xs, fit.params, D, S, M)
    mu = parity.apply32_model(Phi, alpha)
    V = parity.apply32_model(Phi, np.tril(Li).T)
    sd = np.sqrt(PS.kappa(fit.params) * (1.0 + np.sum(V * V, axis=1)))
    r = parity.predict_ratio(mu, sd, mu0, sd0, 'f32')
    print('%s: a correct fp32 predict stands at %.2f of the fp32 bound' % (g, r))
    assert r <= 0.5, r
