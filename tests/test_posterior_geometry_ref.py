"""CPU tier of the geometry sweep of the posterior entry points (tests/posterior_sequence.py: SWEEP_GEOMETRIES, sweep_schedule): the set
covers every geometry class it is there for (the column plan of the apply products, the padding of K, J, D + 1 and S + 1, the rank-S
projection, M < S), restated in Python so that an edit of the list cannot drop one; the sweep schedule of every geometry runs through the
runner on the CPU references, with a second reference context in the f16x3 context's place; no check is vacuous (every bounded record
fails when moved by ten times its bound, every exact one by one ulp); every one of the nineteen entry points had a bounded record moved at
every geometry; the groups of the seventeen older entry points keep the seeds they had before predict_gradcov and predict_pd joined; no
predict_pd step sums its features to a cancellation; and a correct fp32 evaluation of predict, predict_gradcov and predict_pd stays
inside half the fp32 bound under the schedule's own parameters, rows and scalers, so that a miss on the GPU means the kernel."""
import time

import numpy as np
import pytest

from oracle import scfgp_oracle as O
from tests import gradcov_ref as GC
from tests import parity
from tests import pd_ref as PD
from tests import posterior_sequence as PS

GEOS = PS.SWEEP_GEOMETRIES
IDS = ['%d-%d-%d' % g for g in GEOS]
MOVED = {}                  # geometry -> entry points of which an output was moved by ten times its bound
NEW = ('predict_gradcov', 'predict_pd')
# the seeds of the parameters, the rows of the fit, and the first and the last group of the seventeen older entry points, as the schedules
# stood before the two new entry points were appended
OLD_SEEDS = {
    (1, 2, 2): (267044625, 1418682806, 1781960455, 291263497), (7, 12, 3): (2104014140, 366281942, 335817057, 2021640045),
    (70, 5, 60): (1999072146, 972872473, 1549840235, 1322966090), (15, 15, 60): (1998373682, 558553731, 51004279, 1793372304),
    (16, 16, 70): (2003618362, 186290001, 1974658586, 1772684625), (6, 5, 91): (792806809, 1976301653, 296080662, 740317324),
    (9, 8, 120): (429022034, 1356161591, 1846834136, 1869176490), (40, 6, 123): (568823607, 115040132, 1571876481, 1673774771),
    (33, 3, 158): (97341019, 366398862, 317038853, 1316310994), (5, 4, 188): (827559881, 871956715, 673099209, 550049996),
}


def _records(ep, plain, row0, mirror):
    out = {(ep, k, kind) for k, kind in plain}
    out |= {(ep, '(c) ' + k, kind) for k in row0 for kind in ('exact', 'relnorm')}         # RefEngine.ROW_BITS: the pattern, and 1e-10
    return out | {(ep, '(d) ' + k, 'exact') for k in mirror}


# every record the two new entry points must have had moved at every geometry: (entry point, label, kind)
NEW_RECORDS = _records('predict_gradcov', [('outputs are those asked for', 'exact'), ('dmu finite pattern', 'exact'), ('dmu', 'relnorm'),
                                           ('dvar finite pattern', 'exact'), ('dvar', 'relnorm'), ('dcov finite pattern', 'exact'),
                                           ('dcov', 'relnorm'), ('asub', 'relnorm'), ('asub is symmetric', 'exact'),
                                           ('dmu is predict_grad\'s', 'exact'), ('dcov is symmetric', 'exact'),
                                           ('dvar is the diagonal of dcov', 'exact'), ('dvar >= 0', 'exact')],
                       PS.ROW_ALONE['predict_gradcov'], PS.F16X3_EQUAL['predict_gradcov']) | \
    _records('predict_pd', [('outputs are those asked for', 'exact'), ('pd', 'relnorm'), ('sd', 'relnorm'), ('cov', 'relnorm'), ('ice', 'relnorm'),
                            ('cov is symmetric', 'exact'), ('diag(cov) against sd^2', 'relnorm'), ('sd >= 0', 'exact')] +
             [('%s of the reversed dimensions and the grid\'s subset' % k, 'relnorm') for k in ('pd', 'sd', 'cov')],
             PS.ROW_ALONE['predict_pd'], PS.F16X3_EQUAL['predict_pd'])


def fp32_gradcov(a, fit):
    """error / fp32 bound of a correct fp32 evaluation of a predict_gradcov step: the product Psi Li^T (and Psi alpha) as
    parity.apply32_model forms it -- fp32 operands, fp32 result -- and everything after it in fp64, against the dense fp64 closed form"""
    ref = PS._ref_engine(fit)
    X, g, cols, width = ref._rows(a['X'], a['mode'])
    T, D = X.shape
    Q, P = GC.basis(fit.params, D, fit.S, fit.M)
    Psi = GC.dphi(X, fit.params, fit.S, fit.M)[:, None, :] * np.concatenate((Q, Q), 0).T[None, :, :]        # T x q x K
    q, K = Psi.shape[1:]
    C = parity.apply32_model(Psi.reshape(T * q, K), np.tril(a['Li']).T).reshape(T, q, K)
    m = parity.apply32_model(Psi.reshape(T * q, K), np.asarray(a['alpha']).reshape(-1, 1)).reshape(T, q) @ P.T
    Sig = PS.kappa(fit.params) * (P @ (C @ C.transpose(0, 2, 1)) @ P.T)
    if g is not None:
        m, Sig = m * g, Sig * g[:, :, None] * g[:, None, :]
    m0, S0 = GC.gradcov(X, a['alpha'], a['Li'], fit.params, fit.S, fit.M, g=g)
    out = dict(dmu=PS.rel(m, m0) / PS.T_GC.BOUNDS_DMU['f32'], dvar=PS.rel(np.diagonal(Sig, axis1=1, axis2=2), np.diagonal(S0, axis1=1, axis2=2)),
               dcov=PS.rel(Sig, S0), asub=PS.rel(GC.asub(m, Sig, a['w']), GC.asub(m0, S0, a['w'])))
    for k in ('dvar', 'dcov', 'asub'):
        out[k] /= PS.T_GC.BOUNDS['f32']
    return {k: v for k, v in out.items() if k in a['want']}


def fp32_pd(a, fit):
    """the same of the sums of a predict_pd step: the mean feature rows Phibar in fp64 (the device sums them in fp64), then Phibar Li^T
    and Phibar alpha as parity.apply32_model forms them, and everything after in fp64"""
    ref = PS._ref_engine(fit)
    X, dims, grid = ref.pd_scaled(a['X'], a['dims'], a['grid'], a['mode'])
    pd0, sd0, cov0, _, Pb = PD.closed(X, a['w'], a['alpha'], a['Li'], fit.params, fit.S, fit.M, dims, grid, want_ice=False)
    kap = PS.kappa(fit.params)
    pd = np.empty_like(pd0); sd = np.empty_like(sd0); cov = np.empty_like(cov0)
    for i in range(len(dims)):
        C = parity.apply32_model(Pb[i], np.tril(a['Li']).T)
        pd[i] = parity.apply32_model(Pb[i], np.asarray(a['alpha']).reshape(-1, 1)).ravel()
        cov[i] = kap * (C @ C.T); sd[i] = np.sqrt(kap * np.sum(C * C, axis=1))
    out = dict(pd=PS.rel(pd, pd0), sd=PS.rel(sd, sd0), cov=PS.rel(cov, cov0))
    return {k: v / PS.T_PD.BOUNDS['f32'] for k, v in out.items() if k in a['want']}


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
        assert len(PS.SWEEP_ENTRY_POINTS) == 19 and len(set(PS.SWEEP_ENTRY_POINTS)) == 19 and not any(st['op'] in ('fail', 'eval', 'rows', 'train', 'option') for st in steps)
        post = [st for st in steps if st['op'] == 'post']
        assert {st['m'] for st in post} == {5} and {st['T'] for st in post} == {1, 37, 257, 300}
        PS.sweep_schedule.cache_clear()
        assert PS.sweep_schedule(*g) == steps                     # a function of the geometry alone
        # the prefix of the seventeen older entry points is what it was: 85 steps, groups 2 .. 40, their seeds
        lo, hi = PS.SWEEP_OLD_GROUPS
        old = [st for st in steps if st['op'] != 'post' or st['group'] <= hi]
        assert old == steps[:85] and {st['ep'] for st in old[4:]} == set(PS.SWEEP_ENTRY_POINTS) - set(NEW)
        assert [st['group'] for st in steps[85:]] == [hi + 1, hi + 1, hi + 2, hi + 2, hi + 3, hi + 3, hi + 4, hi + 4]
        assert (steps[1]['seed'], steps[2]['seed'], steps[4]['seed'], steps[84]['seed']) == OLD_SEEDS[g] and steps[4]['group'] == lo
        assert steps[84]['group'] == hi and steps[84]['ep'] == 'predict' and set(NEW) == {st['ep'] for st in steps[85:]}
        assert all(n <= hi for n in PS._SALT[g]) or {n for n in PS._SALT[g] if n > hi} <= set(range(hi + 1, hi + 5))
    print('steps per geometry: %d, posterior steps: %d' % (info['steps'], info['posterior']))


@pytest.mark.parametrize('g', GEOS, ids=IDS)
def test_dry_run_on_the_references_and_no_check_is_vacuous(g):
    moved = {'bound': {}, 'exact': 0, 'row0': 0, 'mirror': 0, 'conditioned': 0, 'pd sums': 0, 'new': set(), 'new row 0': set(), 'fp32': 0.0}
    refs = {}
    holder = {}

    def on_records(i, a, got, recs):
        # a condition on the inputs: no norm-relative record of a step on row 0 alone is bounded relative to a cancellation
        refs[i] = {rec[0]: rec[3] for rec in recs if rec[1] == 'relnorm'}
        if 'row0_of' in steps[i]:
            for label, ref in refs[i].items():
                if label in refs[steps[i]['row0_of']]:
                    ok = PS.conditioned_row0(ref, refs[steps[i]['row0_of']][label])
                    assert ok is not False, (i, a['ep'], label)
                    moved['conditioned'] += 1
                    if a['ep'] in NEW and ok:
                        moved['new row 0'].add((a['ep'], label))
            if a['ep'] == 'acquire_kg' and a['T'] == 257 and not (g[0] == 1 and a['R'] == 37):
                assert PS.kg_conditioning(a, holder['run'].fit) <= 1.0, (i, PS.kg_conditioning(a, holder['run'].fit))
            if a['ep'] == 'acquire' and 'grad' in a['want']:
                c = PS.acquire_grad_cancellation(a, holder['run'].fit)
                assert c <= PS.GRAD_CANCEL, (i, a['kind'], c)
        if a['ep'] == 'predict_pd' and set(a['want']) - {'ice'}:
            c = PS.pd_cancellation(a, holder['run'].fit)
            assert c >= PS.PD_CANCEL, (i, c)
            moved['pd sums'] += 1
        # a correct fp32 evaluation of every step of the two new entry points, the steps on row 0 alone included, stays inside half the
        # fp32 bound: their salts are the first for which it does
        if a['ep'] in NEW:
            r32 = (fp32_gradcov if a['ep'] == 'predict_gradcov' else fp32_pd)(a, holder['run'].fit)
            assert r32 and max(r32.values()) <= 0.5, (i, a['ep'], a['T'], r32)
            moved['fp32'] = max(moved['fp32'], max(r32.values()))
        for rec in recs:
            PS.evaluate(rec)
            bad = PS.perturbed(rec)
            if bad is None:
                assert a['ep'] not in NEW, (a['ep'], rec[0])           # every record of the new entry points has something to move
                continue
            with pytest.raises(AssertionError):
                PS.evaluate(bad)
            if a['ep'] in NEW:
                moved['new'].add((a['ep'], rec[0].split(' of row 0')[0].split(' of the f16x3')[0], rec[1]))
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
    # every one of the nineteen entry points had a bounded record moved at this geometry
    assert set(moved['bound']) == set(PS.SWEEP_ENTRY_POINTS), sorted(set(PS.SWEEP_ENTRY_POINTS) - set(moved['bound']))
    assert len(run.min_pivot2) == 2 and min(run.min_pivot2) >= 0.25
    # the new entry points: every record of PS.records, of (c) and of (d) was moved, and every row-aligned record of their steps on row 0
    # alone met conditioned_row0 (asub, pd, sd and cov are sums over the rows and not row-aligned)
    assert moved['pd sums'] == 4                                   # every predict_pd step of the sweep asks for a sum
    assert moved['new'] >= NEW_RECORDS, sorted(NEW_RECORDS - moved['new'])
    assert moved['new row 0'] == {('predict_gradcov', 'dmu'), ('predict_gradcov', 'dvar'), ('predict_gradcov', 'dcov'), ('predict_pd', 'ice')}
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


@pytest.mark.parametrize('g', GEOS, ids=IDS)
def test_a_correct_fp32_gradcov_and_pd_stay_inside_half_the_fp32_bound(g):
    """the first predict_gradcov step and the first predict_pd step of the sweep schedule (257 rows, every output), on the fit as
    condition and forget have left it: parity.apply32_model of Psi Li^T and of Phibar Li^T, everything after in fp64, against the fp64
    closed forms under the bounds imported from the own GPU tests.  A condition on the choice of inputs, not a tolerance."""
    D, S, M = g
    steps = PS.sweep_schedule(*g)
    fit = PS.Fit(D, S, M)
    fit.xs = PS.x_scaler(steps[0]['algo'], D); fit.ys = PS.y_scaler(steps[3]['algo'])
    fit.params = PS.new_params(np.random.default_rng(steps[1]['seed']), D, S, M)
    rng = np.random.default_rng(steps[2]['seed'])
    fit.Xraw = PS.raw_rows(rng, steps[2]['N'], D); fit.yraw = PS.raw_targets(rng, fit.Xraw)
    # the rows condition and forget move, replayed on the CPU model of the fit
    for st in steps:
        if st['op'] == 'post' and st['ep'] in ('condition', 'forget'):
            a = PS.materialise(st, fit)
            if st['ep'] == 'condition':
                fit.Xraw = np.vstack([fit.Xraw, a['Xraw']]); fit.yraw = np.vstack([fit.yraw, a['yraw']])
            else:
                keep = np.setdiff1d(np.arange(fit.Xraw.shape[0]), a['rows'])
                fit.Xraw, fit.yraw = fit.Xraw[keep], fit.yraw[keep]
            fit.touch()
    assert fit.Xraw.shape[0] == PS.SWEEP_N
    for ep, model in (('predict_gradcov', fp32_gradcov), ('predict_pd', fp32_pd)):
        st = next(s for s in steps if s['op'] == 'post' and s['ep'] == ep)
        a = PS.materialise(st, fit)
        assert a['X'].shape[0] == 257 and st['flag'] and a['w'] is not None
        r = model(a, fit)
        print('%s: a correct fp32 %s stands at %s of the fp32 bound' % (g, ep, ' '.join('%s %.3f' % kv for kv in r.items())))
        assert set(r) == set(a['want']) - {'ice'} and max(r.values()) <= 0.5, r
