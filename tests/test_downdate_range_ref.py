"""CPU tier of the near-singular range tests of scfgp_loo, scfgp_forget and scfgp_condition (tests/downdate_range.py): the fixture's
coverage conditions, the numpy restatements against its mpmath truths under 4 x C_REF, a dry run of every check of the GPU tier with the
restatements standing in for the device, and mutants of the restatements that the new bound (8 x C_REF) must catch -- beside the verdict
of today's fixed bound (tests/parity.py: TOL['f64']) on the mild case, which several of them pass.  Needs no GPU and no mpmath."""
import functools
import os

import numpy as np
import pytest

from tests import downdate_range as R
from tests import forget_ref
from tests import parity

FX = R.Fixture()
CREF = FX.cref()

# lam_min(S) of the forget cases and min (1 - lam_max) of the K = 128 loo cases as the case table was drawn up
LAM_MIN = [0.20, 6.6e-4, 1.5e-5, 8.2e-8, 9.2e-9, 1.2e-9, 2.3e-11, 4.2e-5, 1.9e-8, 2.2e-9]
DROPPED = [('k64_n62_a7b3', 64), ('k64_n32_a7b3', 64)]


@functools.lru_cache(maxsize=None)
def _ratios():
    return R.all_ratios(FX)


def test_coverage_conditions():
    # lower triangles only, packed; the case table's triangles are incompressible doubles, so the files cannot be smaller than they are
    # (tests/downdate_range.py has the count: 388 KB of inputs, 371 KB of Li' and 371 KB of A' truths) -- everything else (rows, loo truths and models, alpha, the recorded constants) is < 300 KB
    assert all(FX[k].ndim == 1 for k in FX.d.files if k.endswith('/Li')) and all(FX.a[k].ndim == 1 for k in FX.a.files)
    tri = lambda f, end: 8 * sum(f[k].size for k in f.files if k.endswith(end))
    print('bytes: %s %d (Li triangles %d), %s %d (A triangles %d)' % (os.path.basename(R.FIXTURE), os.path.getsize(R.FIXTURE), tri(FX.d, '/Li'),
                                                                     os.path.basename(R.RESID_FIXTURE), os.path.getsize(R.RESID_FIXTURE), tri(FX.a, '/A')))
    assert os.path.getsize(R.FIXTURE) - tri(FX.d, '/Li') < 300 * 1024 and os.path.getsize(R.RESID_FIXTURE) < 400 * 1024
    assert os.path.getsize(R.FIXTURE) < 2 ** 20
    assert sorted(FX.a.files) == sorted([R.fkey(*c) + '/A' for c in R.FORGET_CASES] + [R.ckey(*c) + '/A' for c in R.COND_CASES])
    cases = [(f, b) for f, bs in R.LOO_CASES for b in bs]
    assert [c for c in cases if not FX.admitted(*c)] == DROPPED
    margins = [float(FX[R.lkey(*c) + '/margin']) for c in cases if FX.admitted(*c)]
    gaps = [float(FX[R.lkey(*c) + '/gap'].min()) for c in cases if FX.admitted(*c)]
    print('admitted loo cases %d, tightest margin %.3g, smallest 1 - lam_max %.3g' % (len(margins), min(margins), min(gaps)))
    assert min(margins) >= R.ADMIT and min(gaps) <= 1e-7
    assert abs(FX[R.lkey('k128_n64_a7', 8) + '/gap'].min() / 5.4e-4 - 1) < 0.05 and abs(FX[R.lkey('k128_n64_a7', 64) + '/gap'].min() / 2.5e-8 - 1) < 0.05
    # block 7 at N = 62: eight full blocks and a ragged one of 6
    assert FX[R.lkey('k64_n62_a7', 7) + '/gap'].size == 9
    for (fit, keep), lam in zip(R.FORGET_CASES, LAM_MIN):
        assert abs(float(FX[R.fkey(fit, keep) + '/lam_min']) / lam - 1) < 0.05, (fit, keep)
    assert {2 * (R.FITS[f][1] + R.FITS[f][2]) for f, _ in R.FORGET_CASES} == {40, 64, 128}
    for fit, n in R.COND_CASES:
        print(R.ckey(fit, n), 'lam_min %.3g lam_max %.3g' % (float(FX[R.ckey(fit, n) + '/lam_min']), float(FX[R.ckey(fit, n) + '/lam_max'])))
    assert max(float(FX[R.ckey(f, n) + '/lam_max']) for f, n in R.COND_CASES) > 1e10
    kh = FX['boundary/copies'] * FX['boundary/h']
    print('boundary k h', kh)
    assert kh[0] < 1.0 < kh[1] and abs(float(FX['boundary/lam_min']) - (1.0 - kh[0])) < 1e-12


def test_the_inputs_are_the_generators():
    """rows, targets and parameters regenerate (to libm's last bits); alpha and Li are stored because LAPACK differs between machines"""
    for k, v in R.make_inputs().items():
        assert np.allclose(FX[k], v, rtol=1e-13, atol=1e-15), k


def test_c_ref_is_the_maximum_of_the_recorded_constants():
    for kind in R.KINDS + R.PRINTED:
        rec = [float(FX[k]) for k in FX.d.files if k.startswith('ref/') and k.endswith('/' + kind)]
        assert rec and max(rec) == CREF[kind]
    print('C_REF', ' '.join('%s=%.3g' % kv for kv in sorted(CREF.items())))
    spread = {}
    for name, kinds in (('simple', ('loo_musd',)), ('component-wise', R.PRINTED)):
        per_case = [max(float(FX['ref/%s/%s' % (R.lkey(f, b), k)]) for k in kinds) for f, bs in R.LOO_CASES for b in bs if FX.admitted(f, b)]
        print('loo model %-14s spread of the restatement\'s constant over %d cases: %.3g .. %.3g (x %.0f)'
              % (name, len(per_case), min(per_case), max(per_case), max(per_case) / min(per_case)))
        spread[name] = max(per_case) / min(per_case)
    assert spread['simple'] < spread['component-wise']                  # the asserted model is the one with the narrower spread


def test_restatements_reproduce_the_recorded_errors():
    """on any machine's LAPACK and libm: every constant within 4 x C_REF.  This is also the dry run of the GPU tier's fp64 checks."""
    r = _ratios()
    print('worst here', R.fmt(R.worst(r)))
    bad = R.failures(r, CREF, R.REF_FACTOR)
    assert not bad, bad
    assert len(r) == len(R.FORGET_CASES) + len(R.COND_CASES) + len(R.PIVOT_CASES) + 1 + 20
    # the fixture round-trips: every recorded per-case constant is met again from the inputs and the restatement.  Loosely, since LAPACK
    # and libm differ between machines: within 3 x the recorded value or a quarter of the kind's C_REF
    r32 = R.cond32_reference(FX)
    n = 0
    for k in FX.d.files:
        if k.startswith('ref/'):
            key, kind = k[4:].rsplit('/', 1)
            new = r32[key][kind] if kind.startswith('cond32') else r[key][kind]
            rec = float(FX[k])
            assert abs(new - rec) <= max(3.0 * rec, 0.25 * CREF[kind]), (k, new, rec)
            n += 1
    assert n == sum(len(v) for v in r.values()) + sum(len(v) for v in r32.values())


def test_dry_run_of_the_fp32_loo_tier():
    """the loo restatement with the C an fp32 context holds, eps32 in the model, on the cases admitted with u = 2^-24"""
    n = 0
    bad = []
    for fit, blocks in R.LOO_CASES:
        for block in blocks:
            if FX.admitted(fit, block, R.U32):
                o = R.restate_loo(FX, fit, block, mutant='apply32')
                r = R.loo_ratios(FX, fit, block, o['mu'], o['std'], o['lev'], float(np.sum(o['joint'])), R.U32)
                print(R.lkey(fit, block), ' '.join('%s=%.3g' % kv for kv in r.items()))
                bad += R.failures({R.lkey(fit, block): r}, CREF, R.DEV_FACTOR)
                n += 1
    assert n >= 3 and not bad, bad


def test_dry_run_of_the_boundary_checks():
    D, S, M, N, params, X, y, alpha, Li = FX.fit(R.BOUNDARY_FIT)
    rows, ks, h = FX['boundary/rows'], FX['boundary/copies'], FX['boundary/h']
    i, k = int(rows[0]), int(ks[0])
    r = _ratios()['boundary']
    print('below: 1 - k h %.3e' % float(FX['boundary/lam_min']), r)
    assert not R.failures({'boundary': r}, CREF, R.REF_FACTOR)
    lo = R.loo_np(np.repeat(X[i:i + 1], k, 0), np.repeat(y[i:i + 1], k), alpha, Li, params, S, M, k)
    assert np.isfinite(lo['mu']).all() and np.isfinite(lo['std']).all()
    i, k = int(rows[1]), int(ks[1])
    with pytest.raises(np.linalg.LinAlgError):
        forget_ref.forget(np.repeat(X[i:i + 1], k, 0), np.repeat(y[i:i + 1], k), alpha, Li, params, S, M)
    with pytest.raises(np.linalg.LinAlgError):
        R.loo_np(np.repeat(X[i:i + 1], k, 0), np.repeat(y[i:i + 1], k), alpha, Li, params, S, M, k)


def _todays_bound(mutant):
    """does the mutant pass today's fixed fp64 bound (tests/parity.py: TOL['f64']) on the mild cases, against the same truths"""
    fit, keep = R.MILD_FORGET
    o = R.restate_forget(FX, fit, keep, mutant)
    key = R.fkey(fit, keep)
    r = [parity.alpha_ratio(o['alpha'], FX[key + '/alpha'], 'f64'), parity.li_ratio(o['Li'], R.unpack(FX[key + '/Li']), 'f64')]
    lo = R.restate_loo(FX, fit, 8, mutant if mutant in ('c32', 'r32') else None)
    r.append(parity.predict_ratio(lo['mu'], lo['std'], FX[R.lkey(fit, 8) + '/mu'], FX[R.lkey(fit, 8) + '/std'], 'f64'))
    return max(r)


def _or_nan(f):
    """a mutant whose factorisation breaks down has failed every check of its case: NaN constants"""
    def g(fx, *case, **kw):
        try:
            return f(fx, *case, **kw)
        except np.linalg.LinAlgError:
            D, S, M, N = R.FITS[case[0]][:4]
            K = 2 * (S + M)
            nan = np.nan
            return dict(alpha=np.full((K, 1), nan), Li=np.full((K, K), nan), pivot2=nan, joint=np.full(1, nan), mu=np.full(N, nan),
                        std=np.full(N, nan), lev=np.full(N, nan))
    return g


def test_mutants_fail_the_new_bound_and_some_pass_todays():
    mild = {R.fkey(*R.MILD_FORGET)} | {R.lkey(R.MILD_FORGET[0], b) for b in R.LOO_BLOCKS} | {R.ckey(*R.COND_CASES[-1])}
    passes_today = {}
    for m in R.MUTANTS:
        loo_m = m if m in ('c32', 'r32') else None
        r = R.all_ratios(FX, forget=functools.partial(_or_nan(R.restate_forget), mutant=m),
                         cond=functools.partial(_or_nan(R.restate_cond), mutant=m),
                         pivot=functools.partial(_or_nan(R.restate_pivot), mutant=m), loo=functools.partial(_or_nan(R.restate_loo), mutant=loo_m))
        bad = R.failures(r, CREF, R.DEV_FACTOR)
        hard = [b for b in bad if b.split()[0] not in mild]
        today = _todays_bound(m)
        passes_today[m] = today <= 1.0
        print('mutant %-13s fails the new bound in %d checks (%d on near-singular cases), worst %s; today\'s bound on the mild case: ratio '
              '%.3g (%s)' % (m, len(bad), len(hard), R.fmt(R.worst(r)), today, 'passes' if today <= 1.0 else 'fails'))
        # a relative error of 1e-12 in one pivot lies below the honest rounding error wherever lam_min(S) < 1e-4: the well-conditioned
        # cases, where the new bound is 1e6 times tighter than today's, are the ones that see it
        assert (bad if m == 'pivot_1e12' else hard), 'mutant %s passes the new bound on every %scase' % (m, '' if m == 'pivot_1e12' else 'near-singular ')
        if m == 'li_small_row':
            # the residual is what sees it at the hard end: the tile-wise norm of D Li' is relative to rows 1e4 times as long
            h = r[R.fkey(*R.HARD_FORGET)]
            print('li_small_row at lam_min = 9.2e-9: forget_Li %.3g (allowed %.3g), forget_resid %.3g (allowed %.3g)'
                  % (h['forget_Li'], R.DEV_FACTOR * CREF['forget_Li'], h['forget_resid'], R.DEV_FACTOR * CREF['forget_resid']))
            assert h['forget_Li'] <= R.DEV_FACTOR * CREF['forget_Li'] and h['forget_resid'] > R.DEV_FACTOR * CREF['forget_resid']
    # the gap this tier closes: mutants that today's fixed bound lets through
    print('pass today\'s fixed bound on the mild case:', [m for m, ok in passes_today.items() if ok])
    assert sum(passes_today.values()) >= 2, passes_today


def test_the_unmutated_variant_is_the_restatement():
    """tests/downdate_range.update_np without a mutant meets the same bound as tests/forget_ref.py and tests/condition_ref.py"""
    r = {}
    for fit, keep in R.FORGET_CASES:
        D, S, M, N, params, X, y, alpha, Li = FX.fit(fit)
        o = R.update_np(X[keep:], y[keep:], alpha, Li, params, S, M, -1.0)
        r[R.fkey(fit, keep)] = R.forget_ratios(FX, fit, keep, o['alpha'], o['Li'], o['pivot2'], o['joint'])
    bad = R.failures(r, CREF, R.REF_FACTOR)
    assert not bad, bad
