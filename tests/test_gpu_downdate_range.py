"""GPU tier of the near-singular range tests of scfgp_loo, scfgp_forget and scfgp_condition: the device on the fixture's inputs
(tests/golden/downdate_kats.npz and downdate_resid_kats.npz: doubles in, 60-digit mpmath truths out) under the conditioning-aware models of tests/downdate_range.py.
Every constant `error / (u model)` is printed; the device is allowed 8 x C_REF[kind], C_REF being the numpy restatement's worst constant
against the same truths (measured by the generator, held to 4 x by tests/test_downdate_range_ref.py).  Reads only the fixture and
tests/downdate_range.py; no mpmath, no oracle fit.

  forget               fp64 in every context (first pass and K x K stage), so f32 contexts are held to the fp64 bound on the factors
  condition            the K x K stage is fp64, C^T C runs in the context's precision: fp64 contexts under the fp64 bound; fp32 contexts
                       with eps32 in the model where eps32 K |S| stays 1e4 below lam_min(S) (the mild case), else as loo below
  loo, fp64 contexts   every admitted case and block: mu / std per row against sigma / (1 - lam_max), leverage, summed joint density
  loo, fp32 contexts   C runs in fp32: eps32 in the model, and only the cases the admission rule passes with u = 2^-24; for the others a
                       return of 0 comes with finite outputs and a failure is SCFGP_ENOTPD with stats untouched
  bit-level claims     a loo block's rows do not depend on its position or on n (the near-singular block first and last in a 64-row
                       group against a call on it alone); stats[5] = max(lev); forget's mu / std = predict with the returned factors;
                       f16x3 forget = fp32 forget on the lam_min = 9.2e-9 case
  last pivot           k copies of one row, chosen so that the LAST pivot of the Cholesky of S is the smallest: stats[5] must hold it
  ENOTPD boundary      k copies of a fit row of leverage h: S = I - k c c^T has the eigenvalue 1 - k h.  k h = 0.9972 succeeds with
                       min M_ii^2 at the truth (1 - k h is the PRODUCT of the pivots, not their minimum); k h = 1.0004 returns
                       SCFGP_ENOTPD with the outputs untouched (loo, the copies as one block: the message names block 0)

"""
import numpy as np
import pytest

from tests import downdate_range as R

pytestmark = pytest.mark.gpu

FX = R.Fixture()
CREF = FX.cref()
# fp64 contexts: the admitted cases; fp32 contexts: all of them, judged by the model only where eps32 admits them
LOO_PARAMS = [(fit, block, dtype) for dtype in ('f64', 'f32') for fit, blocks in R.LOO_CASES for block in blocks
              if dtype == 'f32' or FX.admitted(fit, block)]


def _engine(fit, dtype):
    from scfgp_amd.engine import HipEngine
    D, S, M = R.FITS[fit][:3]
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(FX['fit/%s/params' % fit])
    return eng


def _bits(a, b):
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _judge(tag, ratios, factor=R.DEV_FACTOR):
    print(tag, ' '.join('%s=%.3g' % kv for kv in ratios.items()))
    return ['%s %s: %.3g > %g x %.3g' % (tag, k, v, factor, CREF[k]) for k, v in ratios.items() if k in CREF and not v <= factor * CREF[k]]


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('fit,keep', R.FORGET_CASES)
def test_forget_against_the_truth(fit, keep, dtype):
    D, S, M, N, params, X, y, alpha, Li = FX.fit(fit)
    eng = _engine(fit, dtype)
    al, Ln, mu, sd, st = eng.forget(X[keep:], y[keep:], alpha, Li, factors=True, predict=True)
    bad = _judge('%s %s' % (R.fkey(fit, keep), dtype), R.forget_ratios(FX, fit, keep, al, Ln, st['min_pivot2'], st['log_joint']))
    if not np.all(np.triu(Ln, 1) == 0.0):
        bad.append('entries above the diagonal of Li')
    mu2, sd2 = eng.predict(X[keep:], al, Ln)
    if not (_bits(mu, mu2) and _bits(sd, sd2)):
        bad.append('mu / std are not predict with the returned factors')
    eng.close()
    assert not bad, bad


def test_forget_f16x3_equals_fp32_at_the_hard_case():
    fit, keep = R.HARD_FORGET
    D, S, M, N, params, X, y, alpha, Li = FX.fit(fit)
    out = []
    for dtype in ('f32', 'f16x3'):
        eng = _engine(fit, dtype)
        out.append(eng.forget(X[keep:], y[keep:], alpha, Li, factors=True, predict=True))
        eng.close()
    assert all(_bits(u, v) for u, v in zip(out[0][:4], out[1][:4]))
    assert all(_bits(out[0][4][k], out[1][4][k]) for k in out[0][4]) and out[0][4].keys() == out[1][4].keys()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('fit,n', R.COND_CASES)
def test_condition_against_the_truth(fit, n, dtype):
    """fp32 contexts form C^T C in fp32 (include/scfgp_hip.h): eps32 in the model, for the cases that rule admits; for the others a
    return of 0 comes with finite factors, judged in units of eps32 cond(S) against the restatement with fp32 products, and a failure
    is SCFGP_ENOTPD with the outputs untouched"""
    from scfgp_amd._lib import dptr
    D, S, M, N, params, X, y, alpha, Li = FX.fit(fit)
    Xn, yn = FX.rows(fit, N, N + n)
    eng = _engine(fit, dtype)
    a = np.ascontiguousarray(alpha).ravel(); L = np.ascontiguousarray(Li)
    al = np.full(a.size, 3.0); Ln = np.full(L.shape, 3.0)
    rc = eng.lib.scfgp_condition(eng.ctx, dptr(Xn), dptr(yn), n, dptr(a), dptr(L), 0, dptr(al), dptr(Ln))
    tag = '%s %s' % (R.ckey(fit, n), dtype)
    bad = []
    if dtype == 'f64' or R.cond_admitted_f32(FX, fit, n):
        assert rc == 0, (rc, eng.last_error())
        bad += _judge(tag, R.cond_ratios(FX, fit, n, al, Ln, R.U64 if dtype == 'f64' else R.U32))
    elif rc == 0:
        if not (np.isfinite(al).all() and np.isfinite(Ln).all()):
            bad.append('a return of 0 with non-finite factors')
    else:
        print(tag, 'not admitted at eps32, returned %d: %s' % (rc, eng.last_error()))
        if rc != -3 or not (np.all(al == 3.0) and np.all(Ln == 3.0)):
            bad.append('a failure other than SCFGP_ENOTPD with the outputs untouched: %d' % rc)
    if rc == 0 and dtype == 'f32':
        # every fp32 case that returns 0, admitted or not: in units of eps32 cond(S), within 8 x what the restatement with fp32 products
        # gave for THIS case (the three cases span six decades of that unit, so their maximum would bound nothing)
        r = R.cond32_ratios(FX, fit, n, al, Ln)
        ref = dict((k, float(FX['ref/%s/%s' % (R.ckey(fit, n), k)])) for k in r)
        print(tag, ' '.join('%s=%.3g (ref %.3g)' % (k, v, ref[k]) for k, v in r.items()))
        bad += ['%s %s: %.3g > %g x %.3g' % (tag, k, v, R.DEV_FACTOR, ref[k]) for k, v in r.items() if not v <= R.DEV_FACTOR * ref[k]]
    if rc == 0 and not np.all(np.triu(Ln, 1) == 0.0):
        bad.append('entries above the diagonal of Li')
    eng.close()
    assert not bad, bad


def _loo_call(eng, X, y, alpha, Li, block):
    """(rc, mu, std, lev, stats) of the library call itself, stats pre-filled with 3.0"""
    from scfgp_amd._lib import dptr
    X = np.ascontiguousarray(X, np.float64); y = np.ascontiguousarray(y, np.float64).ravel()
    a = np.ascontiguousarray(alpha, np.float64).ravel(); L = np.ascontiguousarray(Li, np.float64)
    n = X.shape[0]
    mu = np.empty(n); sd = np.empty(n); lev = np.empty(n); stats = np.full(8, 3.0)
    rc = eng.lib.scfgp_loo(eng.ctx, dptr(X), dptr(y), n, dptr(a), dptr(L), 0, int(block), dptr(mu), dptr(sd), dptr(lev), dptr(stats))
    return rc, mu, sd, lev, stats


def _placements(n, block, j):
    """(rows of block j, [(rows of a call, where the block starts in it)]): the block first in a call, and last in the call's first 64-row
    group behind copies of another block; a ragged block can only come last"""
    me = np.arange(j * block, min(n, (j + 1) * block))
    k0 = 0 if j != 0 else block
    g = 64 // block
    if k0 + block > n or g < 2:
        return me, []
    fill = [np.arange(k0, k0 + block)] * (g - 1)
    out = [(np.concatenate(fill + [me]), (g - 1) * block)]
    if me.size == block:
        out.append((np.concatenate([me] + fill), 0))
    return me, out


@pytest.mark.parametrize('fit,block,dtype', LOO_PARAMS)
def test_loo_against_the_truth(fit, block, dtype):
    D, S, M, N, params, X, y, alpha, Li = FX.fit(fit)
    u = R.U64 if dtype == 'f64' else R.U32
    admitted = FX.admitted(fit, block, u)
    key = R.lkey(fit, block)
    eng = _engine(fit, dtype)
    rc, mu, sd, lev, stats = _loo_call(eng, X, y, alpha, Li, block)
    bad = []
    if admitted:
        assert rc == 0, (rc, eng.last_error())
        bad += _judge('%s %s' % (key, dtype), R.loo_ratios(FX, fit, block, mu, sd, lev, stats[4], u))
    elif rc == 0:
        print('%s %s: not admitted at eps32, returned 0' % (key, dtype),
              ' '.join('%s=%.3g' % kv for kv in R.loo_ratios(FX, fit, block, mu, sd, lev, stats[4], u).items()))
        if not (np.isfinite(mu).all() and np.isfinite(sd).all() and np.isfinite(lev).all() and np.isfinite(stats).all()):
            bad.append('a return of 0 with non-finite outputs')
    else:
        print('%s %s: not admitted at eps32, returned %d: %s' % (key, dtype, rc, eng.last_error()))
        if rc != -3 or not np.all(stats == 3.0):
            bad.append('a failure other than SCFGP_ENOTPD with stats untouched: %d %s' % (rc, stats))
    if rc == 0:
        if not _bits(stats[5], np.max(lev)):
            bad.append('stats[5] %r is not max(lev) %r' % (stats[5], np.max(lev)))
        # the near-singular block alone, and first / last in a 64-row group
        j = int(np.argmin(FX[key + '/gap']))
        me, placed = _placements(N, block, j)
        rc1, mu1, sd1, lev1, _ = _loo_call(eng, X[me], y[me], alpha, Li, block)
        if rc1 != 0 or not (_bits(mu1, mu[me]) and _bits(sd1, sd[me]) and _bits(lev1, lev[me])):
            bad.append('block %d alone differs from the block within the call' % j)
        for rows, at in placed:
            rc2, mu2, sd2, lev2, _ = _loo_call(eng, X[rows], y[rows], alpha, Li, block)
            s = slice(at, at + me.size)
            if rc2 != 0 or not (_bits(mu2[s], mu1) and _bits(sd2[s], sd1) and _bits(lev2[s], lev1)):
                bad.append('block %d at row %d of a call differs from the block alone' % (j, at))
    eng.close()
    assert not bad, bad


def _copies(fit, i, k):
    D, S, M, N, params, X, y, alpha, Li = FX.fit(fit)
    return np.repeat(X[i:i + 1], k, axis=0), np.repeat(y[i:i + 1], k), alpha, Li


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('fit,row,k', R.PIVOT_CASES)
def test_forget_where_the_last_pivot_is_the_smallest(fit, row, k, dtype):
    eng = _engine(fit, dtype)
    Xo, yo, alpha, Li = _copies(fit, row, k)
    al, Ln, mu, sd, st = eng.forget(Xo, yo, alpha, Li, factors=True, predict=True)
    bad = _judge('%s %s' % (R.pkey(fit, row, k), dtype), R.pivot_ratios(FX, fit, row, k, al, st['min_pivot2'], st['log_joint']))
    eng.close()
    assert not bad, bad


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_forget_at_the_enotpd_boundary(dtype):
    from scfgp_amd._lib import dptr
    rows, ks, h = FX['boundary/rows'], FX['boundary/copies'], FX['boundary/h']
    assert ks[0] * h[0] < 1.0 < ks[1] * h[1]
    eng = _engine(R.BOUNDARY_FIT, dtype)
    fit, row, k = R.boundary_case(FX)
    Xo, yo, alpha, Li = _copies(fit, row, k)
    al, Ln, mu, sd, st = eng.forget(Xo, yo, alpha, Li, factors=True, predict=True)
    print('%d copies of row %d, 1 - k h = %.3e: min M_ii^2 %.17g (truth %.17g)' % (k, row, float(FX['boundary/lam_min']), st['min_pivot2'],
                                                                                  float(FX['boundary/pivot2'])))
    bad = _judge('boundary %s' % dtype, R.pivot_ratios(FX, fit, row, k, al, st['min_pivot2'], st['log_joint'], key='boundary'))
    assert not bad and 0.0 < st['min_pivot2'] < 1.0, bad
    row, k = int(rows[1]), int(ks[1])
    Xo, yo, alpha, Li = _copies(fit, row, k)
    a = np.ascontiguousarray(alpha).ravel(); L = np.ascontiguousarray(Li); Xo = np.ascontiguousarray(Xo); yo = np.ascontiguousarray(yo)
    outs = [np.full(a.size, 3.0), np.full(L.shape, 3.0), np.full(k, 3.0), np.full(k, 3.0), np.full(8, 3.0)]
    rc = eng.lib.scfgp_forget(eng.ctx, dptr(Xo), dptr(yo), k, dptr(a), dptr(L), 0, *[dptr(v) for v in outs])
    print('%d copies of row %d, 1 - k h = %.3e (%s): rc %d: %s' % (k, row, 1.0 - k * h[1], dtype, rc, eng.last_error()))
    assert rc == -3 and 'not in this fit' in eng.last_error()
    assert all(np.all(o == 3.0) for o in outs)
    with pytest.raises(np.linalg.LinAlgError):
        eng.forget(Xo, yo, alpha, Li)
    eng.close()


def test_loo_at_the_enotpd_boundary():
    """the same copies as one loo block: I - H = I - h 1 1^T"""
    rows, ks, h = FX['boundary/rows'], FX['boundary/copies'], FX['boundary/h']
    eng = _engine(R.BOUNDARY_FIT, 'f64')
    fit, row, k = R.boundary_case(FX)
    Xo, yo, alpha, Li = _copies(fit, row, k)
    rc, mu, sd, lev, stats = _loo_call(eng, Xo, yo, alpha, Li, k)
    print('loo, %d copies below the boundary: rc %d lev %s std %s' % (k, rc, lev, sd))
    assert rc == 0 and np.isfinite(mu).all() and np.isfinite(sd).all() and stats[0] == k and stats[6] == 1
    assert np.all(np.abs(lev - h[0]) <= R.DEV_FACTOR * CREF['loo_lev'] * R.U64 * FX['lev/%s/den_lev' % fit][row])
    row, k = int(rows[1]), int(ks[1])
    Xo, yo, alpha, Li = _copies(fit, row, k)
    rc, mu, sd, lev, stats = _loo_call(eng, Xo, yo, alpha, Li, k)
    print('loo, %d copies above the boundary: rc %d: %s' % (k, rc, eng.last_error()))
    assert rc == -3 and 'block 0 ' in eng.last_error() and np.all(stats == 3.0)
    eng.close()
