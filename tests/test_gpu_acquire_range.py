"""GPU tier of the acquisition range tests: the normal-tail arithmetic of scfgp_acquire (acquire_math.h, acquire.hip: acquire_value<KIND>,
acquire_mes_kernel) and of scfgp_acquire_kg (kg.hip: kg_ref_kernel, kg_finish_kernel through norm_h) per row, at chosen g.
tests/acquire_range.py has the error models, the constants C_REF of the numpy restatement against mpmath (measured and asserted by
tests/test_acquire_range_ref.py) and the construction of the inputs; the device is allowed 8 x C_REF in the same measure.

  exact g          alpha = 0 makes u = +-0, so g = fl(-sgn best / sigma) (MES, n* = 1: fl(sgn f* / sigma)) with sigma read back from the device
                   and the incumbent chosen on the host: the seam doubles -1.0 and -50.0 with their neighbours, -38 .. -39, -10^x, 0, 8.3,
                   38, each verified bit for bit with the device's own expression; the value against the mpmath fixture
                   tests/golden/acquire_kats.npz
  dense sweeps     alpha = scale alpha0 and the incumbent (f*) put at least 4 rows in every unit interval of g in [-60, 8] (MES [-60, 40]);
                   a ladder of rows puts log-EI's g in every decade down to -1e7; value and gradient per row against the restatement at
                   the device's own mu, sigma, the gradient chained with predict_grad's d mu, d sigma -- never a norm over the block
  EI gone          every EI exactly 0: the lowest eligible row wins with val 0.0; log-EI on the same arguments still ranks the pool
  KG, two lines    R = 2: kg against the closed form |b1 - b2| h(-c) per row where the crossing lies inside the nodes, exactly 0 where
                   it lies outside, kg_hi never below it; c from 0 to beyond the last node
Every input condition (which g are met, how many rows per interval of g or c) is computed from the device's own mu, sigma and lines and
asserted before anything is compared; the CPU tier runs the same conditions on the oracle's features.  No mpmath is needed here.

The whole file makes about 500 calls of at most 4096 rows and runs in a few seconds.

Measured on the device (MI355X), worst constant in the model's unit over dtypes, directions and both sigmas, beside the C_REF it is
judged against (allowed: 8 x C_REF):
  exact g, value       pi 0.39 (C_REF 1.9), ei 1.44 (2.7), logei 6.66 (4.5), mes 2.20 (1.9)
  sweeps, value        pi 1.80 (1.9), ei 3.09 (2.7), logei 10.92 (4.5; on the ladder 8.86), mes 5.51 (1.9)
  sweeps, gradient     worst |delta| / allowed over rows and columns: pi 0.17, ei 0.13, logei 0.22 (ladder 0.18), mes 0.25
  KG, two lines        0.24 (C_REF_KG 1.6)
No row failed: the seams at g = -1 and g = -50, the series below -50, the tail partials and the MES g >= 0 form agree with the restatement
within the allowance, so no kernel was changed.
"""
import os

import numpy as np
import pytest

from tests import acquire_range as AR
from tests import acquire_ref as A
from tests import kg_ref as G

pytestmark = pytest.mark.gpu

KATS = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'acquire_kats.npz'))
D, S, M = AR.SHAPE
KK = 2 * (S + M)
PARAMS, ALPHA0, LI = AR.synthetic_factors(D, S, M)
SEAM_G = np.concatenate([AR.around(s) for s in AR.SEAMS])


def _engine(dtype):
    from scfgp_amd.engine import HipEngine
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(PARAMS)
    return eng


def _bits(a, b):
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _sgn(minimize):
    return -1.0 if minimize else 1.0


# ---- 1. exact g ------------------------------------------------------------------------------------------------------------------------
def _fixture_truth(kind, j, sd):
    """the true value of the row from the fixture's entry j and the row's sigma"""
    if kind == 'pi':
        return float(KATS['Phi'][j])
    if kind == 'ei':
        return float(sd * KATS['h'][j])
    if kind == 'logei':
        return float(np.log(sd) + KATS['log_h'][j])
    return float(KATS['mes_term'][j])


# full: every fixture g; seams: the ten doubles around -1.0 and -50.0, for the kinds that branch there
@pytest.mark.parametrize('dtype,minimize,noise,points', [('f64', False, False, 'full'), ('f64', True, True, 'full'), ('f64', True, False, 'seams'),
                                                         ('f32', False, True, 'seams')])
def test_exact_g_against_the_fixture(dtype, minimize, noise, points):
    eng = _engine(dtype)
    Xs = AR.exact_pool()
    zero = np.zeros(KK)
    sgn = _sgn(minimize)
    r0 = eng.acquire(Xs, zero, LI, 'ucb', beta=0.0, noise=noise, minimize=minimize, want=('acq', 'mu', 'sd'))
    sd = r0['sd']
    assert (r0['mu'] == 0.0).all() and np.unique(sd).size == sd.size
    worst = {}
    for kind in (AR.KINDS if points == 'full' else ('ei', 'logei', 'mes')):
        hits, cs = [], []
        for j, gw in enumerate(KATS['g']):
            if points == 'seams' and gw not in SEAM_G:
                continue
            found = AR.hit(gw, sd, start=7 * j)
            if found is None:
                continue
            i, p0 = found
            kw = dict(fstar=np.array([-sgn * p0])) if kind == 'mes' else dict(best=sgn * p0, xi=0.0)
            r = eng.acquire(Xs, zero, LI, kind, noise=noise, minimize=minimize, want=('acq', 'mu', 'sd'), **kw)
            assert _bits(r['sd'], sd) and (r['mu'] == 0.0).all()
            u = sgn * r['mu'][i]
            g = (sgn * kw['fstar'][0] - u) / sd[i] if kind == 'mes' else (u - sgn * kw['best'] - 0.0) / sd[i]      # the device's own expression
            assert _bits(g, gw) or (g == 0.0 and gw == 0.0), (kind, gw, g)
            hits.append(g)
            true = _fixture_truth(kind, j, sd[i])
            got = r['acq'][i]
            assert np.isfinite(got) and not (kind in ('pi', 'ei') and (got < 0 or np.signbit(got))), (kind, gw, got)
            assert abs(got - true) <= AR.allowance(kind, 'acq', g, true), (kind, gw, got, true)
            cs.append(float(AR.constants(kind, 'acq', [got], [true], g)[0]))
        # the input condition: both seams, a neighbour on either side of each, and every other point
        missing = AR.exact_condition(hits, KATS['g'])
        assert [m for m in missing if points == 'full' or m[0] != 'point'] == [], (kind, missing)
        worst[kind] = max(cs)
    print('exact g %s minimize=%d noise=%d (%s): worst constant %s' % (dtype, minimize, noise, points, ' '.join('%s=%.2f' % kv for kv in worst.items())))
    eng.close()


# ---- 2. dense sweeps with partials ------------------------------------------------------------------------------------------------------
def _check_rows(tag, kind, r, kw, noise, dmu, dstd, sd_star, worst):
    """value and gradient of every row in the measured range against the restatement at the call's own mu, sigma"""
    mu, sd = r['mu'], r['sd']
    g = AR.g_of(kind, mu, sd, **kw)
    rows = AR.in_measured_range(kind, g)
    ref = AR.restatement(kind, mu, sd, **kw)
    acq, grad = r['acq'], r['grad']
    assert np.isfinite(acq).all() and np.isfinite(grad[rows]).all(), tag
    if kind == 'logei':
        assert np.isfinite(grad).all(), tag                      # finite on the whole sweep, as the header promises
    if kind in ('pi', 'ei'):                                     # underflow gives +0.0 or a subnormal, never NaN or a negative
        assert (acq >= 0.0).all() and not np.signbit(acq).any(), tag
    if kind == 'mes':
        assert (acq >= 0.0).all(), tag
    bad = np.flatnonzero(rows & ~(np.abs(acq - ref['acq']) <= AR.allowance(kind, 'acq', g, ref['acq'])))
    assert bad.size == 0, (tag, 'acq', [(float(g[i]), float(acq[i]), float(ref['acq'][i])) for i in bad[:5]])
    dsig = dstd if noise else dstd * (sd_star / sd)[:, None]
    sgn = _sgn(kw['minimize'])
    want = sgn * ref['au'][:, None] * dmu + ref['as'][:, None] * dsig
    tol = AR.allowance(kind, 'au', g, ref['au'])[:, None] * np.abs(dmu) + AR.allowance(kind, 'as', g, ref['as'])[:, None] * np.abs(dsig)
    err = np.abs(grad - want)
    bad = np.flatnonzero(rows & ~(err <= tol).all(axis=1))
    assert bad.size == 0, (tag, 'grad', [(float(g[i]), grad[i].tolist(), want[i].tolist()) for i in bad[:5]])
    c = AR.constants(kind, 'acq', acq, ref['acq'], g)[rows]
    with np.errstate(all='ignore'):
        frac = np.where(tol > 0, err / tol, 0.0)[rows]
    worst[kind] = (max(worst.get(kind, (0, 0))[0], float(c.max())), max(worst.get(kind, (0, 0))[1], float(frac.max())))
    return g


@pytest.mark.parametrize('dtype,minimize,noise', [('f64', False, False), ('f64', True, True), ('f64', True, False), ('f64', False, True),
                                                  ('f32', False, True), ('f32', True, False)])
def test_dense_sweep_values_and_gradients_per_row(dtype, minimize, noise):
    eng = _engine(dtype)
    Xs = AR.sweep_pool()
    assert Xs.shape[0] <= 4096
    want = ('acq', 'mu', 'sd', 'grad')
    r0 = eng.acquire(Xs, ALPHA0, LI, 'ucb', beta=0.0, noise=noise, minimize=minimize, want=('acq', 'mu', 'sd'))
    worst = {}
    grads = {}
    for kind in AR.KINDS:
        scale, kw = AR.place(kind, r0['mu'], r0['sd'], minimize)
        alpha = scale * ALPHA0
        r = eng.acquire(Xs, alpha, LI, kind, noise=noise, want=want, **kw)
        assert _bits(r['sd'], r0['sd'])
        if scale not in grads:
            grads[scale] = eng.predict_grad(Xs, alpha, LI)
        _, sd_star, dmu, dstd = grads[scale]
        g = AR.g_of(kind, r['mu'], r['sd'], **kw)
        assert AR.sweep_coverage(g, -60, 40 if kind == 'mes' else 8) == [], (kind, AR.sweep_coverage(g, -60, 40 if kind == 'mes' else 8))
        _check_rows((dtype, kind, minimize, noise), kind, r, kw, noise, dmu, dstd, sd_star, worst)
        if kind == 'ei' and dtype == 'f32':                      # an f16x3 context runs the fp32 kernels: bit-equal
            from scfgp_amd.engine import HipEngine
            e16 = HipEngine(D, S, M, dtype='f16x3'); e16.set_params(PARAMS)
            b = e16.acquire(Xs, alpha, LI, kind, noise=noise, want=want, **kw)
            assert all(_bits(r[k], b[k]) for k in want)
            e16.close()
    # log-EI down the decades: the ladder
    mu_l0 = eng.acquire(AR.ladder_pool(), ALPHA0, LI, 'ucb', beta=0.0, want=('acq', 'mu'))['mu']
    Xl = AR.ladder_pool(AR.ladder_direction(mu_l0, minimize))
    alpha = AR.LADDER_SCALE * ALPHA0
    mu_l = eng.acquire(Xl, alpha, LI, 'ucb', beta=0.0, want=('acq', 'mu'))['mu']
    kw = dict(best=float(mu_l[0]), xi=0.0, minimize=minimize)
    r = eng.acquire(Xl, alpha, LI, 'logei', noise=noise, want=want, **kw)
    assert _bits(r['mu'], mu_l)
    _, sd_star, dmu, dstd = eng.predict_grad(Xl, alpha, LI)
    ladder = {}
    g = _check_rows((dtype, 'ladder', minimize, noise), 'logei', r, kw, noise, dmu, dstd, sd_star, ladder)
    assert g[0] == 0.0 and AR.decade_coverage(g) == [], AR.decade_coverage(g)
    worst['ladder'] = ladder['logei']
    print('sweep %s minimize=%d noise=%d: worst constant of acq, worst |d grad| / allowed: %s'
          % (dtype, minimize, noise, ' '.join('%s=%.2f,%.3f' % (k, v[0], v[1]) for k, v in worst.items())))
    eng.close()


# ---- 3. the pool where EI is gone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('minimize', [False, True])
def test_pool_where_ei_is_gone(dtype, minimize):
    eng = _engine(dtype)
    T = 1000
    Xs = AR.sweep_pool()[:T]
    sgn = _sgn(minimize)
    r0 = eng.acquire(Xs, ALPHA0, LI, 'ucb', beta=0.0, minimize=minimize, want=('acq', 'mu', 'sd'))
    best = sgn * float((sgn * r0["mu"]).max() + 62.0 * r0["sd"].max())      # g <= -62 sigma_max / sigma
    w = np.ones(T); w[:300] = 0.0; w[301] = 0.0                   # a workgroup's rows and more: the lowest eligible row is 300
    for wt, first in ((None, 0), (w, 300)):
        kw = dict(best=best, xi=0.0, minimize=minimize, w=wt, want=('acq', 'argmax', 'mu', 'sd'))
        r = eng.acquire(Xs, ALPHA0, LI, 'ei', **kw)
        g = AR.g_of('ei', r['mu'], r['sd'], best=best, minimize=minimize)
        assert (g < -60.0).all() and (r['acq'] == 0.0).all() and not np.signbit(r['acq']).any()
        assert r['idx'] == first and r['val'] == 0.0 and not np.signbit(r['val'])
        p = eng.acquire(Xs, ALPHA0, LI, 'pi', **kw)
        assert (p['acq'] == 0.0).all() and p['idx'] == first and p['val'] == 0.0
        l = eng.acquire(Xs, ALPHA0, LI, 'logei', **kw)
        ref = A.acquire('logei', l['mu'], l['sd'], best=best, xi=0.0, minimize=minimize)[0]
        assert (np.abs(l['acq'] - ref) <= AR.allowance('logei', 'acq', g, ref)).all()
        ok = np.ones(T, bool) if wt is None else wt > 0
        top = np.sort(ref[ok])[-2:]
        assert top[1] - top[0] > 2 * AR.allowance('logei', 'acq', g, ref).max()        # input condition: the winner is not a matter of rounding
        assert l['idx'] == A.argmax(ref, wt) == A.argmax(l['acq'], wt) and _bits(l['val'], l['acq'][l['idx']])
        assert np.isfinite(l['acq']).all() and l['acq'].max() < -1000.0
    eng.close()


# ---- 4. knowledge gradient with two reference rows ----------------------------------------------------------------------------------------
def _kg_rows(tag, r, d, B, z, worst):
    closed, c, zstar = AR.kg_closed_form(d, B)
    inside, outside = AR.kg_classes(zstar, z)
    allow = np.maximum(AR.DEVICE_FACTOR * AR.C_REF_KG * AR.kg_unit(c, B, z, closed), AR.TINY)
    kg, hi = r['kg'], r['kg_hi']
    assert np.isfinite(kg).all() and np.isfinite(hi).all() and (kg >= 0).all(), tag
    bad = np.flatnonzero(inside & ~(np.abs(kg - closed) <= allow))
    assert bad.size == 0, (tag, 'kg', [(float(c[i]), float(kg[i]), float(closed[i])) for i in bad[:5]])
    bad = np.flatnonzero(outside & (kg != 0.0))
    assert bad.size == 0, (tag, 'kg outside the nodes', [(float(c[i]), float(kg[i])) for i in bad[:5]])
    bad = np.flatnonzero(~(hi >= closed - allow))
    assert bad.size == 0, (tag, 'kg_hi', [(float(c[i]), float(hi[i]), float(closed[i])) for i in bad[:5]])
    with np.errstate(all='ignore'):
        unit = AR.kg_unit(c, B, z, closed)
        k = np.where(inside & (closed >= AR.TINY), np.abs(kg - closed) / unit, 0.0)
    worst[0] = max(worst[0], float(np.nanmax(k)))
    return c, inside, outside


@pytest.mark.parametrize('dtype,minimize,noise,nodes', [('f64', False, True, ('default', 'wide')), ('f64', True, False, ('default', 'wide')),
                                                        ('f64', True, True, ('wide',)), ('f64', False, False, ('default',)),
                                                        ('f32', False, True, ('wide',))])
def test_kg_of_two_reference_rows_per_candidate(dtype, minimize, noise, nodes):
    eng = _engine(dtype)
    Xc, Xr = AR.kg_pools()
    assert Xc.shape == (AR.T_KG, D) and Xr.shape == (2, D)
    cov = eng.predict_cov(Xc, LI, Xb=Xr)
    sd = eng.acquire(Xc, ALPHA0, LI, 'ucb', beta=0.0, noise=noise, want=('acq', 'sd'))['sd']
    B = G.slopes(cov, sd)                                         # tests/test_gpu_acquire_kg.py::_device_lines: the table is bit-equal to this
    mu_r0 = eng.predict(Xr, ALPHA0, LI)[0].ravel()
    want = ('kg', 'kg_hi')
    worst = [0.0]
    for name in nodes:
        z = G.DEFAULT_NODES if name == 'default' else AR.WIDE_NODES
        kw = dict(z=z, noise=noise, minimize=minimize, want=want)
        # Delta = 0 with equal slopes: a duplicated reference row
        r = eng.acquire_kg(Xc, ALPHA0, LI, Xr=np.vstack([Xr[:1], Xr[:1]]), **kw)
        assert (r['kg'] == 0.0).all() and (r['kg_hi'] == 0.0).all()
        cs, n_in, n_out = [], 0, 0
        for mult in AR.KG_DELTAS:
            if mult > 4.0 and name == 'default' and mult not in (10.0, 30.0):
                continue                                          # the multiples that only fill c > 5: beyond these nodes anyway
            alpha = np.zeros(KK) if mult == 0.0 else AR.kg_scale(mult, mu_r0, B) * ALPHA0     # alpha = 0: u = 0 exactly, the crossing at 0
            d = G.offsets(eng.predict(Xr, alpha, LI)[0].ravel(), minimize)
            assert d.max() == 0.0 and (mult != 0.0 or (d == 0.0).all())
            r = eng.acquire_kg(Xc, alpha, LI, Xr=Xr, **kw)
            c, inside, outside = _kg_rows((dtype, name, mult, minimize, noise), r, d, B, z, worst)
            cs.append(c); n_in += int(inside.sum()); n_out += int(outside.sum())
        c = np.concatenate(cs)
        assert n_in >= 4 and n_out >= 4
        if name == 'wide':                                        # c over [0, 38] densely, beyond 38 where kg underflows, beyond the last node
            assert AR.kg_coverage(c) == [], AR.kg_coverage(c)
            assert np.count_nonzero((c > 38) & (c < 60)) >= 4 and np.count_nonzero(c > 60 * (1 + AR.BORDER)) >= 4
        else:
            assert AR.kg_coverage(c, upto=5) == []                 # every unit interval inside these nodes
    print('kg two lines %s minimize=%d noise=%d: worst constant %.2f (C_REF_KG %.2f)' % (dtype, minimize, noise, worst[0], AR.C_REF_KG))
    eng.close()
