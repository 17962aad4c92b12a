"""GPU tier of the greedy choice by integrated variance reduction (scfgp_select_iv).  The device is fed the ORACLE's fit, so only its own
error shows.  fp64: the pick sequence equals tests/select_iv_ref.py's exactly (the reference's own gap between the best and the
second-best score is asserted first), var to TOL['f64']['eps'] relative, red and ivar to that times kappa max a / (1 + d) of the start
values (the size the recurrence rounds at), std_after and ivar[1] under the project's predictive bound against the oracle's refit on the
old rows plus the picks.  fp32: the device's own picks are replayed in the reference and every one of them must be near-optimal there
(ETA below).  Then: chunk boundaries, prefixes, appended rows, f16x3, an explicit copy of the pool as reference, raw mode, closure with
condition + predict_cov, errors, the training state, the facade."""
import functools

import numpy as np
import pytest

from oracle import scfgp_oracle as O
from scfgp_amd import synth
from scfgp_amd.scaler import Scaler
from tests import parity, pred_cov_ref
from tests import select_iv_ref as V
from tests import select_ref as R

pytestmark = pytest.mark.gpu

EPS = {'f64': parity.TOL['f64']['eps'], 'f32': parity.TOL['f32']['eps']}
# fp32: a pick must reach (1 - ETA) of the best score of the fp64 replay, and red[j] lie within ETA kappa max a / (1 + d) (start values)
# of the replay's.  Measured on an MI355X at FP32_RUNS, in units of TOL['f32']['eps'] = 1.5e-6 (DESIGN 4.11's table): the worst pick
# falls short of the best score by MEASURED_PICK (the device picked the fp64 sequence at every shape), the worst red[j] is off by
# MEASURED_RED.  ETA is 4x the larger of the two, the headroom tests/test_gpu_select.py gives.
MEASURED_PICK, MEASURED_RED = 0.0, 0.1616
ETA = 4.0 * max(MEASURED_PICK, MEASURED_RED) * EPS['f32']
REFS = ('pool', 'subset')
LONG_REF = slice(32668, 32868)                                  # the explicit reference rows of the two-chunk case


def reference_set(case, which):
    """(rows of the pool or None for Xr == NULL, weights or None)"""
    T = case[4]
    if which == 'pool':
        return None, None
    if which == 'straddle':
        rows = np.arange(T)[LONG_REF]
        return rows, 0.5 + np.random.default_rng(1).random(len(rows))
    return V.subset_reference(T)


@functools.lru_cache(maxsize=None)
def _fit(case):
    D, S, M, N0, T, m = case
    params, X0, y0, Xp = R.problem(case)
    _, alpha, Li = O.forward(X0, y0, params, S, M, gauss_hermite=False)
    C = pred_cov_ref.factor(Xp, Li, params, S, M)
    w = R.long_weights(T) if case in (R.LONG, R.LONG3) else None
    return params, X0, y0, Xp, alpha, Li, C, w


@functools.lru_cache(maxsize=None)
def _setup(case, which):
    params, X0, y0, Xp, alpha, Li, C, w = _fit(case)
    rows, om = reference_set(case, which)
    Q = V.gram(C if rows is None else C[rows], om)
    Xr = None if rows is None else np.ascontiguousarray(Xp[rows])
    return Q, Xr, om, V.select(C, Q, case[5], w=w, kap=R.kappa(params))


@functools.lru_cache(maxsize=None)
def _refit(case, which, picks):
    """from the oracle's own fit on the old rows plus the rows `picks` of the pool (zero targets): its predictive std at the pool, its
    sum_r omega_r (sigma_r^2 - kappa) over the reference rows, and the sum of the predictive bound's |d sigma^2| / eps over them"""
    D, S, M, N0, T, m = case
    params, X0, y0, Xp = _fit(case)[:4]
    rows, om = reference_set(case, which)
    Xa = np.vstack([X0, Xp[list(picks)]]); ya = np.vstack([y0, np.zeros((len(picks), 1))])
    _, a2, L2 = O.forward(Xa, ya, params, S, M, gauss_hermite=False)
    sd = O.predict(Xp, a2, L2, params, S, M)[1].ravel()
    sr = sd if rows is None else sd[rows]
    om = np.ones(len(sr)) if om is None else om
    return sd, float(om @ (sr ** 2 - R.kappa(params))), float(om @ (2.0 * sr ** 2))


def _engine(D, S, M, dtype, params):
    from scfgp_amd.engine import HipEngine
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params)
    return eng


def _std_ratio(sd, sd0, dtype):
    return float((np.abs(sd - sd0) / (EPS[dtype] * sd0)).max())


def _run_fp64(case, which):
    D, S, M, N0, T, m = case
    params, X0, y0, Xp, alpha, Li, C, w = _fit(case)
    Q, Xr, om, ref = _setup(case, which)
    kap = R.kappa(params)
    assert ref['gap'].min() > 1e-8, 'the input itself has near-ties: no exact sequence to ask for'
    eng = _engine(D, S, M, 'f64', params)
    idx, red, var, ivar, sd = eng.select_iv(Xp, Li, m, Xr=Xr, w=w, wr=om, return_std=True)
    eng.close()
    assert idx.dtype == np.int64 and idx.shape == (m,) and red.shape == (m,) and var.shape == (m,) and ivar.shape == (2,) and sd.shape == (T,)
    scale = V.scale(ref, kap)
    rv = float((np.abs(var - ref['var']) / ref['var']).max())
    rr = float(np.abs(red - ref['red']).max() / scale); ri = float(np.abs(ivar - ref['ivar']).max() / scale)
    sd0, iv0, ivb = _refit(case, which, tuple(ref['idx'].tolist()))
    rf = abs(ivar[1] - iv0) / (EPS['f64'] * ivb)
    print('select_iv f64 %s %s: smallest reference gap %.3g, var rel err %.3g, red err %.3g and ivar err %.3g of kappa max a/(1+d), '
          'std_after ratio to the f64 bound %.3g, ivar[1] against the refit: ratio to the f64 bound %.3g' %
          (case, which, ref['gap'].min(), rv, rr, ri, _std_ratio(sd, sd0, 'f64'), rf))
    assert np.array_equal(idx, ref['idx'])
    assert rv <= EPS['f64'] and rr <= EPS['f64'] and ri <= EPS['f64']
    assert np.all(np.isfinite(sd)) and np.all(var >= 0) and np.all(red > 0)
    parity.check_predict(sd0, sd, sd0, sd0, 'f64')
    assert rf <= 1.0
    return idx, w


@pytest.mark.parametrize('which', REFS)
@pytest.mark.parametrize('case', R.CASES)
def test_fp64_picks_equal_the_reference(case, which):
    _run_fp64(case, which)


@pytest.mark.parametrize('which', ['pool', 'straddle'])
def test_fp64_two_chunks(which):
    """pool as reference: Q is summed over two chunks; explicit reference rows on both sides of row 32768"""
    idx, w = _run_fp64(R.LONG, which)
    assert idx.min() < 32768 <= idx.max() and np.all(w[idx] > 0)


def test_fp64_three_chunks():
    """three chunks of pool and reference: a half of the row feed is reused.  Under this criterion the reference's 8 picks lie in the
    second and the third chunk (six in 32772 .. 32790, then 65537 and 65556): they straddle row 65536"""
    idx, w = _run_fp64(R.LONG3, 'pool')
    assert np.any((idx >= 32768) & (idx < 65536)) and idx.max() >= 65536 and np.all(w[idx] > 0)


def fp32_ratios(case, which, idx, red):
    """worst shortfall of a pick against the best score of the fp64 replay, worst error of red[j] against the replay's in units of kappa
    max a / (1 + d): both in units of TOL['f32']['eps']"""
    params, X0, y0, Xp, alpha, Li, C, w = _fit(case)
    Q, Xr, om, ref = _setup(case, which)
    kap = R.kappa(params)
    As, Ds, scores, qs = V.replay(C, Q, w, idx)
    m = len(idx)
    got = scores[np.arange(m), idx]
    assert np.all(np.isfinite(got)), 'a pick that was not eligible'
    pick = float((1.0 - got / scores.max(axis=1)).max())
    rerr = float(np.abs(red - kap * qs).max() / V.scale(ref, kap))
    return pick / EPS['f32'], rerr / EPS['f32']


FP32_RUNS = [(c, r) for c in R.CASES for r in REFS] + [(R.LONG, 'pool'), (R.LONG, 'straddle'), (R.LONG3, 'pool')]


@pytest.mark.parametrize('case,which', FP32_RUNS)
def test_fp32_picks_are_near_optimal_in_the_reference(case, which):
    D, S, M, N0, T, m = case
    params, X0, y0, Xp, alpha, Li, C, w = _fit(case)
    Q, Xr, om, ref = _setup(case, which)
    eng = _engine(D, S, M, 'f32', params)
    idx, red, var, ivar, sd = eng.select_iv(Xp, Li, m, Xr=Xr, w=w, wr=om, return_std=True)
    eng.close()
    assert len(set(idx.tolist())) == m and idx.min() >= 0 and idx.max() < T
    rp, rr = fp32_ratios(case, which, idx, red)
    sd0 = _refit(case, which, tuple(idx.tolist()))[0]
    rs = _std_ratio(sd, sd0, 'f32')
    print('select_iv f32 %s %s: same sequence as fp64: %s; pick shortfall %.3g eps32, red error %.3g eps32 (ETA = %.3g eps32), '
          'std_after ratio to the f32 bound %.3g' % (case, which, np.array_equal(idx, ref['idx']), rp, rr, ETA / EPS['f32'], rs))
    assert rp * EPS['f32'] <= ETA, ('a pick is not near-optimal in the reference', case, which, rp)
    assert rr * EPS['f32'] <= ETA, ('red outside its bound', case, which, rr)
    assert abs(ivar[0] - red.sum() - ivar[1]) <= 1e-12 * ivar[0]
    assert np.all(np.isfinite(sd)) and rs <= 1.0


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_prefix_property(dtype):
    case = R.CASES[0]
    D, S, M, N0, T, m = case
    params, X0, y0, Xp, alpha, Li, C, w = _fit(case)
    Q, Xr, om, ref = _setup(case, 'subset')
    eng = _engine(D, S, M, dtype, params)
    short = eng.select_iv(Xp, Li, 7, Xr=Xr, wr=om)
    full = eng.select_iv(Xp, Li, m, Xr=Xr, wr=om)
    eng.close()
    for u, v in zip(short[:3], full[:3]):
        assert np.array_equal(u, v[:7])
    assert short[3][0] == full[3][0]


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_appended_rows_of_weight_zero_change_nothing(dtype):
    case = R.CASES[0]
    D, S, M, N0, T, m = case
    params, X0, y0, Xp, alpha, Li, C, w = _fit(case)
    Q, Xr, om, ref = _setup(case, 'subset')
    extra = synth.make_X(99, 500, D)
    eng = _engine(D, S, M, dtype, params)
    base = eng.select_iv(Xp, Li, m, Xr=Xr, wr=om, return_std=True)
    more = eng.select_iv(np.vstack([Xp, extra]), Li, m, Xr=Xr, wr=om, w=np.r_[np.ones(T), np.zeros(500)], return_std=True)
    eng.close()
    for u, v in zip(base[:4], more[:4]):
        assert np.array_equal(u, v)
    assert np.array_equal(base[4], more[4][:T]) and np.all(np.isfinite(more[4][T:]))


def test_f16x3_equals_fp32_bit_for_bit():
    case = R.CASES[3]
    D, S, M, N0, T, m = case
    params, X0, y0, Xp, alpha, Li, C, w = _fit(case)
    Q, Xr, om, ref = _setup(case, 'subset')
    out = []
    for dtype in ('f32', 'f16x3'):
        eng = _engine(D, S, M, dtype, params)
        out.append(eng.select_iv(Xp, Li, m, Xr=Xr, wr=om, return_std=True) + eng.select_iv(Xp, Li, m, return_std=True))
        eng.close()
    for u, v in zip(*out):
        assert np.array_equal(u, v)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_a_copy_of_the_pool_as_reference_equals_the_implicit_one(dtype):
    """values to 1e-12 (fp64) / the same picks; no bit identity is claimed: the explicit reference passes through its own chunk buffer"""
    case = R.CASES[0]
    D, S, M, N0, T, m = case
    params, X0, y0, Xp, alpha, Li, C, w = _fit(case)
    om = 0.5 + np.random.default_rng(2).random(T)
    eng = _engine(D, S, M, dtype, params)
    a = eng.select_iv(Xp, Li, m, wr=om, return_std=True)
    b = eng.select_iv(Xp, Li, m, Xr=Xp.copy(), wr=om, return_std=True)
    eng.close()
    assert np.array_equal(a[0], b[0])
    for u, v in zip(a[1:], b[1:]):
        assert np.linalg.norm(u - v) <= 1e-12 * np.linalg.norm(v)


def _scaled_problem(xalgo, seed=5, N=600):
    """tests/test_gpu_condition.py's problem: an engine trained on scaled data of 4 raw columns, one of them constant"""
    from scfgp_amd.engine import HipEngine
    rng = np.random.default_rng(seed)
    Xr = np.column_stack([rng.uniform(0.5, 3.0, N), rng.gamma(2.0, 1.0, N), np.full(N, 2.5), rng.normal(1.0, 2.0, N)])
    yr = np.exp(0.3 * np.sin(Xr[:, :1]) + 0.1 * Xr[:, 1:2]) + 0.05 * rng.standard_normal((N, 1))
    xs = Scaler(xalgo); xs.fit(Xr); ys = Scaler('normal'); ys.fit(yr)
    D, S, M = 3, 2, 40
    eng = HipEngine(D, S, M, dtype='f64')
    eng.set_params(synth.make_params(seed, D, S, M, abc=(-1.0, 0.0, -4.0)))
    fx = np.ascontiguousarray(xs.forward_transform(Xr)); fy = np.ascontiguousarray(ys.forward_transform(yr))
    eng.set_data(fx[:300], fy[:300])
    _, _, alpha, Li = eng.eval(want_grad=False)
    eng.set_x_scaler(xs)
    return eng, alpha.copy(), Li.copy(), Xr[300:], fx[300:]


@pytest.mark.parametrize('xalgo', Scaler.algos)
def test_raw_mode_equals_scaled_mode(xalgo):
    eng, alpha, Li, Xraw, fx = _scaled_problem(xalgo)
    assert Xraw.shape[1] == 4 and fx.shape[1] == 3                                  # the constant column is dropped
    om = 0.5 + np.random.default_rng(1).random(100)
    raw = eng.select_iv(Xraw[:200], Li, 12, Xr=Xraw[200:], wr=om, raw=True, return_std=True)
    sc = eng.select_iv(fx[:200], Li, 12, Xr=fx[200:], wr=om, return_std=True)
    eng.close()
    assert np.array_equal(raw[0], sc[0])
    for u, v in zip(raw[1:], sc[1:]):
        assert np.linalg.norm(u - v) <= 1e-12 * np.linalg.norm(v)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('case', [R.CASES[0], R.CASES[2]])
def test_closure_with_condition_and_predict_cov(case, dtype):
    """the library against itself: condition on the picked rows with zero targets, then the diagonal of predict_cov over the reference
    rows summed with omega, gives ivar[1]"""
    D, S, M, N0, T, m = case
    params, X0, y0, Xp, alpha, Li, C, w = _fit(case)
    Q, Xr, om, ref = _setup(case, 'subset')
    eng = _engine(D, S, M, dtype, params)
    idx, red, var, ivar = eng.select_iv(Xp, Li, m, Xr=Xr, wr=om)
    a2, L2 = eng.condition(Xp[idx], np.zeros(m), alpha, Li)
    diag = np.diag(eng.predict_cov(Xr, L2)); diag0 = np.diag(eng.predict_cov(Xr, Li))
    eng.close()
    kap = R.kappa(params)
    # the predictive bound |d sigma| <= eps sigma on sigma^2 = kappa + diag, summed with omega
    bound = EPS[dtype] * float(om @ (2.0 * (kap + diag))); bound0 = EPS[dtype] * float(om @ (2.0 * (kap + diag0)))
    r = abs(float(om @ diag) - ivar[1]) / bound; r0 = abs(float(om @ diag0) - ivar[0]) / bound0
    print('select_iv closure %s %s: ivar against predict_cov before and condition + predict_cov after, ratios to the %s bound %.3g, %.3g' %
          (case, dtype, dtype, r0, r))
    assert r <= 1.0 and r0 <= 1.0
    assert float(om @ diag0) - float(om @ diag) > 100.0 * bound               # the picks did move the integrated variance


def test_errors_leave_the_outputs_untouched():
    from scfgp_amd._lib import _c_i64_p, dptr
    from scfgp_amd.engine import HipEngine
    case = R.CASES[0]
    D, S, M, N0, T, m = case
    params, X0, y0, Xp, alpha, Li, C, w = _fit(case)
    Q, Xr, om, ref = _setup(case, 'subset')
    Rn = len(om)
    eng = _engine(D, S, M, 'f64', params)
    idx = np.full(m, -7, np.int64); red = np.full(m, 3.0); var = np.full(m, 3.0); ivar = np.full(2, 3.0); sd = np.full(T, 3.0)
    ones = np.ones(T)

    def lib_call(X_, T_, w_, Xr_, R_, wr_, L_, m_, mode, idx_=idx, engine=eng):
        rc = engine.lib.scfgp_select_iv(engine.ctx, dptr(X_), T_, dptr(w_), dptr(Xr_), R_, dptr(wr_), dptr(L_), m_, mode,
                                        None if idx_ is None else idx_.ctypes.data_as(_c_i64_p), dptr(red), dptr(var), dptr(ivar), dptr(sd))
        engine._check(rc, 'select_iv')
    wneg = ones.copy(); wneg[17] = -1e-3
    wfew = np.zeros(T); wfew[:m - 1] = 1.0
    omneg = om.copy(); omneg[5] = -1e-3
    for args, msg in (((None, T, None, Xr, Rn, om, Li, m, 0), 'bad arguments'), ((Xp, T, None, Xr, Rn, om, None, m, 0), 'bad arguments'),
                      ((Xp, T, None, Xr, Rn, om, Li, m, 2), 'bad arguments'), ((Xp, T, None, Xr, Rn, om, Li, m, -1), 'bad arguments'),
                      ((Xp, 0, None, Xr, Rn, om, Li, m, 0), r'T must lie in 1\.\.1048576'),
                      ((Xp, (1 << 20) + 1, None, Xr, Rn, om, Li, m, 0), r'T must lie in'),
                      ((Xp, T, None, Xr, Rn, om, Li, 0, 0), r'm must lie in 1\.\.4096'), ((Xp, T, None, Xr, Rn, om, Li, 4097, 0), r'm must lie in'),
                      ((Xp, T, None, Xr, 0, om, Li, m, 0), 'R must be at least 1'), ((Xp, T, None, Xr, -3, None, Li, m, 0), 'R must be at least 1'),
                      ((Xp, T, None, Xr, Rn, om, Li, m, 1), 'no X scaler'), ((Xp, T, wneg, Xr, Rn, om, Li, m, 0), 'negative weight at row 17'),
                      ((Xp, T, None, Xr, Rn, omneg, Li, m, 0), 'negative reference weight at row 5'),
                      ((Xp, T, None, Xr, Rn, np.zeros(Rn), Li, m, 0), 'no reference row has a positive weight'),
                      ((Xp, T, None, None, 0, np.zeros(T), Li, m, 0), 'no reference row has a positive weight'),
                      ((Xp, T, wfew, Xr, Rn, om, Li, m, 0), 'only %d rows have a positive weight' % (m - 1)),
                      ((Xp, 5, None, Xr, Rn, om, Li, 6, 0), 'only 5 rows have a positive weight')):
        with pytest.raises(ValueError, match=msg):
            lib_call(*args)
    with pytest.raises(ValueError, match='bad arguments'):
        lib_call(Xp, T, None, Xr, Rn, om, Li, m, 0, idx_=None)
    for bad in (np.nan, np.inf):
        wb = ones.copy(); wb[3] = bad
        with pytest.raises(FloatingPointError, match='non-finite'):
            lib_call(Xp, T, wb, Xr, Rn, om, Li, m, 0)
        ob = om.copy(); ob[3] = bad
        with pytest.raises(FloatingPointError, match='non-finite'):
            lib_call(Xp, T, None, Xr, Rn, ob, Li, m, 0)
        Xb = Xp.copy(); Xb[T - 1, 2] = bad
        with pytest.raises(FloatingPointError, match='non-finite'):
            lib_call(Xb, T, None, Xr, Rn, om, Li, m, 0)
        Xrb = Xr.copy(); Xrb[Rn - 1, 1] = bad
        with pytest.raises(FloatingPointError, match='non-finite'):
            lib_call(Xp, T, None, Xrb, Rn, om, Li, m, 0)
        Lb = Li.copy(); Lb[50, 3] = bad
        with pytest.raises(FloatingPointError, match='non-finite'):
            lib_call(Xp, T, None, Xr, Rn, om, Lb, m, 0)
    assert np.all(idx == -7) and np.all(red == 3.0) and np.all(var == 3.0) and np.all(ivar == 3.0) and np.all(sd == 3.0)
    # the wrapper's own checks
    with pytest.raises(ValueError, match='columns'):
        eng.select_iv(Xp[:, :4], Li, m)
    with pytest.raises(ValueError, match='columns'):
        eng.select_iv(Xp, Li, m, Xr=Xr[:, :4])
    with pytest.raises(ValueError, match='entries'):
        eng.select_iv(Xp, Li, m, w=ones[:-1])
    with pytest.raises(ValueError, match='entries'):
        eng.select_iv(Xp, Li, m, Xr=Xr, wr=om[:-1])
    with pytest.raises(ValueError, match='entries'):
        eng.select_iv(Xp, Li, m, wr=om)                                    # the pool is the reference: T weights
    with pytest.raises(ValueError, match='shape'):
        eng.select_iv(Xp, Li[:-1], m)
    with pytest.raises(ValueError, match='scaler'):
        eng.select_iv(Xp, Li, m, raw=True)
    # entries of Li above the diagonal are not read; the context still works; red, var, ivar and std_after may be left out
    Lu = Li + np.triu(np.full_like(Li, np.nan), 1)
    out = eng.select_iv(Xp, Lu, m, Xr=Xr, wr=om)
    assert np.array_equal(out[0], ref['idx'])
    lib_call(Xp, T, None, Xr, Rn, om, Li, m, 0)
    assert np.array_equal(idx, ref['idx']) and np.array_equal(red, out[1]) and np.array_equal(var, out[2]) and np.array_equal(ivar, out[3])
    idx2 = np.full(m, -7, np.int64)
    assert eng.lib.scfgp_select_iv(eng.ctx, dptr(Xp), T, None, dptr(Xr), Rn, dptr(om), dptr(Li), m, 0, idx2.ctypes.data_as(_c_i64_p), None, None,
                                   None, None) == 0
    assert np.array_equal(idx2, ref['idx'])
    eng.close()
    keep_sd = sd.copy()
    fresh = HipEngine(D, S, M, dtype='f64')                              # no parameters yet
    with pytest.raises(ValueError, match='parameters not set'):
        fresh.select_iv(Xp, Li, m)
    fresh.close()
    big = HipEngine(8, 4, 2100, dtype='f64')                             # K = 4200: Kp above the LDS bound
    big.set_params(synth.make_params(3, 8, 4, 2100, abc=(-1.0, 0.0, -1.0)))
    with pytest.raises(ValueError, match='K above 4096'):
        lib_call(np.zeros((4, 8)), 4, None, None, 0, None, np.zeros(4), 2, 0, engine=big)
    big.close()
    assert np.array_equal(idx, ref['idx']) and np.array_equal(red, out[1]) and np.array_equal(var, out[2]) and np.array_equal(ivar, out[3])
    assert np.all(sd == keep_sd)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_training_state_survives(dtype):
    from scfgp_amd.engine import HipEngine
    D, S, M, N = 20, 20, 280, 1500
    params = synth.make_params(7, D, S, M, abc=(-1.0, 0.0, -1.0))
    X = synth.make_X(7, N, D)
    y = np.sin(3 * X[:, :1]) + 0.1 * synth.normal(10, 0, N)[:, None]
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params); eng.set_data(X, y)
    c0, g0, a0, L0 = eng.eval(want_grad=True)
    c0, g0, a0, L0 = float(c0), g0.copy(), a0.copy(), L0.copy()
    idx, red, var, ivar = eng.select_iv(synth.make_X(8, 700, D), L0, 32, Xr=synth.make_X(9, 300, D))
    assert len(set(idx.tolist())) == 32
    c1, g1, a1, L1 = eng.eval(want_grad=True)
    assert float(c1) == c0 and np.array_equal(g1, g0) and np.array_equal(a1, a0) and np.array_equal(L1, L0)
    eng.close()


def test_facade():
    from scfgp_amd import SCFGP
    rng = np.random.default_rng(5)
    np.random.seed(5)
    N, T, m = 90, 200, 10
    X = rng.uniform(-2, 2, (N + T, 3))
    X = np.column_stack([X[:, :2], np.full(N + T, 4.0), X[:, 2:]])      # a constant column
    y = np.sin(X[:, :1]) + 0.5 * X[:, 1:2] ** 2 + 0.05 * rng.standard_normal((N + T, 1))
    model = SCFGP(sparsity=3, nfeats=12)
    model.fit(X[:N], y[:N], max_iter=15,
              algo={'algo': 'adam', 'algo_params': {'learning_rate': 0.02, 'beta1': 0.9, 'beta2': 0.999, 'epsilon': 1e-8}})
    pool, ref_rows = X[N:N + 150], X[N + 150:]
    a_before, L_before = np.array(model.alpha), np.array(model.Li)
    idx, red, ivar = model.select_iv(pool, m, X_ref=ref_rows)
    assert idx.shape == (m,) and red.shape == (m,) and ivar.shape == (2,) and len(set(idx.tolist())) == m
    assert np.array_equal(model.alpha, a_before) and np.array_equal(model.Li, L_before)
    assert np.all(red > 0) and abs(ivar[0] - red.sum() - ivar[1]) <= 1e-12 * ivar[0]
    owner = model.pred_func.__self__
    _, sd_ref = owner.pred_raw(ref_rows, model.X_scaler, model.alpha, model.Li)
    # weights: the row is not for sale
    w = np.ones(150); w[idx[0]] = 0.0
    idx_w, _, _ = model.select_iv(pool, m, X_ref=ref_rows, weights=w)
    assert idx[0] not in idx_w.tolist()
    # select -> observe -> condition: the summed variance over the reference rows drops by what select_iv announced
    model.condition(pool[idx], y[N:N + 150][idx])
    _, sd_now = owner.pred_raw(ref_rows, model.X_scaler, model.alpha, model.Li)
    drop = float(np.sum(np.asarray(sd_ref).ravel() ** 2) - np.sum(np.asarray(sd_now).ravel() ** 2))
    assert abs(drop - red.sum()) <= 1e-9 * float(np.sum(np.asarray(sd_ref).ravel() ** 2) + np.sum(np.asarray(sd_now).ravel() ** 2)) * 2.0
    # the pool as its own reference, with reference weights
    idx_p, red_p, ivar_p = model.select_iv(pool, m, ref_weights=np.linspace(0.5, 1.5, 150))
    assert len(set(idx_p.tolist())) == m and ivar_p[1] < ivar_p[0]
    with pytest.raises(ValueError, match='m must lie in'):
        model.select_iv(pool, 0)
    with pytest.raises(ValueError, match='rows have a positive weight'):
        model.select_iv(pool, 151)
