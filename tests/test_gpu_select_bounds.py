"""GPU tier of the selection entry points at the far end of their documented ranges (include/scfgp_hip.h: T <= 2^20 rows, m <= 4096 picks,
Kp <= 8192 for scfgp_select and <= 4096 for scfgp_select_iv).  The kernels change behaviour there and nowhere below:

  rows     select_rows_per_group leaves 64 rows per workgroup above T = 262144 (128, then 256 above 524288); selectqei's commit folds 32
           records per thread at T = 2^20
  columns  the sweeps keep u_j (and v) in LDS as fp64: 64 KB of dynamic LDS at either bound
  picks    the projection of pick j runs over ceil(j / 64) chunks of earlier picks: 64 of them at m = 4096, a one-pass Gram-Schmidt
           4096 steps deep

The assertions are those of tests/test_gpu_select.py, test_gpu_select_iv.py and test_gpu_select_qei.py with their constants; the one
bound of this file's own is ETA_DEEP of the 4096-pick shape (measured, below).  Reference inputs are built once per shape and shared
between the dtypes."""
import functools

import numpy as np
import pytest

from oracle import scfgp_oracle as O
from scfgp_amd import synth
from tests import parity, pred_cov_ref
from tests import select_iv_ref as V
from tests import select_qei_ref as Q
from tests import select_ref as R
from tests.test_gpu_sample_argmax import _synthetic
from tests.test_gpu_select import ETA as ETA_SELECT
from tests.test_gpu_select_iv import ETA as ETA_IV
from tests.test_gpu_select_qei import _call, _check_against_block

pytestmark = pytest.mark.gpu

EPS = {'f64': parity.TOL['f64']['eps'], 'f32': parity.TOL['f32']['eps']}
# a pick must reach (1 - ETA) of the best score of the fp64 replay: the fp32 constants of the two files, TOL['f64']['eps'] for fp64
ETA1 = {'select': {'f64': EPS['f64'], 'f32': ETA_SELECT}, 'iv': {'f64': EPS['f64'], 'f32': ETA_IV}}
DTYPES = ['f64', 'f32']

ROWS_SHAPE = (3, 1, 20, 150)                                    # D, S, M, N0: K = 42, Kp = 128
ROWS_T = [262144 + 69, 1 << 20]                                 # 128 rows per group, a ragged last one; 256 and exactly 4096 groups
ROWS_M = 8
KP_SELECT = (4, 32, 4064, 300, 16)                              # D, S, M, T, m: K = Kp = 8192
KP_IV = (4, 32, 2016, 300, 16)                                  # K = Kp = 4096
DEEP = (4, 16, 2288, 6000, 4096)                                # K = Kp = 4608
DEEP_PREFIX = 70                                                # crosses the first boundary of the projection's 64-pick chunks

# The 4096-pick shape, measured on an MI355X against the Cholesky replay (tests/select_ref.py: replay_chol) of the device's own picks,
# in units of the dtype's EPS (DESIGN 4.10's second table): the worst (best_j - got_j) / (1 + d0[p_j]) and the worst
# |var[j] - kappa dp_j| / (kappa (1 + d0[p_j])).  The relative form of the other shapes cannot hold here: the last picks have
# dp = 5e-3 at d0 = 5, three digits cancel.  ETA_DEEP is 4x the larger of the two, the headroom tests/test_gpu_select.py gives.
# CPU_DEEP: the same two figures of select_ref.select's own fp64 recurrence against the Cholesky replay, in units of EPS['f64']: the
# device's fp64 chain is as far from the replay as the reference recurrence is (3.5e-15 of 1 + d0; no pick of either falls short).  The
# fp32 figure, 9.7e-9, is below the fp32 error of var at the shallow shapes (up to 0.0418 eps32) without any cancellation factor.
MEASURED_DEEP = {'f64': (0.0, 3.529e-6), 'f32': (0.0, 0.006451)}
CPU_DEEP = (0.0, 3.537e-6)
ETA_DEEP = {t: 4.0 * max(MEASURED_DEEP[t]) * EPS[t] for t in DTYPES}


def _engine(D, S, M, dtype, params):
    from scfgp_amd.engine import HipEngine
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params)
    return eng


def _std_ratio(sd, sd0, dtype):
    return float((np.abs(sd - sd0) / (EPS[dtype] * sd0)).max())


def _std_of(d, kap):
    return np.sqrt(kap * (1.0 + d))


# ---- 1. the row axis ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rows(T):
    D, S, M, N0 = ROWS_SHAPE
    params, X0, y0, Xp = R.problem((D, S, M, N0, T, ROWS_M))
    _, alpha, Li = O.forward(X0, y0, params, S, M, gauss_hermite=False)
    C = pred_cov_ref.factor(Xp, Li, params, S, M)
    return params, Xp, Li, C, R.edge_weights(T), V.gram(C)


def _assert_edges(T, w, idx):
    """on the reference alone: the picks are weighted rows and reach row T - 1 and a second row of the last group"""
    last = (T - 1) // R.rows_per_group(T) * R.rows_per_group(T)
    assert np.all(w[idx] > 0) and T - 1 in idx.tolist() and np.count_nonzero(idx >= last) >= 2, idx
    rows = R.edge_rows(T)
    assert {0, T - 1, last, 32767, 32768} <= set(rows.tolist()) and len(rows) <= 64 and np.count_nonzero(w) == len(rows)


@pytest.mark.parametrize('T', ROWS_T)
def test_rows_select_sparse_weights_fp64(T):
    D, S, M, N0 = ROWS_SHAPE
    params, Xp, Li, C, w, Qm = _rows(T)
    ref = R.select(C, ROWS_M, w=w, kap=R.kappa(params))
    _assert_edges(T, w, ref['idx'])
    assert ref['gap'].min() > 1e-8, 'the input itself has near-ties: no exact sequence to ask for'
    eng = _engine(D, S, M, 'f64', params)
    idx, var, gain, sd = eng.select(Xp, Li, ROWS_M, w=w, return_std=True)
    eng.close()
    rv = float((np.abs(var - ref['var']) / ref['var']).max()); rg = float((np.abs(gain - ref['gain']) / ref['gain']).max())
    print('select f64 T = %d, %d rows per group, sparse weights: picks %s, smallest reference gap %.3g, var rel err %.3g, gain rel err '
          '%.3g, std_after ratio to the f64 bound %.3g' % (T, R.rows_per_group(T), ref['idx'].tolist(), ref['gap'].min(), rv, rg,
                                                           _std_ratio(sd, ref['std_after'], 'f64')))
    assert np.array_equal(idx, ref['idx'])
    assert rv <= EPS['f64'] and rg <= EPS['f64']
    assert sd.shape == (T,) and np.all(np.isfinite(sd))
    parity.check_predict(ref['std_after'], sd, ref['std_after'], ref['std_after'], 'f64')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('T', ROWS_T)
def test_rows_select_every_row_eligible(T, dtype):
    """select_ones at size; std_after at ALL T rows against the replay: a row that no workgroup visits, or two do, shows there"""
    D, S, M, N0 = ROWS_SHAPE
    params, Xp, Li, C, w, Qm = _rows(T)
    kap = R.kappa(params)
    eng = _engine(D, S, M, dtype, params)
    idx, var, gain, sd = eng.select(Xp, Li, ROWS_M, return_std=True)
    eng.close()
    assert len(set(idx.tolist())) == ROWS_M and idx.min() >= 0 and idx.max() < T
    ds, scores = R.replay(C, None, idx)
    ar = np.arange(ROWS_M)
    got = scores[ar, idx]
    assert np.all(np.isfinite(got)), 'a pick that was not eligible'
    pick = float((1.0 - got / scores.max(axis=1)).max())
    dref = ds[ar, idx]
    verr = float((np.abs(var - kap * dref) / (kap * (1.0 + dref))).max())
    rs = _std_ratio(sd, _std_of(ds[-1], kap), dtype)
    eta = ETA1['select'][dtype]
    print('select %s T = %d, every row eligible: picks %s, pick shortfall %.3g eps, var error %.3g eps (ETA = %.3g eps), std_after at all '
          'rows: ratio to the bound %.3g' % (dtype, T, idx.tolist(), pick / EPS[dtype], verr / EPS[dtype], eta / EPS[dtype], rs))
    assert pick <= eta and verr <= eta
    assert np.allclose(gain, 0.5 * np.log1p(var / kap), rtol=1e-12, atol=0)
    assert sd.shape == (T,) and np.all(np.isfinite(sd)) and rs <= 1.0


@pytest.mark.parametrize('T', ROWS_T)
def test_rows_select_iv_sparse_weights_fp64(T):
    D, S, M, N0 = ROWS_SHAPE
    params, Xp, Li, C, w, Qm = _rows(T)
    kap = R.kappa(params)
    ref = V.select(C, Qm, ROWS_M, w=w, kap=kap)
    _assert_edges(T, w, ref['idx'])
    assert ref['gap'].min() > 1e-8, 'the input itself has near-ties: no exact sequence to ask for'
    eng = _engine(D, S, M, 'f64', params)
    idx, red, var, ivar, sd = eng.select_iv(Xp, Li, ROWS_M, w=w, return_std=True)
    eng.close()
    scale = V.scale(ref, kap)
    rv = float((np.abs(var - ref['var']) / ref['var']).max())
    rr = float(np.abs(red - ref['red']).max() / scale); ri = float(np.abs(ivar - ref['ivar']).max() / scale)
    print('select_iv f64 T = %d, sparse weights: picks %s, smallest reference gap %.3g, var rel err %.3g, red err %.3g and ivar err %.3g of '
          'kappa max a/(1+d), std_after ratio to the f64 bound %.3g' % (T, ref['idx'].tolist(), ref['gap'].min(), rv, rr, ri,
                                                                        _std_ratio(sd, ref['std_after'], 'f64')))
    assert np.array_equal(idx, ref['idx'])
    assert rv <= EPS['f64'] and rr <= EPS['f64'] and ri <= EPS['f64']
    assert np.all(np.isfinite(sd)) and np.all(var >= 0) and np.all(red > 0)
    parity.check_predict(ref['std_after'], sd, ref['std_after'], ref['std_after'], 'f64')


def _iv_near_optimal(C, Qm, w, kap, dtype, out, label):
    """test_gpu_select_iv.py's fp32 form on the device's own picks, and std_after at all rows against the replay"""
    idx, red, var, ivar, sd = out
    T, m = C.shape[0], len(idx)
    assert len(set(idx.tolist())) == m and idx.min() >= 0 and idx.max() < T
    As, Ds, scores, qs = V.replay(C, Qm, w, idx)
    ar = np.arange(m)
    got = scores[ar, idx]
    assert np.all(np.isfinite(got)), 'a pick that was not eligible'
    pick = float((1.0 - got / scores.max(axis=1)).max())
    scale = kap * float((As[0] / (1.0 + Ds[0])).max())
    rerr = float(np.abs(red - kap * qs).max() / scale)
    i0 = kap * float(np.trace(Qm))
    ierr = max(abs(ivar[0] - i0), abs(ivar[1] - (i0 - kap * qs.sum()))) / scale
    rs = _std_ratio(sd, _std_of(Ds[-1], kap), dtype)
    eta = ETA1['iv'][dtype]
    print('select_iv %s %s: picks %s, pick shortfall %.3g eps, red error %.3g eps, ivar error %.3g eps (ETA = %.3g eps), std_after at all '
          'rows: ratio to the bound %.3g' % (dtype, label, idx.tolist(), pick / EPS[dtype], rerr / EPS[dtype], ierr / EPS[dtype],
                                             eta / EPS[dtype], rs))
    assert pick <= eta and rerr <= eta
    assert abs(ivar[0] - red.sum() - ivar[1]) <= 1e-12 * ivar[0]
    assert sd.shape == (T,) and np.all(np.isfinite(sd)) and rs <= 1.0
    return ierr


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('T', ROWS_T)
def test_rows_select_iv_every_row_eligible(T, dtype):
    D, S, M, N0 = ROWS_SHAPE
    params, Xp, Li, C, w, Qm = _rows(T)
    eng = _engine(D, S, M, dtype, params)
    out = eng.select_iv(Xp, Li, ROWS_M, return_std=True)
    eng.close()
    ierr = _iv_near_optimal(C, Qm, None, R.kappa(params), dtype, out, 'T = %d, every row eligible' % T)
    if dtype == 'f64':
        assert ierr <= EPS['f64']                               # tr(Q) summed over 32 chunks of the pool


@pytest.mark.parametrize('dtype', DTYPES)
def test_rows_select_qei(dtype):
    """T = 2^20: 8192 records of the sweep, 32 per thread of the commit.  The pool's row with the best one-point score is moved into the
    last 128-row block, where it is the one row of positive weight: the reference's first pick"""
    T, ns, m = 1 << 20, 7, 8
    eng, params, alpha, Li = _synthetic(3, 1, 20, dtype)
    Xs = synth.make_X(101, T, 3)
    F = eng.sample(Xs, alpha, Li, ns, seed=9, noise=False)
    # the median over the samples of their 99.99 % quantile over the pool.  The seven sample functions of this posterior peak in two
    # rows of the pool: two picks gain, and the other six are ties at an exact 0 among a million rows, which go to the lowest indices
    # through 32 records per thread of the commit (against the median of the column maxima one pick gains)
    best = float(np.median(np.quantile(F, 0.9999, axis=0)))
    top, home = int(np.argmax(Q.scores(F, Q.start(ns, best)[1]))), T - 77
    Xs[[top, home]] = Xs[[home, top]]
    F = eng.sample(Xs, alpha, Li, ns, seed=9, noise=False)       # the device's own block of the pool as it now stands
    w = np.ones(T)
    w[T - 128:] = 0.0
    w[home] = 1.0
    ridx, rgain = Q.greedy(F, m, best, w=w)[:2]
    assert top < T - 128 and ridx[0] == home and rgain[1] > 0.0, (top, ridx, rgain)
    got = _call(eng, Xs, alpha, Li, m, ns, best, seed=9, w=w)
    eng.close()
    print('select_qei %s T = %d: the best row %d moved to %d, reference picks %s, gains %s' % (dtype, T, top, home, ridx.tolist(), rgain))
    _check_against_block(F, got, m, best, w=w)


# ---- 2. the column axis ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _synthetic_inputs(shape):
    D, S, M, T, m = shape
    params, Li, Xp = R.synthetic_problem(D, S, M, T)
    return params, Li, Xp, pred_cov_ref.factor(Xp, Li, params, S, M)


@pytest.mark.parametrize('dtype', DTYPES)
def test_select_at_its_column_bound(dtype):
    """Kp = 8192: the sweep's u_j fills 65536 B of dynamic LDS; the triangular product of the factor pass at four times the K of any
    other test"""
    D, S, M, T, m = KP_SELECT
    params, Li, Xp, C = _synthetic_inputs(KP_SELECT)
    kap = R.kappa(params)
    ref = R.select(C, m, kap=kap)
    if dtype == 'f64':
        assert ref['gap'].min() > 1e-8, 'the input itself has near-ties: no exact sequence to ask for'
    eng = _engine(D, S, M, dtype, params)
    assert eng.K == 8192
    idx, var, gain, sd = eng.select(Xp, Li, m, return_std=True)
    eng.close()
    assert len(set(idx.tolist())) == m and idx.min() >= 0 and idx.max() < T
    ds, scores = R.replay(C, None, idx)
    ar = np.arange(m)
    got = scores[ar, idx]
    assert np.all(np.isfinite(got)), 'a pick that was not eligible'
    pick = float((1.0 - got / scores.max(axis=1)).max())
    dref = ds[ar, idx]
    verr = float((np.abs(var - kap * dref) / (kap * (1.0 + dref))).max())
    rs = _std_ratio(sd, _std_of(ds[-1], kap), dtype)
    print('select %s K = 8192: same sequence as the reference: %s, smallest reference gap %.3g, pick shortfall %.3g eps, var error %.3g eps, '
          'std_after ratio to the bound %.3g' % (dtype, np.array_equal(idx, ref['idx']), ref['gap'].min(), pick / EPS[dtype],
                                                 verr / EPS[dtype], rs))
    if dtype == 'f64':
        assert np.array_equal(idx, ref['idx'])
        assert float((np.abs(var - ref['var']) / ref['var']).max()) <= EPS['f64']
        assert float((np.abs(gain - ref['gain']) / ref['gain']).max()) <= EPS['f64']
    else:
        assert pick <= ETA_SELECT and verr <= ETA_SELECT
        assert np.allclose(gain, 0.5 * np.log1p(var / kap), rtol=1e-12, atol=0)
    assert sd.shape == (T,) and np.all(np.isfinite(sd)) and rs <= 1.0


@pytest.mark.parametrize('dtype', DTYPES)
def test_select_iv_at_its_column_bound(dtype):
    """Kp = 4096: u_j and v fill 65536 B of dynamic LDS, whose head then carries the reduction"""
    D, S, M, T, m = KP_IV
    params, Li, Xp, C = _synthetic_inputs(KP_IV)
    kap = R.kappa(params)
    Qm = V.gram(C)
    eng = _engine(D, S, M, dtype, params)
    assert eng.K == 4096
    out = eng.select_iv(Xp, Li, m, return_std=True)
    eng.close()
    idx, red, var, ivar, sd = out
    if dtype == 'f64':
        ref = V.select(C, Qm, m, kap=kap)
        assert ref['gap'].min() > 1e-8, 'the input itself has near-ties: no exact sequence to ask for'
        scale = V.scale(ref, kap)
        rv = float((np.abs(var - ref['var']) / ref['var']).max())
        rr = float(np.abs(red - ref['red']).max() / scale); ri = float(np.abs(ivar - ref['ivar']).max() / scale)
        print('select_iv f64 K = 4096: smallest reference gap %.3g, var rel err %.3g, red err %.3g and ivar err %.3g of kappa max a/(1+d)' %
              (ref['gap'].min(), rv, rr, ri))
        assert np.array_equal(idx, ref['idx'])
        assert rv <= EPS['f64'] and rr <= EPS['f64'] and ri <= EPS['f64']
        assert np.all(var >= 0) and np.all(red > 0)
    _iv_near_optimal(C, Qm, None, kap, dtype, out, 'K = 4096')


def test_select_refuses_one_tile_above_its_bound():
    from scfgp_amd._lib import _c_i64_p, dptr
    from scfgp_amd.engine import HipEngine
    D, S, M = 4, 32, 4128                                       # K = Kp = 8320 = 8192 + 128
    big = HipEngine(D, S, M, dtype='f64')
    big.set_params(synth.make_params(3, D, S, M, abc=R.ABC))
    assert big.K == 8320
    idx = np.full(2, -7, np.int64); var = np.full(2, 3.0); gain = np.full(2, 3.0); sd = np.full(4, 3.0)
    rc = big.lib.scfgp_select(big.ctx, dptr(np.zeros((4, D))), 4, None, dptr(np.zeros(4)), 2, 0, idx.ctypes.data_as(_c_i64_p), dptr(var),
                              dptr(gain), dptr(sd))
    with pytest.raises(ValueError, match='K above 8192'):
        big._check(rc, 'select')
    big.close()
    assert np.all(idx == -7) and np.all(var == 3.0) and np.all(gain == 3.0) and np.all(sd == 3.0)


# ---- 3. the pick axis --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _deep_run(dtype):
    """the device's 4096 picks and its DEEP_PREFIX picks, and the Cholesky replay of the former"""
    D, S, M, T, m = DEEP
    params, Li, Xp, C = _synthetic_inputs(DEEP)
    eng = _engine(D, S, M, dtype, params)
    full = eng.select(Xp, Li, m, return_std=True)
    short = eng.select(Xp, Li, DEEP_PREFIX, return_std=False)
    eng.close()
    assert len(set(full[0].tolist())) == m and full[0].min() >= 0 and full[0].max() < T, 'the picks are not distinct rows of the pool'
    return full, short, R.replay_chol(C, None, full[0])


def deep_ratios(idx, var, replay, kap):
    """worst (best_j - got_j) / (1 + d0[p_j]) and worst |var[j] - kappa dp_j| / (kappa (1 + d0[p_j])) against the Cholesky replay"""
    ds, scores, dp = replay
    ar = np.arange(len(idx))
    got = scores[ar, idx]
    assert np.all(np.isfinite(got)), 'a pick that was not eligible'
    den = 1.0 + ds[0][idx]
    return float(((scores.max(axis=1) - got) / den).max()), float((np.abs(var - kap * dp) / (kap * den)).max())


@pytest.mark.parametrize('dtype', DTYPES)
def test_4096_picks(dtype):
    """every pick near-optimal and every var[j] right under the ABSOLUTE form |.| <= ETA_DEEP (1 + d0[p_j]), gain, std_after at all rows"""
    D, S, M, T, m = DEEP
    params, Li, Xp, C = _synthetic_inputs(DEEP)
    kap = R.kappa(params)
    (idx, var, gain, sd), short, replay = _deep_run(dtype)
    pick, verr = deep_ratios(idx, var, replay, kap)
    ds, scores, dp = replay
    rs = _std_ratio(sd, _std_of(ds[-1], kap), dtype)
    print('select %s m = 4096: d0 in [%.3g, %.3g], smallest dp %.3g, pick shortfall %.4g eps, var error %.4g eps (ETA_DEEP = %.4g eps), '
          'std_after at all rows: ratio to the bound %.3g' % (dtype, ds[0].min(), ds[0].max(), dp.min(), pick / EPS[dtype],
                                                              verr / EPS[dtype], ETA_DEEP[dtype] / EPS[dtype], rs))
    assert pick <= ETA_DEEP[dtype], ('a pick is not near-optimal in the replay', pick / EPS[dtype])
    assert verr <= ETA_DEEP[dtype], ('var outside its bound', verr / EPS[dtype])
    if dtype == 'f64':                                          # no further from the replay than 4x the reference's own recurrence
        assert max(pick, verr) <= 4.0 * max(CPU_DEEP) * EPS['f64'], ('the fp64 projection chain loses more than that', verr / EPS['f64'])
    assert np.allclose(gain, 0.5 * np.log1p(var / kap), rtol=1e-12, atol=0)
    assert sd.shape == (T,) and np.all(np.isfinite(sd)) and rs <= 1.0


@pytest.mark.parametrize('dtype', DTYPES)
def test_4096_picks_prefix(dtype):
    full, short, replay = _deep_run(dtype)
    for u, v in zip(short, full[:3]):
        assert u.shape == (DEEP_PREFIX,) and np.array_equal(u, v[:DEEP_PREFIX])
