"""Argument checks of the posterior and pool entry points that stand before "parameters not set", in source order, on a context that
needs no GPU: without one scfgp_create returns -2 (HIP error) and still hands back the context, with its geometry and nothing else.  Every
case asserts the status and the whole text of scfgp_last_error; the texts are written out here, not derived.  The checks behind
"parameters not set" are in tests/test_gpu_api_errors.py."""
import ctypes as C

import numpy as np
import pytest

from scfgp_amd import _lib
from scfgp_amd._lib import dptr

D, S, M = 4, 2, 3
K = 2 * (S + M)
EARG = -1
I64 = _lib._c_i64_p

X = np.zeros((1, D)); Y = np.zeros(1); A = np.zeros(K); L = np.eye(K); O = np.zeros(64); W1 = np.ones(1); WK = np.zeros((K, 1))
IDX = np.zeros(8, dtype=np.int64)
Z3 = np.array([-1.0, 0.0, 1.0])
x, y, a, l, o, w1, wk, z3 = (dptr(v) for v in (X, Y, A, L, O, W1, WK, Z3))
idx = IDX.ctypes.data_as(I64)
N_ = None


_KEEP = []                                    # the arrays behind the pointers of _dims


def _dims(*v):
    _KEEP.append(np.array(v, dtype=np.int32))
    return _KEEP[-1].ctypes.data_as(C.POINTER(C.c_int))


# (entry point, arguments behind the context, expected text); the status is SCFGP_EARG throughout
CASES = [
    ('predict', (N_, 1, a, l, o, o), 'predict: bad arguments'),
    ('predict', (x, 0, a, l, o, o), 'predict: bad arguments'),
    ('predict', (x, 1, a, l, o, o), 'predict: parameters not set'),
    ('predict_raw', (x, 1, N_, l, o, o), 'predict: bad arguments'),
    ('predict_raw', (x, 1, a, l, o, o), 'predict: parameters not set'),
    ('predict_y', (x, 1, a, l, N_, o, o, N_), 'predict_y: scalers not set'),
    ('predict_grad', (x, 1, a, l, 3, o, o, o, N_), 'predict_grad: bad arguments'),
    ('predict_grad', (x, 1, a, l, 0, o, o, N_, N_), 'predict_grad: bad arguments'),
    ('predict_grad', (x, 1, a, l, 1, o, o, o, N_), 'predict_grad: no X scaler set'),
    ('predict_grad', (x, 1, a, l, 2, o, o, o, N_), 'predict_grad: no X scaler set'),
    ('predict_grad', (x, 1, a, l, 0, o, o, o, N_), 'predict: parameters not set'),
    ('sample_weights', (a, l, 1, 0, N_), 'sample_weights: bad arguments'),
    ('sample_weights', (a, l, 0, 0, o), 'sample_weights: nsamp must lie in 1..1024'),
    ('sample_weights', (a, l, 1025, 0, o), 'sample_weights: nsamp must lie in 1..1024'),
    ('sample_weights', (a, l, 1, 0, o), 'sample_weights: parameters not set'),
    ('sample', (x, 0, a, l, 1, 0, 0, 0, o), 'sample: bad arguments'),
    ('sample', (x, 1, a, l, 1, 0, 3, 0, o), 'sample: bad arguments'),
    ('sample', (x, 1, a, l, 0, 0, 0, 0, o), 'sample: nsamp must lie in 1..1024'),
    ('sample', (x, 1, a, l, 1, 0, 1, 0, o), 'sample: no X scaler set'),
    ('sample', (x, 1, a, l, 1, 0, 2, 0, o), 'sample: no X scaler set'),
    ('sample', (x, 1, a, l, 1, 0, 0, 0, o), 'sample: parameters not set'),
    ('sample_argmax', (x, 1, N_, a, l, 1, 0, 0, 0, N_, o), 'sample_argmax: bad arguments'),
    ('sample_argmax', (x, 1, N_, a, l, 1025, 0, 0, 0, idx, o), 'sample_argmax: nsamp must lie in 1..1024'),
    ('sample_argmax', (x, 1, N_, a, l, 1, 0, 1, 0, idx, o), 'sample_argmax: no X scaler set'),
    ('sample_argmax', (x, 1, N_, a, l, 1, 0, 2, 0, idx, o), 'sample_argmax: no X scaler set'),
    ('sample_argmax', (x, 1, w1, a, l, 1, 0, 0, 0, idx, o), 'sample_argmax: parameters not set'),
    ('sample_grad', (x, 1, wk, 1, N_, 0, o, N_), 'sample_grad: bad arguments'),
    ('sample_grad', (x, 1, wk, 0, N_, 0, o, o), 'sample_grad: nsamp must lie in 1..1024'),
    ('sample_grad', (x, 1, wk, 1, N_, 1, o, o), 'sample_grad: no X scaler set'),
    ('sample_grad', (x, 1, wk, 1, N_, 2, o, o), 'sample_grad: no X scaler set'),
    ('sample_grad', (x, 1, wk, 1, N_, 0, o, o), 'sample_grad: parameters not set'),
    # acquire(Xs, T, w, alpha, Li, kind, par, npar, fstar, nstar, mode, noise, minimize, acq, idx, val, mu, sd, grad)
    ('acquire', (N_, 1, N_, a, l, 0, o, 1, N_, 0, 0, 0, 0, o, N_, N_, N_, N_, N_), 'acquire: NULL Xs, alpha or Li'),
    ('acquire', (x, 0, N_, a, l, 0, o, 1, N_, 0, 0, 0, 0, o, N_, N_, N_, N_, N_), 'acquire: T must be at least 1'),
    ('acquire', (x, 0, N_, a, l, 5, o, 1, N_, 0, 0, 0, 0, o, N_, N_, N_, N_, N_), 'acquire: T must be at least 1'),      # kind = 5 and T = 0
    ('acquire', (x, 1, N_, a, l, 5, o, 1, N_, 0, 0, 0, 0, o, N_, N_, N_, N_, N_), 'acquire: kind must lie in 0..4'),
    ('acquire', (x, 1, N_, a, l, 0, o, 1, N_, 0, 2, 0, 0, o, N_, N_, N_, N_, N_), 'acquire: mode must be 0 or 1 (there is no raw-y mode)'),
    ('acquire', (x, 1, N_, a, l, 2, o, 1, N_, 0, 0, 0, 0, o, N_, N_, N_, N_, N_), 'acquire: npar does not match the kind'),
    ('acquire', (x, 1, N_, a, l, 2, N_, 2, N_, 0, 0, 0, 0, o, N_, N_, N_, N_, N_), 'acquire: NULL par'),
    ('acquire', (x, 1, N_, a, l, 4, N_, 0, N_, 1, 0, 0, 0, o, N_, N_, N_, N_, N_), 'acquire: MES needs fstar with 1 <= nstar <= 1024'),
    ('acquire', (x, 1, N_, a, l, 4, N_, 0, o, 1025, 0, 0, 0, o, N_, N_, N_, N_, N_), 'acquire: MES needs fstar with 1 <= nstar <= 1024'),
    ('acquire', (x, 1, N_, a, l, 0, o, 1, o, 1, 0, 0, 0, o, N_, N_, N_, N_, N_), 'acquire: fstar given for a kind other than MES'),
    ('acquire', (x, 1, N_, a, l, 0, o, 1, N_, 0, 0, 0, 0, N_, N_, N_, o, o, N_), 'acquire: no output requested (acq, idx and grad are all NULL)'),
    ('acquire', (x, 1, N_, a, l, 0, o, 1, N_, 0, 0, 0, 0, o, N_, o, N_, N_, N_), 'acquire: val without idx'),
    ('acquire', (x, 1, N_, a, l, 0, o, 1, N_, 0, 1, 0, 0, o, N_, N_, N_, N_, N_), 'acquire: no X scaler set'),
    ('acquire', (x, 1, w1, a, l, 0, o, 1, N_, 0, 0, 0, 0, o, N_, N_, N_, N_, N_), 'acquire: parameters not set'),
    # acquire_kg(Xc, T, w, Xr, R, alpha, Li, z, J, mode, noise, minimize, kg, kg_hi, idx, val, m, s)
    ('acquire_kg', (x, 1, N_, N_, 0, a, l, N_, 3, 0, 1, 0, o, N_, N_, N_, N_, N_), 'acquire_kg: NULL Xc, alpha, Li or z'),
    ('acquire_kg', (x, 0, N_, N_, 0, a, l, z3, 3, 0, 1, 0, o, N_, N_, N_, N_, N_), 'acquire_kg: T must be at least 1'),
    ('acquire_kg', (x, 32769, N_, N_, 0, a, l, z3, 3, 0, 1, 0, o, N_, N_, N_, N_, N_),
     'acquire_kg: the symmetric form (Xr == NULL) takes 1..32768 rows'),
    ('acquire_kg', (x, 1, N_, x, 0, a, l, z3, 3, 0, 1, 0, o, N_, N_, N_, N_, N_), 'acquire_kg: R must lie in 1..32768'),
    ('acquire_kg', (x, 1, N_, x, 32769, a, l, z3, 3, 0, 1, 0, o, N_, N_, N_, N_, N_), 'acquire_kg: R must lie in 1..32768'),
    ('acquire_kg', (x, 1, N_, x, 0, a, l, z3, 2, 0, 1, 0, o, N_, N_, N_, N_, N_), 'acquire_kg: R must lie in 1..32768'),           # J = 2 and R = 0
    ('acquire_kg', (x, 1, N_, N_, 0, a, l, z3, 2, 0, 1, 0, o, N_, N_, N_, N_, N_), 'acquire_kg: J must lie in 3..32'),
    ('acquire_kg', (x, 1, N_, N_, 0, a, l, z3, 33, 0, 1, 0, o, N_, N_, N_, N_, N_), 'acquire_kg: J must lie in 3..32'),
    ('acquire_kg', (x, 1, N_, N_, 0, a, l, z3, 3, 2, 1, 0, o, N_, N_, N_, N_, N_), 'acquire_kg: mode must be 0 or 1 (there is no raw-y mode)'),
    ('acquire_kg', (x, 1, N_, N_, 0, a, l, z3, 3, 0, 1, 0, N_, N_, N_, N_, N_, N_),
     'acquire_kg: no output requested (kg, kg_hi, idx, m and s are all NULL)'),
    ('acquire_kg', (x, 1, N_, N_, 0, a, l, z3, 3, 0, 1, 0, o, N_, N_, o, N_, N_), 'acquire_kg: val without idx'),
    ('acquire_kg', (x, 1, N_, N_, 0, a, l, z3, 3, 1, 1, 0, o, N_, N_, N_, N_, N_), 'acquire_kg: no X scaler set'),
    ('acquire_kg', (x, 1, w1, N_, 0, a, l, z3, 3, 0, 1, 0, o, N_, N_, N_, N_, N_), 'acquire_kg: parameters not set'),
    # predict_cov(Xa, Ta, Xb, Tb, Li, mode, noise, cov)
    ('predict_cov', (x, 1, N_, 0, l, 0, 0, N_), 'predict_cov: bad arguments'),
    ('predict_cov', (x, 1, N_, 0, l, 2, 0, o), 'predict_cov: bad arguments'),
    ('predict_cov', (x, 0, N_, 0, l, 0, 0, o), 'predict_cov: Ta must be at least 1'),
    ('predict_cov', (x, 32769, N_, 0, l, 0, 0, o), 'predict_cov: the symmetric form takes 1..32768 rows'),
    ('predict_cov', (x, 1, x, 0, l, 0, 0, o), 'predict_cov: Tb must lie in 1..32768'),
    ('predict_cov', (x, 1, x, 32769, l, 0, 0, o), 'predict_cov: Tb must lie in 1..32768'),
    ('predict_cov', (x, 1, x, 1, l, 0, 1, o), 'predict_cov: noise is defined for the symmetric form (Xb == NULL) only'),
    ('predict_cov', (x, 1, N_, 0, l, 1, 0, o), 'predict_cov: no X scaler set'),
    ('predict_cov', (x, 1, N_, 0, l, 0, 0, o), 'predict_cov: parameters not set'),
    # condition(Xn, yn, n, alpha, Li, mode, alpha_out, Li_out)
    ('condition', (x, N_, 1, a, l, 0, o, o), 'condition: bad arguments'),
    ('condition', (x, y, 1, a, l, 2, o, o), 'condition: bad arguments'),
    ('condition', (x, y, 0, a, l, 0, o, o), 'condition: n must be at least 1'),
    ('condition', (x, y, 1, a, l, 1, o, o), 'condition: no X scaler set'),
    ('condition', (x, y, 1, a, l, 0, o, o), 'condition: parameters not set'),
    # forget(Xo, yo, n, alpha, Li, mode, alpha_out, Li_out, mu, sd, stats)
    ('forget', (x, y, 1, N_, l, 0, o, o, N_, N_, N_), 'forget: bad arguments'),
    ('forget', (x, y, 1, a, l, 0, o, N_, N_, N_, N_), 'forget: alpha_out and Li_out go together'),
    ('forget', (x, y, 1, a, l, 0, o, o, o, N_, N_), 'forget: mu and std go together'),
    ('forget', (x, y, 1, a, l, 0, o, o, N_, N_, o), 'forget: stats need mu and std'),
    ('forget', (x, y, 1, a, l, 0, N_, N_, N_, N_, N_), 'forget: no output asked for'),
    ('forget', (x, y, 0, a, l, 0, o, o, N_, N_, N_), 'forget: n must be at least 1'),
    ('forget', (x, y, 1, a, l, 1, o, o, N_, N_, N_), 'forget: no X scaler set'),
    ('forget', (x, y, 1, a, l, 0, o, o, N_, N_, N_), 'forget: parameters not set'),
    # loo(X, y, n, alpha, Li, mode, block, mu, sd, lev, stats)
    ('loo', (x, N_, 1, a, l, 0, 1, o, o, N_, N_), 'loo: bad arguments'),
    ('loo', (x, y, 1, a, l, 0, 0, o, o, N_, N_), 'loo: block must lie in 1..64'),
    ('loo', (x, y, 1, a, l, 0, 65, o, o, N_, N_), 'loo: block must lie in 1..64'),
    ('loo', (N_, N_, 1, a, l, 1, 1, o, o, N_, N_), 'loo: resident rows are scaled rows (mode must be 0)'),
    ('loo', (N_, N_, 1, a, l, 0, 1, o, o, N_, N_), 'loo: no resident rows (scfgp_set_data)'),
    ('loo', (x, y, 0, a, l, 0, 1, o, o, N_, N_), 'loo: n must be at least 1'),
    ('loo', (x, y, 1, a, l, 1, 1, o, o, N_, N_), 'loo: no X scaler set'),
    ('loo', (x, y, 1, a, l, 0, 1, o, o, N_, N_), 'loo: parameters not set'),
    # predict_gradcov(Xs, T, w, alpha, Li, mode, dmu, dvar, dcov, asub)
    ('predict_gradcov', (x, 0, N_, a, l, 0, o, N_, N_, N_), 'predict_gradcov: bad arguments'),
    ('predict_gradcov', (x, 1, N_, a, l, 0, N_, N_, N_, N_), 'predict_gradcov: no output requested'),
    ('predict_gradcov', (x, 1, N_, a, l, 1, o, N_, N_, N_), 'predict_gradcov: no X scaler set'),
    ('predict_gradcov', (x, 1, w1, a, l, 0, o, N_, N_, o), 'predict_gradcov: parameters not set'),
    # predict_pd(Xs, T, w, alpha, Li, dims, ndim, grid, G, mode, pd, pd_sd, pd_cov, ice)
    ('predict_pd', (x, 1, N_, a, l, _dims(0), 1, N_, 1, 0, o, N_, N_, N_), 'predict_pd: bad arguments'),
    ('predict_pd', (x, 1, N_, a, l, _dims(0), 1, o, 1, 0, N_, N_, N_, N_), 'predict_pd: no output requested'),
    ('predict_pd', (x, 0, N_, a, l, _dims(0), 1, o, 1, 0, o, N_, N_, N_), 'predict_pd: T must be at least 1'),
    ('predict_pd', (x, 1, N_, a, l, _dims(0), 1, o, 0, 0, o, N_, N_, N_), 'predict_pd: G must lie in 1..1024'),
    ('predict_pd', (x, 1, N_, a, l, _dims(1, 1), 2, o, 0, 0, o, N_, N_, N_), 'predict_pd: G must lie in 1..1024'),     # a repeated dimension and G = 0
    ('predict_pd', (x, 1, N_, a, l, _dims(0), 1, o, 1025, 0, o, N_, N_, N_), 'predict_pd: G must lie in 1..1024'),
    ('predict_pd', (x, 1, N_, a, l, _dims(0), 0, o, 1, 0, o, N_, N_, N_), 'predict_pd: ndim must lie in 1..D'),
    ('predict_pd', (x, 1, N_, a, l, _dims(0, 1, 2, 3, 0), 5, o, 1, 0, o, N_, N_, N_), 'predict_pd: ndim must lie in 1..D'),
    ('predict_pd', (x, 1, N_, a, l, _dims(0), 1, o, 1, 2, o, N_, N_, N_), 'predict_pd: bad mode'),
    ('predict_pd', (x, 1, N_, a, l, _dims(0, 7), 2, o, 1, 0, o, N_, N_, N_), 'predict_pd: dimension 7 is out of range'),
    ('predict_pd', (x, 1, N_, a, l, _dims(-1), 1, o, 1, 0, o, N_, N_, N_), 'predict_pd: dimension -1 is out of range'),
    ('predict_pd', (x, 1, N_, a, l, _dims(1, 1), 2, o, 1, 0, o, N_, N_, N_), 'predict_pd: dimension 1 is given twice'),
    ('predict_pd', (x, 1, N_, a, l, _dims(0), 1, o, 1, 1, o, N_, N_, N_), 'predict_pd: no X scaler set'),
    ('predict_pd', (x, 1, w1, a, l, _dims(0), 1, o, 1, 0, o, N_, N_, N_), 'predict_pd: parameters not set'),
    # select(Xc, T, w, Li, m, mode, idx, var, gain, std_after)
    ('select', (x, 1, N_, l, 1, 0, N_, N_, N_, N_), 'select: bad arguments'),
    ('select', (x, 1, N_, l, 0, 2, idx, N_, N_, N_), 'select: bad arguments'),                                       # m = 0 and mode = 2
    ('select', (x, 0, N_, l, 1, 0, idx, N_, N_, N_), 'select: T must lie in 1..1048576'),
    ('select', (x, 1048577, N_, l, 1, 0, idx, N_, N_, N_), 'select: T must lie in 1..1048576'),
    ('select', (x, 1, N_, l, 0, 0, idx, N_, N_, N_), 'select: m must lie in 1..4096'),
    ('select', (x, 1, N_, l, 4097, 0, idx, N_, N_, N_), 'select: m must lie in 1..4096'),
    ('select', (x, 1, N_, l, 1, 1, idx, N_, N_, N_), 'select: no X scaler set'),
    ('select', (x, 1, w1, l, 1, 0, idx, N_, N_, N_), 'select: parameters not set'),
    # select_iv(Xc, T, w, Xr, R, wr, Li, m, mode, idx, red, var, ivar, std_after)
    ('select_iv', (x, 1, N_, N_, 0, N_, N_, 1, 0, idx, N_, N_, N_, N_), 'select_iv: bad arguments'),
    ('select_iv', (x, 0, N_, N_, 0, N_, l, 1, 0, idx, N_, N_, N_, N_), 'select_iv: T must lie in 1..1048576'),
    ('select_iv', (x, 1, N_, N_, 0, N_, l, 0, 0, idx, N_, N_, N_, N_), 'select_iv: m must lie in 1..4096'),
    ('select_iv', (x, 1, N_, x, 0, N_, l, 1, 0, idx, N_, N_, N_, N_), 'select_iv: R must be at least 1'),
    ('select_iv', (x, 1, N_, N_, 0, N_, l, 1, 1, idx, N_, N_, N_, N_), 'select_iv: no X scaler set'),
    ('select_iv', (x, 1, w1, N_, 0, w1, l, 1, 0, idx, N_, N_, N_, N_), 'select_iv: parameters not set'),
    # select_qei(Xc, T, w, Xp, np, alpha, Li, nsamp, seed, best, xi, m, mode, minimize, idx, gain, score0, mstate, qei)
    ('select_qei', (x, 1, N_, N_, 0, a, l, 1, 0, 0.0, 0.0, 1, 0, 0, N_, N_, N_, N_, N_), 'select_qei: NULL Xc, alpha, Li or idx'),
    ('select_qei', (x, 0, N_, N_, 0, a, l, 1, 0, 0.0, 0.0, 1, 0, 0, idx, N_, N_, N_, N_), 'select_qei: T must lie in 1..1048576'),
    ('select_qei', (x, 1, N_, N_, 0, a, l, 1, 0, 0.0, 0.0, 0, 0, 0, idx, N_, N_, N_, N_), 'select_qei: m must lie in 1..4096'),
    ('select_qei', (x, 1, N_, N_, 0, a, l, 0, 0, 0.0, 0.0, 1, 0, 0, idx, N_, N_, N_, N_), 'select_qei: nsamp must lie in 1..1024'),
    ('select_qei', (x, 1, N_, N_, 0, a, l, 1, 0, 0.0, 0.0, 1, 2, 0, idx, N_, N_, N_, N_),
     'select_qei: mode must be 0 or 1 (there is no raw-y mode)'),
    ('select_qei', (x, 1, N_, N_, -1, a, l, 1, 0, 0.0, 0.0, 1, 0, 0, idx, N_, N_, N_, N_), 'select_qei: np must not be negative'),
    ('select_qei', (x, 1, N_, N_, 1, a, l, 1, 0, 0.0, 0.0, 1, 0, 0, idx, N_, N_, N_, N_), 'select_qei: np > 0 with NULL Xp'),
    ('select_qei', (x, 1, N_, N_, 0, a, l, 1, 0, 0.0, 0.0, 1, 1, 0, idx, N_, N_, N_, N_), 'select_qei: no X scaler set'),
    ('select_qei', (x, 1, w1, N_, 0, a, l, 1, 0, 0.0, -1.0, 1, 0, 0, idx, N_, N_, N_, N_), 'select_qei: parameters not set'),
]


@pytest.fixture(scope='module')
def ctx():
    lib = _lib.load()
    c = C.c_void_p()
    rc = lib.scfgp_create(C.byref(c), D, S, M, 0, 0, None)
    assert rc in (0, -2) and c.value            # -2 without a GPU: the context is there all the same
    yield lib, c
    lib.scfgp_destroy(c)


def test_every_entry_point_is_covered():
    names = {n for n, _, _ in CASES}
    assert names == {'predict', 'predict_raw', 'predict_y', 'predict_grad', 'sample_weights', 'sample', 'sample_argmax', 'sample_grad',
                     'acquire', 'acquire_kg', 'predict_cov', 'condition', 'forget', 'loo', 'predict_gradcov', 'predict_pd', 'select',
                     'select_iv', 'select_qei'}


@pytest.mark.parametrize('case', range(len(CASES)), ids=['%s-%d' % (c[0], i) for i, c in enumerate(CASES)])
def test_refusal(ctx, case):
    lib, c = ctx
    name, args, text = CASES[case]
    rc = getattr(lib, 'scfgp_' + name)(c, *args)
    assert rc == EARG
    assert lib.scfgp_last_error(c).decode() == text


@pytest.mark.parametrize('name', sorted({c[0] for c in CASES}))
def test_null_context(name):
    lib = _lib.load()
    args = next(a for n, a, _ in CASES if n == name)
    assert getattr(lib, 'scfgp_' + name)(None, *args) == EARG
