"""CPU tier of the leave-block-out predictions (scfgp_loo): the numpy form (tests/loo_ref.py) from ONE oracle fit on all rows against
the oracle refitted once per block on the other rows, every row under the project's fp64 predictive bound (tests/parity.py, unchanged);
its closed form at block 1; the joint log density against the refits' joint Gaussians; permutations inside a block; and the C entry
point without a context (no GPU needed).  These tests pin the reference the GPU tier is judged against."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import scfgp_oracle as O
from scfgp_amd import _lib
from tests import loo_ref as R
from tests import parity


@functools.lru_cache(maxsize=None)
def _fit(shape, abc):
    D, S, M, N, block = shape
    params, X, y = R.problem(D, S, M, N, abc)
    _, alpha, Li = O.forward(X, y, params, S, M, gauss_hermite=False)
    return params, X, y, alpha, Li


@pytest.mark.parametrize('shape,abc', R.CASES)
def test_loo_ref_equals_the_oracle_refitted_per_block(shape, abc):
    D, S, M, N, block = shape
    params, X, y, alpha, Li = _fit(shape, abc)
    ref = R.loo(X, y, alpha, Li, params, S, M, block)
    mu0, sd0 = R.refit(X, y, params, S, M, block)
    print('loo_ref %s abc %s: ratio %.3g, max eigenvalue of H over the blocks %.3g' %
          (shape, abc, parity.predict_ratio(ref['mu'], ref['std'], mu0, sd0, 'f64'), ref['lmax'].max()))
    assert ref['lmax'].max() < 1.0 and len(ref['joint']) == -(-N // block)
    parity.check_predict(ref['mu'], ref['std'], mu0, sd0, 'f64')             # every row of every block
    # the check has teeth: the in-sample prediction of the fit on all rows misses even the fp32 bound
    mu_in, sd_in = O.predict(X, alpha, Li, params, S, M)
    assert parity.predict_ratio(mu_in, sd_in, mu0, sd0, 'f32') > 1.0


@pytest.mark.parametrize('shape,abc', [c for c in R.CASES if c[0][4] == 1])
def test_block_one_is_the_textbook_closed_form(shape, abc):
    D, S, M, N, block = shape
    params, X, y, alpha, Li = _fit(shape, abc)
    ref = R.loo(X, y, alpha, Li, params, S, M, 1)
    Phi = O.feature_map(X, params, D, S, M)
    h = np.sum((Phi @ np.tril(Li).T) ** 2, axis=1)
    r = y.ravel() - (Phi @ alpha).ravel()
    kap = R.kappa(params)
    assert np.allclose(ref['lev'], h, rtol=1e-12, atol=0)
    assert np.allclose(ref['e'], r / (1 - h), rtol=1e-11, atol=1e-14)
    assert np.allclose(ref['std'] ** 2, kap / (1 - h), rtol=1e-12, atol=0)
    # a block of one row: its joint density is its marginal
    assert np.allclose(ref['joint'], ref['marg'], rtol=1e-11, atol=1e-12)
    assert abs(ref['stats'][4] - ref['stats'][3]) <= 1e-11 * np.sum(np.abs(ref['marg']))
    assert ref['stats'][0] == N and ref['stats'][6] == N and ref['stats'][5] == ref['lev'].max()


@pytest.mark.parametrize('shape,abc', [R.CASES[1], R.CASES[5], R.CASES[2]])
def test_joint_log_density_equals_that_of_the_refits_joint_gaussian(shape, abc):
    D, S, M, N, block = shape
    params, X, y, alpha, Li = _fit(shape, abc)
    ref = R.loo(X, y, alpha, Li, params, S, M, block)
    _, _, joint0 = R.refit(X, y, params, S, M, block, with_joint=True)
    assert joint0.shape == ref['joint'].shape
    assert np.allclose(ref['joint'], joint0, rtol=1e-8, atol=1e-8)
    assert abs(ref['stats'][4] - joint0.sum()) <= 1e-9 * np.sum(np.abs(joint0))
    # the refit's joint covariance is predict_cov's with the noise on its diagonal: kappa (I - H)^-1 = kappa (I + C_-I C_-I^T)
    from tests import pred_cov_ref
    i0, i1 = R.blocks(N, block)[1]
    keep = np.r_[0:i0, i1:N]
    _, a, L = O.forward(np.ascontiguousarray(X[keep]), np.ascontiguousarray(y[keep]), params, S, M, gauss_hermite=False)
    cov = pred_cov_ref.pred_cov(X[i0:i1], L, params, S, M, noise=True)
    C = pred_cov_ref.factor(X[i0:i1], Li, params, S, M)
    mine = R.kappa(params) * np.linalg.inv(np.eye(i1 - i0) - C @ C.T)
    assert np.allclose(mine, cov, rtol=1e-8, atol=1e-10)


def test_permuting_rows_inside_a_block_permutes_the_outputs():
    shape, abc = R.CASES[1]
    D, S, M, N, block = shape
    params, X, y, alpha, Li = _fit(shape, abc)
    ref = R.loo(X, y, alpha, Li, params, S, M, block)
    perm = np.arange(N)
    rng = np.random.default_rng(3)
    for i0, i1 in R.blocks(N, block):
        perm[i0:i1] = i0 + rng.permutation(i1 - i0)
    out = R.loo(X[perm], y[perm], alpha, Li, params, S, M, block)
    for k in ('mu', 'std', 'lev'):
        assert np.allclose(out[k], ref[k][perm], rtol=1e-11, atol=1e-13)
    assert np.allclose(out['joint'], ref['joint'], rtol=1e-11, atol=1e-12)
    # a different blocking is a different question: the answers move
    assert not np.allclose(R.loo(X, y, alpha, Li, params, S, M, 1)['mu'], ref['mu'], rtol=1e-6, atol=0)


def test_entry_point_without_a_context():
    lib = _lib.load()
    assert lib.scfgp_loo(None, None, None, 0, None, None, 0, 1, None, None, None, None) == -1
    assert _lib.SIGNATURES['scfgp_loo'][1][7] is ctypes.c_int
