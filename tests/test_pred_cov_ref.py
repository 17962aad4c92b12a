"""CPU tier of the joint posterior covariance (scfgp_predict_cov): the numpy closed form (tests/pred_cov_ref.py) pinned to things it
shares no code with -- the oracle's pred_func on the diagonal, a linear solve against A rebuilt from the training features, the
exact weight covariance of tests/sample_ref.py's weights -- and the C entry point's argument checks (no GPU needed)."""
import ctypes

import numpy as np

from oracle import scfgp_oracle as O
from scfgp_amd import _lib, synth
from tests import pred_cov_ref as R
from tests import sample_ref

# the predictive shapes of the GPU tier: K = 128, 600, 2112, an odd J, rank-S projection
SHAPES = [(5, 4, 60), (20, 20, 280), (64, 32, 1024), (3, 1, 20), (40, 4, 100)]


def _synthetic(D, S, M):
    """parameters and the synthetic Li of tests/test_gpu_sample.py's engines"""
    seed = 0x5CF65000 + M
    K = 2 * (S + M)
    params = synth.make_params(seed + 0x0202, D, S, M, abc=(-1.0, 0.0, -1.0))
    Li = np.tril(np.random.default_rng(seed).standard_normal((K, K))) / np.sqrt(K)
    return params, Li


def test_diagonal_plus_kappa_is_the_oracles_predictive_variance():
    for D, S, M in SHAPES:
        params, Li = _synthetic(D, S, M)
        Xs = synth.make_X(101, 300, D)
        _, sd = O.predict(Xs, np.zeros(2 * (S + M)), Li, params, S, M)
        cov = R.pred_cov(Xs, Li, params, S, M)
        noisy = R.pred_cov(Xs, Li, params, S, M, noise=True)
        assert np.allclose(np.diag(cov) + R.kappa(params), sd ** 2, rtol=1e-12, atol=0)
        assert np.allclose(np.diag(noisy), sd ** 2, rtol=1e-12, atol=0)
        off = ~np.eye(300, dtype=bool)
        assert np.array_equal(noisy[off], cov[off])
        assert np.array_equal(cov, cov.T)
        # the cross form on the same rows is the symmetric form; blocks of it are the cross form on subsets
        assert np.allclose(R.pred_cov(Xs, Li, params, S, M, Xb=Xs), cov, rtol=0, atol=1e-15 * np.abs(cov).max())
        assert np.allclose(R.pred_cov(Xs[10:50], Li, params, S, M, Xb=Xs[200:]), cov[10:50, 200:], rtol=0, atol=1e-13 * np.abs(cov).max())


def _fit(D=3, S=2, M=12, N=200, seed=3):
    rng = np.random.default_rng(seed)
    params = O.init_params(D, S, M, rng)
    params[:3] = (-1.0, 0.0, -1.0)
    X = rng.uniform(0, 1, (N, D))
    y = np.sin(3 * X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))
    _, alpha, Li = O.forward(X, y, params, S, M, gauss_hermite=False)
    return params, X, alpha, Li, rng.uniform(-0.2, 1.2, (50, D)), rng.uniform(-0.2, 1.2, (31, D)), S, M


def test_equals_the_linear_solve_on_an_oracle_fit():
    """kappa Phi_a A^-1 Phi_b^T with A = Phi^T Phi + (e^{2a} + 1e-6) I rebuilt from the training rows and solved by LU, against the
    factor form through the oracle's own Li = inv(cholesky(A)).  Either route to A^-1 carries a relative error of order cond(A) eps
    (the LU solve directly; Li at sqrt(cond(A)) eps per factor, both factors in the product), so the bound is 100 cond(A) eps with
    cond(A) measured in the test and required to stay below 1e6 for this configuration (lambda = e^-2 + 1e-6 under 200 rows of
    features of scale sqrt(2 / M)): a bound of at most 2.2e-8, far below the O(1) error of a wrong formula."""
    params, X, alpha, Li, Xa, Xb, S, M = _fit()
    D = X.shape[1]
    Phi = O.feature_map(X, params, D, S, M)
    A = Phi.T @ Phi + (np.exp(2 * params[0]) + 1e-6) * np.eye(Phi.shape[1])
    cond = np.linalg.cond(A)
    assert cond < 1e6
    bound = 100 * cond * np.finfo(np.float64).eps
    Pa, Pb = O.feature_map(Xa, params, D, S, M), O.feature_map(Xb, params, D, S, M)
    for other, Pother in ((Xb, Pb), (None, Pa)):
        ref = R.kappa(params) * Pa @ np.linalg.solve(A, Pother.T)
        cov = R.pred_cov(Xa, Li, params, S, M, Xb=other)
        assert np.linalg.norm(cov - ref) / np.linalg.norm(ref) < bound


def test_equals_the_exact_covariance_of_the_sampled_weights():
    """tests/sample_ref.py's weights are W = alpha 1^T + sqrt(kappa) Li^T Z: linear in Z.  With Z = I (one "sample" per unit vector) the
    columns of W - alpha are sqrt(kappa) Li^T e_k, so Cov(w) = sum_k (W - alpha)_k (W - alpha)_k^T = kappa Li^T Li exactly, and the
    function covariance is Phi_a Cov(w) Phi_b^T.  Z = I is fed to the same expression by replacing the generator."""
    params, X, alpha, Li, Xa, Xb, S, M = _fit()
    D = X.shape[1]
    K = alpha.size
    saved = sample_ref.normals
    sample_ref.normals = lambda idx, nsamp, seed, stream: np.eye(len(idx), nsamp)
    try:
        W = sample_ref.weights(alpha, Li, R.kappa(params), K, 0)
    finally:
        sample_ref.normals = saved
    Wc = W - np.asarray(alpha).reshape(-1, 1)
    cov_w = Wc @ Wc.T
    Pa, Pb = O.feature_map(Xa, params, D, S, M), O.feature_map(Xb, params, D, S, M)
    for other, Pother in ((Xb, Pb), (None, Pa)):
        ref = Pa @ cov_w @ Pother.T
        cov = R.pred_cov(Xa, Li, params, S, M, Xb=other)
        assert np.linalg.norm(cov - ref) / np.linalg.norm(ref) < 1e-12


def test_entry_point_declared_exported_and_checked_without_gpu():
    """scfgp_predict_cov is in the header, the library and the binding table, and refuses bad arguments with a message before touching
    a device."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'scfgp_hip.h')).read(), flags=re.S)
    assert re.search(r'\bscfgp_predict_cov\s*\(', header)
    assert 'scfgp_predict_cov' in _lib.SIGNATURES
    lib = _lib.load()
    f = lib.scfgp_predict_cov
    assert len(f.argtypes) == 9
    D, S, M = 3, 2, 5
    K = 2 * (S + M)
    Xa = np.zeros((4, D)); Xb = np.zeros((3, D)); Li = np.eye(K); out = np.empty((4, 4))
    p = _lib.dptr
    assert f(None, p(Xa), 4, None, 0, p(Li), 0, 0, p(out)) == -1
    ctx = ctypes.c_void_p()
    lib.scfgp_create(ctypes.byref(ctx), D, S, M, 0, 0, None)        # fails on a GPU-less box but hands back its context
    assert ctx.value
    try:
        err = lambda: lib.scfgp_last_error(ctx)
        for args in ((None, 4, None, 0, p(Li), 0, 0, p(out)), (p(Xa), 4, None, 0, None, 0, 0, p(out)), (p(Xa), 4, None, 0, p(Li), 0, 0, None),
                     (p(Xa), 4, None, 0, p(Li), -1, 0, p(out)), (p(Xa), 4, None, 0, p(Li), 2, 0, p(out))):
            assert f(ctx, *args) == -1
            assert b'bad arguments' in err()
        for Ta in (0, -2):
            assert f(ctx, p(Xa), Ta, None, 0, p(Li), 0, 0, p(out)) == -1
            assert b'Ta' in err()
            assert f(ctx, p(Xa), Ta, p(Xb), 3, p(Li), 0, 0, p(out)) == -1
            assert b'Ta' in err()
        for Tb in (0, -1, 32769):
            assert f(ctx, p(Xa), 4, p(Xb), Tb, p(Li), 0, 0, p(out)) == -1
            assert b'Tb' in err()
        assert f(ctx, p(Xa), 32769, None, 0, p(Li), 0, 0, p(out)) == -1          # the symmetric form's Tb is Ta
        assert b'32768' in err()
        assert f(ctx, p(Xa), 4, p(Xb), 3, p(Li), 0, 1, p(out)) == -1             # cross form with noise
        assert b'noise' in err()
        assert f(ctx, p(Xa), 4, None, 0, p(Li), 1, 0, p(out)) == -1              # no X scaler registered
        assert b'scaler' in err()
        assert f(ctx, p(Xa), 4, None, 0, p(Li), 0, 0, p(out)) == -1              # parameters not set
        assert b'parameters' in err()
    finally:
        lib.scfgp_destroy(ctx)
