"""CPU tier of the posterior sample functions (scfgp_sample, scfgp_sample_weights): the numpy restatement of the generator
(tests/sample_ref.py) against Random123's known answer and numpy's Philox, the moments of its normals, the semantics of the samples
(mean, covariance and noisy marginals against the oracle's pred_func), and the C entry points' argument checks (no GPU needed)."""
import ctypes

import numpy as np

from oracle import scfgp_oracle as O
from scfgp_amd import _lib
from tests import sample_ref as R


def test_philox_known_answer():
    w = R.philox4x64_10(0, 0, 0, 0, 0, 0)
    assert [int(x) for x in w] == [0x16554d9eca36314c, 0xdb20fe9d672d0fdc, 0xd7e772cee186176b, 0x7e68b68aec7ba23b]


def test_philox_equals_numpy_at_the_next_counter():
    """numpy.random.Philox(counter=c, key=k).random_raw(4) is the block at counter c + 1 (it increments before it draws)."""
    rng = np.random.default_rng(11)
    for _ in range(5):
        c = [int(x) for x in rng.integers(0, 2 ** 63, 4, dtype=np.uint64)]
        k = [int(x) for x in rng.integers(0, 2 ** 63, 2, dtype=np.uint64)]
        ref = np.random.Philox(counter=c, key=k).random_raw(4)
        mine = R.philox4x64_10(c[0] + 1, c[1], c[2], c[3], k[0], k[1])
        assert [int(x) for x in ref] == [int(x) for x in mine]


def test_normals_moments():
    n_idx, ns = 15625, 64                                   # 10^6 normals
    z = R.normals(np.arange(n_idx), ns, seed=2024, stream=0)
    n = z.size
    x = z.ravel()
    assert abs(x.mean()) < 5 / np.sqrt(n)
    assert abs(x.var() - 1) < 5 * np.sqrt(2 / n)
    assert abs((x ** 4).mean() - 3) < 5 * np.sqrt(96 / n)
    # sample s and s + 1 share a Box-Muller pair for even s (cos / sin) or come from neighbouring pairs: uncorrelated either way
    for s in (0, 1, 2, 3):
        r = np.corrcoef(z[:, s], z[:, s + 1])[0, 1]
        assert abs(r) < 5 / np.sqrt(n_idx)
    # the noise stream is another sequence
    assert not np.array_equal(R.normals(np.arange(8), 8, 2024, 1), z[:8, :8])


def test_sample_does_not_depend_on_nsamp_or_rows():
    a = R.normals(np.arange(10, 20), 13, seed=5, stream=1)
    b = R.normals(np.arange(20), 5, seed=5, stream=1)
    assert np.array_equal(a[:, :5], b[10:20])


def _problem(D=3, S=2, M=12, N=200, seed=3):
    rng = np.random.default_rng(seed)
    params = O.init_params(D, S, M, rng)
    params[:3] = (-1.0, 0.0, -1.0)
    X = rng.uniform(0, 1, (N, D))
    y = np.sin(3 * X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))
    _, alpha, Li = O.forward(X, y, params, S, M, gauss_hermite=False)
    return params, alpha, Li, rng.uniform(-0.2, 1.2, (50, D)), S, M


def test_samples_have_the_posterior_moments():
    params, alpha, Li, Xs, S, M = _problem()
    ns = 4096
    f = R.samples(Xs, alpha, Li, params, S, M, ns, seed=77)
    mu, sd = O.predict(Xs, alpha, Li, params, S, M)
    kap = R.kappa(params)
    Phi = O.feature_map(Xs, params, Xs.shape[1], S, M)
    Ainv = Li.T @ Li
    C = kap * Phi @ Ainv @ Phi.T                          # kappa Phi* A^-1 Phi*^T
    assert np.allclose(np.diag(C), sd ** 2 - kap, rtol=1e-10, atol=1e-14)
    # mean: within 5 CLT standard errors of mu*
    se = np.sqrt(np.diag(C) / ns)
    assert np.max(np.abs(f.mean(1) - mu.ravel()) / se) < 5
    # covariance: element-wise standard error of the estimate sqrt((C_ii C_jj + C_ij^2) / n)
    Ce = np.cov(f)
    se_c = np.sqrt((np.outer(np.diag(C), np.diag(C)) + C ** 2) / ns)
    assert np.max(np.abs(Ce - C) / se_c) < 5
    # observation noise: the marginal is pred_func's N(mu*, sigma*^2)
    y = R.samples(Xs, alpha, Li, params, S, M, ns, seed=77, noise=True)
    v = y.var(1, ddof=1)
    assert np.max(np.abs(v - sd ** 2) / (sd ** 2 * np.sqrt(2 / (ns - 1)))) < 5
    assert np.max(np.abs(y.mean(1) - mu.ravel()) / (sd / np.sqrt(ns))) < 5


def test_sample_entry_points_declared_exported_and_checked_without_gpu():
    """scfgp_sample and scfgp_sample_weights are in the header, the library and the binding table, and refuse bad arguments before
    touching a device."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'scfgp_hip.h')).read(), flags=re.S)
    for name in ('scfgp_sample', 'scfgp_sample_weights'):
        assert re.search(r'\b%s\s*\(' % name, header)
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    fs, fw = lib.scfgp_sample, lib.scfgp_sample_weights
    assert len(fs.argtypes) == 10 and len(fw.argtypes) == 6
    D, S, M = 3, 2, 5
    K = 2 * (S + M)
    Xs = np.zeros((4, D)); alpha = np.zeros(K); Li = np.eye(K); out = np.empty((4, 8)); W = np.empty((K, 8))
    p = _lib.dptr
    assert fs(None, p(Xs), 4, p(alpha), p(Li), 8, 0, 0, 0, p(out)) == -1
    assert fw(None, p(alpha), p(Li), 8, 0, p(W)) == -1
    ctx = ctypes.c_void_p()
    lib.scfgp_create(ctypes.byref(ctx), D, S, M, 0, 0, None)        # fails on a GPU-less box but hands back its context
    assert ctx.value
    try:
        err = lambda: lib.scfgp_last_error(ctx)
        for T in (0, -3):
            assert fs(ctx, p(Xs), T, p(alpha), p(Li), 8, 0, 0, 0, p(out)) == -1
        assert b'bad arguments' in err()
        for mode in (-1, 3, 9):
            assert fs(ctx, p(Xs), 4, p(alpha), p(Li), 8, 0, mode, 0, p(out)) == -1
        assert fs(ctx, None, 4, p(alpha), p(Li), 8, 0, 0, 0, p(out)) == -1
        assert fs(ctx, p(Xs), 4, p(alpha), p(Li), 8, 0, 0, 0, None) == -1
        assert fw(ctx, None, p(Li), 8, 0, p(W)) == -1
        assert fw(ctx, p(alpha), p(Li), 8, 0, None) == -1
        assert b'bad arguments' in err()
        for ns in (0, -1, 1025):
            assert fs(ctx, p(Xs), 4, p(alpha), p(Li), ns, 0, 0, 0, p(out)) == -1
            assert b'nsamp' in err()
            assert fw(ctx, p(alpha), p(Li), ns, 0, p(W)) == -1
            assert b'nsamp' in err()
        assert fs(ctx, p(Xs), 4, p(alpha), p(Li), 8, 0, 1, 0, p(out)) == -1      # no X scaler registered
        assert b'scaler' in err()
        assert fs(ctx, p(Xs), 4, p(alpha), p(Li), 8, 0, 0, 0, p(out)) == -1      # parameters not set
        assert b'parameters' in err()
        assert fw(ctx, p(alpha), p(Li), 8, 2 ** 64 - 1, p(W)) == -1
        assert b'parameters' in err()
    finally:
        lib.scfgp_destroy(ctx)
