"""CPU tier of scfgp_predict_pd: the closed form of the partial-dependence posterior and of the ICE curves (tests/pd_ref.py: the
rotation of the zeroed-column features) against brute force over the expanded rows; the PD covariance against the weighted double sum
of the joint predictive covariance (an independent route); T = 1 against the oracle's predict; the vacuity of the GPU tier's bounds
(mutations); and the C entry point's declaration and host-side argument checks (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import scfgp_oracle as O
from scfgp_amd import _lib, synth
from tests import pd_ref as R
from tests import pred_cov_ref as PC

F32_BOUND = 6e-6                                                  # the GPU tier's fp32 bound on pd, sd, cov
F32_BOUND_ICE = 3e-6


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def _case(D, S, M, T=257, G=9):
    params, alpha, Li = R.synthetic(D, S, M)
    Xs = R.points(D, T)
    w = 0.25 + synth.uniform(77, 0, T)
    dims = R.dims_for(D)
    return params, alpha, Li, Xs, w, dims, R.make_grid(Xs, dims, G)


@pytest.mark.parametrize('D,S,M', R.GEOMETRIES)
def test_closed_form_equals_brute_force(D, S, M):
    params, alpha, Li, Xs, w, dims, grid = _case(D, S, M)
    # Input condition of both tiers: the mean feature row keeps at least 0.08 of a row's norm, so pd is not a cancelled sum.  The floor
    # is the one the GPU bounds need: an fp32 rounding error of 6e-8 per term, amplified by at most 1 / 0.08, stays an eighth of the
    # 6e-6 bound.  The smallest share over the geometries is 0.0859, at (70, 5, 60) (0.0877 without the weights).
    share = R.cancellation(Xs, w, params, S, M, dims)
    print((D, S, M), '|phibar0| / |phi| = %.4f' % share)
    assert share >= 0.08
    a = R.closed(Xs, w, alpha, Li, params, S, M, dims, grid)
    b = R.brute(Xs, w, alpha, Li, params, S, M, dims, grid)
    errs = [rel(x, y) for x, y in zip(a, b)]
    print((D, S, M), 'pd %.1e sd %.1e cov %.1e ice %.1e Phibar %.1e' % tuple(errs))
    assert max(errs) < 1e-12
    # without weights, and with rows of weight zero that hold nonsense
    a = R.closed(Xs, None, alpha, Li, params, S, M, dims, grid, want_ice=False)
    b = R.brute(Xs, None, alpha, Li, params, S, M, dims, grid, want_ice=False)
    assert max(rel(x, y) for x, y in zip(a[:3], b[:3])) < 1e-12
    Xz = np.vstack([Xs, np.full((2, D), np.nan)]); wz = np.r_[w, 0.0, 0.0]
    z = R.closed(Xz, wz, alpha, Li, params, S, M, dims, grid, want_ice=False)
    c = R.closed(Xs, w, alpha, Li, params, S, M, dims, grid, want_ice=False)
    assert all(np.array_equal(x, y) for x, y in zip(z[:3], c[:3]))


def test_closed_form_equals_brute_force_over_a_long_pool():
    D, S, M = 7, 12, 3
    params, alpha, Li, Xs, w, dims, grid = _case(D, S, M, T=70000, G=3)
    a = R.closed(Xs, w, alpha, Li, params, S, M, dims[:2], grid[:2], want_ice=False)
    b = R.brute(Xs, w, alpha, Li, params, S, M, dims[:2], grid[:2], want_ice=False)
    errs = [rel(x, y) for x, y in zip(a[:3], b[:3])]
    print('T = 70000: pd %.1e sd %.1e cov %.1e' % tuple(errs))
    assert max(errs) < 1e-12


def test_pd_covariance_is_the_weighted_double_sum_of_the_joint_predictive_covariance():
    """Cov[pd_i, pd_i'] = sum_t sum_t' what_t what_t' Cov[f(x_t^{d->g_i}), f(x_t'^{d->g_i'})]: tests/pred_cov_ref.py on the expanded rows"""
    D, S, M, T, G = 7, 12, 3, 40, 5
    params, alpha, Li, Xs, w, dims, grid = _case(D, S, M, T=T, G=G)
    _, sd, cov, _, _ = R.closed(Xs, w, alpha, Li, params, S, M, dims, grid, want_ice=False)
    what = w / w.sum()
    for a, d in enumerate(dims):
        Xe = np.repeat(Xs[None, :, :], G, 0)                      # G x T x D
        Xe[:, :, d] = grid[a][:, None]
        big = PC.pred_cov(Xe.reshape(G * T, D), Li, params, S, M).reshape(G, T, G, T)
        ref = np.einsum('t,itju,u->ij', what, big, what)
        assert rel(cov[a], ref) < 1e-12
        assert rel(sd[a] ** 2, np.diag(ref)) < 1e-12


@pytest.mark.parametrize('mutate', R.MUTATIONS)
def test_the_gpu_bounds_tell_a_wrong_closed_form_apart(mutate):
    worst = 0.0
    for D, S, M in ((7, 12, 3), (15, 15, 60)):
        params, alpha, Li, Xs, w, dims, grid = _case(D, S, M)
        good = R.brute(Xs, w, alpha, Li, params, S, M, dims, grid)
        bad = R.closed(Xs, w, alpha, Li, params, S, M, dims, grid, mutate=mutate)
        moved = max(rel(bad[0], good[0]) / F32_BOUND, rel(bad[1], good[1]) / F32_BOUND, rel(bad[2], good[2]) / F32_BOUND,
                    rel(bad[3], good[3]) / F32_BOUND_ICE)
        print(mutate, (D, S, M), 'moves an output by %.1e x its fp32 bound' % moved)
        worst = max(worst, moved)
        assert moved > 1e3
    assert worst > 1e3


def test_a_single_row_reduces_to_predict_at_the_replaced_row():
    D, S, M = 7, 12, 3
    params, alpha, Li, Xs, _, dims, grid = _case(D, S, M, T=1, G=6)
    pd, sd, cov, ice, _ = R.closed(Xs, None, alpha, Li, params, S, M, dims, grid)
    for a, d in enumerate(dims):
        Xe = np.repeat(Xs, 6, 0); Xe[:, d] = grid[a]
        mu, std = O.predict(Xe, alpha[:, None], Li, params, S, M)
        latent = np.sqrt(std ** 2 - R.kappa(params))              # the oracle's std carries the noise term kappa
        assert rel(pd[a], mu.ravel()) < 1e-12 and rel(ice[a, 0], mu.ravel()) < 1e-12
        assert rel(sd[a], latent) < 1e-10
        assert rel(np.diag(cov[a]), latent ** 2) < 1e-10


def test_predict_pd_entry_point_declared_exported_and_checked_without_gpu():
    """scfgp_predict_pd is in the header, the library and the binding table with the documented argument types, and refuses bad
    arguments before touching a device or an output."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'scfgp_hip.h')).read(), flags=re.S)
    cd = r'\s*const double\s*\*\s*'
    assert re.search(r'\bint\s+scfgp_predict_pd\s*\(\s*scfgp_ctx\s*\*\s*ctx,' + cd + r'Xs,\s*int64_t T,' + cd + r'w,' + cd + r'alpha,' + cd
                     + r'Li,\s*const int\s*\*\s*dims,\s*int ndim,' + cd + r'grid,\s*int G,\s*int mode,\s*double\s*\*\s*pd,\s*double\s*\*\s*pd_sd,'
                     r'\s*double\s*\*\s*pd_cov,\s*double\s*\*\s*ice\s*\)', header)
    dp = _lib._c_double_p
    res, args = _lib.SIGNATURES['scfgp_predict_pd']
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, dp, ctypes.c_int64, dp, dp, dp, ctypes.POINTER(ctypes.c_int), ctypes.c_int, dp, ctypes.c_int,
                    ctypes.c_int, dp, dp, dp, dp]
    lib = _lib.load()
    fn = lib.scfgp_predict_pd
    D, S, M = 3, 2, 5
    K = 2 * (S + M)
    T, G = 4, 3
    Xs = np.zeros((T, D)); alpha = np.zeros(K); Li = np.eye(K); grid = np.zeros((2, G))
    dims = (ctypes.c_int * 2)(0, 2)
    out = [np.full((2, G), 7.0), np.full((2, G), 7.0), np.full((2, G, G), 7.0), np.full((2, T, G), 7.0)]
    p = _lib.dptr
    o = [p(a) for a in out]
    assert fn(None, p(Xs), T, None, p(alpha), p(Li), dims, 2, p(grid), G, 0, *o) == -1
    ctx = ctypes.c_void_p()
    lib.scfgp_create(ctypes.byref(ctx), D, S, M, 0, 0, None)        # fails on a GPU-less box but hands back its context
    assert ctx.value
    try:
        def refused(match, *a):
            assert fn(ctx, *a) == -1
            assert match in lib.scfgp_last_error(ctx).decode(), lib.scfgp_last_error(ctx)
            assert all(np.all(b == 7.0) for b in out)
        refused('bad arguments', None, T, None, p(alpha), p(Li), dims, 2, p(grid), G, 0, *o)
        refused('bad arguments', p(Xs), T, None, p(alpha), p(Li), None, 2, p(grid), G, 0, *o)
        refused('bad arguments', p(Xs), T, None, p(alpha), p(Li), dims, 2, None, G, 0, *o)
        refused('no output', p(Xs), T, None, p(alpha), p(Li), dims, 2, p(grid), G, 0, None, None, None, None)
        refused('T must', p(Xs), 0, None, p(alpha), p(Li), dims, 2, p(grid), G, 0, *o)
        for g in (0, 1025):
            refused('G must', p(Xs), T, None, p(alpha), p(Li), dims, 2, p(grid), g, 0, *o)
        for nd in (0, D + 1):
            refused('ndim must', p(Xs), T, None, p(alpha), p(Li), dims, nd, p(grid), G, 0, *o)
        refused('out of range', p(Xs), T, None, p(alpha), p(Li), (ctypes.c_int * 2)(0, 3), 2, p(grid), G, 0, *o)
        refused('out of range', p(Xs), T, None, p(alpha), p(Li), (ctypes.c_int * 2)(-1, 1), 2, p(grid), G, 0, *o)
        refused('given twice', p(Xs), T, None, p(alpha), p(Li), (ctypes.c_int * 2)(1, 1), 2, p(grid), G, 0, *o)
        for mode in (-1, 2):
            refused('bad mode', p(Xs), T, None, p(alpha), p(Li), dims, 2, p(grid), G, mode, *o)
        refused('no X scaler', p(Xs), T, None, p(alpha), p(Li), dims, 2, p(grid), G, 1, *o)
        refused('parameters not set', p(Xs), T, None, p(alpha), p(Li), dims, 2, p(grid), G, 0, *o)
    finally:
        lib.scfgp_destroy(ctx)
