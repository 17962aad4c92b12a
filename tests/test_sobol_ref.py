"""CPU tier of scfgp_sobol: the numpy restatement of the closed form (tests/sobol_ref.py) against two routes that share nothing with it
but oracle.feature_map -- tensor Gauss quadrature and pick-freeze Monte Carlo --, the identities of the Sobol decomposition, the
exact-zero case with the quotient form as a mutant, the mutants that the device bound must reject, and the coverage conditions of the
parity inputs that the GPU tier (tests/test_gpu_sobol.py) runs on."""
import itertools

import numpy as np
import pytest

from oracle import scfgp_oracle as O
from scfgp_amd import synth
from tests import gradcov_ref
from tests import sobol_ref as R


def _nodes(kind, p0, p1, n=48):
    """nodes and weights (summing to 1) of input d: Gauss-Legendre on [p0, p1], Gauss-Hermite for normal(p0, p1^2)"""
    if kind == 1:
        x, w = np.polynomial.hermite_e.hermegauss(n)
        return p0 + p1 * x, w / w.sum()
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (p0 + p1) + 0.5 * (p1 - p0) * x, 0.5 * w


def _quadrature(params, D, S, M, kind, p0, p1, W):
    """f0, V, Vmain, Vtot of every column by tensor quadrature through the feature map"""
    ax = [_nodes(kind[d], p0[d], p1[d]) for d in range(D)]
    X = np.stack([g.ravel() for g in np.meshgrid(*[a[0] for a in ax], indexing='ij')], 1)
    wt = np.ones(1)
    for a in ax:
        wt = np.multiply.outer(wt, a[1])
    wt = wt.reshape((len(ax[0][0]),) * D)
    F = (O.feature_map(X, params, D, S, M) @ W).T.reshape((W.shape[1],) + wt.shape)
    f0 = (F * wt).sum(tuple(range(1, D + 1)))
    Fc = F - f0.reshape((-1,) + (1,) * D)
    V = (Fc ** 2 * wt).sum(tuple(range(1, D + 1)))
    Vmain = np.empty((W.shape[1], D)); Vtot = np.empty((W.shape[1], D))
    for d in range(D):
        others = tuple(a for a in range(1, D + 1) if a != d + 1)
        w_d = ax[d][1]
        w_o = wt.sum(d, keepdims=True) if D > 1 else np.ones_like(wt)           # weights of the other inputs, axis d kept at length 1
        cond = (Fc * wt).sum(others) / w_d                                       # E[f - f0 | x_d]
        Vmain[:, d] = (cond ** 2 * w_d).sum(1)
        rest = (Fc * wt).sum(d + 1, keepdims=True) / w_o                         # E[f - f0 | x_-d]
        Vtot[:, d] = V - (rest ** 2 * w_o).sum(tuple(range(1, D + 1)))
    return dict(f0=f0, V=V, Vmain=Vmain, Vtot=Vtot)


@pytest.mark.parametrize('D,S,M,kind', [(3, 2, 5, (0, 1, 0)), (2, 3, 4, (1, 0))])
def test_closed_form_against_tensor_quadrature(D, S, M, kind):
    params, W = R.parity_inputs(D, S, M)
    kind = np.array(kind); p0 = np.where(kind == 1, 0.5, 0.0); p1 = np.where(kind == 1, 0.25, 1.0)
    ref = R.sobol(params, D, S, M, kind, p0, p1, W)
    quad = _quadrature(params, D, S, M, kind, p0, p1, W)
    for k in ('f0', 'V', 'Vmain', 'Vtot'):
        err = float(np.max(np.abs(quad[k] - ref[k]) / (np.abs(ref['f0']) if k == 'f0' else ref['V']).reshape((-1,) + (1,) * (ref[k].ndim - 1))))
        print('quadrature', (D, S, M), k, '%.2e' % err)
        assert err <= 1e-11, (k, err)
    assert abs(ref['phibar'] @ W[:, 0] - ref['f0'][0]) <= 1e-14 * np.abs(ref['phibar']) @ np.abs(W[:, 0])


def test_closed_form_against_pick_freeze_monte_carlo():
    D, S, M = 7, 12, 3
    n = 1 << 17
    params, W = R.parity_inputs(D, S, M)
    w = W[:, 0]
    kind, p0, p1 = R.mixed_measure(D)
    ref = R.sobol(params, D, S, M, kind, p0, p1, w)
    rng = np.random.default_rng(12)
    draw = lambda: np.where(kind == 1, p0 + p1 * rng.standard_normal((n, D)), p0 + (p1 - p0) * rng.random((n, D)))
    f = lambda X: O.feature_map(X, params, D, S, M) @ w
    A, B = draw(), draw()
    fA, fB = f(A), f(B)
    se = lambda t: t.std(ddof=1) / np.sqrt(n)
    assert abs(fA.mean() - ref['f0'][0]) <= 5 * se(fA)
    tV = (fA - ref['f0'][0]) ** 2
    assert abs(tV.mean() - ref['V'][0]) <= 5 * se(tV)
    for d in range(D):
        E = A.copy(); E[:, d] = B[:, d]                          # differs from A in x_d only, shares x_d with B
        fE = f(E)
        tm = fB * (fE - fA)                                      # Saltelli's first-order estimator: E[fB (fE - fA)] = Vmain[d]
        tt = 0.5 * (fA - fE) ** 2                                # Jansen's total-effect estimator
        print('pick-freeze d=%d  Vmain %.4e (%.4e +- %.1e)  Vtot %.4e (%.4e +- %.1e)' % (d, ref['Vmain'][0, d], tm.mean(), se(tm), ref['Vtot'][0, d], tt.mean(), se(tt)))
        assert abs(tm.mean() - ref['Vmain'][0, d]) <= 5 * se(tm), d
        assert abs(tt.mean() - ref['Vtot'][0, d]) <= 5 * se(tt), d


def test_one_input_has_one_effect():
    D, S, M = 1, 2, 2
    params, W = R.parity_inputs(D, S, M)
    for m in (R.mixed_measure(D), (np.array([1]), np.array([0.3]), np.array([0.7]))):
        ref = R.sobol(params, D, S, M, *m, W)
        bd = R.bounds(ref, D)
        assert np.all(np.abs(ref['Vmain'][:, 0] - ref['V']) <= bd['V']) and np.all(np.abs(ref['Vtot'][:, 0] - ref['V']) <= bd['V'])


def test_additive_model_has_no_interactions():
    """S = D, a diagonal l_F and one-hot rows of r_F: every phase depends on one input, so f is a sum of functions of single inputs"""
    D = S = 4; M = 9
    rng = np.random.default_rng(5)
    params = synth.make_params(3, D, S, M, abc=(-1.0, 0.0, -1.0)).copy()
    l_F = np.diag(1.0 + rng.random(D))
    r_F = np.zeros((M, S)); r_F[np.arange(M), rng.integers(0, S, M)] = 0.5 + 2.0 * rng.random(M)
    params[3:3 + D * S] = l_F.ravel(); params[3 + D * S:3 + D * S + M * S] = r_F.ravel()
    W = rng.standard_normal((2 * (S + M), 2))
    ref = R.sobol(params, D, S, M, *R.mixed_measure(D), W)
    bd = R.bounds(ref, D)
    print('additive: sum Vmain / V - 1 =', ref['Vmain'].sum(1) / ref['V'] - 1)
    assert np.all(np.abs(ref['Vmain'].sum(1) - ref['V']) <= D * bd['V'])
    assert np.all(np.abs(ref['Vtot'] - ref['Vmain']) <= bd['Vtot'])
    assert np.all(ref['V'] > 1e3 * bd['V'])


def test_point_masses_give_the_prediction_and_no_variance():
    D, S, M = 7, 12, 3
    params, W = R.parity_inputs(D, S, M)
    x = synth.make_X(11, 1, D)
    ref = R.sobol(params, D, S, M, None, x[0], x[0], W)
    bd = R.bounds(ref, D)
    mu = O.predict(x, W[:, 0], np.eye(W.shape[0]), params, S, M)[0]
    assert abs(ref['f0'][0] - float(mu[0, 0])) <= bd['f0'][0]
    for k in ('V', 'Vmain', 'Vtot'):
        assert np.all(np.abs(ref[k]) <= bd[k]), k


@pytest.mark.parametrize('D,S,M', gradcov_ref.GEOMETRIES)
def test_parity_inputs_cover_what_they_must(D, S, M):
    """the variance is no rounding residue of its terms, interactions are present, and total >= main >= 0 within the bound"""
    params, W = R.parity_inputs(D, S, M)
    ref = R.sobol(params, D, S, M, *R.mixed_measure(D), W)
    bd = R.bounds(ref, D)
    assert np.all(ref['V'] >= 0.02 * ref['Sabs_all']), ref['V'] / ref['Sabs_all']
    if D > 1:
        assert np.max((ref['Vtot'] - ref['Vmain']) / ref['V'][:, None]) > 0.1
    assert np.all(ref['Vmain'] >= -bd['Vmain']) and np.all(ref['Vtot'] - ref['Vmain'] >= -(bd['Vtot'] + bd['Vmain']))


def test_an_exact_zero_factor_needs_explicit_leave_one_out_products():
    D, S, M = 7, 12, 3
    params, W = R.parity_inputs(D, S, M)
    kind, p0, p1 = R.mixed_measure(D)
    kind[2] = 1; p0[2] = 0.5; p1[2] = 1e3
    ref = R.sobol(params, D, S, M, kind, p0, p1, W)
    assert all(np.all(np.isfinite(ref[k])) for k in ('f0', 'V', 'Vmain', 'Vtot', 'phibar'))
    Om = R.phases(params, D, S, M)[0]
    assert np.all(R.psi(kind, p0, p1, Om)[2] == 0.0)                             # the factor IS zero, not merely small
    print('zero psi: S = %.3f, T = %.3f' % (ref['Vmain'][0, 2] / ref['V'][0], ref['Vtot'][0, 2] / ref['V'][0]))
    assert ref['Vtot'][0, 2] / ref['V'][0] > 0.99 and 0.3 < ref['Vmain'][0, 2] / ref['V'][0] < 0.9
    bad = R.sobol(params, D, S, M, kind, p0, p1, W, divide=True)                 # the mutant: prod / psi
    assert np.all(np.isnan(bad['Vtot'][:, 2])) and np.all(np.isnan(bad['Vmain'][:, 2]))


@pytest.mark.parametrize('mutate', R.MUTATIONS)
def test_the_device_bound_rejects_every_mutant(mutate):
    """each mutant exceeds the bound by more than 1e3 on some output; 'no_centre' on a case with f0^2 > 5 V"""
    D, S, M = (1, 2, 2) if mutate == 'no_centre' else (7, 12, 3)
    params, W = R.parity_inputs(D, S, M)
    W = W[:, :1]
    m = R.mixed_measure(D)
    ref = R.sobol(params, D, S, M, *m, W)
    if mutate == 'no_centre':
        assert ref['f0'][0] ** 2 > 5 * ref['V'][0]
    ratios = R.worst_ratio(R.sobol(params, D, S, M, *m, W, mutate=mutate), ref, D)
    print(mutate, ' '.join('%s=%.1e' % kv for kv in sorted(ratios.items())))
    assert max(ratios.values()) > 1e3, ratios
