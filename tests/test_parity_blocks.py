"""
CPU tier of tests/parity.py: the oracle's abs-sum scale is sound, the phase gradient is zero, and every check fails the mutations
it exists for at the fp32 bounds -- mutations a norm over the whole gradient (the old global check, rel < 3e-3 in fp32) accepts.
Each mutated value is built from oracle pieces; nothing on the GPU is mutated.  Output (-s): per mutation and case, its figure
over the fp32 bound and the old global rel with whether the old check accepted it.
"""
import numpy as np
import pytest

from oracle import scfgp_oracle as O
from oracle import autograd_ref as AR
from tests import parity as P
from tests.golden.make_oracle_kats import CASES, case_inputs

OLD = dict(grad=3e-3, alpha=1e-3, Li=1e-3, mu=1e-4)     # the fp32 global checks of the GPU parity tests and of smoke()


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b))


_CACHE = {}


def _ref(name):
    if name not in _CACHE:
        N, D, S, M, T, seed = CASES[name]
        X, y, params, Xs = case_inputs(name)
        _CACHE[name] = (X, y, params, Xs, P.oracle_all(X, y, params, S, M, Xs))
    return _CACHE[name]


def _report(what, name, ratio, old, old_tol, need=10.0):
    acc = old < old_tol
    print('%-34s %-16s fig/bound %9.3g   old rel %.2e (%s)' % (what, name, ratio, old, 'accepted' if acc else 'rejected'))
    assert ratio >= need * (1 - 1e-9), (what, name, ratio)
    return acc


# ---- the scale ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_phase_gradient_is_zero_and_rotation_invariant(name):
    N, D, S, M, T, seed = CASES[name]
    X, y, params, Xs, ref = _ref(name)
    L = P.layout(D, S, M)
    ph = np.concatenate((L['l_P'], L['P']))
    sc = np.concatenate((np.zeros(3), ref['scale']))
    assert np.all(sc[ph] > 0)
    r = np.abs(ref['grad'][ph]) / sc[ph]
    print('%s: phase entries / scale <= %.1e' % (name, r.max()))
    assert r.max() <= 1e-12
    p2 = params.copy()
    p2[ph] += np.random.default_rng(seed).uniform(0, 2 * np.pi, len(ph))
    c2 = O.forward(X, y, p2, S, M, False)[0]
    c1 = O.forward(X, y, params, S, M, False)[0]
    assert abs(c2 - c1) <= 1e-13 * abs(c1), (c1, c2)


@pytest.mark.parametrize('name', list(CASES))
def test_scale_sound_against_autograd(name):
    """the 3-sweep oracle against torch autograd of the literal graph passes the fp64 row with >= 10x margin"""
    N, D, S, M, T, seed = CASES[name]
    X, y, params, Xs, ref = _ref(name)
    c2, g2, a2, L2 = AR.value_and_grad(X, y, params, S, M)
    t = {k: tuple(np.divide(v, 10)) if k == 'rho' else v / 10 for k, v in P.TOL['f64'].items()}      # the fp64 row with 10x margin
    r = P.check_grad(g2, ref['grad'], ref['scale'], D, S, M, t)
    P.check_alpha(a2, ref['alpha'], t); P.check_li(L2, ref['Li'], t)
    print('%s: autograd vs oracle at fp64 / 10: %s' % (name, P.fmt(r)))
    assert np.all(ref['scale'] >= 0) and ref['scale'].shape == (len(ref['grad']) - 3,)


def test_layout():
    D, S, M = 3, 2, 70
    L = P.layout(D, S, M)
    n = O.num_params(D, S, M)
    allix = np.concatenate(([0, 1, 2], L['l_F'], L['r_F'].ravel(), L['l_P'], L['P']))
    assert np.array_equal(allix, np.arange(n))
    assert L['r_F'].shape == (M, S) and P.rf_groups(M) == [(0, 32), (32, 64), (64, 70)]


def test_f16x3_row_is_the_fp32_row():
    assert P.TOL['f16x3'] == P.TOL['f32']


# ---- mutations of the end-to-end outputs --------------------------------------------------------------------------------------
GAP = {('b*1.1', 'kin8nm_like'), ('b*1.1', 'c1_boston_shape'), ('r_F*0.9', 'kin8nm_like')}     # the issue's measured gap


@pytest.mark.parametrize('name', list(CASES))
def test_mutations_fail_the_fp32_bounds(name):
    N, D, S, M, T, seed = CASES[name]
    X, y, params, Xs, ref = _ref(name)
    g0, sc = ref['grad'], ref['scale']
    L = P.layout(D, S, M)
    gr = lambda g: max(P.grad_ratios(g, g0, sc, D, S, M, 'f32').values())
    print()

    def grad_mut(what, g, need=10.0):
        acc = _report(what, name, gr(g), rel(g, g0), OLD['grad'], need)
        if (what, name) in GAP:
            assert acc, (what, name, 'the old global check was expected to accept this')
        return acc

    # b's own fp32 error (4.5e-4, the cancelling closed form) leaves rho_b = 2e-3: its mutation is 10 rho_b, not 1e-3
    for k, f in (('a', 1e-3), ('b', 2e-2), ('c', 1e-3)):
        g = g0.copy(); g[L[k]] *= 1 + f
        acc = grad_mut('%s*(1+%g)' % (k, f), g)
        assert acc or (k, name) == ('b', 'tiny_257x5')
    g = g0.copy(); g[L['b']] *= 1.1
    grad_mut('b*1.1', g)
    g = g0.copy(); g[L['r_F'].ravel()] *= 0.9
    grad_mut('r_F*0.9', g)
    # one r_F group: 0.99 is caught (3.2x .. 9.2x, the tau term of the fp32 row dominates a group's bound); 0.96 by >= 10x
    for f, need in ((0.99, 1.0), (0.96, 10.0)):
        worst, olds = np.inf, []
        for f0, f1 in P.rf_groups(M):
            g = g0.copy(); g[L['r_F'][f0:f1].ravel()] *= f
            worst = min(worst, gr(g)); olds.append(rel(g, g0))
        acc = _report('each r_F group*%g (weakest)' % f, name, worst, max(olds), OLD['grad'], need)
        assert acc or f != 0.99

    def sweep3(**kw):
        return O.value_and_grad(X, y, params, S, M, **kw)[1]

    g = sweep3(rows3=(0, N - 64))
    grad_mut('last 64 rows out of sweep 3', g)
    J = S + M
    for half in ('cos', 'sin'):
        worst, olds = np.inf, []
        for t0 in range(0, J, P.TILE):
            def hook(Zc, Zs, lo, hi, t0=t0):
                Zc = Zc.copy(); Zs = Zs.copy()
                (Zc if half == 'cos' else Zs)[:, t0:t0 + P.TILE] = 0
                return Zc, Zs
            g = sweep3(zbar_hook=hook)
            worst = min(worst, gr(g)); olds.append(rel(g, g0))
        _report('Zbar 64-tile, %s half (weakest)' % half, name, worst, min(olds), OLD['grad'])
    gh = sweep3(rows3=(0, N // 2))
    g = g0.copy(); ph = np.concatenate((L['l_P'], L['P'])); g[ph] = gh[ph]
    grad_mut('phases = first-half column sums', g)

    a0, L0 = ref['alpha'].ravel(), ref['Li']
    # one alpha tile: 1.01 is caught (9x .. 11x at the fp32 row); 1.02 by >= 10x
    for f, need in ((1.01, 1.0), (1.02, 10.0)):
        worst, olds = np.inf, []
        for t0 in range(0, len(a0), P.TILE):
            a = a0.copy(); a[t0:t0 + P.TILE] *= f
            worst = min(worst, P.alpha_ratio(a, a0, 'f32')); olds.append(rel(a, a0))
        _report('alpha 64-tile*%g (weakest)' % f, name, worst, min(olds), OLD['alpha'], need)
    rng = np.random.default_rng(seed)
    worst, olds = np.inf, []
    for r0 in range(0, L0.shape[0], P.TILE):
        Li = L0.copy(); blk = Li[r0:r0 + P.TILE]
        dz = np.tril(rng.standard_normal(blk.shape), r0)
        Li[r0:r0 + P.TILE] += 1e-3 * np.linalg.norm(blk) * dz / np.linalg.norm(dz)
        worst = min(worst, P.li_ratio(Li, L0, 'f32')); olds.append(rel(Li, L0))
    _report('Li 64-row block + 1e-3 (weakest)', name, worst, min(olds), OLD['Li'], 1.0)      # caught, 1.3x at the fp32 row
    mu0, sd0 = ref['mu'].ravel(), ref['std'].ravel()
    t = int(np.argmin(sd0 / (np.abs(mu0) + sd0)))          # the row a global rel of mu sees least
    mu = mu0.copy(); mu[t] += 1e-2 * sd0[t]
    _report('one mu row + 1e-2 sigma', name, P.predict_ratio(mu, sd0, mu0, sd0, 'f32'), rel(mu, mu0), OLD['mu'])


# ---- the stage bounds against an fp32 model and its mutations ------------------------------------------------------------------
def _stage_data(N=9001, D=6, S=20, M=140, seed=0x5CF6B10C):
    from scfgp_amd import synth
    X = synth.make_X(seed, N, D)
    params = synth.make_params(seed + 2, D, S, M, abc=(-1.0, 0.0, -1.0))
    Phi = O.feature_map(X, params, D, S, M).astype(np.float32).astype(np.float64)
    K = Phi.shape[1]
    A = Phi.T @ Phi + np.exp(-2.0) * np.eye(K)
    Li = np.linalg.inv(np.linalg.cholesky(A))
    return Phi, Li.T @ Li


def test_stage_bounds_pass_the_fp32_model_and_fail_mutations():
    Phi, B = _stage_data()
    N, K = Phi.shape
    absP = np.abs(Phi)
    # the Gram: fp32 chains of 4096 rows flushed into fp64
    G = P.gram32_model(Phi)
    Gx = Phi.T @ Phi; GT = absP.T @ absP
    e = P.edges(K, 128)
    bg = P.bound32(4096, n64=-(-N // 4096))
    err = P.stage_error(G, Gx, GT, e, e).max()
    print('\nGram model: worst %.2e, bound %.2e' % (err, bg))
    assert err <= bg
    Gt = G.copy(); Gt[128:256, 0:128] = G[128:256, 0:128].T
    Gl = G - P.gram32_model(Phi[4096:8192])
    for what, Gm in (('Gram tile (1, 0) transposed', Gt), ('one 4096-row flush lost', Gl)):
        r = P.stage_error(Gm, Gx, GT, e, e).max() / bg
        print('%-34s fig/bound %.3g' % (what, r))
        assert r > 10
    # the apply: V = Phi B, fp32 Phi, fp32 copy of B, fp32 accumulation over K, fp32 output
    V = P.apply32_model(Phi, B)
    Vx = Phi @ B; VT = absP @ np.abs(B)
    ba = P.bound32(K, rounded=1, out32=True)
    re, ce = P.edges(N, 256), P.edges(K, 64)
    err = P.stage_error(V, Vx, VT, re, ce).max()
    print('apply model: worst %.2e, bound %.2e' % (err, ba))
    assert err <= ba
    Vz = V.copy(); Vz[(N - 1) // 64 * 64:] = 0
    r = P.stage_error(Vz, Vx, VT, re, ce).max() / ba
    print('%-34s fig/bound %.3g' % ('apply: last 64-row block zeroed', r))
    assert r > 10
