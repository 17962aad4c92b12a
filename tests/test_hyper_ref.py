"""CPU tier of the hyper-parameter range tests: the numpy restatement of scal_kernel, the penalty statistics, the penalty and centring
terms of the gradient and finalize_kernel (tests/hyper_ref.py) against mpmath, on grids and rows that reach the ends of the ranges;
every mutated restatement must fail the same assertions; the grids must reach what they are for; the degenerate std = 0 row is
pinned.  The GPU tier (tests/test_gpu_hyper_range.py) holds the device to multiples of the figures measured here."""
import mpmath
import numpy as np
import pytest

from oracle import scfgp_oracle as O
from tests import hyper_ref as H

# allowance: 2 x the worst error measured for the correct restatement against mpmath (tests/hyper_ref.py: MEASURED_*)
SCALAR_BOUND = {k: 2 * v for k, v in H.MEASURED_SCALAR_ERR.items()}
PEN_BOUND = {k: 2 * v for k, v in H.MEASURED_PEN_ERR.items()}

A_GRID, B_GRID, C_GRID, C_FAR, M_GRID, PEN_SHAPES = H.A_GRID, H.B_GRID, H.C_GRID, H.C_FAR, H.M_GRID, H.PEN_SHAPES


def _rel(x, x0):
    return abs(float((mpmath.mpf(float(x)) - x0) / x0))


def scalar_errors(mutate=None):
    """name -> [(grid value, relative error of the restatement against mpmath)]"""
    out = dict((k, []) for k in H.MEASURED_SCALAR_ERR)
    for a in A_GRID:
        got, ref = H.scalars(a, 0.0, 0.0, 5, mutate), H.mp_scalars(a, 0.0, 0.0, 5)
        for k in ('e2a', 'lam', 'em2a'):
            out[k].append((a, _rel(got[k], ref[k])))
    for M in M_GRID:
        for b in B_GRID:
            out['s'].append((b, _rel(H.scalars(0.0, b, 0.0, M, mutate)['s'], H.mp_scalars(0.0, b, 0.0, M)['s'])))
    for c in C_GRID:
        got, ref = H.scalars(0.0, 0.0, c, 5, mutate), H.mp_scalars(0.0, 0.0, c, 5)
        for k in ('kappa', 'sigc'):
            out[k].append((c, _rel(got[k], ref[k])))
    return out


@pytest.fixture(scope='module')
def correct_scalars():
    return scalar_errors()


def test_scalar_grids(correct_scalars):
    for k, rows in correct_scalars.items():
        worst = max(e for _, e in rows)
        print('scalar %-5s worst relative error %.2e (bound %.2e)' % (k, worst, SCALAR_BOUND[k]))
        assert worst <= SCALAR_BOUND[k], (k, worst)
        assert worst >= H.MEASURED_SCALAR_ERR[k] / 4, (k, worst, 'the recorded figure is stale')


def test_far_c_is_finite_monotone_and_asymptotic():
    cs = sorted(set(C_FAR) | set(C_GRID))
    sc = [H.scalars(0.0, 0.0, c, 5) for c in cs]
    kap = np.array([s['kappa'] for s in sc]); sig = np.array([s['sigc'] for s in sc])
    assert np.isfinite(kap).all() and (kap > 0).all() and (np.diff(kap) > 0).all()
    assert np.isfinite(sig).all() and (sig > 0).all() and (sig <= 1).all() and (np.diff(sig) >= 0).all()
    for c in (100.0, 700.0):                                   # kappa -> c, sigc -> 1
        s = H.scalars(0.0, 0.0, c, 5)
        assert s['kappa'] == c and s['sigc'] == 1.0
    for c in (-100.0, -700.0):                                 # kappa -> e^c, sigc -> e^c
        s = H.scalars(0.0, 0.0, c, 5)
        assert abs(s['kappa'] / np.exp(c) - 1) <= 4e-16 and abs(s['sigc'] / np.exp(c) - 1) <= 4e-16


def test_mutated_kappa_fails_from_minus_14(correct_scalars):
    bad = dict(scalar_errors('kappa_plain')['kappa'])
    low = [c for c in C_GRID if c <= -14.0]
    assert low and all(bad[c] > SCALAR_BOUND['kappa'] for c in low), [(c, bad[c]) for c in low if not bad[c] > SCALAR_BOUND['kappa']]
    assert bad[-14.0] > 1e-11 and bad[-20.0] > 1e-9 and bad[-30.0] > 1e-4        # what log(1 + e^c) has lost by then
    assert H.scalars(0.0, 0.0, -37.0, 5, 'kappa_plain')['kappa'] == 0.0 and H.scalars(0.0, 0.0, -37.0, 5)['kappa'] > 0.0


def test_mutated_lam_fails_at_small_a():
    bad = dict(scalar_errors('lam_e2a')['lam'])
    low = [a for a in A_GRID if a <= -6.0]
    assert low and all(bad[a] > SCALAR_BOUND['lam'] for a in low)
    assert all(bad[a] > 0.1 for a in low)                      # the jitter is over a tenth of lam there


def test_grids_reach_what_they_are_for():
    assert C_GRID.min() <= -30 and C_GRID.max() >= 30
    assert any(EPS > np.exp(2 * a) for a in A_GRID for EPS in (H.EPSILON,))
    for v in (-7.0, -6.0, -4.0, 2.0):
        assert v in A_GRID
    for v in (-30.0, -20.0, -14.0, -10.0, 10.0, 30.0):
        assert v in C_GRID
    signs = set()
    for D, S, M in PEN_SHAPES:
        for name in H.EDGE_CASES:
            l_F, r_F = H.edge_factors(name, D, S, M)
            mF, sF, ml, sl = H.pen_rows(l_F, l_F @ r_F.T)
            signs.add(('w', np.sign(1 - 1 / sF.sum()))); signs.add(('l', np.sign(1 - 1 / sl.sum())))
    assert signs >= {('w', -1.0), ('w', 1.0), ('l', -1.0), ('l', 1.0)}, signs
    l_F, r_F = H.edge_factors('lF_offset', 3, 70, 300)
    mF, sF, ml, sl = H.pen_rows(l_F, l_F @ r_F.T)
    assert (np.abs(ml) / sl).max() >= 1e3
    l_F, r_F = H.edge_factors('F_offset', 3, 70, 300)
    mF, sF, ml, sl = H.pen_rows(l_F, l_F @ r_F.T)
    assert (np.abs(mF) / sF).max() >= 1e3
    assert {M for _, _, M in PEN_SHAPES} == {5, 300} and {S for _, S, _ in PEN_SHAPES} == {2, 70}


def pen_errors(D, S, M, name, mutate=None):
    """errors of the restatement on one edge case: mean (over max |row|), std and R_PEN (relative), the penalty gradient (over its
    largest entry)"""
    l_F, r_F = H.edge_factors(name, D, S, M)
    F = l_F @ r_F.T
    stats = H.pen_rows(l_F, F, mutate)
    pen = H.pen_sums(stats, S, M)[1]
    gF, gl = H.pen_grad(l_F, F, mutate)
    pen0, stats0 = H.mp_penalty(l_F, F)
    gF0, gl0 = H.mp_penalty_grad(l_F, F)
    tops = [np.abs(F).max(1), None, np.abs(l_F).max(1), None]
    e = dict(mean=0.0, std=0.0)
    for q in range(4):
        for d in range(D):
            if q % 2 == 0:
                e['mean'] = max(e['mean'], abs(float(mpmath.mpf(float(stats[q][d])) - stats0[q][d])) / tops[q][d])
            else:
                e['std'] = max(e['std'], _rel(stats[q][d], stats0[q][d]))
    e['pen'] = _rel(pen, pen0)
    e['grad'] = 0.0
    for g, g0 in ((gF, gF0), (gl, gl0)):
        top = max(abs(float(v)) for v in g0.values())
        e['grad'] = max(e['grad'], max(abs(float(mpmath.mpf(float(g[dk])) - v)) for dk, v in g0.items()) / top)
    return e


@pytest.fixture(scope='module')
def correct_pen():
    return dict(((sh, name), pen_errors(*sh, name)) for sh in PEN_SHAPES for name in H.EDGE_CASES)


def test_penalty_edge_rows(correct_pen):
    worst = dict((k, max(e[k] for e in correct_pen.values())) for k in PEN_BOUND)
    print('penalty edge rows, worst: ' + ' '.join('%s %.2e' % kv for kv in worst.items()))
    for k in PEN_BOUND:
        assert worst[k] <= PEN_BOUND[k], (k, worst[k], [c for c, e in correct_pen.items() if e[k] > PEN_BOUND[k]])
        assert worst[k] >= H.MEASURED_PEN_ERR[k] / 4, (k, worst[k], 'the recorded figure is stale')


@pytest.mark.parametrize('mutate,keys', [('sample_std', ('std', 'pen', 'grad')), ('no_mean_term', ('grad',))])
def test_mutated_penalty_fails(mutate, keys):
    for sh in PEN_SHAPES:
        for name in H.EDGE_CASES:
            e = pen_errors(*sh, name, mutate=mutate)
            for key in keys:
                assert e[key] > PEN_BOUND[key], (mutate, sh, name, key, e)


def test_centring_and_rank_S_forms_agree():
    """fbar / lbar: the dense form against mpmath-free algebra -- with XZ = X~^T Zbar and the rank-S operands built from the same Zbar,
    both forms give the same lbar_F, and Fbar's two forms differ by the factored data term exactly"""
    rng = np.random.default_rng(5)
    for D, S, M in PEN_SHAPES:
        l_F, r_F = H.edge_factors('sig_large', D, S, M)
        F = l_F @ r_F.T
        N = 40
        X = rng.random((N, D)); Zb = rng.standard_normal((N, S + M))
        Xt = np.concatenate((X, np.ones((N, 1))), 1)
        XZ = Xt.T @ Zb
        Tt = np.concatenate((X @ l_F, np.ones((N, 1))), 1)
        TZ = Tt.T @ Zb
        XU = X.T @ (Zb[:, :S] + Zb[:, S:] @ r_F)
        Fb = H.fbar(l_F, F, XZ=XZ); Fb_r = H.fbar(l_F, F, TZ=TZ)
        assert np.allclose(Fb - Fb_r, XZ[:D, S:], rtol=0, atol=1e-12 * np.abs(XZ).max())
        lb = H.lbar(l_F, r_F, F, Fb, XZ=XZ); lb_r = H.lbar(l_F, r_F, F, Fb_r, TZ=TZ, XU=XU)
        assert np.abs(lb - lb_r).max() <= 1e-12 * np.abs(lb).max()
        # against the oracle's epilogue (its own order of operations), before the 1 / N
        st3 = dict(XZ=XZ[:D], colsum=XZ[D], bbar=0.0)
        p = np.concatenate((np.zeros(3), l_F.ravel(), r_F.ravel(), np.zeros(S + M)))
        g = O._epilogue(p, D, S, M, st3, 0.0, 0.0, 1.0)
        assert np.abs(lb.ravel() - g[3:3 + D * S]).max() <= 1e-12 * np.abs(lb).max()
        rb = Fb.T @ l_F
        assert np.abs(rb.ravel() - g[3 + D * S:3 + D * S + M * S]).max() <= 1e-12 * np.abs(rb).max()


def test_finalize_against_mpmath():
    """cost and grad[0:3] from given stage scalars, at the corners of (a, c): T3 = em2a (yy - g.alpha) is taken as given"""
    rng = np.random.default_rng(3)
    N, M = 257, 5
    for a in (-7.0, -1.0, 2.0):
        for c in (-30.0, -1.0, 30.0):
            st = dict(zip(('T1', 'T2', 'kbar', 'sumqv', 'sumpmu', 'yy', 'gtalpha', 'trabar', 'trag', 'utg', 'pen'),
                          rng.standard_normal(11) * 10.0))
            st['yy'] = 257.0; st['gtalpha'] = 200.0
            sc = H.scalars(a, 0.0, c, M)
            cost, g = H.finalize(sc, a, st, M, float(N))
            m = H.mp_scalars(a, 0.0, c, M)
            f = dict((k, mpmath.mpf(float(v))) for k, v in st.items())
            T3 = m['em2a'] * (f['yy'] - f['gtalpha'])
            cost0 = (f['T1'] + f['T2'] + T3 + 2 * (N - M) * mpmath.mpf(a) + f['pen']) / N
            terms = [abs(st['T1']), abs(st['T2']), abs(float(T3)), abs(2 * (N - M) * a), abs(st['pen'])]
            assert abs(float(mpmath.mpf(float(cost)) - cost0)) <= 8 * np.finfo(float).eps * sum(terms) / N
            ga0 = (2 * m['e2a'] * f['trabar'] - 2 * T3 + 2 * (N - M)) / N
            sa = (2 * float(m['e2a']) * abs(st['trabar']) + 2 * abs(float(T3)) + 2 * (N - M)) / N
            assert abs(float(mpmath.mpf(float(g[0])) - ga0)) <= 8 * np.finfo(float).eps * sa
            gb0 = (2 * f['trag'] + f['utg'] + 2 * f['sumqv'] + f['sumpmu']) / N
            sb = (2 * abs(st['trag']) + abs(st['utg']) + 2 * abs(st['sumqv']) + abs(st['sumpmu'])) / N
            assert abs(float(mpmath.mpf(float(g[1])) - gb0)) <= 8 * np.finfo(float).eps * sb
            assert _rel(g[2], f['kbar'] * m['sigc'] / N) <= 8 * np.finfo(float).eps


def test_degenerate_std_zero_is_an_infinite_penalty():
    """every row of l_F all-equal (S = 1 always is): sum of stds = 0, -log 0 = +inf -- in the restatement and in the oracle's formula"""
    D, S, M = 3, 2, 5
    l_F, r_F = H.edge_factors('sig_large', D, S, M)
    l_F[:] = l_F[:, :1]
    F = l_F @ r_F.T
    with np.errstate(divide='ignore', invalid='ignore'):
        assert H.penalty(l_F, F) == np.inf and O._penalty(l_F, F, S, M) == np.inf
        l1 = l_F[:, :1].copy()
        assert H.penalty(l1, l1 @ r_F[:, :1].T) == np.inf and O._penalty(l1, l1 @ r_F[:, :1].T, 1, M) == np.inf
    # one all-equal row among others: the penalty is finite, that row's gradient is 0 / 0
    l_F, r_F = H.edge_factors('sig_large', D, S, M)
    l_F[1] = l_F[1, 0]
    gF, gl = H.pen_grad(l_F, l_F @ r_F.T)
    assert np.isfinite(H.penalty(l_F, l_F @ r_F.T)) and np.isnan(gl[1]).all() and np.isfinite(gl[[0, 2]]).all()


def test_mp_objective_meets_the_oracle_at_the_centre():
    """the mpmath objective is the oracle's objective: cost, alpha, Li, mu*, std* and sampled gradient entries at a well-conditioned point"""
    from scfgp_amd import synth
    N, D, S, M = 41, 3, 2, 5
    X = synth.make_X(5, N, D); y = synth.normal(9, 0, N); Xs = synth.make_X(6, 4, D)
    p = synth.make_params(3, D, S, M, abc=(-1.0, 0.0, -1.0))
    pr = H.MpProblem(X, y, S, M, Xs)
    r = pr.evaluate(p, full=True)
    c0, g0, a0, L0 = O.value_and_grad(X, y.reshape(-1, 1), p, S, M)
    cA = float(H.mp_cond(r['A']))
    assert abs(float(r['cost']) - c0) <= 1e-13 * abs(c0)
    assert np.linalg.norm(H.to_f64(r['alpha']) - a0.ravel()) <= 14 * 2.0 ** -53 * cA * np.linalg.norm(a0)
    assert np.linalg.norm(H.to_f64(r['Li']) - L0) <= 14 * 2.0 ** -53 * cA * np.linalg.norm(L0)
    mu0, sd0 = O.predict(Xs, a0, L0, p, S, M)
    assert np.abs(H.to_f64(r['mu']) - mu0.ravel()).max() <= 1e-12 and np.abs(H.to_f64(r['std']) / sd0 - 1).max() <= 1e-12
    for i in (0, 1, 2, 4, 3 + D * S + 1):
        assert abs(float(pr.grad_entry(p, i)) - g0[i]) <= 1e-10 * abs(g0[i]), i
    for i in (3 + D * S + M * S, pr.P - 1):                   # phase entries: exactly invariant
        assert abs(float(pr.grad_entry(p, i))) <= 1e-30
