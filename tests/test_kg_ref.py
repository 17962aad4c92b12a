"""CPU tier of scfgp_acquire_kg: the numpy restatement (tests/kg_ref.py, the device's own forms) on oracle fits.  The two sums bracket
the exact knowledge gradient (the sorted upper envelope of ALL reference rows); nodes that separate every breakpoint recover it; the
default nodes' gap and the restatement's own error against 50-digit arithmetic are measured and pinned; a dropped reference row, the
other tie rule, the missing clamps and a missing zero node are each caught; the ctypes binding matches the header."""
import ctypes as C
import functools

import mpmath as mp
import numpy as np
import pytest

from oracle import scfgp_oracle as O
from tests import kg_ref as G
from tests import pred_cov_ref
from tests import select_ref as R

mp.mp.dps = 50
FITS = {42: (3, 1, 20, 150, 2048, 0), 128: (5, 4, 60, 1000, 2048, 0)}      # K -> a row in tests/select_ref.py's format
RS = (1, 33, 257, 2000)
NCAND = 48
EPS_MAX = 1e-15


@functools.lru_cache(maxsize=None)
def _fit(K):
    case = FITS[K]
    D, S, M = case[:3]
    params, X0, y0, Xp = R.problem(case)
    _, alpha, Li = O.forward(X0, y0, params, S, M, gauss_hermite=False)
    Cf = pred_cov_ref.factor(Xp, Li, params, S, M)
    mu = O.predict(Xp, alpha, Li, params, S, M)[0].ravel()
    return R.kappa(params), Cf, mu


@functools.lru_cache(maxsize=None)
def _lines(K, Rn, noise, minimize=False):
    """(d (R,), B (NCAND, R)): the first NCAND pool rows as candidates against the first R pool rows"""
    kap, Cf, mu = _fit(K)
    v = np.sum(Cf[:NCAND] ** 2, axis=1)
    sd = np.sqrt(kap * (v + 1.0)) if noise else np.sqrt(kap * v)
    return G.offsets(mu[:Rn], minimize), G.slopes(kap * (Cf[:NCAND] @ Cf[:Rn].T), sd)


def _all(K, Rn, noise, z=G.DEFAULT_NODES, minimize=False):
    d, B = _lines(K, Rn, noise, minimize)
    tab = G.node_table(d, B, z)
    kg, hi = G.bounds(*tab, z)
    return d, B, tab, kg, hi, G.kg_exact_rows(d, B)


@pytest.mark.parametrize('noise', [True, False])
@pytest.mark.parametrize('Rn', RS)
@pytest.mark.parametrize('K', sorted(FITS))
def test_the_two_sums_bracket_the_exact_value(K, Rn, noise):
    for minimize in (False, True):
        d, B, tab, kg, hi, exact = _all(K, Rn, noise, minimize=minimize)
        assert (kg >= 0).all() and (hi >= 0).all() and np.isfinite(hi).all()
        if Rn == 1:
            assert (kg == 0).all() and (hi == 0).all() and (exact == 0).all()
            continue
        tol = EPS_MAX * exact.max()
        assert exact.max() > 0
        assert (kg <= exact + tol).all(), float((kg - exact).max() / exact.max())
        assert (exact <= hi + tol).all(), float((exact - hi).max() / exact.max())


def test_nodes_that_separate_every_breakpoint_recover_the_exact_value():
    """one node inside every piece of the envelope between its breakpoints in (-9, 9) (those beyond carry less than h(-9) = 1e-19 of a
    slope difference each), 0.0 and +-10: every line that matters wins at a node, and kg is the exact value"""
    d, B = _lines(42, 33, True)
    scale = G.kg_exact_rows(d, B).max()
    worst, most = 0.0, 0
    for i in range(NCAND):
        bb, aa, c = G.envelope(d, B[i])
        near = np.flatnonzero(np.abs(c) < 9.0)
        cc = c[near]
        ce = np.r_[c[0] - 2.0, c, c[-1] + 2.0]                      # piece k of the envelope is (ce[k], ce[k + 1])
        pieces = np.unique(np.r_[near, near + 1])
        z = np.unique(np.r_[-10.0, 0.5 * (ce[pieces] + ce[pieces + 1]), 0.0, 10.0])
        assert 3 <= z.size <= 32
        most = max(most, cc.size)
        m, s, lo, hi = G.node_table(d, B[i:i + 1], z)
        assert set(bb[near]) | set(bb[near + 1]) <= set(s[0])       # every line next to such a breakpoint wins somewhere
        kg, kg_hi = G.bounds(m, s, lo, hi, z)
        exact = G.kg_exact(d, B[i])
        worst = max(worst, abs(kg[0] - exact) / scale)
        assert kg_hi[0] >= exact - 1e-15 * scale
    assert most >= 10 and worst <= 1e-14, (most, worst)


def test_nested_grids_tighten_both_sums():
    for K in sorted(FITS):
        prev = first = None
        for J in (5, 9, 17):
            z = np.linspace(-4.0, 4.0, J)
            d, B, tab, kg, hi, exact = _all(K, 257, True, z=z)
            tol = 1e-14 * exact.max()
            if prev is not None:
                assert (kg >= prev[0] - tol).all() and (hi <= prev[1] + tol).all()
            first = first if prev is not None else float((hi - kg).max())
            prev = (kg, hi)
        assert (hi - kg).max() < first


def test_the_default_nodes_gap_is_the_recorded_one():
    gap = 0.0
    for K in sorted(FITS):
        for Rn in RS[1:]:
            for noise in (True, False):
                d, B, tab, kg, hi, exact = _all(K, Rn, noise)
                gap = max(gap, float((exact - kg).max() / exact.max()))
    print('default nodes: (exact - kg) / max exact = %.3e' % gap)
    assert G.MEASURED_DEFAULT_GAP / 4 <= gap <= 4 * G.MEASURED_DEFAULT_GAP, gap


def _mp_h(x):
    return x * mp.ncdf(x) + mp.npdf(x)


def _mp_bounds(m, s, bmin, bmax, z):
    """kg_ref.bounds' recurrence on one row in 50-digit arithmetic (the inputs are the doubles themselves)"""
    f = lambda x: mp.mpf(float(x))
    J = len(z)
    mp_, sp = f(m[0]), f(s[0])
    sk, ik = sp, mp_ - sp * f(z[0])
    qp, kg, hi = f(bmin), mp.mpf(0), mp.mpf(0)
    for j in range(1, J):
        mj, sj, zl, zr = f(m[j]), f(s[j]), f(z[j - 1]), f(z[j])
        qj = min(max((mj - mp_) / (zr - zl), sp), sj)
        hi += max(qj - qp, 0) * _mp_h(-abs(zl))
        qp = qj
        if sj > sk:
            ij = mj - sj * zr
            c = min(max((ik - ij) / (sj - sk), zl), zr)
            kg += (sj - sk) * _mp_h(-abs(c))
            sk, ik = sj, ij
        mp_, sp = mj, sj
    hi += max(f(bmax) - qp, 0) * _mp_h(-abs(f(z[J - 1])))
    return kg, hi


def _synthetic_lines(seed, T=16, Rn=200):
    """lines whose breakpoints spread over the whole node range, the tails of h included (the GPU tier's random factors give such)"""
    rng = np.random.default_rng(seed)
    d = -np.abs(rng.standard_normal(Rn)); d[rng.integers(Rn)] = 0.0
    return d, 0.4 * rng.standard_normal((T, Rn))


def test_the_restatements_own_error_against_50_digits():
    worst = 0.0
    z = G.DEFAULT_NODES
    sets = [_lines(K, Rn, noise) for K in sorted(FITS) for Rn, noise in ((33, True), (2000, True), (257, False))]
    sets += [_synthetic_lines(seed) for seed in (1, 2, 3)]
    for d, B in sets:
        m, s, lo, up = G.node_table(d, B, z)
        kg, hi = G.bounds(m, s, lo, up, z)
        ek = eh = 0.0
        for i in range(0, B.shape[0], 3):
            tk, th = _mp_bounds(m[i], s[i], lo[i], up[i], z)
            ek = max(ek, abs(float(mp.mpf(float(kg[i])) - tk))); eh = max(eh, abs(float(mp.mpf(float(hi[i])) - th)))
        worst = max(worst, ek / hi.max(), eh / hi.max())
    print('bounds against 50 digits: max |delta| / max kg_hi = %.3e' % worst)
    assert G.MEASURED_KG_ERR / 4 <= worst <= 4 * G.MEASURED_KG_ERR, worst


def test_mutants_are_caught():
    z = G.DEFAULT_NODES
    d, B, tab, kg, hi, exact = _all(42, 257, True)
    # a dropped reference row: the one every offset is measured from
    r = int(np.argmax(d))
    keep = np.delete(np.arange(d.size), r)
    kg2, hi2 = G.bounds(*G.node_table(d[keep], B[:, keep], z), z)
    assert not np.array_equal(kg2, kg) and not np.array_equal(hi2, hi)
    # ... and one that wins a node of some candidate
    m, s, lo, up = tab
    r = int(np.flatnonzero(B[0] == s[0, -1])[0])
    keep = np.delete(np.arange(d.size), r)
    assert not np.array_equal(G.node_table(d[keep], B[:1, keep], z)[1], s[:1])
    # the tie rule: two reference rows that tie at the node 0.0
    z3 = np.array([-1.0, 0.0, 1.0])
    dt, Bt = np.array([0.0, 0.0]), np.array([[1.0, -1.0]])
    assert G.node_table(dt, Bt, z3)[1][0, 1] == 1.0 and G.node_table(dt, Bt, z3, tie='highest')[1][0, 1] == -1.0
    # the clamps: a crossing that rounding throws far outside its interval, and a chord slope outside its end slopes
    mt = np.array([[-1.0 + 1e-13, 0.0, 1.0 + 2.0 ** -52]]); st = np.array([[1.0, 1.0 + 2.0 ** -52, 1.0 + 2.0 ** -52]])
    a = G.bounds(mt, st, st[:, 0], st[:, -1], z3)
    b = G.bounds(mt, st, st[:, 0], st[:, -1], z3, clamp=False)
    assert a[0][0] != b[0][0] and a[1][0] != b[1][0]
    # one reference row: only the clamp makes the upper sum exactly 0
    d1, B1 = _lines(128, 1, True)
    t1 = G.node_table(d1, B1, z)
    assert (G.bounds(*t1, z)[1] == 0).all() and (G.bounds(*t1, z, clamp=False)[1] > 0).any()
    # the nodes
    for bad in (z + 0.01, np.r_[z[:15], z[16:]], np.r_[-1.0, 0.0, 0.0, 1.0], z[::-1], np.array([-1.0, 0.0]), np.linspace(-1, 1, 33)):
        with pytest.raises(ValueError):
            G.bounds(m, s, lo, up, bad)
    with pytest.raises(FloatingPointError):
        G.check_nodes(np.array([-1.0, 0.0, np.inf]))


def test_the_binding_has_the_headers_argument_types():
    from scfgp_amd import _lib
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    res, args = _lib.SIGNATURES['scfgp_acquire_kg']
    assert res is C.c_int
    assert args == [C.c_void_p, dp, C.c_int64, dp, dp, C.c_int64, dp, dp, dp, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, ip, dp, dp, dp]
