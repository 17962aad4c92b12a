"""CPU tier of the acquisition range tests (tests/acquire_range.py has the models): the numpy restatements tests/acquire_ref.py and
tests/kg_ref.py against 60-digit mpmath per row, value and both partials, under the error models that the GPU tier
(tests/test_gpu_acquire_range.py) then holds the device to; the mutants that those assertions must reject, and the norm-wise check that
lets one of them through; the fixture tests/golden/acquire_kats.npz; dry runs on the oracle's features of every input condition that the
GPU tier asserts, so that its scales, incumbents and pool sizes are settled here."""
import os

import mpmath as mp
import numpy as np
import pytest

from tests import acquire_range as AR
from tests import acquire_ref as A
from tests import kg_ref as G
from tests import pred_cov_ref as PC
from tests import pred_grad_ref as PG
from tests.golden import make_acquire_kats as K

mp.mp.dps = K.DPS
KATS = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'acquire_kats.npz'))


def _mpf(x):
    return mp.mpf(float(x))


def truth(kind, mu, sd, best=None, xi=0.0, fstar=None, minimize=False):
    """{'acq', 'au', 'as'}: lists of mpmath values, every row from the call's own doubles"""
    sgn = -1 if minimize else 1
    out = {k: [] for k in AR.OUTPUTS}
    for m, s in zip(mu, sd):
        u, s = sgn * _mpf(m), _mpf(s)
        if kind == 'mes':
            g = (sgn * _mpf(fstar[0]) - u) / s
            q = K.mes_q(g)
            row = (K.mes_term(g), q / s, g * q / s)
        else:
            g = (u - sgn * _mpf(best) - _mpf(xi)) / s
            if kind == 'pi':
                row = (K.Phi(g), K.phi(g) / s, -g * K.phi(g) / s)
            elif kind == 'ei':
                row = (s * K.h(g), K.Phi(g), K.phi(g))
            else:
                row = (mp.log(s) + K.log_h(g), K.Phi(g) / (s * K.h(g)), K.phi(g) / (s * K.h(g)))
        for k, v in zip(AR.OUTPUTS, row):
            out[k].append(v)
    return out


_TRUTHS = {}


def grid_truth(kind, minimize):
    """[(mu, sd, kwargs, g, truth)] of AR.grid_calls, computed once"""
    key = (kind, minimize)
    if key not in _TRUTHS:
        _TRUTHS[key] = [(mu, sd, kw, AR.g_of(kind, mu, sd, **kw), truth(kind, mu, sd, **kw)) for mu, sd, kw in AR.grid_calls(kind, minimize)]
    return _TRUTHS[key]


def worst_constants(kind, minimize, acquire=A.acquire):
    """{output: (worst constant, g there)} of `acquire` against mpmath over the grid"""
    worst = {k: (0.0, None) for k in AR.OUTPUTS}
    for mu, sd, kw, g, tr in grid_truth(kind, minimize):
        got = AR.restatement(kind, mu, sd, acquire=acquire, **kw)
        for k in AR.OUTPUTS:
            diff = [float(abs(_mpf(v) - t)) if np.isfinite(v) else np.inf for v, t in zip(got[k], tr[k])]
            c = AR.constants(kind, k, got[k], [float(t) for t in tr[k]], g, diff=diff)
            i = int(np.argmax(c))
            if c[i] > worst[k][0]:
                worst[k] = (float(c[i]), float(g[i]))
    return worst


# ---- 1. the restatement under the models ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('minimize', [False, True])
@pytest.mark.parametrize('kind', AR.KINDS)
def test_restatement_constants(kind, minimize):
    w = worst_constants(kind, minimize)
    print('%s minimize=%d: %s' % (kind, minimize, '  '.join('%s %.2f at g = %r (C_REF %.2f)' % (k, w[k][0], w[k][1], AR.C_REF[kind][k])
                                                         for k in AR.OUTPUTS)))
    for k in AR.OUTPUTS:
        assert w[k][0] <= AR.REF_FACTOR * AR.C_REF[kind][k], (k, w[k])


def test_the_grid_is_the_one_the_models_were_set_on():
    for kind in AR.KINDS:
        uni, sp = AR.grid(kind)
        assert uni[0] == -60.0 and uni[-1] == (40.0 if kind == 'mes' else 9.0) and np.allclose(np.diff(uni), 0.1)
        for s in AR.SEAMS:
            assert np.isin(AR.around(s), sp).all() and AR.around(s)[2] == s and np.unique(AR.around(s)).size == 5
        assert np.isin([0.0], sp).all() and np.signbit(sp[sp == 0.0]).any() and not np.signbit(sp[sp == 0.0]).all()
        for mu, sd, kw in AR.grid_calls(kind, False)[1:]:
            g = AR.g_of(kind, mu, sd, **kw)
            assert np.isin(sp, g[sd == 1.0]).all()                # at sigma = 1 the special points are met bit for bit
            assert set(sd) == set(AR.SIGMAS)
    assert np.isin(AR.DECADES, AR.grid('logei')[1]).all() and np.isin([38.0], AR.grid('ei')[1]).all()
    assert np.isin([-1e2, -1e3, -1e4], AR.grid('mes')[1]).all()


def test_outputs_are_finite_and_signed_as_promised():
    for minimize in (False, True):
        for mu, sd, kw in AR.grid_calls('logei', minimize):
            assert all(np.isfinite(v).all() for v in A.acquire('logei', mu, sd, **kw))
        for kind in ('pi', 'ei'):
            for mu, sd, kw in AR.grid_calls(kind, minimize):
                acq = A.acquire(kind, mu, sd, **kw)[0]
                assert np.isfinite(acq).all() and (acq >= 0).all() and not np.signbit(acq).any()
        for mu, sd, kw in AR.grid_calls('mes', minimize):
            assert (A.acquire('mes', mu, sd, **kw)[0] >= 0).all()


# ---- 2. mutants ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(AR.MUTANTS))
def test_mutants_fail_the_per_row_assertion(name):
    kinds, acquire = AR.MUTANTS[name]
    for kind in kinds:
        w = worst_constants(kind, False, acquire=acquire)
        over = {k: w[k] for k in AR.OUTPUTS if not w[k][0] <= AR.REF_FACTOR * AR.C_REF[kind][k]}
        print('%s, %s: %s' % (name, kind, '  '.join('%s %.3g at g = %r' % (k, v[0], v[1]) for k, v in over.items())))
        assert over, (name, kind, w)
        # ... and the device's allowance, 8 x C_REF, does not let it through either
        assert any(not w[k][0] <= 2 * AR.DEVICE_FACTOR * AR.C_REF[kind][k] for k in AR.OUTPUTS), (name, kind, w)


def test_the_norm_wise_chain_check_lets_the_ei_mutant_through():
    """the gap: tests/test_gpu_acquire.py::test_gradient_against_chained_partials on its own pool with its incumbent, the median -- no
    row is in EI's tail, so the mutant passes unseen; the per-row measure with g placed in the tail rejects every row of it"""
    from tests.test_gpu_acquire import CHAIN_BOUND, SHAPE_A, rel
    from scfgp_amd import synth
    D, S, M, T = SHAPE_A
    params, alpha, Li = AR.synthetic_factors(D, S, M)
    Xs = synth.make_X(101, T, D)
    mu, sd_star, dmu, dstd = PG.predict_grad(Xs, alpha, Li, params, S, M)
    mu = mu.ravel()
    mutant = AR.MUTANTS['EI tail: a_u = a_sigma = 0'][1]
    kw = dict(best=float(np.median(mu)), xi=0.01)
    _, au, as_ = A.acquire('ei', mu, sd_star, **kw)
    _, au_m, as_m = mutant('ei', mu, sd_star, **kw)
    ref = au[:, None] * dmu + as_[:, None] * dstd
    bad = au_m[:, None] * dmu + as_m[:, None] * dstd
    assert rel(bad, ref) <= CHAIN_BOUND                           # passes: the existing check cannot see the mutant
    # the per-row check on the same fit with g placed in the tail does: every tail row is off by its whole value
    g = AR.g_of('ei', mu, sd_star, **kw)
    assert (g > -1.0).all()
    kw = dict(best=float(mu.max() + 3 * np.median(sd_star)), xi=0.0)
    g = AR.g_of('ei', mu, sd_star, **kw)
    _, au, as_ = A.acquire('ei', mu, sd_star, **kw)
    _, au_m, as_m = mutant('ei', mu, sd_star, **kw)
    assert (g < -1.0).all() and (AR.constants('ei', 'au', au_m, au, g) > 1e10).all()


# ---- 3. the fixture ------------------------------------------------------------------------------------------------------------------
def test_acquire_kats_file_is_what_its_generator_writes():
    fresh = K.build()
    assert sorted(KATS.files) == sorted(fresh)
    for k in KATS.files:
        assert np.array_equal(KATS[k], fresh[k]) and np.array_equal(np.signbit(KATS[k]), np.signbit(fresh[k])), k
    g = KATS['g']
    for s in AR.SEAMS:
        assert np.isin(AR.around(s), g).all()
    assert np.isin(np.r_[-38.0, -38.5, -39.0, AR.DECADES, 0.0, 8.3, 38.0], g).all() and np.unique(g).size == g.size == 22
    # phi leaves the normal range between -38 and -39
    phi = dict(zip(g, KATS['phi']))
    assert 0 < phi[-38.5] < AR.TINY < 1e-300 > phi[-38.0] > 0 and phi[-39.0] == 0.0


# measured: the building blocks at the fixture's g in the models' units: Phi 0.39, phi 0.52, h 1.50, log h 2.10, Phi / h 2.63, phi / h 1.72,
# MES term 0.98, q 1.04
def test_restatement_at_the_fixture_points():
    g = KATS['g']
    rows = [('pi', 'acq', 'Phi', A.cdf(g)), ('pi', 'acq', 'phi', A.pdf(g)), ('ei', 'acq', 'h', A.h(g)), ('logei', 'acq', 'log_h', A.log_h(g)),
            ('logei', 'au', 'Phi_over_h', A.h_ratios(g)[0]), ('logei', 'as', 'phi_over_h', A.h_ratios(g)[1]),
            ('mes', 'acq', 'mes_term', A.mes_term(g)), ('mes', 'au', 'mes_q', A.mes_q(g))]
    for kind, out, key, got in rows:
        c = AR.constants(kind, out, got, KATS[key], g)
        print('%-10s worst %.2f at g = %r' % (key, c.max(), g[int(np.argmax(c))]))
        assert (c <= AR.REF_FACTOR * AR.C_REF[kind][out]).all(), key


# ---- 4. dry runs of the GPU tier's input conditions, on the oracle's features ---------------------------------------------------------------
@pytest.mark.parametrize('noise', [False, True])
@pytest.mark.parametrize('minimize', [False, True])
@pytest.mark.parametrize('kind', AR.KINDS)
def test_dry_run_of_the_dense_sweep(kind, minimize, noise):
    D, S, M = AR.SHAPE
    params, alpha0, Li = AR.synthetic_factors(D, S, M)
    Xs = AR.sweep_pool()
    mu0, sd = AR.oracle_mu_sd(Xs, params, alpha0, Li, noise)
    scale, kw = AR.place(kind, mu0, sd, minimize)
    mu, sd = AR.oracle_mu_sd(Xs, params, scale * alpha0, Li, noise)
    g = AR.g_of(kind, mu, sd, **kw)
    print('%s minimize=%d noise=%d: scale %.4g, g in [%.2f, %.2f]' % (kind, minimize, noise, scale, g.min(), g.max()))
    assert Xs.shape[0] <= 4096
    assert AR.sweep_coverage(g, -60, 40 if kind == 'mes' else 8) == []
    assert AR.in_measured_range(kind, g).sum() >= 0.8 * g.size
    # the restatement on these very rows stays inside 4 x its constants (every 16th row: mpmath)
    sel = np.arange(0, g.size, 16)
    sel = sel[AR.in_measured_range(kind, g[sel])]
    tr = truth(kind, mu[sel], sd[sel], **kw)
    got = AR.restatement(kind, mu[sel], sd[sel], **kw)
    for k in AR.OUTPUTS:
        diff = [float(abs(_mpf(v) - t)) for v, t in zip(got[k], tr[k])]
        c = AR.constants(kind, k, got[k], [float(t) for t in tr[k]], g[sel], diff=diff)
        assert (c <= AR.REF_FACTOR * AR.C_REF[kind][k]).all(), (k, c.max())


@pytest.mark.parametrize('noise', [False, True])
@pytest.mark.parametrize('minimize', [False, True])
def test_dry_run_of_the_ladder(minimize, noise):
    D, S, M = AR.SHAPE
    params, alpha0, Li = AR.synthetic_factors(D, S, M)
    mu0, _ = AR.oracle_mu_sd(AR.ladder_pool(), params, alpha0, Li, noise)
    Xs = AR.ladder_pool(AR.ladder_direction(mu0, minimize))
    mu, sd = AR.oracle_mu_sd(Xs, params, AR.LADDER_SCALE * alpha0, Li, noise)
    kw = dict(best=float(mu[0]), xi=0.0, minimize=minimize)
    g = AR.g_of('logei', mu, sd, **kw)
    print('ladder minimize=%d noise=%d: g in [%.3g, %.3g], rows per decade of -g from 1e2: %s'
          % (minimize, noise, g.min(), g.max(), [int(((-g >= 10.0 ** x) & (-g < 10.0 ** (x + 1))).sum()) for x in range(2, 7)]))
    assert g[0] == 0.0 and AR.decade_coverage(g) == []
    sel = np.flatnonzero(AR.in_measured_range('logei', g))[::8]
    tr = truth('logei', mu[sel], sd[sel], **kw)
    got = AR.restatement('logei', mu[sel], sd[sel], **kw)
    for k in AR.OUTPUTS:
        diff = [float(abs(_mpf(v) - t)) for v, t in zip(got[k], tr[k])]
        c = AR.constants('logei', k, got[k], [float(t) for t in tr[k]], g[sel], diff=diff)
        assert (c <= AR.REF_FACTOR * AR.C_REF['logei'][k]).all(), (k, c.max())


@pytest.mark.parametrize('noise', [False, True])
def test_dry_run_of_the_exact_g_construction(noise):
    """every fixture g is met bit for bit on some row of the pool by an incumbent that the host can find"""
    D, S, M = AR.SHAPE
    params, alpha0, Li = AR.synthetic_factors(D, S, M)
    _, sd = AR.oracle_mu_sd(AR.exact_pool(), params, 0 * alpha0, Li, noise)
    hits = []
    for j, gw in enumerate(KATS['g']):
        found = AR.hit(gw, sd, start=7 * j)
        if found is not None:
            i, p0 = found
            hits.append((0.0 - p0 - 0.0) / sd[i])
            assert hits[-1] == gw
    assert AR.exact_condition(hits, KATS['g']) == []
    assert AR.exact_condition([h for h in hits if h != -1.0], KATS['g']) == [('seam', -1.0)] and AR.exact_condition([h for h in hits if h != -1e5], KATS['g']) == [('point', -1e5)]


# ---- 5. knowledge gradient with two reference lines -------------------------------------------------------------------------------------
def _kg_truth(d, B):
    out = []
    for b1, b2 in B:
        db = abs(_mpf(b2) - _mpf(b1))
        out.append(db * K.h(-abs(_mpf(d[0]) - _mpf(d[1])) / db) if db != 0 else mp.mpf(0))
    return out


def _slope_pairs(n, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, 2)) * np.exp(rng.uniform(-3.0, 1.0, (n, 1)))
    B[: n // 4, 1] = B[: n // 4, 0] * (1.0 + rng.uniform(-0.1, 0.1, n // 4))        # nearly parallel lines: crossings far out
    return B


# measured: DEFAULT_NODES 0.92 (bounds()), 1.57 (closed form); WIDE_NODES 0.51, 0.51; with the first term of the model alone 746 and 11705
@pytest.mark.parametrize('nodes', ['default', 'wide'])
def test_kg_two_lines_against_mpmath(nodes):
    z = G.DEFAULT_NODES if nodes == 'default' else AR.WIDE_NODES
    B = _slope_pairs(300, 11)
    worst = {'bounds': 0.0, 'closed': 0.0, 'one_term': 0.0}
    seen_in = seen_out = 0
    for delta in AR.KG_DELTAS:
        for d in (np.array([0.0, -delta]), np.array([-delta, 0.0])):
            true = _kg_truth(d, B)
            tf = np.array([float(t) for t in true])
            closed, c, zstar = AR.kg_closed_form(d, B)
            inside, outside = AR.kg_classes(zstar, z)
            kg, hi = G.bounds(*G.node_table(d, B, z), z)
            assert (kg[outside] == 0.0).all()
            unit = AR.kg_unit(c, B, z, tf)
            for name, got, rows in (('bounds', kg, inside), ('closed', closed, np.ones(len(B), bool))):
                for i in np.flatnonzero(rows):
                    dd = float(abs(_mpf(got[i]) - true[i]))
                    if abs(tf[i]) < AR.TINY:
                        assert dd <= AR.TINY
                        continue
                    worst[name] = max(worst[name], dd / unit[i])
                    if name == 'bounds':
                        worst['one_term'] = max(worst['one_term'], dd / (AR.EPS * (1 + c[i] ** 2) * abs(tf[i])))
            assert (hi >= closed * (1.0 - AR.REF_FACTOR * AR.C_REF_KG * unit / np.maximum(np.abs(tf), AR.TINY)) - AR.TINY).all()
            seen_in += int(inside.sum()); seen_out += int(outside.sum())
    print('kg two lines, %s nodes: bounds() %.2f, closed form %.2f of the two-term model (C_REF_KG %.2f); with the first term alone %.1f'
          % (nodes, worst['bounds'], worst['closed'], AR.C_REF_KG, worst['one_term']))
    assert seen_in > 500 and seen_out > 100
    assert worst['bounds'] <= AR.REF_FACTOR * AR.C_REF_KG and worst['closed'] <= AR.REF_FACTOR * AR.C_REF_KG
    assert worst['one_term'] > 10 * AR.REF_FACTOR * AR.C_REF_KG       # the second term is not an ornament: do not drop it


@pytest.mark.parametrize('noise', [False, True])
@pytest.mark.parametrize('minimize', [False, True])
def test_dry_run_of_the_kg_pool(minimize, noise):
    D, S, M = AR.SHAPE
    params, alpha0, Li = AR.synthetic_factors(D, S, M)
    Xc, Xr = AR.kg_pools()
    kap = PC.kappa(params)
    Cc, Cr = PC.factor(Xc, Li, params, S, M), PC.factor(Xr, Li, params, S, M)
    _, sd = AR.oracle_mu_sd(Xc, params, alpha0, Li, noise)
    B = G.slopes(kap * (Cc @ Cr.T), sd)
    mu_r0, _ = AR.oracle_mu_sd(Xr, params, alpha0, Li, noise)
    cs = []
    for mult in AR.KG_DELTAS[1:]:
        d = G.offsets(AR.kg_scale(mult, mu_r0, B) * mu_r0, minimize)
        cs.append(AR.kg_closed_form(d, B)[1])
    c = np.concatenate(cs)
    assert Xc.shape == (AR.T_KG, D) and Xr.shape == (2, D)
    assert AR.kg_coverage(c) == [], AR.kg_coverage(c)
    assert np.count_nonzero((c > 38) & (c < 60)) >= 4 and np.count_nonzero(c > 60 * (1 + AR.BORDER)) >= 4
