"""
CPU tier of the range tests of scfgp_sobol's sin / cos sites (tests/sobol_range.py): the emulation of the device's psi (fast_sincos
restated line by line in tests/sincos_ref.py, the sinc series in true fmas) stays inside every derived bound on every case of the GPU
tier, each mutant exceeds one by at least 100 x, the cases really reach the branches and edges they are there for, and the case that was
found -- uniform on 2.5 2^30 +- 1/8 with max |Om| = 1 -- fails by ten orders of magnitude with the routine's own quadrant while phibar
and every single phase stay in order.  The library refuses that case (tests/test_gpu_sobol_range.py).
Output (-s): per case the worst error over its bound.
Measured here: pair level <= 3.1e-3 of the theta = 0 bound (the d3 main effects; most cases below 1e-4); sinc |error| |t| <= 1.25 eps
of 2.54 eps, and 0.27 eps of 2 eps in the series; the normal amplitude <= 0.27 of its bound; phase factors <= 0.50 of 2 L.  Mutants:
quadrant_wrap 5.5e10, series_to_2 1.3e6, left_edge 1.7e10, no_half_exp 1.4e15 times a bound.
"""
import numpy as np
import pytest

from tests import sincos_ref as S
from tests import sobol_range as SR
from tests import sobol_ref as R

ID = lambda c: c['name'].replace(' ', '_')


@pytest.fixture(scope='module')
def kats():
    return S.load_kats()


@pytest.mark.parametrize('geom', sorted(SR.GEOMETRIES))
def test_geometries_are_exact(geom):
    from oracle import scfgp_oracle as O
    D, S_, M, params = SR.GEOMETRIES[geom]
    Om, s = SR.check_geometry(D, S_, M, params)
    a, b, c, l_F, r_F, F, l_FC, FC = O.unpack_params(params, D, S_, M)
    assert np.all(l_FC == 0) and np.all(FC == 0) and (a, b, c) == (0, 0, 0)
    J = S_ + M
    assert -(-J // 8) * 8 == 16                                        # two blocks of the pair kernel's tile edge
    cols = [tuple(Om[:, j]) for j in range(J)]
    assert any(all(v == 0 for v in c_) for c_ in cols), 'no zero column'
    assert len(set(cols)) < J, 'no repeated column'
    assert any(tuple(-v for v in cols[j]) == cols[k] and any(cols[j]) for j in range(J) for k in range(J)), 'no pair Om_j = -Om_k'
    nz = np.abs(Om[Om != 0])
    print('%s: J = %d, |Om| from 2^%.1f to %g' % (geom, J, np.log2(nz.min()), nz.max()))
    if geom != 'pow2':
        assert nz.max() / nz.min() >= (2.0 ** 9 if D > 1 else 8)


def test_grid_of_measures():
    """the centres and half widths of the issue, all of them but the one pair whose ends are no doubles"""
    left_out = [(c, h) for c in SR.CENTRES for h in SR.HALF_WIDTHS if not SR.representable(c, h)]
    assert left_out == [(2.0 ** 30, 2.0 ** -30)]
    names = {c['name'] for c in SR.CASES}
    assert len(names) == len(SR.CASES)
    for g in ('d1', 'd3', 'd17'):
        assert sum(n.startswith(g + ' uniform c=') for n in names) >= 11 and sum(n.startswith(g + ' normal') for n in names) == len(SR.NORMALS)
    assert max(abs(m) for m, _ in SR.NORMALS) == 2.0 ** 24 and {sd for _, sd in SR.NORMALS} >= {2.0 ** -8, 2.0 ** 3}


def test_diagonal_geometry_reads_raw_psi(kats):
    """E_j = psi_j(1) bit for bit in the order of sobol_tables_kernel: psi_d(0) = {1, 0} and cmul with {1, 0} are exact"""
    D, S_, M, params = SR.diagonal()
    Om, b, s = R.phases(params, D, S_, M)
    assert s == 0.5 and np.all(b == 0) and np.array_equal(Om, np.concatenate((np.eye(D), np.zeros((D, M))), 1))
    rng = np.random.default_rng(1)
    z = np.concatenate((rng.choice(kats['z'], 40), rng.choice(kats['zb'], 24)))
    kind = np.zeros(D, np.int32)
    re, im = SR.emul_tables_E(Om, b, kind, z, z)                       # a point mass per input
    sn, cs = S.emul_sincos64(z)
    assert np.array_equal(re[:D], cs) and np.array_equal(im[:D], sn) and np.all(re[D:] == 1) and np.all(im[D:] == 0)
    # the amplitudes alone: centre 0, so the sine half is an exact zero
    t = np.concatenate((SR.SINC_POINTS, rng.uniform(0, 3, D - len(SR.SINC_POINTS))))
    re, im = SR.emul_tables_E(Om, b, kind, -t, t)
    assert np.array_equal(re[:D], SR.sinc(t)) and np.all(im == 0)
    t = SR.NORMAL_POINTS[:D]
    re, im = SR.emul_tables_E(Om, b, np.ones(D, np.int32), np.zeros(D), t)
    assert np.array_equal(re[:D], SR.normal_amp(t)) and np.all(im == 0)


def _sinc_points():
    k = S.load_kats()
    return np.concatenate((SR.SINC_POINTS, -SR.SINC_POINTS, k['z'], k['zb']))


def _single_value_ratios(mutate=None):
    """{site: worst |emulation - truth| / bound} over the single-value points of sobol_range and, for sinc, the fixture's phases"""
    out = {}
    t = _sinc_points()
    out['sinc'] = float(np.max(S.abs_err(SR.sinc(t, mutate), SR.sinc_truth(t)) / SR.sinc_bound(t)))
    t = SR.NORMAL_POINTS
    err = np.abs(SR.normal_amp(t, mutate).astype(np.longdouble) - SR.normal_truth(t)).astype(np.float64)
    out['normal'] = float(np.max(err / SR.normal_bound(t)))
    return out


def test_single_values_inside_their_bounds(kats):
    r = _single_value_ratios()
    t = _sinc_points()
    e = S.abs_err(SR.sinc(t), SR.sinc_truth(t))
    hi = np.abs(t) >= 0.5
    print('sinc: worst |error| |t| = %.2f eps of %.2f eps (|t| >= 1/2), %.2f eps of 2 eps in the series; normal amplitude %.2f of its bound'
          % ((e[hi] * np.abs(t[hi])).max() / SR.EPS, (2 * SR.L + SR.EPS) / SR.EPS, e[~hi].max() / SR.EPS, r['normal']))
    assert r['sinc'] <= 1 and r['normal'] <= 1, r
    # the exact-zero edge of the normal amplitude
    assert SR.normal_amp(np.array([38.604]))[0] == 0.0 and 0.0 < SR.normal_amp(np.array([38.6037]))[0] < 2.0 ** -1022
    assert SR.sinc(np.array([0.0, 5e-324]))[0] == 1.0 and SR.sinc(np.array([5e-324]))[0] == 1.0
    # the phase factor through psi, at a point mass: the fixture's hard groups and its block beyond
    for z, sn, cs in ((kats['z'], kats['sin'], kats['cos']), (kats['zb'], kats['sinb'], kats['cosb'])):
        p = SR.dev_psi(np.zeros(1, int), np.ones(1), np.ones(1), z[None, :])[0]          # a point mass at 1, Om = z
        w = max(S.abs_err(p.real, cs).max(), S.abs_err(p.imag, sn).max())
        print('phase factor: worst / (2 L) = %.3f over %d phases' % (w / (2 * SR.L), len(z)))
        assert w <= 2 * SR.L


@pytest.mark.parametrize('case', SR.CASES, ids=ID)
def test_emulation_inside_the_pair_bounds(case):
    r = SR.ratios(SR.emulated(case), case)
    print('%-40s error / bound %s' % (case['name'], ' '.join('%s=%.1e' % kv for kv in sorted(r.items()))))
    assert sorted(r) == sorted(SR.ALL) and all(v <= 1 for v in r.values()), r
    if case['D'] == 1:                                                  # three code paths to one number
        dev, bd = SR.emulated(case), R.bounds(SR.reference(case), 1)
        for k in ('Vmain', 'Vtot'):
            assert np.all(np.abs(dev['V'] - dev[k][:, 0]) <= bd['V'] + bd[k][:, 0]), k


def test_the_case_that_was_found():
    """uniform on 2.5 2^30 +- 1/8, Om = (1, 1/2, 1/4, 3/4, -1, 0, 1, 1/8, 5/8): every single phase is inside the domain of fast_sincos and
    phibar is right, the pair phases reach 5.4e9 and V, Vmain, Vtot are wrong by ten orders of magnitude over the exact-phase bound.
    With the right quadrant (the reduction itself is still exact there) the same arithmetic is inside the bound."""
    c = SR.WRAP_CASE
    m0, m1 = SR.measure_form(c['kind'], c['p0'], c['p1'])
    single = np.abs(c['Om'] * m0[:, None]) + np.abs(c['Om'] * m1[:, None])
    z, t, _ = SR.pair_phases(c)
    assert single.max() < 2.7e9 < SR.PHASE_LIMIT < 5.3e9 < np.abs(z).max() and c['Rd'][0] >= SR.PHASE_LIMIT
    good = SR.ratios(SR.emulated(c), c)
    bad = SR.ratios(SR.emulated(c, 'quadrant_wrap'), c)
    print('beyond the domain: repaired quadrant %s\n                   the routine\'s own  %s' % (
        ' '.join('%s=%.1e' % kv for kv in sorted(good.items())), ' '.join('%s=%.1e' % kv for kv in sorted(bad.items()))))
    assert all(v <= 1 for v in good.values())
    assert all(bad[k] >= 100 for k in ('V', 'Vmain', 'Vtot')) and bad['phibar'] <= 1 and bad['f0'] <= 1
    # under the documented bound, with its Theta term, the miss is still there but eight orders smaller: that term hides quadrants
    ref = dict(SR.reference(c)); ref['theta'] = float(np.max(2 * np.abs(c['Om']) * np.maximum(np.abs(c['p0']), np.abs(c['p1']))[:, None]))
    full = R.worst_ratio(SR.emulated(c, 'quadrant_wrap'), ref, 1)
    print('                   under the bound with Theta = %.3g: %s' % (ref['theta'], ' '.join('%s=%.1e' % kv for kv in sorted(full.items()))))
    assert 1 < full['V'] < bad['V'] * 1e-6


@pytest.mark.parametrize('mut', SR.MUTATIONS)
def test_mutant_exceeds_a_bound_by_100(mut):
    worst = dict(('single ' + k, v) for k, v in _single_value_ratios(mut).items())
    cases = [SR.WRAP_CASE] if mut == 'quadrant_wrap' else SR.CASES
    for c in cases:
        r = SR.ratios(SR.emulated(c, mut), c)
        k = max(r, key=r.get)
        worst[c['name'] + ' ' + k] = r[k]
    top = max(worst, key=worst.get)
    n = sum(v >= 100 for v in worst.values())
    print('%-14s worst error / bound %.2e (%s); %d of %d checks reject it by 100 x' % (mut, worst[top], top, n, len(worst)))
    assert worst[top] >= 100


def test_coverage_of_the_pair_cases():
    zmax, hits, big = 0.0, dict.fromkeys(('series', 'sine', 't0', 'half', 'below_half', 'denormal', 'amp_zero', 'amp_denormal'), 0), 0
    for c in SR.CASES:
        z, t, kind = SR.pair_phases(c)
        u, n = np.abs(t[kind == 0]), np.abs(t[kind == 1])
        zmax = max(zmax, float(np.abs(z).max()))
        hits['series'] += int(np.any((u < 0.5) & (u > 0))); hits['sine'] += int(np.any(u >= 0.5))
        hits['t0'] += int(np.any(u == 0)); hits['half'] += int(np.any(u == 0.5)); hits['below_half'] += int(np.any(u == SR.BELOW_HALF))
        hits['denormal'] += int(np.any((u > 0) & (u < 2.0 ** -1022)))
        amp = SR.normal_amp(n)
        hits['amp_zero'] += int(np.any((amp == 0) & (n >= 38.604))); hits['amp_denormal'] += int(np.any((amp > 0) & (amp < 2.0 ** -1022)))
        ref = SR.reference(c)
        with np.errstate(invalid='ignore'):
            big += int(np.all(np.abs(ref['V']) >= 1e-3 * ref['Sabs_all']) and np.all(ref['Sabs_all'] > 0))
    print('coverage: %s; largest pair phase %.3g; V / Sabs >= 1e-3 in %d of %d cases' % (hits, zmax, big, len(SR.CASES)))
    assert all(v > 0 for v in hits.values()), hits
    assert zmax > 1e9 and any(2.0 ** 20 * np.pi / 2 < np.abs(SR.pair_phases(c)[0]).max() < 1e9 for c in SR.CASES)
    assert 2 * big >= len(SR.CASES)
    assert len(SR.GROUP_CASES) >= 10 and all(c['D'] == 17 for c in SR.GROUP_CASES)        # a prefix and a suffix cut at input 16
