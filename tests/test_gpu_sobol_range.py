"""
GPU tier of the range tests of scfgp_sobol's sin / cos sites (sobol.hip: psi, sinc, the normal amplitude in sobol_tables_kernel and in
the three product chains of sobol_pairs_kernel) and of the refusal that keeps the pair phases inside the domain of fast_sincos.  The
geometries, measures, truths and bounds are those of tests/sobol_range.py: every phase is an exact double, so the variances are held
to sobol_ref.bounds with theta = 0 and the single psi values to bounds of a few 2^-53.  Nothing here is taken from a kernel.
Output (-s): per case the worst error over its bound.
Measured on an MI355X, worst error / bound: tables, phase 0.497 of 2 L over 3362 phases; sinc 0.136 in the series and 0.478 from 1/2 on;
normal amplitude inside its bound, at exactly one denormal spacing (ratio 1.0000) on denormal results, where the device's exp is not
correctly rounded; pairs V 1.1e-3, Vmain 4.3e-3, Vtot 6.0e-4, f0 2.2e-6, phibar 6.7e-6 over the 60 cases.
"""
import ctypes as C

import numpy as np
import pytest

from scfgp_amd._lib import dptr
from tests import sincos_ref as S
from tests import sobol_range as SR
from tests import sobol_ref as R

pytestmark = pytest.mark.gpu

ID = lambda c: c['name'].replace(' ', '_')
HARD = ('npio2', 'flip', 'tie', 'special', 'quadrant')
FILLER = 512                                                     # phases of the fixture's 'filler' group that the phase test runs
REFUSAL = "sobol: input %d: the measure's phases leave the sin/cos domain (2 max|Om| |x| < 3.37e9)"
_ENG = {}


def engine(D, S_, M, params, dtype='f64'):
    """one context per geometry and type for the whole module, its unpacked Fall checked bit for bit: Om dyadic as built, row D zero"""
    key = (D, S_, M, dtype, params.tobytes())
    if key not in _ENG:
        from scfgp_amd.engine import HipEngine
        eng = HipEngine(D, S_, M, dtype=dtype); eng.set_params(params)
        d = eng.dims()
        assert np.array_equal(eng.debug_read('Fall', (d['Dp'], d['Jp'])), SR.expected_fall(D, S_, M, params, d['Dp'], d['Jp']))
        _ENG[key] = eng
    return _ENG[key]


@pytest.fixture(scope='module', autouse=True)
def _close_engines():
    yield
    for eng in _ENG.values():
        eng.close()
    _ENG.clear()


def case_engine(case, dtype='f64'):
    return engine(case['D'], case['S'], case['M'], case['params'], dtype)


def run(eng, case, want=SR.ALL):
    return eng.sobol(case['kind'], case['p0'], case['p1'], case['W'], want=want)


# ---- tables: 64 raw psi values per call through the diagonal geometry ------------------------------------------------------------
def diagonal_psi(kind, p0, p1):
    """(Re psi, Im psi) of psi_j(1) under per-input measures, any number of them: calls of 64 with want = ('phibar',); the eight
    frequency-free columns behind them must read {1, 0} exactly"""
    D, S_, M, params = SR.diagonal()
    eng = engine(D, S_, M, params)
    J = S_ + M
    n = len(p0)
    re, im = np.empty(n), np.empty(n)
    for i in range(0, n, D):
        m = min(D, n - i)
        k = np.zeros(D, np.int32); a = np.zeros(D); b = np.zeros(D)
        k[:m] = kind; a[:m] = p0[i:i + m]; b[:m] = p1[i:i + m]
        pb = eng.sobol(k, a, b, None, want=('phibar',))['phibar'] / 0.5
        assert np.all(pb[D:J] == 1.0) and np.all(pb[J + D:] == 0.0) and np.all(pb[m:D] == 1.0) and np.all(pb[J + m:J + D] == 0.0)
        re[i:i + m] = pb[:m]; im[i:i + m] = pb[J:J + m]
    return re, im


def test_tables_phase():
    """Every phase of the hard groups of sincos_kats.npz (npio2, flip, tie, special, quadrant), the whole block beyond |fn| = 2^20
    (|z| up to 1e9) and 512 phases of 'filler' as point masses, 64 per call: Re and Im of phibar / s within 2 L of mpmath's cos and sin.
    Phases run: 3362 = 2034 of the hard groups (all of them) + 512 of filler + 816 beyond (all of them), in 53 calls."""
    k = S.load_kats()
    hard = np.isin(k['group'], [k['groups'].index(g) for g in HARD])
    fill = np.flatnonzero(~hard)[:FILLER]
    pick = np.concatenate((np.flatnonzero(hard), fill))
    z = np.concatenate((k['z'][pick], k['zb']))
    sn = np.concatenate((k['sin'][pick], k['sinb'])); cs = np.concatenate((k['cos'][pick], k['cosb']))
    assert hard.sum() + len(fill) == len(pick) and len(fill) == FILLER and 2 * np.abs(z).max() < SR.PHASE_LIMIT
    re, im = diagonal_psi(0, z, z)
    e = np.maximum(S.abs_err(re, cs), S.abs_err(im, sn))
    i = int(e.argmax())
    msg = 'sobol_range tables, phase: %d phases (%d hard, %d filler, %d beyond), worst / (2 L) = %.4f at z = %r' % (
        len(z), hard.sum(), len(fill), len(k['zb']), e.max() / (2 * SR.L), z[i])
    print('\n' + msg)
    assert e.max() <= 2 * SR.L, msg


def test_tables_amplitudes():
    """Centre or mean 0: phibar[j] / s is the amplitude alone and phibar[J + j] an exact zero.  sinc at 0, denormals, 2^-30, the doubles
    either side of 1/2, the fixture's phases and 1e9; the normal amplitude from 0 to 39 with its exact-zero edge."""
    k = S.load_kats()
    t = np.concatenate((SR.SINC_POINTS, k['z'], k['zb'][::4]))
    t = np.abs(t)                                                 # a half width
    assert 2 * t.max() < SR.PHASE_LIMIT and {0.0, 5e-324, 2.0 ** -30, SR.BELOW_HALF, 0.5, 1e9} <= set(t.tolist())
    re, im = diagonal_psi(0, -t, t)
    assert np.all(im == 0.0)
    r = S.abs_err(re, SR.sinc_truth(t)) / SR.sinc_bound(t)
    lo = t < 0.5
    print('\nsobol_range tables, sinc: %d points, worst / bound = %.4f in the series (at %r), %.4f beyond 1/2 (at %r)' % (
        len(t), r[lo].max(), t[lo][r[lo].argmax()], r[~lo].max(), t[~lo][r[~lo].argmax()]))
    assert re[t == 0][0] == 1.0 and r.max() <= 1
    t = SR.NORMAL_POINTS
    re, im = diagonal_psi(1, np.zeros(len(t)), t)
    assert np.all(im == 0.0)
    err = np.abs(re.astype(np.longdouble) - SR.normal_truth(t)).astype(np.float64)
    r = err / SR.normal_bound(t)
    print('sobol_range tables, normal amplitude: %d points, worst / bound = %.4f at t = %r' % (len(t), r.max(), t[r.argmax()]))
    assert r.max() <= 1
    # the exact-zero edge: the true value is 0.505 2^-1074 at 38.6037 and 0.4996 2^-1074 at 38.604, so round-to-nearest gives 2^-1074 and
    # 0, and an exp good to one unit of the denormal spacing may give either at both; from 39 on (1e-7 of the spacing) only 0 is left
    edge = re[(t >= 38.6037) & (t < 39.0)]
    print('    at t = 38.6037: %r (correctly rounded: 2^-1074); at 38.604: %r' % (re[t == 38.6037][0], re[t == 38.604][0]))
    assert np.all((edge == 0.0) | (edge == 2.0 ** -1074)) and np.all(re[t >= 39.0] == 0.0) and re[t == 0][0] == 1.0
    assert np.any((re > 0) & (re < 2.0 ** -1022))                                # denormal amplitudes are returned, not flushed


# ---- pairs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', SR.CASES, ids=ID)
def test_pairs(case):
    """all five outputs under the theta = 0 bound; at D = 1 V, Vmain[0] and Vtot[0] -- three code paths to one number -- agree within
    the sum of their bounds"""
    eng = case_engine(case)
    out = run(eng, case)
    r = SR.ratios(out, case)
    print('\nsobol_range pairs %-40s error / bound %s' % (case['name'], ' '.join('%s=%.2e' % kv for kv in sorted(r.items()))))
    assert sorted(r) == sorted(SR.ALL) and all(np.all(np.isfinite(out[k])) for k in SR.ALL)
    assert all(v <= 1.0 for v in r.values()), r
    if case['D'] == 1:
        bd = R.bounds(SR.reference(case), 1)
        for k in ('Vmain', 'Vtot'):
            assert np.all(np.abs(out['V'] - out[k][:, 0]) <= bd['V'] + bd[k][:, 0]), k


def test_pairs_in_an_f32_context():
    """promise 4 ties the compute modes together: the same bits from an fp32 context, at the far end too"""
    for case in (SR.CASES[10], SR.GROUP_CASES[-1]):
        a = run(case_engine(case), case); b = run(case_engine(case, 'f32'), case)
        for k in SR.ALL:
            assert np.array_equal(a[k], b[k]), (case['name'], k)


@pytest.mark.parametrize('case', SR.GROUP_CASES, ids=ID)
def test_group_size_changes_no_bit_at_these_ranges(case):
    """promise 5 at D = 17: one group of 16 and one of 1 by default, 17 groups of 1, groups of 5, 5, 5, 2"""
    eng = case_engine(case)
    try:
        eng.set_option('test_sobol_group', 0)
        a = run(eng, case)
        for G in (1, 5):
            eng.set_option('test_sobol_group', G)
            b = run(eng, case)
            for k in SR.ALL:
                assert np.array_equal(a[k], b[k]), (G, k)
    finally:
        eng.set_option('test_sobol_group', 0)


# ---- the domain ------------------------------------------------------------------------------------------------------------------
def _raw_call(eng, case, outs, p0=None, p1=None):
    p0 = case['p0'] if p0 is None else p0; p1 = case['p1'] if p1 is None else p1
    W = np.ascontiguousarray(case['W'])
    return eng.lib.scfgp_sobol(eng.ctx, np.ascontiguousarray(case['kind']).ctypes.data_as(C.POINTER(C.c_int32)), dptr(np.ascontiguousarray(p0)),
                               dptr(np.ascontiguousarray(p1)), dptr(W), W.shape[1], *[dptr(o) for o in outs])


def test_a_measure_beyond_the_domain_is_refused():
    """uniform on 2.5 2^30 +- 1/8 with max |Om| = 1 (R = 5.4e9): SCFGP_EARG with the text that names the input, the outputs untouched,
    and the next call gives the bits of a fresh context.  Every subset of outputs is refused alike -- phibar alone, whose own phases
    are inside the domain, included: the contract is the measure's, not the call's."""
    from scfgp_amd.engine import HipEngine
    c = SR.WRAP_CASE
    good = SR.CASES[0]
    assert good['geom'] == c['geom'] == 'd1'
    eng = HipEngine(c['D'], c['S'], c['M']); eng.set_params(c['params'])
    J = c['J']
    outs = [np.full(2, 7.0), np.full(2, 7.0), np.full((2, 1), 7.0), np.full((2, 1), 7.0), np.full(2 * J, 7.0)]
    assert _raw_call(eng, c, outs) == -1 and eng.last_error() == REFUSAL % 0
    assert all(np.all(o == 7.0) for o in outs)
    assert _raw_call(eng, c, [None] * 4 + [outs[4]]) == -1 and eng.last_error() == REFUSAL % 0 and np.all(outs[4] == 7.0)
    with pytest.raises(ValueError, match='leave the sin/cos domain'):
        run(eng, c)
    # p0 = -DBL_MAX / 2, p1 = DBL_MAX / 2: the centre and the half width are finite (api_host.h: sobol_measure), the phases are not
    big = np.finfo(np.float64).max / 2
    assert _raw_call(eng, c, outs, p0=np.array([-big]), p1=np.array([big])) == -1 and eng.last_error() == REFUSAL % 0
    assert all(np.all(o == 7.0) for o in outs)
    after = run(eng, good)
    eng.close()
    fresh = HipEngine(c['D'], c['S'], c['M']); fresh.set_params(c['params'])
    first = run(fresh, good)
    fresh.close()
    for k in SR.ALL:
        assert np.array_equal(after[k], first[k]), k
    assert all(v <= 1 for v in SR.ratios(after, good).values())


def test_the_refusal_names_the_first_input():
    """D = 3: input 1 out of the domain on its normal mean and input 2 on its half width -> input 1 is named; with input 1 back inside,
    input 2; with both inside the call goes through (the sentinel check of test_gpu_sobol.py, repeated for this refusal)"""
    c = next(x for x in SR.CASES if x['geom'] == 'd3')
    eng = case_engine(c)
    J = c['J']
    outs = [np.full(2, 7.0), np.full(2, 7.0), np.full((2, 3), 7.0), np.full((2, 3), 7.0), np.full(2 * J, 7.0)]
    om = np.abs(c['Om']).max(1)
    kind = np.array([0, 1, 0], np.int32)
    p0 = np.array([0.0, 1.2 * SR.PHASE_LIMIT / (2 * om[1]), -1e15]); p1 = np.array([1.0, 1.0, 1e15])
    bad = dict(c, kind=kind, p0=p0, p1=p1)
    assert _raw_call(eng, bad, outs) == -1 and eng.last_error() == REFUSAL % 1
    p0[1] = 0.9 * SR.PHASE_LIMIT / (2 * om[1])
    assert _raw_call(eng, bad, outs) == -1 and eng.last_error() == REFUSAL % 2
    assert all(np.all(o == 7.0) for o in outs)
    p0[2], p1[2] = 0.0, 1.0
    assert _raw_call(eng, bad, outs) == 0 and not any(np.any(o == 7.0) for o in outs)


@pytest.mark.parametrize('name', ['d1 uniform c=2^30 h=1/8', 'd1 uniform c=1.5 2^30 h=1/8'])
def test_a_measure_just_inside_the_domain_is_accepted(name):
    """max |Om| = 1: centre 2^30 gives R = 2.1e9, centre 1.5 2^30 gives 3.2e9; accepted and inside the theta = 0 bound"""
    case = next(c for c in SR.CASES if c['name'] == name)
    assert 2.1e9 < case['Rd'][0] < SR.PHASE_LIMIT
    r = SR.ratios(run(case_engine(case), case), case)
    print('\nsobol_range edge %-32s R = %.3g: error / bound %s' % (name, case['Rd'][0], ' '.join('%s=%.2e' % kv for kv in sorted(r.items()))))
    assert all(v <= 1 for v in r.values()), r
