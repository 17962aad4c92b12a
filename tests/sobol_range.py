"""
Range tests of the sin / cos sites of scfgp_sobol (scfgp_amd/csrc/sobol.hip: psi, sinc, the normal amplitude, sobol_tables_kernel,
sobol_pairs_kernel): the geometries, the measures, the emulation of the device's psi, the bounds and the mutants, shared by the CPU tier
(tests/test_sobol_range_ref.py) and the GPU tier (tests/test_gpu_sobol_range.py).  numpy only.

Why exact phases.  The device bound of DESIGN 4.21 (tests/sobol_ref.py: bounds) pays for the rounding of the phase products with a term
16 (D + 2) (1 + Theta) eps (sum |a|)^2, Theta = 2 max |Om| |x|.  At Theta of 1e7 .. 1e10 that term is so wide that a wrong QUADRANT
passes under it (a centre of 2^24 with half width 2^10 passes at ratio 0.01 where the ratio against exact phases is 1e7).  So every
geometry and measure here is dyadic with few bits: 1/2 p0 + 1/2 p1, 1/2 p1 - 1/2 p0, Om m0, Om m1, Om_j +- Om_k and (Om_j +- Om_k) m are
all exact doubles -- assert_exact() checks it in Fraction arithmetic for every case when this module is imported -- and the bounds are
taken with Theta = 0.

Bounds (eps = 2^-53, L = test_sincos_ref.law64 = 0.77 eps; all derived, none taken from a kernel):
    a phase factor (cos, sin)                    2 L absolute            the contraction allowance of tests/test_gpu_phase_range.py
    sinc, |t| < 1/2                              2 eps absolute          the last fma rounds a value <= 1 (eps); the inner Horner
                                                                         chain's error enters scaled by u = t^2 <= 1/4
    sinc, |t| >= 1/2                             (2 L + eps) / |t|       the sine's 2 L and the rounding of the quotient, |sin| <= 1
    normal amplitude exp(-t^2 / 2)               (2 + t^2) eps relative + 2^-1074 absolute
                                                                         t * t rounded once (relative eps of the exponent t^2 / 2, so
                                                                         t^2 / 2 eps of the value) and -0.5 * that exact; the 2 covers
                                                                         an exp good to one ulp (2 eps in units of 2^-53), and a
                                                                         denormal result rounds to the spacing 2^-1074
    a product of two factors of modulus <= 1     2 eps more
    variances, f0, phibar at pair level          sobol_ref.bounds with theta = 0

The emulation evaluates psi as sobol.hip writes it, one rounding per operation and the series in true fmas, with
sincos_ref.emul_sincos64 for fast_sincos.  Beyond the routine's domain (|fn| >= 2^31) the emulation's (int)fn saturates, as the
conversion of the hardware does; the unmutated psi here repairs the quadrant there from the exact fn (the reduction itself is still
exact), and the mutant 'quadrant_wrap' leaves it as the routine computes it.  That mutant is the library before scfgp_sobol refused
such measures.
"""
import contextlib
from fractions import Fraction

import numpy as np

from tests import sincos_ref as SR
from tests import sobol_ref as R
from tests.test_sincos_ref import law64

EPS = 2.0 ** -53
L = float(law64(0.0))
PHASE_LIMIT = 3.37e9                                             # api_host.h: SOBOL_PHASE_LIMIT
ALL = ('f0', 'V', 'Vmain', 'Vtot', 'phibar')

# Mutants of the emulated psi, each one way the device could be subtly wrong at the far end of its range
#   quadrant_wrap  the routine's own saturating (int)fn, no repair: what a call beyond the domain computes
#   series_to_2    the sinc series used up to |t| < 2 instead of 1/2 (its truncation error is 2^-64 only below 1/2)
#   left_edge      the uniform's phase taken at p0 instead of the centre
#   no_half_exp    the normal amplitude as exp(-t^2)
MUTATIONS = ('quadrant_wrap', 'series_to_2', 'left_edge', 'no_half_exp')


# ---- the device's psi, emulated --------------------------------------------------------------------------------------------------
def _per_unique(f, x):
    """f over the distinct values of x only (the pair tensors repeat a few hundred phases many times)"""
    x = np.asarray(x, np.float64)
    u, inv = np.unique(x.ravel(), return_inverse=True)
    outs = f(u)
    if isinstance(outs, tuple):
        return tuple(o[inv].reshape(x.shape) for o in outs)
    return outs[inv].reshape(x.shape)


def sincos(z, wrap=False):
    """(sin, cos) as fast_sincos(double) gives them inside its domain; beyond it with the quadrant of the exact fn unless wrap"""
    def f(z):
        sn, cs = SR.emul_sincos64(z)
        fn = np.rint(z * SR.TWO_OVER_PI)
        big = np.abs(fn) >= 2.0 ** 31
        if wrap or not np.any(big):
            return sn, cs
        q_sat = np.clip(fn[big], -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64) & 3
        q_true = np.array([int(v) & 3 for v in fn[big]], np.int64)
        k = (q_true - q_sat) & 3                                 # quarter turns that the saturated conversion lost
        s, c = sn[big], cs[big]
        sn, cs = sn.copy(), cs.copy()
        sn[big] = np.choose(k, [s, c, -s, -c])
        cs[big] = np.choose(k, [c, -s, -c, s])
        return sn, cs
    return _per_unique(f, z)


SERIES = (-1.0 / 1307674368000.0, 1.0 / 6227020800.0, -1.0 / 39916800, 1.0 / 362880, -1.0 / 5040, 1.0 / 120, -1.0 / 6, 1.0)


def sinc(t, mutate=None):
    """sinc() of sobol.hip: the series in fmas below 1/2, sin t / t from fast_sincos elsewhere"""
    edge = 2.0 if mutate == 'series_to_2' else 0.5

    def f(t):
        out = np.empty_like(t)
        low = np.abs(t) < edge
        if np.any(low):
            u = t[low] * t[low]
            r = np.full(u.shape, SERIES[0])
            for c in SERIES[1:]:
                r = SR.fma64(u, r, c)
            out[low] = r
        if np.any(~low):
            sn, _ = sincos(t[~low], wrap=mutate == 'quadrant_wrap')
            out[~low] = sn / t[~low]
        return out
    return _per_unique(f, t)


def normal_amp(t, mutate=None):
    t = np.asarray(t, np.float64)
    with np.errstate(under='ignore'):
        return np.exp(-(t * t)) if mutate == 'no_half_exp' else np.exp(-0.5 * t * t)


def measure_form(kind, p0, p1):
    """api_host.h: sobol_measure -- (m0, m1) = (centre, half width) or (mean, sd)"""
    kind = np.asarray(kind); p0 = np.asarray(p0, np.float64); p1 = np.asarray(p1, np.float64)
    return np.where(kind == 1, p0, 0.5 * p0 + 0.5 * p1), np.where(kind == 1, p1, 0.5 * p1 - 0.5 * p0)


def dev_psi(kind, p0, p1, om, mutate=None):
    """psi() of sobol.hip for every input d (axis 0 of om), complex; the signature of sobol_ref.psi"""
    sh = (-1,) + (1,) * (om.ndim - 1)
    kind = np.asarray(kind).reshape(sh)
    m0, m1 = measure_form(kind, np.asarray(p0, np.float64).reshape(sh), np.asarray(p1, np.float64).reshape(sh))
    if mutate == 'left_edge':
        m0 = np.where(kind == 1, m0, np.asarray(p0, np.float64).reshape(sh))
    sn, cs = sincos(om * m0, wrap=mutate == 'quadrant_wrap')
    t = om * m1
    amp = np.where(kind == 1, normal_amp(t, mutate), sinc(t, mutate))
    return cs * amp + 1j * (sn * amp)


@contextlib.contextmanager
def device_psi():
    """inside: sobol_ref.sobol evaluates every characteristic function as the device does (its `mutate` reaches dev_psi)"""
    keep = R.psi
    R.psi = dev_psi
    try:
        yield
    finally:
        R.psi = keep


def _fma_c(a, b, c):
    return SR.fma64(a, b, c)


def cmul(a, b):
    """cmul of sobol.hip on (re, im) pairs of arrays: {fma(a.re, b.re, -(a.im b.im)), fma(a.re, b.im, a.im b.re)}"""
    return _fma_c(a[0], b[0], -(a[1] * b[1])), _fma_c(a[0], b[1], a[1] * b[0])


def emul_tables_E(Om, b, kind, p0, p1):
    """E of sobol_tables_kernel in its own order: e^{ib} (psi_0 (psi_1 (... psi_{D-1}))), products through cmul.  (re, im)"""
    D, J = Om.shape
    P = dev_psi(kind, p0, p1, Om)
    suf = (np.ones(J), np.zeros(J))
    for d in range(D - 1, -1, -1):
        suf = cmul((P[d].real.copy(), P[d].imag.copy()), suf)
    sn, cs = sincos(b)
    return cmul((cs, sn), suf)


# ---- geometries ------------------------------------------------------------------------------------------------------------------
def _params(l_F, r_F):
    """a = b = c = 0 and the offsets l_P, P that cancel the column means: row D of Fall is l_P - sum_d l_F / D = 0 exactly when the
    column sums are exact, which the few-bit dyadic entries make them"""
    D = l_F.shape[0]
    F = l_F @ r_F.T
    return SR.pack_params(l_F, r_F, l_F.sum(0) / D, F.sum(0) / D)


def diagonal():
    """D = S = 64, M = 8, l_F = I, r_F = 0, l_P = 1 / D: Om[d][j] = delta_dj for j < 64, the last 8 columns zero, b = 0, s = 1/2.
    psi_d(0) = {1, 0} and cmul with {1, 0} are exact, so E_j = psi_j(1) and phibar / s holds 64 raw psi values per call."""
    D = S = 64; M = 8
    l_F = np.eye(D); r_F = np.zeros((M, S))
    params = _params(l_F, r_F)
    assert np.all(params[3 + D * S + M * S:3 + D * S + M * S + S] == 1.0 / D) and np.all(params[-M:] == 0.0)
    return D, S, M, params


def _pair_geometry(D):
    """(D, S, M, params) with J <= 16 (two blocks of the pair kernel's tile edge 8), dyadic Om of at most 6 significant bits whose
    columns hold a zero column, a repeated column, a pair Om_j = -Om_k, and magnitudes over about ten binades up to 1.5"""
    M = 8
    if D == 1:                                                   # Om = (1, 1/2, 1/4, 3/4, -1, 0, 1, 1/8, 5/8)
        l_F = np.array([[1.0]])
        r_F = np.array([[0.5], [0.25], [0.75], [-1.0], [0.0], [1.0], [0.125], [0.625]])
    else:
        S = 3 if D == 3 else 4
        rng = np.random.default_rng(0x50B0 + D)
        mant = rng.choice([-3.0, -1.0, 1.0, 3.0, 5.0, -5.0], (D, S))
        expo = rng.integers(-10, -2, (D, S))
        expo[0, 0] = -2; mant[0, 0] = 3.0                       # 3/4: with the factor 2 below the largest |Om| is 1.5
        expo[-1, -1] = -10
        l_F = np.ldexp(mant, expo)
        r_F = np.zeros((M, S))
        r_F[0, 0] = 2.0                                          # 2 Om_0
        r_F[1, 1] = 1.0                                          # a repeat of column 1
        r_F[2, 0] = -1.0                                         # -Om_0
        #   row 3: the zero column
        r_F[4, 2] = 1.0; r_F[4, 1] = 0.5                         # Om_2 + Om_1 / 2
        r_F[5, S - 1] = 2.0 ** -3
        r_F[6, 0] = 1.0; r_F[6, S - 1] = -1.0
        r_F[7, 1] = -0.25
    return D, l_F.shape[1], M, _params(l_F, r_F)


def pow2_geometry():
    """D = 1, Om = 1/2 (1, 1, 0, -1, 1, 0, -1, 1, 0): every Om_j +- Om_k is 0, +-1/2 or +-1, so that t = (Om_j +- Om_k) m1 is exact for
    ANY double m1 -- the case that puts t on 1/2, on the double below it, and on a denormal"""
    l_F = np.array([[0.5]])
    r_F = np.array([[1.0], [0.0], [-1.0], [1.0], [0.0], [-1.0], [1.0], [0.0]])
    return 1, 1, 8, _params(l_F, r_F)


GEOMETRIES = {'d1': _pair_geometry(1), 'd3': _pair_geometry(3), 'd17': _pair_geometry(17), 'pow2': pow2_geometry()}


def check_geometry(D, S, M, params):
    """Om, s of a geometry after the asserts that make its phases exact: Om dyadic, b exactly 0, s a power of two"""
    Om, b, s = R.phases(params, D, S, M)
    assert M in (8, 32, 128) and np.all(params[:3] == 0) and s in (0.5, 0.25, 0.125)
    assert np.all(b == 0.0), 'the offsets do not cancel the column means'
    assert np.all(Om * 2.0 ** 16 == np.rint(Om * 2.0 ** 16)) and np.abs(Om).max() <= 1.5
    return Om, s


def expected_fall(D, S, M, params, Dp, Jp):
    """what debug_read('Fall', (Dp, Jp)) must hold for a geometry of this file, bit for bit: Om in rows d < D, zeros from row D on"""
    Om, _ = check_geometry(D, S, M, params)
    F = np.zeros((Dp, Jp)); F[:D, :S + M] = Om
    return F


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def _exact(x):
    return Fraction(float(x))


def assert_exact(Om, kind, p0, p1):
    """every sum and product that forms a phase is an exact double (Fraction arithmetic)"""
    D, J = Om.shape
    m0, m1 = measure_form(kind, p0, p1)
    for d in range(D):
        if kind[d] == 0:
            assert _exact(m0[d]) == (_exact(p0[d]) + _exact(p1[d])) / 2 and _exact(m1[d]) == (_exact(p1[d]) - _exact(p0[d])) / 2, (d, p0[d], p1[d])
        oms = set(Om[d].tolist())
        for sign in (1.0, -1.0):
            sums = Om[d][:, None] + sign * Om[d][None, :]
            for a, b_, c in zip(np.repeat(Om[d], J).tolist(), np.tile(sign * Om[d], J).tolist(), sums.ravel().tolist()):
                assert Fraction(a) + Fraction(b_) == Fraction(c)
            oms |= set(sums.ravel().tolist())
        for om in oms:
            for m in (m0[d], m1[d]):
                assert Fraction(om) * _exact(m) == _exact(om * m), (d, om, m)


def _case(name, geom, kind, p0, p1, in_domain=True):
    D, S, M, params = GEOMETRIES[geom]
    Om, s = check_geometry(D, S, M, params)
    kind = np.broadcast_to(np.asarray(kind, np.int32), (D,)).copy()
    p0 = np.broadcast_to(np.asarray(p0, np.float64), (D,)).copy(); p1 = np.broadcast_to(np.asarray(p1, np.float64), (D,)).copy()
    assert_exact(Om, kind, p0, p1)
    m0, m1 = measure_form(kind, p0, p1)
    Rd = 2.0 * np.abs(Om).max(1) * (np.abs(m0) + np.where(kind == 0, m1, 0.0))
    assert bool(np.all(Rd < PHASE_LIMIT)) == in_domain, (name, Rd)
    J = S + M
    W = np.random.default_rng(0x50B1 + J).standard_normal((2 * J, 2))
    for a in (params, kind, p0, p1, W):
        a.setflags(write=False)
    return dict(name=name, geom=geom, D=D, S=S, M=M, J=J, params=params, Om=Om, s=s, kind=kind, p0=p0, p1=p1, W=W, Rd=Rd)


def _uniform(c, h):
    return 0, c - h, c + h


def representable(c, h):
    """c - h and c + h are doubles: the one pair of the issue's grid that is not is (2^30, 2^-30), which needs 61 bits"""
    return _exact(c - h) == _exact(c) - _exact(h) and _exact(c + h) == _exact(c) + _exact(h)


CENTRES = (0.5, 2.0 ** 20, 2.0 ** 30)
HALF_WIDTHS = (0.0, 2.0 ** -30, 0.5, 2.0 ** 10)
NORMALS = ((0.5, 2.0 ** -8), (2.0 ** 10, 2.0 ** -4), (2.0 ** 20, 1.0), (2.0 ** 24, 2.0 ** 3), (2.0 ** 24, 2.0 ** -8), (-2.0 ** 22, 2.0 ** -1))
BELOW_HALF = float(np.nextafter(0.5, 0.0))


def _mixed(D):
    """per input: the uniform and the normal measures above in turn"""
    uni = [(c, h) for c in CENTRES for h in HALF_WIDTHS if representable(c, h)]
    kind = np.zeros(D, np.int32); p0 = np.zeros(D); p1 = np.zeros(D)
    for d in range(D):
        if d % 3 == 2:
            kind[d] = 1; p0[d], p1[d] = NORMALS[(d // 3) % len(NORMALS)]
        else:
            kind[d], p0[d], p1[d] = _uniform(*uni[(5 * d + 3) % len(uni)])
    return kind, p0, p1


def _build_cases():
    cases = []
    for g in ('d1', 'd3', 'd17'):
        for c in CENTRES:
            for h in HALF_WIDTHS:
                if representable(c, h):
                    cases.append(_case('%s uniform c=%g h=%g' % (g, c, h), g, *_uniform(c, h)))
        for mean, sd in NORMALS:
            cases.append(_case('%s normal m=%g sd=%g' % (g, mean, sd), g, 1, mean, sd))
    for g in ('d3', 'd17'):
        cases.append(_case('%s mixed' % g, g, *_mixed(GEOMETRIES[g][0])))
    # t = (Om_j +- Om_k) m1 on 1/2, on the double below it, on a denormal; the normal amplitude exactly zero and denormal
    cases.append(_case('pow2 uniform h=1/2', 'pow2', *_uniform(0.5, 0.5)))
    cases.append(_case('pow2 uniform h=pred(1/2)', 'pow2', *_uniform(0.0, BELOW_HALF)))
    cases.append(_case('pow2 uniform h=2^-1073', 'pow2', *_uniform(0.0, 2.0 ** -1073)))
    cases.append(_case('pow2 normal sd=38.604', 'pow2', 1, 0.5, 38.604))
    cases.append(_case('pow2 normal sd=38.6037', 'pow2', 1, 0.5, 38.6037))
    # the edge of the domain, D = 1 with max |Om| = 1: R = 2.1e9 and 3.2e9 accepted ...
    cases.append(_case('d1 uniform c=2^30 h=1/8', 'd1', *_uniform(2.0 ** 30, 0.125)))
    cases.append(_case('d1 uniform c=1.5 2^30 h=1/8', 'd1', *_uniform(1.5 * 2.0 ** 30, 0.125)))
    return cases


CASES = _build_cases()
# ... and R = 5.4e9 not: every single phase is inside the domain (<= 2.7e9), the pair phases are not.  The library refuses it; the
# emulation with the routine's own quadrant ('quadrant_wrap') shows what it computed before
WRAP_CASE = _case('d1 uniform c=2.5 2^30 h=1/8', 'd1', *_uniform(2.5 * 2.0 ** 30, 0.125), in_domain=False)
GROUP_CASES = [c for c in CASES if c['geom'] == 'd17']


def reference(case):
    """sobol_ref.sobol of a case with theta = 0 (legitimate: the phases are exact), computed once and left unchanged"""
    if 'ref' not in case:
        ref = R.sobol(case['params'], case['D'], case['S'], case['M'], case['kind'], case['p0'], case['p1'], case['W'])
        ref['theta'] = 0.0
        case['ref'] = ref
    return case['ref']


def emulated(case, mutate=None):
    with device_psi():
        return R.sobol(case['params'], case['D'], case['S'], case['M'], case['kind'], case['p0'], case['p1'], case['W'], mutate=mutate)


def ratios(dev, case):
    """{output: worst |dev - ref| / bound at theta = 0} over the outputs dev holds"""
    return R.worst_ratio(dev, reference(case), case['D'])


def pair_phases(case):
    """(z, t, kinds): the phases (Om_j +- Om_k) m0 and the amplitude arguments (Om_j +- Om_k) m1 of every pair, (2, D, J, J)"""
    Om = case['Om']
    m0, m1 = measure_form(case['kind'], case['p0'], case['p1'])
    om = np.stack([Om[:, :, None] + sg * Om[:, None, :] for sg in (1.0, -1.0)])
    return om * m0[None, :, None, None], om * m1[None, :, None, None], np.broadcast_to(case['kind'][None, :, None, None], om.shape)


# ---- single values: truth and bounds ---------------------------------------------------------------------------------------------
def sinc_truth(t):
    tl = np.asarray(t, np.float64).astype(np.longdouble)
    assert np.finfo(np.longdouble).nmant >= 63
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(tl == 0, np.longdouble(1), np.sin(tl) / np.where(tl == 0, np.longdouble(1), tl))


def sinc_bound(t):
    t = np.abs(np.asarray(t, np.float64))
    with np.errstate(divide='ignore'):
        return np.where(t < 0.5, 2 * EPS, (2 * L + EPS) / np.where(t == 0, 1.0, t))


def normal_truth(t):
    tl = np.asarray(t, np.float64).astype(np.longdouble)
    with np.errstate(under='ignore'):
        return np.exp(-(tl * tl) / 2)


def normal_bound(t):
    t = np.asarray(t, np.float64)
    return (2.0 + t * t) * EPS * normal_truth(t).astype(np.float64) + 2.0 ** -1074


SINC_POINTS = np.array([0.0, 5e-324, 2.0 ** -1050, 2.0 ** -1022, 2.0 ** -30, 2.0 ** -8, 0.25, BELOW_HALF, 0.5, float(np.nextafter(0.5, 1.0)),
                        1.0, 1.5, float(np.nextafter(2.0, 0.0)), 2.0, np.pi, 100.0, 1e9])
NORMAL_POINTS = np.concatenate((np.arange(0, 39 * 8 + 1) / 8.0, [2.0 ** -30, 5e-324, 38.5, 38.6037, 38.604, 38.7, 39.0]))
