"""
GPU tier of the phase-range tests: the compiled feature-map kernels (featuremap_reg_kernel<T, 3|4|5|8|9>, featuremap_kernel<T>,
project_kernel; csrc/fmap.hip) element by element against sin / cos of phases that are known exactly, out to |z| = 1e9.

  a  the hard arguments of tests/golden/sincos_kats.npz injected so that the phase of a row is exactly the fixture's z
  b  dyadic inputs whose multi-term contractions are exact in any order, through every dispatch of the feature map
  c  the fixture's block beyond |fn| = 2^20, where fn * pio2_1 alone no longer fits a double

The bounds are absolute (near a zero of sin or cos a relative error means nothing, and the Gram products consume absolute
error): twice the worst error of the CPU emulation against mpmath (tests/test_sincos_ref.py: E64, E32), the factor covering the
single roundings by which a build that contracts a * b + c differs from the emulation.  Nothing here is taken from a kernel.
Output (-s): per case the worst error over its bound.
"""
import numpy as np
import pytest

from tests import sincos_ref as R
from tests.test_sincos_ref import E32, E32_BEYOND, E64, FN_EDGE, law64

pytestmark = pytest.mark.gpu

TDT = {'f64': np.float64, 'f32': np.float32}
_KATS = {}


def kats():
    if not _KATS:
        k = R.load_kats()
        # the reference of a whole block, computed once and shared read-only
        for key in ('z', 'zb', 'sin', 'cos', 'sinb', 'cosb'):
            k[key].setflags(write=False)
        _KATS.update(k)
    return _KATS


def run_phi(D, S, M, dtype, params, X, check=None):
    """set_params, set_data, pass1, debug_read('Phi'): the whole padded array as float64, with the geometry"""
    from scfgp_amd.engine import HipEngine
    eng = HipEngine(D, S, M, dtype=dtype)
    try:
        eng.set_params(params)
        eng.set_data(np.ascontiguousarray(X), np.zeros((X.shape[0], 1)))
        d = eng.dims()
        if check is not None:
            check(eng, d)
        eng.pass1()
        Phi = eng.debug_read('Phi', (d['Np'], d['Kp']), TDT[dtype]).astype(np.float64)
    finally:
        eng.close()
    return Phi, d


def split(Phi, N, S, M):
    """(cos, sin) / s of the live block, after checking that the padding rows and columns are exact zeros"""
    J = S + M
    s = np.sqrt(2.0 / M)
    assert s in (0.5, 0.25, 0.125)                                     # a power of two: Phi / s is the raw output of fast_sincos
    assert np.all(Phi[N:] == 0) and np.all(Phi[:, 2 * J:] == 0)
    assert np.all(np.isfinite(Phi))
    return Phi[:N, :J] / s, Phi[:N, J:2 * J] / s


def worst(cs, sn, tcos, tsin):
    """largest |got - truth| over both halves, in np.longdouble; truth is per row (N,) or per entry (N, J)"""
    tc = tcos[:, None] if tcos.ndim == 1 else tcos
    ts = tsin[:, None] if tsin.ndim == 1 else tsin
    return np.maximum(R.abs_err(cs, tc), R.abs_err(sn, ts))


def injected(kind, dtype, z):
    """Phi / s for phases exactly z in every column, for X and for -X; the unpacked operands checked bit for bit first"""
    D, S, M, params, X = R.inject(kind, z)
    form, kern = R.fmap_dispatch(D, S, M)

    def checker(Xc):
        def check(eng, d):
            Dp, Jp = d['Dp'], d['Jp']
            Fall = eng.debug_read('Fall', (Dp, Jp))
            if form == 'rank':
                Sp = -(-(S + 1) // 16) * 16; Spp = -(-Sp // 64) * 64
                eF, eL, eR = R.inject_expected(D, S, M, Dp, Jp, Sp, Spp)
                assert np.array_equal(eng.debug_read('Lall', (Dp, Spp)), eL)
                assert np.array_equal(eng.debug_read('Rall', (Sp, Jp)), eR)
            else:
                eF = R.inject_expected(D, S, M, Dp, Jp)
            assert np.array_equal(Fall, eF)
            Xt = eng.debug_read('Xt', (d['Np'], Dp))[:len(z)]
            assert np.array_equal(Xt[:, 0], Xc[:, 0]) and np.all(Xt[:, D] == 1) and np.all(Xt[:, 1:D] == 0) and np.all(Xt[:, D + 1:] == 0)
        return check

    Phi, d = run_phi(D, S, M, dtype, params, X, checker(X))
    assert d['Np'] > len(z) and len(z) % 128 != 0
    cs, sn = split(Phi, len(z), S, M)
    Phim, _ = run_phi(D, S, M, dtype, params, -X, checker(-X))
    csm, snm = split(Phim, len(z), S, M)
    return (D, S, M, form, kern), cs, sn, csm, snm


def check_columns_and_symmetry(z, cs, sn, csm, snm):
    # every column has the same phase: independent of lane, column tile and the column split of the launch
    assert np.array_equal(cs, np.repeat(cs[:, :1], cs.shape[1], 1)) and np.array_equal(sn, np.repeat(sn[:, :1], sn.shape[1], 1))
    assert np.array_equal(np.signbit(cs), np.repeat(np.signbit(cs[:, :1]), cs.shape[1], 1))
    assert np.array_equal(np.signbit(sn), np.repeat(np.signbit(sn[:, :1]), sn.shape[1], 1))
    # X -> -X: the cos half bit-identical, the sin half bit-negated.  The one exception to the bits of the sin half is a sine
    # that is zero for both: -0 reaches the routine as +0 (the accumulator starts from +0) and sin is +0 for both signs.  Only a
    # phase that is zero, or the denormal the matrix pipe may flush to zero, can have such a sine.
    assert np.array_equal(csm.view(np.int64), cs.view(np.int64))
    zero = (sn == 0) & (snm == 0)
    assert np.array_equal((-snm).view(np.int64)[~zero], sn.view(np.int64)[~zero])
    rows = np.flatnonzero(zero.any(1))
    assert np.all(np.abs(z[rows]) <= 5e-324), z[rows]
    return z[rows]


INJECTED = [(k, t) for k in ('reg_odd', 'reg_even', 'lds', 'rank') for t in ('f64', 'f32')]


@pytest.mark.parametrize('kind,dtype', INJECTED)
def test_injected_hard_cases(kind, dtype):
    """In-domain block of the fixture (|fn| < 2^20: multiples of pi/2 and their neighbours, quadrant flips, ties of rint, +-0, the
    smallest denormal, all quadrants up to the last exact product), every entry of Phi / s within 2 E of mpmath's value.
    First measurements of these kernels at |z| > 1e2 (MI355X), worst |error| / (2 E): 0.49 in fp64 and 0.50 in fp32 for all
    four kinds alike; the fp32 entries are those of the emulation bit for bit."""
    k = kats()
    z = k['z']
    (D, S, M, form, kern), cs, sn, csm, snm = injected(kind, dtype, z)
    assert (form, kern) == {'reg_odd': ('direct', 'reg3'), 'reg_even': ('direct', 'reg3'), 'lds': ('direct', 'lds'),
                            'rank': ('rank', 'reg3')}[kind]
    assert (S + M) % 2 == (1 if kind in ('reg_odd', 'rank') else 0)
    bound = 2 * (E64 if dtype == 'f64' else E32)
    e = worst(cs, sn, k['cos'], k['sin'])
    i = np.unravel_index(e.argmax(), e.shape)
    msg = 'phase_range a %-8s %s (%s, %s): worst / bound = %.4f at z = %r' % (kind, dtype, form, kern, e.max() / bound, z[i[0]])
    if dtype == 'f32':
        es, ec = R.emul_sincos32(z)
        msg += '; %d of %d entries differ from the emulation' % (int((sn[:, 0] != es).sum() + (cs[:, 0] != ec).sum()), 2 * len(z))
    print('\n' + msg)
    zr = check_columns_and_symmetry(z, cs, sn, csm, snm)
    print('    rows with a zero sine for both signs: z = %s' % zr.tolist())
    assert e.max() <= bound, msg


# (D, S, M) -> form, live rows -> kernel
DYADIC = [
    ((8, 20, 8), 'direct', 'reg3'),         # 9 live
    ((32, 13, 8), 'rank', 'reg4'),          # 14 live, odd J
    ((16, 17, 32), 'direct', 'reg5'),       # 17 live
    ((64, 30, 32), 'rank', 'reg8'),         # 31 live
    ((32, 47, 32), 'direct', 'reg9'),       # 33 live
    ((64, 32, 128), 'rank', 'reg9'),        # 33 live, the headline depth
    ((64, 64, 8), 'direct', 'lds'),         # 65 live
    ((128, 60, 32), 'rank', 'lds'),         # 61 live
]
_DYADIC = {}


def dyadic(shape, target):
    """inputs and the longdouble truth of one case, computed once for both dtypes and left unchanged"""
    key = (shape, target)
    if key not in _DYADIC:
        D, S, M = shape
        X, params, Z, e = R.dyadic_case(D, S, M, target, 0x5CF70000 + 977 * D + 31 * S + M, N=293)
        ts, tc = R.truth(Z)
        for a in (X, params, Z, ts, tc):
            a.setflags(write=False)
        _DYADIC[key] = (X, params, Z, ts, tc, e)
    return _DYADIC[key]


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('target', [1e2, 1e4, 1e6])
@pytest.mark.parametrize('shape,form,kern', DYADIC)
def test_dyadic_exact_phases(shape, form, kern, target, dtype):
    """Every dispatch of the feature map at max |z| of 1e2, 1e4 and 1e6: X, l_F, r_F and the offsets are dyadic, so the phase
    matrix is the same double in any accumulation order and is known exactly from int64 arithmetic; every entry of Phi / s within
    2 E of np.longdouble's sin / cos of it.  N = 293: three row blocks, ragged against the 32-row waves."""
    D, S, M = shape
    assert R.fmap_dispatch(D, S, M) == (form, kern)                    # the rule of FmapKernels::featuremap, restated
    X, params, Z, ts, tc, e2 = dyadic(shape, target)
    N = X.shape[0]
    assert N == 293 and N % 128 != 0 and target / 4 <= np.abs(Z).max() <= target
    assert np.abs(np.rint(Z * R.TWO_OVER_PI)).max() < R.FN_EXACT
    Phi, d = run_phi(D, S, M, dtype, params, X)
    assert d['Np'] % 128 == 0 and d['Np'] > N + 32                     # padding rows inside the last live block and a dead block
    cs, sn = split(Phi, N, S, M)
    bound = 2 * (E64 if dtype == 'f64' else E32)
    e = worst(cs, sn, tc, ts)
    i = np.unravel_index(e.argmax(), e.shape)
    msg = 'phase_range b %-14s %-6s %-4s %s max|z| %.3g (l_F * 2^%d): worst / bound = %.4f at z = %r' % (
        shape, form, kern, dtype, np.abs(Z).max(), e2, e.max() / bound, Z[i])
    print('\n' + msg)
    assert e.max() <= bound, msg


@pytest.mark.parametrize('kind', ['reg_odd', 'reg_even'])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_beyond_exact_products(kind, dtype):
    """The fixture's block at |z| of 1e7, 1e8 and 1e9 (2^20 <= |fn| < 2^31), injected through the register kernel.  fp32 mode
    meets 2 E32 re-measured over this block; fp64 mode stays finite, within the unit circle, and under the growth law of
    tests/test_sincos_ref.py (flat up to |fn| = 2^31: the fused first step of the reduction is exact there too)."""
    k = kats()
    z = k['zb']
    fn = np.rint(z * R.TWO_OVER_PI)
    assert np.all(np.abs(fn) < FN_EDGE) and np.all(np.abs(fn) >= R.FN_EXACT)          # (int)fn stays in range
    (D, S, M, form, kern), cs, sn, csm, snm = injected(kind, dtype, z)
    assert np.all(np.isfinite(cs)) and np.all(np.isfinite(sn))
    e = worst(cs, sn, k['cosb'], k['sinb'])
    bound = 2 * law64(fn)[:, None] if dtype == 'f64' else np.full(e.shape, 2 * E32_BEYOND)
    r = e / bound
    i = np.unravel_index(r.argmax(), r.shape)
    msg = 'phase_range c %-8s %s: worst / bound = %.4f at z = %r' % (kind, dtype, r.max(), z[i[0]])
    print('\n' + msg)
    check_columns_and_symmetry(z, cs, sn, csm, snm)
    if dtype == 'f64':
        tol = 2.0 ** -50
        assert np.abs(cs).max() <= 1 + tol and np.abs(sn).max() <= 1 + tol              # |Phi| <= s (1 + 2^-50)
        ld = np.longdouble
        one = np.abs(cs.astype(ld) ** 2 + sn.astype(ld) ** 2 - 1).astype(np.float64)
        assert one.max() <= tol, one.max()
    assert r.max() <= 1, msg
