"""
CPU tier of the phase-range tests (tests/sincos_ref.py): the numpy restatement of fast_sincos (csrc/sincos.h) against mpmath's
values in tests/golden/sincos_kats.npz.  It fixes the error bounds E64 / E32 the GPU tier (tests/test_gpu_phase_range.py) holds the
kernels to, locates the edge of the routine's domain, and shows that each bound fails the mutations it exists for.
Output (-s): E64, E32, the domain edge, and per mutation its worst error over the bound.
"""
import numpy as np
import pytest

from tests import sincos_ref as R

U64, U32 = 2.0 ** -53, 2.0 ** -24

# Worst absolute error of the emulation over the fixture, from mpmath -- never from a kernel.  The GPU tier allows twice these:
# the factor covers the single roundings by which a build that contracts a * b + c may differ from the emulation.
E64 = 0.77 * U64          # in-domain block (|fn| < 2^20), measured 0.7651 * 2^-53 (a tie point, z = 132.73...)
E32 = 1.21 * U32          # in-domain block, measured 1.2070 * 2^-24 (z = 1244775.19...)
E64_BEYOND = 0.64 * U64   # "beyond" block (2^20 <= |fn| < 2^31, |z| 5e6 .. 1e9), measured 0.6387 * 2^-53
E32_BEYOND = 1.33 * U32   # "beyond" block, measured 1.3212 * 2^-24
# The edge of the domain.  fma(-fn, pio2_1, z) is a true fused operation, and z - fn * pio2_1 is a multiple of 2^-32 below 2 in
# magnitude, so it is exact at every |fn| < 2^31, not only where the product alone fits a double (|fn| < 2^20): the error does
# not grow through the "beyond" block.  What ends the domain is (int)fn: from |fn| = 2^31 on the conversion no longer holds fn
# and the quadrant is wrong.  Growth law of the fp64 overload: flat, law64(fn) = max(E64, E64_BEYOND) = E64 for |fn| < FN_EDGE.
FN_EDGE = 2.0 ** 31       # |z| < 2^31 pi/2 = 3.37e9


def law64(fn):
    assert np.all(np.abs(fn) < FN_EDGE)
    return np.full(np.shape(fn), max(E64, E64_BEYOND))


@pytest.fixture(scope='module')
def kats():
    return R.load_kats()


def _worst(f, z, sn, cs, mut=None):
    s, c = f(z, mut) if mut else f(z)
    return np.maximum(R.abs_err(s, sn), R.abs_err(c, cs))


def test_fixture_layout(kats):
    z, zb = kats['z'], kats['zb']
    fn = np.rint(z * R.TWO_OVER_PI)
    assert len(z) % 128 != 0 and len(zb) % 128 != 0
    assert np.abs(fn).max() == 2 ** 20 - 1 and np.all(np.abs(np.rint(zb * R.TWO_OVER_PI)) < FN_EDGE)
    assert np.abs(np.rint(zb * R.TWO_OVER_PI)).min() >= R.FN_EXACT
    present = {kats['groups'][g] for g in np.unique(kats['group'])}
    assert present == {'npio2', 'flip', 'tie', 'special', 'quadrant', 'filler'}
    tie = z[kats['group'] == kats['groups'].index('tie')]
    t = tie * R.TWO_OVER_PI
    assert np.all(t - np.floor(t) == 0.5) and len(tie) > 100
    assert (np.floor(t) % 2 == 0).sum() > 20 and (np.floor(t) % 2 == 1).sum() > 20 and (t < 0).sum() > 20
    q = fn.astype(np.int64) & 3
    hi = np.abs(fn) >= 2 ** 20 - 4
    for sign in (1, -1):                                               # all four quadrants next to the edge of exact products
        assert set(q[hi & (np.sign(fn) == sign)].tolist()) == {0, 1, 2, 3}
    for v in (0.0, 5e-324, 2.0 ** -30):
        assert np.any((z == v) & ~np.signbit(z)) and np.any((z == -v) & np.signbit(z))
    for mag in (1e7, 1e8, 1e9):
        assert ((np.abs(zb) >= mag / 2) & (np.abs(zb) <= mag)).sum() >= 200


def test_truth_agrees_with_mpmath(kats):
    for z, sn, cs in ((kats['z'], kats['sin'], kats['cos']), (kats['zb'], kats['sinb'], kats['cosb'])):
        ts, tc = R.truth(z)
        d = max(float(np.abs(ts - sn).max()), float(np.abs(tc - cs).max()))
        print('truth vs mpmath: %.3g * 2^-60' % (d * 2.0 ** 60))
        assert d <= 2.0 ** -60


@pytest.mark.parametrize('name', ['fp64', 'fp32'])
def test_emulation_error_and_symmetry(kats, name):
    f, E, EB, u = (R.emul_sincos64, E64, E64_BEYOND, U64) if name == 'fp64' else (R.emul_sincos32, E32, E32_BEYOND, U32)
    e = _worst(f, kats['z'], kats['sin'], kats['cos'])
    eb = _worst(f, kats['zb'], kats['sinb'], kats['cosb'])
    print('%s: E = %.4f * 2^%d in-domain (worst at z = %r), %.4f beyond' % (name, e.max() / u, np.log2(u), kats['z'][e.argmax()], eb.max() / u))
    for g, gn in enumerate(kats['groups']):
        print('    %-9s %.4f' % (gn, e[kats['group'] == g].max() / u))
    assert e.max() <= E and eb.max() <= EB
    assert e.max() >= 0.98 * E and eb.max() >= 0.98 * EB                 # the constants are the measurement, not a loose cap
    for z in (kats['z'], kats['zb']):
        s, c = f(z); sm, cm = f(-z)
        # odd / even bit for bit: equal values are equal bits except for the sign of a zero, which sin(-0) = +0 does not keep
        assert np.array_equal(sm, -s) and np.array_equal(cm, c)
        nz = s != 0
        assert np.array_equal(np.signbit(sm[nz]), ~np.signbit(s[nz]))
        ld = np.longdouble
        one = np.abs(s.astype(ld) ** 2 + c.astype(ld) ** 2 - 1).astype(np.float64)
        assert one.max() <= 4 * 2 * u, one.max() / (2 * u)               # 4 units in the last place of 1


def test_fp64_domain_edge(kats):
    """The fp64 bound holds at every |fn| of the fixture, through the "beyond" block: the largest |fn| at which it holds is the
    largest there is, and the error does not grow.  Past FN_EDGE the quadrant is lost."""
    z = np.concatenate((kats['z'], kats['zb']))
    sn = np.concatenate((kats['sin'], kats['sinb'])); cs = np.concatenate((kats['cos'], kats['cosb']))
    fn = np.abs(np.rint(z * R.TWO_OVER_PI))
    e = _worst(R.emul_sincos64, z, sn, cs)
    ok = e <= law64(fn)
    edge = fn[ok].max()
    print('fp64 bound holds up to |fn| = %.0f (|z| = %.4g), the largest in the fixture; structural edge |fn| < 2^31' % (edge, edge * np.pi / 2))
    assert np.all(ok) and edge == fn.max() and 6e8 < edge < FN_EDGE
    for lo, hi in ((0, 2 ** 20), (2 ** 20, 2 ** 24), (2 ** 24, 2 ** 27), (2 ** 27, 2 ** 31)):
        m = (fn >= lo) & (fn < hi)
        print('    |fn| in [2^%d, 2^%d): worst %.4f * 2^-53 over %d points' % (np.log2(max(lo, 1)), np.log2(hi), e[m].max() / U64, m.sum()))
        assert m.sum() > 100
    # either side of the edge, against np.longdouble: the last quadrants that still come out, the first that do not
    k = np.arange(1, 41, dtype=np.float64)
    below = (FN_EDGE - k) * (np.pi / 2) + 0.3
    above = (FN_EDGE + k) * (np.pi / 2) + 0.3
    for f, E in ((R.emul_sincos64, E64), (R.emul_sincos32, E32_BEYOND)):
        ts, tc = R.truth(below)
        assert np.all(np.abs(np.rint(below * R.TWO_OVER_PI)) < FN_EDGE)
        assert _worst(f, below, ts, tc).max() <= E
        ts, tc = R.truth(above)
        bad = _worst(f, above, ts, tc) > 0.1
        print('    past the edge: %d of %d points with the wrong quadrant' % (bad.sum(), len(above)))
        assert bad.sum() >= len(above) // 2


MUTANTS = [(n, m) for n in ('fp64', 'fp32') for m in R.MUTATIONS if m != 'mod4' and not (n == 'fp64' and m == 'reduce32')]


@pytest.mark.parametrize('name,mut', MUTANTS)
def test_mutation_breaks_the_gpu_bound(kats, name, mut):
    """Each mutation of the emulation exceeds the bound the GPU tier uses (2 E, element by element) on the in-domain fixture."""
    f, E, u = (R.emul_sincos64, E64, U64) if name == 'fp64' else (R.emul_sincos32, E32, U32)
    e = _worst(f, kats['z'], kats['sin'], kats['cos'], mut)
    n = int((e > 2 * E).sum())
    print('%s %-9s worst / (2 E) = %9.3g, %d of %d points over the bound' % (name, mut, e.max() / (2 * E), n, len(e)))
    assert e.max() > 2 * E
    # and a norm over all entries, the check the suite had, would have let the subtle ones through
    s, c = f(kats['z'], mut); s0, c0 = f(kats['z'])
    nrm = np.sqrt(((s - s0).astype(np.float64) ** 2).sum() + ((c - c0).astype(np.float64) ** 2).sum()) / np.sqrt(len(e))
    print('    norm-wise difference from the unmutated routine: %.2e' % nrm)


@pytest.mark.parametrize('name', ['fp64', 'fp32'])
def test_mod4_is_the_same_function(kats, name):
    """(int)fn % 4 with C's truncating remainder is not a mutation at all: n % 4 is congruent to n mod 4, and the routine only
    looks at bits 0 and 1 of q (q & 1, q & 2, (q + 1) & 2), which two's complement keeps for a negative remainder.  No bound can
    catch it; the neighbouring slip that loses the sign of fn before the mask ('abs_q') is caught above."""
    f = R.emul_sincos64 if name == 'fp64' else R.emul_sincos32
    for z in (kats['z'], kats['zb']):
        s, c = f(z); sm, cm = f(z, 'mod4')
        assert np.array_equal(s, sm) and np.array_equal(c, cm) and np.any(z < 0)


def test_fmaf_single_rounding():
    """the fp32 fma of the emulation against exact rational arithmetic, on products built to land on ties of the double sum"""
    from fractions import Fraction
    rng = np.random.default_rng(7)
    a = rng.standard_normal(4000).astype(np.float32); b = rng.standard_normal(4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(np.float32)          # heavy cancellation
    c[::2] = rng.standard_normal(2000).astype(np.float32)
    # exact ties of the fp32 result with a nonzero remainder behind them: (1 + 2^-24) + 2^-60
    a[:4] = np.float32(1 + 2.0 ** -12); b[:4] = np.float32(1 + 2.0 ** -12)
    c[:4] = np.float32([-2.0 ** -11 + 2.0 ** -24, 2.0 ** -40, -2.0 ** -40, 0.0])
    got = R.fmaf(a, b, c)
    for i in range(len(a)):
        e = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        # nearest float to an exact rational: through a double only when that is exact, else by comparing the two neighbours
        d = np.float32(float(e)); lo, hi = np.nextafter(d, np.float32(-np.inf)), np.nextafter(d, np.float32(np.inf))
        best = min((lo, d, hi), key=lambda v: abs(Fraction(float(v)) - e))
        ties = [v for v in (lo, d, hi) if abs(Fraction(float(v)) - e) == abs(Fraction(float(best)) - e)]
        if len(ties) == 1:
            assert got[i] == best, (i, a[i], b[i], c[i])


def test_inject_and_dispatch():
    z = R.load_kats()['z']
    for kind, (D, S, M) in R.INJECT_KINDS.items():
        D_, S_, M_, params, X = R.inject(kind, z)
        assert (D_, S_, M_) == (D, S, M) and X.shape == (len(z), D) and len(params) == 3 + D * S + M * S + S + M
        from oracle import scfgp_oracle as O
        a, b, c, l_F, r_F, F, l_FC, FC = O.unpack_params(params, D, S, M)
        assert np.all(l_FC == 0) and np.all(FC == 0) and np.all(F[0] == 1) and np.all(F[1:] == 0)
        assert np.exp(b) * np.sqrt(2.0 / M) in (0.5, 0.25, 0.125)
    assert R.fmap_dispatch(1, 1, 8) == ('direct', 'reg3') and R.fmap_dispatch(1, 2, 32) == ('direct', 'reg3')
    assert R.fmap_dispatch(64, 64, 8) == ('direct', 'lds') and R.fmap_dispatch(64, 1, 128) == ('rank', 'reg3')
    assert (1 + 8) % 2 == 1 and (2 + 32) % 2 == 0


@pytest.mark.parametrize('D,S,M', [(8, 20, 8), (64, 32, 128)])
@pytest.mark.parametrize('target', [1e2, 1e6])
def test_dyadic_case_is_exact(D, S, M, target):
    """the int64 phases are what the oracle computes in floating point, to its rounding, and land in the intended regime"""
    from oracle import scfgp_oracle as O
    X, params, Z, e = R.dyadic_case(D, S, M, target, 0x5CF0 + D)
    a, b, c, l_F, r_F, F, l_FC, FC = O.unpack_params(params, D, S, M)
    FF = np.concatenate((X @ l_F + l_FC, X @ F + FC), 1)
    assert Z.shape == FF.shape == (293, S + M)
    assert target / 4 <= np.abs(Z).max() <= target
    # with every partial sum exact, numpy's own order gives the same doubles
    assert np.array_equal(FF, Z)
    assert np.all(X * 256 == np.rint(X * 256)) and X.min() >= 0 and X.max() < 1
