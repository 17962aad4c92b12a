"""
Reference side of the phase-range tests of the feature map's sin / cos (csrc/sincos.h: fast_sincos), shared by the CPU tier
(tests/test_sincos_ref.py) and the GPU tier (tests/test_gpu_phase_range.py).

  emul_sincos64 / emul_sincos32   the two overloads of fast_sincos restated line by line in numpy, with named mutations
  truth                           sin / cos of the exact double through np.longdouble (64-bit significand)
  load_kats                       tests/golden/sincos_kats.npz (mpmath at 200 bits, made by tests/golden/make_sincos_kats.py)
  inject                          parameters and inputs whose phase is exactly a given z in every column, no rounding anywhere
  dyadic_case                     real multi-term contractions whose phases are known exactly (int64 arithmetic)
  fmap_dispatch                   the kernel FmapKernels::featuremap picks for (D, S, M), restated

Where the emulation can differ from a compiled kernel: it evaluates every expression of the fp64 overload with one rounding per
operation, as written.  A build that contracts a * b + c (the compiler's default) fuses `r - fn * pio2_1t`, `(r - x) - w`, the
Horner steps of both polynomials, `0.5 * y - v * rs`, `... - v * S1` and `z2 * rc - x * y` into fmas, each of which drops one
rounding of a term that is at most |x|^3 / 6 (sin) or |x|^4 / 24 (cos) of the result -- a fraction of 2^-53 each.  The fp32
overload is written in explicit fma / fmaf calls with bare products in between, so there is nothing left to contract: the
emulation is expected to match it bit for bit.
"""
import os
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KATS = os.path.join(HERE, 'golden', 'sincos_kats.npz')

TWO_OVER_PI = 6.36619772367581382433e-01
PIO2_1 = 1.57079632673412561417e+00          # first 33 bits of pi/2: fn * PIO2_1 is exact for |fn| < 2^20
PIO2_1T = 6.07710050650619224932e-11         # pi/2 - PIO2_1, rounded
FN_EXACT = 2.0 ** 20                         # below this |fn| the product fn * PIO2_1 fits a double
S64 = (-1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04,
       2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10)
C64 = (4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05,
       -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11)
S32 = (-1.6666654611e-1, 8.3321608736e-3, -1.9515295891e-4)
C32 = (4.166664568298827e-2, -1.388731625493765e-3, 2.443315711809948e-5)

# Mutations of the emulation (tests/test_sincos_ref.py): each restates one way the routine could be subtly wrong.
#   no_tail   the pio2_1t term of the reduction dropped
#   trunc     fn by truncation instead of rint
#   cos_q     the sign of cos from q & 2 instead of (q + 1) & 2
#   reduce32  fp32 overload only: the reduction itself in fp32
#   s1_digit  S1 one unit off in the last decimal digit its format guarantees (the 15th for fp64, the 6th for fp32)
#   abs_q     the quadrant from |fn|: the sign of a negative fn lost before the mask
#   mod4      (int)fn % 4 with C's truncating remainder instead of & 3 -- see test_mod4_is_the_same_function
MUTATIONS = ('no_tail', 'trunc', 'cos_q', 'reduce32', 's1_digit', 'abs_q', 'mod4')


# ---- exact fused multiply-adds -------------------------------------------------------------------------------------------------
def fma64(a, b, c):
    """fma(a, b, c) in fp64 with its single rounding, element by element in exact rational arithmetic."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    out = np.empty(a.shape)
    flat = out.reshape(-1)
    for i, (x, y, w) in enumerate(zip(a.ravel().tolist(), b.ravel().tolist(), c.ravel().tolist())):
        e = Fraction(x) * Fraction(y) + Fraction(w)
        flat[i] = float(e) if e else x * y + w          # an exact zero takes its sign from the IEEE sum; int / int is correctly rounded
    return out


def fmaf(a, b, c):
    """fmaf(a, b, c) in fp32 with its single rounding.  The product of two floats is exact in a double; the sum is formed with its
    rounding error (TwoSum), and where it lands exactly half way between two floats the error decides the direction, so the
    second rounding to fp32 cannot differ from a single one."""
    a = np.asarray(a, np.float32).astype(np.float64); b = np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    p = a * b
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    bits = s.view(np.int64) if s.ndim else np.asarray(s).reshape(1).view(np.int64)
    tie = ((bits & np.int64((1 << 29) - 1)) == np.int64(1 << 28)).reshape(np.shape(s))
    nudge = np.where(err > 0, np.nextafter(s, np.inf), np.where(err < 0, np.nextafter(s, -np.inf), s))
    return np.where(tie & (err != 0), nudge, s).astype(np.float32)


def _reduce_first(fn, z):
    """fma(-fn, pio2_1, z): a plain subtract where the product is exact, the exact fma elsewhere"""
    r = z - fn * PIO2_1
    big = np.abs(fn) >= FN_EXACT
    if np.any(big):
        r = r.copy()
        r[big] = fma64(-fn[big], PIO2_1, z[big])
    return r


def _quadrant(fn, mut):
    n = np.clip(fn, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)  # (int)fn; it saturates where the int cannot hold fn (|fn| >= 2^31)
    if mut == 'abs_q':
        return np.abs(n) & 3
    if mut == 'mod4':
        return np.fmod(n, 4)                                    # C's %: the sign of the dividend
    return n & 3


def _select(s, c, q, mut):
    odd = (q & 1) != 0
    ss = np.where(odd, c, s); cc = np.where(odd, s, c)
    sn = np.where((q & 2) != 0, -ss, ss)
    cs = np.where(((q if mut == 'cos_q' else q + 1) & 2) != 0, -cc, cc)
    return sn, cs


def _fn(z, mut):
    t = z * TWO_OVER_PI
    return np.trunc(t) if mut == 'trunc' else np.rint(t)        # rint: ties to even, as the hardware rounds


def emul_sincos64(z, mut=None):
    """fast_sincos(double, double&, double&) of csrc/sincos.h, one rounding per written operation."""
    z = np.atleast_1d(np.asarray(z, np.float64))
    fn = _fn(z, mut)
    r = _reduce_first(fn, z)
    w = fn * (0.0 if mut == 'no_tail' else PIO2_1T)
    x = r - w
    y = (r - x) - w
    z2 = x * x
    S1, S2, S3, S4, S5, S6 = S64
    if mut == 's1_digit':
        S1 = -1.66666666666667e-01                              # ...666e-01 at 15 digits, its last one up by one
    v = z2 * x
    rs = S2 + z2 * (S3 + z2 * (S4 + z2 * (S5 + z2 * S6)))
    s = x - ((z2 * (0.5 * y - v * rs) - y) - v * S1)
    C1, C2, C3, C4, C5, C6 = C64
    rc = z2 * (C1 + z2 * (C2 + z2 * (C3 + z2 * (C4 + z2 * (C5 + z2 * C6)))))
    hz = 0.5 * z2
    wc = 1.0 - hz
    c = wc + (((1.0 - wc) - hz) + (z2 * rc - x * y))
    return _select(s, c, _quadrant(fn, mut), mut)


def emul_sincos32(z, mut=None):
    """fast_sincos(double, float&, float&): the fp64 reduction in two exact fmas, then the cephes kernels in fp32."""
    f = np.float32
    z = np.atleast_1d(np.asarray(z, np.float64))
    if mut == 'reduce32':
        zf = z.astype(f)
        t = zf * f(TWO_OVER_PI)
        fn = np.rint(t).astype(np.float64)
        x = fmaf(-fn.astype(f), f(PIO2_1T), fmaf(-fn.astype(f), f(PIO2_1), zf))
    else:
        fn = _fn(z, mut)
        r = _reduce_first(fn, z)
        if mut != 'no_tail':
            r = fma64(-fn, PIO2_1T, r)                          # the one inexact fma of this overload
        x = r.astype(f)
    z2 = x * x
    S1, S2, S3 = (f(v) for v in S32)
    if mut == 's1_digit':
        S1 = f(-1.66666e-1)                                     # -1.66667e-1 at 6 digits, its last one off by one
    C1, C2, C3 = (f(v) for v in C32)
    s = fmaf(x * z2, fmaf(z2, fmaf(z2, S3, S2), S1), x)
    c = fmaf(z2 * z2, fmaf(z2, fmaf(z2, C3, C2), C1), fmaf(f(-0.5), z2, f(1.0)))
    return _select(s, c, _quadrant(fn, mut), mut)


# ---- truth ---------------------------------------------------------------------------------------------------------------------
def truth(z):
    """(sin z, cos z) of the exact doubles z as np.longdouble.  The x87 format carries a 64-bit significand and the C library's
    sinl / cosl reduce the argument exactly, so the values are good to about 2^-63: 2^-10 of an fp64 ulp of headroom.
    tests/test_sincos_ref.py holds them against mpmath (the fixture) to 2^-60."""
    assert np.finfo(np.longdouble).nmant >= 63, 'np.longdouble is no wider than a double on this platform'
    zl = np.asarray(z, np.float64).astype(np.longdouble)
    return np.sin(zl), np.cos(zl)


def load_kats():
    """The fixture as a dict: 'z', 'sin', 'cos' (in-domain block, |fn| < 2^20) and 'zb', 'sinb', 'cosb' (the "beyond" block,
    2^20 <= |fn| < 2^31); sin / cos as np.longdouble = hi + lo of the stored double pairs (about 106 bits of mpmath's value)."""
    d = np.load(KATS)
    ld = np.longdouble
    out = {'z': d['z'], 'zb': d['zb'], 'group': d['group'], 'groups': [str(g) for g in d['groups']]}
    for k in ('sin', 'cos', 'sinb', 'cosb'):
        out[k] = d[k][:, 0].astype(ld) + d[k][:, 1].astype(ld)
    return out


def abs_err(got, ref):
    """|got - ref| in np.longdouble, as float64 (the differences are far above the double's underflow)"""
    return np.abs(np.asarray(got).astype(np.longdouble) - ref).astype(np.float64)


# ---- injected phases -----------------------------------------------------------------------------------------------------------
INJECT_KINDS = {
    #            D   S   M     what runs
    'reg_odd': (1, 1, 8),      # 2 live rows: featuremap_reg_kernel<T, 3>, J = 9 (scalar stores of the sine half)
    'reg_even': (1, 2, 32),    # the same kernel, J = 34 (vector stores)
    'lds': (64, 64, 8),        # 65 live rows, Sp = Dp: the direct form through featuremap_kernel<T>
    'rank': (64, 1, 128),      # Sp = 16 < Dp = 80: project_kernel, then the register kernel on T~
}


def pack_params(l_F, r_F, l_P, P, abc=(0.0, 0.0, 0.0)):
    """the flat vector [a b c | l_F (D x S) | r_F (M x S) | l_P (S) | P (M)]"""
    return np.concatenate([np.asarray(abc, np.float64), np.ravel(l_F), np.ravel(r_F), np.ravel(l_P), np.ravel(P)]).astype(np.float64)


def inject(kind, z):
    """(D, S, M, params, X) whose phase in row n is exactly z[n] in every one of the J = S + M columns.  a = b = c = 0 and M is
    8, 32 or 128, so the scale s = e^b sqrt(2 / M) is a power of two and Phi / s is the raw output of fast_sincos.  Row 0 of l_F is
    ones, column 0 of r_F is ones, everything else zero: F[0][m] = 1 exactly, and l_P = P = 1 / D cancel the column means, so the
    only nonzero term of every phase is x[n][0] * 1."""
    D, S, M = INJECT_KINDS[kind]
    z = np.asarray(z, np.float64).ravel()
    l_F = np.zeros((D, S)); l_F[0] = 1.0
    r_F = np.zeros((M, S)); r_F[:, 0] = 1.0
    l_P = np.full(S, 1.0 / D); P = np.full(M, 1.0 / D)
    X = np.zeros((len(z), D)); X[:, 0] = z
    # in integers: the coefficient of x[:, 0] is 1, of every other column 0, and D * offset = D * l_P - sum_d l_F = 0
    Li = l_F.astype(np.int64); Ri = r_F.astype(np.int64)
    assert np.array_equal(Li, l_F) and np.array_equal(Ri, r_F) and D & (D - 1) == 0
    coef = np.concatenate((Li, Li @ Ri.T), 1)                                   # D x J
    assert np.all(coef[0] == 1) and np.all(coef[1:] == 0)
    DlP = l_P * D; DP = P * D
    assert np.all(DlP == np.rint(DlP)) and np.all(DP == np.rint(DP))
    off = np.concatenate((DlP.astype(np.int64), DP.astype(np.int64))) - coef.sum(0)
    assert np.all(off == 0) and np.all(X[:, 1:] == 0)
    assert M in (8, 32, 128)
    return D, S, M, pack_params(l_F, r_F, l_P, P), X


def inject_expected(D, S, M, Dp, Jp, Sp=None, Spp=None):
    """What the unpacking kernels must leave for inject()'s parameters, bit for bit: Fall (Dp x Jp), and with Sp the factors
    Lall (Dp x Spp) = [l_F | e_D] and Rall (Sp x Jp) = [e_s | r_F^T ; offsets] of the rank-S form."""
    J = S + M
    Fall = np.zeros((Dp, Jp)); Fall[0, :J] = 1.0
    if Sp is None:
        return Fall
    Lall = np.zeros((Dp, Spp)); Lall[0, :S] = 1.0; Lall[D, S] = 1.0
    Rall = np.zeros((Sp, Jp))
    Rall[:S, :S] = np.eye(S); Rall[0, S:J] = 1.0
    return Fall, Lall, Rall


# ---- exact phases from real contractions ---------------------------------------------------------------------------------------
def dyadic_case(D, S, M, target, seed, N=293):
    """X, l_F, r_F, l_P, P as integer multiples of 2^-8 drawn from synth.uniform (X and r_F in [0, 1), l_F in [-1, 1), the phases
    in [0, 2 pi)), l_F then scaled by the largest power of two 2^e that keeps max |z| <= target (so it is above target / 4).  D is a power of two, so the
    column means are exact, and every product, partial sum and offset is an integer multiple of u = 2^(e - 24) / D whose
    magnitude over u stays below 2^53 however the sum is ordered -- through Fall directly or through the rank-S factors.  So the
    phase matrix is the same double in any accumulation order, and it is returned computed in int64.
    Returns (X, params, Z (N x J float64, exact), e)."""
    from scfgp_amd import synth
    assert D & (D - 1) == 0, 'D must be a power of two'
    lgD = D.bit_length() - 1
    i64 = np.int64
    Xi = np.floor(synth.uniform(seed, 0, N * D) * 256).astype(i64).reshape(N, D)                 # / 2^8
    Li = (np.floor(synth.uniform(seed + 1, 0, D * S) * 512).astype(i64) - 256).reshape(D, S)      # / 2^8, before the scale
    Ri = np.floor(synth.uniform(seed + 2, 0, M * S) * 256).astype(i64).reshape(M, S)             # / 2^8
    lPi = np.floor(synth.uniform(seed + 3, 0, S) * 1608).astype(i64)                              # / 2^8, [0, 2 pi)
    Pi = np.floor(synth.uniform(seed + 4, 0, M) * 1608).astype(i64)
    Fi = Li @ Ri.T                                                                                # / 2^16

    def phases(e):
        # in units of u = 2^(e - 24 - lgD): the offsets l_P, P (2^-8) need the shift sh >= 0 to be integers there
        sh = 16 - e + lgD
        assert sh >= 0, 'the scale 2^%d leaves the phase offsets no exact place' % e
        # X l_F is in 2^(e - 16) = 256 D u, the mean of l_F in 2^(e - 8) / D = 65536 u; X F in D u, the mean of F in 256 u
        ZL = 256 * D * (Xi @ Li) - 65536 * Li.sum(0) + (lPi << sh)
        ZM = D * (Xi @ Fi) - 256 * Fi.sum(0) + (Pi << sh)
        # every partial sum, in any order and through either form, is bounded by the sum of the magnitudes
        aL = 256 * D * (np.abs(Xi) @ np.abs(Li)) + 65536 * np.abs(Li).sum(0) + (lPi << sh)
        aM = D * (np.abs(Xi) @ (np.abs(Li) @ Ri.T)) + 256 * (np.abs(Li) @ Ri.T).sum(0) + (Pi << sh)
        return np.concatenate((ZL, ZM), 1), max(int(aL.max()), int(aM.max()))

    Z0, _ = phases(0)
    base = float(np.abs(Z0).max()) * 2.0 ** (-24 - lgD)
    e = int(np.floor(np.log2(target / base))) + 1                 # the offsets do not scale with e: step down to the target
    while True:
        Zi, bound = phases(e)
        if float(np.abs(Zi).max()) * 2.0 ** (e - 24 - lgD) <= target:
            break
        e -= 1
    assert bound < 2 ** 53, 'bit budget: a partial sum could need %d bits' % bound.bit_length()
    u = 2.0 ** (e - 24 - lgD)
    Z = Zi.astype(np.float64) * u                                  # |Zi| < 2^53 and u a power of two: exact
    assert np.array_equal(Z / u, Zi.astype(np.float64))
    zmax = np.abs(Z).max()
    assert target / 4 <= zmax <= target, (zmax, target)
    X = Xi / 256.0
    l_F = Li * 2.0 ** (e - 8); r_F = Ri / 256.0
    return X, pack_params(l_F, r_F, lPi / 256.0, Pi / 256.0), Z, e


# ---- dispatch ------------------------------------------------------------------------------------------------------------------
def fmap_dispatch(D, S, M):
    """(form, kernel) FmapKernels::featuremap picks: 'direct' | 'rank', 'reg3' | 'reg4' | 'reg5' | 'reg8' | 'reg9' | 'lds'."""
    up = lambda v, m: -(-v // m) * m
    Dp, Sp = up(D + 1, 16), up(S + 1, 16)
    lowrank = Sp < Dp                                              # through the S columns when that is narrower
    Kd = Sp if lowrank else Dp                                     # depth of the contraction that ends in sin / cos
    live = (S if lowrank else D) + 1
    nk = (live + 3) // 4
    kern = 'lds'
    if nk <= 9:
        for NK, need in ((3, 12), (4, 16), (5, 20), (8, 32)):      # the next instantiated depth inside the padded leading dimension
            if nk <= NK and Kd >= need:
                kern = 'reg%d' % NK
                break
        else:
            if Kd >= 36:
                kern = 'reg9'
    return ('rank' if lowrank else 'direct'), kern
