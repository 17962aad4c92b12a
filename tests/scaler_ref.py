"""
Reference side of the range tests of the scaler transforms on the device, shared by the CPU tier (tests/test_scaler_ref.py) and the
GPU tier (tests/test_gpu_scaler_range.py).  The six device functions are

  scale_x, scale_x_deriv   csrc/fmap.hip            pd_scale_x        csrc/pd.hip (the same text as scale_x)
  norm_ppf, y_backward     csrc/yscale.h            y_backward_deriv  csrc/kernels_params.hip

and the two formulas built on them, std_y of ypost_kernel and dstd of ygrad_kernel (csrc/kernels_params.hip).

  ppf, scale_x, scale_x_deriv, y_backward, y_backward_deriv, y_std, y_dstd
        the restatement: numpy, operation by operation in the device's evaluation order, one rounding per operation, with the named
        mutations of MUTATIONS and, for the ppf, any table of the 48 AS 241 coefficients (mutated_coef)
  model_ppf, model_scale_x, model_scale_x_deriv, model_y_backward, model_y_backward_deriv, model_y_std, model_y_dstd
        value and allowance of one result from one text for two arithmetics: MP (mpmath at 60 digits: the value is the reference, ppf
        is the true quantile -- erfinv in the upper half, Newton on log ncdf(z) - log p in the lower) and FL (fp64: the allowance at
        arguments that are only known on the GPU machine, where mpmath is not needed)
  classify, judge
        result classes and the comparison of an array of results with reference, allowance and class
  load_kats
        tests/golden/scaler_kats.npz, made by tests/golden/make_scaler_kats.py

The error model.  The allowance of a result f is its first-order forward error bound

    allow = 2^-53 * sum over the fp64 intermediates v of the evaluation order of  b_v * |df/dv| * |v|

with the partial derivatives written out analytically.  b_v = 1 for the result of + - * / and sqrt (IEEE: half an ulp, so 2^-53 |v|)
and b_v = 16 for the result of every exp, log, pow and erfc call.  Source of the 16: the OpenCL C specification's table of relative
errors for the full profile ("Relative Error as ULPs": exp <= 3 ulp, log <= 3 ulp, pow <= 16 ulp, erfc <= 16 ulp in double
precision), which is what the ROCm device library (ocml) is specified to; 16 is the loosest of the four and is used for all of them.
No document with the library's own measured figures ships with the ROCm install, so these are not replaced by tighter ones.
Arguments and scaler parameters are fp64 already and carry no budget.  |v| is floored at 2^-1022: below it a rounding costs half a
subnormal step whatever v is.  Three places go beyond the bare first-order sum, each because the sum is not a bound there:

  * the rational approximations of AS 241 are exact to "about 1 part in 10^16" (Wichura 1988), which no rounding accounts for:
    B_AS241 = 2 units of 2^-53 |z| are added to every ppf result;
  * u = t lm + 1 reaches pow(|u|, .) with an absolute error, so next to u = 0 a derivative at one point says nothing about the
    neighbourhood: that one term is the exact change of the (monotone) power over the interval u +- E_u instead.  Where the
    interval holds 0 and the exponent is negative (y_backward_deriv with lm > 1) no bound exists: class UNB below;
  * the reference stored in the fixture is itself rounded to fp64: 2^-53 |ref| is added when the fixture is written.

A build that contracts a * b + c into an fma drops a rounding the model counts, so it stays inside the allowance.

Classes.  Where the reference is 0, +-inf or NaN the allowance means nothing and the class is compared: ZERO (either sign), PINF, NINF,
NAN.  SUB: the reference is below 2^-1022 in magnitude; the allowance is at least one subnormal step per operation.  ANYNF: the
true value is the product of an underflowed density and an infinite factor (scale_x_deriv mode 5 at t = 0 with lm < 1 where
exp(-z^2 / 2) is 0 in fp64): the device forms 0 * inf, and any non-finite result is accepted.  UNB: the allowance is unbounded
(above); any result but NaN is accepted.  The fixture may hold at most 1 % of a function's arguments in SUB, ANYNF and UNB together.

On the GPU machine the arguments of the y scaler's functions are whatever bits the device produced, so no mpmath value exists for
them.  There the reference is this restatement evaluated in np.longdouble (64-bit significand: its own roundings are 2^-11 of
fp64's, and exp, log, pow and sqrt exist in that type), and the allowance is the model's in FL arithmetic, taken once.
"""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KATS = os.path.join(HERE, 'golden', 'scaler_kats.npz')

U = 2.0 ** -53
TINY = 2.0 ** -1022
STEP = 2.0 ** -1074
B_OP, B_FN, B_AS241 = 1, 16, 2

INV_SQRT_2PI = 0.39894228040143267794
SQRT_HALF = 0.70710678118654752440
SPLIT1 = 0.425
SPLIT2 = 5.0

# AS 241 (PPND16) as csrc/yscale.h writes it: numerator and denominator of the three branches, highest power first, the constant 1 of
# every denominator included -- 48 numbers
COEF = np.array([
    [2.5090809287301226727e3, 3.3430575583588128105e4, 6.7265770927008700853e4, 4.5921953931549871457e4,
     1.3731693765509461125e4, 1.9715909503065514427e3, 1.3314166789178437745e2, 3.3871328727963666080e0],
    [5.2264952788528545610e3, 2.8729085735721942674e4, 3.9307895800092710610e4, 2.1213794301586595867e4,
     5.3941960214247511077e3, 6.8718700749205790830e2, 4.2313330701600911252e1, 1.0],
    [7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e0,
     3.64784832476320460504e0, 5.76949722146069140550e0, 4.63033784615654529590e0, 1.42343711074968357734e0],
    [1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
     6.89767334985100004550e-1, 1.67638483018380384940e0, 2.05319162663775882187e0, 1.0],
    [2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
     2.96560571828504891230e-1, 1.78482653991729133580e0, 5.46378491116411436990e0, 6.65790464350110377720e0],
    [2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
     1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0]])
COEF.setflags(write=False)

# Coefficient mutations that cannot move any fp64 result by more than the allowance anywhere in [5e-324, 1 - 2^-53], as
# (index 0..47, computed bound of the relative change of the result over the branch, smallest relative allowance of the branch).
# None is needed: every one of the 48 breaks the allowance somewhere in the fixture (test_every_as241_coefficient_is_pinned).
EXEMPT = []

#   swap_tail        the tail argument taken from the wrong side (1 - p where q < 0)
#   no_tail_sign     the tail result returned without its sign
#   no_sign_bc       sign(t) dropped in the Box-Cox map of scale_x (and of scale_x_deriv's z)
#   no_sign_ibc      sign(u) dropped in the inverse Box-Cox map of y_backward
#   pow_lm           scale_x_deriv: pow(|t|, lm) for pow(|t|, lm - 1)
#   inv_lm           y_backward_deriv: exponent 1 / lm for 1 / lm - 1
#   mode3_algebraic  y_backward mode 3 as the algebraic inverse ppf(x) std + mu of the forward map (the reference's own expression,
#                    which the device follows, is (ppf(x) - mu) / std)
#   no_range_x       (max - min) dropped from scale_x_deriv
#   no_range_y       (max - min) dropped from y_backward_deriv
#   one_sided        the std formula as bw(m + s) - bw(m) for (bw(m + s) - bw(m - s)) / 2
MUTATIONS = ('swap_tail', 'no_tail_sign', 'no_sign_bc', 'no_sign_ibc', 'pow_lm', 'inv_lm', 'mode3_algebraic', 'no_range_x',
             'no_range_y', 'one_sided')

VALUE, ZERO, PINF, NINF, NAN, SUB, ANYNF, UNB = range(8)
CLASS_NAMES = ('value', 'zero', '+inf', '-inf', 'nan', 'subnormal', 'any non-finite', 'unbounded')
LEFT_OUT = (SUB, ANYNF, UNB)                                           # the classes that the value comparison leaves out
LAMBDAS = (math.log1p(math.exp(-5.0)), 0.3, 1.0, math.log1p(math.exp(5.0)))      # softplus(-5), 0.3, 1, softplus(5)


def mutated_coef(i):
    """COEF with coefficient i (row-major, 0..47) moved by one unit in its 6th significant digit"""
    c = COEF.copy()
    v = c.flat[i]
    c.flat[i] = v + 10.0 ** (math.floor(math.log10(abs(v))) - 5)
    return c


# ---- the restatement -----------------------------------------------------------------------------------------------------------
_erfc = np.frompyfunc(math.erfc, 1, 1)


def erfc(x):
    """libm's erfc element by element (numpy has none)"""
    return _erfc(np.asarray(x, np.float64)).astype(np.float64)


def _arr(x):
    """fp64, or np.longdouble where the caller asks for the restatement in that type (see the module docstring)"""
    x = np.asarray(x)
    return x if x.dtype == np.longdouble else x.astype(np.float64)


def ld(par):
    """scaler parameters as np.longdouble, so that a restatement on them runs in that type throughout"""
    return np.asarray(par, np.longdouble)


def _horner(c, r):
    acc = c[0] * r + c[1]
    for k in range(2, 8):
        acc = acc * r + c[k]
    return acc


def _sign(t):
    """(t < 0 ? -1.0 : (t > 0 ? 1.0 : 0.0)): 0 for a NaN too"""
    return np.where(t < 0, -1.0, np.where(t > 0, 1.0, 0.0))


def ppf(p, coef=COEF, mut=None):
    """norm_ppf of csrc/yscale.h"""
    p = _arr(p)
    with np.errstate(all='ignore'):
        q = p - 0.5
        r = 0.180625 - q * q
        central = q * _horner(coef[0], r) / _horner(coef[1], r)
        lower = (q >= 0) if mut == 'swap_tail' else (q < 0)
        r = np.sqrt(-np.log(np.where(lower, p, 1.0 - p)))
        r2 = r - 1.6
        v2 = _horner(coef[2], r2) / _horner(coef[3], r2)
        r3 = r - 5.0
        v3 = _horner(coef[4], r3) / _horner(coef[5], r3)
        v = np.where(r <= SPLIT2, v2, v3)
        tail = v if mut == 'no_tail_sign' else np.where(q < 0, -v, v)
        out = np.where(np.abs(q) <= SPLIT1, central, tail)
        out = np.where(p == 0.0, -np.inf, np.where(p == 1.0, np.inf, out))
        return np.where((p >= 0.0) & (p <= 1.0), out, np.nan)


def ppf_branch(p):
    """0 central, 1 the middle branch (r <= 5), 2 the far tail (r > 5), -1 where norm_ppf returns before any branch"""
    p = _arr(p)
    with np.errstate(all='ignore'):
        q = p - 0.5
        r = np.sqrt(-np.log(np.where(q < 0, p, 1.0 - p)))
        b = np.where(np.abs(q) <= SPLIT1, 0, np.where(r <= SPLIT2, 1, 2))
        return np.where((p > 0.0) & (p < 1.0), b, -1)


def _boxcox_z(x, mn, mx, lm, mu, sd, mut):
    t = (x - mn) / (mx - mn)
    s = 1.0 if mut == 'no_sign_bc' else _sign(t)
    bc = (s * np.power(np.abs(t), lm) - 1.0) / lm
    return t, (bc - mu) / sd


def scale_x(x, mode, par, mut=None):
    """scale_x of csrc/fmap.hip (and pd_scale_x of csrc/pd.hip); par = (min, max, boxcox, mu, std), each broadcast against x"""
    x = _arr(x)
    mn, mx, lm, mu, sd = par
    with np.errstate(all='ignore'):
        if mode == 0:
            return x + 0.0
        if mode == 1:
            return (x - mn) / (mx - mn)
        if mode == 2:
            return (x - mu) / sd
        if mode == 3:
            return 0.5 * erfc(-((x - mu) / sd) * SQRT_HALF)
        t, z = _boxcox_z(x, mn, mx, lm, mu, sd, mut)
        return z if mode == 4 else 0.5 * erfc(-z * SQRT_HALF)


def scale_x_deriv(x, mode, par, mut=None):
    """scale_x_deriv of csrc/fmap.hip"""
    x = _arr(x)
    mn, mx, lm, mu, sd = par
    one = np.ones(np.broadcast(x, mn).shape)
    with np.errstate(all='ignore'):
        if mode == 0:
            return one
        if mode == 1:
            return one * (1.0 if mut == 'no_range_x' else 1.0 / (mx - mn))
        if mode == 2:
            return one * (1.0 / sd)
        if mode == 3:
            z = (x - mu) / sd
            return INV_SQRT_2PI * np.exp(-0.5 * z * z) / sd
        t, z = _boxcox_z(x, mn, mx, lm, mu, sd, mut)
        ex = lm if mut == 'pow_lm' else lm - 1.0
        dz = np.power(np.abs(t), ex) / (sd if mut == 'no_range_x' else (mx - mn) * sd)
        return dz if mode == 4 else INV_SQRT_2PI * np.exp(-0.5 * z * z) * dz


def y_backward(x, mode, par, mut=None, coef=COEF):
    """y_backward of csrc/yscale.h; par = (min, max, boxcox, mu, std)"""
    x = _arr(x)
    mn, mx, lm, mu, sd = par
    with np.errstate(all='ignore'):
        if mode == 0:
            return x + 0.0
        if mode == 1:
            return x * (mx - mn) + mn
        if mode == 2:
            return x * sd + mu
        if mode == 3:
            return ppf(x, coef, mut) * sd + mu if mut == 'mode3_algebraic' else (ppf(x, coef, mut) - mu) / sd
        t = x * sd + mu if mode == 4 else ppf(x, coef, mut) * sd + mu
        u = t * lm + 1.0
        s = 1.0 if mut == 'no_sign_ibc' else _sign(u)
        ib = s * np.power(np.abs(u), 1.0 / lm)
        return ib * (mx - mn) + mn


def y_backward_deriv(x, mode, par, mut=None, coef=COEF):
    """y_backward_deriv of csrc/kernels_params.hip"""
    x = _arr(x)
    mn, mx, lm, mu, sd = par
    one = np.ones(np.broadcast(x, mn).shape)
    with np.errstate(all='ignore'):
        if mode == 0:
            return one
        if mode == 1:
            return one * (1.0 if mut == 'no_range_y' else mx - mn)
        if mode == 2:
            return one * sd
        if mode == 3:
            z = ppf(x, coef, mut)
            return 1.0 / (INV_SQRT_2PI * np.exp(-0.5 * z * z) * sd)
        if mode == 4:
            t = x * sd + mu
            dt = one * sd
        else:
            z = ppf(x, coef, mut)
            t = z * sd + mu
            dt = sd / (INV_SQRT_2PI * np.exp(-0.5 * z * z))
        ex = 1.0 / lm if mut == 'inv_lm' else 1.0 / lm - 1.0
        return (1.0 if mut == 'no_range_y' else (mx - mn)) * np.power(np.abs(t * lm + 1.0), ex) * dt


def y_std(m, s, mode, par, mut=None):
    """std_y of ypost_kernel: half the transformed +-1 std band"""
    m = _arr(m)
    s = _arr(s)
    with np.errstate(all='ignore'):
        if mut == 'one_sided':
            return y_backward(m + s, mode, par) - y_backward(m, mode, par)
        return 0.5 * (y_backward(m + s, mode, par, mut) - y_backward(m - s, mode, par, mut))


def y_dstd(m, s, gm, gs, mode, par, mut=None):
    """dstd of ygrad_kernel"""
    m, s, gm, gs = (_arr(a) for a in (m, s, gm, gs))
    with np.errstate(all='ignore'):
        return 0.5 * (y_backward_deriv(m + s, mode, par, mut) * (gm + gs) - y_backward_deriv(m - s, mode, par, mut) * (gm - gs))


# ---- two arithmetics for the model ----------------------------------------------------------------------------------------------
class FL(object):
    """fp64: numbers are Python floats; overflow, division by zero and invalid operations give inf / nan as on the device"""
    name = 'fl'
    inf = float('inf')
    nan = float('nan')

    @staticmethod
    def num(x):
        return float(x)

    @staticmethod
    def exp(x):
        try:
            return math.exp(x)
        except OverflowError:
            return float('inf')

    @staticmethod
    def log(x):
        if x != x or x < 0:
            return float('nan')
        return math.log(x) if x > 0 else -float('inf')

    @staticmethod
    def sqrt(x):
        return math.sqrt(x) if x >= 0 else float('nan')

    @staticmethod
    def erfc(x):
        return math.erfc(x)

    @staticmethod
    def pow(a, b):
        """a >= 0"""
        if a != a or b != b:
            return float('nan')
        if a == 0:
            return float('inf') if b < 0 else (1.0 if b == 0 else 0.0)
        if math.isinf(a):
            return float('inf') if b > 0 else (1.0 if b == 0 else 0.0)
        try:
            return math.pow(a, b)
        except OverflowError:
            return float('inf')

    @staticmethod
    def div(a, b):
        if b == 0:
            return float('nan') if (a == 0 or a != a) else math.copysign(float('inf'), a) * math.copysign(1.0, b)
        return a / b

    @staticmethod
    def isnan(x):
        return x != x

    @staticmethod
    def isinf(x):
        return x in (float('inf'), -float('inf'))

    @staticmethod
    def ppf(p):
        return float(ppf(p))


def mp_arith(dps=60):
    """mpmath at `dps` digits with the same interface; inf and nan are Python floats"""
    import mpmath as mp
    mp.mp.dps = dps
    mpf = mp.mpf

    class MP(object):
        name = 'mp'
        inf = float('inf')
        nan = float('nan')
        module = mp

        @staticmethod
        def num(x):
            x = float(x) if not isinstance(x, mpf) else x
            return x if isinstance(x, float) and (x != x or x in (float('inf'), -float('inf'))) else mpf(x)

        @staticmethod
        def isnan(x):
            return x != x

        @staticmethod
        def isinf(x):
            return x == float('inf') or x == -float('inf')

        @staticmethod
        def exp(x):
            if MP.isnan(x):
                return MP.nan
            if MP.isinf(x):
                return MP.inf if x > 0 else mpf(0)
            return mp.exp(x)

        @staticmethod
        def log(x):
            if MP.isnan(x) or x < 0:
                return MP.nan
            if x == 0:
                return -MP.inf
            return MP.inf if MP.isinf(x) else mp.log(x)

        @staticmethod
        def sqrt(x):
            if MP.isnan(x) or x < 0:
                return MP.nan
            return MP.inf if MP.isinf(x) else mp.sqrt(x)

        @staticmethod
        def erfc(x):
            if MP.isnan(x):
                return MP.nan
            if MP.isinf(x):
                return mpf(0) if x > 0 else mpf(2)
            return mp.erfc(x)

        @staticmethod
        def pow(a, b):
            if MP.isnan(a) or MP.isnan(b):
                return MP.nan
            if a == 0:
                return MP.inf if b < 0 else (mpf(1) if b == 0 else mpf(0))
            if MP.isinf(a):
                return MP.inf if b > 0 else (mpf(1) if b == 0 else mpf(0))
            return mp.power(a, b)

        @staticmethod
        def div(a, b):
            if MP.isnan(a) or MP.isnan(b):
                return MP.nan
            if b == 0:
                return MP.nan if a == 0 else (MP.inf if a > 0 else -MP.inf)
            if MP.isinf(b):
                return MP.nan if MP.isinf(a) else mpf(0)
            return a / b

        @staticmethod
        def ppf(p):
            """the true quantile of an exact p in [0, 1]"""
            if p == 0:
                return -MP.inf
            if p == 1:
                return MP.inf
            if p >= 0.5:
                return mp.sqrt(2) * mp.erfinv(2 * p - 1)
            z = mpf(float(ppf(float(p)))) if p >= 1e-320 else -mp.sqrt(-2 * mp.log(p))
            lp = mp.log(p)
            for _ in range(8):                                        # Newton on log ncdf(z) - log p; quadratic from 1e-16 on
                c = mp.erfc(-z / mp.sqrt(2)) / 2
                z = z - (mp.log(c) - lp) * c / (mp.exp(-z * z / 2) / mp.sqrt(2 * mp.pi))
            return z

    return MP


def _a(A, x):
    return x if x >= 0 else -x


def _fl(v):
    """|v| floored at the smallest normal number: the magnitude that a rounding of v is relative to"""
    v = v if v >= 0 else -v
    return v if v >= TINY else TINY


def _bad(A, *xs):
    return any(A.isnan(x) or A.isinf(x) for x in xs)


def _horner_model(A, c, r):
    """value of the Horner form, sum over its 14 intermediates v of |dP/dv| |v|, and dP/dr"""
    ar = _a(A, r)
    acc = A.num(c[0])
    der = A.num(0.0)
    parts = []
    for k in range(1, 8):
        der = der * r + acc
        acc = acc * r
        parts.append(acc)
        acc = acc + A.num(c[k])
        parts.append(acc)
    # the result of step k (its product, then its sum) is multiplied by r another 7 - k times
    s = A.num(0.0)
    for i, v in enumerate(parts):
        k = i // 2 + 1
        s = s + _fl(v) * ar ** (7 - k)
    return acc, s, der


def model_ppf(A, p, coef=COEF):
    """(z, allowance, operations) of norm_ppf at the fp64 number p"""
    pf = float(p)
    if not (0.0 <= pf <= 1.0):
        return A.nan, 0.0, 0
    if pf == 0.0:
        return -A.inf, 0.0, 0
    if pf == 1.0:
        return A.inf, 0.0, 0
    p = A.num(pf)
    z = A.ppf(p)
    az = _a(A, z)
    q = p - A.num(0.5)
    qf = pf - 0.5                                                      # the branch the device takes, decided in fp64
    if abs(qf) <= SPLIT1:
        qq = q * q
        r = A.num(0.180625) - qq
        num, snum, dnum = _horner_model(A, coef[0], r)
        den, sden, dden = _horner_model(A, coef[1], r)
        dR = dnum / den - num * dden / (den * den)                     # d (num / den) / dr
        allow = az * (snum / _a(A, num) + sden / _a(A, den) + 2 + B_AS241)             # ... q * num, / den
        allow = allow + _a(A, q * dR) * (3 * qq + _fl(r))              # q (twice into q * q), q * q and r through dR / dr
        allow = allow + _fl(z)                                         # q itself through the leading factor
        return z, U * allow, 34
    lower = qf < 0
    pp = p if lower else A.num(1.0) - p
    L = A.log(pp)
    aL = _a(A, L)
    cond = A.exp(L + z * z / 2) / A.num(INV_SQRT_2PI)                  # pp / pdf(z) = |dz / d log pp|, without an underflowing pdf
    rr = A.sqrt(-L)
    rf = math.sqrt(-math.log(pf if lower else 1.0 - pf))
    shift, cn, cd = (1.6, coef[2], coef[3]) if rf <= SPLIT2 else (5.0, coef[4], coef[5])
    r = rr - A.num(shift)
    num, snum, dnum = _horner_model(A, cn, r)
    den, sden, dden = _horner_model(A, cd, r)
    allow = az * (snum / _a(A, num) + sden / _a(A, den) + 1 + B_AS241)
    allow = allow + cond * ((0 if lower else _fl(pp)) / pp + B_FN * aL + 2 * aL + 2 * aL * _fl(r) / rr)  # 1 - p, log, sqrt, r - shift
    return z, U * allow, 34


def _pdf(A, z):
    return A.num(INV_SQRT_2PI) * A.exp(-z * z / 2)


def _pdf_parts(A, z):
    """pdf(z) = c * e with e = exp(-z * z / 2), and the sum over the product z * z, e and c * e of |d pdf / dv| |v| (units of U; e
    and c * e may be subnormal, where the floor of |v| is what counts)"""
    e = A.exp(-z * z / 2)
    ce = A.num(INV_SQRT_2PI) * e
    return ce, ce * (z * z / 2) + B_FN * _fl(e) * INV_SQRT_2PI + _fl(ce)


def _x_z(A, x, par):
    """Box-Cox part shared by scale_x and scale_x_deriv in modes 4 and 5: t, |t|, z, E_z (absolute, in units of U)"""
    mn, mx, lm, mu, sd = (A.num(v) for v in par)
    xm = x - mn
    rng = mx - mn
    t = A.div(xm, rng)
    if _bad(A, t):
        return t, t, A.nan, A.nan
    at = _a(A, t)
    sg = -1 if t < 0 else (1 if t > 0 else 0)
    pw = A.pow(at, lm)
    m1 = sg * pw - 1
    bc = m1 / lm
    d = bc - mu
    z = d / sd
    # t carries three roundings (x - min, max - min, the quotient), all relative: d z / d t * t = |t|^lm / std
    ez = (3 * lm * _fl(pw) + B_FN * _fl(pw)) / (lm * _a(A, sd)) + (_fl(m1) / lm + _fl(bc) + _fl(d)) / _a(A, sd) + _fl(z)
    return t, at, z, ez


def model_scale_x(A, x, mode, par):
    """(value, allowance, operations) of scale_x at the fp64 number x"""
    xf = float(x)
    if xf != xf:
        return A.nan, 0.0, 0
    x = A.num(xf)
    mn, mx, lm, mu, sd = (A.num(v) for v in par)
    if mode == 0:
        return x, 0.0, 0
    if mode == 1:
        f = (x - mn) / (mx - mn)
        return f, U * 3 * _fl(f), 3
    if mode == 2:
        f = (x - mu) / sd
        return f, U * 2 * _fl(f), 2
    if mode == 3:
        z = (x - mu) / sd
        ez, n = 2 * _fl(z), 2
    else:
        t, at, z, ez = _x_z(A, x, par)
        n = 9
        if mode == 4:
            return z, U * ez, n
    w = -z * A.num(SQRT_HALF)
    e = A.erfc(w)
    f = e / 2
    allow = (ez + _fl(z)) * _pdf(A, z) + B_FN * _fl(e) / 2             # z and the product z * sqrt(1/2) through Phi' = pdf; erfc
    return f, U * allow, n + 3


def model_scale_x_deriv(A, x, mode, par):
    """(value, allowance, operations) of scale_x_deriv at the fp64 number x"""
    xf = float(x)
    if xf != xf:
        return A.nan, 0.0, 0
    x = A.num(xf)
    mn, mx, lm, mu, sd = (A.num(v) for v in par)
    if mode == 0:
        return A.num(1.0), 0.0, 0
    if mode == 1:
        f = 1 / (mx - mn)
        return f, U * 2 * _fl(f), 2
    if mode == 2:
        f = 1 / sd
        return f, U * _fl(f), 1
    if mode == 3:
        z = (x - mu) / sd
        ce, sce = _pdf_parts(A, z)
        f = ce / sd
        # z (two roundings) through z * z: 2 z^2; the density's own intermediates; the quotient
        return f, U * (_a(A, f) * 2 * z * z + sce / _a(A, sd) + _fl(f)), 7
    t, at, z, ez = _x_z(A, x, par)
    if _bad(A, t):
        return A.nan, 0.0, 0
    ex = lm - 1
    pw2 = A.pow(at, ex)
    rs = (mx - mn) * sd
    dz = A.div(pw2, rs) if not A.isinf(pw2) else (A.inf if rs > 0 else -A.inf)
    if A.isinf(dz):
        if mode == 4:
            return dz, 0.0, 0
        dens = float(np.exp(-0.5 * np.float64(float(z)) ** 2))
        return (dz, 0.0, 0) if dens > 0 else ('anynf', 0.0, 0)
    lg = _a(A, A.log(at)) if at > 0 else 0
    # t three times through |t|^(lm - 1); lm - 1 through log|t|; pow; max - min, the product with std, the quotient
    rel = 3 * _a(A, ex) + _fl(ex) * lg + B_FN + 3
    if mode == 4:
        return dz, U * _fl(dz) * rel, 16
    ce, sce = _pdf_parts(A, z)
    f = ce * dz
    allow = _a(A, f) * rel + sce * _a(A, dz) + _fl(f) + _a(A, f) * _a(A, z) * ez
    return f, U * allow, 21


def _pow_span(A, u, eu, ex):
    """largest change of |.|^ex (signed where `ex` is the inverse Box-Cox exponent: monotone) over [u - eu, u + eu]"""
    def F(v):
        return A.pow(_a(A, v), ex)
    lo, hi = u - eu, u + eu
    if ex < 0 and lo <= 0 <= hi:
        return A.inf
    f0 = F(u)
    return max(_a(A, F(lo) - f0), _a(A, F(hi) - f0))


def _signed_pow_span(A, u, eu, ex):
    def F(v):
        w = A.pow(_a(A, v), ex)
        return -w if v < 0 else w
    f0 = F(u)
    return max(_a(A, F(u - eu) - f0), _a(A, F(u + eu) - f0))


def _y_u(A, x, mode, par):
    """t, u = t lm + 1 and E_u (absolute, U applied), dt / dx and its relative allowance (U applied), for modes 4 and 5"""
    mn, mx, lm, mu, sd = (A.num(v) for v in par)
    if mode == 4:
        t1 = x * sd
        t = t1 + mu
        et = U * (_fl(t1) + _fl(t))
        dt, rdt, z, az = sd, 0.0, None, 0.0
    else:
        z, az, _ = model_ppf(A, x)
        if _bad(A, z):
            return z, z, 0.0, z, 0.0, z, 0.0
        zs = z * sd
        t = zs + mu
        et = az * _a(A, sd) + U * (_fl(zs) + _fl(t))
        ce, sce = _pdf_parts(A, z)
        dt = sd / ce
        rdt = az * _a(A, z) + U * (sce / ce + 1)                       # z through exp(-z^2 / 2); the density's intermediates; the quotient
    tl = t * lm
    u = tl + 1
    eu = et * lm + U * (_fl(tl) + _fl(u))
    return t, u, eu, dt, rdt, z, az


def model_y_backward(A, x, mode, par):
    """(value, allowance, operations) of y_backward at the fp64 number x"""
    xf = float(x)
    if xf != xf:
        return A.nan, 0.0, 0
    x = A.num(xf)
    mn, mx, lm, mu, sd = (A.num(v) for v in par)
    if mode == 0:
        return x, 0.0, 0
    if A.isinf(x) and mode in (1, 2, 4):
        return (x if mode != 4 else A.nan), 0.0, 0                     # not used by the fixture
    if mode == 1:
        v = x * (mx - mn)
        f = v + mn
        return f, U * (2 * _fl(v) + _fl(f)), 3
    if mode == 2:
        v = x * sd
        f = v + mu
        return f, U * (_fl(v) + _fl(f)), 2
    if mode == 3:
        z, az, n = model_ppf(A, x)
        if _bad(A, z):
            return (z if A.isnan(z) else (z if sd > 0 else -z)), 0.0, 0
        d = z - mu
        f = d / sd
        return f, (az + U * _fl(d)) / _a(A, sd) + U * _fl(f), n + 2
    t, u, eu, dt, rdt, z, az = _y_u(A, x, mode, par)
    if _bad(A, t):
        if A.isnan(t):
            return A.nan, 0.0, 0
        big = t * lm > 0                                               # u = +-inf: ib = +-inf
        s = (mx - mn) * (1 if big else -1)
        return (A.inf if s > 0 else (-A.inf if s < 0 else A.nan)), 0.0, 0
    il = 1 / lm
    au = _a(A, u)
    pw = A.pow(au, il)
    ib = -pw if u < 0 else (pw if u > 0 else A.num(0.0))
    rng = mx - mn
    v = ib * rng
    f = v + mn
    lg = _a(A, A.log(au)) if au > 0 else 0
    # u (interval form), 1 / lm through log|u|, pow (which may be subnormal where the product is not), max - min, the product, the sum
    allow = _signed_pow_span(A, u, eu, il) * _a(A, rng) + U * (_a(A, v) * (lg * il + 1) + B_FN * _fl(pw) * _a(A, rng) + _fl(v) + _fl(f))
    return f, allow, (8 if mode == 4 else 42)


def model_y_backward_deriv(A, x, mode, par, second=False):
    """(value, allowance, operations) of y_backward_deriv at the fp64 number x; second: (..., d value / dx) for the dstd formula"""
    def ret(f, a, n, d2=0.0):
        return (f, a, n, d2) if second else (f, a, n)
    xf = float(x)
    if xf != xf:
        return ret(A.nan, 0.0, 0)
    x = A.num(xf)
    mn, mx, lm, mu, sd = (A.num(v) for v in par)
    if mode == 0:
        return ret(A.num(1.0), 0.0, 0)
    if mode == 1:
        f = mx - mn
        return ret(f, U * _fl(f), 1)
    if mode == 2:
        return ret(sd, 0.0, 0)
    if mode == 3:
        z, az, n = model_ppf(A, x)
        if A.isnan(z):
            return ret(A.nan, 0.0, 0)
        if A.isinf(z):
            return ret(A.inf if sd > 0 else -A.inf, 0.0, 0)            # 1 / (0 * std)
        pdf, sce = _pdf_parts(A, z)
        f = 1 / (pdf * sd)
        allow = _a(A, f) * az * _a(A, z) + U * (_a(A, f) * (sce / pdf + _fl(pdf * sd) / _a(A, pdf * sd)) + _fl(f))
        return ret(f, allow, n + 5, A.div(A.div(z, pdf), pdf * sd))
    t, u, eu, dt, rdt, z, az = _y_u(A, x, mode, par)
    if A.isnan(t):
        return ret(A.nan, 0.0, 0)
    if A.isinf(t):
        return ret('anynf', 0.0, 0)                                    # x = 0 or 1 in mode 5: pow(inf, .) * sd / 0
    il = 1 / lm
    ex = il - 1
    au = _a(A, u)
    pw = A.pow(au, ex)
    rng = mx - mn
    if A.isinf(pw):
        s = rng * dt
        return ret(A.inf if s > 0 else (-A.inf if s < 0 else A.nan), 0.0, 0)
    f = rng * pw * dt
    lg = _a(A, A.log(au)) if au > 0 else 0
    span = _pow_span(A, u, eu, ex)
    # u (interval form); 1 / lm and 1 / lm - 1 through log|u|; pow; max - min and two products; dt
    allow = span * _a(A, rng * dt) + _a(A, f) * rdt + U * (_a(A, f) * (lg * (il + _fl(ex)) + 1) + B_FN * _fl(pw) * _a(A, rng * dt)
                                                           + _fl(rng * pw) * _a(A, dt) + _fl(f))
    if not second:
        return f, allow, (12 if mode == 4 else 50)
    sg = -1 if u < 0 else 1
    d2 = rng * ex * A.pow(au, ex - 1) * sg * lm * dt * dt if u != 0 else A.nan
    if mode == 5:
        d2 = d2 + f * z / _pdf(A, z)
    return f, allow, (12 if mode == 4 else 50), d2


def model_y_std(A, m, s, mode, par):
    """(value, allowance, operations) of std_y = (bw(m + s) - bw(m - s)) / 2 at the fp64 numbers m, s"""
    m, s = float(m), float(s)
    out, allow, nops = [], 0.0, 2
    for a in (m + s, m - s):                                           # the sums as the device forms them: their rounding is an
        f, af, n = model_y_backward(A, a, mode, par)                   # error of a through bw' = y_backward_deriv
        if _bad(A, f):
            out.append(f)
            continue
        d = model_y_backward_deriv(A, a, mode, par)[0]
        exact = A.num(m) + A.num(s) if a == m + s else A.num(m) - A.num(s)
        moved = _a(A, exact - A.num(a))                                # what the sum's rounding did, exactly (fp64: 0 -> U |a|)
        if A.name == 'fl':
            moved = U * _fl(a)
        if _bad(A, d) or isinstance(d, str):
            d, moved = 0.0, 0.0
        allow = allow + af + _a(A, d) * moved
        nops += n + 1
        out.append(f)
    hi, lo = out
    if A.isnan(hi) or A.isnan(lo) or (A.isinf(hi) and A.isinf(lo) and hi == lo):
        return A.nan, 0.0, 0
    if A.isinf(hi) or A.isinf(lo):
        return (hi if A.isinf(hi) else -lo), 0.0, 0
    f = (hi - lo) / 2
    return f, allow / 2 + U * _fl(f), nops


def model_y_dstd(A, m, s, gm, gs, mode, par):
    """(value, allowance, operations) of dstd = (D(m + s) (gm + gs) - D(m - s) (gm - gs)) / 2, D = y_backward_deriv"""
    m, s, gm, gs = float(m), float(s), float(gm), float(gs)
    terms, allow, nops = [], 0.0, 2
    for a, g, ge in ((m + s, gm + gs, A.num(gm) + A.num(gs)), (m - s, gm - gs, A.num(gm) - A.num(gs))):
        d, ad, n, d2 = model_y_backward_deriv(A, a, mode, par, second=True)
        if isinstance(d, str):
            return 'anynf', 0.0, 0
        if A.isnan(d):
            return A.nan, 0.0, 0
        if A.isinf(d):
            terms.append(d * g if g != 0 else A.nan)
            continue
        v = d * A.num(g)
        d2 = 0.0 if _bad(A, d2) else d2
        # D's own allowance, the rounding of m +- s through D', of gm +- gs, of the product
        allow = allow + ad * abs(g) + _a(A, d2) * U * _fl(a) * abs(g) + U * _a(A, d) * _fl(g) + U * _fl(v)
        nops += n + 3
        terms.append(v)
    hi, lo = terms
    if A.isnan(hi) or A.isnan(lo) or (A.isinf(hi) and A.isinf(lo) and hi == lo):
        return A.nan, 0.0, 0
    if A.isinf(hi) or A.isinf(lo):
        return (hi if A.isinf(hi) else -lo), 0.0, 0
    f = (hi - lo) / 2
    return f, allow / 2 + U * _fl(f), nops


# ---- classes and the comparison ---------------------------------------------------------------------------------------------------
def to_double(v):
    """nearest double to an mpf (exact rational arithmetic: correct in the subnormal range and at overflow) or a float"""
    if isinstance(v, float):
        return v
    from fractions import Fraction
    from mpmath import libmp, isfinite
    if not isfinite(v):
        return float(v)
    if v == 0 or abs(v) * 2 ** 1100 < 1:
        return 0.0
    if abs(v) > 2 ** 1025:                                             # to_rational would build the whole integer
        return math.copysign(float('inf'), v)
    p, q = libmp.to_rational(v._mpf_)
    try:
        return float(Fraction(p, q))
    except OverflowError:
        return math.copysign(float('inf'), p)


def classify(value, allow, nops):
    """(reference as fp64, allowance as fp64, class) of one model result"""
    if isinstance(value, str):
        return float('nan'), 0.0, ANYNF
    if value != value:
        return float('nan'), 0.0, NAN
    ref = to_double(value)
    if ref == float('inf'):
        return ref, 0.0, PINF
    if ref == -float('inf'):
        return ref, 0.0, NINF
    if value == 0:
        return 0.0, 0.0, ZERO
    mag = abs(value)
    if not isinstance(mag, float) and mag * 2 ** 1080 < 1:             # rounds to zero with room to spare
        return 0.0, 0.0, ZERO
    al = to_double(allow) if not isinstance(allow, float) else allow
    if al != al or al == float('inf'):
        return ref, float('inf'), UNB
    if mag < TINY:
        return ref, max(al, nops * STEP) + STEP, SUB
    return ref, al + U * abs(ref), VALUE


def judge(got, ref, allow, cls):
    """(ok, ratio): element-wise verdict, and |got - ref| / allowance where a value is compared (0 elsewhere)"""
    got, ref, allow, cls = np.broadcast_arrays(np.asarray(got, np.float64), ref, allow, cls)
    with np.errstate(all='ignore'):
        ld = np.longdouble
        err = np.abs(got.astype(ld) - ref.astype(ld)).astype(np.float64)
        val = (cls == VALUE) | (cls == SUB)
        ratio = np.where(val, np.where(err == 0, 0.0, err / allow), 0.0)
        ok = np.where(val, np.isfinite(got) & (err <= allow), False)
        ok = np.where(cls == ZERO, got == 0, ok)
        ok = np.where(cls == PINF, got == np.inf, ok)
        ok = np.where(cls == NINF, got == -np.inf, ok)
        ok = np.where(cls == NAN, np.isnan(got), ok)
        ok = np.where(cls == ANYNF, ~np.isfinite(got), ok)
        ok = np.where(cls == UNB, ~np.isnan(got), ok)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
    return ok.astype(bool), ratio


def model_array(fn, A, args, *rest):
    """fn over the rows of `args` (tuples of arguments): arrays of reference, allowance and class"""
    n = len(args)
    ref = np.empty(n); allow = np.empty(n); cls = np.empty(n, np.int8)
    for i, a in enumerate(args):
        a = a if isinstance(a, tuple) else (a,)
        ref[i], allow[i], cls[i] = classify(*fn(A, *(a + rest)))
    return ref, allow, cls


def load_kats():
    with np.load(KATS) as z:
        return {k: z[k] for k in z.files}


# ---- shared by the two tiers: the fixture, hand-filled host scalers, and the steering of the y-scaler tests -----------------------
X_MODES = (1, 2, 3, 4, 5)
ALGOS = ('min-max', 'normal', 'inv-normal', 'auto-normal', 'auto-inv-normal')
_KATS = {}
_STEER = {}


def kats():
    """the fixture, read once and left unchanged"""
    if not _KATS:
        k = load_kats()
        for a in k.values():
            a.setflags(write=False)
        _KATS.update(k)
    return _KATS


def host_scaler(mode, par):
    """a scfgp_amd.scaler.Scaler of `mode` filled by hand with par = (min, max, boxcox, mu, std), (5,) or (5, D)"""
    from scfgp_amd.scaler import Scaler
    s = Scaler(ALGOS[mode - 1])
    par = np.asarray(par, np.float64).reshape(5, -1)
    s.data = {'cols': list(range(par.shape[1])), 'min': par[0], 'max': par[1], 'boxcox': par[2], 'mu': par[3], 'std': par[4]}
    return s


STEER_D, STEER_S, STEER_M, STEER_T = 4, 2, 4, 257
# per mode: the range that the ramp covers at offset 0 and scale 1
STEER_TARGET = {1: (-3.0, 4.0), 2: (-3.0, 4.0), 3: (0.03, 0.97), 4: (-3.0, 1.5), 5: (0.03, 0.97)}
# (name, offset, scale, c, band): the scaled mean is offset + scale * ramp; sigma = sqrt(kappa), kappa = log(1 + e^c) as the library and
# the reference write it -- a multiple of 2^-53 and 0 from c = -37 down, so sigma cannot follow the mean below 1e-8.  band: mu +- sigma
# stays inside (0, 1) in the modes that go through the ppf, so that std_y and dstd are finite too; elsewhere they are judged by class.
#   body, 1e-4    central and middle branch of the ppf, both sides of 0.075 and 0.925
#   r5            the lower r = 5 boundary p = e^-25 from both sides
#   far, 1e-100, 1e-300   the far tail down to the last decades of the normal range
#   upper         1 - p on both sides of e^-25: the upper middle branch, the upper far tail and its boundary
STEER_STEPS = (('body', 0.0, 1.0, -14.0, True), ('1e-4', 0.0, 1e-4, -32.0, True), ('r5', 0.0, 4e-11, -32.0, False),
               ('far', 0.0, 1e-13, -32.0, False), ('1e-100', 0.0, 1e-100, -32.0, False), ('1e-300', 0.0, 1e-300, -32.0, False),
               ('upper', 1.0 - 3e-11, 2.9e-11, -32.0, False))


def steer_params(c):
    """parameters of the y-scaler tests: column 0 of l_F is zero, so that feature 0 is the same number in every row and a weight on
    it alone is an offset of the mean"""
    from scfgp_amd import synth
    params = synth.make_params(0x5CA1E202, STEER_D, STEER_S, STEER_M, abc=(-1.0, 0.0, c))
    params[3:3 + STEER_D * STEER_S:STEER_S] = 0.0
    return params


def steering(i):
    """(mode, par, X, a_const, a_ramp) of parameter set i of the fixture: rows on a short segment, the weights whose mean is 1 in every
    row and those whose mean follows a ramp over STEER_TARGET[mode] (least squares on the oracle's feature map).  alpha of a step is
    offset * a_const + scale * a_ramp."""
    from oracle import scfgp_oracle as O
    from scfgp_amd import synth
    if i not in _STEER:
        k = kats()
        mode, par = int(k['y_mode'][i]), k['y_par'][i]
        s = synth.uniform(0x5CA1E300, 0, STEER_T)
        X = 0.5 + 0.6 * s[:, None] * np.array([0.3, -0.2, 0.25, 0.15])[None, :]
        Phi = O.feature_map(X, steer_params(-14.0), STEER_D, STEER_S, STEER_M)
        assert np.all(Phi[:, 0] == Phi[0, 0]) and abs(Phi[0, 0]) > 0.05
        a_const = np.zeros(Phi.shape[1]); a_const[0] = 1.0 / Phi[0, 0]
        lo, hi = STEER_TARGET[mode]
        a_ramp = np.linalg.lstsq(Phi, lo + (hi - lo) * s, rcond=None)[0]
        for a in (X, a_const, a_ramp, Phi):
            a.setflags(write=False)
        _STEER[i] = (mode, par, X, a_const, a_ramp, Phi)
    return _STEER[i][:5]


def steering_means(i):
    """per step the scaled means on the oracle's feature map and sigma: what the CPU tier checks the steering on"""
    steering(i)
    Phi = _STEER[i][5]
    _, _, _, a_const, a_ramp = _STEER[i][:5]
    return [(name, Phi @ (off * a_const + scale * a_ramp), float(np.sqrt(np.log(1.0 + np.exp(c)))), band)
            for name, off, scale, c, band in STEER_STEPS]


def fl_model(fn, rows, mode, par):
    """reference-free allowance and class at fp64 arguments: (allowance, class) from the model in FL arithmetic"""
    _, allow, cls = model_array(fn, FL, rows, mode, tuple(np.asarray(par, np.float64).tolist()))
    return allow, cls
