"""
Range tests of the acquisition tails (scfgp_amd/csrc/acquire_math.h, acquire.hip, kg.hip): the grids, the construction of inputs that put
g where it is wanted, the per-row error models and the mutants, shared by the CPU tier (tests/test_acquire_range_ref.py: the numpy
restatement tests/acquire_ref.py and tests/kg_ref.py against mpmath) and the GPU tier (tests/test_gpu_acquire_range.py: the device against
the restatement and against tests/golden/acquire_kats.npz).  numpy only: the GPU tier must not need mpmath.

Error models.  With g formed from the call's own doubles and eps = 2^-52, the error of an output is measured per row in units of

    PI, EI and all their partials; log-EI's partials      eps (1 + g^2) |true|     the exponent g^2 / 2 carries g's own rounding, and
                                                                                    tail_r cancels to eps g^2
    log-EI's value                                        eps max(1, |true|)       absolute
    MES term (n* = 1)                                     eps (|true| + g^2)       the two g^2 / 2 of a term cancel
    MES a_u, a_sigma                                      eps (1 + g^4) |true|     1 + g (g + lam) cancels twice

and a truth below the smallest normal double only has to be met to within that number (tests/acquire_ref.py: TINY).  C_REF holds the
worst such constant of the restatement against mpmath over the grids below, as the CPU tier measures it and asserts it within 4 x; the
GPU tier allows the device 8 x C_REF in the same measure (the margin of tests/test_gpu_acquire.py's PARITY_BOUND: the device's erfc,
erfcx, exp, log and log1p are other implementations).

Knowledge gradient of two reference lines d = (0, -Delta) with slopes b1, b2: KG = |b1 - b2| h(-c), c = Delta / |b1 - b2|, and the lower
bound kg equals it when the crossing lies inside the nodes, and is 0 when it lies outside.  kg is measured in units of

    eps [ (1 + c^2) + Phi(-c) / h(-c) max|z| (|b1| + |b2|) / |b1 - b2| ] |true|

The second term is the rounding of the intercepts m - s z, taken at nodes as far out as max|z|, carried into c (d h(-c) / d c = -Phi(-c)).
It cannot be dropped: the first term alone is off by about 700 x with the default nodes and 10^4 x with the wide ones (|z| up to 60), at
small c.
"""
import contextlib

import numpy as np

from oracle import scfgp_oracle as O
from scfgp_amd import synth
from tests import acquire_ref as A
from tests import pred_cov_ref as PC


EPS = float(np.finfo(np.float64).eps)
TINY = A.TINY
KINDS = ('pi', 'ei', 'logei', 'mes')
OUTPUTS = ('acq', 'au', 'as')
DEVICE_FACTOR = 8                                                # tests/test_gpu_acquire.py: PARITY_BOUND = 8 x MEASURED_KIND_ERR
REF_FACTOR = 4                                                   # the CPU tier's margin over its own measurement

# The restatement's worst constants against 60-digit arithmetic over the grids of this file (both directions, sigma in SIGMAS), as
# tests/test_acquire_range_ref.py::test_restatement_constants measures them and asserts them within 4 x.  Measured (acq / a_u / a_sigma,
# the worse direction): pi 1.85 / 1.13 / 1.10, ei 2.69 / 1.85 / 1.12, logei 4.44 / 3.12 / 2.67, mes 1.82 / 2.07 / 2.05
C_REF = {
    'pi': {'acq': 1.9, 'au': 1.2, 'as': 1.1},
    'ei': {'acq': 2.7, 'au': 1.9, 'as': 1.2},
    'logei': {'acq': 4.5, 'au': 3.2, 'as': 2.7},
    'mes': {'acq': 1.9, 'au': 2.1, 'as': 2.1},
}
# bounds() and the numpy closed form against mpmath under the two-term model, the worst over DEFAULT_NODES and WIDE_NODES
C_REF_KG = 1.6

SIGMAS = np.array([0.37, 1.0, 2.9])
BEST, XI = 0.3, 0.05
SEAMS = (-1.0, -50.0)
DECADES = -10.0 ** np.arange(2, 8)
WIDE_NODES = np.r_[-60.0, -30.0, -15.0, np.linspace(-8.0, 8.0, 25), 15.0, 30.0, 60.0]


# ---- grids -------------------------------------------------------------------------------------------------------------------------
def around(x, n=2):
    """the double x with its n neighbours on either side, ascending (tests/golden/make_acquire_kats.py has its own copy)"""
    lo, hi = [x], [x]
    for _ in range(n):
        lo.append(np.nextafter(lo[-1], -np.inf)); hi.append(np.nextafter(hi[-1], np.inf))
    return np.array(lo[:0:-1] + hi)


def _special():
    return np.concatenate([around(s) for s in SEAMS] + [[0.0, -0.0]])


def grid(kind):
    """(uniform part, special points): [-60, 9] at step 0.1 ([-60, 40] for MES); the seam doubles with two neighbours on either side,
    +-0, 38 and -10^x (x = 2 .. 7 for log-EI with 41 log-spaced points between, which the GPU tier's ladder visits; 2 .. 4 for MES)"""
    if kind == 'mes':
        return np.arange(-600, 401) / 10.0, np.concatenate([_special(), [-1e2, -1e3, -1e4]])
    sp = np.concatenate([_special(), [38.0]])
    if kind == 'logei':
        sp = np.concatenate([sp, DECADES, -np.logspace(2.0, 7.0, 41)])
    return np.arange(-600, 91) / 10.0, sp


def grid_calls(kind, minimize):
    """the calls of the CPU tier: [(mu, sd, kwargs of A.acquire)].  The uniform part with sigma cycling through SIGMAS and the incumbent
    and xi at (BEST, XI); the special points at every sigma with the incumbent (f*) and xi at 0, so that at sigma = 1 g is the point
    itself, bit for bit"""
    sgn = -1.0 if minimize else 1.0
    uni, sp = grid(kind)
    s_uni = SIGMAS[np.arange(uni.size) % 3]
    g_sp, s_sp = np.repeat(sp, 3), np.tile(SIGMAS, sp.size)
    if kind == 'mes':
        f = 0.25
        return [(sgn * (sgn * f - uni * s_uni), s_uni, dict(fstar=np.array([f]), minimize=minimize)),
                (sgn * (-g_sp * s_sp), s_sp, dict(fstar=np.array([0.0]), minimize=minimize))]
    return [(sgn * (uni * s_uni + sgn * BEST + XI), s_uni, dict(best=BEST, xi=XI, minimize=minimize)),
            (sgn * (g_sp * s_sp), s_sp, dict(best=0.0, xi=0.0, minimize=minimize))]


def g_of(kind, mu, sd, best=None, xi=0.0, fstar=None, minimize=False):
    """g of every row in the expression of the device and of tests/acquire_ref.py (MES: n* = 1)"""
    sgn = -1.0 if minimize else 1.0
    u = sgn * np.asarray(mu, np.float64).reshape(-1)
    s = np.asarray(sd, np.float64).reshape(-1)
    with np.errstate(all='ignore'):
        if kind == 'mes':
            return (sgn * float(np.asarray(fstar).reshape(-1)[0]) - u) / s
        return (u - sgn * best - xi) / s


# ---- error models ------------------------------------------------------------------------------------------------------------------
def unit(kind, out, g, true):
    """the absolute size of one unit of the model of (kind, output) at g, given the true value (doubles)"""
    g = np.asarray(g, np.float64); t = np.abs(np.asarray(true, np.float64))
    g2 = g * g
    if kind == 'logei' and out == 'acq':
        return EPS * np.maximum(1.0, t)
    if kind == 'mes':
        return EPS * (t + g2) if out == 'acq' else EPS * (1.0 + g2 * g2) * t
    return EPS * (1.0 + g2) * t


def relative(kind, out):
    """is the measure of (kind, output) relative to the true value (so that TINY's rule applies)?"""
    return not (out == 'acq' and kind in ('logei', 'mes'))


def constants(kind, out, got, true, g, diff=None):
    """per row: |got - true| in units of the model.  diff: |got - true| where the caller formed it in higher precision.  Where the
    measure is relative and |true| < TINY, the row's constant is 0 if |got - true| <= TINY and inf otherwise; a non-finite `got` is inf"""
    got = np.asarray(got, np.float64).reshape(-1); true = np.asarray(true, np.float64).reshape(-1)
    with np.errstate(all='ignore'):
        d = np.abs(got - true) if diff is None else np.asarray(diff, np.float64).reshape(-1)
        c = d / unit(kind, out, g, true)
        if relative(kind, out):
            small = np.abs(true) < TINY
            c = np.where(small, np.where(d <= TINY, 0.0, np.inf), c)
    return np.where(np.isfinite(got), c, np.inf)


def allowance(kind, out, g, true, factor=DEVICE_FACTOR):
    """the absolute allowance of a row: factor x C_REF x the model's unit, and TINY where the truth is below it"""
    a = factor * C_REF[kind][out] * unit(kind, out, g, true)
    return np.maximum(a, TINY) if relative(kind, out) else a


def restatement(kind, mu, sd, acquire=A.acquire, **kw):
    """{'acq', 'au', 'as'} of A.acquire (or of a mutant of it)"""
    return dict(zip(OUTPUTS, acquire(kind, mu, sd, **kw)))


# ---- mutants: variants of the restatement that the per-row assertion must reject ---------------------------------------------------------
@contextlib.contextmanager
def _patched(**kw):
    old = {k: getattr(A, k) for k in kw}
    for k, v in kw.items():
        setattr(A, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(A, k, v)


def _tail_r_plus3(g):
    g = A._f(g)
    with np.errstate(all='ignore'):
        w = 1.0 / g
        w2 = w * w
        series = w2 * (1.0 + w2 * (3.0 + w2 * (15.0 + w2 * (-105.0 + w2 * 945.0))))
        direct = 1.0 - A.SQRT_PI * (-g * A.INV_SQRT2) * A.erfcx(-g * A.INV_SQRT2)
    return np.where(g < -50.0, series, direct)


def _log_ndtr_neg(g):
    g = A._f(g)
    with np.errstate(all='ignore'):
        return np.log(0.5 * A.erfcx(np.abs(g) * A.INV_SQRT2)) - 0.5 * g * g


def _lam_neg(g):
    g = A._f(g)
    with np.errstate(all='ignore'):
        return A.SQRT_2_OVER_PI / A.erfcx(np.abs(g) * A.INV_SQRT2)


def _tail_edit(kind, edit):
    def acquire(k, mu, sd, **kw):
        assert k == kind
        acq, au, as_ = A.acquire(k, mu, sd, **kw)
        tail = ~(g_of(k, mu, sd, **kw) > -1.0)
        s = np.asarray(sd, np.float64).reshape(-1)
        au2, as2 = edit(au, as_, s)
        return acq, np.where(tail, au2, au), np.where(tail, as2, as_)
    return acquire


def _with(**patch):
    def acquire(k, mu, sd, **kw):
        with _patched(**patch):
            return A.acquire(k, mu, sd, **kw)
    return acquire


def _pi_sign(k, mu, sd, **kw):
    acq, au, as_ = A.acquire(k, mu, sd, **kw)
    return acq, au, -as_


# name -> (the kinds it shows in, the mutated acquire).  The series of tail_r runs below -50, where EI itself is 0 in float64: only log-EI
# and its ratios can see it
MUTANTS = {
    'tail_r: -3 -> +3': (('logei',), _with(tail_r=_tail_r_plus3)),
    'tail_r: SQRT_PI -> SQRT_PI_OVER_2': (('ei', 'logei'), _with(SQRT_PI=A.SQRT_PI_OVER_2)),
    'EI tail: a_u = a_sigma = 0': (('ei',), _tail_edit('ei', lambda au, as_, s: (0.0 * au, 0.0 * as_))),
    'log-EI tail: a_u and a_sigma swapped': (('logei',), _tail_edit('logei', lambda au, as_, s: (as_, au))),
    'log-EI tail: no 1 / sigma': (('logei',), _tail_edit('logei', lambda au, as_, s: (au * s, as_ * s))),
    'PI: a_sigma with the wrong sign': (('pi',), _pi_sign),
    'MES: the g < 0 branch for g >= 0': (('mes',), _with(log_ndtr=_log_ndtr_neg, lam=_lam_neg)),
}


# ---- the synthetic fit of the GPU tier and its pools ------------------------------------------------------------------------------------
SHAPE = (3, 1, 20)                                               # K = 42
T_SWEEP = 4096
SEED_SWEEP, SEED_EXACT, SEED_KG_C, SEED_KG_R = 303, 404, 505, 612


def synthetic_factors(D, S, M):
    """tests/test_gpu_acquire.py::_synthetic without the engine: (params, alpha0, Li)"""
    seed = 0x5CF65000 + M
    K = 2 * (S + M)
    params = synth.make_params(seed + 0x0202, D, S, M, abc=(-1.0, 0.0, -1.0))
    rng = np.random.default_rng(seed)
    alpha = rng.standard_normal(K) / np.sqrt(K)
    Li = np.tril(rng.standard_normal((K, K))) / np.sqrt(K)
    return params, alpha, Li


def oracle_mu_sd(Xs, params, alpha, Li, noise, D=SHAPE[0], S=SHAPE[1], M=SHAPE[2]):
    """(mu, sigma) of the rows from the oracle's features: the CPU tier's stand-in for the device's 'mu', 'sd'"""
    mu = O.feature_map(Xs, params, D, S, M) @ np.asarray(alpha, np.float64).reshape(-1)
    v = np.sum(PC.factor(Xs, Li, params, S, M) ** 2, axis=1)
    return mu, A.sigma(PC.kappa(params), v, noise)


def sweep_pool():
    return synth.make_X(SEED_SWEEP, T_SWEEP, SHAPE[0])


def exact_pool():
    """the rows of the exact-g calls: all that matters is that their sigma differ"""
    return synth.make_X(SEED_EXACT, 64, SHAPE[0])


# The dense sweep: alpha = scale alpha0 stretches u / sigma (mu is linear in alpha), the incumbent (f*) shifts it.  place() chooses both from
# the mu, sigma of alpha0 so that the middle 97 % of the rows run from `lo` - 5 to `hi` + 5.
def place(kind, mu0, sd, minimize, lo=None, hi=None):
    """(scale, kwargs of the call) that put g of the pool over [lo, hi] (default: [-60, 8], MES [-60, 40])"""
    sgn = -1.0 if minimize else 1.0
    lo = -60.0 if lo is None else lo
    hi = (40.0 if kind == 'mes' else 8.0) if hi is None else hi
    r = sgn * np.asarray(mu0) / np.asarray(sd)                    # u / sigma at scale 1
    if kind == 'mes':
        r = -r
    q0, q1 = np.percentile(r, [1.5, 98.5])                       # the ends of r are thin (u is smooth: few rows sit near its extremes)
    scale = (hi - lo + 10.0) / (q1 - q0)
    shift = float(np.median(sd)) * (hi + 5.0 - scale * q1)       # g = scale r + shift / sigma
    if kind == 'mes':
        return scale, dict(fstar=np.array([sgn * shift]), minimize=minimize)
    return scale, dict(best=-sgn * shift, xi=0.0, minimize=minimize)


# The ladder: rows x0 + t w at log-spaced t, so that u(x) - u(x0) runs over the decades; with the incumbent at row 0's own u and alpha large,
# g = (u - u0) / sigma reaches -1e7 with every decade of -g from 1e2 up populated (a uniform pool puts almost nothing near u0: a
# decade holds a tenth of the rows of the one above it).  Rows on which u rises above u0 have g > 0 and are not compared.
T_LADDER = 512
LADDER_SCALE = 3.0e8


def ladder_pool(direction=1.0):
    t = np.r_[0.0, np.logspace(-7.5, -0.5, T_LADDER - 1)]
    x0 = np.array([0.31, 0.47, 0.59])
    w = direction * np.array([0.6, -0.5, 0.7])
    return x0[None, :] + t[:, None] * w[None, :]


def ladder_direction(mu0, minimize):
    """+1 or -1: the sign of w along which u falls from row 0 (from mu of the ladder pool at alpha0)"""
    sgn = -1.0 if minimize else 1.0
    return -1.0 if sgn * (mu0[T_LADDER // 2] - mu0[0]) > 0 else 1.0


def sweep_coverage(g, lo, hi, need=4):
    """the unit intervals [k, k + 1) of [lo, hi) that hold fewer than `need` of g"""
    g = np.asarray(g)
    return [k for k in range(int(lo), int(hi)) if np.count_nonzero((g >= k) & (g < k + 1)) < need]


def decade_coverage(g, need=4):
    """the decades [10^x, 10^(x+1)) of -g, x = 2 .. 6, that hold fewer than `need` rows"""
    g = -np.asarray(g)
    return [x for x in range(2, 7) if np.count_nonzero((g >= 10.0 ** x) & (g < 10.0 ** (x + 1))) < need]


def in_measured_range(kind, g):
    """rows whose g lies where C_REF was measured: [-60, 9] ([-60, 40] for MES); log-EI down to -1e7, MES down to -1e4"""
    g = np.asarray(g)
    hi = 40.0 if kind == 'mes' else 9.0
    lo = {'logei': -1e7, 'mes': -1e4}.get(kind, -60.0)
    return (g >= lo) & (g <= hi)


# ---- exact g: an incumbent (f*) that makes fl(-p0 / sigma) a wanted double -----------------------------------------------------------------
def hit(g_want, sd, start=0):
    """(row, p0) with (0.0 - p0 - 0.0) / sd[row] == g_want bit for bit, searching the rows from `start` on and p0 over the doubles next to
    -g_want sd[row]; None if no row does.  u = +-0 (alpha = 0), xi = 0; for MES p0 stands for -sgn f*"""
    T = sd.size
    for k in range(T):
        i = (start + k) % T
        p = -g_want * sd[i]
        cand, up, dn = [p], p, p
        for _ in range(3):
            up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
            cand += [up, dn]
        for p0 in cand:
            if _same_double((0.0 - p0 - 0.0) / sd[i], g_want):
                return i, float(p0)
    return None


def exact_condition(hit_g, fixture_g):
    """the input condition of the exact-g tests: -1.0 and -50.0 and at least one of the two doubles next to them on either side are hit,
    and every other fixture g.  Returns the list of what is missing.  (A neighbour can be out of reach: just above -1.0 the doubles are
    half as far apart as sigma's, and the quotient -p0 / sigma skips some of them for every sigma of a fit.)"""
    hit_g = np.asarray(hit_g, np.float64)
    has = lambda x: bool(np.any((hit_g == x) & (np.signbit(hit_g) == np.signbit(x)))) if x != 0.0 else bool(np.any(hit_g == 0.0))
    missing = []
    near = np.concatenate([around(s) for s in SEAMS])
    for s in SEAMS:
        a = around(s)
        if not has(a[2]):
            missing.append(('seam', s))
        if not (has(a[0]) or has(a[1])):
            missing.append(('below', s))
        if not (has(a[3]) or has(a[4])):
            missing.append(('above', s))
    return missing + [('point', float(x)) for x in fixture_g if x not in near and not has(x)]


def _same_double(a, b):
    return np.float64(a).view(np.int64) == np.float64(b).view(np.int64) or (a == 0.0 and b == 0.0)


# ---- knowledge gradient with two reference lines -----------------------------------------------------------------------------------------
# multiples of the pool's median |b1 - b2|; 5, 15, 20 and 25 fill the unit intervals of c between 27 and 38 that 10 and 30 leave thin
KG_DELTAS = (0.0, 1e-6, 1e-3, 0.1, 1.0, 3.0, 10.0, 30.0, 5.0, 15.0, 20.0, 25.0)
T_KG = 256
BORDER = 1e-9                                                    # crossings this close (relatively) to the outermost node are in neither class


def kg_closed_form(d, B):
    """(KG, c, z*) per row of B (T, 2) for the two lines d (2,) + B z, max d = 0: KG = |b1 - b2| h(-c), c = Delta / |b1 - b2|; z* is the
    signed crossing.  Equal slopes: KG = 0, c = inf"""
    d = np.asarray(d, np.float64).reshape(-1); B = np.asarray(B, np.float64)
    db = B[:, 1] - B[:, 0]
    with np.errstate(all='ignore'):
        zstar = (d[0] - d[1]) / db
        c = np.abs(zstar)
        kg = np.where(db != 0.0, np.abs(db) * A.h(-c), 0.0)
    return kg, np.where(db != 0.0, c, np.inf), np.where(db != 0.0, zstar, np.inf)


def kg_classes(zstar, z):
    """(inside, outside): the crossing lies strictly inside / outside the nodes, BORDER away from the outermost node on its side"""
    z = np.asarray(z, np.float64)
    edge = np.where(zstar < 0, -z[0], z[-1])
    a = np.abs(zstar)
    return a < edge * (1.0 - BORDER), a > edge * (1.0 + BORDER)


def kg_unit(c, B, z, true):
    """one unit of the two-term model of kg (absolute)"""
    B = np.asarray(B, np.float64)
    db = np.abs(B[:, 1] - B[:, 0])
    c = np.where(db != 0.0, c, 0.0)                               # equal slopes: the truth is 0 and so is the unit
    with np.errstate(all='ignore'):
        ratio = A.h_ratios(-c)[0]                                 # Phi(-c) / h(-c) in its tail form: about c far out
        second = np.where(db != 0.0, ratio * np.abs(np.asarray(z)).max() * (np.abs(B[:, 0]) + np.abs(B[:, 1])) / db, 0.0)
    return EPS * ((1.0 + c * c) + second) * np.abs(true)


def kg_pools():
    """(candidates (T_KG, D), two reference rows)"""
    return synth.make_X(SEED_KG_C, T_KG, SHAPE[0]), synth.make_X(SEED_KG_R, 2, SHAPE[0])


def kg_scale(mult, mu_ref0, B):
    """the scale of alpha0 at which Delta = |u1 - u2| is mult x the median |b1 - b2| of the pool (mu_ref0: the two rows' mu at alpha0)"""
    return mult * float(np.median(np.abs(B[:, 1] - B[:, 0]))) / abs(float(mu_ref0[0]) - float(mu_ref0[1]))


def kg_coverage(c, need=4, upto=38):
    """the unit intervals of c in [0, upto) that hold fewer than `need` crossings"""
    c = np.asarray(c)
    return [k for k in range(upto) if np.count_nonzero((c >= k) & (c < k + 1)) < need]
