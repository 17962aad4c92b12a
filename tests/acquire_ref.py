"""
numpy restatement of the acquisition functions of scfgp_acquire (include/scfgp_hip.h; scfgp_amd/csrc/acquire.hip) and of their partials
in u = sgn mu and sigma, in the device's own forms and order of operations:

    UCB    u + beta sigma                       PI     Phi(g),  g = (u - sgn best - xi) / sigma
    EI     sigma h(g),  h = g Phi + phi         LOGEI  log sigma + log h(g)
    MES    mean_s [ g_s lam(g_s) / 2 - log Phi(g_s) ],  g_s = (sgn f*_s - u) / sigma,  lam = phi / Phi

Tail forms, t = -g / sqrt 2:  log Phi = log(erfcx(t) / 2) - g^2 / 2 and lam = sqrt(2 / pi) / erfcx(t) for g < 0; log Phi = log1p(-c),
c = erfcx(-t) exp(-g^2 / 2) / 2, lam = phi / (1 - c) for g >= 0; for g <= -1: h = phi r with r = 1 - sqrt(pi) t erfcx(t) (g >= -50) or
the series g^-2 (1 - 3 g^-2 + 15 g^-4 - 105 g^-6 + 945 g^-8) (g < -50), log h = -g^2 / 2 - log(2 pi) / 2 + log r, Phi / h =
sqrt(pi / 2) erfcx(t) / r, phi / h = 1 / r.
"""
import numpy as np
from scipy.special import erfc, erfcx

KINDS = ('ucb', 'pi', 'ei', 'logei', 'mes')
INV_SQRT2 = 0.70710678118654752440
INV_SQRT_2PI = 0.39894228040143267794
SQRT_2_OVER_PI = 0.79788456080286535588
HALF_LOG_2PI = 0.91893853320467274178
SQRT_PI = 1.77245385090551602730
SQRT_PI_OVER_2 = 1.25331413731550025121


def _f(g):
    return np.atleast_1d(np.asarray(g, np.float64))


def pdf(g):
    g = _f(g)
    return INV_SQRT_2PI * np.exp(-0.5 * g * g)


def cdf(g):
    return 0.5 * erfc(-_f(g) * INV_SQRT2)


def tail_r(g):
    """h / phi for g <= -1 (elsewhere the value is not used)"""
    g = _f(g)
    with np.errstate(all='ignore'):
        w = 1.0 / g
        w2 = w * w
        series = w2 * (1.0 + w2 * (-3.0 + w2 * (15.0 + w2 * (-105.0 + w2 * 945.0))))
        direct = 1.0 - SQRT_PI * (-g * INV_SQRT2) * erfcx(-g * INV_SQRT2)
    return np.where(g < -50.0, series, direct)


def log_ndtr(g):
    g = _f(g)
    with np.errstate(all='ignore'):
        e = erfcx(np.abs(g) * INV_SQRT2)
        hg2 = 0.5 * g * g
        neg = np.log(0.5 * e) - hg2
        pos = np.log1p(-(0.5 * e * np.exp(-hg2)))
    return np.where(g < 0.0, neg, pos)


def lam(g):
    """phi / Phi"""
    g = _f(g)
    with np.errstate(all='ignore'):
        e = erfcx(np.abs(g) * INV_SQRT2)
        ex = np.exp(-0.5 * g * g)
        neg = SQRT_2_OVER_PI / e
        pos = INV_SQRT_2PI * ex / (1.0 - 0.5 * e * ex)
    return np.where(g < 0.0, neg, pos)


def log_h(g):
    g = _f(g)
    with np.errstate(all='ignore'):
        body = np.log(g * cdf(g) + pdf(g))
        tail = -0.5 * g * g - HALF_LOG_2PI + np.log(tail_r(g))
    return np.where(g > -1.0, body, tail)


def h(g):
    g = _f(g)
    with np.errstate(all='ignore'):
        return np.where(g > -1.0, g * cdf(g) + pdf(g), pdf(g) * tail_r(g))


def h_ratios(g):
    """(Phi / h, phi / h)"""
    g = _f(g)
    with np.errstate(all='ignore'):
        hb = g * cdf(g) + pdf(g)
        r = tail_r(g)
        e = erfcx(-g * INV_SQRT2)
        a = np.where(g > -1.0, cdf(g) / hb, SQRT_PI_OVER_2 * e / r)
        b = np.where(g > -1.0, pdf(g) / hb, 1.0 / r)
    return a, b


def mes_term(g):
    """g lam(g) / 2 - log Phi(g) >= 0"""
    g = _f(g)
    return 0.5 * g * lam(g) - log_ndtr(g)


def mes_q(g):
    """-d mes_term / d g = (lam / 2) (1 + g (g + lam))"""
    g = _f(g)
    l = lam(g)
    return 0.5 * l * (1.0 + g * (g + l))


def mes_order_sum(x, lanes=16):
    """the device's order of the sum over the samples (x: (..., n*)): lane l adds the samples l, l + 16, ... in turn, then the lanes'
    partial sums meet in a butterfly (offsets 8, 4, 2, 1)"""
    x = np.asarray(x, np.float64)
    n = x.shape[-1]
    part = np.zeros(x.shape[:-1] + (lanes,))
    for k in range(0, n, lanes):
        blk = x[..., k:k + lanes]
        part[..., :blk.shape[-1]] += blk
    off = lanes // 2
    while off >= 1:
        part = part + part[..., np.arange(lanes) ^ off]
        off //= 2
    return part[..., 0]


def acquire(kind, mu, sd, best=None, xi=0.0, beta=None, fstar=None, minimize=False):
    """(acq, a_u, a_sigma) at mu (T,), sd (T,): the value and its partials in u = sgn mu and in sigma"""
    mu = np.asarray(mu, np.float64).reshape(-1)
    s = np.asarray(sd, np.float64).reshape(-1)
    sgn = -1.0 if minimize else 1.0
    u = sgn * mu
    with np.errstate(all='ignore'):
        if kind == 'ucb':
            return u + beta * s, np.ones_like(u), np.full_like(u, float(beta))
        if kind == 'mes':
            f = sgn * np.asarray(fstar, np.float64).reshape(-1)
            g = (f[None, :] - u[:, None]) / s[:, None]
            q = mes_q(g)
            ns = float(f.size)
            return mes_order_sum(mes_term(g)) / ns, mes_order_sum(q) / ns / s, mes_order_sum(g * q) / ns / s
        g = (u - sgn * best - xi) / s
        if kind == 'pi':
            ph = pdf(g)
            return cdf(g), ph / s, -g * ph / s
        if kind == 'ei':
            return np.where(g > -1.0, s * h(g), s * (pdf(g) * tail_r(g))), cdf(g), pdf(g)
        if kind == 'logei':
            a, b = h_ratios(g)
            hb = g * cdf(g) + pdf(g)
            au = np.where(g > -1.0, cdf(g) / (s * hb), a / s)
            as_ = np.where(g > -1.0, pdf(g) / (s * hb), b / s)
            return np.log(s) + log_h(g), au, as_
    raise ValueError('unknown kind %r' % (kind,))


def sigma(kappa, v, noise):
    """the standard deviation in use, from v = ||Li phi(x)||^2 itself: sqrt(kappa v) (latent) or sqrt(kappa (1 + v)) (predictive)"""
    v = np.asarray(v, np.float64)
    return np.sqrt(kappa * (v + 1.0)) if noise else np.sqrt(kappa * v)


def argmax(acq, w=None):
    """the lowest eligible index of the largest value"""
    acq = np.asarray(acq, np.float64).reshape(-1)
    ok = np.ones(acq.size, bool) if w is None else np.asarray(w).reshape(-1) > 0
    idx = np.flatnonzero(ok)
    return int(idx[np.argmax(acq[idx])])


# The restatement's own maximum error per kind against 50-digit arithmetic, as tests/test_acquire_ref.py measures and asserts it (within
# 4 x): relative where the true value is a normal double; ucb over |u| + beta sigma; logei absolute over max(1, |.|).
MEASURED_KIND_ERR = {'ucb': 1.3e-16, 'pi': 3.9e-13, 'ei': 4.0e-13, 'logei': 1.1e-15, 'mes': 2.3e-13}
TINY = 2.3e-308                 # below the smallest normal double: only underflow is asked for


def kind_error(kind, got, ref, mu=None, sd=None, beta=None):
    """the maximum error of `got` against `ref` (doubles) in the measure of MEASURED_KIND_ERR"""
    got = np.asarray(got, np.float64).reshape(-1); ref = np.asarray(ref, np.float64).reshape(-1)
    if not np.isfinite(got).all():
        return float('inf')
    d = np.abs(got - ref)
    if kind == 'ucb':
        return float(np.max(d / (np.abs(np.asarray(mu).reshape(-1)) + beta * np.asarray(sd).reshape(-1))))
    if kind == 'logei':
        return float(np.max(d / np.maximum(1.0, np.abs(ref))))
    small = np.abs(ref) < TINY
    if (d[small] > TINY).any():
        return float('inf')
    return float(np.max(d[~small] / np.abs(ref[~small]))) if (~small).any() else 0.0
