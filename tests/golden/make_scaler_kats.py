"""
Known-answer vectors for the scaler transforms on the device (csrc/fmap.hip: scale_x, scale_x_deriv; csrc/pd.hip: pd_scale_x;
csrc/yscale.h: norm_ppf, y_backward; csrc/kernels_params.hip: y_backward_deriv and the std / dstd formulas): hard arguments, and per
argument the reference from mpmath at 60 digits rounded to fp64, the allowance of the error model and the result class, all three
from tests/scaler_ref.py (model_*, classify).  The tests read the fixture; only this maker needs mpmath.

    python tests/golden/make_scaler_kats.py        ->  tests/golden/scaler_kats.npz

  ppf_*            norm_ppf: p = 10^-u down to 1e-300, uniform draws, 1 - 10^-u, +-1e-6 (relative) and +-3 ulp around the branch
                   boundaries 0.075, 0.925 and e^-25, +-20 ulp around 1 - e^-25, 1/2 and its neighbours, 5e-324, the smallest normal,
                   1 - 2^-53, and the arguments that return before any branch: 0, 1, -0.0, a negative, 1 + 2^-52, NaN
  x{m}_*, dx{m}_*  scale_x and scale_x_deriv in mode m = 1..5: an argument matrix of four columns, column j with its own min, max, mu,
                   std and the Box-Cox exponent LAMBDAS[j]; rows inside [min, max], at both ends, min + 10^-u (max - min), below min
                   and above max out to 15 range widths, z spread over +-38 and beyond, and around the x0 at which bc - mu cancels
  y_*, dy_*        y_backward and y_backward_deriv for 11 parameter sets (modes 1, 2, 3 and modes 4, 5 with each exponent): the ppf's
                   arguments thinned, arguments outside [0, 1], and arguments around u = t lm + 1 = 0 from both sides
  ys_*, yd_*       the std and dstd formulas at (m, s) with s from 1e-12 |m| to bands that leave (0, 1) on one side and on both

The draws come from scfgp_amd.synth.uniform and the archive is written with fixed member dates and no compression, so a second run
reproduces the file bit for bit.
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from scfgp_amd import synth                                    # noqa: E402
from tests import scaler_ref as R                              # noqa: E402
from tests.golden.make_sincos_kats import write_npz            # noqa: E402

SEED = 0x5CA1E000
E25 = math.exp(-25.0)
X_RANGES = ((0.0, 1.0), (-3.5, 12.25), (1e-3, 2.5e-3), (100.0, 100.5))
X_STD = (0.8, 0.11, 0.29, 0.013)
T0 = 0.37
Y_RANGE = (-3.5, 12.25)


def ulps(x, ks=(-3, -2, -1, 0, 1, 2, 3)):
    out = []
    for k in ks:
        v = np.float64(x)
        for _ in range(abs(k)):
            v = np.nextafter(v, np.inf if k > 0 else -np.inf)
        out.append(float(v))
    return out


def around(b, n):
    """b (1 +- 1e-6 k / n) for k = 1..n and b +- 0..3 ulp"""
    out = ulps(b)
    for k in range(1, n + 1):
        out += [b * (1 - 1e-6 * k / n), b * (1 + 1e-6 * k / n)]
    return out


def ppf_args(n_pow, n_uni, n_one, n_edge, seed):
    p = [10.0 ** -(300.0 * (i + 0.5) / n_pow) for i in range(n_pow)]
    p += synth.uniform(seed, 0, n_uni).tolist()
    p += [1.0 - 10.0 ** -(15.9 * (i + 0.5) / n_one) for i in range(n_one)]
    for b in (0.075, 0.925, E25):
        p += around(b, n_edge)
    p += ulps(1.0 - E25, range(-n_edge, n_edge + 1))                   # 1 - p = e^-25 is a 17-bit multiple of 2^-53 there: 1e-6 of
                                                                       # it is a tenth of a step, so this boundary is walked in ulps
    p += ulps(0.5, (-1, 0, 1)) + [5e-324, 2.0 ** -1022, 1.0 - 2.0 ** -53]
    return p


PPF_EARLY = [0.0, 1.0, -0.0, -0.25, 1.0 + 2.0 ** -52, float('nan')]


def x_params(mode):
    """(5, 4): min, max, boxcox, mu, std of the four columns; mu is placed where bc - mu (modes 4, 5) or x - mu cancels at x0"""
    par = np.empty((5, 4))
    for j, ((mn, mx), lm, sd) in enumerate(zip(X_RANGES, R.LAMBDAS, X_STD)):
        x0 = mn + T0 * (mx - mn)
        if mode >= 4:
            t = (x0 - mn) / (mx - mn)
            mu = (t ** lm - 1.0) / lm
        else:
            mu, sd = x0, sd * (mx - mn)
        par[:, j] = mn, mx, lm, mu, sd
    return par


def x_args(mode, par):
    cols = []
    for j in range(4):
        mn, mx, lm, mu, sd = par[:, j]
        rng = mx - mn
        x = [mn + t * rng for t in synth.uniform(SEED + 16 + j, 0, 60).tolist()]
        x += [mn, mx] + [mn + 10.0 ** -(15.0 * (i + 0.5) / 40) * rng for i in range(40)]
        w = [10.0 ** (-12.0 + (12.0 + math.log10(15.0)) * i / 29) for i in range(30)]
        x += [mn - v * rng for v in w] + [mx + v * rng for v in w]
        for z in np.linspace(-38.0, 38.0, 41).tolist() + [-45.0, -39.0, 39.0, 45.0]:
            if mode >= 4:
                base = lm * (mu + sd * z) + 1.0
                t = math.copysign(abs(base) ** (1.0 / lm), base)
                x.append(mn + t * rng)
            else:
                x.append(mu + sd * z)
        x0 = mn + T0 * rng
        x += ulps(x0) + [x0 * (1 - 1e-13), x0 * (1 + 1e-13), x0 * (1 - 1e-12), x0 * (1 + 1e-12)]
        cols.append(x)
    return np.array(cols).T.copy()


def y_sets():
    """(mode, [min, max, boxcox, mu, std]) of the 11 sets; modes 4 and 5: u = 1/2 + x / 4 resp. 1/2 + ppf(x) / 4, zero at -2"""
    mn, mx = Y_RANGE
    sets = [(1, [mn, mx, 1.0, 0.3, 1.7]), (2, [mn, mx, 1.0, 0.3, 1.7]), (3, [mn, mx, 1.0, 0.3, 1.7])]
    for mode in (4, 5):
        for lm in R.LAMBDAS:
            sets.append((mode, [mn, mx, lm, -0.5 / lm, 0.25 / lm]))
    return sets


def y_args(mode, seed):
    x = ppf_args(40, 60, 30, 2, seed) + PPF_EARLY[:5]
    x += (-3.0 + 7.0 * synth.uniform(seed + 1, 0, 20)).tolist()
    deltas = [10.0 ** -k for k in (15, 12, 9, 6, 3, 1)] + [0.5]
    if mode == 5:
        zs = [-2.0 * (1 + s * d) for d in deltas for s in (1, -1)] + [-2.0]
        x += [0.5 * math.erfc(-z / math.sqrt(2.0)) for z in zs] + ulps(0.5 * math.erfc(2.0 / math.sqrt(2.0)), (-2, -1, 0, 1, 2))
    else:
        x += [-2.0 * (1 + s * d) for d in deltas for s in (1, -1)] + ulps(-2.0, (-1, 0, 1)) + [-5.0, -40.0, 30.0]
    return x


def std_args(seed):
    m, s = [], []
    for mm in (0.5, 0.3, 0.9, 0.02, 1e-5, 0.999, 0.075, 0.925, 0.7):
        for k in (12, 10, 8, 6, 4, 2, 1):
            m.append(mm); s.append(mm * 10.0 ** -k)
    for mm, ss in ((0.9, 0.2), (0.1, 0.3), (0.5, 0.7), (0.5, 0.5), (0.25, 0.24999999), (0.75, 0.24999999), (-2.0, 0.5), (-2.0, 1e-9)):
        m.append(mm); s.append(ss)
    n = len(m)
    gm = 4.0 * synth.uniform(seed, 0, n) - 2.0
    gs = 2.0 * synth.uniform(seed + 1, 0, n) - 1.0
    return np.array(m), np.array(s), gm, gs


def build():
    A = R.mp_arith()
    items = []
    p = np.array(ppf_args(150, 150, 100, 20, SEED) + PPF_EARLY)
    ref, allow, cls = R.model_array(R.model_ppf, A, p.tolist())
    items += [('ppf_p', p), ('ppf_ref', ref), ('ppf_allow', allow), ('ppf_cls', cls)]
    for mode in range(1, 6):
        par = x_params(mode)
        X = x_args(mode, par)
        assert X.shape[0] % 256 != 0
        items += [('x%d_par' % mode, par), ('x%d_arg' % mode, X)]
        for name, fn in (('x', R.model_scale_x), ('dx', R.model_scale_x_deriv)):
            out = [R.model_array(fn, A, X[:, j].tolist(), mode, tuple(par[:, j].tolist())) for j in range(4)]
            for k, key in enumerate(('ref', 'allow', 'cls')):
                items.append(('%s%d_%s' % (name, mode, key), np.stack([o[k] for o in out], 1)))
    sets = y_sets()
    items += [('y_mode', np.array([s[0] for s in sets], np.int8)), ('y_par', np.array([s[1] for s in sets]))]
    args = np.array([y_args(mode, SEED + 64 + 2 * i) for i, (mode, _) in enumerate(sets)])
    items.append(('y_arg', args))
    for name, fn in (('y', R.model_y_backward), ('dy', R.model_y_backward_deriv)):
        out = [R.model_array(fn, A, args[i].tolist(), mode, tuple(par)) for i, (mode, par) in enumerate(sets)]
        for k, key in enumerate(('ref', 'allow', 'cls')):
            items.append(('%s_%s' % (name, key), np.stack([o[k] for o in out], 0)))
    m, s, gm, gs = std_args(SEED + 128)
    items += [('ys_m', m), ('ys_s', s), ('yd_gm', gm), ('yd_gs', gs)]
    out = [R.model_array(R.model_y_std, A, list(zip(m.tolist(), s.tolist())), mode, tuple(par)) for mode, par in sets]
    for k, key in enumerate(('ref', 'allow', 'cls')):
        items.append(('ys_%s' % key, np.stack([o[k] for o in out], 0)))
    rows = list(zip(m.tolist(), s.tolist(), gm.tolist(), gs.tolist()))
    out = [R.model_array(R.model_y_dstd, A, rows, mode, tuple(par)) for mode, par in sets]
    for k, key in enumerate(('ref', 'allow', 'cls')):
        items.append(('yd_%s' % key, np.stack([o[k] for o in out], 0)))
    return items


if __name__ == '__main__':
    path = os.path.join(HERE, 'scaler_kats.npz')
    items = build()
    write_npz(path, items)
    d = dict(items)
    print('wrote %s: %d ppf arguments, %d x rows of 4 columns in 5 modes, %d y arguments in %d sets, %d bytes' % (
        path, len(d['ppf_p']), d['x1_arg'].shape[0], d['y_arg'].shape[1], d['y_arg'].shape[0], os.path.getsize(path)))
