"""
Known-answer vectors for the normal-tail arithmetic of scfgp_acquire and scfgp_acquire_kg (scfgp_amd/csrc/acquire_math.h, acquire.hip,
kg.hip): the 60-digit mpmath values, rounded once to float64, of

    Phi, phi, h = g Phi + phi, log h, Phi / h, phi / h, the MES term g lam / 2 - log Phi and q = (lam / 2) (1 + g (g + lam)), lam = phi / Phi

at exactly representable g: the doubles -1.0 and -50.0 (the seams of acquire_math.h::tail_r and acquire.hip::acquire_value) with their
two neighbours on either side, -38, -38.5, -39 (where phi leaves the normal range), -10^x for x = 2 .. 7, 0, 8.3 and 38.

    python tests/golden/make_acquire_kats.py        ->  tests/golden/acquire_kats.npz

Keys of the .npz: 'g' (n,), 'Phi', 'phi', 'h', 'log_h', 'Phi_over_h', 'phi_over_h', 'mes_term', 'mes_q' (n, each).  A value below the
smallest subnormal is stored as 0.0.  tests/test_acquire_range_ref.py checks that the committed file is what build() returns and
imports the functions below as its truths; the GPU tier (tests/test_gpu_acquire_range.py) reads the file and needs no mpmath.
"""
import os

import mpmath as mp
import numpy as np

DPS = 60


def Phi(x): return mp.ncdf(x)
def phi(x): return mp.npdf(x)
def h(x): return x * Phi(x) + phi(x)
def log_h(x): return mp.log(h(x))
def Phi_over_h(x): return Phi(x) / h(x)
def phi_over_h(x): return phi(x) / h(x)
def log_Phi(x): return mp.log(Phi(x)) if x < 0 else mp.log1p(-Phi(-x))       # 1 - 1e-300 needs more than 60 digits
def lam(x): return phi(x) / Phi(x)
def mes_term(x): return x * lam(x) / 2 - log_Phi(x)
def mes_q(x): return (lam(x) / 2) * (1 + x * (x + lam(x)))


FUNCS = {'Phi': Phi, 'phi': phi, 'h': h, 'log_h': log_h, 'Phi_over_h': Phi_over_h, 'phi_over_h': phi_over_h, 'mes_term': mes_term,
         'mes_q': mes_q}


def around(x, n=2):
    """the double x with its n neighbours on either side, ascending"""
    lo, hi = [x], [x]
    for _ in range(n):
        lo.append(np.nextafter(lo[-1], -np.inf)); hi.append(np.nextafter(hi[-1], np.inf))
    return np.array(lo[:0:-1] + hi)


def points():
    return np.concatenate([around(-1.0), around(-50.0), [-38.0, -38.5, -39.0], -10.0 ** np.arange(2, 8), [0.0, 8.3, 38.0]])


def build():
    g = points()
    z = {'g': g}
    with mp.workdps(DPS):
        for name, f in FUNCS.items():
            z[name] = np.array([float(f(mp.mpf(float(x)))) for x in g])
    return z


if __name__ == '__main__':
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'acquire_kats.npz')
    np.savez(path, **build())
    print('wrote', path)
