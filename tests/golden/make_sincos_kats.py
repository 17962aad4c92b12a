"""
Known-answer vectors for the feature map's sin / cos (csrc/sincos.h): hard arguments of the reduction by pi/2 and their sin / cos
from mpmath at 200 bits, each stored as a (hi, lo) pair of doubles (hi the nearest double, lo the nearest double to the rest:
about 106 bits).  The tests read the fixture; only this maker needs mpmath.

    python tests/golden/make_sincos_kats.py        ->  tests/golden/sincos_kats.npz

Two blocks.  In-domain ('z', 'sin', 'cos'; 'group' indexes 'groups'), every point with |fn| = |rint(z 2/pi)| < 2^20:
  npio2     the nearest double to n pi/2 and both its neighbours, |n| log-uniform up to 2^20 - 1, both signs
  flip      the doubles at and either side of (2k + 1) pi/4, where rint changes quadrant
  tie       doubles whose fp64 product z * (2/pi) is exactly k + 1/2 (rint rounds a tie to even), k of both parities and signs
  special   +-0, +- the smallest denormal, +-2^-30, +-pi/4
  quadrant  points inside each quadrant at |fn| in {1, 2, 3, 2^20 - 4 .. 2^20 - 1}, both signs
  filler    uniform draws per decade from 1 to 1.6e6, random signs
Beyond ('zb', 'sinb', 'cosb'): uniform draws and near-multiples of pi/2 at magnitudes 1e7, 1e8 and 1e9, all with |fn| < 2^31.

The draws come from scfgp_amd.synth.uniform (a pure function of seed and index) and the archive is written with fixed member
dates and no compression, so a second run reproduces the file bit for bit.
"""
import io
import os
import sys
import zipfile
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from scfgp_amd import synth                                    # noqa: E402

GROUPS = ('npio2', 'flip', 'tie', 'special', 'quadrant', 'filler')
TWO_OVER_PI = 6.36619772367581382433e-01
SEED = 0x51C05000


def to_double(v):
    """nearest double to an mpf, through exact rational arithmetic"""
    from mpmath import libmp
    p, q = libmp.to_rational(v._mpf_)
    return float(Fraction(p, q))


def neighbours(x):
    return [np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)]


def log_ints(lo, hi, count):
    """about `count` distinct integers spread log-uniformly over [lo, hi], both ends included"""
    v = np.unique(np.rint(np.exp(np.linspace(np.log(lo), np.log(hi), count))).astype(np.int64))
    return [int(k) for k in v]


def in_domain(mp):
    hp = mp.pi / 2
    pts = []                                                   # (group, z)
    for n in log_ints(1, 2 ** 20 - 1, 200):
        for sg in (1, -1):
            pts += [('npio2', z) for z in neighbours(to_double(sg * n * hp))]
    for k in log_ints(1, 2 ** 20 - 2, 100) + [0]:
        for sg in (1, -1):
            pts += [('flip', z) for z in neighbours(to_double(sg * (2 * k + 1) * mp.pi / 4))]
    for k in log_ints(1, 2 ** 20 - 3, 120) + log_ints(2, 2 ** 20 - 4, 77) + [0]:
        for sg in (1, -1):
            half = sg * (k + 0.5)
            z0 = to_double(mp.mpf(half) * hp)
            cand = [z0]
            for _ in range(3):
                cand = [np.nextafter(cand[0], -np.inf)] + cand + [np.nextafter(cand[-1], np.inf)]
            pts += [('tie', z) for z in cand if z * TWO_OVER_PI == half]
    for v in (0.0, 5e-324, 2.0 ** -30, to_double(mp.pi / 4)):
        pts += [('special', v), ('special', -v)]
    for n in (1, 2, 3, 2 ** 20 - 4, 2 ** 20 - 3, 2 ** 20 - 2, 2 ** 20 - 1):
        for sg in (1, -1):
            for d in (-0.75, -0.4, -0.1, 0.1, 0.4, 0.75):
                pts.append(('quadrant', to_double(sg * (n * hp + d))))
    edges = [1.0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1.6e6]
    for i in range(len(edges) - 1):
        u = synth.uniform(SEED + i, 0, 150); sg = np.where(synth.uniform(SEED + 64 + i, 0, 150) < 0.5, -1.0, 1.0)
        pts += [('filler', float(z)) for z in sg * (edges[i] + (edges[i + 1] - edges[i]) * u)]
    seen, out = set(), []
    for g, z in pts:                                           # first occurrence wins; +0 and -0 are different points
        key = np.float64(z).tobytes()
        if key not in seen:
            seen.add(key); out.append((g, float(z)))
    z = np.array([p[1] for p in out])
    fn = np.rint(z * TWO_OVER_PI)
    assert np.all(np.abs(fn) < 2 ** 20), np.abs(fn).max()
    group = np.array([GROUPS.index(p[0]) for p in out], dtype=np.int8)
    return z, group


def beyond(mp):
    hp = mp.pi / 2
    z = []
    for i, mag in enumerate((1e7, 1e8, 1e9)):
        u = synth.uniform(SEED + 128 + i, 0, 200); sg = np.where(synth.uniform(SEED + 160 + i, 0, 200) < 0.5, -1.0, 1.0)
        z += [float(v) for v in sg * mag * (0.5 + 0.5 * u)]
        for n in log_ints(int(0.32 * mag), int(0.63 * mag), 12):
            for sg1 in (1, -1):
                z += neighbours(to_double(sg1 * n * hp))
    z = np.array(z)
    fn = np.rint(z * TWO_OVER_PI)
    assert np.all((np.abs(fn) >= 2 ** 20) & (np.abs(fn) < 2 ** 31))
    return z


def pairs(mp, f, z):
    out = np.empty((len(z), 2))
    for i, v in enumerate(z.tolist()):
        t = f(mp.mpf(v))
        hi = to_double(t)
        out[i] = hi, to_double(t - mp.mpf(hi))
    return out


def build():
    import mpmath as mp
    mp.mp.prec = 200
    z, group = in_domain(mp)
    assert len(z) % 128 != 0, 'the GPU tier wants a row count that is no multiple of the 128-row block'
    zb = beyond(mp)
    return [('z', z), ('group', group), ('groups', np.array(GROUPS)), ('sin', pairs(mp, mp.sin, z)), ('cos', pairs(mp, mp.cos, z)),
            ('zb', zb), ('sinb', pairs(mp, mp.sin, zb)), ('cosb', pairs(mp, mp.cos, zb))]


def write_npz(path, items):
    """an .npz np.load reads, with nothing in it that depends on when it was written"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_STORED) as zf:
        for name, arr in items:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arr), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


if __name__ == '__main__':
    path = os.path.join(HERE, 'sincos_kats.npz')
    items = build()
    write_npz(path, items)
    print('wrote %s: %d in-domain points, %d beyond, %d bytes' % (path, len(items[0][1]), len(items[5][1]), os.path.getsize(path)))
