"""
GPU tier of the range tests of scfgp_predict_pd's sin / cos sites (pd.hip): fast_sincos(g_i Fall[d][j]) on grid values in
pd_mean_rows_kernel and pd_ice_weights_kernel, and fast_sincos(z - x_d f) in the context's type in pd_sums_kernel, each driven with the
phases of tests/golden/sincos_kats.npz (mpmath) through constructions in which nothing else rounds.

  grid values   the inject geometries of tests/sincos_ref.py (Fall[0][.] = 1, b = 0, s a power of two), a pool of all-zero rows,
                dims = [0], Li = I and a one-hot alpha: the zeroed-column features are (s .. s | 0 .. 0), their mean too, so the
                stacked row of grid point i is s (cos g_i | sin g_i), pd[0][i] = s cos g_i for alpha_j = 1 and s sin g_i for
                alpha_{J+j} = 1, and ice[0][t][i] the same number through the rotated weights.  Bound: 2 L s in an fp64 context (L =
                test_sincos_ref.law64, the factor 2 the contraction allowance of tests/test_gpu_phase_range.py), plus one rounding
                to float, 2^-24 s, in an fp32 context (the stored row; the stored weight).
  pool rows     the 'lds' and 'rank' kinds with the fixture's phases in column 0, dims = [1] -- a column of zeros with a zero row of
                Fall, so z0 = z exactly -- 128 rows of weight 1, one grid value 0 (rotation by exactly {1, 0}): pd is the block mean
                of s cos z_t or s sin z_t.  Bound on pd / s: the mean of the per-element bounds 2 E64 (2 E32 in an fp32 context) plus
                128 eps for the fixed summation tree over 128 terms of modulus <= 1.  One wrong quadrant in a block is 1 / 128.

There is no refusal here: a grid value is a coordinate like a row's own, and the limit |g Fall[d][j]| < 3.37e9 is the feature map's
(sincos.h; include/scfgp_hip.h states it).  Output (-s): per case the worst error over its bound.
Measured on an MI355X, worst error / bound: grid values 0.492 (fp64) and 0.500 (fp32), the same for pd and ice and for all four
geometries; pool rows 0.0012 (fp64) and 0.036 (fp32).
"""
import numpy as np
import pytest

from oracle import scfgp_oracle as O
from tests import sincos_ref as S
from tests.test_sincos_ref import E32, E64, law64

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
L = float(law64(0.0))
HARD = ('npio2', 'flip', 'tie', 'special', 'quadrant')
_KATS = {}


def kats():
    if not _KATS:
        k = S.load_kats()
        k['g'] = np.concatenate((k['z'], k['zb'])); k['gs'] = np.concatenate((k['sin'], k['sinb'])); k['gc'] = np.concatenate((k['cos'], k['cosb']))
        for key in ('g', 'gs', 'gc'):
            k[key].setflags(write=False)
        _KATS.update(k)
    return _KATS


def _engine(D, S_, M, params, dtype):
    from scfgp_amd.engine import HipEngine
    eng = HipEngine(D, S_, M, dtype=dtype); eng.set_params(params)
    d = eng.dims()
    assert np.array_equal(eng.debug_read('Fall', (d['Dp'], d['Jp'])), S.inject_expected(D, S_, M, d['Dp'], d['Jp']))
    return eng


def one_hot(K, k):
    a = np.zeros(K); a[k] = 1.0
    return a


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('kind', sorted(S.INJECT_KINDS))
def test_grid_values_through_the_mean_rows_and_the_ice_weights(kind, dtype):
    """every phase of the fixture, both blocks (|g| up to 1e9), as a grid value, 1024 per call; pd and ice against mpmath"""
    k = kats()
    g, gs, gc = k['g'], k['gs'], k['gc']
    D, S_, M, params, _ = S.inject(kind, np.zeros(1))
    J = S_ + M; K = 2 * J
    s = float(np.sqrt(2.0 / M))
    T = 2
    Xs = np.zeros((T, D))
    # the terms that must vanish, on the CPU: the zeroed-column features are (s .. s | 0 .. 0), so with a one-hot alpha a single product
    # s * cos g or s * sin g is left in pd and in ice, and its partner is multiplied by an exact zero
    Phi0 = O.feature_map(Xs, params, D, S_, M)
    assert s in (0.5, 0.25, 0.125) and np.all(Phi0[:, :J] == s) and np.all(Phi0[:, J:] == 0.0)
    eng = _engine(D, S_, M, params, dtype)
    bound = 2 * L * s + (2.0 ** -24 * s if dtype == 'f32' else 0.0)
    j = J - 1
    worst = {}
    for half, truth in ((0, gc), (1, gs)):
        alpha = one_hot(K, half * J + j)
        for i in range(0, len(g), 1024):
            gi = g[i:i + 1024]
            out = eng.predict_pd(Xs, alpha, np.eye(K), [0], gi[None, :], want=('pd', 'ice'))
            ref = s * truth[i:i + 1024]
            e_pd = S.abs_err(out['pd'][0], ref)
            e_ice = S.abs_err(out['ice'][0], ref[None, :]).max(0)
            assert np.array_equal(out['ice'][0][0], out['ice'][0][1])
            for name, e in (('pd', e_pd), ('ice', e_ice)):
                key = '%s %s' % (name, 'sin' if half else 'cos')
                if e.max() / bound > worst.get(key, (0.0, 0.0))[0]:
                    worst[key] = (float(e.max() / bound), float(gi[e.argmax()]))
    eng.close()
    msg = 'pd_range grid %-8s %s: %d grid values, worst / bound %s' % (
        kind, dtype, len(g), ' '.join('%s=%.4f (g = %r)' % (n, v[0], v[1]) for n, v in sorted(worst.items())))
    print('\n' + msg)
    assert all(v[0] <= 1 for v in worst.values()), msg


def blocks():
    """twelve blocks of 128 phases: the hard groups of the fixture's in-domain block strided into nine, three from the block beyond"""
    k = kats()
    hard = np.flatnonzero(np.isin(k['group'], [k['groups'].index(n) for n in HARD]))
    out = []
    sel = hard[np.unique(np.rint(np.linspace(0, len(hard) - 1, 9 * 128)).astype(np.int64))]      # 1152 of them, evenly over the groups
    for b in range(9):
        idx = sel[b::9]
        assert len(idx) == 128
        out.append((k['z'][idx], k['sin'][idx], k['cos'][idx], set(k['group'][idx].tolist())))
    for b in range(3):
        idx = np.arange(len(k['zb']))[b::3][:128]
        out.append((k['zb'][idx], k['sinb'][idx], k['cosb'][idx], set()))
    seen = set().union(*[o[3] for o in out])
    assert seen == {k['groups'].index(n) for n in HARD} and len(out) == 12
    return out


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('kind', ['lds', 'rank'])
def test_pool_rows_through_the_sums(kind, dtype):
    k = kats()
    D, S_, M = S.INJECT_KINDS[kind]
    J = S_ + M; K = 2 * J
    s = float(np.sqrt(2.0 / M))
    E = E64 if dtype == 'f64' else E32
    bound = 2 * E + 128 * EPS                                    # on pd / s: the mean of 128 equal per-element bounds, and the tree
    eng = None
    worst = (0.0, None)
    for b, (z, sn, cs, _) in enumerate(blocks()):
        D_, S2, M_, params, X = S.inject(kind, z)
        assert np.all(X[:, 1] == 0) and len(z) == 128
        if eng is None:
            eng = _engine(D, S_, M, params, dtype)
        ld = np.longdouble
        for half, truth in ((0, cs), (1, sn)):
            out = eng.predict_pd(X, one_hot(K, half * J + (J - 1)), np.eye(K), [1], np.zeros((1, 1)), want=('pd',))
            e = float(abs(ld(out['pd'][0, 0]) / ld(s) - truth.sum() / ld(128)))
            if e / bound > worst[0]:
                worst = (e / bound, (b, 'sin' if half else 'cos'))
    eng.close()
    msg = 'pd_range sums %-5s %s: 12 blocks of 128 rows, worst / bound = %.4f at block %s' % (kind, dtype, worst[0], worst[1])
    print('\n' + msg)
    assert worst[0] <= 1, msg
