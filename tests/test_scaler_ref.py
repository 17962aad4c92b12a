"""
CPU tier of the range tests of the scaler transforms (tests/scaler_ref.py, tests/golden/scaler_kats.npz): the numpy restatement of
the six device functions against the mpmath reference of the fixture under the allowance of the error model, what the fixture has
to cover, the mutations that the fixture has to catch, and the host transforms of scfgp_amd/scaler.py under the same allowance.
The GPU tier (tests/test_gpu_scaler_range.py) compares the compiled kernels with the same fixture and the same restatement.
Output (-s): per function the worst error over its allowance.
"""
import numpy as np
import pytest

from tests import scaler_ref as R

kats = R.kats
X_MODES = R.X_MODES


def blocks(mut=None, coef=R.COEF):
    """(function, block, restated results, reference, allowance, class) over the whole fixture"""
    k = kats()
    yield 'norm_ppf', 'ppf', R.ppf(k['ppf_p'], coef, mut), k['ppf_ref'], k['ppf_allow'], k['ppf_cls']
    for m in X_MODES:
        par, X = k['x%d_par' % m], k['x%d_arg' % m]
        yield 'scale_x', 'mode %d' % m, R.scale_x(X, m, par, mut), k['x%d_ref' % m], k['x%d_allow' % m], k['x%d_cls' % m]
        yield ('scale_x_deriv', 'mode %d' % m, R.scale_x_deriv(X, m, par, mut), k['dx%d_ref' % m], k['dx%d_allow' % m],
               k['dx%d_cls' % m])
    for i, (m, par) in enumerate(zip(k['y_mode'].tolist(), k['y_par'])):
        tag = 'set %d (mode %d, lm %.4g)' % (i, m, par[2])
        yield 'y_backward', tag, R.y_backward(k['y_arg'][i], m, par, mut, coef), k['y_ref'][i], k['y_allow'][i], k['y_cls'][i]
        yield ('y_backward_deriv', tag, R.y_backward_deriv(k['y_arg'][i], m, par, mut, coef), k['dy_ref'][i], k['dy_allow'][i],
               k['dy_cls'][i])
        yield 'std', tag, R.y_std(k['ys_m'], k['ys_s'], m, par, mut), k['ys_ref'][i], k['ys_allow'][i], k['ys_cls'][i]
        yield ('dstd', tag, R.y_dstd(k['ys_m'], k['ys_s'], k['yd_gm'], k['yd_gs'], m, par, mut), k['yd_ref'][i], k['yd_allow'][i],
               k['yd_cls'][i])


FUNCTIONS = ('norm_ppf', 'scale_x', 'scale_x_deriv', 'y_backward', 'y_backward_deriv', 'std', 'dstd')


def broken(mut=None, coef=R.COEF, only=None):
    """the (function, block, count) in which a mutated restatement leaves the allowance or the class"""
    out = []
    for fn, tag, got, ref, allow, cls in blocks(mut, coef):
        if only is None or fn in only:
            ok, _ = R.judge(got, ref, allow, cls)
            if not ok.all():
                out.append((fn, tag, int((~ok).sum())))
    return out


@pytest.mark.parametrize('function', FUNCTIONS)
def test_restatement_meets_the_allowance(function):
    """Every argument of the fixture: the restatement within the model's allowance of the mpmath value, or in its class."""
    worst, n = 0.0, 0
    for fn, tag, got, ref, allow, cls in blocks():
        if fn != function:
            continue
        ok, ratio = R.judge(got, ref, allow, cls)
        bad = np.argwhere(~ok)
        assert ok.all(), '%s %s: %d of %d outside, first at %s: got %r, reference %r, allowance %r, class %s' % (
            fn, tag, len(bad), ok.size, tuple(bad[0]), np.asarray(got)[tuple(bad[0])], ref[tuple(bad[0])], allow[tuple(bad[0])],
            R.CLASS_NAMES[cls[tuple(bad[0])]])
        worst = max(worst, float(ratio.max())); n += ok.size
    print('\nscaler_ref %-16s %5d arguments, worst error / allowance = %.3f' % (function, n, worst))
    assert n > 0 and worst <= 1


def test_fixture_is_reproducible():
    """The generator writes the committed fixture again, bit for bit."""
    pytest.importorskip('mpmath')
    from tests.golden import make_scaler_kats as G
    k = kats()
    items = G.build()
    assert sorted(n for n, _ in items) == sorted(k)
    for name, arr in items:
        a = np.ascontiguousarray(arr)
        assert a.dtype == k[name].dtype and a.shape == k[name].shape and a.tobytes() == k[name].tobytes(), name


def test_fixture_covers_the_ppf_branches_and_boundaries():
    k = kats()
    p = k['ppf_p']
    br = R.ppf_branch(p)
    for b in (0, 1, 2):
        assert (br == b).sum() >= 20, (b, int((br == b).sum()))
    near = lambda c: np.abs(p - c) <= 1.5e-6 * c
    for c, inner, outer in ((0.075, 1, 0), (0.925, 1, 0), (np.exp(-25.0), 2, 1), (1 - np.exp(-25.0), 2, 1)):
        # one side of the boundary is the branch `inner`, the other side `outer`: 20 arguments within 1e-6 on each
        m = near(c) if c < 0.9999 else np.abs((1 - p) - np.exp(-25.0)) <= 21 * 2.0 ** -53
        assert (br[m] == inner).sum() >= 20 and (br[m] == outer).sum() >= 20, (c, np.bincount(br[m] + 1))
    for v in (0.5, np.nextafter(0.5, 0), np.nextafter(0.5, 1), 5e-324, 2.0 ** -1022, 1 - 2.0 ** -53, 1.0, 1 + 2.0 ** -52):
        assert (p == v).any(), v
    assert ((p == 0) & ~np.signbit(p)).any() and ((p == 0) & np.signbit(p)).any() and (p < 0).any() and np.isnan(p).any()
    assert p[(p > 0) & (p < 1)].min() == 5e-324 and (p < np.exp(-25.0)).sum() >= 100


def test_fixture_covers_every_class_and_leaves_little_out():
    seen = np.zeros(len(R.CLASS_NAMES), int)
    total = dict.fromkeys(FUNCTIONS, 0); out = dict.fromkeys(FUNCTIONS, 0)
    for fn, tag, got, ref, allow, cls in blocks():
        seen += np.bincount(cls.ravel(), minlength=len(R.CLASS_NAMES))
        total[fn] += cls.size
        out[fn] += int(np.isin(cls, R.LEFT_OUT).sum())
        assert np.all(np.isfinite(allow[np.isin(cls, (R.VALUE, R.SUB))]))
    assert np.all(seen > 0), dict(zip(R.CLASS_NAMES, seen.tolist()))
    for fn in FUNCTIONS:
        # subnormal, any-non-finite and unbounded (beside u = 0): at most 1 % of a function's arguments
        assert out[fn] <= 0.01 * total[fn], (fn, out[fn], total[fn])
    assert all(2000 <= total[fn] <= 5000 for fn in FUNCTIONS[1:5]) and total['norm_ppf'] >= 500, total


def test_fixture_covers_t_and_u_on_both_sides():
    k = kats()
    for m in X_MODES:
        par, X = k['x%d_par' % m], k['x%d_arg' % m]
        assert np.array_equal(par[2], R.LAMBDAS)
        t = (X - par[0]) / (par[1] - par[0])
        for j in range(4):                                             # every mode x exponent pair
            tj = t[:, j]
            assert (tj < 0).sum() >= 20 and (tj == 0).sum() >= 1 and ((tj > 0) & (tj < 1)).sum() >= 60 and (tj > 1).sum() >= 20
            assert (tj == 1).any() and tj.min() <= -14 and tj.max() >= 15
        if m in (3, 5):                                                # the erfc argument out to the deep tails and past them
            z = R.scale_x(X, 4 if m == 5 else 2, par)
            assert (np.abs(z) >= 37.5).sum() >= 8 and (np.abs(z) > 38.6).sum() >= 8
        if m >= 4:                                                     # bc - mu cancelling to within 1e-12
            mn, mx, lm, mu, sd = par
            bc = (np.sign(t) * np.abs(t) ** lm - 1) / lm
            assert np.all(((np.abs(bc - mu) <= 1e-12 * np.abs(mu)).sum(0)) >= 5)
    lams = set()
    for i, (m, par) in enumerate(zip(k['y_mode'].tolist(), k['y_par'])):
        if m < 4:
            continue
        lams.add((m, par[2]))
        x = k['y_arg'][i]
        with np.errstate(all='ignore'):
            u = (x * par[4] + par[3] if m == 4 else R.ppf(x) * par[4] + par[3]) * par[2] + 1.0
        assert (u < 0).sum() >= 5 and (u > 0).sum() >= 100 and (np.abs(u) <= 1e-12).sum() >= 2, (i, m)
        if par[2] == 1.0 and m == 4:
            assert (u == 0).any()
    assert lams == {(m, lm) for m in (4, 5) for lm in R.LAMBDAS}
    # the std band: inside (0, 1), out on one side, out on both
    a, b = k['ys_m'] + k['ys_s'], k['ys_m'] - k['ys_s']
    inside = lambda v: (v > 0) & (v < 1)
    assert (inside(a) & inside(b)).sum() >= 30 and (inside(a) ^ inside(b)).sum() >= 2 and (~inside(a) & ~inside(b)).sum() >= 2
    assert (k['ys_s'] <= 1e-12 * np.abs(k['ys_m'])).any()


@pytest.mark.parametrize('i', range(48))
def test_every_as241_coefficient_is_pinned(i):
    """One unit in the 6th significant digit of any of the 48 coefficients leaves the allowance somewhere in the ppf's block."""
    assert len(R.EXEMPT) <= 6
    if i in [e[0] for e in R.EXEMPT]:
        idx, change, smallest = [e for e in R.EXEMPT if e[0] == i][0]
        assert change < smallest
        return
    assert R.mutated_coef(i).flat[i] != R.COEF.flat[i] and (R.mutated_coef(i) != R.COEF).sum() == 1
    assert broken(coef=R.mutated_coef(i), only=('norm_ppf',)), 'coefficient %d moves nothing past the allowance' % i


# mutation -> the functions in which it has to show
MUTATION_SHOWS = {
    'swap_tail': ('norm_ppf', 'y_backward'), 'no_tail_sign': ('norm_ppf', 'y_backward'),
    'no_sign_bc': ('scale_x', 'scale_x_deriv'), 'no_sign_ibc': ('y_backward', 'std'),
    'pow_lm': ('scale_x_deriv',), 'inv_lm': ('y_backward_deriv', 'dstd'), 'mode3_algebraic': ('y_backward', 'std'),
    'no_range_x': ('scale_x_deriv',), 'no_range_y': ('y_backward_deriv', 'dstd'), 'one_sided': ('std',),
}


@pytest.mark.parametrize('mut', R.MUTATIONS)
def test_mutation_is_caught(mut):
    assert set(MUTATION_SHOWS) == set(R.MUTATIONS)
    hit = broken(mut=mut)
    fns = {h[0] for h in hit}
    print('\nscaler_ref mutation %-16s breaks %s' % (mut, sorted(fns)))
    for fn in MUTATION_SHOWS[mut]:
        assert fn in fns, (mut, fn, hit)
    if mut in ('pow_lm', 'inv_lm'):                                    # the exponent off by one: in both Box-Cox modes, every exponent
        fn = MUTATION_SHOWS[mut][0]
        assert len([h for h in hit if h[0] == fn]) == (2 if mut == 'pow_lm' else 8), hit


def test_host_scaler_meets_the_same_allowance():
    """scfgp_amd/scaler.py, the path the facade takes when the device scalers are off: forward_transform on the scale_x blocks and
    backward_transform on the y_backward blocks, under the fixture's allowances and classes."""
    k = kats()
    worst = {}
    with np.errstate(all='ignore'):
        for m in X_MODES:
            s = R.host_scaler(m, k['x%d_par' % m])
            ok, ratio = R.judge(s.forward_transform(k['x%d_arg' % m]), k['x%d_ref' % m], k['x%d_allow' % m], k['x%d_cls' % m])
            bad = np.argwhere(~ok)
            assert ok.all(), ('forward', m, len(bad), bad[:4].tolist(), k['x%d_arg' % m][tuple(bad[0])])
            worst['forward %d' % m] = float(ratio.max())
        for i, (m, par) in enumerate(zip(k['y_mode'].tolist(), k['y_par'])):
            s = R.host_scaler(m, par)
            got = s.backward_transform(k['y_arg'][i][:, None])[:, 0]
            ok, ratio = R.judge(got, k['y_ref'][i], k['y_allow'][i], k['y_cls'][i])
            bad = np.flatnonzero(~ok)
            assert ok.all(), ('backward', i, m, len(bad), k['y_arg'][i][bad[:4]], got[bad[:4]], k['y_ref'][i][bad[:4]])
            worst['backward %d/%d' % (m, i)] = float(ratio.max())
    print('\nscaler_ref host scaler, worst error / allowance: %s' % ', '.join('%s %.3f' % kv for kv in sorted(worst.items())))


# ---- the steering of the GPU tier's y-scaler tests, checked here where mpmath and a GPU are not needed ----------------------------
PPF_SETS = [i for i, m in enumerate(R.load_kats()['y_mode'].tolist()) if m in (3, 5)]


def test_longdouble_restatement_is_the_same_function():
    """The GPU tier's reference for arguments that exist only on the device: the restatement in np.longdouble, against the fixture
    under the same allowance (its own rounding is 2^-11 of fp64's; what is left is the method error of AS 241)."""
    assert np.finfo(np.longdouble).nmant >= 63
    k = kats()
    worst = 0.0
    for i, (m, par) in enumerate(zip(k['y_mode'].tolist(), k['y_par'])):
        x = k['y_arg'][i].astype(np.longdouble)
        for got, key in ((R.y_backward(x, m, R.ld(par)), 'y'), (R.y_backward_deriv(x, m, R.ld(par)), 'dy')):
            assert got.dtype == np.longdouble
            with np.errstate(over='ignore'):
                got = got.astype(np.float64)
            ok, ratio = R.judge(got, k[key + '_ref'][i], k[key + '_allow'][i], k[key + '_cls'][i])
            assert ok.all(), (i, m, key, int((~ok).sum()))
            worst = max(worst, float(ratio.max()))
    print('\nscaler_ref longdouble restatement, worst error / allowance = %.3f' % worst)


@pytest.mark.parametrize('i', range(11))
def test_steering_keeps_the_rows_finite(i):
    """at least 90 % of the rows finite on the reference side, per quantity: mu_y in every step, std_y where the band stays inside"""
    mode, par, X, a_const, a_ramp = R.steering(i)
    for name, m, sg, band in R.steering_means(i):
        with np.errstate(all='ignore'):
            assert np.isfinite(R.y_backward(m, mode, par)).mean() >= 0.9, (i, mode, name)
            if band:
                assert np.isfinite(R.y_std(m, sg, mode, par)).mean() >= 0.9, (i, mode, name)


@pytest.mark.parametrize('i', PPF_SETS)
def test_steering_reaches_every_ppf_branch_and_boundary(i):
    p = np.concatenate([m for _, m, _, _ in R.steering_means(i)])
    br = R.ppf_branch(p)
    assert np.all(br >= 0)
    for lower in (True, False):                                        # each branch on each side of 1/2, so each side of every boundary
        side = (p < 0.5) == lower
        for b in (0, 1, 2):
            assert (side & (br == b)).sum() >= 20, (i, lower, b, int((side & (br == b)).sum()))
    assert p.min() < 1e-300 and (1 - p).min() < 1e-11


@pytest.mark.parametrize('c', range(48))
def test_steering_pins_every_as241_coefficient(c):
    """Each mutated table replayed as the device at the steering arguments of the inv-normal set: outside the GPU tier's bound (the
    model's allowance, once, around the longdouble restatement) somewhere."""
    i = PPF_SETS[0]
    mode, par, X, a_const, a_ramp = R.steering(i)
    assert mode == 3
    caught = 0
    for name, m, sg, band in R.steering_means(i):
        key = ('pin', i, name)
        if key not in R._STEER:
            with np.errstate(all='ignore'):
                ref = R.y_backward(m.astype(np.longdouble), mode, R.ld(par))
                R._STEER[key] = (ref,) + R.fl_model(R.model_y_backward, m.tolist(), mode, par)
        ref, allow, cls = R._STEER[key]
        with np.errstate(all='ignore'):
            ok, _ = R.judge(R.y_backward(m, mode, par, coef=R.mutated_coef(c)), ref, allow, cls)
        caught += int((~ok).sum())
    assert caught > 0, 'coefficient %d moves nothing past the bound at the steering arguments' % c
