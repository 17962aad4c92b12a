"""
GPU tier of the range tests of the scaler transforms: the compiled scale_x, scale_x_deriv (csrc/fmap.hip), pd_scale_x (csrc/pd.hip),
norm_ppf, y_backward (csrc/yscale.h) and y_backward_deriv (csrc/kernels_params.hip) element by element, through the entry points that
run them, against tests/golden/scaler_kats.npz (mpmath) and the restatement of tests/scaler_ref.py, under the allowance of its error
model.  No mpmath is needed here.

  scale_x           predict_raw on the fixture's argument matrix, then debug_read("pXt"): every element against the fixture
  scale_x_deriv     predict_grad mode 1 on the raw arguments against mode 0 on the "pXt" bits times the fixture's derivative
  pd_scale_x        predict_pd in raw mode with the arguments as grid values against scaled mode on the "pXt" bits
  y_backward        predict_y, sample mode 2 and sample_grad mode 2 against the restatement at the device's own scaled outputs
  y_backward_deriv  predict_grad mode 2 against the restatement of ygrad_kernel at mode 1's outputs
  seam              D = 17, T = 32768 + 257: two chunks and a grid-stride pass of xgrad_kernel / ygrad_kernel, bit-equal to T = 257

Where the arguments are the device's own bits the reference is the restatement evaluated in np.longdouble (its own roundings are
2^-11 of fp64's; tests/test_scaler_ref.py holds it to the fixture) and the bound is the model's allowance at those bits, once.  The
steering of the y-scaler tests (tests/scaler_ref.py: STEER_STEPS) takes the scaled mean through all three branches of norm_ppf on
both sides of 1/2, down to 1e-300 and up to 1 - 2e-12; tests/test_scaler_ref.py asserts that, and that every mutated AS 241 table
replayed as the device is caught at those arguments.  Output (-s): per case the worst error over its bound.

Worst error / bound observed on an MI355X, for the record (it decides nothing):
  scale_x 0.682 (mode 3), scale_x_deriv 0.673 (mode 3), pd_scale_x 0 (the curves were bit-equal in all five modes),
  y_backward 0.417, std 0.833, y_backward_deriv 0.459, dstd 0.556; the seam case was bit-equal in every row.
"""
import ctypes as C

import numpy as np
import pytest

from scfgp_amd import synth
from tests import scaler_ref as R

pytestmark = pytest.mark.gpu

D, S, M = 4, 2, 4
K = 2 * (S + M)
X_MODES = R.X_MODES
kats = R.kats
_CACHE = {}


def factors(K=K, seed=0x5CA1E):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(K) / np.sqrt(K), np.tril(rng.standard_normal((K, K))) / np.sqrt(K)


def engine(dtype='f64', c=-1.0, D=D):
    from scfgp_amd.engine import HipEngine
    eng = HipEngine(D, S, M, dtype=dtype)
    eng.nonfinite = 'return'
    eng.set_params(synth.make_params(0x5CA1E202, D, S, M, abc=(-1.0, 0.0, c)))
    return eng


def packed(mode, dtype='f64'):
    """predict_raw on the fixture's arguments of one mode, then "pXt": the padded chunk and the geometry; computed once per (mode,
    dtype) and left unchanged"""
    key = (mode, dtype)
    if key not in _CACHE:
        k = kats()
        X, par = k['x%d_arg' % mode], k['x%d_par' % mode]
        alpha, Li = factors()
        eng = engine(dtype)
        try:
            eng.set_x_scaler(R.host_scaler(mode, par))
            buf = np.empty(8)
            assert eng.lib.scfgp_debug_read(eng.ctx, b'pXt', buf.ctypes.data_as(C.c_void_p), buf.nbytes) == -1   # before any call
            eng.predict_raw(X, alpha, Li)
            Dp = eng.dims()['Dp']
            rows = -(-X.shape[0] // 256) * 256
            big = np.full((rows + 256) * Dp, -7.0)
            n = eng.lib.scfgp_debug_read(eng.ctx, b'pXt', big.ctypes.data_as(C.c_void_p), big.nbytes)
            assert n == 8 * rows * Dp and np.all(big[rows * Dp:] == -7.0), (n, rows, Dp)
            P = big[:rows * Dp].reshape(rows, Dp).copy()
            assert np.array_equal(P, eng.debug_read('pXt', (rows, Dp)), equal_nan=True)
        finally:
            eng.close()
        P.setflags(write=False)
        _CACHE[key] = P
    return _CACHE[key]


def report(name, ok, ratio, extra=''):
    msg = 'scaler_range %-34s worst error / bound = %.3f over %d values%s' % (name, float(ratio.max()), ok.size, extra)
    print('\n' + msg)
    return msg


@pytest.mark.parametrize('mode', X_MODES)
def test_scale_x_against_the_fixture(mode):
    """Every element of the packed chunk within the fixture's allowance of the mpmath value, or in its class; ones in column D, zeros in
    the padding; the same bits from an fp32 context (the transform is fp64 in every compute mode)."""
    k = kats()
    X = k['x%d_arg' % mode]
    T = X.shape[0]
    P = packed(mode)
    assert T % 256 != 0 and P.shape[0] > T
    assert np.all(P[:T, D] == 1.0) and np.all(P[:T, D + 1:] == 0.0) and np.all(P[T:] == 0.0)
    ok, ratio = R.judge(P[:T, :D], k['x%d_ref' % mode], k['x%d_allow' % mode], k['x%d_cls' % mode])
    bad = np.argwhere(~ok)
    msg = report('scale_x mode %d' % mode, ok, ratio)
    assert ok.all(), '%s; %d outside, first at %s: x = %r, got %r, reference %r' % (
        msg, len(bad), tuple(bad[0]), X[tuple(bad[0])], P[tuple(bad[0])], k['x%d_ref' % mode][tuple(bad[0])])
    P32 = packed(mode, 'f32')
    assert P32.shape == P.shape and P32.tobytes() == P.tobytes()


def _expected_product(g, ref, allow, cls):
    """reference, allowance and class of g * f for a factor f given by (ref, allow, cls) and an fp64 number g that is exact"""
    with np.errstate(all='ignore'):
        special = np.select([cls == R.ZERO, cls == R.PINF, cls == R.NINF, cls == R.NAN], [0.0, np.inf, -np.inf, np.nan], 1.0)
        ld = np.longdouble
        prod = np.where(np.isin(cls, (R.VALUE, R.SUB)), g.astype(ld) * np.asarray(ref, ld), (g * special).astype(ld))
        pcls = np.where(np.isin(cls, (R.VALUE, R.SUB)), R.VALUE, cls).astype(np.int8)
        pcls = np.where(np.isnan(prod) & (pcls != R.ANYNF), R.NAN, pcls)
        pcls = np.where(np.isposinf(prod) & (pcls != R.ANYNF), R.PINF, pcls)
        pcls = np.where(np.isneginf(prod) & (pcls != R.ANYNF), R.NINF, pcls)
        pcls = np.where((prod == 0) & (pcls != R.ANYNF), R.ZERO, pcls)
        # the factor's allowance scaled by |g| and the product's own rounding: half an ulp, in the subnormal range a step (half a step
        # is no fp64 number); the reference product is formed in longdouble
        pallow = np.abs(g) * np.where(np.isfinite(allow), allow, 0.0) + np.maximum(R.U * np.abs(prod).astype(np.float64), R.STEP)
    return prod, pallow, pcls


@pytest.mark.parametrize('mode', X_MODES)
def test_scale_x_deriv_against_the_fixture(mode):
    """predict_grad in raw inputs = predict_grad at the packed bits, times the fixture's derivative of the X scaler: dmu and dstd within
    |gradient| * allowance + the product's half ulp, mu and sigma bit-equal."""
    k = kats()
    X, par = k['x%d_arg' % mode], k['x%d_par' % mode]
    T = X.shape[0]
    Xs = np.ascontiguousarray(packed(mode)[:T, :D])
    alpha, Li = factors()
    eng = engine()
    try:
        eng.set_x_scaler(R.host_scaler(mode, par))
        mu0, sd0, dmu0, dsd0 = eng.predict_grad(Xs, alpha, Li, mode='scaled')
        mu1, sd1, dmu1, dsd1 = eng.predict_grad(X, alpha, Li, mode='raw')
    finally:
        eng.close()
    assert mu1.tobytes() == mu0.tobytes() and sd1.tobytes() == sd0.tobytes()
    assert np.all(np.isfinite(dmu0)) and np.all(np.isfinite(dsd0)) and np.abs(dsd0).max() > 0
    ref, allow, cls = k['dx%d_ref' % mode], k['dx%d_allow' % mode], k['dx%d_cls' % mode]
    for name, g0, g1 in (('dmu', dmu0, dmu1), ('dstd', dsd0, dsd1)):
        prod, pallow, pcls = _expected_product(g0, ref, allow, cls)
        ok, ratio = R.judge(g1, prod, pallow, pcls)
        bad = np.argwhere(~ok)
        msg = report('scale_x_deriv mode %d %s' % (mode, name), ok, ratio)
        assert ok.all(), '%s; %d outside, first at %s: x = %r, got %r, expected %r (class %s), scaled gradient %r' % (
            msg, len(bad), tuple(bad[0]), X[tuple(bad[0])], g1[tuple(bad[0])], prod[tuple(bad[0])],
            R.CLASS_NAMES[pcls[tuple(bad[0])]], g0[tuple(bad[0])])


@pytest.mark.parametrize('mode', X_MODES)
def test_pd_scale_x_against_scale_x(mode):
    """predict_pd with the fixture's arguments as raw grid values = predict_pd in scaled mode on the packed bits of the same values.
    pd = Phibar . alpha and sd^2 = kappa |Li Phibar|^2 with Phibar the mean zeroed-column features rotated by g Fall[d] (tests/pd_ref.py),
    so a grid value off by dg moves pd by at most dg sum_j |F_dj| (|mc_j| + |ms_j|) (|ac_j| + |as_j|) and sd by at most
    dg sqrt(kappa) |Li|_2 |F_d| |m|_2; dg is at most two allowances (the two compiled copies are each within one of the true value).
    The rounding of the curves themselves is the same on both sides when the grid bits agree, and is bounded by K + 4 roundings of the
    absolute sum otherwise."""
    from oracle import scfgp_oracle as O
    from tests import pd_ref
    from tests.pred_grad_ref import fall
    k = kats()
    X, par = k['x%d_arg' % mode], k['x%d_par' % mode]
    T = X.shape[0]
    Xs = np.ascontiguousarray(packed(mode)[:T, :D])
    alpha, Li = factors()
    dims = list(range(D))
    eng = engine()
    try:
        params = eng.get_params()
        eng.set_x_scaler(R.host_scaler(mode, par))
        raw = eng.predict_pd(X, alpha, Li, dims, np.ascontiguousarray(X.T), mode='raw', want=('pd', 'sd'))
        sc = eng.predict_pd(Xs, alpha, Li, dims, np.ascontiguousarray(Xs.T), mode='scaled', want=('pd', 'sd'))
    finally:
        eng.close()
    same = all(raw[q].tobytes() == sc[q].tobytes() for q in ('pd', 'sd'))
    J = S + M
    Om = fall(params, D, S, M)
    kap = pd_ref.kappa(params)
    ac, as_ = np.abs(alpha[:J]), np.abs(alpha[J:])
    allow, cls = k['x%d_allow' % mode], k['x%d_cls' % mode]
    dg = np.where(np.isin(cls, (R.VALUE, R.SUB)), 2 * allow, 0.0).T                  # (D, G)
    worst = 0.0
    for d in dims:
        X0 = Xs.copy(); X0[:, d] = 0.0
        m0 = O.feature_map(X0, params, D, S, M).mean(0)
        mc, ms = np.abs(m0[:J]), np.abs(m0[J:])
        amp = float(((mc + ms) * (ac + as_)).sum())
        bpd = dg[d] * float((np.abs(Om[d]) * (mc + ms) * (ac + as_)).sum()) + (K + 4) * 2 * R.U * amp
        nli = np.linalg.norm(np.tril(Li), 2)
        nm = np.linalg.norm(m0)
        bsd = np.sqrt(kap) * nli * (dg[d] * np.linalg.norm(Om[d]) * nm + (K + 4) * 2 * R.U * nm * np.sqrt(K))
        e_pd = np.abs(raw['pd'][d] - sc['pd'][d]); e_sd = np.abs(raw['sd'][d] - sc['sd'][d])
        assert np.all(np.isfinite(raw['pd'][d])) and np.all(np.isfinite(raw['sd'][d]))
        msg = 'pd_scale_x mode %d dim %d: curves %s; worst |pd diff| / bound %.3g, |sd diff| / bound %.3g' % (
            mode, d, 'bit-equal' if same else 'NOT bit-equal', float((e_pd / bpd).max()), float((e_sd / bsd).max()))
        worst = max(worst, float((e_pd / bpd).max()), float((e_sd / bsd).max()))
        assert np.all(e_pd <= bpd) and np.all(e_sd <= bsd), msg
    print('\nscaler_range pd_scale_x mode %d: curves %s, worst difference / bound = %.3g' % (
        mode, 'bit-equal' if same else 'NOT bit-equal', worst))


# ---- the y scaler ------------------------------------------------------------------------------------------------------------------
TY = R.STEER_T
assert (D, S, M) == (R.STEER_D, R.STEER_S, R.STEER_M)


def y_engine(c, mode, par):
    from scfgp_amd.engine import HipEngine
    eng = HipEngine(D, S, M)
    eng.nonfinite = 'return'
    eng.set_params(R.steer_params(c))
    eng.set_x_scaler(R.host_scaler(1, np.array([[0.0] * D, [1.0] * D, [1.0] * D, [0.0] * D, [1.0] * D])))   # (x - 0) / (1 - 0)
    eng.set_y_scaler(R.host_scaler(mode, par))
    return eng


def ldv(a):
    return np.asarray(a, np.longdouble)


def check(name, tag, got, restated, allow, cls, finite):
    """device against the longdouble restatement under the model's allowance; finite: at least 90 % of the reference finite (asked of
    the values in every step; of std_y and of the derivatives where the band stays inside (0, 1): in the far tails 1 / pdf times the
    Box-Cox power overflows, and the class decides)"""
    if finite:
        assert np.isfinite(restated).mean() >= 0.9, (tag, name, float(np.isfinite(restated).mean()))
    ok, ratio = R.judge(got, restated, allow, cls)
    bad = np.flatnonzero(~ok)
    msg = report('%s %s' % (name, tag), ok, ratio)
    assert ok.all(), '%s; %d outside, first: got %r, restated %r, allowance %r, class %s' % (
        msg, len(bad), np.ravel(got)[bad[0]], np.ravel(restated)[bad[0]], np.ravel(allow)[bad[0]], R.CLASS_NAMES[np.ravel(cls)[bad[0]]])


@pytest.mark.parametrize('i', range(11))
def test_y_backward_at_the_device_s_own_arguments(i):
    """predict_y's mu_y and std_y, every sample of `sample` in mode 2 and every value of sample_grad in mode 2 against the restatement
    of y_backward (and of the std formula) at the bits that predict_raw, sample mode 1 and sample_grad mode 1 return, in every step of
    the steering."""
    assert np.finfo(np.longdouble).nmant >= 63
    mode, par, X, a_const, a_ramp = R.steering(i)
    lpar = R.ld(par)
    Li0 = np.zeros((K, K))
    _, Lis = factors()
    for step, off, scale, c, band in R.STEER_STEPS:
        a = off * a_const + scale * a_ramp
        Lsm = 0.05 * scale * Lis
        eng = y_engine(c, mode, par)
        try:
            mu_f, sd_f = eng.predict_raw(X, a, Li0)
            mu_y, sd_y, _ = eng.predict_y(X, a, Li0)
            s1 = eng.sample(X, a, Lsm, 3, seed=7, mode='raw')
            s2 = eng.sample(X, a, Lsm, 3, seed=7, mode='y')
            W = eng.sample_weights(a, Lsm, 3, seed=7)
            v1, g1 = eng.sample_grad(X, W, mode='raw')
            v2, g2 = eng.sample_grad(X, W, mode='y')
        finally:
            eng.close()
        m = mu_f[:, 0]
        assert np.all(sd_f == sd_f[0]) and sd_f[0] > 0 and np.unique(m).size > TY // 2      # Li = 0: sigma = sqrt(kappa) in every row
        tag = 'set %d (mode %d, lm %.4g) step %s' % (i, mode, par[2], step)
        inside = band or mode not in (3, 5)
        with np.errstate(all='ignore'):
            check('y_backward mu_y', tag, mu_y[:, 0], R.y_backward(ldv(m), mode, lpar),
                  *R.fl_model(R.model_y_backward, m.tolist(), mode, par), finite=True)
            check('std std_y', tag, sd_y[:, 0], R.y_std(ldv(m), ldv(sd_f), mode, lpar),
                  *R.fl_model(R.model_y_std, list(zip(m.tolist(), sd_f.tolist())), mode, par), finite=inside)
            check('y_backward sample', tag, s2.ravel(), R.y_backward(ldv(s1.ravel()), mode, lpar),
                  *R.fl_model(R.model_y_backward, s1.ravel().tolist(), mode, par), finite=True)
            check('y_backward sample_grad value', tag, v2, R.y_backward(ldv(v1), mode, lpar),
                  *R.fl_model(R.model_y_backward, v1.tolist(), mode, par), finite=True)
            # the gradient of a sample in y units: y_backward_deriv at the sample's scaled value, times its gradient in x
            dallow, dcls = R.fl_model(R.model_y_backward_deriv, v1.tolist(), mode, par)
            dv = R.y_backward_deriv(ldv(v1), mode, lpar)
            prod, pallow, pcls = _expected_product(g1, dv[:, None], dallow[:, None], dcls[:, None])
            check('y_backward_deriv sample_grad', tag, g2.ravel(), prod.ravel(), pallow.ravel(), pcls.ravel(), finite=inside)


@pytest.mark.parametrize('i', range(11))
def test_y_backward_deriv_through_predict_grad(i):
    """predict_grad in y units against mode 1's mu, sigma, dmu, dsigma put through the restatement of ygrad_kernel and ypost_kernel;
    where the band mu +- sigma leaves (0, 1) the class decides."""
    mode, par, X, a_const, a_ramp = R.steering(i)
    lpar = R.ld(par)
    _, Lis = factors()
    Li = 0.5 * Lis
    for step, off, scale, c, band in R.STEER_STEPS:
        a = off * a_const + scale * a_ramp
        eng = y_engine(c, mode, par)
        try:
            mu1, sd1, dmu1, dsd1 = eng.predict_grad(X, a, Li, mode='raw')
            mu2, sd2, dmu2, dsd2 = eng.predict_grad(X, a, Li, mode='y')
        finally:
            eng.close()
        m, s = mu1[:, 0], sd1
        tag = 'set %d (mode %d, lm %.4g) step %s' % (i, mode, par[2], step)
        inside = band or mode not in (3, 5)
        assert np.abs(dsd1).max() > 0 and np.all(np.isfinite(dmu1)) and np.all(np.isfinite(dsd1))
        with np.errstate(all='ignore'):
            check('y_backward mu', tag, mu2[:, 0], R.y_backward(ldv(m), mode, lpar),
                  *R.fl_model(R.model_y_backward, m.tolist(), mode, par), finite=True)
            check('std', tag, sd2, R.y_std(ldv(m), ldv(s), mode, lpar),
                  *R.fl_model(R.model_y_std, list(zip(m.tolist(), s.tolist())), mode, par), finite=inside)
            # dmu = D(mu) * dmu
            dallow, dcls = R.fl_model(R.model_y_backward_deriv, m.tolist(), mode, par)
            dv = R.y_backward_deriv(ldv(m), mode, lpar)
            prod, pallow, pcls = _expected_product(dmu1, dv[:, None], dallow[:, None], dcls[:, None])
            check('y_backward_deriv dmu', tag, dmu2.ravel(), prod.ravel(), pallow.ravel(), pcls.ravel(), finite=inside)
            # dstd = (D(mu + s) (dmu + ds) - D(mu - s) (dmu - ds)) / 2
            rows = [(m[t], s[t], dmu1[t, d], dsd1[t, d]) for t in range(TY) for d in range(D)]
            allow, cls = R.fl_model(R.model_y_dstd, rows, mode, par)
            restated = R.y_dstd(ldv(m)[:, None], ldv(s)[:, None], ldv(dmu1), ldv(dsd1), mode, lpar)
            check('dstd', tag, dsd2.ravel(), restated.ravel(), allow, cls, finite=inside)


def test_grid_stride_pass_and_chunk_seam():
    """D = 17 and T = 32768 + 257: two chunks, and T D is more than one pass of the 2048 x 256 threads of xgrad_kernel and ygrad_kernel.
    X scaler in mode 5, y scaler in mode 4; every row's predict_grad output in y units is bit-equal to the same row in a T = 257 call."""
    k = kats()
    Dw, step = 17, 257
    T = 32768 + step
    assert T * Dw > 2048 * 256 and T > 32768
    par = np.tile(k['x5_par'], (1, 5))[:, :Dw]
    cols = np.tile(k['x5_arg'], (1, 5))[:, :Dw]                                     # the fixture's arguments, cycled over the rows
    X = np.ascontiguousarray(cols[(np.arange(T)[:, None] * 7 + np.arange(Dw)[None, :] * 13) % cols.shape[0], np.arange(Dw)[None, :]])
    i = int(np.flatnonzero((k['y_mode'] == 4) & (k['y_par'][:, 2] == 0.3))[0])
    ypar = k['y_par'][i]
    alpha, Li = factors()
    eng = engine(D=Dw)
    try:
        eng.set_x_scaler(R.host_scaler(5, par))
        eng.set_y_scaler(R.host_scaler(4, ypar))
        whole = eng.predict_grad(X, alpha, Li, mode='y')
        Dp = eng.dims()['Dp']
        tail = np.empty((1024, Dp))                                                # "pXt" holds the last chunk: 257 rows padded to 512
        assert eng.lib.scfgp_debug_read(eng.ctx, b'pXt', tail.ctypes.data_as(C.c_void_p), tail.nbytes) == 8 * 512 * Dp
        assert np.all(tail[:step, Dw] == 1.0) and np.all(tail[step:512] == 0.0)
        rows = 0
        for t0 in range(0, T, step):
            part = eng.predict_grad(X[t0:t0 + step], alpha, Li, mode='y')
            n = part[0].shape[0]
            for a, b in zip(whole, part):
                assert a[t0:t0 + n].tobytes() == b.tobytes(), t0
            rows += n
        assert rows == T
    finally:
        eng.close()
    assert np.isfinite(whole[2]).mean() > 0.5 and np.isfinite(whole[3]).mean() > 0.5
