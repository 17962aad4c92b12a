"""GPU tier of the greedy Monte-Carlo batch expected improvement (selectqei.hip: scfgp_select_qei).  The reference in every test is the
numpy restatement (tests/select_qei_ref.py) applied to the device's own scfgp_sample block, to which the call's F is bit-equal by
construction, so no feature-map tolerance enters: idx and mstate exactly, gain / score0 / qei within the bound of an nsamp-term sum.
Then the exact properties on the device (monotone gains, prefix, appended weight-0 rows, moved rows, a duplicated pool), the mask,
pending rows, the all-zero tail, raw mode, the f16x3 context, the errors with untouched outputs and the survival of the training state,
and the SCFGP.select_qei facade."""
import numpy as np
import pytest

from scfgp_amd import synth
from scfgp_amd.scaler import Scaler
from tests import select_qei_ref as Q
from tests.test_gpu_sample_argmax import _same_bits, _synthetic

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _bound(nsamp):
    """a sum of nsamp non-negative fp64 terms in any order, plus the division: relative"""
    return (nsamp + 1) * U


def _close(got, ref, nsamp):
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    return got.shape == ref.shape and bool(np.all(np.abs(got - ref) <= _bound(nsamp) * np.abs(ref)))


def _median_best(F, minimize):
    return float(np.median(F.min(axis=0) if minimize else F.max(axis=0)))


def _check_against_block(F, got, m, best, xi=0.0, w=None, pending=None, minimize=False, rows=None):
    """got = (idx, gain, qei, score0, mstate) of the device against the restatement on the device's own block F.  The precondition is
    asserted on the reference alone: at every pick the two best eligible scores differ by more than four times the bound, or the best
    score is exactly 0 -- then every remaining score is an exact 0 on both sides (a sum of zeros has no rounding) and the tie goes to
    the lowest index on both."""
    ns = F.shape[1]
    idx, gain, qei, score0, mstate = got
    ridx, rgain, rscore0, rm, rqei = Q.greedy(F, m, best, xi, w, pending, minimize)
    gaps = Q.top_two_gaps(F, m, best, xi, w, pending, minimize)
    assert np.all((gaps > 4 * _bound(ns)) | (rgain == 0.0)), (gaps, rgain)
    assert idx.dtype == np.int64 and np.array_equal(idx, ridx), (idx, ridx)
    rows = slice(None) if rows is None else rows
    err = lambda a, b: float(np.max(np.abs(a - b) / np.where(b != 0, np.abs(b), 1.0))) / U
    print('nsamp %d minimize %d: gain %.1f u, score0 %.1f u, qei %.1f u (bound %d u); gains %s' % (
        ns, minimize, err(gain, rgain), err(score0[rows], rscore0[rows]), err(qei, rqei), ns + 1, np.array2string(rgain, precision=3)))
    assert _close(gain, rgain, ns)
    assert _close(score0[rows], rscore0[rows], ns)
    assert _same_bits(mstate, rm)
    assert _close(qei, rqei, ns)


def _call(eng, Xs, alpha, Li, m, ns, best, **kw):
    return eng.select_qei(Xs, alpha, Li, m, ns, best, return_score0=True, return_state=True, **kw)


# A: K = 42, ragged rows, every launch width of the product; B: the second chunk is a ragged tail.  nsamp covers both lane-group widths
# (16 lanes up to 64 samples, a wave above), odd row pitches, a single sample and the documented bound 1024.  best = the median of the block's column maxima
# (minima when minimising): some samples can still improve and some cannot.
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('D,S,M,T,counts', [(3, 1, 20, 700, (1, 7, 17, 100, 300, 1024)), (5, 4, 60, 32768 + 500, (7, 65))])
def test_parity_with_the_restatement_on_the_device_block(D, S, M, T, counts, dtype):
    eng, params, alpha, Li = _synthetic(D, S, M, dtype)
    Xs = synth.make_X(101, T, D)
    for ns in counts:
        F = eng.sample(Xs, alpha, Li, ns, seed=9, noise=False)
        for minimize in (False, True):
            best = _median_best(F, minimize)
            got = _call(eng, Xs, alpha, Li, 6, ns, best, seed=9, minimize=minimize)
            _check_against_block(F, got, 6, best, minimize=minimize)
    eng.close()


@pytest.mark.parametrize('ns', [17, 100])
@pytest.mark.parametrize('T', [700, 32768 - 100])
def test_exact_properties(T, ns):
    eng, params, alpha, Li = _synthetic(5, 4, 60, 'f32')
    Xs = synth.make_X(55, T, 5)
    col = eng.sample(Xs, alpha, Li, ns, seed=4)
    for minimize in (False, True):
        best, xi = _median_best(col, minimize), 0.01
        kw = dict(xi=xi, seed=4, minimize=minimize)
        idx, gain, qei, score0, mstate = _call(eng, Xs, alpha, Li, 9, ns, best, **kw)
        assert gain[0] > 0.0 and np.all(gain[1:] <= gain[:-1]) and np.all(gain >= 0.0)
        assert len(set(idx.tolist())) == 9
        i3, g3, q3, s3, m3 = _call(eng, Xs, alpha, Li, 3, ns, best, **kw)
        assert np.array_equal(i3, idx[:3]) and _same_bits(g3, gain[:3]) and _same_bits(s3, score0) and _same_bits(q3[:1], qei[:1])
        # 300 rows of weight 0 behind the pool (T = 32668: they cross the chunk boundary): a score depends on its row only
        more = np.concatenate([Xs, synth.make_X(56, 300, 5)])
        w = np.r_[np.ones(T), np.zeros(300)]
        ia, ga, qa, sa, ma = _call(eng, more, alpha, Li, 9, ns, best, w=w, **kw)
        assert np.array_equal(ia, idx) and _same_bits(ga, gain) and _same_bits(sa[:T], score0) and _same_bits(ma, mstate)
        # the first 70 rows moved to the end: the picks move with their rows (those of gain 0 go by index, so they are left out)
        im, gm, qm, sm, mm = _call(eng, np.concatenate([Xs[70:], Xs[:70]]), alpha, Li, 9, ns, best, **kw)
        k = int(np.count_nonzero(gain > 0.0))
        assert k >= 5 and np.array_equal(im[:k], np.where(idx >= 70, idx - 70, idx + T - 70)[:k]) and _same_bits(gm, gain)
        assert _same_bits(sm, np.concatenate([score0[70:], score0[:70]])) and _same_bits(mm, mstate) and _same_bits(qm, qei)
        # every row again behind the pool: each score ties with its copy, the lowest index wins
        i2, g2, q2, s2, m2 = _call(eng, np.concatenate([Xs, Xs]), alpha, Li, 9, ns, best, **kw)
        assert np.array_equal(i2, idx) and _same_bits(g2, gain) and _same_bits(s2, np.r_[score0, score0]) and _same_bits(q2, qei)
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_mask(dtype):
    eng, params, alpha, Li = _synthetic(5, 4, 60, dtype)
    T, ns, m = 3001, 17, 6
    Xs = synth.make_X(101, T, 5)
    F = eng.sample(Xs, alpha, Li, ns, seed=9)
    for minimize in (False, True):
        best = _median_best(F, minimize)
        free = _call(eng, Xs, alpha, Li, m, ns, best, seed=9, minimize=minimize)
        w = np.full(T, 2.0)
        w[free[0]] = 0.0                                            # every unmasked pick
        w[256:384] = 0.0                                            # a whole workgroup's rows of the sweep
        got = _call(eng, Xs, alpha, Li, m, ns, best, seed=9, w=w, minimize=minimize)
        assert not np.isin(got[0], free[0]).any() and not ((got[0] >= 256) & (got[0] < 384)).any()
        assert _same_bits(got[3], free[3])                          # score0 of every row, eligible or not
        _check_against_block(F, got, m, best, w=w, minimize=minimize)
        few = np.zeros(T); few[[5, 1234, 2999, 300, 301]] = 1e-300  # m equal to the eligible count
        got = _call(eng, Xs, alpha, Li, 5, ns, best, seed=9, w=few, minimize=minimize)
        assert sorted(got[0].tolist()) == [5, 300, 301, 1234, 2999]
        _check_against_block(F, got, 5, best, w=few, minimize=minimize)
        for wt in (np.ones(T), 3.5 * np.ones(T)):                   # positive values are not multiplied in
            same = _call(eng, Xs, alpha, Li, m, ns, best, seed=9, w=wt, minimize=minimize)
            assert all(_same_bits(a, b) for a, b in zip(same[1:], free[1:])) and np.array_equal(same[0], free[0])
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('ns', [17, 100])
def test_pending(ns, dtype):
    eng, params, alpha, Li = _synthetic(5, 4, 60, dtype)
    T = 3001
    Xs = synth.make_X(101, T, 5)
    F = eng.sample(Xs, alpha, Li, ns, seed=9)
    for minimize in (False, True):
        best = _median_best(F, minimize)
        p, gain, qei, score0, mstate = _call(eng, Xs, alpha, Li, 3, ns, best, seed=9, minimize=minimize)
        assert gain[2] > 0.0
        w = np.ones(T); w[p[:2]] = 0.0
        got = _call(eng, Xs, alpha, Li, 1, ns, best, seed=9, w=w, pending=Xs[p[:2]], minimize=minimize)
        assert got[0][0] == p[2] and _same_bits(got[1], gain[2:])
        assert _same_bits(got[4], mstate)
        assert _close(got[2][0], gain[0] + gain[1], ns) and _close(got[2][1], qei[1], ns)
        _check_against_block(F, got, 1, best, w=w, pending=F[p[:2]], minimize=minimize)
        # pending rows from outside the pool
        Xp = synth.make_X(77, 130, 5)
        got = _call(eng, Xs, alpha, Li, 4, ns, best, seed=9, pending=Xp, minimize=minimize)
        _check_against_block(F, got, 4, best, pending=eng.sample(Xp, alpha, Li, ns, seed=9), minimize=minimize)
    eng.close()


def test_all_zero_tail():
    eng, params, alpha, Li = _synthetic(3, 1, 20, 'f64')
    T, ns, m = 700, 17, 5
    Xs = synth.make_X(101, T, 3)
    F = eng.sample(Xs, alpha, Li, ns, seed=9)
    w = np.ones(T); w[[0, 2, 3]] = 0.0
    for minimize in (False, True):
        far = float(np.abs(F).max()) + 10.0
        best = -far if minimize else far
        idx, gain, qei, score0, mstate = _call(eng, Xs, alpha, Li, m, ns, best, seed=9, w=w, minimize=minimize)
        assert np.array_equal(idx, [1, 4, 5, 6, 7]) and np.all(gain == 0.0) and np.all(score0 == 0.0) and np.all(qei == 0.0)
        assert np.all(mstate == far)
        # some picks improve, then nothing is left: one sample, so the first pick takes all there is
        best = _median_best(F[:, :1], minimize) - (-1.0 if minimize else 1.0)
        got = _call(eng, Xs, alpha, Li, m, 1, best, seed=9, w=w, minimize=minimize)
        assert got[1][0] > 0.0 and np.all(got[1][1:] == 0.0)
        assert np.array_equal(np.sort(got[0][1:]), [t for t in (1, 4, 5, 6, 7, 8) if t != got[0][0]][:m - 1])
        _check_against_block(F[:, :1], got, m, best, w=w, minimize=minimize)
    eng.close()


def _scaled_problem(xalgo, seed=5, N=600):
    """tests/test_gpu_select.py's problem: an engine trained on scaled data of 4 raw columns, one of them constant"""
    from scfgp_amd.engine import HipEngine
    rng = np.random.default_rng(seed)
    Xr = np.column_stack([rng.uniform(0.5, 3.0, N), rng.gamma(2.0, 1.0, N), np.full(N, 2.5), rng.normal(1.0, 2.0, N)])
    yr = np.exp(0.3 * np.sin(Xr[:, :1]) + 0.1 * Xr[:, 1:2]) + 0.05 * rng.standard_normal((N, 1))
    xs = Scaler(xalgo); xs.fit(Xr); ys = Scaler('normal'); ys.fit(yr)
    D, S, M = 3, 2, 40
    eng = HipEngine(D, S, M, dtype='f64')
    eng.set_params(synth.make_params(seed, D, S, M, abc=(-1.0, 0.0, -4.0)))
    fx = np.ascontiguousarray(xs.forward_transform(Xr)); fy = np.ascontiguousarray(ys.forward_transform(yr))
    eng.set_data(fx[:300], fy[:300])
    _, _, alpha, Li = eng.eval(want_grad=False)
    eng.set_x_scaler(xs)
    return eng, alpha.copy(), Li.copy(), Xr[300:], fx[300:]


# the two X scalers whose device transform is the host's arithmetic operation for operation; the others go through erfc / pow, which
# are different implementations on the two sides, and are covered against the device's own raw-mode block
@pytest.mark.parametrize('xalgo', Scaler.algos)
def test_raw_mode(xalgo):
    eng, alpha, Li, Xr, fx = _scaled_problem(xalgo)
    assert Xr.shape[1] == 4 and fx.shape[1] == 3                    # the constant column is dropped
    ns, m = 24, 5
    F = eng.sample(Xr, alpha, Li, ns, seed=8, mode='raw')
    for minimize in (False, True):
        best = _median_best(F, minimize)
        raw = _call(eng, Xr[10:], alpha, Li, m, ns, best, seed=8, pending=Xr[:10], mode='raw', minimize=minimize)
        _check_against_block(F[10:], raw, m, best, pending=F[:10], minimize=minimize)
        if xalgo in ('min-max', 'normal'):
            sc = _call(eng, fx[10:], alpha, Li, m, ns, best, seed=8, pending=fx[:10], minimize=minimize)
            assert np.array_equal(raw[0], sc[0]) and all(_same_bits(a, b) for a, b in zip(raw[1:], sc[1:]))
    eng.close()


def test_f16x3_context_equals_fp32_context():
    from scfgp_amd.engine import HipEngine
    D, S, M, T = 5, 4, 60, 32768 + 500
    e32, params, alpha, Li = _synthetic(D, S, M, 'f32')
    e16 = HipEngine(D, S, M, dtype='f16x3'); e16.set_params(params)
    Xs = synth.make_X(202, T, D)
    w = np.ones(T); w[::3] = 0.0
    for ns, wt, minimize in ((17, None, False), (100, w, True)):
        best = _median_best(e32.sample(Xs[:2000], alpha, Li, ns, seed=1), minimize)
        a = _call(e32, Xs, alpha, Li, 5, ns, best, seed=1, w=wt, pending=Xs[:3], minimize=minimize)
        b = _call(e16, Xs, alpha, Li, 5, ns, best, seed=1, w=wt, pending=Xs[:3], minimize=minimize)
        assert np.array_equal(a[0], b[0]) and all(_same_bits(u, v) for u, v in zip(a[1:], b[1:]))
    e32.close(); e16.close()


def test_errors_leave_the_outputs_untouched():
    from scfgp_amd.engine import HipEngine
    from scfgp_amd._lib import dptr, _c_i64_p
    eng, params, alpha, Li = _synthetic(5, 4, 60, 'f64')
    T, ns, m = 300, 4, 3
    Xs = synth.make_X(3, T, 5)
    Xp = synth.make_X(4, 7, 5)
    idx = np.full(m, -77, np.int64)
    gain = np.full(m, -77.5); score0 = np.full(T, -77.5); mstate = np.full(ns, -77.5); qei = np.full(2, -77.5)

    def call(e=None, X=Xs, rows=T, w=None, P=None, npend=0, a=alpha, L=Li, n=ns, best=0.0, xi=0.0, picks=m, mode=0, i=idx):
        e = e or eng
        rc = e.lib.scfgp_select_qei(e.ctx, dptr(X), rows, dptr(w), dptr(P), npend, dptr(a), dptr(L), n, 0, best, xi, picks, mode, 0,
                                    None if i is None else i.ctypes.data_as(_c_i64_p), dptr(gain), dptr(score0), dptr(mstate), dptr(qei))
        assert np.all(idx == -77) and all(np.all(v == -77.5) for v in (gain, score0, mstate, qei))
        return rc, e.last_error()

    neg = np.ones(T); neg[7] = -1.0
    two = np.zeros(T); two[[4, 9]] = 1.0
    cases = [(dict(X=None), 'NULL'), (dict(a=None), 'NULL'), (dict(L=None), 'NULL'), (dict(i=None), 'NULL'),
             (dict(rows=0), 'T must lie'), (dict(rows=2 ** 20 + 1), 'T must lie'), (dict(picks=0), 'm must lie'), (dict(picks=4097), 'm must lie'),
             (dict(n=0), 'nsamp must lie in 1..1024'), (dict(n=1025), 'nsamp must lie in 1..1024'),
             (dict(mode=2), 'mode must be 0 or 1'), (dict(mode=-1), 'mode must be 0 or 1'),
             (dict(P=Xp, npend=-1), 'np must not be negative'), (dict(npend=3), 'NULL Xp'), (dict(xi=-1e-3), 'xi must not be negative'),
             (dict(mode=1), 'no X scaler'), (dict(w=neg), 'negative weight at row 7'), (dict(w=two), 'only 2 rows have a positive weight'),
             (dict(picks=T + 1), 'only 300 rows')]
    for kw, msg in cases:
        rc, err = call(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)
    for kw in (dict(best=np.nan), dict(best=np.inf), dict(xi=np.nan), dict(xi=np.inf)):
        rc, err = call(**kw)
        assert rc == -4 and 'non-finite' in err, (kw, rc, err)
    for bad in (np.inf, np.nan):
        w = np.ones(T); w[11] = bad
        rc, err = call(w=w)
        assert rc == -4 and 'non-finite' in err
    Xn = Xs.copy(); Xn[123, 2] = np.nan
    rc, err = call(X=Xn)                                            # a NaN row in an eligible position
    assert rc == -4 and 'non-finite' in err
    w = np.ones(T); w[123] = 1e-300
    rc, err = call(X=Xn, w=w)                                       # the same with explicit weights
    assert rc == -4 and 'non-finite' in err
    Pn = Xp.copy(); Pn[3, 0] = np.inf
    rc, err = call(P=Pn, npend=7)                                   # a non-finite pending row
    assert rc == -4 and 'non-finite' in err
    with pytest.raises(FloatingPointError, match='non-finite'):
        eng.select_qei(Xn, alpha, Li, m, ns, 0.0)
    w[123] = 0.0                                                    # the NaN row excluded: not an error, and the others keep their bits
    got = _call(eng, Xn, alpha, Li, m, ns, 0.0, w=w)
    want = _call(eng, Xs, alpha, Li, m, ns, 0.0, w=w)
    keep = np.arange(T) != 123
    assert np.array_equal(got[0], want[0]) and _same_bits(got[1], want[1]) and _same_bits(got[2], want[2])
    assert _same_bits(got[3][keep], want[3][keep]) and _same_bits(got[4], want[4])
    with pytest.raises(ValueError, match='w has'):
        eng.select_qei(Xs, alpha, Li, m, ns, 0.0, w=np.ones(T - 1))
    with pytest.raises(ValueError, match='scaler'):
        eng.select_qei(Xs, alpha, Li, m, ns, 0.0, mode='raw')
    only_idx = np.full(m, -1, np.int64)                             # every output but idx may be NULL
    assert eng.lib.scfgp_select_qei(eng.ctx, dptr(Xs), T, None, None, 0, dptr(alpha), dptr(Li), ns, 0, 0.0, 0.0, m, 0, 0,
                                    only_idx.ctypes.data_as(_c_i64_p), None, None, None, None) == 0
    assert np.array_equal(only_idx, eng.select_qei(Xs, alpha, Li, m, ns, 0.0)[0])
    eng.close()
    fresh = HipEngine(5, 4, 60, dtype='f64')                        # no parameters yet
    rc, err = call(e=fresh)
    assert rc == -1 and 'parameters not set' in err
    fresh.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_training_state_survives(dtype):
    from scfgp_amd.engine import HipEngine
    D, S, M = 5, 4, 60
    params = synth.make_params(7, D, S, M, abc=(-1.0, 0.0, -1.0))
    X = synth.make_X(7, 1500, D)
    y = np.sin(3 * X[:, :1]) + 0.1 * synth.normal(10, 0, 1500)[:, None]
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params); eng.set_data(X, y)
    c0, g0, a0, L0 = eng.eval(want_grad=True)
    c0, g0, a0, L0 = float(c0), g0.copy(), a0.copy(), L0.copy()
    Xs = synth.make_X(9, 33000, D)
    w = np.ones(33000); w[:100] = 0.0
    eng.select_qei(Xs, a0, L0, 4, 40, float(y.max()), seed=2, w=w, pending=Xs[:5])
    Xn = Xs.copy(); Xn[200, 0] = np.nan
    with pytest.raises(FloatingPointError):                         # an error return leaves the state alone as well
        eng.select_qei(Xn, a0, L0, 4, 40, float(y.max()), seed=2, w=w)
    c1, g1, a1, L1 = eng.eval(want_grad=True)
    assert float(c1) == c0 and np.array_equal(g1, g0) and np.array_equal(a1, a0) and np.array_equal(L1, L0)
    eng.close()


def test_facade_select_qei():
    from scfgp_amd import SCFGP
    rng = np.random.default_rng(5)
    np.random.seed(5)
    X = rng.uniform(-2, 2, (300, 3))
    X = np.column_stack([X[:, :2], np.full(300, 4.0), X[:, 2:]])     # a constant column
    y = np.sin(X[:, :1]) + 0.5 * X[:, 1:2] ** 2 + 0.05 * rng.standard_normal((300, 1))
    model = SCFGP(sparsity=3, nfeats=12, device_scaler=True)
    model.set_data(X[:240], y[:240])
    model.optimize(X[240:], y[240:], max_iter=20,
                   algo={'algo': 'adam', 'algo_params': {'learning_rate': 0.02, 'beta1': 0.9, 'beta2': 0.999, 'epsilon': 1e-8}})
    pool, m = X[240:], 6
    a0, L0 = model.alpha.copy(), model.Li.copy()
    for minimize in (False, True):
        # an incumbent in the middle of the targets, in raw y units: there is room for improvement
        idx, gain = model.select_qei(pool, m, nsamples=64, best=float(np.median(y)), seed=3, minimize=minimize)
        assert idx.dtype == np.int64 and idx.shape == (m,) and gain.shape == (m,)
        assert len(set(idx.tolist())) == m and idx.min() >= 0 and idx.max() < 60
        assert gain[0] > 0.0 and np.all(gain[1:] <= gain[:-1])
        w = np.ones(60); w[idx[:3]] = 0.0
        i2, g2 = model.select_qei(pool, m - 3, nsamples=64, best=float(np.median(y)), seed=3, weights=w, pending=pool[idx[:3]],
                                  minimize=minimize)
        assert np.array_equal(i2, idx[3:]) and _same_bits(g2, gain[3:])
        i3, g3 = model.select_qei(pool, m, nsamples=64, seed=3, minimize=minimize)      # best: the best observed training target
        assert len(set(i3.tolist())) == m and np.all(g3[1:] <= g3[:-1]) and np.all(g3 >= 0.0)
    assert np.array_equal(model.alpha, a0) and np.array_equal(model.Li, L0)
    other = SCFGP(sparsity=3, nfeats=12)
    other.pred_func = lambda Xs, alpha, Li: None
    with pytest.raises(TypeError):
        other.select_qei(pool, 4)
