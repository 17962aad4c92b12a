"""
Stale-state sequences across the posterior entry points (not a test, not a conftest: the helper of tests/test_posterior_sequence_ref.py
and tests/test_gpu_posterior_sequence.py).

One context lives through a seeded schedule of calls: the eighteen posterior entry points added after tests/test_gpu_round3.py's sequence
test was written (predict_raw, predict_y, predict_grad, sample, sample_weights, sample_argmax, sample_grad, acquire, predict_cov,
condition, forget, loo, select, select_iv, select_qei, predict_gradcov, predict_pd, acquire_kg) and predict, in the modes their
registered scalers allow, with set_params,
scaler changes, the training calls of that test and documented failing calls between them.  Every posterior step is checked

  (a) bit for bit against a TWIN: a fresh context with the same parameters, scalers, options and resident rows that makes the same call
      once (include/scfgp_hip.h documents for each of these entry points that an output depends on its inputs only);
  (b) against the CPU references (tests/*_ref.py and the oracle) under the bound the entry point's own GPU test uses: the constants are
      imported from those modules, none is restated.

The schedule is symbolic (kinds, row counts, modes, seeds); `Fit` is the CPU-side model of the fit it moves: raw rows and targets, the
parameters, the scalers and the oracle's (alpha, Li) on the rows currently in the fit.  The device is always fed the ORACLE's factors, so
only the entry point under test contributes error.  `RefEngine` puts the references behind HipEngine's interface, so that the runner
and every check can be exercised without a GPU.

Modes.  'raw': the reference is evaluated on the host-transformed rows (Scaler.forward_transform; gradients chained with
pred_grad_ref.x_scaler_deriv) under the entry point's own bound -- the device's element-wise fp64 transform agrees with the host's to
1e-11 (tests/test_gpu_parity.py), far inside every such bound.  'y': the y scaler's backward transform is not Lipschitz (normal ppf), so
a y-mode step follows a raw-mode step on the same rows and is checked, as the own tests do, against the host tail applied to the
DEVICE's raw-mode outputs of that step with those tests' tolerances.

The geometry sweep (SWEEP_GEOMETRIES, sweep_schedule; the helper of tests/test_posterior_geometry_ref.py and
tests/test_gpu_posterior_geometry.py) uses the same runner, references and records on a lean schedule per geometry (scfgp_acquire_kg
was once in that schedule only; it now lives through the sequences too), with two further checks: (c) a call on row 0 alone against
row 0 of the 257-row call, bit for bit, and (d) an f16x3 context against the f32 context, bit for bit.

Input conditions.  Some checks are fair only for inputs that are not a cancellation or near-degenerate: kg_conditioning (acquire_kg),
pd_cancellation (predict_pd's sums), conditioned_row0 and acquire_grad_cancellation
(steps on row 0 alone).  They are computed from the fp64 references alone and never change a bound.  The sweep meets them through the
salt of a group's seed; a sequence, whose fit is known only once its schedule has run so far, repeats the draw of such a step at run time
until the condition holds (materialise).  Both CPU tiers assert every one of them.
"""
import functools

import numpy as np

from oracle import scfgp_oracle as O
from scfgp_amd.scaler import Scaler
from tests import acquire_ref as A
from tests import condition_ref, forget_ref, loo_ref, parity, pred_cov_ref
from tests import gradcov_ref as GC
from tests import kg_ref as KG
from tests import pd_ref as PD
from tests import pred_grad_ref as G
from tests import sample_argmax_ref as AM
from tests import sample_grad_ref as SG
from tests import sample_ref as SR
from tests import select_iv_ref as V
from tests import select_qei_ref as Q
from tests import select_ref as R
# tolerance constants of the entry points' own GPU tests (importing these modules needs no GPU)
from tests import test_gpu_acquire as T_ACQ
from tests import test_gpu_acquire_kg as T_KG
from tests import test_gpu_predict_cov as T_COV
from tests import test_gpu_predict_grad as T_PG
from tests import test_gpu_predict_gradcov as T_GC
from tests import test_gpu_predict_pd as T_PD
from tests import test_gpu_round3 as T_R3
from tests import test_gpu_sample as T_SMP
from tests import test_gpu_sample_grad as T_SG
from tests import test_gpu_select as T_SEL
from tests import test_gpu_select_iv as T_IV
from tests import test_gpu_select_qei as T_QEI

GEOMETRIES = [(7, 3, 40), (5, 4, 60), (40, 6, 150), (5, 12, 200)]       # K = 86 < Kp; K = 128 = Kp; rank-S projection live; K = 424
DTYPES = ('f64', 'f32')
CASES = [(g, dt) for g in GEOMETRIES for dt in DTYPES]
SIZES = (1, 37, 255, 256, 257, 700, 3000)                                # either side of the 256-row padding
BIG = (32768, 32769, 65536 + 300)                                        # one chunk exactly, two chunks, three (both halves reused)
def gradcov_points_per_chunk(D, S, want_cov):
    """include/scfgp_hip.h's np of scfgp_predict_gradcov restated: whole groups of 64 / q points (q = min(D, S)) in the 32 768-row
    buffers and, where a D x D array per point is wanted (dcov, asub), at most a 64 MiB slot of them"""
    q = min(D, S)
    gs = (64 // q) * q
    n = (32768 // gs) * (64 // q)
    return min(n, max(1, (64 << 20) // (8 * D * D))) if want_cov else n


# scripted big visits per geometry, at entry points whose CPU reference is affordable at that size; predict_gradcov at three of its own
# chunks (the chunk of geometry 1 with a D x D array per point), predict_pd at three row chunks
BIG_GRADCOV = 2 * gradcov_points_per_chunk(5, 4, True) + 300
BIG_VISITS = {0: (('condition', BIG[0]), ('sample_argmax', BIG[2]), ('predict_pd', BIG[2])),
              1: (('acquire', BIG[1]), ('predict_raw', BIG[0]), ('predict_gradcov', BIG_GRADCOV)),
              2: (('sample', BIG[2]),), 3: (('predict_grad', BIG[1]),)}
POSTERIOR = ('predict_raw', 'predict_y', 'predict_grad', 'sample', 'sample_weights', 'sample_argmax', 'sample_grad', 'acquire',
             'predict_cov', 'condition', 'forget', 'loo', 'select', 'select_iv', 'select_qei', 'predict_gradcov', 'predict_pd', 'acquire_kg')
# the first posterior call of case i: ensure_pred_factor, ensure_update, ensure_loo and ensure_forget are each reached first somewhere
FIRST = ('predict_grad', 'condition', 'loo', 'forget', 'select_iv', 'predict_cov', 'acquire', 'sample')
Y_MODE = ('predict_grad', 'sample', 'sample_argmax', 'sample_grad')      # entry points with a raw-y mode (predict_y is one by itself)
NSAMP = (1, 7, 300)
GRID = (1, 9, 64)                                                        # grid values per dimension of a predict_pd step
KG_REFS = (0, 37)                                                        # reference rows of an acquire_kg step (0: the candidates themselves)
KG_NODES = (None, 3, 17)                                                 # its nodes: the default set, or tests/test_gpu_acquire_kg.py's NODES
PICKS = (1, 5, 40)
OPTIONS = [('gram64', (0, 2, 3)), ('factor_form', (-1, 1)), ('lowrank_bwd', (-1, 0, 1)), ('gram_nsplit', (0, 3)), ('gram_taper', (0, 1)),
           ('apply_dma', (-1, 0, 1, 2))]                                 # those of the round-3 sequence test

# (ctol, gtol, ptol) of the training steps: read off the round-3 sequence test's own parametrisation, unchanged
SEQ_TOL = {}
for _m in T_R3.test_one_context_through_a_random_sequence_of_calls.pytestmark:
    if _m.name == 'parametrize' and _m.args[0].startswith('dtype'):
        SEQ_TOL = {v[0]: tuple(v[1:]) for v in _m.args[1]}
assert set(SEQ_TOL) == {'f64', 'f32'}
EPS = {dt: parity.TOL[dt]['eps'] for dt in DTYPES}


def kappa(params):
    return float(np.log1p(np.exp(params[2])))


# ---- data ------------------------------------------------------------------------------------------------------------------------------
CONST_COL = 1                                                            # a constant raw column: every X scaler drops it


def raw_rows(rng, n, D, spread=1.0):
    """(n, D + 1) positive raw rows, column CONST_COL constant (spread < 1: a narrower pool around the same centre)"""
    X = np.exp(0.5 * spread * rng.standard_normal((n, D)))
    return np.ascontiguousarray(np.insert(X, CONST_COL, 2.5, axis=1))


def raw_targets(rng, Xraw):
    return np.exp(0.3 * np.sin(Xraw[:, :1]) + 0.1 * rng.standard_normal((Xraw.shape[0], 1)))


@functools.lru_cache(maxsize=None)
def x_scaler(algo, D):
    """fitted on small data (60 rows)"""
    s = Scaler(algo); s.fit(raw_rows(np.random.default_rng(4001 + D), 60, D))
    return s


@functools.lru_cache(maxsize=None)
def y_scaler(algo):
    rng = np.random.default_rng(4002)
    s = Scaler(algo); s.fit(raw_targets(rng, raw_rows(rng, 60, 3)))
    return s


def new_params(rng, D, S, M):
    """the round-3 sequence test's draw, c = -0.6 included.  The noise parameter stays in the range the fp32 row of parity.TOL was set
    at (c = -1 .. -0.6 in every fp32 test of the project): the predictive bound eps sigma0 shrinks with sqrt(kappa) = sqrt(softplus(c))
    while the fp32 rounding error of mu = phi^T alpha does not.  At c = -4 (the value the fp64-only scaler tests use) a correct fp32
    evaluation of plain predict (parity.apply32_model of the oracle's Phi, alpha, Li at these geometries) already stands at 0.5 to 1.6
    of that bound, against 0.1 to 0.3 at c = -0.6, so a miss there would say nothing about the call under test."""
    p = O.init_params(D, S, M, rng)
    p[0] = -0.4 + 0.2 * rng.standard_normal(); p[1] = 0.1; p[2] = -0.6; p[3:3 + D * S] *= 0.6
    return p


class Fit(object):
    """CPU-side model of the fit: raw rows in it, parameters, scalers, and the oracle's factors on those rows"""

    def __init__(self, D, S, M):
        self.D, self.S, self.M = D, S, M
        self.params = None; self.xs = None; self.ys = None
        self.Xraw = None; self.yraw = None
        self.options = {}
        self.resident = None                  # (X, y) scaled, as last given to set_data
        self.resident_in_fit = False
        self._cache = None

    def touch(self):
        self._cache = None

    def fx(self, Xraw):
        return np.ascontiguousarray(self.xs.forward_transform(Xraw))

    def fy(self, yraw):
        """scaled targets: the y scaler's forward transform, a fixed affine map while none is registered"""
        if self.ys is None:
            return (np.asarray(yraw) - 1.1) / 0.4
        return np.ascontiguousarray(self.ys.forward_transform(np.asarray(yraw).reshape(-1, 1)))

    def X(self):
        return self.fx(self.Xraw)

    def y(self):
        return self.fy(self.yraw)

    def factors(self):
        if self._cache is None:
            _, a, L = O.forward(self.X(), self.y(), self.params, self.S, self.M, gauss_hermite=False)
            self._cache = (a, L)
        return self._cache


# ---- the references behind HipEngine's interface -----------------------------------------------------------------------------------------
def y_tail(ys, mu, sd):
    """the host tail of SCFGP.predict as tests/test_gpu_parity.py writes it: (mu_y (T,1), std_y (T,1))"""
    mu = np.asarray(mu, np.float64).reshape(-1, 1); sd = np.asarray(sd, np.float64).reshape(-1, 1)
    with np.errstate(all='ignore'):
        return ys.backward_transform(mu), 0.5 * (ys.backward_transform(mu + sd) - ys.backward_transform(mu - sd))


def y_metrics(mu_h, sd_h, ys_raw):
    with np.errstate(all='ignore'):
        err = mu_h - ys_raw
        mae, mse = np.mean(np.abs(err)), np.mean(err ** 2.)
        mnlp = 0.5 * np.mean((err / sd_h) ** 2 + np.log(2 * np.pi * sd_h ** 2))
        nmse = mse / np.var(ys_raw)
        return np.array([mae, mae / np.std(ys_raw), mse, nmse, mnlp, nmse / (1 + np.exp(-mnlp))])


def bw(ys, f):
    f = np.asarray(f, np.float64)
    with np.errstate(all='ignore'):
        return ys.backward_transform(f.reshape(-1, 1)).reshape(f.shape)


def _finite(*arrays):
    return all(np.all(np.isfinite(a)) for a in arrays if a is not None)


class RefEngine(object):
    """tests/*_ref.py and the oracle behind the methods of HipEngine that the sequences call"""
    METRICS = ('MAE', 'NMAE', 'MSE', 'NMSE', 'MNLP', 'SCORE')
    ROW_BITS = False                          # numpy's products promise no bits of a row across row counts: (c) is checked to 1e-10 here

    def __init__(self, D, S, M, dtype='f64'):
        self.D, self.S, self.M = D, S, M
        self.K = 2 * (S + M)
        self.params = None; self.xs = None; self.ys = None; self.Xd = None; self.yd = None; self._opt = None

    def close(self):
        pass

    def dims(self):
        ru = lambda v, m: (v + m - 1) // m * m
        k64 = ru(self.K, 64)
        return dict(K=self.K, Kp=(k64 // 128 + k64 // 64 % 2) * 128, Jp=ru(self.K // 2, 128), Dp=ru(self.D + 1, 16), Sp=ru(self.S + 1, 16))

    # state
    def set_params(self, p):
        self.params = np.array(p, np.float64)

    def get_params(self):
        return self.params.copy()

    def set_data(self, X, y):
        self.Xd, self.yd = np.array(X), np.array(y)

    def set_option(self, name, value):
        pass

    def set_x_scaler(self, s):
        self.xs = s

    def set_y_scaler(self, s):
        self.ys = s

    # training
    def eval(self, want_grad=True):
        c, g, a, L = O.value_and_grad(self.Xd, self.yd, self.params, self.S, self.M)
        return np.array(c), (g if want_grad else None), a, L

    def eval_rows(self, idx, want_grad=True):
        c, g, a, L = O.value_and_grad(self.Xd[idx], self.yd[idx], self.params, self.S, self.M)
        return np.array(c), (g if want_grad else None), a, L

    def opt_init(self, algo, learning_rate=0.01):
        self._opt = float(learning_rate)

    def train(self, n):
        """n plain Adam iterations on the oracle's gradient"""
        m = np.zeros_like(self.params); v = np.zeros_like(self.params); hist = np.empty(n)
        for t in range(1, n + 1):
            c, g, a, L = O.value_and_grad(self.Xd, self.yd, self.params, self.S, self.M)
            hist[t - 1] = c
            m = 0.9 * m + 0.1 * g; v = 0.999 * v + 0.001 * g * g
            self.params = self.params - self._opt * (m / (1 - 0.9 ** t)) / (np.sqrt(v / (1 - 0.999 ** t)) + 1e-8)
        return hist, a, L

    # rows of a mode
    def _rows(self, X, mode):
        """(scaled rows, d scaled / d raw per kept column or None, kept columns or None, number of input columns)"""
        X = np.asarray(X, np.float64)
        if mode in ('scaled', False, 0):
            return X, None, None, X.shape[1]
        if self.xs is None:
            raise ValueError('no X scaler')
        return np.ascontiguousarray(self.xs.forward_transform(X)), G.x_scaler_deriv(self.xs, X), list(self.xs.data['cols']), X.shape[1]

    @staticmethod
    def _chain(g, J, cols, width):
        if J is None:
            return g
        out = np.zeros((g.shape[0], width)); out[:, cols] = g * J
        return out

    def _need_y(self):
        if self.ys is None:
            raise ValueError('no y scaler')

    # the predict family
    def predict(self, Xs, alpha, Li):
        return O.predict(Xs, alpha, Li, self.params, self.S, self.M)

    def predict_raw(self, Xs, alpha, Li):
        return O.predict(self._rows(Xs, 'raw')[0], alpha, Li, self.params, self.S, self.M)

    def predict_y(self, Xs, alpha, Li, ys=None):
        self._need_y()
        mu, sd = self.predict_raw(Xs, alpha, Li)
        mu_h, sd_h = y_tail(self.ys, mu, sd)
        met = None if ys is None else dict(zip(self.METRICS, y_metrics(mu_h, sd_h, np.asarray(ys).reshape(-1, 1)).tolist()))
        return mu_h, sd_h, met

    def predict_grad(self, Xs, alpha, Li, mode='scaled', want_std=True):
        X, J, cols, width = self._rows(Xs, 'scaled' if mode == 'scaled' else 'raw')
        mu, sd, dmu, dsd = G.predict_grad(X, alpha, Li, self.params, self.S, self.M)
        dmu, dsd = self._chain(dmu, J, cols, width), self._chain(dsd, J, cols, width)
        if mode == 'y':
            self._need_y()
            with np.errstate(all='ignore'):
                dmu, dsd = G.y_chain(self.ys, mu, sd, dmu, dsd)
            mu, sd = y_tail(self.ys, mu, sd); sd = sd.ravel()
        return mu, sd, dmu, (dsd if want_std else None)

    def gradcov_points_per_chunk(self, want_cov):
        return gradcov_points_per_chunk(self.D, self.S, want_cov)

    def predict_gradcov(self, Xs, alpha, Li, w=None, mode='scaled', want=('dmu', 'dvar', 'asub')):
        """tests/gradcov_ref.py's dense closed form, 256 rows at a time (the T x K x D Jacobian of a long call does not fit); raw mode
        chained as g o m and diag(g) Sigma diag(g).  dmu is this engine's predict_grad's (the header's promise 1); Sigma_t and asub are
        made symmetric, which the closed form's products are up to their last bits."""
        want = (want,) if isinstance(want, str) else tuple(want)
        if mode not in ('scaled', 'raw') or not want or any(k not in T_GC.ALL for k in want):
            raise ValueError('predict_gradcov: bad mode or want')
        X, J, cols, width = self._rows(Xs, mode)
        T, D = X.shape
        wv = np.ones(T)
        if 'asub' in want and w is not None:
            wv = np.asarray(w, np.float64).reshape(-1)
            if wv.size != T or not np.all(np.isfinite(wv)) or np.any(wv < 0) or not wv.sum() > 0:
                raise ValueError('predict_gradcov: a negative or non-finite weight, or weights that sum to zero')
        dv = np.empty((T, D)); dc = np.empty((T, D, D)) if 'dcov' in want else None; acc = np.zeros((D, D))
        if set(want) - {'dmu'}:
            with np.errstate(all='ignore'):
                for t0 in range(0, T, 256):
                    sl = slice(t0, min(T, t0 + 256))
                    m, Sig = GC.gradcov(X[sl], alpha, Li, self.params, self.S, self.M, g=None if J is None else J[sl])
                    Sig = 0.5 * (Sig + Sig.transpose(0, 2, 1))
                    dv[sl] = np.diagonal(Sig, axis1=1, axis2=2)
                    if dc is not None:
                        dc[sl] = Sig
                    if 'asub' in want:
                        acc += np.einsum('t,tde->de', wv[sl], m[:, :, None] * m[:, None, :] + Sig)

        def wide(a, matrix=False):
            if cols is None:
                return a
            o = np.zeros(a.shape[:-1] + (width,)); o[..., cols] = a
            if matrix:                                                       # rows of the matrices too
                b = np.zeros(o.shape[:-2] + (width, width)); b[..., cols, :] = o
                o = b
            return o

        out = {}
        if 'dmu' in want:
            out['dmu'] = self.predict_grad(Xs, alpha, Li, mode=mode, want_std=False)[2]
        if 'dvar' in want:
            out['dvar'] = wide(dv)
        if 'dcov' in want:
            out['dcov'] = wide(dc, True)
        if 'asub' in want:
            A_ = acc / wv.sum()
            out['asub'] = wide(0.5 * (A_ + A_.T), True)
        return out

    def pd_scaled(self, Xs, dims, grid, mode):
        """the arguments of predict_pd in scaled units: (rows, dims as scaled columns, grid); in raw mode every grid value goes through
        the X scaler's forward transform of its own column, on the host"""
        dims = [int(d) for d in np.asarray(dims).reshape(-1)]
        grid = np.asarray(grid, np.float64)
        if grid.ndim != 2 or grid.shape[0] != len(dims) or len(set(dims)) != len(dims):
            raise ValueError('predict_pd: grid must be (ndim, G) with one row per distinct entry of dims')
        X = self._rows(Xs, mode)[0]
        if mode == 'scaled':
            if any(not 0 <= d < X.shape[1] for d in dims):
                raise ValueError('predict_pd: dimension out of range')
            return X, dims, grid
        Xr = np.asarray(Xs, np.float64)
        kept = list(self.xs.data['cols'])
        if any(d not in kept for d in dims):
            raise ValueError('predict_pd: dims names a column that the X scaler dropped or that does not exist')
        fin = np.flatnonzero(np.isfinite(Xr).all(axis=1))
        base = Xr[fin[0]] if fin.size else np.ones(Xr.shape[1])
        out = np.empty_like(grid)
        with np.errstate(all='ignore'):
            for a, cc in enumerate(dims):
                fake = np.repeat(base[None, :], grid.shape[1], 0); fake[:, cc] = grid[a]
                out[a] = self.xs.forward_transform(fake)[:, kept.index(cc)]
        return X, [kept.index(d) for d in dims], out

    def predict_pd(self, Xs, alpha, Li, dims, grid, w=None, mode='scaled', want=('pd', 'sd')):
        """tests/pd_ref.py's closed form (pinned to its brute force by tests/test_pd_ref.py); cov is made symmetric, which the closed
        form's product is up to its last bits"""
        want = (want,) if isinstance(want, str) else tuple(want)
        if mode not in ('scaled', 'raw') or not want or any(k not in T_PD.ALL for k in want):
            raise ValueError('predict_pd: bad mode or want')
        X, dims, grid = self.pd_scaled(Xs, dims, grid, mode)
        live = np.ones(len(X), bool)
        if w is not None:
            w = np.asarray(w, np.float64).reshape(-1)
            if w.size != len(X) or np.any(w < 0) or (np.all(np.isfinite(w)) and not np.any(w > 0)):
                raise ValueError('predict_pd: a negative weight, or no row of positive weight')
            if not np.all(np.isfinite(w)):
                raise FloatingPointError('predict_pd: non-finite weights')
            live = w > 0
        if not _finite(grid):
            raise FloatingPointError('predict_pd: non-finite grid')
        if set(want) - {'ice'} and not _finite(X[live]):
            raise FloatingPointError('predict_pd: non-finite weighted sum of the features')
        with np.errstate(all='ignore'):
            pd, sd, cov, ice, _ = PD.closed(X, w, alpha, Li, self.params, self.S, self.M, dims, grid, want_ice='ice' in want)
        out = dict(pd=pd, sd=sd, cov=0.5 * (cov + cov.transpose(0, 2, 1)), ice=ice)
        return {k: out[k] for k in T_PD.ALL if k in want}

    # samples
    def sample_weights(self, alpha, Li, nsamp, seed=0):
        return SR.weights(alpha, Li, kappa(self.params), nsamp, seed)

    def sample(self, Xs, alpha, Li, nsamp, seed=0, mode='scaled', noise=False):
        X = self._rows(Xs, 'scaled' if mode == 'scaled' else 'raw')[0]
        with np.errstate(all='ignore'):
            f = SR.samples(X, alpha, Li, self.params, self.S, self.M, nsamp, seed, noise=noise)
        if mode == 'y':
            self._need_y()
            f = bw(self.ys, f)
        return f

    def sample_argmax(self, Xs, alpha, Li, nsamp, seed=0, w=None, mode='scaled', minimize=False):
        out = self.sample(Xs, alpha, Li, nsamp, seed, mode='scaled' if mode == 'scaled' else 'raw')
        rows = slice(None) if w is None else np.asarray(w) > 0
        if not _finite(out[rows]):
            raise FloatingPointError('sample_argmax: non-finite value of an eligible row')
        idx, val = AM.argmax(out, w, minimize)
        if mode == 'y':
            self._need_y()
            val = bw(self.ys, val)
        return idx, val

    def sample_grad(self, Xs, W, sidx=None, mode='scaled', want_val=True):
        X, J, cols, width = self._rows(Xs, 'scaled' if mode == 'scaled' else 'raw')
        val, grad = SG.sample_grad(X, W, sidx, self.params, self.S, self.M)
        grad = self._chain(grad, J, cols, width)
        if mode == 'y':
            self._need_y()
            with np.errstate(all='ignore'):
                grad = G.y_backward_deriv(self.ys, val)[:, None] * grad
            val = bw(self.ys, val)
        return (val if want_val else None), grad

    def acquire(self, Xs, alpha, Li, kind, best=None, xi=0.0, beta=None, fstar=None, w=None, mode='scaled', noise=False, minimize=False,
                want=('acq', 'argmax')):
        X, J, cols, width = self._rows(Xs, mode)
        mu, sd_star, dmu, dsd = G.predict_grad(X, alpha, Li, self.params, self.S, self.M)
        kap = kappa(self.params)
        v = sd_star ** 2 / kap - 1.0 if noise else np.sum(pred_cov_ref.factor(X, Li, self.params, self.S, self.M) ** 2, axis=1)
        sd = sd_star if noise else A.sigma(kap, v, False)
        kw = {'ucb': dict(beta=beta), 'mes': dict(fstar=fstar)}.get(kind, dict(best=best, xi=xi))
        acq, au, as_ = A.acquire(kind, mu.ravel(), sd, minimize=minimize, **kw)
        out = {}
        if 'acq' in want:
            out['acq'] = acq
        if 'argmax' in want:
            out['idx'] = A.argmax(acq, w); out['val'] = float(acq[out['idx']])
        if 'mu' in want:
            out['mu'] = mu.ravel()
        if 'sd' in want:
            out['sd'] = sd
        if 'grad' in want:
            dsig = dsd if noise else dsd * (sd_star / sd)[:, None]
            out['grad'] = self._chain((-1.0 if minimize else 1.0) * au[:, None] * dmu + as_[:, None] * dsig, J, cols, width)
        return out

    def acquire_kg(self, Xc, alpha, Li, Xr=None, z=None, w=None, mode='scaled', noise=True, minimize=False, want=('kg', 'idx', 'val')):
        """tests/kg_ref.py's restatement on the lines of this engine's own predict_cov, predict and sigma (the calls the records form the
        device's lines from)"""
        z = KG.check_nodes(KG.DEFAULT_NODES if z is None else z)
        Xb = Xc if Xr is None else Xr
        cov = self.predict_cov(Xc, Li, Xb=Xb, mode=mode)
        mu_r = (self.predict if mode == 'scaled' else self.predict_raw)(Xb, alpha, Li)[0].ravel()
        sd = self.acquire(Xc, alpha, Li, 'ucb', beta=0.0, mode=mode, noise=noise, want=('acq', 'sd'))['sd']
        m, s, lo, hi = KG.node_table(KG.offsets(mu_r, minimize), KG.slopes(cov, sd), z)
        kg, kg_hi = KG.bounds(m, s, lo, hi, z)
        out = dict(kg=kg, kg_hi=kg_hi, m=m, s=s, idx=int(KG.argmax(kg, w)))
        out['val'] = float(kg[out['idx']])
        return {k: v for k, v in out.items() if k in want}

    def predict_cov(self, Xa, Li, Xb=None, mode='scaled', noise=False):
        Xa = self._rows(Xa, mode)[0]
        Xb = None if Xb is None else self._rows(Xb, mode)[0]
        return pred_cov_ref.pred_cov(Xa, Li, self.params, self.S, self.M, Xb=Xb, noise=noise)

    # moving the fit
    def condition(self, Xn, yn, alpha, Li, mode='scaled'):
        if not _finite(Xn, yn, alpha, Li):
            raise FloatingPointError('condition: non-finite input')
        return condition_ref.condition(self._rows(Xn, mode)[0], yn, alpha, Li, self.params, self.S, self.M)

    FORGET_STATS = ('n', 'sum_e2', 'sum_abs_e', 'sum_log_marginal', 'log_joint', 'min_pivot2', 'blocks')

    def forget(self, X, y, alpha, Li, factors=True, predict=False, mode='scaled'):
        if not _finite(X, y, alpha, Li):
            raise FloatingPointError('forget: non-finite input')
        r = forget_ref.forget(self._rows(X, mode)[0], y, alpha, Li, self.params, self.S, self.M)
        out = (r['alpha'], r['Li']) if factors else ()
        if predict:
            st = dict(zip(self.FORGET_STATS, r['stats'].tolist())); st['n'] = int(st['n']); st['blocks'] = int(st['blocks'])
            e = np.asarray(y, np.float64).ravel() - r['mu']         # the device forms these two in row order, one thread
            st['sum_e2'] = functools.reduce(lambda s, v: s + v, (e * e).tolist(), 0.0)
            st['sum_abs_e'] = functools.reduce(lambda s, v: s + v, np.abs(e).tolist(), 0.0)
            out = out + (r['mu'].reshape(-1, 1), r['std'], st)
        return out

    LOO_STATS = ('n', 'sum_e2', 'sum_abs_e', 'sum_log_marginal', 'sum_log_joint', 'max_leverage', 'blocks')

    def loo(self, X=None, y=None, alpha=None, Li=None, block=1, mode='scaled'):
        if X is None:
            X, y = self.Xd, self.yd
        else:
            X = self._rows(X, mode)[0]
        if not _finite(X, y, alpha, Li):
            raise FloatingPointError('loo: non-finite input')
        r = loo_ref.loo(X, y, alpha, Li, self.params, self.S, self.M, block)
        st = dict(zip(self.LOO_STATS, r['stats'].tolist())); st['n'] = int(st['n']); st['blocks'] = int(st['blocks'])
        if block == 1:
            st['sum_log_joint'] = st['sum_log_marginal']            # the header: block 1, the same number bit for bit
        return r['mu'].reshape(-1, 1), r['std'], r['lev'], st

    # selection
    def select(self, Xc, Li, m, w=None, raw=False, return_std=False):
        C = pred_cov_ref.factor(self._rows(Xc, 'raw' if raw else 'scaled')[0], Li, self.params, self.S, self.M)
        r = R.select(C, m, w=w, kap=kappa(self.params))
        return (r['idx'], r['var'], r['gain']) + ((r['std_after'],) if return_std else ())

    def select_iv(self, Xc, Li, m, Xr=None, w=None, wr=None, raw=False, return_std=False):
        mode = 'raw' if raw else 'scaled'
        C = pred_cov_ref.factor(self._rows(Xc, mode)[0], Li, self.params, self.S, self.M)
        CR = C if Xr is None else pred_cov_ref.factor(self._rows(Xr, mode)[0], Li, self.params, self.S, self.M)
        r = V.select(C, V.gram(CR, wr), m, w=w, kap=kappa(self.params))
        return (r['idx'], r['red'], r['var'], r['ivar']) + ((r['std_after'],) if return_std else ())

    def select_qei(self, Xc, alpha, Li, m, nsamp, best, xi=0.0, seed=0, w=None, pending=None, mode='scaled', minimize=False,
                   return_score0=False, return_state=False):
        F = self.sample(Xc, alpha, Li, nsamp, seed, mode=mode)
        P = None if pending is None or len(pending) == 0 else self.sample(pending, alpha, Li, nsamp, seed, mode=mode)
        idx, gain, score0, mstate, qei = Q.greedy(F, m, best, xi, w, P, minimize)
        return (idx, gain, qei) + ((score0,) if return_score0 else ()) + ((mstate,) if return_state else ())


# ---- schedules -------------------------------------------------------------------------------------------------------------------------
OLD_POSTERIOR = POSTERIOR[:15]                                           # the entry points the sequences held before the last three joined
NEWEST = POSTERIOR[15:]


def _posterior_block(ep, rng, T=None):
    """one posterior step, or a raw-mode step and the y-mode step that is checked against it"""
    st = dict(op='post', ep=ep, T=int(rng.choice(SIZES)) if T is None else int(T), seed=int(rng.integers(1, 2 ** 31)), u=float(rng.random()))
    st['mode'] = str(rng.choice(['scaled', 'raw']))
    if ep == 'predict':
        st['mode'] = 'scaled'
    elif ep in ('predict_raw', 'predict_y'):
        st['mode'] = 'raw'
    st['mask'] = bool(rng.integers(2)); st['minimize'] = bool(rng.integers(2)); st['noise'] = bool(rng.integers(2))
    st['nsamp'] = int(rng.choice(NSAMP)); st['m'] = int(rng.choice(PICKS)); st['block'] = int(rng.integers(1, 65))
    st['flag'] = bool(rng.integers(2))         # want_std / want_val / targets given / cross form / explicit reference / pending / resident
    st['kind'] = str(rng.choice(A.KINDS))
    if ep == 'predict_y':
        return [dict(st, ep='predict_raw'), dict(st, mode='y')]
    if ep in Y_MODE and rng.integers(3) == 0:
        return [dict(st, mode='raw', pair=True), dict(st, mode='y', pair=True)]
    return [st]


def _newest_block(ep, rng, T=None):
    """one step of predict_gradcov, predict_pd or acquire_kg: _posterior_block's draw from the generator of the new blocks, and the
    options of these three.  predict_gradcov, predict_pd: weights by `mask`, all four outputs or the two cheap ones by `flag`; predict_pd's
    grid and dimensions.  acquire_kg: reference rows and nodes; the candidates are their own reference set up to 700 rows only (the
    reference's node table is T x R per node).  `new` marks the steps that were not in the schedules before these three joined; `redraw`
    those whose draw is repeated at run time until their input condition holds (materialise)."""
    st = _posterior_block(ep, rng, T)[0]
    st['G'] = int(rng.choice(GRID)); st['pdims'] = str(rng.choice(['all', 'one']))
    st['R'] = int(rng.choice(KG_REFS)); st['nodes'] = KG_NODES[int(rng.integers(len(KG_NODES)))]
    if st['R'] == 0 and st['T'] > 700:
        st['R'] = KG_REFS[1]
    st['new'] = True
    if ep in ('acquire_kg', 'predict_pd'):
        st['redraw'] = True
    return [st]


def _failing_blocks(rng):
    """documented error returns, each followed directly by a valid call of another entry point that shares its buffers"""
    seed = lambda: int(rng.integers(1, 2 ** 31))
    base = dict(op='post', mode='scaled', mask=False, minimize=False, noise=False, nsamp=7, m=5, block=7, flag=False, kind='ei', u=0.5)
    fail = lambda ep, err, T, **kw: dict(base, op='fail', ep=ep, err=err, T=T, seed=seed(), **kw)
    ok = lambda ep, T, **kw: dict(base, ep=ep, T=T, seed=seed(), **kw)
    return [
        [fail('forget', 'nonfinite', 257), ok('condition', 37)],
        [fail('loo', 'notpd', 64), ok('predict_grad', 255, flag=True)],
        [fail('predict_cov', 'arg', 37, noise=True), ok('loo', 256)],
        [ok('sample', 700, nan_row=True), fail('sample_argmax', 'nonfinite', 700), ok('acquire', 257, flag=True)],
    ]


def _newest_failing_blocks(rng):
    """the same for predict_gradcov and predict_pd, from the generator of the new blocks"""
    seed = lambda: int(rng.integers(1, 2 ** 31))
    base = dict(op='post', mode='scaled', mask=False, minimize=False, noise=False, nsamp=7, m=5, block=7, flag=False, kind='ei', u=0.5,
                G=9, pdims='all', R=37, nodes=None, new=True)
    fail = lambda ep, err, T, **kw: dict(base, op='fail', ep=ep, err=err, T=T, seed=seed(), **kw)
    ok = lambda ep, T, **kw: dict(base, ep=ep, T=T, seed=seed(), **kw)
    return [
        # weights that sum to 0, then the sibling block kernel
        [fail('predict_gradcov', 'arg', 257, flag=True), ok('loo', 256)],
        # a NaN in a row of positive weight, found on the device; then the product of the ICE block's shape
        [fail('predict_pd', 'nonfinite', 700, flag=True), ok('sample', 255)],
        # a NaN row is no error of predict_gradcov: it stays in that point's outputs (promise 2)
        [ok('predict_gradcov', 255, nan_row=True, want=('dmu', 'dvar', 'dcov')), ok('predict_cov', 37)],
    ]


def _draw(ci, sub):
    """The blocks of the fifteen older entry points, their order and the head are drawn exactly as before predict_gradcov, predict_pd
    and acquire_kg joined (one generator, the same calls in the same order), so that every older step keeps its arguments, its seed and
    its place among the older steps; none of the new steps moves the fit, so the older steps also see the fit they saw.  The new blocks
    come from a second generator and are inserted into that order, behind the early y scaler and before the closing predict."""
    (D, S, M), dtype = CASES[ci]
    gi = GEOMETRIES.index((D, S, M))
    rng = np.random.default_rng([0x5EC, ci, sub])
    algos = list(Scaler.algos)
    blocks = []
    for ep in OLD_POSTERIOR + ('predict',):
        for _ in range(2):
            blocks.append(_posterior_block(ep, rng))
    for ep, T in BIG_VISITS[gi]:
        if ep in NEWEST:
            continue
        b = _posterior_block(ep, rng, T)[:1]
        b[0].update(nsamp=7, m=5, flag=ep == 'predict_grad', mode='raw' if ep == 'predict_raw' else 'scaled', pair=False)
        blocks.append(b)
    for _ in range(2):
        blocks.append([dict(op='params', seed=int(rng.integers(1, 2 ** 31)))])
    blocks.append([dict(op='xscaler', algo=algos[(ci + 2) % 5])])
    blocks.append([dict(op='yscaler', algo=algos[(ci + 3) % 5])])
    blocks.append([dict(op='yscaler', algo=algos[(ci + 4) % 5])])
    for op in ('data', 'data', 'eval', 'eval', 'rows', 'train', 'option', 'option', 'option'):
        blocks.append([dict(op=op, seed=int(rng.integers(1, 2 ** 31)))])
    blocks += _failing_blocks(rng)
    order = rng.permutation(len(blocks))
    blocks = [blocks[i] for i in order]
    # the first posterior call of this case, and a posterior call at the end (a change is always followed by one)
    k = next(i for i, b in enumerate(blocks) if b[0]['op'] == 'post' and b[0]['ep'] == FIRST[ci] and len(b) == 1 and b[0]['T'] <= 3000)
    blocks.insert(0, blocks.pop(k))
    k = next(i for i in range(len(blocks) - 1, 0, -1) if blocks[i][0]['op'] == 'post' and blocks[i][0]['ep'] == 'predict')
    blocks.append(blocks.pop(k))
    # the first y scaler early, so that the y modes are allowed in most of the schedule
    k = next(i for i, b in enumerate(blocks) if b[0]['op'] == 'yscaler')
    blocks.insert(2, blocks.pop(k))
    # the failing loo before the failing predict_cov's valid loo
    f = {b[0]['ep']: i for i, b in enumerate(blocks) if b[0]['op'] == 'fail'}
    if f['loo'] > f['predict_cov']:
        blocks[f['loo']], blocks[f['predict_cov']] = blocks[f['predict_cov']], blocks[f['loo']]
    head = [dict(op='xscaler', algo=algos[ci % 5]), dict(op='params', seed=int(rng.integers(1, 2 ** 31)), head=True),
            dict(op='data', seed=int(rng.integers(1, 2 ** 31)), N=3000, head=True)]
    # the three newest entry points: twice each, their scripted big visits and their failing blocks, from a generator of their own
    rng2 = np.random.default_rng([0x5ED, ci, sub])
    fresh = []
    for ep in NEWEST:
        for _ in range(2):
            fresh.append(_newest_block(ep, rng2))
    for ep, T in BIG_VISITS[gi]:
        if ep in NEWEST:
            b = _newest_block(ep, rng2, T)
            b[0].update(nsamp=7, m=5, flag=True, mode='scaled', G=5, pdims='all')      # every output; all D = 7 dimensions of predict_pd
            fresh.append(b)
    fresh += _newest_failing_blocks(rng2)
    for b in fresh:
        blocks.insert(int(rng2.integers(3, len(blocks))), b)
    return _resolve(head + [st for b in blocks for st in b], D)


def _resolve(steps, D):
    """walk the schedule with the fit's row count and fix what depends on it: rows of forget (at most a third of the fit) and loo (rows
    of the fit), the resident form of loo, the y modes before a y scaler is registered"""
    N = 0; nres = 0; res_ok = False; has_y = False
    out = []
    for st in steps:
        st = dict(st)
        op = st['op']
        if op == 'data':
            st.setdefault('N', int(np.random.default_rng(st['seed']).choice([257, 700, 1500, 3000])))
            N = nres = st['N']; res_ok = True
        elif op in ('xscaler', 'yscaler'):
            has_y = has_y or op == 'yscaler'
            nres = N; res_ok = N > 0                             # the scaled rows change: the runner makes the fit resident again
        elif op in ('post', 'fail'):
            ep = st['ep']
            if st['mode'] == 'y' and not has_y:
                st['mode'] = 'raw'
                st['ep'] = ep = 'predict_raw' if ep == 'predict_y' else ep
            if ep == 'forget':
                allowed = [s for s in SIZES if s <= N // 3]
                st['T'] = allowed[int(st['u'] * len(allowed))] if op == 'post' else min(st['T'], N)
                if op == 'post':
                    N -= st['T']; res_ok = False
            elif ep == 'loo' and op == 'post':
                st['resident'] = bool(st['flag'] and res_ok and st['mode'] == 'scaled' and nres <= 3000)
                allowed = [s for s in SIZES if s <= N]
                st['T'] = nres if st['resident'] else allowed[int(st['u'] * len(allowed))]
            elif ep == 'condition' and op == 'post':
                N += st['T']
            elif ep == 'predict_cov':
                st['T'] = min(st['T'], 3000)
        out.append(st)
    return out


def rows_used(st):
    return st['T']


def check_schedule(steps, ci):
    """the coverage conditions every schedule must meet (conditions, not tuning)"""
    post = [st for st in steps if st['op'] == 'post']
    count = {ep: sum(st['ep'] == ep for st in post) for ep in POSTERIOR}
    assert min(count.values()) >= 2, ('every posterior entry point at least twice', count)
    stale = 0
    for prev, st in zip(steps[:-1], steps[1:]):
        if st['op'] == 'post' and prev['op'] in ('post', 'fail') and prev['ep'] != st['ep'] and rows_used(prev) > rows_used(st):
            stale += 1
    assert stale >= 5, ('steps that follow a larger call of another entry point', stale)
    first = next(st for st in steps if st['op'] in ('post', 'fail'))
    assert first['op'] == 'post' and first['ep'] == FIRST[ci], first
    is_post = [st['op'] == 'post' for st in steps]
    for op, least in (('params', 2), ('scaler', 2)):
        at = [i for i, st in enumerate(steps) if (st['op'] == 'params' if op == 'params' else st['op'] in ('xscaler', 'yscaler'))
              and not st.get('head') and any(is_post[:i])]
        assert len(at) >= least, (op, at)
        assert all(any(is_post[:i]) and any(is_post[i + 1:]) for i in at), (op, 'posterior calls before and after')
    fails = [(i, st) for i, st in enumerate(steps) if st['op'] == 'fail']
    assert len(fails) >= 3 and len({st['err'] for _, st in fails}) >= 2, fails
    follow = {'forget': 'condition', 'loo': 'predict_grad', 'predict_cov': 'loo', 'sample_argmax': 'acquire', 'predict_gradcov': 'loo',
              'predict_pd': 'sample'}
    assert set(follow) == {st['ep'] for _, st in fails}
    for i, st in fails:
        nxt = steps[i + 1]
        assert nxt['op'] == 'post' and nxt['ep'] == follow[st['ep']], (st, nxt)
    i = next(i for i, st in fails if st['ep'] == 'sample_argmax')
    assert steps[i - 1]['ep'] == 'sample' and steps[i - 1].get('nan_row')          # a NaN row through `sample`, then the failing call
    i = next(i for i, st in enumerate(steps) if st['op'] == 'post' and st['ep'] == 'predict_gradcov' and st.get('nan_row'))
    assert 'asub' not in steps[i]['want'] and steps[i + 1]['op'] == 'post' and steps[i + 1]['ep'] == 'predict_cov'   # a NaN row that is no error
    assert all(bool(st.get('redraw')) == (st['ep'] in ('acquire_kg', 'predict_pd')) for st in post)
    assert all(bool(st.get('new')) == (st['ep'] in NEWEST) for st in post if st['ep'] in NEWEST + ('acquire', 'predict_raw', 'condition'))
    N = 0
    for st in steps:
        if st['op'] == 'data':
            N = st['N']
        elif st['op'] == 'post' and st['ep'] == 'condition':
            N += st['T']
        elif st['op'] == 'post' and st['ep'] == 'forget':
            assert 1 <= st['T'] <= N // 3, ('forget removes at most a third of the fit', st['T'], N)
            N -= st['T']
    for i, st in enumerate(steps):
        if st['op'] == 'post' and st['mode'] == 'y':
            p = steps[i - 1]
            assert p['op'] == 'post' and p['seed'] == st['seed'] and p['mode'] == 'raw' and p['ep'] == st['ep'].replace('predict_y', 'predict_raw')
    return dict(count=count, stale=stale, steps=len(steps), posterior=len(post))


@functools.lru_cache(maxsize=None)
def make_schedule(ci):
    last = None
    for sub in range(64):
        try:
            steps = _draw(ci, sub)
            check_schedule(steps, ci)
            return steps
        except (AssertionError, StopIteration) as e:
            last = e
    raise AssertionError('no schedule of case %d meets the coverage conditions: %r' % (ci, last))


def check_all_schedules():
    """the conditions that span the cases"""
    scheds = [make_schedule(ci) for ci in range(len(CASES))]
    firsts = [next(st['ep'] for st in s if st['op'] == 'post') for s in scheds]
    assert len(set(firsts)) == len(firsts), firsts
    assert {'predict_grad', 'condition', 'loo', 'forget'} <= set(firsts)      # ensure_pred_factor / _update / _loo / _forget first
    for dt in DTYPES:
        seen = {st['T'] for (g, d), s in zip(CASES, scheds) if d == dt for st in s if st['op'] == 'post'}
        assert set(BIG) <= seen, (dt, sorted(seen))
        big = {(st['ep'], st['T']) for (g, d), s in zip(CASES, scheds) if d == dt for st in s if st['op'] == 'post' and st['flag']}
        assert {('predict_gradcov', BIG_GRADCOV), ('predict_pd', BIG[2])} <= big and BIG_GRADCOV == 16684, (dt, sorted(big))
    algos = {st['algo'] for s in scheds for st in s if st['op'] in ('xscaler', 'yscaler')}
    assert algos == set(Scaler.algos)
    return scheds


# ---- the geometry sweep -------------------------------------------------------------------------------------------------------------------
# What a posterior call launches depends on a few integer classes of (D, S, M); this set visits the classes the sequences above never
# reach (tests/test_posterior_geometry_ref.py asserts that it covers them, tests/test_gpu_posterior_geometry.py runs it).  M = 1 is left
# out on purpose: at (1, 1, 1) the oracle's penalty takes the log of a zero variance and the cost is infinite.
SWEEP_GEOMETRIES = [
    (1, 2, 2),        # K = 8:   D = 1; the smallest K of the training tests; one 64-tile, strip only
    (7, 12, 3),       # K = 30:  M < S
    (70, 5, 60),      # K = 130: 3 tiles, 2 live columns in the last, 4 partial slots; Dp = 80 > 64; rank-S projection live
    (15, 15, 60),     # K = 150: D + 1 = Dp = 16 and S + 1 = Sp = 16 exactly
    (16, 16, 70),     # K = 172: one past both (Dp = Sp = 32)
    (6, 5, 91),       # K = 192: 3 full 64-tiles, the fourth block all padding
    (9, 8, 120),      # K = 256: the last small plan; K = Kp; J = Jp = 128
    (40, 6, 123),     # K = 258: the first 128-wide plan; remainder tile with 2 live columns; J = 129 -> Jp = 256; rank-S live
    (33, 3, 158),     # K = 322: remainder of two 64-tiles, the second with 2 live columns
    (5, 4, 188),      # K = 384: 128-wide plan with no remainder launch; K = Kp
]
SWEEP_ENTRY_POINTS = ('predict',) + POSTERIOR                            # all nineteen
SWEEP_OLD_GROUPS = (2, 40)                                               # first and last group of the seventeen older entry points
SWEEP_GRID = (9, 1)                                                      # grid values of the two predict_pd groups
SWEEP_T = (257, 1)                                                       # one row past the 256-row padding, and its row 0 alone
SWEEP_N = 300                                                            # rows in the fit
SWEEP_MOVED = (1, 37)                                                    # rows condition and forget move; R of acquire_kg; pending / Xb rows


# The seed of a group of steps of a geometry's schedule is drawn from (D, S, M, the group's number, its salt).  An output bounded relative to its own norm is a fair check only
# where that norm is not a cancellation: row 0 alone may hold one number (one sample, D = 1) that happens to lie near 0 while the error
# of its sum does not shrink with it.  A group's salt is the first for which conditioned_row0 holds for every such record of its steps,
# a correct fp32 predict stands inside half its bound, and acquire's gradient terms do not cancel (acquire_grad_cancellation);
# and the lines of an acquire_kg step on 257 rows are not near-parallel (kg_conditioning <= 1; at D = 1, K = 8 no draw of the step with
# 37 reference rows meets it, and that step is exempt); tests/test_posterior_geometry_ref.py asserts all of it on the CPU references.  These are conditions on the choice of inputs, computed from the fp64 references alone, not tolerances.
# The groups of predict_gradcov and predict_pd (41 to 44) are held to conditioned_row0 for dmu, dvar, dcov and ice, to pd_cancellation >=
# PD_CANCEL, and to a correct fp32 evaluation of every one of their steps (row 0 alone included) inside half the fp32 bound; only the
# first of the three ever turned a salt down.  No step of either entry point is exempt.
# (D, S, M) -> {group number: salt}; every other group: 0
_SALT = {
    (1, 2, 2): {0: 1, 5: 1, 6: 1, 15: 1, 16: 1, 18: 13, 19: 1, 21: 13, 24: 237, 34: 1, 35: 2},
    (7, 12, 3): {12: 1, 14: 2, 18: 2, 21: 6, 22: 9},
    (70, 5, 60): {6: 3, 13: 1, 14: 1, 16: 2, 21: 2, 22: 1, 41: 1},
    (15, 15, 60): {18: 1, 19: 1, 21: 10, 22: 1},
    (16, 16, 70): {12: 1, 14: 2, 16: 2, 19: 2, 21: 14, 22: 6, 24: 1, 44: 1},
    (6, 5, 91): {4: 2, 6: 6, 14: 1, 15: 3, 16: 8, 17: 1, 20: 2, 21: 4, 41: 3, 42: 3},
    (9, 8, 120): {14: 1, 15: 3, 16: 2, 21: 1, 35: 1, 42: 9},
    (40, 6, 123): {10: 1, 12: 1, 13: 1, 14: 2, 18: 2, 21: 11, 22: 8, 35: 1, 42: 6, 43: 1},
    (33, 3, 158): {4: 2, 5: 1, 6: 3, 10: 1, 14: 2, 15: 3, 16: 5, 18: 5, 19: 2, 20: 3, 21: 8, 22: 2, 41: 1, 42: 10},
    (5, 4, 188): {4: 4, 6: 2, 16: 4, 17: 2, 20: 3, 21: 2, 41: 2, 42: 20},
}
SWEEP_SALT = {g + (n,): v for g, d in _SALT.items() for n, v in d.items()}
ROW0_NORM = 0.5


def conditioned_row0(ref_row0, ref_big):
    """the reference of a norm-relative record of a step on row 0 alone holds at least ROW0_NORM of the rms row norm of the same record of
    the 257-row step: the smaller check is then at most 1 / ROW0_NORM times as tight as the larger one (None: the two are not
    row-aligned, as the symmetric covariance, whose 1 x 1 form is a variance)"""
    r = np.asarray(ref_row0, np.float64); b = np.asarray(ref_big, np.float64)
    if r.ndim == 0 or b.ndim == 0 or r.size == 0 or r.shape[1:] != b.shape[1:] or b.shape[0] <= r.shape[0]:
        return None
    fin = np.isfinite(b).reshape(len(b), -1).all(axis=1)
    if not fin.any() or not np.isfinite(r).all():
        return None
    rms = float(np.linalg.norm(b[fin])) / np.sqrt(fin.sum() / len(r))
    return bool(float(np.linalg.norm(r)) >= ROW0_NORM * rms)


GRAD_CANCEL = 2.0


def acquire_grad_cancellation(a, fit):
    """(|a_u d mu| + |a_sigma d sigma|) / |a_u d mu + a_sigma d sigma| in norm over the step's rows, from the fp64 references: acquire's
    gradient is a sum of two products, and tests/test_gpu_acquire.py's CHAIN_BOUND (a dozen ulp, norm-wise over thousands of elements)
    is a fair check of a handful of elements only where the two do not cancel.  A condition on the inputs of the steps on row 0 alone:
    at most GRAD_CANCEL."""
    ref = _ref_engine(fit)
    X = ref._rows(a['X'], a['mode'])[0]
    mu, sd_star, dmu, dsd = G.predict_grad(X, a['alpha'], a['Li'], fit.params, fit.S, fit.M)
    sd = sd_star if a['noise'] else A.sigma(kappa(fit.params), np.sum(pred_cov_ref.factor(X, a['Li'], fit.params, fit.S, fit.M) ** 2, axis=1), False)
    kw = {'ucb': dict(beta=a['beta']), 'mes': dict(fstar=a['fstar'])}.get(a['kind'], dict(best=a['best'], xi=a['xi']))
    _, au, as_ = A.acquire(a['kind'], mu.ravel(), sd, minimize=a['minimize'], **kw)
    t1 = au[:, None] * dmu; t2 = as_[:, None] * (dsd if a['noise'] else dsd * (sd_star / sd)[:, None])
    s = float(np.linalg.norm((-1.0 if a['minimize'] else 1.0) * t1 + t2))
    return float(np.linalg.norm(np.abs(t1) + np.abs(t2))) / s if s > 0 else np.inf


def kg_conditioning(a, fit):
    """acquire_kg's sums are compared with tests/kg_ref.py's at the device's own node table in the measure max |delta| / max kg_hi under
    tests/test_gpu_acquire_kg.py's VALUE_BOUND.  Both form J chord slopes q_j = (m_j+1 - m_j) / (z_j+1 - z_j) of size up to max |b| and
    sum their DIFFERENCES, weighted by h(-|z_j|) <= h(0) < 0.4: one ulp of a quotient (another division, a fused multiply-add) moves a
    sum by up to J 0.4 u max |b|, whatever the sums are.  Where the lines of the reference rows are nearly parallel (few features, D = 1)
    max kg_hi is far smaller than max |b| and that measure is no check of the kernel.  Returns J 0.4 u max |b| / (VALUE_BOUND max kg_hi)
    from the fp64 references: a condition on the inputs, at most 1 (0 where R = 1: both sums are exactly 0)."""
    ref = _ref_engine(fit)
    z = KG.DEFAULT_NODES if a['z'] is None else a['z']
    Xb = a['X'] if a['Xr'] is None else a['Xr']
    if len(Xb) == 1:
        return 0.0
    cov = ref.predict_cov(a['X'], a['Li'], Xb=Xb, mode=a['mode'])
    sd = ref.acquire(a['X'], a['alpha'], a['Li'], 'ucb', beta=0.0, mode=a['mode'], noise=a['noise'], want=('acq', 'sd'))['sd']
    hi = ref.acquire_kg(a['X'], a['alpha'], a['Li'], Xr=a['Xr'], z=a['z'], mode=a['mode'], noise=a['noise'], minimize=a['minimize'],
                        want=('kg_hi',))['kg_hi']
    return float(len(z) * 0.4 * 2.0 ** -53 * np.abs(KG.slopes(cov, sd)).max() / (T_KG.VALUE_BOUND * hi.max()))


PD_CANCEL = 0.08


def pd_cancellation(a, fit):
    """tests/pd_ref.py's cancellation of a predict_pd step with sums: how much of a feature row's norm survives the weighted mean over
    the step's rows.  A condition on the inputs, at least PD_CANCEL (the figure tests/test_pd_ref.py holds the own GPU tests' inputs to):
    pd, sd and cov are bounded relative to their own norms, which is a fair check only where the mean row is no cancellation."""
    X, dims, _ = _ref_engine(fit).pd_scaled(a['X'], a['dims'], a['grid'], a['mode'])
    return PD.cancellation(X, a['w'], fit.params, fit.S, fit.M, dims)


def geometry_classes(D, S, M):
    """the integer classes of a geometry, restated from ApplyPlan (apply.hip) and derive_geom: the column plan of the apply products
    (n128 tiles 128 wide, then n64 tiles 64 wide, `last` live columns in the last 64-wide tile), the padding of K (Kp, gfull, gstrip;
    `slots` = Kp / 64 partial slots against `covered`, the 64-column blocks the plan's tiles span), and the pads of J, D + 1 and S + 1"""
    ru = lambda v, m: (v + m - 1) // m * m
    K = 2 * (S + M); J = S + M
    small = K <= 256
    n128 = 0 if small else K // 128
    n64 = -(-(K - 128 * n128) // 64)
    last = K - 128 * n128 - 64 * (n64 - 1) if n64 else 0
    k64 = ru(K, 64) // 64
    gfull, gstrip = k64 // 2, k64 % 2
    Kp = 128 * (gfull + gstrip)
    Jp, Dp, Sp = ru(J, 128), ru(D + 1, 16), ru(S + 1, 16)
    return dict(K=K, J=J, small=small, n128=n128, n64=n64, last=last, tiles=n128 + n64, covered=2 * n128 + n64, slots=Kp // 64, Kp=Kp,
                gfull=gfull, gstrip=gstrip, Jp=Jp, jpad=Jp - J, Dp=Dp, dpad=Dp - (D + 1), Sp=Sp, spad=Sp - (S + 1), lowrank=Sp < Dp,
                m_lt_s=M < S)


# the classes the set is there for: name -> condition on geometry_classes' dict (D is passed beside it)
SWEEP_CLASSES = {
    'D = 1': lambda c, D: D == 1,
    'K < 42': lambda c, D: c['K'] < 42,
    'K = 8, strip only': lambda c, D: c['K'] == 8 and c['gfull'] == 0 and c['gstrip'] == 1 and c['tiles'] == 1,
    'M < S': lambda c, D: c['m_lt_s'],
    'small plan of three tiles': lambda c, D: c['small'] and c['n64'] == 3 and 128 < c['K'] <= 192,
    'three tiles, 2 live columns in the last, four partial slots': lambda c, D: c['small'] and c['n64'] == 3 and c['last'] == 2 and c['slots'] == 4,
    'three full 64-tiles, the fourth block all padding': lambda c, D: c['small'] and c['n64'] == 3 and c['last'] == 64 and c['slots'] == 4,
    'more partial slots than the plan covers': lambda c, D: c['slots'] > c['covered'],
    'Dp > 64': lambda c, D: c['Dp'] > 64,
    'rank-S projection live, small plan': lambda c, D: c['lowrank'] and c['small'],
    'rank-S projection live, 128-wide plan': lambda c, D: c['lowrank'] and not c['small'],
    'rank-S projection off': lambda c, D: not c['lowrank'],
    'D + 1 = Dp and S + 1 = Sp': lambda c, D: c['dpad'] == 0 and c['spad'] == 0,
    'D + 1 and S + 1 one past the 16 boundary': lambda c, D: c['dpad'] == 15 and c['spad'] == 15,
    'K = 256 = Kp, the last small plan, J = Jp': lambda c, D: c['K'] == 256 and c['small'] and c['Kp'] == 256 and c['jpad'] == 0,
    'K = 258: first 128-wide plan, 2 live remainder columns, J one past Jp': lambda c, D: (c['K'] == 258 and c['n128'] == 2 and c['n64'] == 1
                                                                                         and c['last'] == 2 and c['jpad'] == 127),
    'remainder of two 64-tiles, 2 live columns in the second': lambda c, D: c['n128'] > 0 and c['n64'] == 2 and c['last'] == 2,
    '128-wide plan with no remainder launch, K = Kp': lambda c, D: c['n128'] > 0 and c['n64'] == 0 and c['K'] == c['Kp'],
    'a strip (odd number of 64-blocks)': lambda c, D: c['gstrip'] == 1 and c['gfull'] > 0,
    'no strip': lambda c, D: c['gstrip'] == 0,
    'K <= 256: no f16x3 split products': lambda c, D: c['small'],
    'K > 256: f16x3 split products run': lambda c, D: not c['small'],
}


def classes_of(D, S, M):
    c = geometry_classes(D, S, M)
    return {name for name, cond in SWEEP_CLASSES.items() if cond(c, D)}


# (c) outputs of which include/scfgp_hip.h documents that a row's values depend on that row alone (not on T, the row's position or the
# chunk): sample ("the same functions on any rows", eps by the row's index), sample_grad, acquire, acquire_kg with explicit reference
# rows, predict_cov's element guarantee, loo for rows of the same block (block 1 here), select_qei's scores, predict_gradcov's promise 2
# (dvar, dcov; its dmu is predict_grad's, of which no such promise is made) and predict_pd's promise 5 (ice)
ROW_ALONE = {'sample': ('out',), 'sample_grad': ('val', 'grad'), 'acquire': ('acq', 'mu', 'sd', 'grad'), 'acquire_kg': ('kg', 'kg_hi', 'm', 's'),
             'predict_cov': ('cov',), 'loo': ('mu', 'sd', 'lev'), 'select_qei': ('score0',), 'predict_gradcov': ('dvar', 'dcov'),
             'predict_pd': ('ice',)}
# (d) outputs of which the header says that SCFGP_F16X3 contexts agree with SCFGP_F32 bit for bit (forget: the fp64 first pass and K x K
# stage, i.e. the factors; its mu / std come from predict's pass, for which nothing is claimed)
F16X3_EQUAL = {'sample': ('out',), 'sample_argmax': ('idx', 'val'), 'sample_grad': ('val', 'grad'),
               'acquire': ('acq', 'idx', 'val', 'mu', 'sd', 'grad'), 'acquire_kg': T_KG.ALL, 'predict_cov': ('cov',),
               'condition': ('alpha', 'Li'), 'forget': ('alpha', 'Li'), 'loo': ('mu', 'sd', 'lev', 'stats'),
               'select': ('idx', 'var', 'gain', 'sd'), 'select_iv': ('idx', 'red', 'var', 'ivar', 'sd'),
               'select_qei': ('idx', 'gain', 'qei', 'score0', 'mstate'), 'predict_gradcov': T_GC.ALL, 'predict_pd': T_PD.ALL}


def row_alone(a):
    """does (c) apply to this step"""
    ep = a['ep']
    if ep not in ROW_ALONE:
        return False
    if ep == 'loo':
        return a['block'] == 1 and not a.get('resident')
    if ep == 'acquire_kg':
        return a['Xr'] is not None
    return True


@functools.lru_cache(maxsize=None)
def sweep_schedule(D, S, M):
    """the lean schedule of one geometry, a function of the geometry alone: parameters, 300 rows, an X and a y scaler, then every posterior
    entry point in every mode it has, each at T = 257 and then on row 0 of those rows alone (`row0_of` names the step whose arguments
    the T = 1 step takes row 0 of).  No training calls, option changes or failing calls: the sequences above cover those."""
    count = [0]

    def seed():
        """the seed of the next group of steps: a function of the geometry, the group's number and its salt"""
        n = count[0]; count[0] += 1
        return int(np.random.default_rng([0x6E0, D, S, M, n, SWEEP_SALT.get((D, S, M, n), 0)]).integers(1, 2 ** 31))

    algos = list(Scaler.algos)
    h = D + 3 * S + 7 * M
    steps = [dict(op='xscaler', algo=algos[h % 5]), dict(op='params', seed=seed(), head=True), dict(op='data', seed=seed(), N=SWEEP_N, head=True),
             dict(op='yscaler', algo=algos[(h + 2) % 5])]
    base = dict(op='post', mode='scaled', mask=False, minimize=False, noise=False, nsamp=7, m=5, block=1, flag=False, kind='ei', u=0.5)

    def both(ep, mode='scaled', **kw):
        """the step (mode 'pair': its raw-mode step and the y-mode step checked against it) at T = 257, then on row 0"""
        st = dict(base, ep=ep, group=count[0], seed=seed(), **kw)
        if ep == 'predict_y':
            group = [dict(st, ep='predict_raw', mode='raw'), dict(st, mode='y')]
        elif mode == 'pair':
            group = [dict(st, mode='raw', pair=True), dict(st, mode='y', pair=True)]
        else:
            group = [dict(st, mode=mode)]
        ids = [len(steps) + i for i in range(len(group))]
        steps.extend(dict(g, T=SWEEP_T[0]) for g in group)
        steps.extend(dict(g, T=SWEEP_T[1], row0_of=i) for g, i in zip(group, ids))

    one = lambda ep, T, mode='scaled', **kw: steps.append(dict(base, ep=ep, T=T, mode=mode, group=count[0], seed=seed(), **kw))
    both('predict')
    both('predict_y', flag=True)                                                   # predict_raw, then predict_y with targets
    both('predict_grad', flag=True); both('predict_grad', flag=False); both('predict_grad', 'pair', flag=True)
    for ns in (1, 7):
        one('sample_weights', 1, nsamp=ns)
    both('sample', nsamp=7, noise=True); both('sample', 'raw', nsamp=1); both('sample', 'pair', nsamp=7)
    both('sample_argmax', nsamp=7, mask=True); both('sample_argmax', 'pair', nsamp=1, minimize=True)
    both('sample_grad', nsamp=7, flag=True, noise=True); both('sample_grad', 'raw', nsamp=7); both('sample_grad', 'pair', nsamp=1)
    for i, kind in enumerate(A.KINDS):
        both('acquire', ('scaled', 'raw')[i % 2], kind=kind, flag=True, noise=i % 3 == 0, minimize=i % 2 == 1, mask=i == 2, nsamp=(7, 1)[i % 2])
    both('acquire_kg', R=SWEEP_MOVED[1], nodes=None, noise=True, mask=True)
    both('acquire_kg', 'raw', R=SWEEP_MOVED[0], nodes=3, noise=False)
    both('acquire_kg', R=0, nodes=17, noise=True, minimize=True)                   # the candidates are their own reference set
    both('predict_cov', flag=False, noise=True); both('predict_cov', 'raw', flag=True)
    one('loo', SWEEP_N, block=64, flag=True, resident=True)
    both('loo', 'raw', block=1); both('loo', block=64)
    both('select', mask=True); both('select', 'raw')
    both('select_iv', flag=True, mask=True); both('select_iv', 'raw', flag=False)
    both('select_qei', nsamp=7, flag=True, mask=True); both('select_qei', 'raw', nsamp=1, flag=False, minimize=True)
    # condition and forget move the fit last: 300 -> 301 -> 338 -> 337 -> 300 rows (u picks forget's output groups in `call`)
    one('condition', SWEEP_MOVED[0]); one('condition', SWEEP_MOVED[1], 'raw')
    one('forget', SWEEP_MOVED[0], 'raw', u=2.5 / 997); one('forget', SWEEP_MOVED[1], u=1.5 / 997)
    both('predict')                                                                # the moved fit is used once more
    # the two newest entry points come last, so that every group above keeps its number, seed and salt; they run on the moved fit, which
    # takes ensure_pred_factor through once more
    both('predict_gradcov', flag=True, mask=True)                                  # all four outputs, zeros behind the last weighted row
    both('predict_gradcov', 'raw', flag=False)                                     # dmu and dvar only: the long chunks
    both('predict_pd', flag=True, mask=True, G=SWEEP_GRID[0], pdims='all')         # pd_ref.dims_for(D), all four outputs
    both('predict_pd', 'raw', nsamp=1, G=SWEEP_GRID[1], pdims='one', want=('pd', 'ice'))
    for st in steps:
        if st['op'] == 'post' and st['ep'] == 'loo':
            st.setdefault('resident', False)
    return steps


def check_sweep(steps):
    """what the sweep schedule must hold (conditions, not tuning)"""
    assert [st['op'] for st in steps[:4]] == ['xscaler', 'params', 'data', 'yscaler'] and steps[2]['N'] == SWEEP_N
    post = steps[4:]
    assert all(st['op'] == 'post' for st in post)
    by = lambda ep: [st for st in post if st['ep'] == ep]
    assert {st['ep'] for st in post} == set(SWEEP_ENTRY_POINTS)
    for ep in SWEEP_ENTRY_POINTS:
        Ts = {st['T'] for st in by(ep)}
        if ep in ('condition', 'forget'):
            assert Ts == set(SWEEP_MOVED), (ep, Ts)
        elif ep != 'sample_weights':
            assert set(SWEEP_T) <= Ts, (ep, Ts)
        modes = {st['mode'] for st in by(ep)}
        want = {'predict': {'scaled'}, 'predict_raw': {'raw'}, 'predict_y': {'y'}, 'sample_weights': {'scaled'}}.get(
            ep, {'scaled', 'raw', 'y'} if ep in Y_MODE else {'scaled', 'raw'})
        assert modes == want, (ep, modes)
    for i, st in enumerate(steps):
        if st['op'] == 'post' and st['mode'] == 'y':                               # a raw-mode step directly before its y-mode step
            p = steps[i - 1]
            assert p['seed'] == st['seed'] and p['T'] == st['T'] and p['mode'] == 'raw' and p['ep'] == st['ep'].replace('predict_y', 'predict_raw')
        if 'row0_of' in st:
            b = steps[st['row0_of']]
            assert st['T'] == 1 and b['T'] == SWEEP_T[0] and b['seed'] == st['seed'] and b['ep'] == st['ep'] and b['mode'] == st['mode']
    assert {(st['block'], st['resident']) for st in by('loo')} == {(64, True), (1, False), (64, False)}
    assert {st['flag'] for st in by('predict_cov')} == {True, False} and {st['flag'] for st in by('select_qei')} == {True, False}
    assert {st['R'] for st in by('acquire_kg')} == {0} | set(SWEEP_MOVED)
    for ep in ('sample', 'sample_weights', 'sample_argmax', 'sample_grad', 'select_qei'):
        assert {st['nsamp'] for st in by(ep)} == {1, 7}, ep
    assert {st['kind'] for st in by('acquire')} == set(A.KINDS)
    assert {(st['mode'], st['flag'], st['mask']) for st in by('predict_gradcov')} == {('scaled', True, True), ('raw', False, False)}
    assert {(st['mode'], st['G'], st['pdims'], st['mask'], st.get('want')) for st in by('predict_pd')} == {
        ('scaled', 9, 'all', True, None), ('raw', 1, 'one', False, ('pd', 'ice'))}
    new = [st['ep'] for st in post if st.get('group', 0) > SWEEP_OLD_GROUPS[1]]     # the new groups stand at the end
    assert new == ['predict_gradcov'] * 4 + ['predict_pd'] * 4 and [st['ep'] for st in post[-8:]] == new
    return dict(steps=len(steps), posterior=len(post))


def _row0(big, T):
    """the arguments of the T-row step made on the first T rows of a prepared step's rows: every per-row argument cut, the call's
    scalars (incumbents, sampled maxima, weights W, reference and pending rows) kept"""
    a = dict(big, T=T)
    for k in ('X', 'Xraw', 'y', 'yraw', 'targets', 'sidx', 'rows'):
        if a.get(k) is not None:
            a[k] = np.ascontiguousarray(a[k][:T])
    if 'w' in a:
        a['w'] = None                                                              # as materialise: no mask on fewer rows than it keeps
    if 'm' in a and a['ep'].startswith('select'):
        a['m'] = min(big['m'], T)
    if a['ep'] == 'select_iv' and a.get('ref_rows') is not None:
        a['ref_rows'] = np.arange(0, T, 3)
        a['Xr'] = np.ascontiguousarray(a['X'][a['ref_rows']]); a['wr'] = big['wr'][:len(a['ref_rows'])]
    return a


def row0_records(a, got, big_got, bits=True):
    """(c) the outputs of the call on row 0 alone against row 0 of the larger call's: bit for bit (bits=False, for references whose
    products promise no bits across row counts: the finite pattern and 1e-10)"""
    recs = []
    T = a['T']
    for k in ROW_ALONE[a['ep']]:
        g, b = got.get(k), big_got.get(k)
        if g is None or b is None:
            continue
        rows = len(np.asarray(b))
        if a['ep'] == 'predict_pd':                                                # ice is (ndim, T, G): the rows are its second axis
            rows = np.asarray(b).shape[1]; g = np.asarray(g); b = np.asarray(b)[:, :T]
        else:
            g = np.asarray(g); b = np.asarray(b)[:T]
        if a['ep'] == 'predict_cov' and a['Xb'] is None:
            b = b[:, :T]
        label = '(c) %s of row 0 alone against the %d-row call\'s' % (k, rows)
        if bits:
            recs.append((label, 'exact', g, b, None))
        else:
            fin = np.isfinite(g) & np.isfinite(b)
            recs.append((label + ' finite pattern', 'exact', np.isfinite(g), np.isfinite(b), None))
            recs.append((label, 'relnorm', g[fin], b[fin], 1e-10))
    return recs


def mirror_records(a, got, other, name):
    """(d) the outputs of a second context that made the same call, where the header says the two modes agree bit for bit"""
    recs = []
    for k in F16X3_EQUAL.get(a['ep'], ()):
        if k not in got or got[k] is None:
            continue
        g, o = got[k], other[k]
        if isinstance(g, dict):
            g = np.array([g[j] for j in sorted(g)], np.float64); o = np.array([o[j] for j in sorted(o)], np.float64)
        recs.append(('(d) %s of the %s context against this one\'s' % (k, name), 'exact', np.asarray(o), np.asarray(g), None))
    return recs


def ratio(rec):
    """how far into its bound a bounded record went (error / allowance; None for the exact ones and where nothing is bounded)"""
    label, kind, got, ref, par = rec
    with np.errstate(all='ignore'):
        if kind == 'relnorm':
            n = float(np.linalg.norm(np.asarray(ref)))
            return float(np.linalg.norm(np.asarray(got) - np.asarray(ref))) / (par * n) if n > 0 else None
        if kind == 'abs':
            e = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)); p = np.broadcast_to(np.asarray(par, np.float64), e.shape)
            ok = p > 0
            return float((e[ok] / p[ok]).max()) if np.any(ok) else None
        if kind == 'allclose':
            g = np.asarray(got, np.float64); r = np.asarray(ref, np.float64)
            return float((np.abs(g - r) / (par[1] + par[0] * np.abs(r))).max()) if g.size else None
        if kind == 'predict':
            return float(parity.predict_ratio(got[0], got[1], ref[0], ref[1], par))
        if kind == 'alpha':
            return float(parity.alpha_ratio(got, ref, par))
        if kind == 'li':
            return float(parity.li_ratio(got, ref, par))
        if kind == 'kinderr':
            k, mu, sd, beta = par
            return float(A.kind_error(k, got, ref, mu, sd, beta) / T_ACQ.PARITY_BOUND[k])
    return None


# ---- checks: records (label, kind, got, ref, par) -------------------------------------------------------------------------------------
def evaluate(rec):
    """assert one record"""
    label, kind, got, ref, par = rec
    if kind == 'exact':
        ok = np.array_equal(np.asarray(got), np.asarray(ref), equal_nan=np.asarray(ref).dtype.kind == 'f')
        assert ok, (label, 'not equal')
    elif kind == 'relnorm':
        d = float(np.linalg.norm(np.asarray(got) - np.asarray(ref))); n = float(np.linalg.norm(np.asarray(ref)))
        assert (d < par * n) or d == 0.0, (label, 'relative error %.3g, bound %.3g' % (d / n if n else np.inf, par))
    elif kind == 'abs':
        e = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
        ok = e <= par
        assert np.all(ok), (label, 'worst error / allowance %.3g' % float(np.nanmax(np.where(ok, 0.0, e / np.maximum(par, 1e-300))))
                            if np.all(np.isfinite(e)) else 'non-finite')
    elif kind == 'allclose':
        assert np.allclose(got, ref, rtol=par[0], atol=par[1]), (label, 'not close', par)
    elif kind == 'predict':
        assert _finite(got[0], got[1]), (label, 'non-finite')
        r = parity.predict_ratio(got[0], got[1], ref[0], ref[1], par)
        assert r <= 1.0, (label, 'predictive row outside its bound, ratio %.3g' % r)
        parity.check_predict(got[0], got[1], ref[0], ref[1], par)
    elif kind == 'alpha':
        assert _finite(got), (label, 'non-finite')
        parity.check_alpha(got, ref, par)
    elif kind == 'li':
        assert _finite(got), (label, 'non-finite')
        parity.check_li(got, ref, par)
    elif kind == 'kinderr':
        k, mu, sd, beta = par
        e = A.kind_error(k, got, ref, mu, sd, beta)
        assert e <= T_ACQ.PARITY_BOUND[k], (label, k, e, T_ACQ.PARITY_BOUND[k])
    else:
        raise ValueError(kind)


def perturbed(rec, factor=10.0):
    """the record with its output moved by `factor` times the bound of its check in one place (one ulp for the exact ones): None where
    the record has nothing to move (an empty output, a zero allowance)"""
    label, kind, got, ref, par = rec
    if kind == 'exact':
        g = np.array(got, order='C')                              # C order: ravel() below must be a view
        if g.size == 0:
            return None
        if g.dtype.kind == 'f':
            i = np.flatnonzero(np.isfinite(g.ravel()))
            if i.size == 0:
                return None
            g.ravel()[i[0]] = np.nextafter(g.ravel()[i[0]], np.inf)
        elif g.dtype.kind == 'b':
            g = g.reshape(-1); g[0] = not g[0]
        else:
            g.ravel()[0] += 1
        return (label, kind, g.reshape(np.shape(got)), ref, par)
    if kind == 'relnorm':
        if np.size(ref) == 0:
            return None
        g = np.array(ref, np.float64, order='C'); g.ravel()[0] += factor * par * np.linalg.norm(ref)
        return (label, kind, g, ref, par) if np.linalg.norm(ref) > 0 else None
    if kind == 'abs':
        g = np.array(np.broadcast_to(np.asarray(ref, np.float64), np.broadcast(np.asarray(ref), np.asarray(par)).shape))
        p = np.broadcast_to(np.asarray(par, np.float64), g.shape)
        i = int(np.argmax(p)) if p.size else 0
        if not p.size or not p.ravel()[i] > 0:
            return None
        g.ravel()[i] += factor * p.ravel()[i]
        return (label, kind, g, ref, par)
    if kind == 'allclose':
        g = np.array(ref, np.float64, order='C')
        i = np.flatnonzero(np.isfinite(g.ravel()))
        if i.size == 0:
            return None
        g.ravel()[i[0]] += factor * (par[1] + par[0] * abs(g.ravel()[i[0]]))
        return (label, kind, g, ref, par)
    if kind == 'predict':
        mu = np.array(ref[0], np.float64)
        mu.ravel()[0] += factor * parity.TOL[par]['eps'] * np.ravel(ref[1])[0]
        return (label, kind, (mu, np.array(ref[1])), ref, par)
    if kind in ('alpha', 'li'):
        t = parity.TOL[par]
        b, tau = (t['vbeta'], t['vtau']) if kind == 'alpha' else (t['lbeta'], t['ltau'])
        g = np.array(ref, np.float64, order='C')
        tile = g[:parity.TILE]
        g.ravel()[0] += factor * (b * np.linalg.norm(tile) + tau * np.linalg.norm(ref))
        return (label, kind, g, ref, par)
    if kind == 'kinderr':
        k, mu, sd, beta = par
        g = np.array(ref, np.float64, order='C')
        i = int(np.argmax(np.abs(g) >= 1e-300)) if k not in ('ucb', 'logei') else 0
        scale = (abs(np.ravel(mu)[0]) + beta * np.ravel(sd)[0]) if k == 'ucb' else max(1.0, abs(g[0])) if k == 'logei' else abs(g[i])
        g[i] += factor * T_ACQ.PARITY_BOUND[k] * scale
        return (label, kind, g, ref, par) if scale > 0 else None
    raise ValueError(kind)


def same_bits(a, b):
    """twin comparison of one output (arrays, scalars, dicts of them, None)"""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    a = np.asarray(a); b = np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')


# ---- one step: arguments, the call, the auxiliary calls, the records ---------------------------------------------------------------------
REDRAWS = 64


def materialise(st, fit):
    """the arrays of a posterior step, drawn from its seed; rows in the mode's units.  A step marked `redraw` (acquire_kg and predict_pd
    in the sequences, whose fit is known only once the schedule has run so far) is drawn from seed, seed + 1, .. until its
    input condition holds (input_condition): a condition on the inputs, computed from the fp64 references alone"""
    if not st.get('redraw'):
        return _materialise(st, fit)
    for j in range(REDRAWS):
        draw = dict(st, seed=st['seed'] + j, draw=j)
        if j and st['ep'] == 'acquire_kg':
            # On a fit of thousands of rows the lines are far apart against their slopes: with the observation noise in sigma and 31
            # nodes, 1 draw in 18 meets the condition at 3000 fitted rows and none at 36 000; without the noise and with 3 nodes nearly
            # every draw does.  So a repeated draw takes these two options from its seed as well.  The runner's log names the draw
            # that was used with its options, and the CPU tier asserts the coverage of the options as they ran, not as scheduled.
            r = np.random.default_rng([st['seed'], j])
            draw.update(noise=bool(r.integers(2)), nodes=KG_NODES[int(r.integers(len(KG_NODES)))])
        if j and st['ep'] == 'predict_pd':
            # Under an X scaler that spreads the phases over many periods (D = 40, standardised columns) the mean feature row of a few
            # hundred rows is a cancellation whatever the seed.  A repeated draw narrows the pool instead: the rows' log-normal spread is
            # halved from draw to draw, down to PD_SPREAD_MIN.  Every row carries the sums with its drawn weight, so the block tree and
            # the running sums across chunks are exercised as on the first draw.
            draw['spread'] = max(PD_SPREAD_MIN, 0.5 ** j)
        a = _materialise(draw, fit)
        if input_condition(a, fit):
            return a
    raise AssertionError('no draw of this step meets its input condition: %r' % (st,))


PD_SPREAD_MIN = 1.0 / 64


def input_condition(a, fit):
    """acquire_kg: kg_conditioning <= 1; predict_pd with sums: pd_cancellation >= PD_CANCEL"""
    if a['ep'] == 'acquire_kg':
        return kg_conditioning(a, fit) <= 1.0
    if a['ep'] == 'predict_pd' and set(a['want']) - {'ice'}:
        return pd_cancellation(a, fit) >= PD_CANCEL
    return True


def used_draw(a):
    """what the runner's log says of a step drawn at run time: which draw was used, and the options a repeated draw may have replaced"""
    if a.get('draw') is None:
        return ''
    if a['ep'] == 'acquire_kg':
        return ' draw=%d noise=%s nodes=%s R=%d' % (a['draw'], a['noise'], a['nodes'], a['R'])
    return ' draw=%d spread=%g' % (a['draw'], a.get('spread', 1.0))


def _materialise(st, fit):
    D, S, M = fit.D, fit.S, fit.M
    rng = np.random.default_rng(st['seed'])
    ep, T, mode = st['ep'], st['T'], st['mode']
    a = dict(st)
    alpha, Li = fit.factors()
    a['alpha'], a['Li'] = alpha, Li
    give = lambda Xraw: Xraw if mode != 'scaled' else fit.fx(Xraw)

    def mask(n, least=1):
        if not st['mask'] or n <= least:
            return None
        w = np.where(rng.random(n) < 0.5, 0.0, 0.5 + rng.random(n))
        w[rng.choice(n, least, replace=False)] = 1.0
        return w

    if ep in ('forget', 'loo'):
        N = fit.Xraw.shape[0]
        if st['op'] == 'fail' and ep == 'loo':
            # rows that are not in this fit: fresh rows, and the factor scaled until the largest leverage in the call is 4
            Xraw = raw_rows(rng, T, D)
            C = pred_cov_ref.factor(fit.fx(Xraw), Li, fit.params, S, M)
            a['Li'] = Li * max(1.0, np.sqrt(4.0 / np.sum(C * C, axis=1).max()))
            a['rows'] = None; a['X'] = give(Xraw); a['y'] = fit.fy(raw_targets(rng, Xraw)).ravel()
        elif ep == 'loo' and st.get('resident'):
            a['rows'] = None; a['X'] = None; a['y'] = None
        else:
            i0 = int(rng.integers(0, N - T + 1))
            a['rows'] = np.arange(i0, i0 + T) if ep == 'loo' else np.sort(rng.choice(N, T, replace=False))
            a['X'] = give(fit.Xraw[a['rows']]); a['y'] = fit.y()[a['rows']].ravel()
            if st['op'] == 'fail':
                a['y'] = a['y'].copy(); a['y'][T // 2] = np.nan
        return a
    Xraw = raw_rows(rng, T, D, st.get('spread', 1.0))
    a['Xraw'] = Xraw
    if st.get('nan_row') or (st['op'] == 'fail' and ep in ('sample_argmax', 'predict_pd')):
        Xraw[T // 3, 0] = np.nan
    with np.errstate(all='ignore'):
        a['X'] = give(Xraw)
    if ep == 'condition':
        a['yraw'] = raw_targets(rng, Xraw); a['y'] = fit.fy(a['yraw']).ravel()
    elif ep == 'predict_y':
        a['targets'] = raw_targets(rng, Xraw) if st['flag'] else None
    elif ep == 'sample_grad':
        a['W'] = SR.weights(alpha, Li, kappa(fit.params), st['nsamp'], st['seed'] % 1000)
        a['sidx'] = rng.integers(0, st['nsamp'], T) if st['flag'] else None
        a['want_val'] = bool(st['noise'] or st.get('pair'))
    elif ep in ('sample_argmax', 'acquire'):
        a['w'] = mask(T)
    elif ep in ('predict_gradcov', 'predict_pd'):
        # weights with zeros among them and, on more than 8 rows, behind the last weighted row
        a['w'] = mask(T)
        if a['w'] is not None and T > 8:
            a['w'][T - 3:] = 0.0
            a['w'][0] = max(a['w'][0], 1.0)
        if ep == 'predict_gradcov':
            a['want'] = tuple(st['want']) if st.get('want') else T_GC.ALL if st['flag'] else ('dmu', 'dvar')
            if st['op'] == 'fail':
                a['w'] = np.zeros(T)                                               # weights that sum to 0: refused when asub is wanted
        else:
            a['want'] = tuple(st['want']) if st.get('want') else T_PD.ALL if st['flag'] else ('pd', 'sd')
            dims = PD.dims_for(D) if st['pdims'] == 'all' else [int(st['u'] * D)]
            cols = list(fit.xs.data['cols'])
            a['dims'] = dims if mode == 'scaled' else [cols[d] for d in dims]     # raw mode names raw columns
            fin = np.isfinite(a['X']).all(axis=1)
            a['grid'] = PD.make_grid(a['X'][fin], a['dims'], st['G'], seed=st['seed'] % 1000)
            # the auxiliary call's arguments: the dimensions reversed, a permuted proper subset of the grid (all of it at G = 1)
            a['sub'] = np.arange(st['G'])[::-2]
    elif ep == 'acquire_kg':
        a['w'] = mask(T)
        a['Xr'] = give(raw_rows(rng, st['R'], D)) if st['R'] else None      # R = 0: the candidates are their own reference set
        a['z'] = None if st['nodes'] is None else T_KG.NODES[st['nodes']]
    elif ep == 'predict_cov':
        if st['flag'] or st['op'] == 'fail':
            Tb = int(rng.choice([1, 37, 257, 3000])) if T <= 700 else int(rng.choice([1, 37, 257]))
            a['Xb'] = give(raw_rows(rng, Tb, D))
        else:
            a['Xb'] = None
            a['X'] = a['X'][:700]; a['Xraw'] = Xraw[:700]                  # the symmetric form is T x T
    elif ep in ('select', 'select_iv', 'select_qei'):
        a['w'] = mask(T, least=min(T, st['m']))
        a['m'] = min(st['m'], T)
        if ep == 'select_iv':
            if st['flag']:
                rows = np.arange(0, T, 3)
                a['ref_rows'] = rows; a['Xr'] = np.ascontiguousarray(a['X'][rows]); a['wr'] = 0.5 + rng.random(len(rows))
            else:
                a['ref_rows'] = None; a['Xr'] = None; a['wr'] = None
        if ep == 'select_qei':
            a['pending'] = give(raw_rows(rng, 3, D)) if st['flag'] else None
    return a


def prepare(eng, a, fit):
    """device calls whose results are ARGUMENTS of the step (made once, on the context under test): the sampled maxima of MES and the
    incumbents"""
    ep = a['ep']
    if ep == 'acquire':
        mu0 = O.predict(fit.fx(a['Xraw']), a['alpha'], a['Li'], fit.params, fit.S, fit.M)[0]
        a['best'] = float(np.median(mu0)); a['xi'] = 0.01; a['beta'] = 1.5
        a['fstar'] = None
        if a['kind'] == 'mes':
            a['fstar'] = eng.sample_argmax(a['X'], a['alpha'], a['Li'], a['nsamp'], seed=3, mode=a['mode'], minimize=a['minimize'])[1]
        a['want'] = ('acq', 'argmax', 'mu', 'sd') + (('grad',) if a['flag'] else ())
    elif ep == 'select_qei':
        F = SR.samples(fit.fx(a['Xraw']), a['alpha'], a['Li'], fit.params, fit.S, fit.M, a['nsamp'], a['seed'] % 1000)
        a['best'] = float(np.median(F.min(axis=0) if a['minimize'] else F.max(axis=0)))
    return a


def call(eng, a):
    """the step's own call: a dict of its outputs"""
    ep, al, Li, X, mode = a['ep'], a['alpha'], a['Li'], a['X'], a['mode']
    raw = mode != 'scaled'
    if ep == 'predict':
        return dict(zip(('mu', 'sd'), eng.predict(X, al, Li)))
    if ep == 'predict_raw':
        return dict(zip(('mu', 'sd'), eng.predict_raw(X, al, Li)))
    if ep == 'predict_y':
        mu, sd, met = eng.predict_y(X, al, Li, a['targets'])
        return dict(mu=mu, sd=sd, metrics=None if met is None else np.array([met[k] for k in RefEngine.METRICS]))
    if ep == 'predict_grad':
        return dict(zip(('mu', 'sd', 'dmu', 'dsd'), eng.predict_grad(X, al, Li, mode=mode, want_std=a['flag'])))
    if ep == 'sample_weights':
        return dict(W=eng.sample_weights(al, Li, a['nsamp'], seed=a['seed'] % 1000))
    if ep == 'sample':
        return dict(out=eng.sample(X, al, Li, a['nsamp'], seed=a['seed'] % 1000, mode=mode, noise=a['noise']))
    if ep == 'sample_argmax':
        return dict(zip(('idx', 'val'), eng.sample_argmax(X, al, Li, a['nsamp'], seed=a['seed'] % 1000, w=a['w'], mode=mode,
                                                          minimize=a['minimize'])))
    if ep == 'sample_grad':
        return dict(zip(('val', 'grad'), eng.sample_grad(X, a['W'], sidx=a['sidx'], mode=mode, want_val=a['want_val'])))
    if ep == 'acquire':
        kw = {'ucb': dict(beta=a['beta']), 'mes': dict(fstar=a['fstar'])}.get(a['kind'], dict(best=a['best'], xi=a['xi']))
        return eng.acquire(X, al, Li, a['kind'], w=a['w'], mode=mode, noise=a['noise'], minimize=a['minimize'], want=a['want'], **kw)
    if ep == 'acquire_kg':
        return eng.acquire_kg(X, al, Li, Xr=a['Xr'], z=a['z'], w=a['w'], mode=mode, noise=a['noise'], minimize=a['minimize'], want=T_KG.ALL)
    if ep == 'predict_gradcov':
        return eng.predict_gradcov(X, al, Li, w=a['w'], mode=mode, want=a['want'])
    if ep == 'predict_pd':
        return eng.predict_pd(X, al, Li, a['dims'], a['grid'], w=a['w'], mode=mode, want=a['want'])
    if ep == 'predict_cov':
        return dict(cov=eng.predict_cov(X, Li, Xb=a['Xb'], mode=mode, noise=a['noise'] and (a['Xb'] is None or a['op'] == 'fail')))
    if ep == 'condition':
        return dict(zip(('alpha', 'Li'), eng.condition(X, a['y'], al, Li, mode=mode)))
    if ep == 'forget':
        factors, predict = (True, True) if a['op'] == 'fail' else ((True, False), (True, True), (False, True))[int(a['u'] * 997) % 3]
        out = eng.forget(X, a['y'], al, Li, factors=factors, predict=predict, mode=mode)
        return dict(zip((('alpha', 'Li') if factors else ()) + (('mu', 'sd', 'stats') if predict else ()), out))
    if ep == 'loo':
        return dict(zip(('mu', 'sd', 'lev', 'stats'), eng.loo(X, a['y'], al, Li, block=a['block'], mode=mode)))
    if ep == 'select':
        return dict(zip(('idx', 'var', 'gain', 'sd'), eng.select(X, Li, a['m'], w=a['w'], raw=raw, return_std=True)))
    if ep == 'select_iv':
        return dict(zip(('idx', 'red', 'var', 'ivar', 'sd'), eng.select_iv(X, Li, a['m'], Xr=a['Xr'], w=a['w'], wr=a['wr'], raw=raw,
                                                                          return_std=True)))
    if ep == 'select_qei':
        return dict(zip(('idx', 'gain', 'qei', 'score0', 'mstate'),
                        eng.select_qei(X, al, Li, a['m'], a['nsamp'], a['best'], xi=0.01, seed=a['seed'] % 1000, w=a['w'], pending=a['pending'],
                                       mode=mode, minimize=a['minimize'], return_score0=True, return_state=True)))
    raise ValueError(ep)


def auxiliary(eng, a, got, fit):
    """further calls on the context under test whose DEVICE outputs the references of this step are formed from (as the own tests do)"""
    ep, al, Li, X, mode = a['ep'], a['alpha'], a['Li'], a['X'], a['mode']
    aux = {}
    if ep == 'sample_argmax' and mode != 'y':
        aux['block'] = eng.sample(X, al, Li, a['nsamp'], seed=a['seed'] % 1000, mode=mode, noise=False)
    elif ep == 'select_qei':
        aux['F'] = eng.sample(X, al, Li, a['nsamp'], seed=a['seed'] % 1000, mode=mode, noise=False)
        aux['P'] = None if a['pending'] is None else eng.sample(a['pending'], al, Li, a['nsamp'], seed=a['seed'] % 1000, mode=mode, noise=False)
    elif ep == 'acquire' and 'grad' in a['want']:
        aux['pg'] = eng.predict_grad(X, al, Li, mode=mode)
    elif ep == 'acquire_kg':
        # the lines of tests/test_gpu_acquire_kg.py's _device_lines, in the step's mode: the device's own predict_cov, predict and sigma
        Xb = X if a['Xr'] is None else a['Xr']
        aux['cov'] = eng.predict_cov(X, Li, Xb=Xb, mode=mode)
        aux['mu_r'], aux['sd_r'] = (eng.predict if mode == 'scaled' else eng.predict_raw)(Xb, al, Li)
        aux['sd'] = eng.acquire(X, al, Li, 'ucb', beta=0.0, mode=mode, noise=a['noise'], want=('acq', 'sd'))['sd']
    elif ep == 'predict_gradcov':
        # promise 1: predict_grad of the same mode on the same context, which is thereby the direct successor of every gradcov call
        aux['dmu'] = eng.predict_grad(X, al, Li, mode=mode, want_std=False)[2]
    elif ep == 'predict_pd':
        # promises 2, 3 and 7: the dimensions reversed, a permuted proper subset of the grid, the sums only.  A context whose products
        # promise no bits across shapes (RefEngine.ROW_BITS) is compared to 1e-10 instead
        aux['sub'] = eng.predict_pd(X, al, Li, a['dims'][::-1], a['grid'][::-1][:, a['sub']], w=a['w'], mode=mode, want=('pd', 'sd', 'cov'))
        aux['bits'] = getattr(eng, 'ROW_BITS', True)
    elif ep in ('condition', 'forget') and 'alpha' in got:
        aux['probe'] = fit.fx(raw_rows(np.random.default_rng(a['seed'] + 1), 200, fit.D))
        aux['predict'] = eng.predict(aux['probe'], got['alpha'], got['Li'])
    return aux


def _ref_engine(fit, dtype='f64'):
    r = RefEngine(fit.D, fit.S, fit.M)
    r.set_params(fit.params)
    r.xs, r.ys = fit.xs, fit.ys
    if fit.resident is not None:
        r.set_data(*fit.resident)
    return r


def _fin_records(label, got, ref):
    """the finite pattern of a y-mode output against the host tail's, and the mask of the rows to compare"""
    fg, fr = np.isfinite(got), np.isfinite(ref)
    return [(label + ' finite pattern', 'exact', fg, fr, None)], fg & fr


def _replay_picks(label, scores, idx, tol):
    """the device's picks in the reference's replay: eligible, not taken twice, and within tol of the best score of their step"""
    m = len(idx)
    got = scores[np.arange(m), idx]
    best = scores.max(axis=1)
    return [(label + ' picks are eligible and distinct', 'exact', np.array([bool(np.all(np.isfinite(got))), len(set(idx.tolist())) == m]),
             np.array([True, True]), None),
            (label + ' picks near-optimal in the replay', 'abs', got, best, tol * np.abs(best))]


def records(a, got, aux, fit, dtype, prev):
    """the checks of a posterior step against the CPU references"""
    ep, mode, S, M = a['ep'], a['mode'], fit.S, fit.M
    al, Li, params = a['alpha'], a['Li'], fit.params
    kap = kappa(params)
    ref = _ref_engine(fit)
    recs = []
    add = lambda *r: recs.append(r)
    Xs = fit.fx(a['Xraw']) if 'Xraw' in a else None                      # the scaled rows, whatever the mode
    if mode == 'y':
        # against the host tail of the device's own raw-mode outputs of the step before (tolerances of the own tests' y-mode checks)
        ys = fit.ys
        if ep == 'predict_y' or ep == 'predict_grad':
            mu_h, sd_h = y_tail(ys, prev['mu'], prev['sd'])
            gmu, gsd = np.asarray(got['mu']).reshape(-1, 1), np.asarray(got['sd']).reshape(-1, 1)
            add('mu_y nan pattern', 'exact', np.isnan(gmu), np.isnan(mu_h), None)
            add('std_y nan pattern', 'exact', np.isnan(gsd), np.isnan(sd_h), None)
            ok = ~(np.isnan(mu_h) | np.isnan(sd_h))
            add('mu_y', 'allclose', gmu[ok], mu_h[ok], (1e-9, 1e-12))     # tests/test_gpu_parity.py: predict_y
            add('std_y', 'allclose', gsd[ok], sd_h[ok], (1e-8, 1e-12))
            if ep == 'predict_y' and a['targets'] is not None:
                m_ref = y_metrics(mu_h, sd_h, a['targets'])
                fin = np.isfinite(m_ref)
                add('metrics nan pattern', 'exact', np.isnan(got['metrics']), np.isnan(m_ref), None)
                add('metrics', 'abs', got['metrics'][fin], m_ref[fin], 1e-8 * np.maximum(1.0, np.abs(m_ref[fin])))
            if ep == 'predict_grad':
                with np.errstate(all='ignore'):
                    dmu, dsd = G.y_chain(ys, prev['mu'], prev['sd'], prev['dmu'], prev['dsd'] if prev['dsd'] is not None else 0.0 * prev['dmu'])
                okr = ok.ravel() & np.isfinite(dmu).all(1)
                add('dmu_y', 'relnorm', got['dmu'][okr], dmu[okr], 1e-5)                 # tests/test_gpu_predict_grad.py: y mode
                if got['dsd'] is not None:
                    okr = okr & np.isfinite(dsd).all(1)
                    add('dstd_y finite where the tail is', 'exact', np.isfinite(got['dsd'][okr]).all(), np.True_, None)
                    add('dstd_y', 'relnorm', got['dsd'][okr], dsd[okr], 1e-5)
        elif ep == 'sample':
            want = bw(ys, prev['out'])
            r, fin = _fin_records('sample y', got['out'], want); recs += r
            add('sample y', 'relnorm', got['out'][fin], want[fin], 1e-12)                # tests/test_gpu_sample.py: y mode
        elif ep == 'sample_argmax':
            add('idx is the raw mode\'s', 'exact', got['idx'], prev['idx'], None)        # the row is chosen in scaled units
            want = bw(ys, prev['val'])
            r, fin = _fin_records('sample_argmax y', got['val'], want); recs += r
            add('val y', 'relnorm', got['val'][fin], want[fin], 1e-12)
        elif ep == 'sample_grad':
            want = bw(ys, prev['val'])
            r, fin = _fin_records('sample_grad y', got['val'], want); recs += r
            add('val y', 'relnorm', got['val'][fin], want[fin], 1e-12)
            with np.errstate(all='ignore'):
                g = G.y_backward_deriv(ys, prev['val'])[:, None] * prev['grad']
            okr = fin & np.isfinite(g).all(1)
            add('grad y', 'relnorm', got['grad'][okr], g[okr], 1e-5)                     # tests/test_gpu_sample_grad.py: y mode
        return recs
    if ep in ('predict', 'predict_raw'):
        add('predict', 'predict', (got['mu'], got['sd']), O.predict(Xs, al, Li, params, S, M), dtype)
    elif ep == 'predict_grad':
        mu0, sd0, dmu0, dsd0 = ref.predict_grad(a['X'], al, Li, mode=mode)
        add('predict', 'predict', (got['mu'], got['sd']), (mu0, sd0), dtype)
        add('dmu', 'relnorm', got['dmu'], dmu0, T_PG.BOUNDS[dtype][0])
        add('dstd given iff asked for', 'exact', got['dsd'] is not None, a['flag'], None)
        if got['dsd'] is not None:
            add('dstd', 'relnorm', got['dsd'], dsd0, T_PG.BOUNDS[dtype][1])
    elif ep == 'sample_weights':
        add('W', 'relnorm', got['W'], ref.sample_weights(al, Li, a['nsamp'], a['seed'] % 1000), 1e-12)      # tests/test_gpu_sample.py
    elif ep == 'sample':
        want = ref.sample(a['X'], al, Li, a['nsamp'], seed=a['seed'] % 1000, mode=mode, noise=a['noise'])
        r, fin = _fin_records('sample', got['out'], want); recs += r
        add('sample', 'relnorm', got['out'][fin], want[fin], T_SMP.BOUNDS[dtype])
    elif ep == 'sample_argmax':
        ridx, rval = AM.argmax(aux['block'], a['w'], a['minimize'])                      # on the device's own block, bit for bit
        add('idx', 'exact', got['idx'], ridx, None); add('val', 'exact', got['val'], rval, None)
        want = ref.sample(a['X'], al, Li, a['nsamp'], seed=a['seed'] % 1000, mode=mode)
        add('block', 'relnorm', aux['block'], want, T_SMP.BOUNDS[dtype])
    elif ep == 'sample_grad':
        v0, g0 = ref.sample_grad(a['X'], a['W'], sidx=a['sidx'], mode=mode)
        add('val given iff asked for', 'exact', got['val'] is not None, a['want_val'], None)
        if got['val'] is not None:
            add('val', 'relnorm', got['val'], v0, T_SG.VAL_BOUNDS[dtype])
        add('grad', 'relnorm', got['grad'], g0, T_SG.GRAD_BOUNDS[dtype])
    elif ep == 'acquire':
        mu0, sds = O.predict(Xs, al, Li, params, S, M)
        mu0 = mu0.ravel()
        mu, sd, kind = got['mu'], got['sd'], a['kind']
        add('mu', 'abs', mu, mu0, EPS[dtype] * sds)                                      # predict's bound on mu
        if a['noise']:
            add('sd', 'abs', sd, sds, EPS[dtype] * sds)
        else:
            # sigma_f = sqrt(kappa v) where predict's sigma* = sqrt(kappa (1 + v)): the same error of v moves sigma_f by sigma* / sigma_f
            # times what it moves sigma* by, so predict's bound eps sigma* becomes eps sigma*^2 / sigma_f
            sf = A.sigma(kap, np.sum(pred_cov_ref.factor(Xs, Li, params, S, M) ** 2, axis=1), False)
            add('sd (latent)', 'abs', sd, sf, EPS[dtype] * sds ** 2 / sf)
        kw = {'ucb': dict(beta=a['beta']), 'mes': dict(fstar=a['fstar'])}.get(kind, dict(best=a['best'], xi=a['xi']))
        acq0, au, as_ = A.acquire(kind, mu, sd, minimize=a['minimize'], **kw)          # the restatement at the device's mu, sd
        add('acq', 'kinderr', got['acq'], acq0, (kind, mu, sd, a['beta']))
        add('argmax idx', 'exact', got['idx'], A.argmax(got['acq'], a['w']), None)
        add('argmax val', 'exact', got['val'], float(got['acq'][got['idx']]), None)
        if 'grad' in a['want']:
            _, sd_star, dmu, dstd = aux['pg']
            dsig = dstd if a['noise'] else dstd * (sd_star / sd)[:, None]
            add('grad', 'relnorm', got['grad'], (-1.0 if a['minimize'] else 1.0) * au[:, None] * dmu + as_[:, None] * dsig, T_ACQ.CHAIN_BOUND)
    elif ep == 'acquire_kg':
        z = KG.DEFAULT_NODES if a['z'] is None else a['z']
        Xb = a['X'] if a['Xr'] is None else a['Xr']
        # the lines themselves against the references, under predict_cov's and predict's bounds
        # element by element: cov_ij = kappa <c_i, c_j> is bilinear in two factor rows, each good to half of predict_cov's bound relative
        # to its own norm (tests/test_gpu_predict_cov.py: BOUNDS), so |delta cov_ij| <= BOUNDS kappa |c_i| |c_j|.  The norm-wise form of
        # that test does not carry over to R = 1 or T = 1, where the matrix is a few off-diagonal elements that may cancel
        ni = np.linalg.norm(pred_cov_ref.factor(Xs, Li, params, S, M), axis=1)
        nj = ni if a['Xr'] is None else np.linalg.norm(pred_cov_ref.factor(ref._rows(a['Xr'], mode)[0], Li, params, S, M), axis=1)
        add('cov of the lines', 'abs', aux['cov'], ref.predict_cov(a['X'], Li, Xb=Xb, mode=mode), T_COV.BOUNDS[dtype] * kap * np.outer(ni, nj))
        add('mu of the reference rows', 'predict', (aux['mu_r'], aux['sd_r']),
            (ref.predict if mode == 'scaled' else ref.predict_raw)(Xb, al, Li), dtype)
        # tests/test_gpu_acquire_kg.py: the node table bit for bit from the device's own lines, the sums at the device's own table
        m, s, lo, hi = KG.node_table(KG.offsets(np.ravel(aux['mu_r']), a['minimize']), KG.slopes(aux['cov'], aux['sd']), z)
        add('m', 'exact', got['m'], m, None); add('s', 'exact', got['s'], s, None)
        add('m is 0 at the node 0', 'exact', got['m'][:, list(z).index(0.0)] == 0.0, np.ones(len(m), bool), None)
        kg, kg_hi = KG.bounds(got['m'], got['s'], lo, hi, z)
        allow = T_KG.VALUE_BOUND * kg_hi.max()
        add('kg', 'abs', got['kg'], kg, allow); add('kg_hi', 'abs', got['kg_hi'], kg_hi, allow)
        add('0 <= kg <= kg_hi', 'exact', np.array([bool((got['kg'] >= 0).all()), bool((got['kg'] <= got['kg_hi'] + allow).all())]),
            np.ones(2, bool), None)
        if len(Xb) == 1:
            add('both sums are 0 at R = 1', 'exact', np.array([np.abs(got['kg']).max(), np.abs(got['kg_hi']).max()]), np.zeros(2), None)
        add('argmax idx', 'exact', got['idx'], int(KG.argmax(got['kg'], a['w'])), None)
        add('argmax val', 'exact', got['val'], float(got['kg'][got['idx']]), None)
    elif ep == 'predict_gradcov':
        want = a['want']
        add('outputs are those asked for', 'exact', np.array([k in got for k in T_GC.ALL]), np.array([k in want for k in T_GC.ALL]), None)
        r = ref.predict_gradcov(a['X'], al, Li, w=a['w'], mode=mode, want=want)
        fin = np.isfinite(ref._rows(a['X'], mode)[0]).all(axis=1)                          # a NaN row stays in its own point's outputs
        for k in ('dmu', 'dvar', 'dcov'):
            if k in want:
                add(k + ' finite pattern', 'exact', np.isfinite(got[k]), np.isfinite(r[k]), None)
                add(k, 'relnorm', got[k][fin], r[k][fin], (T_GC.BOUNDS_DMU if k == 'dmu' else T_GC.BOUNDS)[dtype])
        if 'asub' in want:
            add('asub', 'relnorm', got['asub'], r['asub'], T_GC.BOUNDS[dtype])
            add('asub is symmetric', 'exact', got['asub'], got['asub'].T, None)
        if 'dmu' in want:
            add('dmu is predict_grad\'s', 'exact', got['dmu'], aux['dmu'], None)
        if 'dcov' in want:
            add('dcov is symmetric', 'exact', got['dcov'], got['dcov'].transpose(0, 2, 1), None)
            if 'dvar' in want:
                add('dvar is the diagonal of dcov', 'exact', got['dvar'], np.diagonal(got['dcov'], axis1=1, axis2=2), None)
        if 'dvar' in want:
            add('dvar >= 0', 'exact', not np.any(got['dvar'] < 0), True, None)
    elif ep == 'predict_pd':
        want = a['want']
        add('outputs are those asked for', 'exact', np.array([k in got for k in T_PD.ALL]), np.array([k in want for k in T_PD.ALL]), None)
        sums = tuple(k for k in ('pd', 'sd', 'cov') if k in want)
        if sums:
            r = ref.predict_pd(a['X'], al, Li, a['dims'], a['grid'], w=a['w'], mode=mode, want=sums)
            for k in sums:
                add(k, 'relnorm', got[k], r[k], T_PD.BOUNDS[dtype])
        if 'ice' in want:
            # rows first, so that a step on row 0 alone is row-aligned with the larger one (conditioned_row0); a long call is compared
            # on the rows around its chunk boundaries, as tests/test_gpu_predict_pd.py does
            T = a['X'].shape[0]
            sel = np.arange(T) if T <= 3000 else np.r_[0:4, 32766:32770, 65534:65538, T - 2:T]
            r = ref.predict_pd(a['X'][sel], al, Li, a['dims'], a['grid'], mode=mode, want=('ice',))
            add('ice', 'relnorm', got['ice'][:, sel].transpose(1, 0, 2), r['ice'].transpose(1, 0, 2), T_PD.BOUNDS_ICE[dtype])
        if 'cov' in want:
            add('cov is symmetric', 'exact', got['cov'], got['cov'].transpose(0, 2, 1), None)
            if 'sd' in want:                                                               # tests/test_gpu_predict_pd.py: under BOUNDS
                add('diag(cov) against sd^2', 'relnorm', np.diagonal(got['cov'], axis1=1, axis2=2), got['sd'] ** 2, T_PD.BOUNDS[dtype])
        if 'sd' in want:
            add('sd >= 0', 'exact', bool(np.all(got['sd'] >= 0)), True, None)
        sub = a['sub']
        for k in sums:
            full = got[k][::-1][:, sub] if k != 'cov' else got[k][::-1][:, sub][:, :, sub]
            if aux['bits']:
                add('%s of the reversed dimensions and the grid\'s subset' % k, 'exact', aux['sub'][k], full, None)
            else:
                add('%s of the reversed dimensions and the grid\'s subset' % k, 'relnorm', aux['sub'][k], full, 1e-10)
    elif ep == 'predict_cov':
        add('cov', 'relnorm', got['cov'], ref.predict_cov(a['X'], Li, Xb=a['Xb'], mode=mode, noise=a['noise'] and a['Xb'] is None),
            T_COV.BOUNDS[dtype])
    elif ep in ('condition', 'forget'):
        if ep == 'condition':
            Xall = np.vstack([fit.X(), Xs]); yall = np.vstack([fit.y().reshape(-1, 1), a['y'].reshape(-1, 1)])
        else:
            keep = np.setdiff1d(np.arange(fit.Xraw.shape[0]), a['rows'])
            Xall, yall = fit.X()[keep], fit.y().reshape(-1, 1)[keep]
        _, a1, L1 = O.forward(Xall, yall, params, S, M, gauss_hermite=False)
        a['new_factors'] = (a1, L1)
        if 'alpha' in got:
            add('alpha', 'alpha', got['alpha'], a1, dtype); add('Li', 'li', got['Li'], L1, dtype)
            add('zeros above the diagonal', 'exact', np.all(np.triu(got['Li'], 1) == 0.0), np.True_, None)
            add('predict with the returned factors', 'predict', aux['predict'], O.predict(aux['probe'], a1, L1, params, S, M), dtype)
        if 'mu' in got:
            Xo = fit.X()[a['rows']]
            r = forget_ref.forget(Xo, a['y'], al, Li, params, S, M)
            a['min_pivot2'] = float(r['stats'][5])
            add('held-out predictions', 'predict', (got['mu'], got['sd']), O.predict(Xo, a1, L1, params, S, M), dtype)
            st = got['stats']
            e = a['y'] - got['mu'].ravel(); sd = got['sd']
            add('stats n, blocks', 'exact', np.array([st['n'], st['blocks']]), np.array([len(e), 1]), None)
            add('sum_e2', 'exact', st['sum_e2'], functools.reduce(lambda s, v: s + v, (e * e).tolist(), 0.0), None)
            add('sum_abs_e', 'exact', st['sum_abs_e'], functools.reduce(lambda s, v: s + v, np.abs(e).tolist(), 0.0), None)
            marg = -0.5 * (e * e / (sd * sd) + np.log(2 * np.pi * (sd * sd)))
            add('sum_log_marginal', 'abs', st['sum_log_marginal'], np.sum(marg), 1e-12 * np.sum(np.abs(marg)))
            # the first pass and the K x K stage are fp64 in every context (include/scfgp_hip.h): the fp64 figure of the own test's
            # comparison of this number, 1e-8, in both
            add('log_joint', 'abs', st['log_joint'], r['stats'][4], 1e-8 * abs(r['stats'][4]))
            add('min_pivot2', 'abs', st['min_pivot2'], r['stats'][5], 1e-8 * r['stats'][5])
        elif ep == 'forget':
            a['min_pivot2'] = float(forget_ref.forget(fit.X()[a['rows']], a['y'], al, Li, params, S, M)['stats'][5])
    elif ep == 'loo':
        if a.get('resident'):
            Xl, yl = fit.resident
        else:
            Xl, yl = fit.X()[a['rows']], a['y']
        r = loo_ref.loo(Xl, yl, al, Li, params, S, M, a['block'])
        n = len(r['mu'])
        if dtype == 'f64':
            add('held-out rows', 'predict', (got['mu'], got['sd']), (r['mu'], r['std']), 'f64')
        else:
            allow = EPS['f32'] * r['std'] / (1.0 - loo_ref.row_lmax(r, n, a['block']))      # tests/test_gpu_loo.py: _ratio32
            add('held-out mu', 'abs', got['mu'].ravel(), r['mu'], allow); add('held-out std', 'abs', got['sd'], r['std'], allow)
        add('lev', 'abs', got['lev'], r['lev'], (1e-9 if dtype == 'f64' else 1e-5) * np.maximum(r['lev'], 1e-3))
        st = got['stats']
        add('stats n, blocks', 'exact', np.array([st['n'], st['blocks']]), np.array([n, -(-n // a['block'])]), None)
        e = np.ravel(yl) - got['mu'].ravel(); var = got['sd'] ** 2
        marg = -0.5 * (e * e / var + np.log(2 * np.pi * var))
        tol = 4 * parity.bound64(n)                                                         # tests/test_gpu_loo.py: test_stats
        add('sum_e2', 'abs', st['sum_e2'], np.sum(e * e), tol * np.sum(e * e))
        add('sum_abs_e', 'abs', st['sum_abs_e'], np.sum(np.abs(e)), tol * np.sum(np.abs(e)))
        add('sum_log_marginal', 'abs', st['sum_log_marginal'], np.sum(marg), tol * np.sum(np.abs(marg)))
        add('max_leverage', 'exact', st['max_leverage'], got['lev'].max(), None)
        if a['block'] == 1:
            add('sum_log_joint', 'exact', st['sum_log_joint'], st['sum_log_marginal'], None)
        else:
            add('sum_log_joint', 'abs', st['sum_log_joint'], r['stats'][4], EPS[dtype] / (1 - r['lmax'].max()) * np.sum(np.abs(r['joint'])))
    elif ep in ('select', 'select_iv'):
        C = pred_cov_ref.factor(Xs, Li, params, S, M)
        idx = got['idx']
        m = len(idx)
        add('idx type and range', 'exact', np.array([idx.dtype == np.int64, m == a['m'], idx.min() >= 0, idx.max() < len(C)]), np.ones(4, bool),
            None)
        if ep == 'select':
            ds, scores = R.replay(C, a['w'], idx)
            tol_pick = EPS['f64'] if dtype == 'f64' else T_SEL.ETA
        else:
            Qm = V.gram(C if a['ref_rows'] is None else C[a['ref_rows']], a['wr'])
            As, ds, scores, qs = V.replay(C, Qm, a['w'], idx)
            tol_pick = EPS['f64'] if dtype == 'f64' else T_IV.ETA
        recs += _replay_picks(ep, scores, idx, tol_pick)
        dref = ds[np.arange(m), idx]
        # var[j] = kappa dp_j: fp64 relative (the own fp64 tests), fp32 within ETA kappa (1 + d) (tests/test_gpu_select.py: fp32_ratios)
        add('var', 'abs', got['var'], kap * dref, EPS['f64'] * kap * dref if dtype == 'f64' else T_SEL.ETA * kap * (1.0 + dref))
        sd0 = np.sqrt(kap * (1.0 + ds[m]))
        add('std_after', 'abs', got['sd'], sd0, EPS[dtype] * sd0)
        if ep == 'select':
            add('gain', 'allclose', got['gain'], 0.5 * np.log1p(got['var'] / kap), (1e-12, 0.0))
        else:
            scale = kap * float((As[0] / (1.0 + ds[0])).max())
            tol = EPS['f64'] if dtype == 'f64' else T_IV.ETA
            add('red', 'abs', got['red'], kap * qs, tol * scale)
            iv0 = kap * float(np.trace(Qm))
            if dtype == 'f64':
                add('ivar', 'abs', got['ivar'], np.array([iv0, iv0 - kap * np.sum(qs)]), EPS['f64'] * scale)
            else:
                # kappa tr Q is a weighted sum of the diagonal of predict_cov's matrix over the reference rows, formed by the same fp32
                # Gram: its relative bound; ivar[1] follows from the identity below and red's bound
                add('ivar[0]', 'abs', got['ivar'][0], iv0, T_COV.BOUNDS['f32'] * iv0)
            add('ivar[0] - sum red = ivar[1]', 'abs', got['ivar'][0] - got['red'].sum() - got['ivar'][1], 0.0, 1e-12 * got['ivar'][0])
    elif ep == 'select_qei':
        F, P, ns = aux['F'], aux['P'], a['nsamp']
        add('F', 'relnorm', F, ref.sample(a['X'], al, Li, ns, seed=a['seed'] % 1000, mode=mode), T_SMP.BOUNDS[dtype])
        u = -F if a['minimize'] else F
        free = (np.ones(len(F), bool) if a['w'] is None else a['w'] > 0).copy()
        b, mstate = Q.start(ns, a['best'], 0.01, a['minimize'], P)
        qei = [Q.qei_of(mstate, b)]
        bound = T_QEI._bound(ns)
        idx = got['idx']
        legal, sc_got, sc_best = [], [], []
        for j, p in enumerate(idx.tolist()):
            sc = Q.scores(u, mstate)
            if j == 0:
                add('score0', 'abs', got['score0'], sc, bound * np.abs(sc))
            rows = np.flatnonzero(free)
            top = sc[rows].max()
            # a pick within the own test's tie precondition (4 x the bound) of the best eligible score; exact zeros go to the lowest row
            legal.append(bool(free[p]) and (p == rows[0] if top == 0.0 else True))
            sc_got.append(sc[p]); sc_best.append(top)
            free[p] = False
            mstate = np.maximum(mstate, u[p])
        qei.append(Q.qei_of(mstate, b))
        add('picks are eligible and distinct', 'exact', np.array(legal), np.ones(len(idx), bool), None)
        add('picks near-optimal in the replay', 'abs', np.array(sc_got), np.array(sc_best), 4 * bound * np.abs(sc_best))
        add('gain', 'abs', got['gain'], np.array(sc_got), bound * np.abs(sc_got))
        add('mstate', 'exact', got['mstate'], mstate, None)
        add('qei', 'abs', got['qei'], np.array(qei), bound * np.abs(qei))
    else:
        raise ValueError(ep)
    return recs


# ---- failing calls -------------------------------------------------------------------------------------------------------------------------
ERRORS = {'nonfinite': (FloatingPointError, -4), 'notpd': (np.linalg.LinAlgError, -3), 'arg': (ValueError, -1)}


def failing_call(eng, a):
    """make the failing call; returns (exception or None, True / False / None: were the outputs the header promises left untouched)"""
    ep, al, Li, X = a['ep'], a['alpha'], a['Li'], a['X']
    untouched = None
    try:
        if hasattr(eng, 'lib'):                                  # the C ABI itself, with outputs filled beforehand
            from scfgp_amd._lib import dptr, _c_i64_p
            alv = np.ascontiguousarray(al, np.float64).ravel(); Lv = np.ascontiguousarray(Li, np.float64)
            Xv = np.ascontiguousarray(X, np.float64); n = Xv.shape[0]
            if ep == 'forget':
                outs = [np.full(alv.size, 3.0), np.full(Lv.shape, 3.0), np.full(n, 3.0), np.full(n, 3.0), np.full(8, 3.0)]
                rc = eng.lib.scfgp_forget(eng.ctx, dptr(Xv), dptr(np.ascontiguousarray(a['y'])), n, dptr(alv), dptr(Lv), 0,
                                          *[dptr(o) for o in outs])
            elif ep == 'loo':
                outs = [np.full(8, 3.0)]
                mu = np.full(n, 3.0); sd = np.full(n, 3.0)
                rc = eng.lib.scfgp_loo(eng.ctx, dptr(Xv), dptr(np.ascontiguousarray(a['y'])), n, dptr(alv), dptr(Lv), 0, a['block'], dptr(mu),
                                       dptr(sd), None, dptr(outs[0]))
            elif ep == 'sample_argmax':
                idx = np.full(a['nsamp'], 3, np.int64); val = np.full(a['nsamp'], 3.0)
                outs = [idx, val]
                rc = eng.lib.scfgp_sample_argmax(eng.ctx, dptr(Xv), n, None, dptr(alv), dptr(Lv), a['nsamp'], a['seed'] % 1000, 0, 0,
                                                 idx.ctypes.data_as(_c_i64_p), dptr(val))
            elif ep == 'predict_gradcov':
                D = Xv.shape[1]
                outs = [np.full((n, D), 3.0), np.full((n, D), 3.0), np.full((n, D, D), 3.0), np.full((D, D), 3.0)]
                rc = eng.lib.scfgp_predict_gradcov(eng.ctx, dptr(Xv), n, dptr(np.ascontiguousarray(a['w'], np.float64)), dptr(alv), dptr(Lv), 0,
                                                   *[dptr(o) for o in outs])
            elif ep == 'predict_pd':
                import ctypes
                grid = np.ascontiguousarray(a['grid'], np.float64); nd, ng = grid.shape
                dims = np.ascontiguousarray(a['dims'], np.int32)
                outs = [np.full((nd, ng), 3.0), np.full((nd, ng), 3.0), np.full((nd, ng, ng), 3.0), np.full((nd, n, ng), 3.0)]
                rc = eng.lib.scfgp_predict_pd(eng.ctx, dptr(Xv), n, None, dptr(alv), dptr(Lv), dims.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                              nd, dptr(grid), ng, 0, *[dptr(o) for o in outs])
            else:
                outs = None
            if outs is not None:
                untouched = all(bool(np.all(o == 3)) for o in outs)
                if rc == -4:
                    raise FloatingPointError(eng.last_error())
                eng._check(rc, ep)
                return None, untouched
        call(eng, a)
    except (FloatingPointError, np.linalg.LinAlgError, ValueError) as e:
        return e, untouched
    return None, untouched


# ---- the runner ----------------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300))


class Runner(object):
    """one context through one schedule.  make_engine(D, S, M, dtype) builds the context under test and every twin.  `ci`: a case number
    of CASES, whose schedule make_schedule(ci) is; or a tuple (D, S, M, dtype), with explicit steps given to run() (the geometry sweep).
    `mirror`: the dtype of a second context that lives through the same schedule and makes every posterior step's call once more, its
    outputs compared bit for bit where F16X3_EQUAL lists them (d).  A step with `row0_of` takes row 0 of that earlier step's arguments
    and is compared with its outputs where ROW_ALONE lists them (c)."""

    def __init__(self, ci, make_engine, twins=True, on_records=None, mirror=None, collect=False):
        if isinstance(ci, tuple):
            self.D, self.S, self.M, self.dtype = ci
        else:
            (self.D, self.S, self.M), self.dtype = CASES[ci]
        self.ci = ci
        self.mirror = mirror
        self.failures = [] if collect else None       # collect: the records that miss are listed here, the schedule goes on
        self.make_engine = make_engine
        self.twins = twins
        self.on_records = on_records
        self.fit = Fit(self.D, self.S, self.M)
        self.eng = make_engine(self.D, self.S, self.M, self.dtype)
        self.engines = [self.eng] + ([make_engine(self.D, self.S, self.M, mirror)] if mirror is not None else [])
        self.log = []
        self.prev = None
        self.kept = {}                        # step number -> (arguments, outputs) of the steps a later `row0_of` names
        self.min_pivot2 = []
        self.counts = dict(twin=0, records=0, failing=0, row0=0, mirror=0)

    def close(self):
        for e in self.engines:
            e.close()

    def _where(self, i):
        return 'step %d of case %s %s %s; steps so far: %s' % (i, self.ci, (self.D, self.S, self.M), self.dtype, self.log)

    def _resident(self):
        f = self.fit
        X, y = f.X(), f.y()
        for e in self.engines:
            e.set_data(X, y)
        f.resident = (X, y); f.resident_in_fit = True

    def _twin(self, a):
        f = self.fit
        t = self.make_engine(self.D, self.S, self.M, self.dtype)
        try:
            t.set_params(f.params)
            t.set_x_scaler(f.xs)
            if f.ys is not None:
                t.set_y_scaler(f.ys)
            for k, v in f.options.items():
                t.set_option(k, v)
            if a['ep'] == 'loo' and a.get('resident'):
                t.set_data(*f.resident)
            return call(t, a)
        finally:
            t.close()

    def run(self, steps=None):
        steps = make_schedule(self.ci) if steps is None else steps
        self.row0_wanted = {st['row0_of'] for st in steps if 'row0_of' in st}
        for i, st in enumerate(steps):
            self.log.append(' '.join([st['op']] + ['%s=%s' % (k, st[k]) for k in ('ep', 'T', 'mode', 'err', 'algo', 'N') if k in st]))
            try:
                self.step(i, st)
            except AssertionError as e:
                raise AssertionError('%s\n%s' % (e, self._where(i)))
            except Exception as e:
                raise AssertionError('%s: %s\n%s' % (type(e).__name__, e, self._where(i)))
        return self.counts

    def step(self, i, st):
        f, eng, dtype, D, S, M = self.fit, self.eng, self.dtype, self.D, self.S, self.M
        ctol, gtol, ptol = SEQ_TOL[dtype]
        op = st['op']
        if op == 'xscaler':
            f.xs = x_scaler(st['algo'], D); f.touch()
            for e in self.engines:
                e.set_x_scaler(f.xs)
            if f.Xraw is not None:
                self._resident()
        elif op == 'yscaler':
            f.ys = y_scaler(st['algo']); f.touch()
            for e in self.engines:
                e.set_y_scaler(f.ys)
            if f.Xraw is not None:
                self._resident()
        elif op == 'params':
            f.params = new_params(np.random.default_rng(st['seed']), D, S, M); f.touch()
            for e in self.engines:
                e.set_params(f.params)
        elif op == 'data':
            rng = np.random.default_rng(st['seed'])
            f.Xraw = raw_rows(rng, st['N'], D); f.yraw = raw_targets(rng, f.Xraw); f.touch()
            self._resident()
        elif op == 'option':
            rng = np.random.default_rng(st['seed'])
            name, values = OPTIONS[int(rng.integers(len(OPTIONS)))]
            v = int(rng.choice(values)); eng.set_option(name, v); f.options[name] = v; self.log[-1] += ' %s=%d' % (name, v)
        elif op in ('eval', 'rows', 'train'):
            # the round-3 sequence test's training calls and tolerances, against the oracle (no twin: the precision level of an fp32
            # context is legitimately sticky)
            X, y = f.resident
            if op == 'eval':
                wg = bool(st['seed'] % 2)
                c, g, alpha, Li = eng.eval(want_grad=wg)
                c0, g0, a0, L0 = O.value_and_grad(X, y, f.params, S, M)
                assert abs(float(c) - c0) < ctol * max(1.0, abs(c0)), ('eval cost', float(c), c0)
                assert rel(alpha, a0) < max(ptol, 0 if dtype == 'f64' else 1e-3), ('eval alpha', rel(alpha, a0))
                if wg:
                    assert rel(g, g0) < gtol, ('eval grad', rel(g, g0))
                    parity.oracle_check((c, g, alpha, Li), X, y, f.params, S, M, dtype, alpha_li=dtype == 'f64', label='sequence')
            elif op == 'rows':
                rng = np.random.default_rng(st['seed'])
                n = int(rng.choice([1, 10, max(1, X.shape[0] // 2), X.shape[0]]))
                idx = rng.integers(0, X.shape[0], n)
                c, g, alpha, Li = eng.eval_rows(idx, True)
                c0, g0, a0, L0 = O.value_and_grad(X[idx], y[idx], f.params, S, M)
                assert abs(float(c) - c0) < ctol * max(1.0, abs(c0)), ('eval_rows cost', float(c), c0)
                assert rel(g, g0) < gtol, ('eval_rows grad', rel(g, g0))
            else:
                eng.opt_init('adam', learning_rate=1e-3)
                hist, alpha, Li = eng.train(2)
                c0, g0, a0, L0 = O.value_and_grad(X, y, f.params, S, M)
                assert abs(hist[0] - c0) < ctol * max(1.0, abs(c0)), ('train cost', hist[0], c0)
                f.params = eng.get_params(); f.touch()
                c1, _, _, _ = O.value_and_grad(X, y, f.params, S, M)
                c, _, alpha, Li = eng.eval(want_grad=False)
                assert abs(float(c) - c1) < ctol * max(1.0, abs(c1)), ('cost after train', float(c), c1)
        elif op == 'fail':
            a = materialise(st, f)
            exc, untouched = failing_call(eng, a)
            want = ERRORS[st['err']][0]
            assert isinstance(exc, want), ('the documented error', want.__name__, repr(exc))
            assert untouched is not False, 'a failing call wrote to its outputs'
            self.counts['failing'] += 1
            self.prev = None
            return
        elif op == 'post':
            if 'row0_of' in st:
                a = _row0(self.kept[st['row0_of']][0], st['T'])
            else:
                a = prepare(eng, materialise(st, f), f)
                self.log[-1] += used_draw(a)
            got = call(eng, a)
            aux = auxiliary(eng, a, got, f)
            if i in self.row0_wanted:
                self.kept[i] = (dict(a), got)
            if self.twins:
                twin = self._twin(a)
                assert got.keys() == twin.keys()
                for k in got:
                    assert same_bits(got[k], twin[k]), ('(a) output %r differs from a fresh context\'s' % k)
                self.counts['twin'] += 1
            recs = records(a, got, aux, f, dtype, self.prev)
            if 'row0_of' in st and row_alone(a):
                r0 = row0_records(a, got, self.kept[st['row0_of']][1], bits=getattr(eng, 'ROW_BITS', True))
                recs += r0; self.counts['row0'] += len(r0)
            if self.mirror is not None:
                rm = mirror_records(a, got, call(self.engines[1], a), self.mirror)
                recs += rm; self.counts['mirror'] += len(rm)
            if self.on_records is not None:
                self.on_records(i, a, got, recs)
            for r in recs:
                try:
                    evaluate(r)
                except AssertionError as e:
                    msg = '%s%s %s' % ('' if str(r[0]).startswith('(') else '(b) ', a['ep'], e)
                    if self.failures is None:
                        raise AssertionError(msg)
                    self.failures.append('step %d (%s): %s' % (i, self.log[-1], msg))
            self.counts['records'] += len(recs)
            self.prev = got if st['mode'] == 'raw' else None
            # condition and forget move the fit
            if a['ep'] == 'condition':
                f.Xraw = np.vstack([f.Xraw, a['Xraw']]); f.yraw = np.vstack([f.yraw, a['yraw']]); f._cache = a['new_factors']
            elif a['ep'] == 'forget':
                self.min_pivot2.append(a['min_pivot2'])
                keep = np.setdiff1d(np.arange(f.Xraw.shape[0]), a['rows'])
                f.Xraw, f.yraw = f.Xraw[keep], f.yraw[keep]; f._cache = a['new_factors']; f.resident_in_fit = False
            return
        else:
            raise ValueError(op)
        if op != 'post':
            self.prev = None
