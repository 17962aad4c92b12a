"""
HipEngine: thin, typed Python face of one scfgp_ctx (one GPU, one shard of rows).

It adds nothing numerically -- every method is one call through the C ABI of
libscfgp_hip.so (include/scfgp_hip.h) with numpy buffers allocated for the caller,
and turns error codes into the exceptions the reference raises
(numpy.linalg.LinAlgError for a failed Cholesky, SCFGP/SCFGP.py:106).
"""
import ctypes as C
import sys

import numpy as np

from . import _lib
from ._lib import SCFGP_F16X3, SCFGP_F32, SCFGP_F64, dptr

# 'f16x3': fp32 mode whose four N-sized products (apply and Gram) run as a three-term fp16 split (include/scfgp_hip.h: SCFGP_F16X3) -- a
# labelled secondary mode, chosen explicitly, never a default
_DTYPES = {'f64': SCFGP_F64, 'float64': SCFGP_F64, 'f32': SCFGP_F32, 'float32': SCFGP_F32, 'f16x3': SCFGP_F16X3,
           SCFGP_F64: SCFGP_F64, SCFGP_F32: SCFGP_F32, SCFGP_F16X3: SCFGP_F16X3}


def num_params(D, S, M):
    """Length of the flat hyper-parameter vector (SCFGP/SCFGP.py:72)."""
    return 3 + D * S + M * S + S + M


def _scatter(g, cols, width, square=False):
    """(.., len(cols)) gradients -> (.., width), zero in the columns not listed; square: (.., len(cols), len(cols)) matrices ->
    (.., width, width), rows and columns alike"""
    out = np.zeros(g.shape[:-1] + (width,))
    out[..., cols] = g
    if square:
        g, out = out, np.zeros(g.shape[:-2] + (width, width))
        out[..., cols, :] = g
    return out


def _i64(a):
    return None if a is None else a.ctypes.data_as(_lib._c_i64_p)


def _seed(seed):
    return int(seed) & (2 ** 64 - 1)


def _count(n, lo, hi):
    """n, or 0 outside lo..hi: the library refuses such a count before it writes, so the outputs sized by it stay empty"""
    return n if lo <= n <= hi else 0


class PeerFailed(RuntimeError):
    """Row shards: another rank failed in this evaluation (SCFGP_EPEER); no rank's results are valid."""


class HipEngine(object):

    def __init__(self, D, S, M, dtype='f64', device=0, stream=None):
        self.lib = _lib.load()
        self.D, self.S, self.M = int(D), int(S), int(M)
        self.J = self.S + self.M
        self.K = 2 * self.J
        self.P = num_params(D, S, M)
        self.dtype = _DTYPES[dtype]
        self.device = int(device)
        self.ctx = C.c_void_p()
        self._pool = {}
        rc = self.lib.scfgp_create(C.byref(self.ctx), self.D, self.S, self.M, self.dtype, int(device),
                                   C.c_void_p(stream) if stream else None)
        if rc != 0:
            # a failed create still hands back the half-built context (for its error message): it must be destroyed
            msg = self.lib.scfgp_last_error(self.ctx).decode() if self.ctx else ''
            self.close()
            raise RuntimeError('scfgp_create failed (%d): %s' % (rc, msg))
        self.N = 0
        self.n_global = 0

    _pool = None
    nonfinite = 'raise'            # 'return': a NaN / Inf cost comes back as a value (what the reference's functions do)

    def close(self):
        if getattr(self, 'ctx', None):
            self.lib.scfgp_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- error mapping ----------------------------------------------------------------
    def _check(self, rc, what):
        if rc == 0:
            return
        msg = self.lib.scfgp_last_error(self.ctx).decode()
        if rc == -3:
            raise np.linalg.LinAlgError('%s: %s' % (what, msg))
        if rc == -4:
            # the outputs have been delivered; the reference's Theano functions do not trap a NaN / Inf cost (SCFGP/SCFGP.py:249-258
            # treats it as "no improvement"), so the callable triple asks for it back (funcs.py), a direct caller gets the error
            if self.nonfinite == 'return':
                return
            raise FloatingPointError('%s: %s' % (what, msg))
        if rc == -1:
            raise ValueError('%s: %s' % (what, msg))
        if rc == _lib.SCFGP_EPEER:
            raise PeerFailed('%s: %s' % (what, msg))
        raise RuntimeError('%s failed (%d, %s): %s' % (what, rc, _lib.ERRORS.get(rc, '?'), msg))

    # -- state --------------------------------------------------------------------------
    def set_params(self, params):
        p = np.ascontiguousarray(params, dtype=np.float64).ravel()
        if p.size != self.P:
            raise ValueError('expected %d parameters, got %d' % (self.P, p.size))
        self._check(self.lib.scfgp_set_params(self.ctx, dptr(p), self.P), 'set_params')

    def get_params(self):
        p = np.empty(self.P)
        self._check(self.lib.scfgp_get_params(self.ctx, dptr(p), self.P), 'get_params')
        return p

    @staticmethod
    def _check_xy(X, y, D):
        # Theano's dmatrix inputs reject anything but 2-d float64 (SCFGP/SCFGP.py:95)
        if not isinstance(X, np.ndarray) or X.dtype != np.float64 or X.ndim != 2:
            raise TypeError('X must be a 2-d float64 ndarray')
        if X.shape[1] != D:
            raise ValueError('X has %d columns, expected %d' % (X.shape[1], D))
        if y is not None:
            if not isinstance(y, np.ndarray) or y.dtype != np.float64 or y.ndim != 2 or y.shape != (X.shape[0], 1):
                raise TypeError('y must be a float64 ndarray of shape (N,1)')

    def set_data(self, X, y, n_global=None):
        self._check_xy(X, y, self.D)
        X = np.ascontiguousarray(X); y = np.ascontiguousarray(y)
        N = X.shape[0]
        self.N = N
        self.n_global = int(n_global) if n_global else N
        self._check(self.lib.scfgp_set_data(self.ctx, dptr(X), dptr(y), N, self.n_global), 'set_data')

    # -- whole evaluations ------------------------------------------------------------------
    def _fresh(self, shape):
        """An output array nobody else holds.  The reference's functions return freshly allocated arrays on every call; a
        fresh K x K float64 array (35.7 MB at K = 2112) costs the host ~1.4 ms per call in page faults and their release
        (measured against reused buffers, tests/gpu_wall.py).  So arrays handed out earlier are kept in a small pool and one
        is used again only once the caller has dropped every reference to it (views hold one through .base): from the
        caller's side it cannot be told from a new array."""
        pool = self._pool.setdefault(shape, [])
        for i in range(len(pool)):
            if sys.getrefcount(pool[i]) == 2:                  # the pool's reference + getrefcount's argument
                return pool[i]
        a = np.empty(shape)
        if len(pool) < 4:
            pool.append(a)
        return a

    def _outputs(self, want_grad, factors=True):
        cost = np.zeros(1)
        grad = np.empty(self.P) if want_grad else None
        alpha = self._fresh((self.K, 1)) if factors else None
        Li = self._fresh((self.K, self.K)) if factors else None
        return cost, grad, alpha, Li

    def eval(self, X=None, y=None, want_grad=True):
        """(cost 0-d, grad|None, alpha (K,1), Li (K,K)); X=None evaluates the resident rows."""
        cost, grad, alpha, Li = self._outputs(want_grad)
        if X is not None:
            self._check_xy(X, y, self.D)
            X = np.ascontiguousarray(X); y = np.ascontiguousarray(y)
            self.N = X.shape[0]; self.n_global = self.N
        rc = self.lib.scfgp_eval(self.ctx, dptr(X), dptr(y), 0 if X is None else X.shape[0], int(bool(want_grad)),
                                 dptr(cost), dptr(grad), dptr(alpha), dptr(Li))
        self._check(rc, 'eval')
        return cost.reshape(()), grad, alpha, Li

    def eval_rows(self, idx, want_grad=True):
        """Evaluation on the rows `idx` of the resident data set (device-side gather; per-batch N)."""
        idx = np.ascontiguousarray(idx, dtype=np.int64).ravel()
        cost, grad, alpha, Li = self._outputs(want_grad)
        rc = self.lib.scfgp_eval_rows(self.ctx, idx.ctypes.data_as(C.POINTER(C.c_int64)), idx.size, int(bool(want_grad)),
                                      dptr(cost), dptr(grad), dptr(alpha), dptr(Li))
        self._check(rc, 'eval_rows')
        return cost.reshape(()), grad, alpha, Li

    def predict(self, Xs, alpha, Li):
        """pred_func (SCFGP/SCFGP.py:138-148): returns mu (T,1), std (T,)."""
        self._check_xy(Xs, None, self.D)
        Xs = np.ascontiguousarray(Xs)
        alpha, Li = self._factors(alpha, Li)
        T = Xs.shape[0]
        mu = np.empty((T, 1)); sd = np.empty(T)
        self._check(self.lib.scfgp_predict(self.ctx, dptr(Xs), T, dptr(alpha), dptr(Li), dptr(mu), dptr(sd)), 'predict')
        return mu, sd

    @staticmethod
    def scaler_key(scaler):
        """Contents of a fitted Scaler (it is refitted IN PLACE by SCFGP.set_data, so identity says nothing)."""
        d = scaler.data
        return (scaler.algo,) + tuple((k, np.asarray(d[k], dtype=np.float64).tobytes()) for k in sorted(d) if np.size(d[k]))

    SCALER_MODES = {'min-max': 1, 'normal': 2, 'inv-normal': 3, 'auto-normal': 4, 'auto-inv-normal': 5}

    def set_x_scaler(self, scaler):
        """Register a fitted scfgp_amd.scaler.Scaler so predict_raw can transform inputs on the device."""
        d = scaler.data
        arr = lambda k: np.ascontiguousarray(d[k], dtype=np.float64) if k in d and np.ndim(d[k]) else None
        bufs = [arr(k) for k in ('min', 'max', 'boxcox', 'mu', 'std')]
        for b in bufs:
            if b is not None and b.size != self.D:
                raise ValueError('scaler was fitted on %d columns, engine has D=%d' % (b.size, self.D))
        self._check(self.lib.scfgp_set_x_scaler(self.ctx, self.SCALER_MODES[scaler.algo], *[dptr(b) for b in bufs]),
                    'set_x_scaler')
        self._xcols = list(d['cols'])

    def predict_raw(self, Xs_raw, alpha, Li):
        """pred_func on UNSCALED inputs: column selection here, the element-wise transform on the GPU."""
        Xs = np.ascontiguousarray(np.asarray(Xs_raw, dtype=np.float64)[:, self._xcols])
        alpha = np.ascontiguousarray(alpha, dtype=np.float64).reshape(-1)
        Li = np.ascontiguousarray(Li, dtype=np.float64)
        T = Xs.shape[0]
        mu = np.empty((T, 1)); sd = np.empty(T)
        self._check(self.lib.scfgp_predict_raw(self.ctx, dptr(Xs), T, dptr(alpha), dptr(Li), dptr(mu), dptr(sd)), 'predict_raw')
        return mu, sd

    METRICS = ('MAE', 'NMAE', 'MSE', 'NMSE', 'MNLP', 'SCORE')

    def set_y_scaler(self, scaler):
        """Register the fitted single-column target scaler for predict_y."""
        d = scaler.data
        val = lambda k: float(np.asarray(d[k]).reshape(-1)[0]) if k in d and np.size(d[k]) else 0.0
        if len(d['cols']) != 1:
            raise ValueError('the y scaler must have exactly one column')
        self._check(self.lib.scfgp_set_y_scaler(self.ctx, self.SCALER_MODES[scaler.algo],
                                                *[val(k) for k in ('min', 'max', 'boxcox', 'mu', 'std')]), 'set_y_scaler')

    def predict_y(self, Xs_raw, alpha, Li, ys=None):
        """SCFGP.predict (SCFGP/SCFGP.py:278-294) entirely on the device: X scaling, pred_func, y-scaler backward
        transform of the mean and of the +-1 std band and, with raw targets ys, the six metrics.
        Returns mu_y (T,1), std_y (T,1), metrics dict or None."""
        Xs = np.asarray(Xs_raw, dtype=np.float64)
        if getattr(self, '_xcols', None) is not None:
            Xs = Xs[:, self._xcols]
        Xs = np.ascontiguousarray(Xs)
        alpha = np.ascontiguousarray(alpha, dtype=np.float64).reshape(-1)
        Li = np.ascontiguousarray(Li, dtype=np.float64)
        T = Xs.shape[0]
        mu = np.empty((T, 1)); sd = np.empty((T, 1)); met = np.empty(6)
        if ys is not None:
            ys = np.ascontiguousarray(ys, dtype=np.float64).reshape(-1)
            if ys.size != T:
                raise ValueError('ys has %d entries for %d test rows' % (ys.size, T))
        self._check(self.lib.scfgp_predict_y(self.ctx, dptr(Xs), T, dptr(alpha), dptr(Li), dptr(ys), dptr(mu), dptr(sd),
                                             dptr(met) if ys is not None else None), 'predict_y')
        return mu, sd, (dict(zip(self.METRICS, met.tolist())) if ys is not None else None)

    # -- arguments of the posterior and pool entry points -------------------------------------------------
    def _mode(self, who, table, mode, rows=True):
        """(the library's number of `mode`, the columns the registered X scaler kept -- None where rows go in as they are); rows=False:
        the call brings no rows, so no scaler is asked for"""
        if mode not in table:
            raise ValueError('%s: mode must be one of %s' % (who, sorted(table)))
        m = table[mode]
        cols = getattr(self, '_xcols', None) if m and rows else None
        if m and rows and cols is None:
            raise ValueError('%s: mode %r needs a registered X scaler (set_x_scaler)' % (who, mode))
        return m, cols

    def _raw_cols(self, who, raw):
        """_mode for the entry points with a `raw` flag"""
        cols = getattr(self, '_xcols', None) if raw else None
        if raw and cols is None:
            raise ValueError('%s: raw rows need a registered X scaler (set_x_scaler)' % who)
        return cols

    def _rows(self, X, name, cols=None):
        """X as the library reads it: contiguous (n, D) float64, the columns `cols` of it; a copy only where one is needed"""
        X = np.asarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise TypeError('%s must be a 2-d float64 array' % name)
        if cols is not None:
            X = X[:, cols]
        X = np.ascontiguousarray(X)
        if X.shape[1] != self.D:
            raise ValueError('%s has %d columns, expected %d' % (name, X.shape[1], self.D))
        return X

    @staticmethod
    def _weights(v, n, name):
        """n weights (or targets) as a flat contiguous float64 array; None stays None"""
        if v is None:
            return None
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
        if v.size != n:
            raise ValueError('%s has %d entries for %d rows' % (name, v.size, n))
        return v

    def _Li(self, Li):
        Li = np.ascontiguousarray(Li, dtype=np.float64)
        if Li.shape != (self.K, self.K):
            raise ValueError('Li has the wrong shape for K=%d' % self.K)
        return Li

    def _factors(self, alpha, Li):
        alpha = np.ascontiguousarray(alpha, dtype=np.float64).reshape(-1)
        Li = np.ascontiguousarray(Li, dtype=np.float64)
        if alpha.size != self.K or Li.shape != (self.K, self.K):
            raise ValueError('alpha/Li have the wrong shape for K=%d' % self.K)
        return alpha, Li

    @staticmethod
    def _wanted(who, want, allowed, some=False):
        """`want` as a tuple of names out of `allowed`; some: at least one (each entry point keeps its wording)"""
        want = (want,) if isinstance(want, str) else tuple(want)
        if some:
            if not want or any(k not in allowed for k in want):
                raise ValueError('%s: want must name some of %s' % (who, allowed))
        else:
            for k in want:
                if k not in allowed:
                    raise ValueError('%s: want holds %r; allowed: %s' % (who, k, allowed))
        return want

    def _check_undelivered(self, rc, who):
        """_check for the entry points that deliver nothing when the result is not finite: -4 is an error whatever self.nonfinite says
        (unlike an evaluation's NaN cost, which comes with its outputs).  predict, predict_raw, predict_y, predict_grad,
        predict_gradcov, sample_weights, sample and predict_cov go through the plain _check instead, so under nonfinite = 'return'
        they hand back what the library wrote; tests/test_engine_marshal.py pins which method does which."""
        if rc == -4:
            raise FloatingPointError('%s: %s' % (who, self.last_error()))
        self._check(rc, who)

    PREDICT_GRAD_MODES = {'scaled': 0, 'raw': 1, 'y': 2}

    def predict_grad(self, Xs, alpha, Li, mode='scaled', want_std=True):
        """Gradients of pred_func's outputs in its inputs (include/scfgp_hip.h: scfgp_predict_grad).  mode 'scaled': Xs as predict
        takes it; 'raw': unscaled Xs through the registered X scaler, as predict_raw; 'y': that and the y scaler, as predict_y.
        Returns mu (T,1), std (T,), dmu (T,D), dstd (T,D) (None without want_std); mu and std are those of the matching predict call, bit
        for bit.  In the 'raw' / 'y' modes dmu, dstd are (T, D_raw): the constant columns the X scaler dropped get zero gradients."""
        m, cols = self._mode('predict_grad', self.PREDICT_GRAD_MODES, mode)
        X = self._rows(Xs, 'Xs', cols)
        alpha, Li = self._factors(alpha, Li)
        T = X.shape[0]
        mu = np.empty((T, 1)); sd = np.empty(T)
        dmu = np.empty((T, self.D)); dsd = np.empty((T, self.D)) if want_std else None
        self._check(self.lib.scfgp_predict_grad(self.ctx, dptr(X), T, dptr(alpha), dptr(Li), m, dptr(mu), dptr(sd), dptr(dmu), dptr(dsd)),
                    'predict_grad')
        if cols is not None:
            D_in = np.shape(Xs)[1]
            dmu, dsd = _scatter(dmu, cols, D_in), (None if dsd is None else _scatter(dsd, cols, D_in))
        return mu, sd, dmu, dsd

    GRADCOV_MODES = {'scaled': 0, 'raw': 1}
    GRADCOV_OUTPUTS = ('dmu', 'dvar', 'dcov', 'asub')

    def gradcov_points_per_chunk(self, want_cov):
        """Points per chunk of predict_gradcov (the formula of include/scfgp_hip.h).  want_cov: the call asks for 'dcov' or 'asub', so
        a chunk carries a D x D array per point and stays within the 64 MiB slot budget."""
        q = min(self.D, self.S)
        ppg = 64 // q
        n = 32768 // (ppg * q) * ppg
        if want_cov:
            n = min(n, max(1, (64 << 20) // (8 * self.D * self.D)))
        return n

    def predict_gradcov(self, Xs, alpha, Li, w=None, mode='scaled', want=('dmu', 'dvar', 'asub')):
        """Posterior distribution of the input gradient (include/scfgp_hip.h: scfgp_predict_gradcov): a dict with the outputs named in
        `want` -- 'dmu' (T, D) the mean (predict_grad's dmu, bit for bit), 'dvar' (T, D) the marginal variances, 'dcov' (T, D, D) the
        covariance of grad f at every row, 'asub' (D, D) the active-subspace matrix sum_t w_t (m_t m_t^T + Sigma_t) / sum_t w_t of the
        call's rows (w: T weights >= 0, None: all 1).  mode 'scaled': Xs as predict takes it; 'raw': unscaled Xs through the registered
        X scaler, outputs in the D_raw raw columns with zeros for the columns the scaler dropped, as predict_grad.  Needs min(D, S) <=
        64."""
        m, cols = self._mode('predict_gradcov', self.GRADCOV_MODES, mode)
        want = self._wanted('predict_gradcov', want, self.GRADCOV_OUTPUTS, some=True)
        X = self._rows(Xs, 'Xs', cols)
        alpha, Li = self._factors(alpha, Li)
        T, D = X.shape[0], self.D
        w = self._weights(w, T, 'w')
        shapes = {'dmu': (T, D), 'dvar': (T, D), 'dcov': (T, D, D), 'asub': (D, D)}
        out = {k: np.empty(shapes[k]) for k in self.GRADCOV_OUTPUTS if k in want}
        self._check(self.lib.scfgp_predict_gradcov(self.ctx, dptr(X), T, dptr(w), dptr(alpha), dptr(Li), m,
                                                   *[dptr(out.get(k)) for k in self.GRADCOV_OUTPUTS]), 'predict_gradcov')
        if cols is not None:
            for k in out:
                out[k] = _scatter(out[k], cols, np.shape(Xs)[1], square=k in ('dcov', 'asub'))
        return out

    PD_MODES = {'scaled': 0, 'raw': 1}
    PD_OUTPUTS = ('pd', 'sd', 'cov', 'ice')

    def predict_pd(self, Xs, alpha, Li, dims, grid, w=None, mode='scaled', want=('pd', 'sd')):
        """Partial-dependence and ICE curves of single inputs over the pool rows Xs (include/scfgp_hip.h: scfgp_predict_pd): a dict with
        the outputs named in `want` -- 'pd' (ndim, G) the PD curve of every dimension in `dims` over its row of `grid` (ndim, G), 'sd'
        (ndim, G) its latent posterior standard deviation, 'cov' (ndim, G, G) its posterior covariance, 'ice' (ndim, T, G) the individual
        curves; all in scaled y units.  w: T weights >= 0 (None: all 1); rows of weight 0 count for 'ice' only.  mode 'scaled': Xs and the
        grid as predict takes them; 'raw': unscaled Xs through the registered X scaler, `dims` naming raw columns (none that the scaler
        dropped) and the grid in raw units of its column.  1 <= G <= 1024."""
        m, cols = self._mode('predict_pd', self.PD_MODES, mode)
        want = self._wanted('predict_pd', want, self.PD_OUTPUTS, some=True)
        Xs = self._rows(Xs, 'Xs', cols)
        dims = np.asarray(dims, dtype=np.int64).reshape(-1)
        if cols is not None:
            where = {int(cc): i for i, cc in enumerate(cols)}
            if any(int(d) not in where for d in dims):
                raise ValueError('predict_pd: dims names a column that the X scaler dropped or that does not exist')
            dims = np.array([where[int(d)] for d in dims], dtype=np.int64)
        grid = np.ascontiguousarray(grid, dtype=np.float64)
        if grid.ndim != 2 or grid.shape[0] != dims.size:
            raise ValueError('grid must be (ndim, G) with one row per entry of dims')
        alpha, Li = self._factors(alpha, Li)
        T, nd, G = Xs.shape[0], int(dims.size), int(grid.shape[1])
        w = self._weights(w, T, 'w')
        dims32 = np.ascontiguousarray(dims, dtype=np.int32)
        shapes = {'pd': (nd, G), 'sd': (nd, G), 'cov': (nd, G, G), 'ice': (nd, T, G)}
        out = {k: np.empty(shapes[k]) for k in self.PD_OUTPUTS if k in want}
        rc = self.lib.scfgp_predict_pd(self.ctx, dptr(Xs), T, dptr(w), dptr(alpha), dptr(Li), dims32.ctypes.data_as(C.POINTER(C.c_int)), nd,
                                       dptr(grid), G, m, *[dptr(out.get(k)) for k in self.PD_OUTPUTS])
        self._check_undelivered(rc, 'predict_pd')
        return out

    SAMPLE_MODES = {'scaled': 0, 'raw': 1, 'y': 2}

    def sample_weights(self, alpha, Li, nsamp, seed=0):
        """Weights of nsamp posterior sample functions (include/scfgp_hip.h: scfgp_sample_weights): W (K, nsamp) = alpha 1^T +
        sqrt(kappa) Li^T Z with Z drawn from `seed` by the library's counter-based generator; column s is the same for any nsamp."""
        alpha, Li = self._factors(alpha, Li)
        W = np.empty((self.K, int(nsamp)))
        self._check(self.lib.scfgp_sample_weights(self.ctx, dptr(alpha), dptr(Li), int(nsamp), _seed(seed), dptr(W)), 'sample_weights')
        return W

    def sample(self, Xs, alpha, Li, nsamp, seed=0, mode='scaled', noise=False):
        """nsamp posterior sample functions evaluated at the rows of Xs (include/scfgp_hip.h: scfgp_sample): (T, nsamp), column s =
        phi(x)^T w_s (+ sqrt(kappa) eps with noise).  mode 'scaled': Xs as predict takes it; 'raw': unscaled Xs through the registered
        X scaler, as predict_raw; 'y': that and the y scaler's backward transform of every sample, as predict_y."""
        m, cols = self._mode('sample', self.SAMPLE_MODES, mode)
        Xs = self._rows(Xs, 'Xs', cols)
        alpha, Li = self._factors(alpha, Li)
        T = Xs.shape[0]
        out = np.empty((T, max(int(nsamp), 0)))
        self._check(self.lib.scfgp_sample(self.ctx, dptr(Xs), T, dptr(alpha), dptr(Li), int(nsamp), _seed(seed), m, int(bool(noise)),
                                          dptr(out)), 'sample')
        return out

    def sample_argmax(self, Xs, alpha, Li, nsamp, seed=0, w=None, mode='scaled', minimize=False):
        """Per-sample maximisers over the pool Xs (include/scfgp_hip.h: scfgp_sample_argmax): (idx (nsamp,) int64, val (nsamp,)) with
        idx[s] the lowest eligible row at which sample function s of `sample` (same seed, no noise) is largest (minimize: smallest)
        and val[s] its value there, bit for bit what `sample` returns.  w (T,): row t is eligible iff w[t] > 0 (None: every row).
        mode as in `sample`; with 'y' the row is chosen in scaled units and val is in raw y units."""
        m, cols = self._mode('sample_argmax', self.SAMPLE_MODES, mode)
        Xs = self._rows(Xs, 'Xs', cols)
        T = Xs.shape[0]
        w = self._weights(w, T, 'w')
        alpha, Li = self._factors(alpha, Li)
        nsamp = int(nsamp)
        n = _count(nsamp, 1, 1024)
        idx = np.empty(n, dtype=np.int64); val = np.empty(n)
        rc = self.lib.scfgp_sample_argmax(self.ctx, dptr(Xs), T, dptr(w), dptr(alpha), dptr(Li), nsamp, _seed(seed), m, int(bool(minimize)),
                                          _i64(idx), dptr(val))
        self._check_undelivered(rc, 'sample_argmax')
        return idx, val

    ACQUIRE_KINDS = {'ucb': 0, 'pi': 1, 'ei': 2, 'logei': 3, 'mes': 4}
    ACQUIRE_MODES = {'scaled': 0, 'raw': 1}
    ACQUIRE_WANT = ('acq', 'argmax', 'mu', 'sd', 'grad')

    def acquire(self, Xs, alpha, Li, kind, best=None, xi=0.0, beta=None, fstar=None, w=None, mode='scaled', noise=False, minimize=False,
                want=('acq', 'argmax')):
        """Acquisition functions over the pool Xs (include/scfgp_hip.h: scfgp_acquire), in scaled y units.  kind 'ucb' (beta), 'pi',
        'ei', 'logei' (best, xi) or 'mes' (fstar: sampled maxima, what sample_argmax returns in val with mode 'scaled' / 'raw' and the
        same minimize).  noise: the predictive std sigma* instead of the latent sigma_f.  w (T,): row t is eligible iff w[t] > 0.  mode
        'scaled' or 'raw' (through the registered X scaler).  want: any of 'acq' (T,), 'argmax' (idx, val: the lowest eligible row with
        the largest value, and that value), 'mu' (T,), 'sd' (T,), 'grad' (T, D; (T, D_raw) in mode 'raw' with zero columns where the
        scaler dropped a constant column).  Returns a dict with the keys asked for ('argmax' gives 'idx' and 'val')."""
        if kind not in self.ACQUIRE_KINDS:
            raise ValueError('acquire: kind must be one of %s' % sorted(self.ACQUIRE_KINDS))
        m, cols = self._mode('acquire', self.ACQUIRE_MODES, mode)
        want = self._wanted('acquire', want, self.ACQUIRE_WANT)
        k = self.ACQUIRE_KINDS[kind]
        X = self._rows(Xs, 'Xs', cols)
        T = X.shape[0]
        w = self._weights(w, T, 'w')
        alpha, Li = self._factors(alpha, Li)
        if k == 0:
            if beta is None:
                raise ValueError("acquire: kind 'ucb' needs beta")
            par = np.array([beta], dtype=np.float64)
        elif k == 4:
            par = None
        else:
            if best is None:
                raise ValueError('acquire: kind %r needs best' % kind)
            par = np.array([best, xi], dtype=np.float64)
        if fstar is not None:
            fstar = np.ascontiguousarray(fstar, dtype=np.float64).reshape(-1)
        out = {}
        acq = np.empty(T) if 'acq' in want else None
        idx = np.empty(1, dtype=np.int64) if 'argmax' in want else None
        val = np.empty(1) if 'argmax' in want else None
        mu = np.empty(T) if 'mu' in want else None
        sd = np.empty(T) if 'sd' in want else None
        grad = np.empty((T, self.D)) if 'grad' in want else None
        rc = self.lib.scfgp_acquire(self.ctx, dptr(X), T, dptr(w), dptr(alpha), dptr(Li), k, dptr(par), 0 if par is None else par.size,
                                    dptr(fstar), 0 if fstar is None else fstar.size, m, int(bool(noise)), int(bool(minimize)), dptr(acq),
                                    _i64(idx), dptr(val), dptr(mu), dptr(sd), dptr(grad))
        self._check_undelivered(rc, 'acquire')
        if acq is not None:
            out['acq'] = acq
        if idx is not None:
            out['idx'] = int(idx[0]); out['val'] = float(val[0])
        if mu is not None:
            out['mu'] = mu
        if sd is not None:
            out['sd'] = sd
        if grad is not None:
            out['grad'] = _scatter(grad, cols, np.shape(Xs)[1]) if cols is not None else grad
        return out

    KG_WANT = ('kg', 'kg_hi', 'idx', 'val', 'm', 's')
    KG_DEFAULT_NODES = np.linspace(-5.0, 5.0, 31)

    def acquire_kg(self, Xc, alpha, Li, Xr=None, z=None, w=None, mode='scaled', noise=True, minimize=False, want=('kg', 'idx', 'val')):
        """Knowledge gradient of the candidates Xc (T, D) over the reference rows Xr (R <= 32768 rows; None: the candidates themselves,
        T <= 32768), in scaled y units (include/scfgp_hip.h: scfgp_acquire_kg).  z: the nodes, strictly increasing and holding exactly one
        0.0, 3..32 of them (None: linspace(-5, 5, 31)).  noise: the candidate is observed with noise (sigma*), the normal case.  w (T,):
        row t is eligible iff w[t] > 0.  mode 'scaled' or 'raw' (Xc and Xr through the registered X scaler).  want: any of 'kg' (T,: the
        lower bound), 'kg_hi' (T,: the upper bound), 'idx' (the lowest eligible row with the largest kg), 'val' (its kg; needs 'idx'),
        'm', 's' ((T, J) each: the node table).  Returns a dict with the keys asked for."""
        md, cols = self._mode('acquire_kg', self.ACQUIRE_MODES, mode)
        want = self._wanted('acquire_kg', want, self.KG_WANT)
        Xc = self._rows(Xc, 'Xc', cols)
        T = Xc.shape[0]
        R = 0
        if Xr is not None:
            Xr = self._rows(Xr, 'Xr', cols)
            R = Xr.shape[0]
        w = self._weights(w, T, 'w')
        z = np.ascontiguousarray(self.KG_DEFAULT_NODES if z is None else z, dtype=np.float64).reshape(-1)
        J = z.size
        alpha, Li = self._factors(alpha, Li)
        nj = _count(J, 3, 32)
        kg = np.empty(T) if 'kg' in want else None
        hi = np.empty(T) if 'kg_hi' in want else None
        idx = np.empty(1, dtype=np.int64) if 'idx' in want else None
        val = np.empty(1) if 'val' in want else None
        m = np.empty((T, nj)) if 'm' in want else None
        s = np.empty((T, nj)) if 's' in want else None
        rc = self.lib.scfgp_acquire_kg(self.ctx, dptr(Xc), T, dptr(w), dptr(Xr), R, dptr(alpha), dptr(Li), dptr(z), J, md, int(bool(noise)),
                                       int(bool(minimize)), dptr(kg), dptr(hi), _i64(idx), dptr(val), dptr(m), dptr(s))
        self._check_undelivered(rc, 'acquire_kg')
        out = {}
        for k, a in (('kg', kg), ('kg_hi', hi), ('m', m), ('s', s)):
            if a is not None:
                out[k] = a
        if idx is not None:
            out['idx'] = int(idx[0])
        if val is not None:
            out['val'] = float(val[0])
        return out

    def sample_grad(self, Xs, W, sidx=None, mode='scaled', want_val=True):
        """Values and input gradients of sample functions, one sample per row (include/scfgp_hip.h: scfgp_sample_grad): (val (T,),
        grad (T, D)) with val[t] = phi(x_t)^T W[:, sidx[t]] and grad[t] its gradient in x_t.  W (K, nsamp) as sample_weights returns
        it (any K-vectors: W = alpha[:, None] gives the mean); sidx (T,) ints in [0, nsamp), None: t % nsamp.  mode as in
        predict_grad: 'raw' chains grad through the X scaler and returns (T, D_raw) with zero columns where the scaler dropped a
        constant column; 'y' also maps val through the y scaler's backward transform and grad through its derivative.  val is None
        without want_val."""
        m, cols = self._mode('sample_grad', self.SAMPLE_MODES, mode)
        X = self._rows(Xs, 'Xs', cols)
        W = np.ascontiguousarray(W, dtype=np.float64)
        if W.ndim != 2 or W.shape[0] != self.K:
            raise ValueError('W must be (K, nsamp) with K=%d' % self.K)
        T, nsamp = X.shape[0], W.shape[1]
        if sidx is not None:
            sidx = np.ascontiguousarray(sidx, dtype=np.int64).reshape(-1)
            if sidx.size != T:
                raise ValueError('sidx has %d entries for %d rows' % (sidx.size, T))
        val = np.empty(T) if want_val else None
        grad = np.empty((T, self.D))
        rc = self.lib.scfgp_sample_grad(self.ctx, dptr(X), T, dptr(W), nsamp, _i64(sidx), m, dptr(val), dptr(grad))
        self._check_undelivered(rc, 'sample_grad')
        if cols is not None:
            grad = _scatter(grad, cols, np.shape(Xs)[1])
        return val, grad

    PREDICT_COV_MODES = {'scaled': 0, 'raw': 1}

    def predict_cov(self, Xa, Li, Xb=None, mode='scaled', noise=False):
        """Joint posterior covariance of the function values at the rows of Xa and Xb (include/scfgp_hip.h: scfgp_predict_cov):
        (Ta, Tb) float64, cov[i][j] = kappa <Li phi(a_i), Li phi(b_j)>, in the units of the scaled target.  Xb=None is the symmetric
        form (Ta, Ta), symmetric bit for bit; noise=True (symmetric form only) adds kappa to its diagonal.  mode 'scaled': inputs as
        predict takes them; 'raw': unscaled inputs through the registered X scaler, as predict_raw."""
        m, cols = self._mode('predict_cov', self.PREDICT_COV_MODES, mode)
        Xa = self._rows(Xa, 'Xa', cols)
        Xb = None if Xb is None else self._rows(Xb, 'Xb', cols)
        Li = self._Li(Li)
        Ta, Tb = Xa.shape[0], (Xa.shape[0] if Xb is None else Xb.shape[0])
        if Xb is not None and Tb == 0:
            raise ValueError('predict_cov: Xb has no rows')           # an empty array has no pointer to tell it from Xb=None
        cov = np.empty((Ta, Tb) if _count(Tb, 1, 32768) else (0, 0))
        self._check(self.lib.scfgp_predict_cov(self.ctx, dptr(Xa), Ta, dptr(Xb), Tb, dptr(Li), m, int(bool(noise)), dptr(cov)),
                    'predict_cov')
        return cov

    # -- staged evaluation (row-sharded data parallelism) --------------------------------------
    def pass1(self):
        self._check(self.lib.scfgp_pass1(self.ctx), 'pass1')

    def factor(self):
        """False when the library asks for the stages again from pass1 (SCFGP_REDO: the ranks have just agreed on a lower
        precision level than some of them ran pass 1 at -- every rank gets the same answer); True otherwise."""
        rc = self.lib.scfgp_factor(self.ctx)
        self._early = None
        if rc == _lib.SCFGP_REDO:
            return False
        self._check(rc, 'factor')
        return True

    def fail_stage(self, stage, want_grad=True):
        """This rank cannot compute sweep `stage` (1..3) of the evaluation in progress: mark its exchange buffer failed and, with
        a communicator attached, run the sum -- so that the peers reach their finish() and raise PeerFailed there instead of
        waiting in a collective (include/scfgp_hip.h, "ranks decide together")."""
        self._check(self.lib.scfgp_fail_stage(self.ctx, int(stage), int(bool(want_grad))), 'fail_stage')

    def fetch_factors(self):
        """Fetch alpha / Li as soon as the factor stage is done (overlaps the sweeps already queued); finish() returns them."""
        alpha = self._fresh((self.K, 1)); Li = self._fresh((self.K, self.K))
        self._check(self.lib.scfgp_fetch_factors(self.ctx, dptr(alpha), dptr(Li)), 'fetch_factors')
        self._early = (alpha, Li)

    def pass2(self, want_grad=True):
        self._check(self.lib.scfgp_pass2(self.ctx, int(bool(want_grad))), 'pass2')

    def adjoint(self):
        self._check(self.lib.scfgp_adjoint(self.ctx), 'adjoint')

    def pass3(self):
        self._check(self.lib.scfgp_pass3(self.ctx), 'pass3')

    def finish(self, want_grad=True):
        """(cost, grad, alpha, Li) -- or None when the library asks for the stages to be run again at the precision level
        it has just raised (SCFGP_REDO, include/scfgp_hip.h: the condition estimate of this evaluation was too high
        for the level it ran at)."""
        early = getattr(self, '_early', None)
        cost, grad, alpha, Li = self._outputs(want_grad, factors=early is None)
        if early is not None:
            alpha, Li = early
            rc = self.lib.scfgp_finish(self.ctx, int(bool(want_grad)), dptr(cost), dptr(grad), None, None)
        else:
            rc = self.lib.scfgp_finish(self.ctx, int(bool(want_grad)), dptr(cost), dptr(grad), dptr(alpha), dptr(Li))
        self._early = None
        if rc == _lib.SCFGP_REDO:
            return None
        self._check(rc, 'finish')
        return cost.reshape(()), grad, alpha, Li

    def stream_fence(self, peer_stream, direction):
        """Order the library's stream against `peer_stream` (a raw hipStream_t handle, 0/None = legacy default
        stream): direction 0 = peer waits for the library (before a collective), 1 = the library waits for peer."""
        self._check(self.lib.scfgp_stream_fence(self.ctx, C.c_void_p(peer_stream) if peer_stream else None, int(direction)),
                    'stream_fence')

    def exchange_ptr(self, stage):
        """(device pointer, number of float64) of exchange buffer `stage` (1..3)."""
        p = C.c_void_p(); n = C.c_int64()
        self._check(self.lib.scfgp_exchange(self.ctx, int(stage), C.byref(p), C.byref(n)), 'exchange')
        return p.value, n.value

    def exchange(self, stage):
        """The exchange buffer as a torch CUDA tensor aliasing the library's device memory."""
        import torch
        ptr, n = self.exchange_ptr(stage)

        class _Alias(object):
            __cuda_array_interface__ = {'shape': (n,), 'typestr': '<f8', 'data': (ptr, False), 'version': 2}
        # name the engine's own GPU: a bare 'cuda' is torch's CURRENT device and as_tensor would silently copy
        return torch.as_tensor(_Alias(), device=torch.device('cuda', self.device))

    # -- the sums inside the library (RCCL) -----------------------------------------------------------
    def comm_unique_id(self):
        """128 bytes identifying a new communicator (rank 0 creates them and hands them to the other ranks)."""
        buf = C.create_string_buffer(128)
        rc = self.lib.scfgp_comm_unique_id(buf)
        if rc != 0:
            raise RuntimeError('scfgp_comm_unique_id failed (%d): is librccl.so loadable?' % rc)
        return buf.raw

    def comm_init(self, nranks, rank, unique_id):
        """Join the communicator (collective over the ranks): from now on pass1 / pass2 / pass3 -- and with them eval() and
        eval_rows() -- end in their ncclAllReduce on the library's stream; no ShardedEvaluator, no fences."""
        if len(unique_id) != 128:
            raise ValueError('the unique id is 128 bytes')
        self._check(self.lib.scfgp_comm_init(self.ctx, int(nranks), int(rank), C.c_char_p(bytes(unique_id))), 'comm_init')

    def comm_destroy(self):
        self._check(self.lib.scfgp_comm_destroy(self.ctx), 'comm_destroy')

    # -- on-device optimiser ------------------------------------------------------------------------
    ALGOS = {'sgd': 0, 'adagrad': 1, 'rmsprop': 2, 'adadelta': 3, 'adam': 4, 'adamax': 5}

    def opt_init(self, algo, learning_rate=0.01, beta1=0.9, beta2=0.999, epsilon=1e-8, momentum=0.9):
        """Device-side update rule (beta1 doubles as rho for rmsprop/adadelta); momentum<0: no Nesterov."""
        h = np.array([learning_rate, beta1, beta2, epsilon], dtype=np.float64)
        self._check(self.lib.scfgp_opt_init(self.ctx, self.ALGOS[algo], dptr(h), 4, float(momentum)), 'opt_init')

    def opt_state(self, which, value=None):
        buf = np.empty(1 if which == 3 else self.P) if value is None else np.ascontiguousarray(value, dtype=np.float64).ravel()
        self._check(self.lib.scfgp_opt_state(self.ctx, 0 if value is None else 1, int(which), dptr(buf)), 'opt_state')
        return buf

    def opt_step(self, grad):
        """One step of the device rule with the given gradient (no evaluation); returns the updated parameter vector."""
        g = np.ascontiguousarray(grad, dtype=np.float64).ravel()
        self._check(self.lib.scfgp_opt_step(self.ctx, dptr(g), g.size), 'opt_step')
        return self.get_params()

    def train(self, n_iters, want_factors=True):
        """n_iters x (NLML+grad evaluation + update) on the resident rows without host round trips.
        Returns (cost history (n,), alpha, Li of the last evaluation)."""
        hist = np.empty(int(n_iters))
        alpha = np.empty((self.K, 1)) if want_factors else None
        Li = np.empty((self.K, self.K)) if want_factors else None
        self._check(self.lib.scfgp_train(self.ctx, int(n_iters), dptr(hist), dptr(alpha), dptr(Li)), 'train')
        return hist, alpha, Li

    # -- introspection ----------------------------------------------------------------------------
    def dims(self):
        out = (C.c_int64 * 7)()
        self._check(self.lib.scfgp_get_dims(self.ctx, out, 7), 'get_dims')
        return dict(zip(('K', 'Kp', 'Jp', 'Dp', 'Np', 'P', 'tile'), [int(v) for v in out]))

    CONDITION = ('cond_est', 'level', 'gram_fp64', 'alpha_err_fp32', 'threshold', 'threshold_w', 'Lmin2', 'Lmax2', 'Bmax')

    CONDITION_MODES = {'scaled': 0, 'raw': 1}

    def condition(self, Xn=None, yn=None, alpha=None, Li=None, mode='scaled'):
        """Two things under one name.  Without arguments: the condition estimate of A and the precision level of the last finished
        evaluation (scfgp_get_condition), a dict.  With rows: absorb the observations (Xn, yn) into the fitted posterior (alpha, Li)
        (include/scfgp_hip.h: scfgp_condition) and return (alpha' (K,1), Li' (K,K)), the factors of the fit on the old rows and the new
        ones together, at the context's current parameters.  mode 'scaled': Xn as predict takes it; 'raw': unscaled Xn through the
        registered X scaler, as predict_raw.  yn (n,) or (n,1) is the SCALED target in either mode."""
        if Xn is not None or yn is not None or alpha is not None or Li is not None:
            return self._condition(Xn, yn, alpha, Li, mode)
        out = np.zeros(len(self.CONDITION))
        self._check(self.lib.scfgp_get_condition(self.ctx, dptr(out), out.size), 'get_condition')
        return dict(zip(self.CONDITION, out.tolist()))

    def _condition(self, Xn, yn, alpha, Li, mode):
        m, cols = self._mode('condition', self.CONDITION_MODES, mode)
        if Xn is None or yn is None or alpha is None or Li is None:
            raise ValueError('condition: Xn, yn, alpha and Li are all needed')
        Xn = self._rows(Xn, 'Xn', cols)
        yn = self._weights(yn, Xn.shape[0], 'yn')
        alpha, Li = self._factors(alpha, Li)
        alpha_out = np.empty((self.K, 1)); Li_out = np.empty((self.K, self.K))
        rc = self.lib.scfgp_condition(self.ctx, dptr(Xn), dptr(yn), Xn.shape[0], dptr(alpha), dptr(Li), m, dptr(alpha_out), dptr(Li_out))
        self._check_undelivered(rc, 'condition')
        return alpha_out, Li_out

    def condition_grad(self, X, G, alpha, Li, dims=None, rho=None, y=None, raw=False):
        """Absorb observed partial derivatives into the fitted posterior (alpha, Li) (include/scfgp_hip.h: scfgp_condition_grad) and
        return (alpha' (K,1), Li' (K,K)).  G (n, nd): G[t, j] = d f / d x_dims[j] at row t of X, in SCALED target units; dims: the
        observed inputs (distinct, any order; None: all of them, in order); rho (n, nd) >= 0: every observation's precision relative to
        the value noise (None: 1; 0: not observed); y (n,) or (n,1): the SCALED values observed at the same points (None: none).
        raw=False: X as predict takes it, derivatives in the scaled inputs.  raw=True: unscaled X through the registered X scaler,
        derivatives in the RAW inputs, dims naming raw columns and -- dims=None -- G, rho with one column per raw column; what refers
        to a constant column that the scaler dropped is ignored, since the model does not depend on it."""
        cols = self._raw_cols('condition_grad', raw)
        if X is None or G is None or alpha is None or Li is None:
            raise ValueError('condition_grad: X, G, alpha and Li are all needed')
        D_in = np.shape(X)[1] if np.ndim(X) == 2 else self.D
        X = self._rows(X, 'X', cols)
        n = X.shape[0]
        G = np.asarray(G, dtype=np.float64)
        rho = None if rho is None else np.asarray(rho, dtype=np.float64)
        if dims is None:
            dims = np.arange(D_in)
        dims = np.asarray(dims, dtype=np.int64).reshape(-1)
        if G.ndim != 2 or G.shape != (n, dims.size) or (rho is not None and rho.shape != G.shape):
            raise ValueError('condition_grad: G (and rho) must be (%d, %d): one column per observed input' % (n, dims.size))
        if cols is not None:
            if dims.size and (dims.min() < 0 or dims.max() >= D_in):
                raise ValueError('condition_grad: dims names a column that does not exist')
            where = {int(cc): i for i, cc in enumerate(cols)}
            keep = [j for j, d in enumerate(dims) if int(d) in where]
            dims = np.array([where[int(dims[j])] for j in keep], dtype=np.int64)
            G = G[:, keep]
            rho = None if rho is None else rho[:, keep]
        if dims.size == 0:
            raise ValueError('condition_grad: no observed input is left')
        G = np.ascontiguousarray(G)
        rho = None if rho is None else np.ascontiguousarray(rho)
        y = self._weights(y, n, 'y')
        alpha, Li = self._factors(alpha, Li)
        nd = int(dims.size)
        dims32 = None if nd == self.D and np.array_equal(dims, np.arange(nd)) else np.ascontiguousarray(dims, dtype=np.int32)
        alpha_out = np.empty((self.K, 1)); Li_out = np.empty((self.K, self.K))
        rc = self.lib.scfgp_condition_grad(self.ctx, dptr(X), n, None if dims32 is None else dims32.ctypes.data_as(C.POINTER(C.c_int32)), nd,
                                           dptr(G), dptr(rho), dptr(y), dptr(alpha), dptr(Li), 1 if raw else 0, dptr(alpha_out), dptr(Li_out))
        self._check_undelivered(rc, 'condition_grad')
        return alpha_out, Li_out

    def condition_grad_points_per_chunk(self, nd, values):
        """Points per chunk of condition_grad (the formula of include/scfgp_hip.h): whole blocks of nb = nd + (1 with values) rows"""
        return 32768 // (int(nd) + (1 if values else 0))

    SOBOL_OUTPUTS = ('f0', 'V', 'Vmain', 'Vtot', 'phibar')

    def sobol(self, kind, p0, p1, W=None, want=('f0', 'V', 'Vmain', 'Vtot')):
        """Closed-form Sobol variances of the sample functions W under a product measure over the SCALED inputs (include/scfgp_hip.h:
        scfgp_sobol).  kind (D,) ints: 0 = uniform on [p0, p1], 1 = normal(p0, p1^2) (None: all uniform); W (K, nw) as sample_weights
        returns it, or (K,) / (K, 1) such as alpha for the posterior mean.  Returns a dict of the outputs named in want: 'f0' (nw,)
        the mean of f, 'V' (nw,) its variance, 'Vmain', 'Vtot' (nw, D) the main-effect and total-effect variances, 'phibar' (K,) the
        mean feature vector.  The Sobol indices are Vmain / V and Vtot / V; V may be 0."""
        want = tuple(want)
        bad = [k for k in want if k not in self.SOBOL_OUTPUTS]
        if bad:
            raise ValueError('sobol: unknown output %r (one of %s)' % (bad[0], ', '.join(self.SOBOL_OUTPUTS)))
        p0 = np.ascontiguousarray(p0, dtype=np.float64).reshape(-1)
        p1 = np.ascontiguousarray(p1, dtype=np.float64).reshape(-1)
        if p0.size != self.D or p1.size != self.D:
            raise ValueError('sobol: p0 and p1 must have D=%d entries' % self.D)
        k32 = None
        if kind is not None:
            k32 = np.ascontiguousarray(kind, dtype=np.int32).reshape(-1)
            if k32.size != self.D:
                raise ValueError('sobol: kind must have D=%d entries' % self.D)
        nw = 0
        if W is not None:
            W = np.asarray(W, dtype=np.float64)
            W = np.ascontiguousarray(W.reshape(-1, 1) if W.ndim == 1 else W)
            if W.ndim != 2 or W.shape[0] != self.K:
                raise ValueError('sobol: W must be (K, nw) with K=%d' % self.K)
            nw = W.shape[1]
        shapes = {'f0': (nw,), 'V': (nw,), 'Vmain': (nw, self.D), 'Vtot': (nw, self.D), 'phibar': (self.K,)}
        out = {k: np.empty(shapes[k]) for k in want}
        rc = self.lib.scfgp_sobol(self.ctx, None if k32 is None else k32.ctypes.data_as(C.POINTER(C.c_int32)), dptr(p0), dptr(p1), dptr(W), nw,
                                  *[dptr(out.get(k)) for k in self.SOBOL_OUTPUTS])
        self._check_undelivered(rc, 'sobol')
        return out

    FORGET_STATS = ('n', 'sum_e2', 'sum_abs_e', 'sum_log_marginal', 'log_joint', 'min_pivot2', 'blocks')

    def forget(self, X, y, alpha, Li, factors=True, predict=False, mode='scaled'):
        """Remove the observations (X, y), rows that ARE in the fit (alpha, Li), from the posterior (include/scfgp_hip.h: scfgp_forget).
        factors: return (alpha' (K,1), Li' (K,K)), the factors of the fit on the remaining rows.  predict: return (mu (n,1), std (n,),
        stats dict), the held-out predictions of the removed rows under that fit -- bit for bit predict(X, alpha', Li') -- and
        FORGET_STATS with e = y - mu; with factors=False Li' never leaves the device.  Both: (alpha', Li', mu, std, stats).  mode
        'scaled': X as predict takes it; 'raw': unscaled X through the registered X scaler.  y (n,) or (n,1) is the SCALED target."""
        m, cols = self._mode('forget', self.CONDITION_MODES, mode)
        if X is None or y is None or alpha is None or Li is None:
            raise ValueError('forget: X, y, alpha and Li are all needed')
        if not factors and not predict:
            raise ValueError('forget: nothing asked for (factors and predict are both False)')
        X = self._rows(X, 'X', cols)
        n = X.shape[0]
        y = self._weights(y, n, 'y')
        alpha, Li = self._factors(alpha, Li)
        alpha_out = np.empty((self.K, 1)) if factors else None
        Li_out = np.empty((self.K, self.K)) if factors else None
        mu = np.empty((n, 1)) if predict else None
        sd = np.empty(n) if predict else None
        stats = np.zeros(8) if predict else None
        rc = self.lib.scfgp_forget(self.ctx, dptr(X), dptr(y), n, dptr(alpha), dptr(Li), m, dptr(alpha_out), dptr(Li_out), dptr(mu), dptr(sd),
                                   dptr(stats))
        self._check_undelivered(rc, 'forget')
        out = (alpha_out, Li_out) if factors else ()
        if predict:
            st = dict(zip(self.FORGET_STATS, stats.tolist()))
            st['n'] = int(st['n']); st['blocks'] = int(st['blocks'])
            out = out + (mu, sd, st)
        return out

    LOO_STATS = ('n', 'sum_e2', 'sum_abs_e', 'sum_log_marginal', 'sum_log_joint', 'max_leverage', 'blocks')

    def loo(self, X=None, y=None, alpha=None, Li=None, block=1, mode='scaled'):
        """Exact leave-block-out predictions of rows that are IN the fit (alpha, Li), without a refit (include/scfgp_hip.h: scfgp_loo):
        (mu (n,1), std (n,), lev (n,), stats dict).  Row i's mu / std are what predict would return for it from the fit on all rows but
        the `block` consecutive rows of its block ([j block, (j+1) block); block 1: leave-one-out); lev is the leverage h_i.  X=None and
        y=None: the rows made resident by set_data.  mode 'scaled': X as predict takes it; 'raw': unscaled X through the registered X
        scaler.  y (n,) or (n,1) is the SCALED target in either mode.  stats: LOO_STATS, sums over the call's rows with e = y - mu."""
        m, cols = self._mode('loo', self.CONDITION_MODES, mode, rows=X is not None)
        if alpha is None or Li is None:
            raise ValueError('loo: alpha and Li are needed')
        if (X is None) != (y is None):
            raise ValueError('loo: X and y go together (both None: the resident rows)')
        alpha, Li = self._factors(alpha, Li)
        if X is None:
            d = (C.c_int64 * 8)()
            self._check(self.lib.scfgp_get_dims(self.ctx, d, 8), 'get_dims')
            n = int(d[7])                                   # the rows made resident by set_data (0: the library refuses)
        else:
            X = self._rows(X, 'X', cols)
            n = X.shape[0]
            y = self._weights(y, n, 'y')
        mu = np.empty((n, 1)); sd = np.empty(n); lev = np.empty(n); stats = np.zeros(8)
        rc = self.lib.scfgp_loo(self.ctx, dptr(X), dptr(y), n, dptr(alpha), dptr(Li), m, int(block), dptr(mu), dptr(sd), dptr(lev),
                                dptr(stats))
        self._check_undelivered(rc, 'loo')
        out = dict(zip(self.LOO_STATS, stats.tolist()))
        out['n'] = int(out['n']); out['blocks'] = int(out['blocks'])
        return mu, sd, lev, out

    def select(self, Xc, Li, m, w=None, raw=False, return_std=False):
        """Greedy maximum-information choice of m rows from the pool Xc (include/scfgp_hip.h: scfgp_select): (idx (m,) int64, var (m,),
        gain (m,)) and, with return_std, std_after (T,).  idx: the picks in order, indices into Xc; var[j]: the posterior variance of f
        at pick j when it was picked (scaled-y units, noise excluded); gain[j]: its information gain log1p(var / kappa) / 2;
        std_after: what predict reports as std at every pool row once the picks have been observed (condition), whatever their
        targets.  w (T,): non-negative weights of the criterion, 0 excludes a row.  raw: unscaled Xc through the registered X scaler,
        as predict_raw.  Only Li is needed; condition on pending points first, with any targets."""
        Xc = self._rows(Xc, 'Xc', self._raw_cols('select', raw))
        T = Xc.shape[0]
        w = self._weights(w, T, 'w')
        Li = self._Li(Li)
        m = int(m)
        n = _count(m, 1, 4096)
        idx = np.empty(n, dtype=np.int64); var = np.empty(n); gain = np.empty(n)
        sd = np.empty(T) if return_std else None
        rc = self.lib.scfgp_select(self.ctx, dptr(Xc), T, dptr(w), dptr(Li), m, int(bool(raw)), _i64(idx), dptr(var), dptr(gain), dptr(sd))
        self._check_undelivered(rc, 'select')
        return (idx, var, gain, sd) if return_std else (idx, var, gain)

    def select_iv(self, Xc, Li, m, Xr=None, w=None, wr=None, raw=False, return_std=False):
        """Greedy choice of m rows from the pool Xc by integrated variance reduction (include/scfgp_hip.h: scfgp_select_iv): (idx (m,)
        int64, red (m,), var (m,), ivar (2,)) and, with return_std, std_after (T,).  Pick j is the row whose observation most reduces
        sum_r wr_r Var[f(Xr_r)] given the picks before it; red[j] is that reduction, var[j] the posterior variance of f at the pick
        when it was picked, ivar = (integrated variance before the picks, after them), all in scaled-y units, noise excluded.  Xr
        None: the pool is its own reference (wr then has T entries).  w (T,): non-negative weights of the criterion, 0 excludes a row;
        wr: non-negative weights of the reference rows.  raw: unscaled Xc and Xr through the registered X scaler."""
        cols = self._raw_cols('select_iv', raw)
        Xc = self._rows(Xc, 'Xc', cols)
        T = Xc.shape[0]
        Xr = None if Xr is None else self._rows(Xr, 'Xr', cols)
        R = T if Xr is None else Xr.shape[0]
        w = self._weights(w, T, 'w'); wr = self._weights(wr, R, 'wr')
        Li = self._Li(Li)
        m = int(m)
        n = _count(m, 1, 4096)
        idx = np.empty(n, dtype=np.int64); red = np.empty(n); var = np.empty(n); ivar = np.empty(2)
        sd = np.empty(T) if return_std else None
        rc = self.lib.scfgp_select_iv(self.ctx, dptr(Xc), T, dptr(w), dptr(Xr), R, dptr(wr), dptr(Li), m, int(bool(raw)), _i64(idx),
                                      dptr(red), dptr(var), dptr(ivar), dptr(sd))
        self._check_undelivered(rc, 'select_iv')
        return (idx, red, var, ivar, sd) if return_std else (idx, red, var, ivar)

    def select_qei(self, Xc, alpha, Li, m, nsamp, best, xi=0.0, seed=0, w=None, pending=None, mode='scaled', minimize=False,
                   return_score0=False, return_state=False):
        """Greedy Monte-Carlo batch expected improvement over the pool Xc (include/scfgp_hip.h: scfgp_select_qei): (idx (m,) int64,
        gain (m,), qei (2,)), then score0 (T,) with return_score0 and mstate (nsamp,) with return_state.  The nsamp sample functions
        are `sample`'s (same seed, no noise); best and xi are in scaled y units, as in `acquire`.  Pick j is the eligible row that adds
        most to the mean over the samples of max(best of pending rows and picks so far - (best + xi), 0); gain[j] is what it adds.
        pending (np, D): rows chosen earlier and not yet observed, in the pool's mode; w (T,): row t is eligible iff w[t] > 0.  qei =
        (q-EI of the pending rows alone, q-EI of pending rows plus picks); score0: the one-point Monte-Carlo EI of every row given the
        pending rows; mstate: the per-sample running maximum after the last pick.  mode 'scaled' or 'raw'."""
        md, cols = self._mode('select_qei', self.ACQUIRE_MODES, mode)
        Xc = self._rows(Xc, 'Xc', cols)
        T = Xc.shape[0]
        Xp = None if pending is None or len(pending) == 0 else self._rows(pending, 'pending', cols)
        w = self._weights(w, T, 'w')
        alpha, Li = self._factors(alpha, Li)
        m, nsamp = int(m), int(nsamp)
        n = _count(m, 1, 4096)
        idx = np.empty(n, dtype=np.int64); gain = np.empty(n); qei = np.empty(2)
        score0 = np.empty(T) if return_score0 else None
        mstate = np.empty(_count(nsamp, 1, 1024)) if return_state else None
        rc = self.lib.scfgp_select_qei(self.ctx, dptr(Xc), T, dptr(w), dptr(Xp), 0 if Xp is None else Xp.shape[0], dptr(alpha), dptr(Li),
                                       nsamp, _seed(seed), float(best), float(xi), m, md, int(bool(minimize)), _i64(idx), dptr(gain),
                                       dptr(score0), dptr(mstate), dptr(qei))
        self._check_undelivered(rc, 'select_qei')
        out = (idx, gain, qei)
        if return_score0:
            out += (score0,)
        if return_state:
            out += (mstate,)
        return out

    def last_error(self):
        """Message of the last failure -- or refusal (a precision level whose buffers could not be had) -- on this context."""
        return self.lib.scfgp_last_error(self.ctx).decode()

    def set_profiling(self, on=True):
        self._check(self.lib.scfgp_set_profiling(self.ctx, int(bool(on))), 'set_profiling')

    def timings(self):
        """[(stage name, milliseconds)] of the last evaluation (profiling must be on)."""
        n = 64
        ms = (C.c_double * n)(); names = (C.c_char_p * n)()
        k = self.lib.scfgp_get_timings(self.ctx, ms, names, n)
        return [(names[i].decode(), ms[i]) for i in range(max(k, 0))]

    def set_option(self, name, value):
        self._check(self.lib.scfgp_set_option(self.ctx, name.encode(), int(value)), 'set_option')

    def debug_read(self, name, shape, dtype=np.float64):
        out = np.empty(shape, dtype=dtype)
        n = self.lib.scfgp_debug_read(self.ctx, name.encode(), out.ctypes.data_as(C.c_void_p), out.nbytes)
        if n < 0:
            self._check(int(n), 'debug_read')
        return out
