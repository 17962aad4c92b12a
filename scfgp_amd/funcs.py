"""
The "compiled function triple" -- drop-in for what theano.function produces in
SCFGP.build_theano_models (SCFGP/SCFGP.py:132-137,145-148):

    train_func(X, y)          -> [cost, alpha, Li]
    train_iter_func(X, y)     -> [cost, alpha, Li]  (at the PRE-update parameters) and then
                                 applies the update rule to the shared parameter vector
    pred_func(Xs, alpha, Li)  -> [mu (T,1), std (T,)]

As in the reference the hyper-parameters are implicit state (givens=[(params,
self.params)], SCFGP/SCFGP.py:134-137,147-148): the three callables share one `Shared`
vector plus the optimiser moments created when the triple is built, so a triple handed
to another model through optimize(funcs=...) keeps training ITS vector, exactly like a
reused Theano triple does.

All numerics happen in libscfgp_hip.so; this module only moves numpy buffers across the
C ABI.  X and y stay resident on the GPU between calls while the caller keeps passing
the same arrays (optimize() does: SCFGP/SCFGP.py:237).
"""
import numpy as np

from .engine import HipEngine
from .optimizer import Optimizer as OPT, Shared, apply_updates
from .sharded import ShardedEvaluator


class _GradSlot(object):
    def __init__(self, P):
        self._g = np.zeros(P)

    def get_value(self, borrow=False):
        return self._g

    def set_value(self, g):
        self._g = g


_pool = None
_warned_sampled = False


def _hash_piece(mv):
    try:
        import xxhash                     # declared in README.md ("Dependencies"); without it crc32 is used, several times slower
        return xxhash.xxh3_64_intdigest(mv)
    except ImportError:
        import zlib
        h = len(mv) // 2
        return (zlib.crc32(mv[:h]) << 32) | zlib.crc32(mv[h:])


def _hash64(buf):
    """64-bit hashes of a contiguous buffer (xxh3 when the module is there, else crc32 of the two halves); buffers
    above 4 MiB are hashed in pieces on a small thread pool (both hash functions release the GIL)."""
    global _pool
    mv = memoryview(buf).cast('B')
    if len(mv) <= (4 << 20):
        return _hash_piece(mv)
    if _pool is None:
        import os
        from concurrent.futures import ThreadPoolExecutor
        _pool = ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 4))
    n = len(mv); pieces = 32 if n > (64 << 20) else 8; step = -(-n // pieces)
    return tuple(_pool.map(_hash_piece, [mv[i:i + step] for i in range(0, n, step)]))


def _content_key(a, trusted):
    """What identifies the CONTENTS of an array for the residency check.
    Default, at EVERY size: a 64-bit hash of every byte (threaded xxh3: 2.6 ms for config C2, tens of ms for the 512 MB of
    the headline X against its 220 ms evaluation) -- any in-place edit is seen; the reference re-reads its arguments on
    every call too (SCFGP/SCFGP.py:237).
    `trusted` (the caller maintains a version token with set_data_version): contents cannot change unnoticed, so 4096
    evenly spaced 512-byte blocks identify the array."""
    flat = a.reshape(-1)
    if not trusted or flat.size <= (1 << 16):
        return ('full', _hash64(np.ascontiguousarray(flat)))
    nblk, blk = 4096, 64
    starts = np.linspace(0, flat.size - blk, nblk).astype(np.int64)
    sample = np.concatenate([flat[s:s + blk] for s in starts])
    return ('sampled', _hash64(sample))


def _fingerprint(X, y, version=None):
    """Identity of a data set for the residency check: shapes, the caller's version token and the content keys of both
    arrays (see _content_key).  Addresses are NOT part of it: a freed array's address is handed out again."""
    trusted = version is not None
    return (X.shape, y.shape, version, _content_key(X, trusted), _content_key(y, trusted))


def _nobody_can_write(a):
    """True when no ndarray through which `a`'s memory could be edited exists on its ownership chain: `a` and every array
    in its .base chain are read-only, and the chain ends in memory numpy allocated itself (or an immutable bytes object).
    A read-only VIEW of a writeable array is not frozen -- the base still writes through."""
    while isinstance(a, np.ndarray):
        if a.flags.writeable:
            return False
        a = a.base
    return a is None or isinstance(a, bytes)


class CompiledFuncs(object):
    """Owns one HipEngine (one GPU) and the shared parameter/optimiser state."""

    def __init__(self, D, S, M, params, algo='adam', algo_params=None, momentum=0.9,
                 dtype='f64', device=0, stream=None, allreduce=None, n_global=None, device_optimizer=False):
        self.engine = HipEngine(D, S, M, dtype=dtype, device=device, stream=stream)
        # Theano's functions return a NaN / Inf cost as a value and SCFGP.optimize reads it as "no improvement"
        # (SCFGP/SCFGP.py:249-258); only a failed Cholesky raises (LinAlgError)
        self.engine.nonfinite = 'return'
        self.evaluator = ShardedEvaluator(self.engine, allreduce)
        self.allreduce = allreduce
        self.n_global = n_global
        self.params = params if isinstance(params, Shared) else Shared(params)
        self.grads = _GradSlot(self.engine.P)
        if algo not in OPT.algos or algo.startswith('apply_'):
            raise ValueError("unknown update rule %r (choose from %s)" % (algo, OPT.algos[2:]))
        algo_params = {} if algo_params is None else algo_params
        self.algo, self.algo_params, self.momentum, self.dtype = algo, dict(algo_params), momentum, dtype
        updates = getattr(OPT, algo)(self.params, self.grads, **algo_params)          # SCFGP.py:130
        self.updates = OPT.apply_nesterov_momentum(updates, momentum=momentum)        # SCFGP.py:131
        self._uploaded_version = None
        self._resident = None
        # device_optimizer: the same rule runs as a device kernel behind the evaluation and whole
        # iterations are replayed as one hipGraph (single GPU); the host update dictionary above is
        # then bypassed, so a user-supplied callback cannot be used in this mode.
        self.device_optimizer = bool(device_optimizer)
        if self.device_optimizer:
            if allreduce is not None:
                raise ValueError('device_optimizer needs the whole evaluation on one GPU')
            import inspect
            sig = inspect.signature(getattr(OPT, algo)).parameters
            kw = {k: v.default for k, v in sig.items() if v.default is not inspect._empty}
            kw.update(algo_params)
            self.engine.opt_init(algo, learning_rate=kw.get('learning_rate', 0.01),
                                 beta1=kw.get('beta1', kw.get('rho', 0.9)), beta2=kw.get('beta2', 0.999),
                                 epsilon=kw.get('epsilon', 1e-8), momentum=momentum)

    # -- state sync ----------------------------------------------------------------------
    def _sync_params(self):
        if self._uploaded_version != self.params.version:
            self.engine.set_params(self.params.get_value(borrow=True))
            self._uploaded_version = self.params.version

    def set_data_version(self, version):
        """Caller-supplied token for very large arrays: change it whenever X or y were edited in place."""
        self.data_version = version

    def _sync_data(self, X, y):
        """Upload X, y unless the resident copy is provably current.
          * the SAME array objects as last time, both frozen (_nobody_can_write): nothing is hashed -- their contents cannot have
            changed, and holding a reference to them means their memory cannot have been handed to another array either.  This is
            the steady state of SCFGP.optimize, whose model freezes the arrays it creates in set_data (SCFGP/SCFGP.py:161-162,237);
          * anything else -- writeable arrays, read-only views of writeable arrays, new objects: every byte of both arrays is
            hashed on every call (sampled only under a caller-maintained version token)."""
        version = getattr(self, 'data_version', None)
        held = getattr(self, '_resident_frozen', None)
        if (held is not None and self._resident is not None and held[0] is X and held[1] is y and held[2] == version
                and _nobody_can_write(X) and _nobody_can_write(y)):
            return
        fp = _fingerprint(X, y, version)
        # strong references, kept only for frozen arrays (a writeable array is re-hashed anyway)
        self._resident_frozen = (X, y, version) if _nobody_can_write(X) and _nobody_can_write(y) else None
        if fp != self._resident:
            n_global = self.n_global
            if self.allreduce is not None and n_global is None:
                n = np.array([float(X.shape[0])])
                self.allreduce(n)
                n_global = int(n[0])
            self.engine.set_data(X, y, n_global)
            self._resident = fp

    def _sync_scalers(self, x_scaler, y_scaler):
        """Register the scalers on the device when their CONTENTS changed: SCFGP.set_data refits the same Scaler
        objects in place (SCFGP/SCFGP.py:155-156), so object identity cannot be the key."""
        if x_scaler is not None:
            key = self.engine.scaler_key(x_scaler)
            if key != getattr(self, '_xscaler_key', None):
                self.engine.set_x_scaler(x_scaler)
                self._xscaler_key = key
        if y_scaler is not None:
            key = self.engine.scaler_key(y_scaler)
            if key != getattr(self, '_yscaler_key', None):
                self.engine.set_y_scaler(y_scaler)
                self._yscaler_key = key

    # -- optimiser state (checkpoints) ---------------------------------------------------------
    def get_opt_state(self):
        """Everything train_iter_func mutates besides the parameter vector, as a list of float64 arrays: the rule's
        state variables in update-dictionary order (adam: m, v, t -- SCFGP/Optimizer.py:314-323) and the Nesterov
        velocity (:92-93); in device_optimizer mode the device's [s1, s2, velocity, t]."""
        if self.device_optimizer:
            return [self.engine.opt_state(w).copy() for w in range(4)]
        return [np.atleast_1d(var.get_value()) for var in self.updates if var is not self.params]

    def set_opt_state(self, arrays):
        arrays = [np.asarray(a, dtype=np.float64) for a in arrays]
        if self.device_optimizer:
            if len(arrays) != 4:
                raise ValueError('device optimiser state has 4 arrays, got %d' % len(arrays))
            for w, a in enumerate(arrays):
                self.engine.opt_state(w, a)
            return
        slots = [var for var in self.updates if var is not self.params]
        if len(slots) != len(arrays):
            raise ValueError('update rule %r has %d state variables, checkpoint has %d' % (self.algo, len(slots), len(arrays)))
        for var, a in zip(slots, arrays):
            cur = var.get_value(borrow=True)
            var.set_value(a.reshape(np.shape(cur)))

    def invalidate(self):
        """Forget the resident data set: the next call uploads its X, y again."""
        self._resident = None
        self._resident_frozen = None

    def _evaluate(self, X, y, want_grad):
        self._sync_params()
        self._sync_data(X, y)
        return self.evaluator.eval(want_grad)

    # -- the triple ------------------------------------------------------------------------
    def train_func(self, X, y):
        cost, _, alpha, Li = self._evaluate(X, y, False)
        return [cost, alpha, Li]

    def train_iters(self, X, y, n):
        """n training iterations on the device (device_optimizer mode): cost history, alpha, Li of
        the last evaluation; the shared vector is refreshed from the device afterwards."""
        if not self.device_optimizer:
            raise RuntimeError('train_iters needs device_optimizer=True')
        self._sync_params()
        self._sync_data(X, y)
        hist, alpha, Li = self.engine.train(n)
        self.params.set_value(self.engine.get_params())
        self._uploaded_version = self.params.version           # device already holds this vector
        return hist, alpha, Li

    def train_iter_func(self, X, y):
        if self.device_optimizer:
            hist, alpha, Li = self.train_iters(X, y, 1)
            return [np.array(hist[0]), alpha, Li]
        cost, grad, alpha, Li = self._evaluate(X, y, True)
        self.grads.set_value(grad)
        apply_updates(self.updates)
        return [cost, alpha, Li]

    def train_iter_rows(self, X, y, idx):
        """train_iter_func on rows `idx` of (X, y) without re-uploading them: X, y become (or stay) the
        resident data set and the batch is gathered on the device (single GPU, host update rule)."""
        if self.allreduce is not None or self.device_optimizer:
            return self.train_iter_func(np.ascontiguousarray(X[idx]), np.ascontiguousarray(y[idx]))
        self._sync_params()
        self._sync_data(X, y)
        cost, grad, alpha, Li = self.engine.eval_rows(idx, True)
        self.grads.set_value(grad)
        apply_updates(self.updates)
        return [cost, alpha, Li]

    def pred_func(self, Xs, alpha, Li):
        self._sync_params()
        mu, sd = self.engine.predict(Xs, alpha, Li)
        return [mu, sd]

    def pred_raw(self, Xs_raw, x_scaler, alpha, Li):
        """pred_func on unscaled inputs: the X scaler's element-wise transform runs on the GPU."""
        self._sync_params()
        self._sync_scalers(x_scaler, None)
        return self.engine.predict_raw(Xs_raw, alpha, Li)

    def pred_y(self, Xs_raw, x_scaler, y_scaler, alpha, Li, ys=None):
        """All of SCFGP.predict on the GPU: mu_y, std_y (T,1) and the metric dict (None without targets)."""
        self._sync_params()
        self._sync_scalers(x_scaler, y_scaler)
        return self.engine.predict_y(Xs_raw, alpha, Li, ys)

    def pred_grad_func(self, Xs, alpha, Li):
        """pred_func and its input gradients: [mu (T,1), std (T,), dmu (T,D), dstd (T,D)] for scaled Xs."""
        self._sync_params()
        return list(self.engine.predict_grad(Xs, alpha, Li))

    def pred_grad_y(self, Xs_raw, x_scaler, y_scaler, alpha, Li):
        """pred_y's mu_y, std_y and their gradients in the raw inputs: [mu_y (T,1), std_y (T,), dmu_y (T,D_raw), dstd_y (T,D_raw)]."""
        self._sync_params()
        self._sync_scalers(x_scaler, y_scaler)
        return list(self.engine.predict_grad(Xs_raw, alpha, Li, mode='y'))

    def sample_y(self, Xs_raw, x_scaler, y_scaler, alpha, Li, nsamp, seed=0, noise=False):
        """nsamp posterior sample functions at the raw rows Xs_raw, in raw y units (T, nsamp)."""
        self._sync_params()
        self._sync_scalers(x_scaler, y_scaler)
        return self.engine.sample(Xs_raw, alpha, Li, nsamp, seed=seed, mode='y', noise=noise)

    def sample_argmax_y(self, Xs_raw, x_scaler, y_scaler, alpha, Li, nsamp, seed=0, weights=None, minimize=False):
        """Per-sample maximisers (idx, val) of sample_y's functions over the raw pool rows Xs_raw, val in raw y units
        (engine.sample_argmax)."""
        self._sync_params()
        self._sync_scalers(x_scaler, y_scaler)
        return self.engine.sample_argmax(Xs_raw, alpha, Li, nsamp, seed=seed, w=weights, mode='y', minimize=minimize)

    def acquire_raw(self, Xs_raw, x_scaler, alpha, Li, kind, **kw):
        """Acquisition functions over the raw pool rows Xs_raw, in scaled y units (engine.acquire with mode 'raw'; kw: its best, xi,
        beta, fstar, w, noise, minimize, want)."""
        self._sync_params()
        self._sync_scalers(x_scaler, None)
        return self.engine.acquire(Xs_raw, alpha, Li, kind, mode='raw', **kw)

    def acquire_kg_raw(self, Xc_raw, x_scaler, alpha, Li, Xr_raw=None, **kw):
        """Knowledge gradient of the raw candidate rows Xc_raw over the raw reference rows Xr_raw, in scaled y units (engine.acquire_kg
        with mode 'raw'; kw: its z, w, noise, minimize, want)."""
        self._sync_params()
        self._sync_scalers(x_scaler, None)
        return self.engine.acquire_kg(Xc_raw, alpha, Li, Xr=Xr_raw, mode='raw', **kw)

    def sample_argmax_raw(self, Xs_raw, x_scaler, alpha, Li, nsamp, seed=0, weights=None, minimize=False):
        """Per-sample maximisers (idx, val) over the raw pool rows Xs_raw with val in SCALED y units: the f* of acquire_raw's 'mes'."""
        self._sync_params()
        self._sync_scalers(x_scaler, None)
        return self.engine.sample_argmax(Xs_raw, alpha, Li, nsamp, seed=seed, w=weights, mode='raw', minimize=minimize)

    def sample_weights(self, alpha, Li, nsamp, seed=0):
        """W (K, nsamp): the weights of sample_y's functions at the shared parameter vector (engine.sample_weights)."""
        self._sync_params()
        return self.engine.sample_weights(alpha, Li, nsamp, seed=seed)

    def sample_grad_raw(self, Xs_raw, x_scaler, y_scaler, W, sidx=None, y_units=False, want_val=True):
        """Values and gradients (val (T,), grad (T, D_raw)) of the sample functions with weights W at the raw rows Xs_raw, row t under
        function sidx[t]: in scaled y units, or with y_units in raw y units through the y scaler (engine.sample_grad)."""
        self._sync_params()
        self._sync_scalers(x_scaler, y_scaler if y_units else None)
        return self.engine.sample_grad(Xs_raw, W, sidx=sidx, mode='y' if y_units else 'raw', want_val=want_val)

    def pred_gradcov_raw(self, Xs_raw, x_scaler, alpha, Li, w=None, want=('dmu', 'dvar', 'asub')):
        """Posterior mean, variance / covariance of the input gradient at the raw rows Xs_raw and their active-subspace matrix, in raw
        X units and scaled y units (engine.predict_gradcov with mode 'raw'): a dict of the outputs named in `want`."""
        self._sync_params()
        self._sync_scalers(x_scaler, None)
        return self.engine.predict_gradcov(Xs_raw, alpha, Li, w=w, mode='raw', want=want)

    def pred_pd_raw(self, Xs_raw, x_scaler, alpha, Li, dims, grid, w=None, want=('pd', 'sd')):
        """Partial-dependence and ICE curves of the raw columns `dims` over the raw pool rows Xs_raw, the grid (ndim, G) in raw units of
        its columns, the curves in scaled y units (engine.predict_pd with mode 'raw'): a dict of the outputs named in `want`."""
        self._sync_params()
        self._sync_scalers(x_scaler, None)
        return self.engine.predict_pd(Xs_raw, alpha, Li, dims, grid, w=w, mode='raw', want=want)

    def sobol_raw(self, kind, p0, p1, x_scaler, W=None, want=('f0', 'V', 'Vmain', 'Vtot'), scaled=False):
        """Closed-form Sobol variances (engine.sobol) of the sample functions W under a product measure stated per RAW column: kind
        (D_raw,) 0 = uniform on [p0, p1], 1 = normal(p0, p1^2) (None: all uniform), in raw X units.  An affine X scaler ('min-max',
        'normal') maps such an input to one of the same kind -- bounds and mean through the transform, the standard deviation through its
        slope -- on the columns it kept; any other scaler does not, and the call raises a ValueError unless scaled=True states that the
        measure is already in scaled units.  What refers to a constant column that the scaler dropped is ignored.  Vmain and Vtot come
        back (nw, D_raw) with zeros at the dropped columns, as predict_grad's gradients do."""
        from .engine import _scatter
        self._sync_params()
        cols = [int(cc) for cc in x_scaler.data['cols']]
        p0 = np.asarray(p0, dtype=np.float64).reshape(-1); p1 = np.asarray(p1, dtype=np.float64).reshape(-1)
        D_raw = p0.size
        kind = np.zeros(D_raw, dtype=np.int32) if kind is None else np.asarray(kind, dtype=np.int32).reshape(-1)
        if p1.size != D_raw or kind.size != D_raw or (cols and max(cols) >= D_raw):
            raise ValueError('sobol: kind, p0 and p1 need one entry per raw column')
        k, q0, q1 = kind[cols], p0[cols], p1[cols]
        if not scaled:
            if not x_scaler.affine:
                raise ValueError("sobol: the X scaler %r is not affine, so a uniform or normal raw input is neither after it: state the "
                                 "measure in scaled units (scaled=True)" % x_scaler.algo)
            z = np.zeros((1, D_raw))
            off = np.asarray(x_scaler.forward_transform(z), dtype=np.float64)[0]             # x~ = off + slope x, slope > 0
            slope = np.asarray(x_scaler.forward_derivative(z), dtype=np.float64)[0]
            q0 = off + slope * q0
            q1 = np.where(k == 1, slope * q1, off + slope * q1)
        out = self.engine.sobol(k, q0, q1, W, want=want)
        for key in ('Vmain', 'Vtot'):
            if key in out:
                out[key] = _scatter(out[key], cols, D_raw)
        return out

    def pred_cov_raw(self, Xa_raw, x_scaler, Li, Xb_raw=None, noise=False):
        """Joint posterior covariance of the scaled target between the raw rows Xa_raw and Xb_raw (None: among Xa_raw): (Ta, Tb)."""
        self._sync_params()
        self._sync_scalers(x_scaler, None)
        return self.engine.predict_cov(Xa_raw, Li, Xb=Xb_raw, mode='raw', noise=noise)

    def condition_raw(self, X_raw, y_scaled, x_scaler, alpha, Li):
        """The factors (alpha', Li') of the posterior (alpha, Li) after the observations (X_raw, y_scaled) are absorbed into it, at the
        shared parameter vector: raw rows through the X scaler on the device, targets already scaled (engine.condition)."""
        self._sync_params()
        self._sync_scalers(x_scaler, None)
        return self.engine.condition(X_raw, y_scaled, alpha, Li, mode='raw')

    def condition_grad_raw(self, X_raw, G, x_scaler, alpha, Li, dims=None, rho=None, y_scaled=None):
        """The factors (alpha', Li') of the posterior (alpha, Li) after the derivative observations G (scaled target per RAW input; dims,
        rho as engine.condition_grad takes them with raw=True) and, given y_scaled, the values at the same rows are absorbed into it, at
        the shared parameter vector: raw rows through the X scaler on the device."""
        self._sync_params()
        self._sync_scalers(x_scaler, None)
        return self.engine.condition_grad(X_raw, G, alpha, Li, dims=dims, rho=rho, y=y_scaled, raw=True)

    def forget_raw(self, X_raw, y_scaled, x_scaler, alpha, Li, factors=True, predict=False):
        """engine.forget of the rows (X_raw, y_scaled), which must be rows of the fit (alpha, Li), at the shared parameter vector: raw
        rows through the X scaler on the device, targets already scaled."""
        self._sync_params()
        self._sync_scalers(x_scaler, None)
        return self.engine.forget(X_raw, y_scaled, alpha, Li, factors=factors, predict=predict, mode='raw')

    def forget_func(self, X, y, alpha, Li, factors=True, predict=False):
        """forget_raw for SCALED rows (X, y), as train_func takes them."""
        self._sync_params()
        return self.engine.forget(X, y, alpha, Li, factors=factors, predict=predict, mode='scaled')

    def loo_raw(self, X_raw, y_scaled, x_scaler, alpha, Li, block=1):
        """Leave-block-out predictions (mu, std, lev, stats) of the rows (X_raw, y_scaled), which must be rows of the fit (alpha, Li), at
        the shared parameter vector: raw rows through the X scaler on the device, targets already scaled (engine.loo)."""
        self._sync_params()
        self._sync_scalers(x_scaler, None)
        return self.engine.loo(X_raw, y_scaled, alpha, Li, block=block, mode='raw')

    def loo_func(self, X, y, alpha, Li, block=1):
        """loo_raw for the scaled training set (X, y) train_func takes: it becomes (or stays) the resident data set and the device
        reads the rows where they lie."""
        self._sync_params()
        self._sync_data(X, y)
        return self.engine.loo(None, None, alpha, Li, block=block)

    def select_raw(self, X_raw, x_scaler, Li, m, weights=None, return_std=False):
        """Greedy maximum-information choice of m of the raw pool rows X_raw under the posterior with factor Li, at the shared parameter
        vector: (idx, var, gain[, std_after]) in scaled-y units, raw rows through the X scaler on the device (engine.select)."""
        self._sync_params()
        self._sync_scalers(x_scaler, None)
        return self.engine.select(X_raw, Li, m, w=weights, raw=True, return_std=return_std)

    def select_iv_raw(self, X_raw, x_scaler, Li, m, Xr_raw=None, weights=None, ref_weights=None, return_std=False):
        """Greedy choice of m of the raw pool rows X_raw by integrated variance reduction over the raw reference rows Xr_raw (None: the
        pool itself) under the posterior with factor Li, at the shared parameter vector: (idx, red, var, ivar[, std_after]) in scaled-y
        units, raw rows through the X scaler on the device (engine.select_iv)."""
        self._sync_params()
        self._sync_scalers(x_scaler, None)
        return self.engine.select_iv(X_raw, Li, m, Xr=Xr_raw, w=weights, wr=ref_weights, raw=True, return_std=return_std)

    def select_qei_raw(self, X_raw, x_scaler, alpha, Li, m, nsamp, best, **kw):
        """Greedy Monte-Carlo batch expected improvement over the raw pool rows X_raw under the posterior (alpha, Li), at the shared
        parameter vector: engine.select_qei with mode 'raw' (best and xi in scaled y units; kw: its xi, seed, w, pending (raw rows),
        minimize, return_score0, return_state)."""
        self._sync_params()
        self._sync_scalers(x_scaler, None)
        return self.engine.select_qei(X_raw, alpha, Li, m, nsamp, best, mode='raw', **kw)

    def value_and_grad(self, X, y):
        """cost, grad, alpha, Li at the current parameters without touching them."""
        return self._evaluate(X, y, True)

    def triple(self):
        return self.train_func, self.train_iter_func, self.pred_func
