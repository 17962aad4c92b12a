"""
SCFGP model facade: the reference's public class (SCFGP/SCFGP.py:21) with its
constructor, attributes and methods -- set_data, optimize, predict, save, load,
get_compiled_funcs, minibatches, message -- plus the README-advertised fit()
(README.md:47-52).  Every number comes from the HIP library through the function
triple of scfgp_amd.funcs; this file is bookkeeping around it.

Deliberate departures from the reference:
  * parameters live in an explicit `Shared` vector, so "restore the best iterate" and
    the pull-back perturbation (SCFGP/SCFGP.py:256,263-264) act on the vector the
    compiled functions really use.  The reference re-binds self.params to new symbolic
    objects there, which makes those lines no-ops; `compat_noop_restore=True`
    reproduces that observable behaviour.
  * np.inf instead of np.Infinity (:224), guarded max_iter//10 (:242), a working
    rmsprop.
  * save()/load() use a portable .npz of arrays (the reference pickles compiled Theano
    functions, :296-310, which cannot be loaded without Theano).
"""
import string
import sys
import time
import warnings

import numpy as np
import numpy.random as npr

from .funcs import CompiledFuncs
from .optimizer import Optimizer as OPT, Shared
from .scaler import Scaler


# optimize(**args) defaults, SCFGP/SCFGP.py:185-202
_OPT_DEFAULTS = dict(obj='COST', algo={'algo': None}, nbatches=1, batchsize=150, cvrg_tol=1e-4,
                     max_cvrg=18, max_iter=500)
_ADAM_DEFAULTS = dict(learning_rate=0.01, beta1=0.9, beta2=0.999, epsilon=1e-8)
_METRICS = (("SCORE", "Model Selection Score"), ("COST", "Hyperparameter Selection Cost"),
            ("MAE", "Mean Absolute Error"), ("NMAE", "Normalized Mean Absolute Error"),
            ("MSE", "Mean Square Error"), ("NMSE", "Normalized Mean Square Error"),
            ("MNLP", "Mean Negative Log Probability"), ("TIME(s)", "Training Time"))


class SCFGP(object):

    """Sparsely Correlated Fourier Features Based Gaussian Process (MI355X build)"""

    ID, NAME, verbose = "", "", True
    X_scaler, y_scaler = [None] * 2
    M, N, D = -1, -1, -1
    X, y, hyper, Li, alpha, train_func, pred_func = [None] * 7

    def __init__(self, sparsity=20, nfeats=18, evals=None,
                 X_scaling_method='auto-inv-normal', y_scaling_method='auto-normal', verbose=False,
                 dtype='f64', device=0, compat_noop_restore=False, device_optimizer=False, device_scaler=False):
        self.S = sparsity
        self.M = nfeats
        self.X_scaler = Scaler(X_scaling_method)
        self.y_scaler = Scaler(y_scaling_method)
        self.evals = {k: [title, []] for k, title in _METRICS} if evals is None else evals
        self.verbose = verbose
        self.dtype, self.device = dtype, device
        self.compat_noop_restore = compat_noop_restore
        self.device_optimizer = device_optimizer
        self.device_scaler = device_scaler          # predict(): X scaling inside the GPU packing kernel
        self.generate_ID()

    def message(self, *arg):
        if self.verbose:
            print(" ".join(map(str, arg)))
            sys.stdout.flush()

    def generate_ID(self):
        self.ID = ''.join(chr(npr.choice([ord(c) for c in (string.ascii_uppercase + string.digits)]))
                          for _ in range(5))
        self.NAME = "SCFGP (Sparsity=%d, Fourier Features=%d)" % (self.S, self.M)

    def init_params(self):
        """Same draw order and distributions as SCFGP/SCFGP.py:64-72."""
        a = npr.randn(1)
        b = npr.randn(1)
        c = npr.randn(1)
        l_f = npr.randn(self.D * self.S)
        r_f = npr.rand(self.M * self.S)
        l_p = 2 * np.pi * npr.rand(self.S)
        p = 2 * np.pi * npr.rand(self.M)
        self.params = Shared(np.concatenate([a, b, c, l_f, r_f, l_p, p]))

    # -- "compilation" ------------------------------------------------------------------------
    def build_hip_models(self, algo, algo_params, momentum=0.9):
        """Counterpart of build_theano_models (SCFGP/SCFGP.py:92-148): creates the GPU context
        and optimiser state bound to self.params; no symbolic build, no C compile.  momentum: the Nesterov
        momentum the reference hard-codes at SCFGP/SCFGP.py:131 (negative: none)."""
        self._compiled = CompiledFuncs(self.D, self.S, self.M, self.params, algo, algo_params, momentum=momentum,
                                       dtype=self.dtype, device=self.device,
                                       device_optimizer=self.device_optimizer)
        self.train_func, self.train_iter_func, self.pred_func = self._compiled.triple()

    build_theano_models = build_hip_models          # drop-in name

    def get_compiled_funcs(self):
        return self.train_func, self.train_iter_func, self.pred_func

    # -- data -----------------------------------------------------------------------------------
    def set_data(self, X, y):
        """X: (N,D) inputs, y: (N,1) targets in original units (SCFGP/SCFGP.py:153-170)."""
        self.message("-" * 60, "\nNormalizing SCFGP training data...")
        self.X_scaler.fit(X)
        self.y_scaler.fit(y)
        # the model's own copies, frozen: the triple's residency check then never hashes them again (funcs.py: _sync_data)
        self.X = np.array(self.X_scaler.forward_transform(X), dtype=np.float64, order='C')
        self.y = np.array(self.y_scaler.forward_transform(y), dtype=np.float64, order='C')
        self.X.flags.writeable = False
        self.y.flags.writeable = False
        self.message("done.")
        self.N, self.D = self.X.shape
        if 'train_func' not in self.__dict__.keys():
            self.message("-" * 60, "\nInitializing SCFGP hyperparameters...")
            self.init_params()
            self.message("done.")
        else:
            cost, self.alpha, self.Li = self.train_func(self.X, self.y)

    def minibatch_indices(self, n, batchsize, shuffle=True):
        """Row indices of successive minibatches (same shuffling and truncation as SCFGP.py:172-182)."""
        inds = np.arange(n)
        if shuffle:
            np.random.shuffle(inds)
        for start_ind in range(0, n - batchsize + 1, batchsize):
            yield inds[start_ind:start_ind + batchsize]

    def minibatches(self, X, y, batchsize, shuffle=True):
        assert len(X) == len(y)
        for batch in self.minibatch_indices(len(X), batchsize, shuffle):
            yield np.ascontiguousarray(X[batch]), np.ascontiguousarray(y[batch])

    # -- training ---------------------------------------------------------------------------------
    def optimize(self, Xv=None, yv=None, funcs=None, visualizer=None, **args):
        """Training driver, SCFGP/SCFGP.py:184-276 (same keyword arguments and defaults)."""
        opt = dict(_OPT_DEFAULTS)
        opt.update({k: v for k, v in args.items() if k in opt})
        obj = str(opt['obj']).upper()
        obj = obj if obj in self.evals else 'COST'
        algo, nbatches, batchsize = opt['algo'], opt['nbatches'], opt['batchsize']
        cvrg_tol, max_cvrg, max_iter = opt['cvrg_tol'], opt['max_cvrg'], opt['max_iter']
        if algo.get('algo') not in OPT.algos:
            algo = {'algo': 'adam', 'algo_params': dict(_ADAM_DEFAULTS)}
        for metric in self.evals.keys():
            self.evals[metric][1] = []
        if funcs is None:
            self.message("-" * 50, "\nCreating SCFGP HIP context...")
            self.build_hip_models(algo['algo'], algo.get('algo_params', {}))
            self.message("done.")
        else:
            self.train_func, self.train_iter_func, self.pred_func = funcs
        # the vector the triple really trains (a reused triple owns its own: Appendix B)
        owner = getattr(self.train_iter_func, '__self__', None)
        live = owner.params if isinstance(owner, CompiledFuncs) else self.params
        animate = None
        if visualizer is not None:
            visualizer.model = self
            animate = visualizer.train_with_plot()
        if Xv is None or yv is None:
            obj = 'COST'
            for k in ('MAE', 'NMAE', 'MSE', 'NMSE', 'MNLP', 'SCORE'):
                self.evals[k][1].append(0)
        self.min_obj_ind = 0
        train_start_time = time.time()
        min_obj_val, argmin_params, cvrg_iter = np.inf, live.get_value(), 0
        for iter in range(max_iter):
            if nbatches > 1:
                cost_sum, params_list, batch_count = 0, [], 0
                for batch in self.minibatch_indices(len(self.X), batchsize):
                    params_list.append(live.get_value())
                    if isinstance(owner, CompiledFuncs):      # gather the batch from the resident rows on the GPU
                        cost, self.alpha, self.Li = owner.train_iter_rows(self.X, self.y, batch)
                    else:
                        cost, self.alpha, self.Li = self.train_iter_func(np.ascontiguousarray(self.X[batch]),
                                                                         np.ascontiguousarray(self.y[batch]))
                    cost_sum += cost; batch_count += 1
                    if batch_count == nbatches:
                        break
                if not self.compat_noop_restore:
                    live.set_value(np.median(np.array(params_list), axis=0))       # :234
                self.evals['COST'][1].append(np.double(cost_sum / batch_count))
            else:
                cost, self.alpha, self.Li = self.train_iter_func(self.X, self.y)
                self.evals['COST'][1].append(cost)
            self.evals['TIME(s)'][1].append(time.time() - train_start_time)
            if Xv is not None and yv is not None:
                self.predict(Xv, yv)
            if iter % max(max_iter // 10, 1) == 1:
                self.message("-" * 17, "VALIDATION ITERATION", iter, "-" * 17)
                self._print_current_evals()
            if animate is not None:
                animate(iter)
            obj_val = self.evals[obj][1][-1]
            if obj_val < min_obj_val:
                if min_obj_val - obj_val < cvrg_tol:
                    cvrg_iter += 1
                else:
                    cvrg_iter = 0
                min_obj_val = obj_val
                self.min_obj_ind = len(self.evals['COST'][1]) - 1
                argmin_params = live.get_value()
            else:
                cvrg_iter += 1
            if iter > 30 and cvrg_iter > max_cvrg:
                break
            elif cvrg_iter > max_cvrg * 0.5 and not self.compat_noop_restore:
                randp = np.random.rand() * cvrg_iter / max_cvrg * 0.5
                live.set_value((1 - randp) * live.get_value() + randp * argmin_params)   # :263
        if not self.compat_noop_restore:
            live.set_value(argmin_params)                                                 # :264
        self.params = live
        cost, self.alpha, self.Li = self.train_func(self.X, self.y)
        self.evals['COST'][1].append(np.double(cost))
        self.evals['TIME(s)'][1].append(time.time() - train_start_time)
        if Xv is not None and yv is not None:
            self.predict(Xv, yv)
        self.min_obj_ind = len(self.evals['COST'][1]) - 1
        disp = self.verbose
        self.verbose = True
        self.message("-" * 19, "OPTIMIZATION RESULT", "-" * 20)
        self._print_current_evals()
        self.message("-" * 60)
        self.verbose = disp

    def fit(self, X, y, Xv=None, yv=None, funcs=None, visualizer=None, **opt):
        """README.md:47-52 / experiments/kin8nm/kin8nm.py:55,58: set_data + optimize."""
        self.set_data(X, y)
        self.optimize(Xv, yv, funcs, visualizer, **opt)
        return self

    # -- prediction ---------------------------------------------------------------------------------
    def predict(self, Xs, ys=None):
        """SCFGP/SCFGP.py:278-294."""
        owner = getattr(self.pred_func, '__self__', None)
        if self.device_scaler and isinstance(owner, CompiledFuncs):
            # scaling, pred_func, back-transform and metrics in one device call
            mu_y, std_y, met = owner.pred_y(Xs, self.X_scaler, self.y_scaler, self.alpha, self.Li, ys)
            if met is not None:
                for k in met:
                    self.evals[k][1].append(met[k])
            return mu_y, std_y
        else:
            self.Xs = np.ascontiguousarray(self.X_scaler.forward_transform(Xs), dtype=np.float64)
            mu_f, std_f = self.pred_func(self.Xs, self.alpha, self.Li)
        mu_y = self.y_scaler.backward_transform(mu_f)
        up_bnd_y = self.y_scaler.backward_transform(mu_f + std_f[:, None])
        dn_bnd_y = self.y_scaler.backward_transform(mu_f - std_f[:, None])
        std_y = 0.5 * (up_bnd_y - dn_bnd_y)
        if ys is not None:
            err = mu_y - ys
            mae, mse = np.mean(np.abs(err)), np.mean(err ** 2.)
            mnlp = 0.5 * np.mean((err / std_y) ** 2 + np.log(2 * np.pi * std_y ** 2))
            nmse = mse / np.var(ys)
            for k, v in (('MAE', mae), ('NMAE', mae / np.std(ys)), ('MSE', mse), ('NMSE', nmse),
                         ('MNLP', mnlp), ('SCORE', nmse / (1 + np.exp(-mnlp)))):
                self.evals[k][1].append(v)
        return mu_y, std_y

    def predict_grad(self, Xs):
        """Predictions and their gradients in the inputs, in raw X and raw y units: mu_y (T,1), std_y (T,1), dmu_y (T,D), dstd_y (T,D)
        with D the raw column count (zero columns where the X scaler dropped a constant column).  mu_y, std_y are those of
        predict(Xs) with device_scaler=True, bit for bit."""
        owner = self._owner('predict_grad')
        mu_y, std_y, dmu_y, dstd_y = owner.pred_grad_y(Xs, self.X_scaler, self.y_scaler, self.alpha, self.Li)
        return mu_y, std_y[:, None], dmu_y, dstd_y

    def predict_gradcov(self, Xs, full=False):
        """Posterior distribution of the gradient of the latent function at the raw rows Xs, in raw X units and the SCALED target's
        units: (mean (T,D), std (T,D)) and, with full=True, also cov (T,D,D) -- grad f(x_t) ~ N(mean[t], cov[t]), std its marginal
        standard deviations; D the raw column count (zeros where the X scaler dropped a constant column).  There are no raw-y units:
        through a non-affine y scaler the gradient is not Gaussian, the argument of predict_cov (include/scfgp_hip.h:
        scfgp_predict_gradcov)."""
        owner = self._owner('predict_gradcov')
        out = owner.pred_gradcov_raw(Xs, self.X_scaler, self.alpha, self.Li, want=('dmu', 'dvar') + (('dcov',) if full else ()))
        res = (out['dmu'], np.sqrt(out['dvar']))
        return res + (out['dcov'],) if full else res

    def active_subspace(self, Xs, w=None):
        """Active subspace of the fitted function over the raw rows Xs (weights w >= 0, None: all 1): (eigenvalues descending (D,),
        eigenvectors (D,D) in columns, asub (D,D)) of asub = E[grad f grad f^T] averaged over the rows -- the posterior mean of the
        gradient's outer product, sum_t w_t (m_t m_t^T + Sigma_t) / sum_t w_t, formed on the device without a (T,D,D) array; the
        eigendecomposition of the D x D matrix runs on the host.  Raw X units, scaled target units."""
        owner = self._owner('active_subspace')
        asub = owner.pred_gradcov_raw(Xs, self.X_scaler, self.alpha, self.Li, w=w, want=('asub',))['asub']
        lam, vec = np.linalg.eigh(asub)
        return lam[::-1].copy(), vec[:, ::-1].copy(), asub

    def _measure(self, who, bounds, measure):
        """(kind, p0, p1, scaled) of sobol / integral: bounds (D_raw, 2) = uniform raw inputs, measure = (kind, p0, p1) per raw column
        in raw units; neither: uniform on the per-column range of the scaled training inputs, at the kept columns"""
        if bounds is not None and measure is not None:
            raise ValueError('%s: give bounds or measure, not both' % who)
        if measure is not None:
            kind, p0, p1 = measure
            return kind, np.asarray(p0, dtype=np.float64), np.asarray(p1, dtype=np.float64), False
        if bounds is not None:
            b = np.asarray(bounds, dtype=np.float64)
            if b.ndim != 2 or b.shape[1] != 2:
                raise ValueError('%s: bounds must be (D, 2)' % who)
            return None, b[:, 0].copy(), b[:, 1].copy(), False
        if getattr(self, 'X', None) is None:
            raise ValueError('%s: no training inputs to take the default measure from (a restored checkpoint): give bounds or measure' % who)
        cols = [int(cc) for cc in self.X_scaler.data['cols']]
        D_raw = max(cols) + 1
        p0 = np.zeros(D_raw); p1 = np.zeros(D_raw)
        p0[cols] = self.X.min(0); p1[cols] = self.X.max(0)
        return None, p0, p1, True

    def sobol(self, bounds=None, measure=None, nsamples=0, seed=0):
        """Variance-based sensitivity of the fitted function under a product measure over the inputs, in closed form (include/
        scfgp_hip.h: scfgp_sobol): a dict with 'S' (D_raw,) the first-order and 'T' (D_raw,) the total-effect Sobol indices of the
        posterior MEAN, 'V' its variance and 'f0' its mean in SCALED y units (the y scaler's backward transform is not affine:
        partial_dependence's argument).  bounds (D_raw, 2): independent uniform inputs in raw X units; measure = (kind, p0, p1) per raw
        column: 0 = uniform on [p0, p1], 1 = normal(p0, p1^2); both need an affine X scaler ('min-max', 'normal').  Neither: uniform on
        the range of the scaled training inputs, which any scaler allows.  Columns the scaler dropped get S = T = 0.  nsamples > 0 adds
        the posterior distribution of every index over that many exact draws of the weights (sample_weights with `seed`): 'S_samples',
        'T_samples' (nsamples, D_raw), 'V_samples', and 'S_mean', 'S_q05', 'S_q95', 'T_mean', 'T_q05', 'T_q95' (NaN-aware).  A function
        whose variance is not above rounding level (1e-12 of its mean square) has no indices: NaN, not a division by zero.
        A measure so far out that its phases leave the domain of the feature map's sin / cos (2 max|Om| |x| >= 3.37e9 in SCALED units)
        raises ValueError; the input that the text names is counted over the SCALED columns, those the X scaler kept, not the raw ones."""
        owner = self._owner('sobol')
        kind, p0, p1, scaled = self._measure('sobol', bounds, measure)

        def ratios(o):
            V = o['V']
            ok = V > 1e-12 * (V + o['f0'] ** 2)
            den = np.where(ok, V, np.nan)[:, None]
            with np.errstate(invalid='ignore', divide='ignore'):
                return o['Vmain'] / den, o['Vtot'] / den

        o = owner.sobol_raw(kind, p0, p1, self.X_scaler, np.asarray(self.alpha, dtype=np.float64).reshape(-1, 1), scaled=scaled)
        S, T = ratios(o)
        out = {'S': S[0], 'T': T[0], 'V': float(o['V'][0]), 'f0': float(o['f0'][0])}
        if nsamples > 0:
            W = owner.sample_weights(self.alpha, self.Li, int(nsamples), seed=seed)
            os_ = owner.sobol_raw(kind, p0, p1, self.X_scaler, W, scaled=scaled)
            Ss, Ts = ratios(os_)
            out.update(S_samples=Ss, T_samples=Ts, V_samples=os_['V'])
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)          # a column that is NaN in every sample
                for name, v in (('S', Ss), ('T', Ts)):
                    out[name + '_mean'] = np.nanmean(v, 0)
                    out[name + '_q05'], out[name + '_q95'] = np.nanquantile(v, [0.05, 0.95], 0)
        return out

    def integral(self, bounds=None, measure=None):
        """Bayesian quadrature: (mean, sd) of the integral of the latent function against the product measure of sobol(), in SCALED y
        units: int f dmu ~ N(phibar^T alpha, kappa |Li phibar|^2) with phibar = E_mu phi(x) from the device (scfgp_sobol) and the
        K-vector products on the host."""
        owner = self._owner('integral')
        kind, p0, p1, scaled = self._measure('integral', bounds, measure)
        phibar = owner.sobol_raw(kind, p0, p1, self.X_scaler, None, want=('phibar',), scaled=scaled)['phibar']
        kappa = float(np.log1p(np.exp(owner.params.get_value(borrow=True)[2])))
        mean = float(phibar @ np.asarray(self.alpha, dtype=np.float64).reshape(-1))
        return mean, float(np.sqrt(kappa) * np.linalg.norm(np.asarray(self.Li, dtype=np.float64) @ phibar))

    def partial_dependence(self, X, dims=None, grid=20, weights=None, ice=False, cov=False):
        """Partial-dependence (PD) curves of single inputs over the raw pool rows X, with their exact posterior uncertainty: a dict with
        'dims' (the raw columns, default: every column the X scaler kept), 'grid' (ndim, G) in raw X units, 'pd' (ndim, G) the curve
        pd[d][i] = sum_t w_t f(x_t with column d set to grid[d][i]) / sum_t w_t, 'sd' (ndim, G) its latent posterior standard deviation,
        'importance' (ndim,) the standard deviation of pd[d] over its grid (the PD-based importance measure) and, on request, 'cov'
        (ndim, G, G) the posterior covariance of every curve and 'ice' (ndim, T, G) the individual conditional expectation curves.
        grid: an integer G for that many quantiles of the pool's own column (per dimension), or an array (G,) shared by all dimensions or
        (ndim, G).  weights: T row weights >= 0.  pd, sd, cov and ice are in the SCALED target's units: the y scaler's backward transform
        is not affine, so a PD curve in raw y units is not Gaussian -- the argument of predict_cov and acquire (include/scfgp_hip.h:
        scfgp_predict_pd)."""
        owner = self._owner('partial_dependence')
        X = np.asarray(X, dtype=np.float64)
        kept = [int(cc) for cc in self.X_scaler.data['cols']]
        dims = kept if dims is None else [int(d) for d in np.atleast_1d(dims)]
        if np.ndim(grid) == 0:
            G = int(grid)
            q = (np.arange(G) + 0.5) / G
            grid = np.stack([np.quantile(X[:, d], q) for d in dims])
        else:
            grid = np.asarray(grid, dtype=np.float64)
            if grid.ndim == 1:
                grid = np.tile(grid, (len(dims), 1))
        want = ('pd', 'sd') + (('cov',) if cov else ()) + (('ice',) if ice else ())
        out = owner.pred_pd_raw(X, self.X_scaler, self.alpha, self.Li, dims, grid, w=weights, want=want)
        out['dims'] = np.array(dims)
        out['grid'] = grid
        out['importance'] = out['pd'].std(axis=1)
        return out

    def sample(self, Xs, nsamples, seed=0, noise=False):
        """nsamples posterior sample functions of the fitted model at the raw rows Xs, in raw y units: (T, nsamples).  Column s is
        phi(x)^T w_s with w_s ~ N(alpha, kappa A^-1) (plus observation noise with noise=True), mapped through the y scaler's backward
        transform; the same seed gives the same functions on any rows (include/scfgp_hip.h: scfgp_sample)."""
        owner = self._owner('sample')
        return owner.sample_y(Xs, self.X_scaler, self.y_scaler, self.alpha, self.Li, nsamples, seed=seed, noise=noise)

    def sample_argmax(self, X_pool, nsamples, seed=0, weights=None, minimize=False):
        """For each of nsamples posterior sample functions, the row of the raw pool X_pool (T,D) that maximises it (minimize: minimises
        it) and its value there: (idx (nsamples,) indices into the pool, val (nsamples,) in raw y units).  The functions are those of
        sample(X_pool, nsamples, seed): val[s] is sample(...)[idx[s], s] bit for bit, and no T x nsamples block is formed anywhere
        (include/scfgp_hip.h: scfgp_sample_argmax).  weights (T,): row t is eligible iff weights[t] > 0.  The row is chosen in scaled
        y units; ties go to the lowest index.  val is a draw of the maximum f* (max-value entropy search), and the share of samples
        that name a row estimates its probability of being the best."""
        owner = self._owner('sample_argmax')
        return owner.sample_argmax_y(X_pool, self.X_scaler, self.y_scaler, self.alpha, self.Li, nsamples, seed=seed, weights=weights,
                                     minimize=minimize)

    def thompson(self, X_pool, m, seed=0, weights=None, minimize=False):
        """Thompson sampling of a batch: m distinct rows of the raw pool X_pool (T,D), row j the maximiser (minimize: minimiser) of
        posterior sample function j.  It runs in rounds of sample_argmax with nsamples = m fixed, so sample j stays the same function:
        round 1 is the plain call; among samples that name the same row the lowest-numbered keeps it; every further round masks the
        rows held so far, calls again and resolves the samples still without a row by the same rule, until all m hold distinct rows.
        weights (T,): row t is eligible iff weights[t] > 0.  ValueError if m exceeds the number of eligible rows.  Returns idx (m,)
        int64, the row held by sample 0 .. m-1; observe them and absorb the results with condition(), as with select()."""
        m = int(m)
        T = np.asarray(X_pool).shape[0]
        w = np.ones(T) if weights is None else np.array(weights, dtype=np.float64).reshape(-1)
        if w.size != T:
            raise ValueError('thompson: weights has %d entries for %d rows' % (w.size, T))
        eligible = int(np.count_nonzero(w > 0))
        if m > eligible:
            raise ValueError('thompson: m = %d but only %d rows are eligible' % (m, eligible))
        held = np.full(max(m, 0), -1, dtype=np.int64)
        first = True
        while first or (held < 0).any():
            idx, _ = self.sample_argmax(X_pool, m, seed=seed, weights=None if first and weights is None else w, minimize=minimize)
            for s in np.flatnonzero(held < 0):                   # ascending: the lowest-numbered sample keeps a contested row
                if not (held == idx[s]).any():
                    held[s] = idx[s]
            w[held[held >= 0]] = 0.0
            first = False
        return held

    def sample_maximize(self, X_pool, nsamples, seed=0, weights=None, bounds=None, minimize=False, max_iter=60, gtol=1e-6):
        """Continuous maximisers (minimize: minimisers) of nsamples posterior sample functions: each function's best row of the raw
        pool X_pool (T,D), as sample_argmax names it, refined off the grid by projected-gradient ascent in raw X (scfgp_amd.ascent on
        include/scfgp_hip.h: scfgp_sample_grad; one device call per step for all samples).  The functions are those of
        sample(., nsamples, seed): their weights come from one sample_weights call.  The ascent runs on the scaled y value: the y
        scaler's backward transform is monotone, so the maximiser is the same.  bounds = (lo, hi), scalars or (D,), default the
        pool's per-column minimum and maximum; weights (T,): pool row t may start a sample iff weights[t] > 0.
        Returns X_best (nsamples, D) raw points inside the bounds, val_y (nsamples,) the functions' values there in raw y units,
        idx_start (nsamples,) the pool rows the ascents started from, converged (nsamples,) bool (projected-gradient norm <=
        gtol max(1, |value|) within max_iter iterations).  In scaled units no value is worse than at its start row.  Nothing of the
        model is touched."""
        from .ascent import ascend
        owner = self._owner('sample_maximize')
        X_pool = np.asarray(X_pool, dtype=np.float64)
        nsamples = int(nsamples)
        idx, _ = self.sample_argmax(X_pool, nsamples, seed=seed, weights=weights, minimize=minimize)
        W = owner.sample_weights(self.alpha, self.Li, nsamples, seed=seed)
        lo, hi = (X_pool.min(0), X_pool.max(0)) if bounds is None else bounds
        fg = lambda X, s: owner.sample_grad_raw(X, self.X_scaler, self.y_scaler, W, sidx=s)
        X_best, _, converged, _ = ascend(fg, X_pool[idx], np.arange(nsamples), lo, hi, minimize=minimize, max_iter=max_iter, gtol=gtol)
        val_y, _ = owner.sample_grad_raw(X_best, self.X_scaler, self.y_scaler, W, sidx=np.arange(nsamples), y_units=True)
        return X_best, val_y, idx, converged

    def _acquire_best(self, best, minimize):
        """the incumbent in scaled y units: `best` (raw y) through the y scaler, or the best observed training target"""
        if best is None:
            y = np.asarray(self.y, dtype=np.float64)
            return float(y.min() if minimize else y.max())
        return float(np.asarray(self.y_scaler.forward_transform(np.array([[float(best)]]))).reshape(-1)[0])

    @staticmethod
    def _acquire_starts(X_pool, acq, weights, starts):
        """the `starts` best distinct eligible pool rows by acq: descending value, ties to the lowest index, a row that repeats an
        earlier start's coordinates skipped"""
        acq = np.asarray(acq, dtype=np.float64).reshape(-1)
        ok = np.ones(acq.size, dtype=bool) if weights is None else np.asarray(weights).reshape(-1) > 0
        order = np.flatnonzero(ok)
        order = order[np.argsort(-acq[order], kind='stable')]
        picked, seen = [], set()
        for t in order:
            key = np.ascontiguousarray(X_pool[t], dtype=np.float64).tobytes()
            if key not in seen:
                seen.add(key); picked.append(int(t))
                if len(picked) == int(starts):
                    break
        return np.array(picked, dtype=np.int64)

    def _owner(self, who):
        owner = getattr(self.pred_func, '__self__', None)
        if not isinstance(owner, CompiledFuncs):
            raise TypeError('%s needs the library\'s pred_func (build_hip_models / fit); got %r' % (who, self.pred_func))
        return owner

    def acquire(self, X_pool, kind, best=None, xi=0.0, beta=None, fstar=None, weights=None, noise=False, minimize=False,
                want=('acq', 'argmax')):
        """Acquisition function `kind` ('ucb', 'pi', 'ei', 'logei', 'mes') at every row of the raw pool X_pool (T,D), and the best
        eligible row (include/scfgp_hip.h: scfgp_acquire).  best: the incumbent in RAW y units (it goes through the y scaler's forward
        transform); None: the best observed training target in the direction of minimize.  xi >= 0: the improvement margin and beta >= 0
        UCB's weight, both in SCALED y units; fstar ('mes'): sampled maxima in scaled y units (see mes()).  The returned acq, val,
        mu and sd are in SCALED y units, the space the model is Gaussian in: the y scaler's backward transform is not affine, so EI
        in raw y has no closed form.  grad is d acq / d x with x in raw X units.  The acquisition is always maximised;
        minimize says that small targets are good.  noise: use the predictive std sigma* instead of the latent sigma_f.  Returns the
        dict of engine.acquire (want: 'acq', 'argmax' -> 'idx', 'val', 'mu', 'sd', 'grad')."""
        owner = self._owner('acquire')
        kw = dict(w=weights, noise=noise, minimize=minimize, want=want)
        if kind == 'ucb':
            kw['beta'] = beta
        elif kind == 'mes':
            kw['fstar'] = fstar
        else:
            kw['best'] = self._acquire_best(best, minimize); kw['xi'] = xi
        return owner.acquire_raw(X_pool, self.X_scaler, self.alpha, self.Li, kind, **kw)

    def kg(self, X_pool, X_ref=None, nodes=None, weights=None, noise=True, minimize=False):
        """Knowledge gradient of every row of the raw pool X_pool (T,D) over the raw reference rows X_ref (R <= 32768; None: the pool
        itself, T <= 32768): the expected gain in the best posterior MEAN over the reference rows from observing the candidate
        (include/scfgp_hip.h: scfgp_acquire_kg), in SCALED y units.  nodes: 3..32 strictly increasing values with exactly one 0.0
        (None: linspace(-5, 5, 31)).  noise: the observation is noisy (the normal case).  minimize: small targets are good.  Returns a
        dict: 'kg' (T,) a lower and 'kg_hi' (T,) an upper bound of the exact value -- their gap certifies the nodes -- and 'idx',
        'val': the lowest eligible row (weights > 0) with the largest kg, and that kg."""
        owner = self._owner('kg')
        return owner.acquire_kg_raw(X_pool, self.X_scaler, self.alpha, self.Li, Xr_raw=X_ref, z=nodes, w=weights, noise=noise,
                                    minimize=minimize, want=('kg', 'kg_hi', 'idx', 'val'))

    def mes(self, X_pool, nsamples, seed=0, weights=None, minimize=False):
        """Max-value entropy search over the raw pool: one sample_argmax call for nsamples draws of the maximum f* in scaled y units,
        then acquire('mes') on the same pool.  Returns acquire's dict with 'fstar' added."""
        owner = self._owner('mes')
        _, fstar = owner.sample_argmax_raw(X_pool, self.X_scaler, self.alpha, self.Li, int(nsamples), seed=seed, weights=weights,
                                           minimize=minimize)
        out = self.acquire(X_pool, 'mes', fstar=fstar, weights=weights, minimize=minimize)
        out['fstar'] = fstar
        return out

    def acquire_maximize(self, X_pool, kind, best=None, xi=0.0, beta=None, fstar=None, weights=None, noise=False, minimize=False,
                         bounds=None, starts=8, max_iter=60, gtol=1e-6):
        """Continuous maximisers of an acquisition function: the `starts` best distinct eligible rows of the raw pool by acquire(),
        refined off the grid by projected-gradient ascent in raw X (scfgp_amd.ascent; one acquire call with grad per step for all
        starts).  bounds = (lo, hi), scalars or (D,), default the pool's per-column minimum and maximum.  Returns X_best (n, D) raw
        points inside the bounds, val (n,) the acquisition values there (scaled units), idx_start (n,) the pool rows the ascents started
        from (descending value), converged (n,) bool; n = min(starts, distinct eligible rows).  No value is below its start row's."""
        from .ascent import ascend
        owner = self._owner('acquire_maximize')
        X_pool = np.asarray(X_pool, dtype=np.float64)
        kw = dict(noise=noise, minimize=minimize)
        if kind == 'ucb':
            kw['beta'] = beta
        elif kind == 'mes':
            kw['fstar'] = fstar
        else:
            kw['best'] = self._acquire_best(best, minimize); kw['xi'] = xi
        acq = owner.acquire_raw(X_pool, self.X_scaler, self.alpha, self.Li, kind, w=weights, want=('acq',), **kw)['acq']
        idx = self._acquire_starts(X_pool, acq, weights, starts)
        lo, hi = (X_pool.min(0), X_pool.max(0)) if bounds is None else bounds

        def fg(X, sidx):                                        # one function for every row: sidx is ignored
            r = owner.acquire_raw(X, self.X_scaler, self.alpha, self.Li, kind, want=('acq', 'grad'), **kw)
            return r['acq'], r['grad']
        X_best, val, converged, _ = ascend(fg, X_pool[idx], np.zeros(idx.size, dtype=np.int64), lo, hi, max_iter=max_iter, gtol=gtol)
        return X_best, val, idx, converged

    def predict_cov(self, Xs, Xs2=None, noise=False):
        """Joint posterior covariance of the fitted model's function values between the raw rows Xs and Xs2 (None: among the rows of
        Xs, a bit-for-bit symmetric matrix): (T, T2) = kappa phi(x)^T A^-1 phi(x').  Inputs are in raw X units; the covariance is that
        of the SCALED target, the space the model is Gaussian in: the y scaler's backward transform is not affine (Box-Cox, normal
        CDF), so no covariance in raw y units follows from the model.  For joint statistics of raw y draw functions with `sample`.
        noise=True (Xs2=None only) adds the observation noise kappa to the diagonal; the diagonal then equals the squared scaled
        std that pred_func reports (include/scfgp_hip.h: scfgp_predict_cov)."""
        owner = self._owner('predict_cov')
        return owner.pred_cov_raw(Xs, self.X_scaler, self.Li, Xb_raw=Xs2, noise=noise)

    def condition(self, X, y):
        """Absorb the observations (X, y), raw inputs (n,D) and raw targets (n,1), into the fitted posterior: self.alpha and self.Li
        become those of the fit on the rows seen so far and these together, at the current hyper-parameters, through a K x K update
        that needs no old rows (include/scfgp_hip.h: scfgp_condition) -- so it works on a model restored by load() that never saw
        set_data.  The scalers are the fitted ones: they are not refitted.  self.X / self.y are NOT touched: a later optimize() or
        set_data() recomputes the factors from the training set it holds, without the absorbed rows.  Returns self."""
        owner = self._owner('condition')
        ys = np.asarray(self.y_scaler.forward_transform(np.asarray(y, dtype=np.float64).reshape(-1, 1)), dtype=np.float64)
        self.alpha, self.Li = owner.condition_raw(X, ys, self.X_scaler, self.alpha, self.Li)
        return self

    def condition_grad(self, X, dY, y=None, rho=None, dims=None):
        """Absorb observed partial derivatives into the fitted posterior, as condition absorbs values (include/scfgp_hip.h:
        scfgp_condition_grad).  X: raw inputs (n,D); dY: the derivatives of the RAW target in the raw inputs, (n,D) or -- with dims, the
        raw columns that were observed -- (n, len(dims)); rho: every observation's precision relative to the value noise, shaped like
        dY (None: 1; 0: not observed); y: the raw targets (n,1) observed at the same points, absorbed as values in the same call (None:
        derivatives only).  A derivative in a constant column that the X scaler dropped is ignored: the model does not depend on it.
        The chain rule through the y scaler needs its forward derivative at the observed y, so a scaler that is not affine ('min-max'
        and 'normal' are) needs y.  Scalers, self.X / self.y and the restored-checkpoint case are as in condition.  Returns self."""
        owner = self._owner('condition_grad')
        dY = np.asarray(dY, dtype=np.float64)
        if dY.ndim != 2:
            raise ValueError('condition_grad: dY must be (n, D) or (n, len(dims))')
        if y is None:
            if not self.y_scaler.affine:
                raise ValueError("condition_grad: the y scaler %r is not affine, so its derivative depends on the observed y: pass y"
                                 % self.y_scaler.algo)
            ys, dfy = None, self.y_scaler.forward_derivative(np.zeros((1, len(self.y_scaler.data['cols']))))
        else:
            y = np.asarray(y, dtype=np.float64).reshape(-1, 1)
            ys = np.asarray(self.y_scaler.forward_transform(y), dtype=np.float64)
            dfy = self.y_scaler.forward_derivative(y)
        self.alpha, self.Li = owner.condition_grad_raw(X, dY * dfy, self.X_scaler, self.alpha, self.Li, dims=dims, rho=rho, y_scaled=ys)
        return self

    def forget(self, X, y):
        """Remove the observations (X, y), raw inputs (n,D) and raw targets (n,1) that ARE rows of the fit, from the fitted posterior:
        self.alpha and self.Li become those of the fit on the remaining rows, at the current hyper-parameters, through a K x K
        downdate that needs no other rows (include/scfgp_hip.h: scfgp_forget): the inverse of condition(X, y), a sliding window when
        the two alternate.  Units, scalers and what is left alone are as in condition: the scalers are not refitted and self.X /
        self.y are NOT touched.  Rows that were not in the fit raise the library's 'not positive definite' error (or, if few, go
        unnoticed: the library cannot check membership).  Returns self."""
        owner = self._owner('forget')
        ys = np.asarray(self.y_scaler.forward_transform(np.asarray(y, dtype=np.float64).reshape(-1, 1)), dtype=np.float64)
        self.alpha, self.Li = owner.forget_raw(X, ys, self.X_scaler, self.alpha, self.Li)
        return self

    def cv(self, X=None, y=None, folds=5, seed=0):
        """K-fold cross-validation of the fitted model with arbitrary folds, without a refit: (mu_y (n,1), std_y (n,1), metrics,
        fold_stats).  Every row is predicted from the fit on all rows but those of its fold, at the current hyper-parameters and with
        the fitted scalers: one scfgp_forget call per fold, which downdates the factors on the device and predicts the fold's rows
        there (no K x K matrix comes back).  folds: an integer k >= 2 -- a random partition into k folds of nearly equal size drawn
        from numpy's default_rng(seed) -- or an array (n,) of fold ids.  Without X, y the rows are the model's own training set; raw
        (X, y) -- ALL rows of the fit, or the held-out predictions condition on more than 'the other rows' -- may be passed instead,
        the only way for a model restored by load().  mu_y / std_y and the six metrics are in raw y units as loo returns them;
        metrics['CV_LPD'] is the mean log predictive density of the scaled targets and 'CV_LOG_JOINT' the sum of the folds' joint log
        densities; fold_stats is the list of the folds' stats (engine.FORGET_STATS, scaled units) with 'fold' (its id) added, in
        ascending id order.  Neither self.evals nor self.alpha / self.Li are touched."""
        owner = self._owner('cv')
        if (X is None) != (y is None):
            raise ValueError('cv: X and y go together (both None: the training set)')
        if X is None:
            if getattr(self, "X", None) is None or getattr(self, "y", None) is None:
                raise ValueError('cv: the model holds no training rows (restored by load()?): pass the raw (X, y) of the fit')
            Xr = np.asarray(self.X, dtype=np.float64)
            fy = np.asarray(self.y, dtype=np.float64).reshape(-1, 1)
            ys = self.y_scaler.backward_transform(fy)
            call = lambda rows: owner.forget_func(Xr[rows], fy[rows], self.alpha, self.Li, factors=False, predict=True)
        else:
            Xr = np.asarray(X, dtype=np.float64)
            ys = np.asarray(y, dtype=np.float64).reshape(-1, 1)
            fy = np.asarray(self.y_scaler.forward_transform(ys), dtype=np.float64)
            call = lambda rows: owner.forget_raw(Xr[rows], fy[rows], self.X_scaler, self.alpha, self.Li, factors=False, predict=True)
        n = Xr.shape[0]
        if np.ndim(folds) == 0:
            k = int(folds)
            if k < 2 or k > n:
                raise ValueError('cv: folds must lie in 2..n')
            ids = np.empty(n, dtype=np.int64)
            ids[np.random.default_rng(seed).permutation(n)] = np.arange(n) % k
        else:
            ids = np.asarray(folds).reshape(-1)
            if ids.size != n:
                raise ValueError('cv: folds has %d entries for %d rows' % (ids.size, n))
        mu_f = np.empty((n, 1)); std_f = np.empty(n); fold_stats = []
        for f in np.unique(ids):
            rows = np.flatnonzero(ids == f)
            m, s, st = call(rows)
            mu_f[rows] = m; std_f[rows] = s
            st['fold'] = f.item()
            fold_stats.append(st)
        mu_y = self.y_scaler.backward_transform(mu_f)
        up_bnd_y = self.y_scaler.backward_transform(mu_f + std_f[:, None])
        dn_bnd_y = self.y_scaler.backward_transform(mu_f - std_f[:, None])
        std_y = 0.5 * (up_bnd_y - dn_bnd_y)
        err = mu_y - ys
        mae, mse = np.mean(np.abs(err)), np.mean(err ** 2.)
        mnlp = 0.5 * np.mean((err / std_y) ** 2 + np.log(2 * np.pi * std_y ** 2))
        nmse = mse / np.var(ys)
        metrics = {'MAE': mae, 'NMAE': mae / np.std(ys), 'MSE': mse, 'NMSE': nmse, 'MNLP': mnlp, 'SCORE': nmse / (1 + np.exp(-mnlp)),
                   'CV_LPD': sum(st['sum_log_marginal'] for st in fold_stats) / n,
                   'CV_LOG_JOINT': sum(st['log_joint'] for st in fold_stats)}
        return mu_y, std_y, metrics, fold_stats

    def loo(self, X=None, y=None, block=1):
        """Exact leave-block-out predictions of training rows, without a refit: (mu_y (n,1), std_y (n,1), metrics).  Row i is predicted
        from the fit on all training rows except the `block` consecutive rows of its block (block=1: leave-one-out; 1..64; permute the
        rows for other folds) at the current hyper-parameters and with the fitted scalers (include/scfgp_hip.h: scfgp_loo).  Without
        arguments the rows are the model's own training set; raw (X, y) -- rows that ARE in the fit -- may be passed instead, which
        is the only way for a model restored by load(), which holds no rows.  mu_y / std_y are in raw y units, through the y scaler
        exactly as predict does it; metrics holds predict's six numbers (MAE, NMAE, MSE, NMSE, MNLP, SCORE) of the held-out
        predictions against y, and 'LOO_LPD', the mean log predictive density of the scaled targets.  Neither self.evals nor
        self.alpha / self.Li are touched."""
        owner = self._owner('loo')
        if (X is None) != (y is None):
            raise ValueError('loo: X and y go together (both None: the training set)')
        if X is None:
            if getattr(self, "X", None) is None or getattr(self, "y", None) is None:
                raise ValueError('loo: the model holds no training rows (restored by load()?): pass the raw (X, y) of the fit')
            mu_f, std_f, _, stats = owner.loo_func(self.X, self.y, self.alpha, self.Li, block=block)
            ys = self.y_scaler.backward_transform(np.asarray(self.y, dtype=np.float64))
        else:
            ys = np.asarray(y, dtype=np.float64).reshape(-1, 1)
            fy = np.asarray(self.y_scaler.forward_transform(ys), dtype=np.float64)
            mu_f, std_f, _, stats = owner.loo_raw(X, fy, self.X_scaler, self.alpha, self.Li, block=block)
        mu_y = self.y_scaler.backward_transform(mu_f)
        up_bnd_y = self.y_scaler.backward_transform(mu_f + std_f[:, None])
        dn_bnd_y = self.y_scaler.backward_transform(mu_f - std_f[:, None])
        std_y = 0.5 * (up_bnd_y - dn_bnd_y)
        err = mu_y - ys
        mae, mse = np.mean(np.abs(err)), np.mean(err ** 2.)
        mnlp = 0.5 * np.mean((err / std_y) ** 2 + np.log(2 * np.pi * std_y ** 2))
        nmse = mse / np.var(ys)
        metrics = {'MAE': mae, 'NMAE': mae / np.std(ys), 'MSE': mse, 'NMSE': nmse, 'MNLP': mnlp, 'SCORE': nmse / (1 + np.exp(-mnlp)),
                   'LOO_LPD': stats['sum_log_marginal'] / stats['n']}
        return mu_y, std_y, metrics

    def select(self, X_pool, m, weights=None):
        """Which m rows of the raw pool X_pool (T,D) to observe next: (idx (m,) indices into the pool in the order they are picked,
        std (m,), gain (m,)).  Pick j is the row whose function value is most uncertain (times its weight) given the training set and
        the picks before it -- the exact greedy maximiser of the batch's information gain, without targets and without a refit per
        pick (include/scfgp_hip.h: scfgp_select).  std[j] is the posterior std of f at pick j when it was picked, in scaled-y units
        (noise excluded); gain[j] its information gain in nats.  weights (T,) >= 0 scale the criterion, 0 excludes a row.  Points that
        are pending (chosen but not yet observed) are handled by condition(X_pending, any y) on a copy of the model first: the
        choice depends on Li alone.  The library's message is raised on error.  Nothing of the model is touched."""
        owner = self._owner('select')
        idx, var, gain = owner.select_raw(X_pool, self.X_scaler, self.Li, m, weights=weights)
        return idx, np.sqrt(var), gain

    def select_iv(self, X_pool, m, X_ref=None, weights=None, ref_weights=None):
        """Which m rows of the raw pool X_pool (T,D) to observe next so that the model is most certain over X_ref (R,D; None: the
        pool itself): (idx (m,) indices into the pool in the order they are picked, red (m,), ivar (2,)).  Pick j is the row whose
        observation most reduces the posterior variance of f summed over the reference rows (times ref_weights), given the training
        set and the picks before it -- integrated variance reduction (ALC / A-optimal), without targets and without a refit per pick
        (include/scfgp_hip.h: scfgp_select_iv).  red[j] is the reduction pick j achieved and ivar the summed variance before and
        after the m picks, in squared scaled-y units (noise excluded).  weights (T,) >= 0 scale the criterion, 0 excludes a row.
        Pending points: condition(X_pending, any y) on a copy of the model first.  Nothing of the model is touched."""
        owner = self._owner('select_iv')
        idx, red, _, ivar = owner.select_iv_raw(X_pool, self.X_scaler, self.Li, m, Xr_raw=X_ref, weights=weights, ref_weights=ref_weights)
        return idx, red, ivar

    def select_qei(self, X_pool, m, nsamples=256, best=None, xi=0.0, seed=0, weights=None, pending=None, minimize=False):
        """Which m rows of the raw pool X_pool (T,D) to try together, for improvement over the incumbent: (idx (m,) indices into the pool
        in the order they are picked, gain (m,)).  The greedy maximiser of the Monte-Carlo batch expected improvement (q-EI) under
        nsamples joint posterior sample functions (include/scfgp_hip.h: scfgp_select_qei): pick j is the row that adds most to the
        expected improvement of the batch so far, and gain[j] is what it adds, in SCALED y units; the gains never increase, and a gain
        of 0 says that no sample can still improve.  best: the incumbent in RAW y units, None: the best observed training target in
        the direction of minimize (as acquire); xi >= 0: the improvement margin in scaled y units.  weights (T,): row t is eligible
        iff weights[t] > 0.  pending (np,D): raw rows chosen earlier whose results are not in yet; they count through their sampled
        values, so the new picks go elsewhere.  The same seed gives the same functions in every call.  A loop with parallel,
        unequally long experiments:

            running, best = np.empty((0, D)), float(y_train.min())       # rows under way; the incumbent in raw y units
            while budget:
                idx, gain = model.select_qei(pool, free_slots, best=best, pending=running, minimize=True)
                running = np.vstack([running, pool[idx]])                # start them
                X_done, y_done = wait_for_some(running)                  # observe
                model.condition(X_done, y_done)                          # absorb the results (condition leaves model.y alone,
                best = min(best, float(y_done.min()))                    #  so the caller keeps the incumbent)
                running = remove_rows(running, X_done)                   # the unfinished ones stay pending

        Nothing of the model is touched."""
        owner = self._owner('select_qei')
        idx, gain, _ = owner.select_qei_raw(X_pool, self.X_scaler, self.alpha, self.Li, m, int(nsamples), self._acquire_best(best, minimize),
                                            xi=xi, seed=seed, w=weights, pending=pending, minimize=minimize)
        return idx, gain

    # -- persistence -----------------------------------------------------------------------------------
    def save(self, path):
        """Portable checkpoint (arrays only; never pickles code).  The reference pickles the compiled
        train_iter_func itself (SCFGP/SCFGP.py:296-302), i.e. its Adam moments, step counter and Nesterov velocity
        (SCFGP/Optimizer.py:314-323,92-93); here they are saved as arrays next to the rule's name and keyword
        arguments, so load() + optimize(funcs=model.get_compiled_funcs()) continues the same trajectory."""
        import json
        sc = {}
        for tag, s in (('X', self.X_scaler), ('y', self.y_scaler)):
            sc[tag + '_algo'] = s.algo
            for k, v in s.data.items():
                sc['%s_scaler_%s' % (tag, k)] = np.asarray(v)
        ev = {'evals_' + k: np.asarray(v[1], dtype=np.float64) for k, v in self.evals.items()}
        opt = {}
        cf = getattr(self, '_compiled', None)
        owner = getattr(getattr(self, 'train_iter_func', None), '__self__', None)
        if isinstance(owner, CompiledFuncs):
            cf = owner                                     # a reused triple owns the state that is being trained
        if cf is not None:
            plain = {k: (v.item() if isinstance(v, np.generic) else v) for k, v in cf.algo_params.items()}   # np.float32(0.01) etc.
            opt = {'opt_algo': cf.algo, 'opt_kwargs': json.dumps(plain, sort_keys=True),
                   'opt_momentum': float(cf.momentum), 'opt_device': bool(cf.device_optimizer), 'dtype': str(cf.dtype)}
            for i, a in enumerate(cf.get_opt_state()):
                opt['opt_state_%d' % i] = a
        with open(path, 'wb') as f:
            np.savez(f, ID=self.ID, S=self.S, M=self.M, D=self.D, params=self.params.get_value(),
                     alpha=self.alpha, Li=self.Li, **sc, **ev, **opt)

    def load(self, path):
        import json
        algo, kwargs, opt_state, momentum = 'adam', dict(_ADAM_DEFAULTS), None, 0.9
        with np.load(path, allow_pickle=False) as z:
            self.ID = str(z['ID']); self.S = int(z['S']); self.M = int(z['M']); self.D = int(z['D'])
            self.params = Shared(z['params'])
            self.alpha, self.Li = z['alpha'], z['Li']
            for tag in ('X', 'y'):
                s = Scaler(str(z[tag + '_algo']))
                pre = '%s_scaler_' % tag
                for k in z.files:
                    if k.startswith(pre):
                        v = z[k]
                        s.data[k[len(pre):]] = [int(c) for c in v] if k.endswith('cols') else v
                setattr(self, tag + '_scaler', s)
            for k in self.evals:
                if 'evals_' + k in z.files:
                    self.evals[k][1] = list(z['evals_' + k])
            if 'opt_algo' in z.files:                       # checkpoints written before the optimiser was saved lack these
                algo, kwargs = str(z['opt_algo']), json.loads(str(z['opt_kwargs']))
                self.device_optimizer = bool(z['opt_device']); self.dtype = str(z['dtype'])
                momentum = float(z['opt_momentum']) if 'opt_momentum' in z.files else 0.9
                n = len([k for k in z.files if k.startswith('opt_state_')])
                opt_state = [z['opt_state_%d' % i] for i in range(n)]
        self.NAME = "SCFGP (Sparsity=%d, Fourier Features=%d)" % (self.S, self.M)
        self.build_hip_models(algo, kwargs, momentum)
        if opt_state is not None:
            self._compiled.set_opt_state(opt_state)

    def _print_current_evals(self):
        for metric in sorted(self.evals.keys()):
            if len(self.evals[metric][1]) < len(self.evals['COST'][1]):
                continue
            best_perform_eval = self.evals[metric][1][self.min_obj_ind]
            self.message(self.NAME, "%7s = %.4e" % (metric, best_perform_eval))
