/*
 * scfgp_hip.h -- C ABI of libscfgp_hip.so: the MI355X (gfx950) implementation of the
 * SCFGP Fourier-feature marginal-likelihood hot path.
 *
 * The library stands behind the reference's "compiled function triple"
 *     train_func(X,y)       -> [cost, alpha, Li]              SCFGP/SCFGP.py:132-135
 *     train_iter_func(X,y)  -> same outputs + parameter update SCFGP/SCFGP.py:136-137
 *     pred_func(Xs,alpha,Li)-> [mu, std]                       SCFGP/SCFGP.py:138-148
 * i.e. it replaces what theano.function compiled from build_theano_models
 * (SCFGP/SCFGP.py:92-148, gradient from TT.grad at :129).  The optimiser update rule
 * (SCFGP/Optimizer.py) stays on the host above this boundary so its callback signature
 * remains user-extensible; the library returns the exact gradient it needs.
 *
 * Conventions
 *   - every function returns 0 or a negative error code (scfgp_finish and scfgp_factor may also return SCFGP_REDO = 1);
 *     nothing throws across the ABI;
 *     scfgp_last_error() gives a message for the last failure on that context
 *   - the caller owns every host buffer; the library owns all device memory
 *   - host matrices are row-major, C-contiguous float64 regardless of compute dtype
 *     (the reference's graph is float64 throughout: TT.dmatrices, SCFGP/SCFGP.py:95-96,138)
 *   - a context is bound to one GPU and is not thread-safe; calls are synchronous unless
 *     stated otherwise (results are on the host when the call returns)
 *   - K = 2*(S+M) is the Gram dimension, P = 3 + D*S + M*S + S + M the parameter count
 *     (SCFGP/SCFGP.py:72)
 */
#ifndef SCFGP_HIP_H
#define SCFGP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct scfgp_ctx scfgp_ctx;

#define SCFGP_OK            0
#define SCFGP_EARG         -1   /* bad argument / wrong call order                       */
#define SCFGP_EHIP         -2   /* HIP runtime error                                     */
#define SCFGP_ENOTPD       -3   /* A = Phi^T Phi + (e^{2a}+1e-6) I not positive definite:
                                   the reference raises numpy.linalg.LinAlgError from its
                                   Cholesky op (SCFGP/SCFGP.py:106)                      */
#define SCFGP_ENONFINITE   -4   /* cost is NaN/Inf                                       */
#define SCFGP_EPEER        -5   /* row shards: ANOTHER rank failed in this evaluation (its exchange
                                   buffers carried the failure mark, scfgp_fail_stage): every rank
                                   returns this from scfgp_finish / scfgp_eval / scfgp_train; the
                                   results are not valid, the context stays usable            */
#define SCFGP_REDO          1   /* not an error, staged API only.  scfgp_finish: the evaluation
                                   ran at a lower precision level than its own condition estimate
                                   asks for; the level has been raised.  scfgp_factor: the ranks
                                   have just agreed on a lower level than some of them ran pass 1
                                   at.  Either way: run the stages again from scfgp_pass1
                                   (scfgp_eval / scfgp_eval_rows do that themselves)      */

#define SCFGP_F64 0             /* fp64 MFMA everywhere (reference numerics)             */
#define SCFGP_F32 1             /* N-sized products in exact-fp32 MFMA, fp64 projection,
                                   fp64 cross-chunk accumulation and fp64 K x K stage    */
#define SCFGP_F16X3 2           /* SECONDARY mode, never what a benchmark headline quotes: SCFGP_F32 in everything but the four
                                   N-sized products (V = Phi B, Phibar = 2 Phi Abar + ..., Phi^T Phi, V^T diag(q) V), which run as a
                                   THREE-TERM fp16 split on the fp16 matrix pipe wherever fp32 mode uses its 256-wide LDS-DMA tiles
                                   (K >= 1024, >= 65536 rows) at precision level 0: x = (h + l) 2^-e, h, l fp16, one power-of-two
                                   scale per operand matrix; h.h + l.h + h.l in fp32 accumulators (fp16 products are exact in
                                   fp32; the Gram folds its accumulators every 512 rows because the instruction truncates).
                                   Errors within 4x of SCFGP_F32's (scfgp_amd/csrc/apply_f16.hip, gram_f16.hip); it runs fp32
                                   mode's parity tier.  Option "f16_gram" = 0 keeps the fp32 Gram in this mode               */

/* ---- life cycle --------------------------------------------------------------------
 * Replaces SCFGP.build_theano_models (SCFGP/SCFGP.py:92-148): "compile" becomes "create a
 * context".  D,S,M as in SCFGP.__init__/set_data (SCFGP/SCFGP.py:36-37,164).
 * `stream` is a hipStream_t (NULL = the context creates its own); passing the stream of
 * the host framework keeps the library's work ordered with that framework's collectives.
 * On failure (negative return) *out is still set whenever the context object itself could be made -- so that
 * scfgp_last_error(*out) can say which allocation or HIP call failed -- and holds whatever was allocated up to that point:
 * the caller must hand it to scfgp_destroy (scfgp_amd/engine.py does). */
int  scfgp_create(scfgp_ctx** out, int D, int S, int M, int dtype, int device, void* stream);
void scfgp_destroy(scfgp_ctx* ctx);
const char* scfgp_last_error(const scfgp_ctx* ctx);

/* ---- implicit state: the shared parameter vector -------------------------------------
 * The reference binds hyper-parameters with givens=[(params, self.params)]
 * (SCFGP/SCFGP.py:134-137,147-148): they are state of the compiled functions, not
 * arguments.  Layout [a,b,c,l_f(D*S),r_f(M*S),l_p(S),p(M)] (SCFGP/SCFGP.py:72,74-90).
 *
 * Range of the three scalars.  s = e^b sqrt(2/M), lam = e^{2a} + 1e-6, kappa = softplus(c) (formed as log1p(e^c), or c + log1p(e^-c)
 * for c > 0), e^{-2a} and sigmoid(c) are formed in fp64 in every mode, each to a few ulp, over a in [-8, 3], b in [-6, 6] and
 * c in [-36, 36]; over that range results are held to the mode's precision times what the point's conditioning costs any float64
 * evaluation: alpha and Li carry cond(A) u, and cond(A) grows like e^{2b} / lam; the cost's term e^{-2a} (y^T y - g^T alpha) cancels
 * at small a, in the reference's formula too (tests/test_gpu_hyper_range.py holds every output to the float64 oracle's own error
 * against an mpmath evaluation at the same point).  Outside it: c beyond +-36 stays finite and monotone (kappa -> c above,
 * kappa -> e^c > 0 below, down to c = -700); a and b are limited by the overflow of e^{2a}, e^{-2a} and e^b alone.
 * A row of l_f whose entries are all equal (always, with S = 1) or such a row of F = l_f r_f^T has standard deviation 0: when every
 * row of one of the two is so, the penalty's -log(sum of stds) is +infinity, as in the reference, and the evaluation returns that
 * cost with SCFGP_ENONFINITE; a single such row among others leaves the cost finite and that row's penalty gradient 0/0 = NaN. */
int scfgp_set_params(scfgp_ctx* ctx, const double* params, int P);
int scfgp_get_params(scfgp_ctx* ctx, double* params, int P);

/* ---- training data: upload once, keep resident ----------------------------------------
 * X (N,D), y (N) already scaled (what SCFGP.set_data stores in self.X/self.y,
 * SCFGP/SCFGP.py:161-162).  n_global is the N the objective divides by and uses in
 * 2(N-M)a (X.shape[0] at SCFGP/SCFGP.py:126,128): equal to N on one GPU, the sum over
 * ranks when rows are sharded. */
int scfgp_set_data(scfgp_ctx* ctx, const double* X, const double* y, int64_t N, int64_t n_global);

/* ---- train_func / train_iter_func ------------------------------------------------------
 * One evaluation at the current parameters.  X==NULL uses the resident rows; otherwise
 * (minibatches, SCFGP/SCFGP.py:226-235) the given rows replace them first.
 * want_grad=0 is train_func (forward only); want_grad=1 additionally returns
 * d cost / d params (P) -- what TT.grad (SCFGP/SCFGP.py:129) feeds the update rule.
 * Outputs (any may be NULL): cost (1), grad (P), alpha (K), Li (K*K row-major, lower
 * triangular, zeros above the diagonal).
 * Range of the phases, here and in every entry point that evaluates the feature map (predict, predict_grad, predict_cov, sample,
 * condition, loo, select): sin / cos are good to the last bit or so for |z| < 2^31 pi/2 = 3.37e9 rad in both modes; beyond that
 * (unscaled X, parameters blown up by a large step) Phi is finite, of the right magnitude and in the wrong quadrant, silently. */
int scfgp_eval(scfgp_ctx* ctx, const double* X, const double* y, int64_t N, int want_grad,
               double* cost, double* grad, double* alpha, double* Li);

/* ---- minibatches by index list ----------------------------------------
 * The reference's minibatch loop (SCFGP/SCFGP.py:172-182,226-235) fancy-indexes host copies of X, y
 * and re-passes them; here the batch is a gather of n rows of the RESIDENT data set on the device.
 * Same per-batch semantics (N := n in 2(N-M)a and /N).  A later scfgp_eval(X=NULL) sees all rows again. */
int scfgp_eval_rows(scfgp_ctx* ctx, const int64_t* idx, int64_t n, int want_grad,
                    double* cost, double* grad, double* alpha, double* Li);

/* ---- pred_func  (SCFGP/SCFGP.py:138-148) ------------------------------------------------
 * mu (T), std (T) for Xs (T,D) given alpha (K) and Li (K*K) as returned by scfgp_eval. */
int scfgp_predict(scfgp_ctx* ctx, const double* Xs, int64_t T, const double* alpha, const double* Li,
                  double* mu, double* std);

/* ---- predict on unscaled inputs (input side) -------------------------------
 * SCFGP.predict applies X_scaler.forward_transform on the host before pred_func
 * (SCFGP/SCFGP.py:279, SCFGP/Scaler.py:99-116): min-max, Box-Cox, z-score / normal CDF per column.
 * With the fitted per-column parameters registered once (D doubles each; NULL = unused by `mode`:
 * 0 none, 1 min-max, 2 normal, 3 inv-normal, 4 auto-normal, 5 auto-inv-normal) scfgp_predict_raw
 * takes the column-selected raw Xs and applies the transform inside its packing kernel. */
int scfgp_set_x_scaler(scfgp_ctx* ctx, int mode, const double* min, const double* max, const double* boxcox,
                       const double* mu, const double* std);
int scfgp_predict_raw(scfgp_ctx* ctx, const double* Xs_raw, int64_t T, const double* alpha, const double* Li,
                      double* mu, double* std);
/* The rest of SCFGP.predict on the device (SCFGP/SCFGP.py:281-293, SCFGP/Scaler.py:118-135): with the
 * fitted single-column y scaler registered (same mode numbers), scfgp_predict_y returns
 * mu_y = backward(mu_f) and std_y = (backward(mu_f + std_f) - backward(mu_f - std_f)) / 2 (T doubles each)
 * and, when raw targets ys (T) are given, metrics[6] = MAE, NMAE, MSE, NMSE, MNLP, SCORE.  The X scaler
 * registered with scfgp_set_x_scaler (or none) is applied to Xs_raw as in scfgp_predict_raw. */
int scfgp_set_y_scaler(scfgp_ctx* ctx, int mode, double min, double max, double boxcox, double mu, double std);
int scfgp_predict_y(scfgp_ctx* ctx, const double* Xs_raw, int64_t T, const double* alpha, const double* Li,
                    const double* ys, double* mu_y, double* std_y, double* metrics);
/* Gradients of the predictive mean and std in the inputs.  mu, std (T doubles each) as the predict call of `mode` returns them, bit
 * for bit; dmu, dstd (T x D row-major) their derivatives in the inputs that call takes:
 *   mode 0  scaled Xs, as scfgp_predict: d mu / d x, d std / d x
 *   mode 1  column-selected raw Xs through the registered X scaler, as scfgp_predict_raw: the same chained through the derivative of
 *           the scaler's forward transform, column by column
 *   mode 2  mode 1 and the y scaler, as scfgp_predict_y: mu, std are mu_y, std_y; dmu = bw'(mu) d mu,
 *           dstd = (bw'(mu + std) (d mu + d std) - bw'(mu - std) (d mu - d std)) / 2 (bw = the y scaler's backward transform)
 * dstd may be NULL: then only the mean gradient is formed (no V* = Phi* B product).  SCFGP_EARG for bad arguments, a missing scaler
 * (modes 1, 2) or parameters not set.  Where a scaler's derivative is an infinite factor times a normal density that has underflowed to 0
 * in fp64 (X mode 5 at x = min with an exponent below 1 and |z| > 38.6; y mode 5 at mu, mu +- std = 0 or 1) the product is formed as 0 * inf
 * and the entry is NaN where the limit is infinite: non-finite either way. */
int scfgp_predict_grad(scfgp_ctx* ctx, const double* Xs, int64_t T, const double* alpha, const double* Li, int mode,
                       double* mu, double* std, double* dmu, double* dstd);
/* ---- posterior sample functions (no reference counterpart: the reference reports the marginals only) ---------------------------
 * With A = Phi^T Phi + (sigma_n^2 + eps) I = L L^T, Li = L^-1, alpha = Li^T Li Phi^T y and kappa = softplus(c) (SCFGP/SCFGP.py:103-110),
 * pred_func's marginals are mu*(x) = phi(x)^T alpha and sigma*(x)^2 = kappa (1 + ||Li phi(x)||^2).  Since A^-1 = Li^T Li, the weights
 *     w_s = alpha + sqrt(kappa) Li^T z_s,   z_s ~ N(0, I_K),   i.e. w ~ N(alpha, kappa A^-1),
 * give sample functions f_s(x) = phi(x)^T w_s with mean mu*, variance sigma*^2 - kappa and covariance kappa phi(x)^T A^-1 phi(x');
 * y_s(x) = f_s(x) + sqrt(kappa) eps_s(x) has pred_func's marginal N(mu*, sigma*^2).  Index k of w runs over alpha's layout (the J cosine
 * features, then the J sine features).
 * Random numbers (part of the contract: a sample function is a function -- the same seed gives the same S functions in any call, on any
 * rows, in any chunking, and sample s does not depend on nsamp or T): Philox4x64-10 (Random123), counter (c0, c1, 0, 0), key (seed, stream);
 * U(u) = ((u >> 11) + 0.5) 2^-53; with the four words w of a block and p = (s & 3) >> 1, r = sqrt(-2 ln U(w[2p])), the normal is
 * r cos(2 pi U(w[2p+1])) for even s, r sin(2 pi U(w[2p+1])) for odd s (fp64).
 *     z[k][s]    block (k, s >> 2), stream 0            eps[t][s]  block (t, s >> 2), stream 1   (t: the row's index in the call's Xs)
 * 1 <= nsamp <= 1024; alpha, Li as scfgp_eval returns them (Li lower triangular: entries above the diagonal are not read).
 * scfgp_sample_weights: W (K x nsamp, row-major, fp64) = alpha 1^T + sqrt(kappa) Li^T Z, computed in fp64 in every compute mode.
 * scfgp_sample: out (T x nsamp, row-major) = f_s(x_t), plus sqrt(kappa) eps[t][s] if `noise`; mode 0 scaled Xs (as scfgp_predict),
 *   1 column-selected raw Xs through the registered X scaler (as scfgp_predict_raw), 2 mode 1 and then the y scaler's backward transform
 *   of every element (as scfgp_predict_y: samples in raw y units).  Phi* W runs in the context's precision (fp64 MFMA; exact fp32 MFMA
 *   with fp64 partial sums in SCFGP_F32 and SCFGP_F16X3, which agree bit for bit); device memory does not grow with T.
 * SCFGP_EARG for bad arguments, a missing scaler (modes 1, 2) or parameters not set. */
int scfgp_sample_weights(scfgp_ctx* ctx, const double* alpha, const double* Li, int nsamp, uint64_t seed, double* W);
int scfgp_sample(scfgp_ctx* ctx, const double* Xs, int64_t T, const double* alpha, const double* Li, int nsamp,
                 uint64_t seed, int mode, int noise, double* out);
/* scfgp_sample_argmax: for each of nsamp sample functions, the pool row that maximises it and its value there -- Thompson sampling, and
 * the sampled maxima f* of max-value entropy search and "probability of being the best row".  The sample functions are scfgp_sample's:
 * the same generator, W and seed contract.  With out[t][s] what scfgp_sample(..., noise = 0) returns for these rows in mode
 * min(mode, 1), and row t eligible iff w == NULL or w[t] > 0:
 *     idx[s] = the lowest eligible t at which out[t][s] is largest (minimize != 0: smallest)        val[s] = out[idx[s]][s], bit for bit
 * val may be NULL, idx may not.  There is no noise argument: the maximiser of a noisy draw means nothing.  w (T, may be NULL = every row
 * is eligible) has scfgp_select's meaning "0 excludes"; positive values are not multiplied in.  mode 0: scaled rows; 1: column-selected
 * raw rows through the registered X scaler; 2: mode 1, and val[s] is the y scaler's backward transform of the mode-1 value by the device
 * function scfgp_sample mode 2 applies (equal bits; with the inv-normal y scalers it may be non-finite, as there), while idx is chosen in
 * scaled units and equals mode 1's.
 * The product Phi* W is scfgp_sample's kernel with a second epilogue: its feature loop, its fp64 folding of the fp32 accumulators and its
 * launch plan are shared, so every value has scfgp_sample's bits, and nothing of size T x nsamp is written anywhere.  Each workgroup
 * reduces its rows to one (value, row) record per sample, and one thread per sample merges the records into a running best that stays on
 * the device across chunks.  One rule at every level: record a = (v, t) beats b iff key(a) > key(b), or the keys are equal and
 * a.t < b.t, with key = v, or -v when minimising (exact).  On the eligible records that is a total order, so the result does not depend
 * on how the records are grouped: lanes, waves, workgroups, column-tile launches or chunks.
 * Bounds: 1 <= nsamp <= 1024; T >= 1 without limit: the rows go through in chunks, and device memory holds the per-workgroup records of
 * two chunks, never a T x nsamp buffer.
 * Guarantees: idx[s] and val[s] do not depend on nsamp (a call with fewer samples returns a prefix).  A value depends on its row only
 * and ties go to the lowest index, so appending rows, or duplicating rows later in the pool, changes nothing.  SCFGP_F16X3 contexts run
 * fp32 mode's kernels and agree with it bit for bit.  The training state of the context survives.
 * SCFGP_EARG (with a scfgp_last_error text, before any device work) for NULL Xs, alpha, Li or idx, T < 1, nsamp out of range, a bad
 * mode, a missing X scaler (modes 1, 2) or y scaler (mode 2), parameters not set, a negative w, or no row with w > 0; SCFGP_ENONFINITE for
 * a non-finite w, and for a non-finite value of an eligible row in any sample (a non-finite row with w = 0 is not an error): the outputs
 * are untouched in both cases.  Row-sharded use needs no communicator: each rank calls it on its rows and the caller merges the
 * (val, idx + offset) pairs by the rule above (for mode 2, merge mode-1 values and transform afterwards, or rely on the transform being
 * monotone).  Continuous refinement of a maximiser off the pool: scfgp_sample_grad gives the value and input gradient of a sample
 * function at any point.  A batch chosen for improvement from the same sample functions: scfgp_select_qei.  Out of scope: top-k per
 * sample, and weights or factors kept on the device between calls. */
int scfgp_sample_argmax(scfgp_ctx* ctx, const double* Xs, int64_t T, const double* w, const double* alpha, const double* Li, int nsamp,
                        uint64_t seed, int mode, int minimize, int64_t* idx, double* val);
/* scfgp_sample_grad: values and input gradients of sample functions, one sample per row -- what a gradient method needs to move each
 * sample's best pool row off the grid (Thompson sampling or max-value entropy search in a continuous domain).
 *     val[t] = f_s(x_t) = phi(x_t)^T w_s,   grad[t][:] = d f_s / d x at x_t,   s = sidx[t]   (sidx == NULL: s = t % nsamp)
 * W (K x nsamp, row-major, fp64) is what scfgp_sample_weights returns: column s is w_s in alpha's layout (J cosine features, then J
 * sine features).  Any K-vectors are allowed: W = alpha with nsamp = 1 gives the mean.  The call takes W, not (alpha, Li, seed): an
 * optimiser calls it tens of times with the same functions and pays K nsamp doubles of upload per call, never the K x K factor or the
 * weight kernel.  val (T) may be NULL; grad (T x D, row-major) may not.  This is the paired form (row t belongs to one sample: one
 * current point per sample, or a few starts per sample); the cross form, every row under every sample, is obtained by repeating rows.
 * Modes as scfgp_predict_grad: 0 scaled rows; 1 column-selected raw rows through the registered X scaler, grad chained through the
 * derivative of its forward transform column by column; 2 mode 1, and val = bw(f) by the device function scfgp_sample mode 2 applies,
 * grad = bw'(f) grad f (bw: the y scaler's backward transform).
 * Numerics: Phi* in the context's type.  With Zbar_j = phi_c_j w[J + j] - phi_s_j w[j] formed in fp64 from the fp64 weights and rounded
 * once to the context's type, grad = Zbar F_all^T by fp64 MFMA (fp64 contexts) or exact-fp32 MFMA (SCFGP_F32 and SCFGP_F16X3, which agree
 * bit for bit): scfgp_predict_grad's loop for dmu with the row's own weights in alpha's place, same feature order and MFMA pairing.
 * val = sum_j phi_c_j w[j] + phi_s_j w[J + j] is summed in fp64 in one fixed order that depends on J alone; it does not claim
 * scfgp_sample's bits (in fp32 contexts it is the more accurate of the two: scfgp_sample sums in fp32 MFMA).
 * Bounds: 1 <= nsamp <= 1024; T >= 1 without limit: the rows go through in chunks and device memory does not grow with T.
 * Guarantees: a row's val and grad depend on the row, its weight vector and the parameters only, bit for bit -- not on T, the row's
 * position, the chunk, nsamp or the other samples present.  With nsamp = 1 and W = alpha, mode-0 grad equals scfgp_predict_grad's dmu
 * bit for bit.  The training state of the context survives.
 * SCFGP_EARG (with a scfgp_last_error text, before any device work) for NULL Xs, W or grad, T < 1, nsamp out of range, a bad mode, a
 * missing X scaler (modes 1, 2) or y scaler (mode 2), parameters not set, or an sidx entry outside [0, nsamp) (the text names the first
 * such row); SCFGP_ENONFINITE for a non-finite W: the outputs are untouched in both cases.  Non-finite rows give non-finite outputs and
 * no error, as scfgp_sample.
 * Out of scope: the T x nsamp x D cross form, gradients of noisy draws, Hessians, a device-resident optimiser, weights kept on the
 * device between calls, a row-sharded form (per-row work: each rank calls it on its own rows). */
int scfgp_sample_grad(scfgp_ctx* ctx, const double* Xs, int64_t T, const double* W, int nsamp, const int64_t* sidx, int mode,
                      double* val, double* grad);

/* ---- acquisition functions over a pool (no reference counterpart) -------------------------------------------------------------------------
 * scfgp_acquire: UCB, probability of improvement, expected improvement, log-EI and max-value entropy search at every row of a pool, the
 * best eligible row, and the input gradient of the acquisition value -- the criteria of a Bayesian-optimisation loop as a by-product of
 * scfgp_predict's chunk.  Everything is in scaled-y units (scfgp_predict's).  With sgn = +1, or -1 when `minimize` is set, u = sgn mu*(x),
 * sigma = sigma_f = sqrt(kappa v) for noise == 0 (the spread of scfgp_sample's noise-free functions; v = ||Li phi(x)||^2) or
 * sigma = sigma* = sqrt(kappa (1 + v)) for noise != 0 (pred_func's std), Phi / phi the standard normal CDF / PDF, lam = phi / Phi and
 * h(g) = g Phi(g) + phi(g):
 *     kind 0  UCB    u + beta sigma                                             par = [beta], beta >= 0
 *     kind 1  PI     Phi(g),   g = (u - sgn best - xi) / sigma                  par = [best, xi], xi >= 0
 *     kind 2  EI     sigma h(g)                                                 par = [best, xi]
 *     kind 3  LOGEI  log sigma + log h(g): EI's logarithm, finite where EI underflows
 *     kind 4  MES    (1 / n*) sum_s [ g_s lam(g_s) / 2 - log Phi(g_s) ],  g_s = (sgn f*_s - u) / sigma    no par; fstar (nstar = n*), 1 <= n* <= 1024
 * fstar is what scfgp_sample_argmax(..., mode <= 1, the same minimize) returns in val; every MES term is >= 0.  The acquisition is always
 * maximised, whatever minimize is.  sigma_f is formed from the fp64 v itself, never as sqrt(sigma*^2 - kappa).  All acquisition arithmetic
 * is fp64 in every compute mode; only mu and v come from the context's precision (SCFGP_F16X3 contexts run fp32 mode's kernels and agree
 * with it bit for bit).  The tail forms (scfgp_amd/csrc/acquire.hip) keep log Phi, lam and log h accurate for very negative g; a MES term
 * loses absolute eps g^2 there, where two g^2 / 2 cancel.
 * Outputs, each may be NULL, but not acq, idx and grad all together:
 *     acq (T)        the value of every row
 *     idx, val (1)   row t is eligible iff w == NULL or w[t] > 0 (scfgp_sample_argmax's meaning and host-side checks); idx[0] = the lowest
 *                    eligible t at which acq is largest, val[0] = acq[idx[0]] bit for bit; scfgp_sample_argmax's merge rule at every level,
 *                    the running best stays on the device across chunks; val needs idx
 *     mu, sd (T)     mu* with scfgp_predict's bits (the same partial sums in the same order) and the sigma used (with noise != 0:
 *                    scfgp_predict's std bit for bit)
 *     grad (T x D)   d acq / d x = sgn a_u d mu* / d x + a_sigma d sigma / d x with scfgp_predict_grad's kernels (a_u, a_sigma: the partials
 *                    of the value in u and sigma); in mode 1 chained through the X scaler's derivative
 * mode 0: scaled rows; 1: column-selected raw rows through the registered X scaler.  There is no raw-y mode: the y scaler's backward
 * transform is not affine, so EI in raw y units has no closed form (as scfgp_predict_cov).
 * Bounds: T >= 1 without limit: the rows go through in chunks; device memory beside the chunk buffers is 3 T doubles (mu, sd, acq) plus
 * T x D for grad.
 * Guarantees: a row's acq, mu, sd and grad depend only on the row, the factors, the parameters and the call's scalars and fstar -- not on T,
 * the row's position, the chunk or w.  idx and val do not change when the pool is appended to itself.  The MES sum over the samples runs in
 * one fixed order that depends on n* alone.  The training state of the context survives.
 * SCFGP_EARG (with a scfgp_last_error text, before any device work) for NULL Xs, alpha or Li, T < 1, a bad kind or mode, npar not matching
 * the kind, NULL par where the kind needs one, beta < 0 or xi < 0, kind 4 with NULL fstar or nstar outside [1, 1024], fstar given for
 * another kind, a missing X scaler in mode 1, parameters not set, a negative w, no positive w, no output requested, val without idx.
 * SCFGP_ENONFINITE for a non-finite par, fstar or w (on the host, before any device work) and for an eligible row whose mu, sigma or value
 * is non-finite or whose sigma is 0 (found on the device); a non-finite row with w = 0 is not an error and its acq is whatever comes out.
 * The outputs are untouched in every error case.  Row-sharded use: each rank calls it on its rows and the caller merges (val, idx + offset)
 * by the merge rule.  Batch (q-) expected improvement: scfgp_select_qei.  Knowledge gradient: scfgp_acquire_kg.  Out of scope: top-k,
 * raw-y acquisitions, factors or f* kept on the device between calls. */
int scfgp_acquire(scfgp_ctx* ctx, const double* Xs, int64_t T, const double* w, const double* alpha, const double* Li,
                  int kind, const double* par, int npar, const double* fstar, int nstar, int mode, int noise, int minimize,
                  double* acq, int64_t* idx, double* val, double* mu, double* sd, double* grad);

/* ---- knowledge gradient over a pool (no reference counterpart) ---------------------------------------------------------------------------
 * scfgp_acquire_kg: the acquisition for the case where the answer reported at the end is the best posterior MEAN over a reference set (the
 * pool, a grid, the region of interest), not the best observed value -- the normal case with noisy observations.  Candidates Xc (T rows),
 * reference rows Xr (R rows); sgn = +1, or -1 with `minimize`; u_r = sgn mu*(x_r) with scfgp_predict's bits, d_r = u_r - max_r u_r <= 0.
 * Observing candidate i moves every u_r to u_r + b_ir Z, Z ~ N(0, 1), with
 *     b_ir = kappa <Li phi(x_i), Li phi(x_r)> / sigma_i
 * whose numerator is scfgp_predict_cov's element bit for bit and whose sigma_i is scfgp_acquire's with the same `noise` (sigma* =
 * sqrt(kappa (1 + v_i)) for noise != 0, a noisy observation; sigma_f = sqrt(kappa v_i) for noise == 0).  The knowledge gradient is
 *     KG_i = E[ max_r (d_r + b_ir Z) ] >= 0,
 * the expectation of the upper envelope of R lines.  The T x R matrix b is never formed: the caller passes J nodes z_1 < ... < z_J (finite,
 * exactly one of them 0.0) and the product's epilogue reduces every element into
 *     m_ij = max_r (d_r + b_ir z_j)          the envelope's value at z_j; formed as t = b z, then d + t: two roundings, no fma
 *     s_ij = b_ir at the maximiser           its slope there; ties go to the lowest r
 *     bmin_i, bmax_i = min_r, max_r b_ir     its slopes at -inf, +inf
 * With h(x) = x Phi(x) + phi(x) (scfgp_acquire's, with its tail forms), two closed-form numbers per candidate bracket KG_i:
 *     kg (T)      the expected maximum of the J tangents (m_ij, s_ij): slopes that do not exceed the last kept one merge with it; the
 *                 tangents kept at nodes j' < j meet at c = (icpt' - icpt_j) / (s_j - s'), icpt = m - s z, clamped into [z_{j-1}, z_j]
 *                 (where it lies in exact arithmetic); kg_i = sum (s_j - s') h(-|c|).  This is the exact knowledge gradient over the
 *                 reference rows that win at some node: never above KG_i.  The node 0.0 makes the tangent envelope 0 at 0 (max d = 0).
 *     kg_hi (T)   the expectation of the chord interpolant through (z_j, m_ij), continued with the slopes bmin_i, bmax_i outside the nodes:
 *                 kg_hi_i = sum_j max(q_j - q_{j-1}, 0) h(-|z_j|), q_j = (m_{i,j+1} - m_ij) / (z_{j+1} - z_j) clamped into [s_ij, s_{i,j+1}]
 *                 (a convex function's chord lies between its end slopes; exact arithmetic needs no clamp), q_0 = bmin_i, q_J = bmax_i:
 *                 never below KG_i.  The gap kg_hi - kg is the caller's certificate that the nodes were enough.
 * Every term of both sums is >= 0.  With R = 1 both are 0 exactly.  All node arithmetic is fp64 in every compute mode (SCFGP_F16X3
 * contexts run fp32 mode's kernels and agree with it bit for bit).
 * Xr == NULL: the reference set is the candidates (R is ignored, T <= 32768); the result is bit-equal to the call with Xr = Xc.
 * Outputs, each may be NULL, but not all of kg, kg_hi, idx, m and s together:
 *     kg, kg_hi (T)       as above
 *     idx, val (1)        row t is eligible iff w == NULL or w[t] > 0 (scfgp_acquire's meaning and host-side checks); idx[0] = the lowest
 *                         eligible t at which kg is largest, val[0] = kg[idx[0]] bit for bit, by scfgp_acquire's merge rule; val needs idx
 *     m, s (T x J each)   the node table, row-major
 * mode 0: scaled rows; 1: column-selected raw rows through the registered X scaler (Xc and Xr alike).  There is no raw-y mode (as
 * scfgp_acquire and scfgp_predict_cov).
 * Bounds: 1 <= R <= 32768 (scfgp_predict_cov's Tb bound: the reference rows' factor stays resident for the call); T >= 1 without limit, in
 * chunks; 3 <= J <= 32 (the node state of a 128-row strip shares the CU's LDS with the product's operand images).  Device memory beside
 * the chunk buffers: 2 T doubles, 2 T J more with m or s, and a fixed 64 K x (2 J + 2) doubles of node state: nothing grows with T x R.
 * Guarantees: a candidate's kg, kg_hi, m and s depend on its own row, the SET of reference rows, the factors, the parameters and z -- not
 * on T, the row's position, the chunk, w or the column split of the launch.  Permuting the reference rows, or appending the reference set
 * to itself, leaves every output bit-identical unless two reference rows with different b tie exactly at a node (max is exact and
 * order-free).  idx and val do not change when the pool is appended to itself.  The training state of the context survives.
 * SCFGP_EARG (with a scfgp_last_error text, before any device work) for NULL Xc, alpha, Li or z, T < 1, R outside [1, 32768], T > 32768 in
 * the symmetric form, J outside [3, 32], nodes that are not strictly increasing or do not hold exactly one 0.0, a bad mode, a missing X
 * scaler in mode 1, parameters not set, a negative w, no positive w, no output requested, val without idx.  SCFGP_ENONFINITE for a
 * non-finite z or w (on the host, before any device work), a non-finite u_r, and an eligible candidate whose sigma is 0 or whose sigma, kg
 * or kg_hi is non-finite (found on the device); a non-finite candidate with w = 0 is not an error and its outputs are whatever comes out.
 * The outputs are untouched in every error case.  Out of scope: the exact envelope on the device, the input gradient of KG, batch or
 * pending-row KG, reference-row weights, more than 32 nodes, a raw-y form, factors kept on the device between calls. */
int scfgp_acquire_kg(scfgp_ctx* ctx, const double* Xc, int64_t T, const double* w, const double* Xr, int64_t R,
                     const double* alpha, const double* Li, const double* z, int J, int mode, int noise, int minimize,
                     double* kg, double* kg_hi, int64_t* idx, double* val, double* m, double* s);

/* ---- joint posterior covariance between test points (no reference counterpart: the reference reports the marginals only) -------
 * Under the weight posterior w ~ N(alpha, kappa A^-1) above, two function values have covariance kappa phi(x)^T A^-1 phi(x'); with
 * A^-1 = Li^T Li that is
 *     cov[i][j] = Cov[f(a_i), f(b_j)] = kappa <Li phi(a_i), Li phi(b_j)>        (Ta x Tb, row-major, fp64)
 * the exact matrix of which the sample covariance of scfgp_sample's draws is an estimate.  Its diagonal is sigma*^2 - kappa.
 * Xb == NULL is the symmetric form: Tb is ignored, the result is Ta x Ta, symmetric bit for bit and equal bit for bit to the cross form
 * with Xb = Xa; noise != 0 adds kappa to its diagonal (the covariance of the noisy observations that scfgp_sample(..., noise = 1) draws).
 * With Xb given, noise != 0 is SCFGP_EARG: row i of Xa and row j of Xb are different observations even if the numbers agree.
 * mode 0: scaled inputs (as scfgp_predict); 1: column-selected raw inputs through the registered X scaler (as scfgp_predict_raw).  There
 * is no raw-y mode: the y scaler's backward transform is not affine (Box-Cox, normal CDF), so the model defines no covariance in raw y
 * units; scfgp_sample mode 2 is the route to joint statistics of raw y.
 * Li as scfgp_eval returns it (entries above the diagonal are not read); alpha is not needed.  1 <= Tb <= 32768 (in the symmetric form,
 * Ta); Ta >= 1 otherwise without limit: the rows of Xa go through in chunks and the result leaves through two staging panels, so device
 * memory does not grow with Ta x Tb.  The products run in the context's precision (fp64 MFMA; exact fp32 MFMA with fp64 partial sums
 * in SCFGP_F32 and SCFGP_F16X3, which agree bit for bit); an element's value depends on its two rows only, not on Ta, Tb or its place
 * in the call.  The training state of the context survives.  SCFGP_EARG (with a scfgp_last_error text, before any device work) for bad
 * arguments, a missing X scaler in mode 1 or parameters not set. */
int scfgp_predict_cov(scfgp_ctx* ctx, const double* Xa, int64_t Ta, const double* Xb, int64_t Tb, const double* Li, int mode, int noise,
                      double* cov);

/* ---- absorbing new observations into a fitted posterior (no reference counterpart: the reference refits on all rows) --------------
 * The posterior of a Fourier-feature model is a Bayesian linear model in K weights, so n new rows enter it through a K x K update that
 * never looks at the old rows.  With A = Phi^T Phi + lam I = L L^T, Li = L^-1, alpha = A^-1 Phi^T y a fit and (Xn, yn) new rows with
 * features Phi_n at the SAME hyper-parameters:
 *     C = Phi_n Li^T (n x K)         r = yn - Phi_n alpha              S = I + C^T C = M M^T  (M lower; eigenvalues >= 1)
 *     Li' = M^-1 Li                  gamma = S^-1 C^T r                alpha' = alpha + Li^T gamma
 * A' = A + Phi_n^T Phi_n = L S L^T = (L M)(L M)^T and L M is lower triangular with a positive diagonal, so Li' is THE inverse Cholesky
 * factor of the fit on all rows and (alpha', Li') are what scfgp_eval returns on the concatenated data: everything that takes
 * (alpha, Li) keeps working.  Nothing but alpha, Li and the parameters is needed (a model restored from a checkpoint has no rows).
 * mode 0: scaled rows (as scfgp_predict); 1: column-selected raw Xn through the registered X scaler (as scfgp_predict_raw).  yn is always
 * the SCALED target: the device has only the y scaler's backward transform.  alpha (K) and Li (K x K, entries above the diagonal are not
 * read) as scfgp_eval returns them; alpha_out (K) and Li_out (K x K, lower triangular, zeros above the diagonal) may alias the inputs and
 * are written only on success.  n >= 1 without limit: the rows go through in chunks whose C^T C and C^T r are summed in fp64, so device
 * memory does not grow with n.  The feature map uses the context's CURRENT parameters; that they are the ones Li was computed with is the
 * caller's contract (the library cannot check it).  The products run in the context's precision (fp64 MFMA; exact fp32 MFMA with fp64
 * sums across 4096-row blocks in SCFGP_F32 and SCFGP_F16X3, which agree bit for bit); the K x K stage is fp64: Cholesky of S, and
 * Li' = M^-1 Li as a lower-triangular x lower-triangular product that skips the zero blocks of both operands (K^3 / 3 flops).  The training
 * state of the context survives (resident rows, exchange buffers, Li / B of the last evaluation, optimiser state, precision level).
 * SCFGP_EARG (with a scfgp_last_error text, before any device work) for NULL pointers, n < 1, a bad mode, a missing X scaler in mode 1 or
 * parameters not set; SCFGP_ENONFINITE for non-finite rows, targets or factors; SCFGP_ENOTPD if the Cholesky of S fails: the outputs are
 * untouched in all three cases.  S has eigenvalues >= 1 in exact arithmetic; in SCFGP_F32 / SCFGP_F16X3 contexts C^T C carries an error of
 * eps32 |S|, so the Cholesky can fail once |S| nears 1 / eps32 (seen at lam_max(S) = 9e8: 46 rows joining a fit of 16 at a = -7, b = 3).
 * Out of scope: a communicator / row-sharded form (the update is replicated work on n rows: every rank
 * calls it with the same rows) and keeping the factors resident on the device between calls.  Removing observations: scfgp_forget. */
int scfgp_condition(scfgp_ctx* ctx, const double* Xn, const double* yn, int64_t n, const double* alpha, const double* Li, int mode,
                    double* alpha_out, double* Li_out);

/* ---- absorbing derivative observations into a fitted posterior (no reference counterpart: the reference refits, on values only) -----
 * The gradient of the model is linear in its weights, grad f(x) = J(x)^T w, so an observed partial derivative is a linear observation of w
 * like an observed value, and it enters the posterior through scfgp_condition's update with another row.  Notation as there.  n points Xn
 * (n x D); dims (nd entries in 0..D-1, distinct, in any order; NULL: all D inputs in order, and then nd must be D) names the inputs whose
 * partial derivative was observed; Gn (n x nd): Gn[t][j] = d f / d x_dims[j] at point t, observed with noise of variance kappa / rho[t][j];
 * rho (n x nd; NULL: all 1): the precision of every observation relative to the value noise, >= 0 and finite, 0 = "not observed"; yn (n;
 * NULL: none): the values observed at the same points, with noise kappa -- one call then absorbs (f, grad f) as one run of a simulator
 * with an adjoint returns them.  Every point contributes a block of nb = nd + (yn ? 1 : 0) consecutive rows to Phi_n:
 *     the value row      phi_t                                                                       target  yn[t]
 *     derivative row j   psi_tj = sqrt(rho[t][j]) g_t[d] (-phi_s o F_all[d, :] | phi_c o F_all[d, :])       target  sqrt(rho[t][j]) Gn[t][j]
 * with d = dims[j], phi = (phi_c | phi_s) = s (cos z | sin z) the features of point t and F_all the x-part of the phase projection
 * (d z / d x).  From these rows C, r, S = I + C^T C = M M^T, Li' = M^-1 Li and alpha' = alpha + Li^T gamma are exactly scfgp_condition's,
 * so (alpha', Li') are the factors of A' = A + Phi_n^T Phi_n and everything that takes (alpha, Li) keeps working.  A value update followed
 * by a derivative update equals the joint update, in either order.
 * mode 0: scaled rows, Gn the derivative of the SCALED target in the SCALED input (g_t = 1); 1: column-selected raw rows through the
 * registered X scaler, Gn the derivative of the scaled target in the RAW input: the row carries the scaler's derivative g_t[d] at the raw
 * input, the factor scfgp_predict_grad and scfgp_predict_gradcov chain their outputs with.  There is no raw-y mode, as in scfgp_condition.
 * Promises: Li_out is exactly zero above the diagonal; alpha_out (K) and Li_out (K x K) may alias alpha and Li and are written only on
 * success; the training state of the context survives; SCFGP_F16X3 contexts agree with SCFGP_F32 ones bit for bit; an entry with rho = 0
 * contributes exact zeros, and the outputs do not depend, bit for bit, on what Gn holds there as long as it is finite (rho of all ones
 * has rho == NULL's bits); n >= 1 without limit: the points go through in chunks of floor(32768 / nb) whole points whose C^T C and C^T r
 * are summed in fp64, so device memory does not grow with n.  The first pass (features, rows, C, C^T C, C^T r) and the K x K stage are fp64
 * in every context, as in scfgp_forget and on its buffers: a derivative row is |F_all[d, :]| sqrt(rho / J) times as long as a value row, the
 * rounding errors of fp32 products grow with the square of that, and a precise observation (rho = 100) at K = 2112 put the predictions 200
 * fp32 bounds off; SCFGP_F32 and SCFGP_F16X3 contexts run the fp64 kernels of precision level 1 for it.  D is not limited: dims selects
 * rows of F_all.
 * SCFGP_EARG (with a scfgp_last_error text "condition_grad: ...", before any device work) for a NULL Xn, Gn, alpha, Li or output; n < 1;
 * nd < 1, nd > D or nb > 32768; dims == NULL with nd != D; a dims entry out of range or repeated (the text names its position); a bad mode;
 * a missing X scaler in mode 1 or parameters not set; a negative rho, reported by its first (row, column) even where it stands behind a
 * non-finite one; every rho zero with no yn.  SCFGP_ENONFINITE for non-finite rows, observations, rho or factors; SCFGP_ENOTPD if the
 * Cholesky of S fails: the outputs are untouched in all three cases.  Out of scope: the downdate (taking derivative observations back out;
 * scfgp_forget removes values only), derivatives along arbitrary directions, a communicator / row-sharded form, and factors kept resident
 * on the device between calls. */
int scfgp_condition_grad(scfgp_ctx* ctx, const double* Xn, int64_t n, const int32_t* dims, int nd, const double* Gn, const double* rho,
                         const double* yn, const double* alpha, const double* Li, int mode, double* alpha_out, double* Li_out);

/* ---- removing observations from a fitted posterior (no reference counterpart: the reference refits on the remaining rows) ------------
 * The mirror image of scfgp_condition: n rows (Xo, yo) that ARE in the fit leave it through a K x K downdate that needs only alpha, Li,
 * the parameters and the rows being removed.  Notation as there; Phi_o the features of the removed rows at the SAME hyper-parameters:
 *     C = Phi_o Li^T (n x K)         r = yo - Phi_o alpha              S = I - C^T C = M M^T  (M lower; eigenvalues in (0, 1])
 *     Li' = M^-1 Li                  gamma = S^-1 C^T r                alpha' = alpha - Li^T gamma
 * A' = A - Phi_o^T Phi_o = L S L^T = (L M)(L M)^T, so (alpha', Li') are what scfgp_eval returns on the remaining rows (A' alpha' = A alpha -
 * Phi_o^T yo gives the sign).  S is positive definite exactly when the rows were in the fit; otherwise it may have no Cholesky factor
 * and the call returns SCFGP_ENOTPD.  The held-out predictions of the removed rows under the downdated fit -- the next step of
 * cross-validation with arbitrary folds -- are formed on the device from factors that never leave it: mu_i = phi_i^T alpha',
 * std_i = sqrt(kappa (1 + |Li' phi_i|^2)), and the joint log density of the block given the other rows needs no n x n matrix
 * (det(I - C C^T) = det S, (I - C C^T)^-1 = I + C S^-1 C^T):
 *     log p(yo | rest) = -1/2 [ (r^T r + |M^-1 C^T r|^2) / kappa + n log(2 pi kappa) - 2 sum_i log M_ii ]
 * which is scfgp_loo's block formula for any n.
 * mode 0: scaled rows; 1: column-selected raw rows through the registered X scaler.  yo is always the SCALED target.  alpha (K) and Li
 * (K x K, entries above the diagonal are not read) as scfgp_eval returns them.  Three output groups, of which at least one is asked for:
 *   alpha_out (K), Li_out (K x K, exactly zero above the diagonal): both or neither; they may alias alpha and Li;
 *   mu, std (n each): both or neither; bit for bit what scfgp_predict (mode 0) or scfgp_predict_raw (mode 1) returns for the same rows
 *     when given the returned (alpha', Li'): a second pass over Xo after the K x K stage, on the typed transpose of the device's Li';
 *   stats (8 doubles, may be NULL, needs mu / std), with e = yo - mu: [0] n, [1] sum e^2, [2] sum |e|, [3] sum_i log N(yo_i; mu_i,
 *     std_i^2), [4] the joint log density above, [5] min_i M_ii^2 (how close to singular the downdate was: M_ii^2 <= 1, and a value
 *     near 0 says that what remains barely determines some direction of the weights), [6] 1, [7] 0.  [0] to [3] are formed from the
 *     rounded outputs in row order by one thread: the same bits on every run.
 * With the factor outputs omitted a cross-validation fold uploads Li once and downloads 2 n + 8 doubles.  All outputs are written only
 * on success.  n >= 1 without limit: the rows go through in chunks of 32768 in both passes, so device memory does not grow with n.  The
 * first pass (features, C, C^T C, C^T r) and the K x K stage are fp64 in every context: where scfgp_condition adds the rounding error of
 * C^T C to eigenvalues >= 1, here it is divided by lam_min(S), so SCFGP_F32 and SCFGP_F16X3 contexts run the fp64 kernels of precision
 * level 1 for it (on fp64 chunk buffers of the call's own, allocated by the first call) and agree bit for bit; the second pass is
 * scfgp_predict's, in the context's precision.  Removing nearly everything a direction of the weights was determined by costs accuracy
 * in any precision, and stats[5] shows it.  The training state of the context survives.  SCFGP_EARG (with a scfgp_last_error text, before any device work) for NULL inputs, n < 1, a
 * bad mode, half an output group, stats without mu / std, no output group at all, a missing X scaler in mode 1 or parameters not set;
 * SCFGP_ENONFINITE for non-finite rows, targets or factors; SCFGP_ENOTPD if S has no Cholesky factor (the rows were not in this fit):
 * the outputs are untouched in all three cases.  Out of scope: a communicator / row-sharded form, raw-y units, factors kept resident
 * on the device between calls, and gradients of these numbers in the hyper-parameters. */
int scfgp_forget(scfgp_ctx* ctx, const double* Xo, const double* yo, int64_t n, const double* alpha, const double* Li, int mode,
                 double* alpha_out, double* Li_out, double* mu, double* std, double* stats);

/* ---- exact leave-one-out / leave-block-out predictions of rows that are IN the fit (no reference counterpart: the reference refits) --
 * How well does the fitted model predict rows it has not seen -- without a refit.  With A = Phi^T Phi + lam I = L L^T, Li = L^-1,
 * alpha = A^-1 Phi^T y the fit on all rows and I a set of b of ITS rows (features Phi_I, targets y_I):
 *     C = Phi_I Li^T (b x K)         H = C C^T = Phi_I A^-1 Phi_I^T  (eigenvalues in [0, 1): lam > 0)        r = y_I - Phi_I alpha
 *     I - H = R R^T (R lower)        e = y_I - mu^{-I} = (I - H)^-1 r          Sigma^{-I} = kappa (I - H)^-1  (noise included, as predict)
 *     log p(y_I | the other rows) = -1/2 [ |R^-1 r|^2 / kappa + b log(2 pi kappa) - 2 sum_i log R_ii ]         leverage h_i = H_ii
 * (Woodbury on A - Phi_I^T Phi_I; b = 1: e = r / (1 - h), sigma^2 = kappa / (1 - h)).  mu^{-I} and sigma_i = sqrt(kappa [(I - H)^-1]_ii)
 * are exactly what scfgp_predict returns for the rows I from the fit on the OTHER rows.
 * X (n x D), y (n, the SCALED targets): rows that are in the fit (alpha, Li) was computed from, at the context's current parameters --
 * the caller's contract, as in scfgp_condition.  mode 0: scaled rows; 1: column-selected raw rows through the registered X scaler.
 * X == NULL && y == NULL: the rows made resident by scfgp_set_data (n is ignored, mode must be 0); they are featurised again chunk by
 * chunk from the stored rows at the current parameters, never read from the evaluation's working set (which may hold a minibatch).
 * block (1..64): the held-out sets are the consecutive rows [j block, min(n, (j + 1) block)) of the call's rows, the last one may be
 * ragged; for other folds permute the rows.  Outputs: mu, std (n each): held-out mean and std of every row when its block is left out;
 * lev (n, may be NULL): h_i; stats (8 doubles, may be NULL), with e = y - mu: [0] n, [1] sum e^2, [2] sum |e|, [3] sum_i log N(y_i; mu_i,
 * std_i^2), [4] sum over blocks of the joint log density (block 1: the same number as [3], bit for bit), [5] max h_i, [6] number of
 * blocks, [7] 0.  The sums are fp64, formed from the rounded outputs in block order by one thread: the same bits on every run.
 * n >= 1 without limit: the rows go through in chunks of floor(32768 / block) whole blocks, so device memory does not grow with n.  A
 * row's outputs depend on the rows of its own block only, bit for bit (not on n, the chunk or the block's position).  C runs in the
 * context's precision (SCFGP_F16X3 contexts run fp32 mode's kernels and agree with it bit for bit); H = C C^T is formed by fp64 MFMA and
 * everything after it is fp64.  Accuracy goes with 1 / (1 - lam_max(H_I)): |D mu|, |D sigma| stay within a modest multiple of
 * u sigma / (1 - lam_max) with u = 2^-53 in SCFGP_F64 contexts and eps32 = 2^-24 in SCFGP_F32 / SCFGP_F16X3 ones (measured down to
 * 1 - lam_max = 6e-9 in fp64).  In SCFGP_F32 / SCFGP_F16X3 contexts rows that ARE in the fit can draw SCFGP_ENOTPD once 1 - lam_max
 * approaches eps32 || |C||C|^T ||: seen at 1 - lam_max = 2e-8 with 62 rows of a K = 64 fit in one block and, where C has large cancelling
 * entries (a = -7, b = 3), already at 4e-7 for single rows, while 4e-6 still went through; stats[5] near 1 is the warning.  The training
 * state of the context survives (resident rows, exchange buffers, optimiser state, precision
 * level).  SCFGP_EARG (with a scfgp_last_error text, before any device work) for bad pointers, mode or block, a missing X scaler in mode
 * 1, no resident rows, or parameters not set; SCFGP_ENONFINITE for non-finite rows, targets or factors; SCFGP_ENOTPD if some I - H has no
 * Cholesky factor (the rows were not in the fit): the message names the first such block.  On these two stats is untouched and mu, std,
 * lev hold nothing of use.  Row-sharded use needs no communicator: each rank calls it on its own rows with the common (alpha, Li) and
 * the caller adds the stats ([5]: the maximum).  Out of scope: folds of more than 64 rows or of rows that are not consecutive (they want
 * the K x K downdate: scfgp_forget), gradients of these numbers in the hyper-parameters, raw-y units, and factors kept on the device between calls. */
int scfgp_loo(scfgp_ctx* ctx, const double* X, const double* y, int64_t n, const double* alpha, const double* Li, int mode, int block,
              double* mu, double* std, double* lev, double* stats);

/* ---- posterior covariance of the input gradient, and the active-subspace matrix of a pool (no reference counterpart) -------------------
 * scfgp_predict_grad differentiates the two predictive moments; this is the posterior DISTRIBUTION of grad f(x) itself.  Notation of
 * Phi = s [cos Z | sin Z], Z = X~ F_all, F_all[d] = [l_F[d,:] | F[d,:]], F = l_F r_F^T, B = A^-1 = Li^T Li, kappa =
 * softplus(c).  grad f(x) = J(x)^T w is linear in the K weights w ~ N(alpha, kappa A^-1), hence Gaussian with mean grad mu* and
 * covariance kappa J(x)^T A^-1 J(x).  The derivative partner of a feature row is phi'(x) = (-phi_s | phi_c) = s [-sin z | cos z].
 * Every phase is z = x l_F [I | r_F^T] + offset, so every gradient lies in span(l_F): with q = min(D, S), Q (J x q) and P (D x q) such that
 * F_all[d][j] = sum_i P[d][i] Q[j][i],
 *     D <= S (dense form,  q = D): Q[j][i] = F_all[i][j], P = I            D > S (latent form, q = S): Q = [I_S | r_F^T]^T, P = l_F
 * and per point t
 *     Psi_t (q x K): row i = phi'_t o (Q[:,i] ; Q[:,i])     C'_t = Psi_t Li^T (q x K)     H_t = C'_t C'_t^T (q x q)
 *     Sigma_t = kappa P H_t P^T (D x D) = Cov[grad f(x_t)]          m_t = grad mu*(x_t)  (scfgp_predict_grad's dmu)
 * There is no noise term: the observation noise has no gradient.  mode 0: scaled Xs.  mode 1: column-selected raw Xs through the
 * registered X scaler; with g_t[d] the derivative of its forward transform at the raw input (the factors scfgp_predict_grad applies),
 * m_t -> g_t o m_t and Sigma_t -> diag(g_t) Sigma_t diag(g_t).  There is no raw-y mode: through a non-affine y scaler the gradient is
 * not Gaussian (the argument of SCFGP.predict_cov).
 * Active-subspace matrix of the call's rows, with optional weights w_t >= 0 (w == NULL: all 1):
 *     asub = sum_t w_t (m_t m_t^T + Sigma_t) / sum_t w_t  (D x D) = E[grad f grad f^T] averaged over the rows.
 * Outputs, each may be NULL, at least one must be given: dmu (T x D), dvar (T x D, the diagonal of Sigma_t), dcov (T x D x D), asub
 * (D x D).  w is read only when asub is given.
 * Limit: min(D, S) <= 64 -- a point's q derivative rows lie in one 64-row group of the block kernel, as scfgp_loo's block <= 64.
 * Chunks: the rows go through in chunks of np points,
 *     np = floor(32768 / gs) (64 / q)   with gs = (64 / q) q  (integer divisions; whole groups of 64 / q points in the 32 768-row buffers)
 * and, when dcov or asub is wanted (a D x D array per point: a dcov slot, the records of asub), np = min(np, max(1, floor(64 MiB /
 * (8 D^2)))).  HipEngine.gradcov_points_per_chunk(want_cov) returns it.
 * Promises:
 *  1. dmu is scfgp_predict_grad's dmu of the same mode, bit for bit.
 *  2. A point's dvar / dcov depend on that point alone: not on T, its position or the chunk.
 *  3. dcov[t] is symmetric bit for bit and dvar[t][d] == dcov[t][d][d] bit for bit (the lower triangle is computed, the upper is its
 *     mirror).
 *  4. asub is symmetric bit for bit.
 *  5. The sums of asub are added in row order in fp64, one summation order per entry, continued across chunks: the same bits on every
 *     run; rows of weight 0 behind the last weighted row do not change them.
 *  6. SCFGP_F16X3 contexts agree with SCFGP_F32 bit for bit (none of these products uses the split).  C' runs in the context's
 *     precision; H_t is formed by fp64 MFMA and everything after it is fp64.
 *  7. Device memory does not grow with T.
 * SCFGP_EARG (with a scfgp_last_error text, before any output is written) for bad pointers, T < 1, a bad mode, no output, a missing X
 * scaler in mode 1, parameters not set, a negative or non-finite weight, sum w = 0, or min(D, S) > 64. */
int scfgp_predict_gradcov(scfgp_ctx* ctx, const double* Xs, int64_t T, const double* w, const double* alpha, const double* Li, int mode,
                          double* dmu, double* dvar, double* dcov, double* asub);

/* ---- partial dependence and ICE curves of single inputs over a pool (no reference counterpart) ------------------------------------------
 * Which inputs matter, and how?  Pool rows x_t (t < T), weights w_t >= 0 (w == NULL: all 1), W = sum w_t, a dimension d and grid values
 * g_0 .. g_{G-1} of that dimension; x_t^{d->g} is row t with coordinate d replaced by g.
 *     ice[t][i] = mu*(x_t^{d->g_i})                       the individual conditional expectation (ICE) curves
 *     pd[i]     = sum_t (w_t / W) f(x_t^{d->g_i})         the partial-dependence (PD) curve, a linear functional of f: exactly Gaussian
 * A phase is linear in x: z_j = sum_e x_e F_all[e][j] + b_j.  With the zeroed-column features phi0_t = phi(x_t^{d->0}) (phase z_tj -
 * x_td F_all[d][j]), c_ij = cos(g_i F_all[d][j]) and s_ij = sin(g_i F_all[d][j]), the features of x_t^{d->g_i} are phi0_t rotated pair by pair:
 *     phi_c = phi0_c c_ij - phi0_s s_ij        phi_s = phi0_s c_ij + phi0_c s_ij
 * so with alpha = (J cosine weights | J sine weights)
 *     ice[t][i] = sum_k Phi0[t][k] R[k][i],   R[j][i] = alpha_j c_ij + alpha_{J+j} s_ij,   R[J+j][i] = alpha_{J+j} c_ij - alpha_j s_ij
 *     Phibar[i] = the same rotation of the mean row phibar0 = sum_t (w_t / W) phi0_t  (K numbers per dimension, whatever T is)
 *     pd[i] = Phibar[i] . alpha      pd_cov[i][i'] = kappa Phibar[i]^T A^-1 Phibar[i'] = kappa (Cbar Cbar^T)[i][i'],  Cbar = Phibar Li^T
 *     pd_sd[i] = sqrt(kappa |Cbar[i]|^2)
 * pd_sd and pd_cov describe the latent function: a PD curve is not an observation, so there is no noise term.
 * dims: ndim distinct dimensions in [0, D); grid (ndim x G): row a holds the grid values of dimension dims[a].  Outputs, each may be NULL,
 * at least one must be given: pd (ndim x G), pd_sd (ndim x G), pd_cov (ndim x G x G), ice (ndim x T x G).  All values are in scaled y
 * units.  mode 0: scaled rows and scaled grid values.  mode 1: column-selected raw rows through the registered X scaler, as
 * scfgp_predict_raw; the grid is given in raw units of its column and goes through the same per-column forward transform on the device.
 * There is no raw-y mode: the y scaler's backward transform is not affine, so a PD curve in raw y units is not Gaussian (the argument of
 * scfgp_predict_cov and scfgp_acquire).
 * Bounds: 1 <= G <= 1024 (the ICE block is the product of scfgp_sample), 1 <= ndim <= D, T >= 1 without limit.
 * A grid value is a coordinate like a row's own and is not refused for its size: the curves rotate by g_i F_all[d][j] through the feature
 * map's sin / cos (csrc/sincos.h), so they are right for |g_i F_all[d][j]| < 3.37e9 (2^31 pi/2) and carry a wrong quadrant beyond, as a
 * row's own phase would.
 * Rows with w_t == 0 contribute nothing to the sums: their term is selected away, not multiplied by zero, so a non-finite row of weight 0
 * is not an error.  They still get their ice rows.
 * How it runs.  The rows go through in chunks of 32768, at most twice: once for the sums (pd, pd_sd or pd_cov wanted), once for ice.  The
 * sums kernel forms Z = X~ F_all by fp64 MFMA as the feature map does and, in place of its store, sums w_t phi0_t over each 128-row block
 * for every dimension; Phi0 is never written.  A launch covers as many dimensions as keep its block records within 64 MiB.  ice stages two
 * T_chunk x G blocks, pd_cov two G x G blocks; device memory beside the chunk buffers does not grow with T.
 * Promises:
 *  1. The same call gives the same bits on every run: no atomics.  Within a 128-row block (aligned to the call-wide row index; 128 divides
 *     the chunk) the sum runs over a fixed tree: a lane's 8 rows, the 4 lanes of a column, the 4 waves of a column.  The block records are
 *     then added in row order into running fp64 sums that stay on the device across chunks.
 *  2. pd, pd_sd and pd_cov of a dimension do not depend on which other dimensions are in dims, nor on their order.
 *  3. pd[a][i], pd_sd[a][i] and ice[a][t][i] depend on g_i alone among the grid values: a shorter or permuted grid gives the matching
 *     entries.  An entry of pd_cov depends on its two grid values alone.
 *  4. pd_cov[a] is symmetric bit for bit (scfgp_predict_cov's promise: the same kernel with both operands equal).
 *  5. ice[a][t][:] depends on row t, the dimension, the grid, the factors and the parameters only: not on T, the row's position, the chunk
 *     or w.
 *  6. Appending rows with w = 0 changes no bit of pd, pd_sd or pd_cov.
 *  7. Every combination of requested outputs gives the same bits for the outputs it shares with another: pd never takes a shortcut
 *     through ice.
 *  8. SCFGP_F16X3 contexts run fp32 mode's kernels and agree with an SCFGP_F32 context bit for bit.
 * The training state of the context survives the call.
 * SCFGP_EARG (with a scfgp_last_error text, before any device work) for NULL Xs, alpha, Li, dims or grid, all four outputs NULL, T, G or
 * ndim out of range, a dimension out of range or given twice, a bad mode, a missing X scaler in mode 1, parameters not set, a negative w,
 * or no row with w > 0.  SCFGP_ENONFINITE for a non-finite w, a non-finite grid value (after the transform in mode 1) or a non-finite
 * weighted sum.  The outputs are untouched in both cases and the context stays usable. */
int scfgp_predict_pd(scfgp_ctx* ctx, const double* Xs, int64_t T, const double* w, const double* alpha, const double* Li,
                     const int* dims, int ndim, const double* grid, int G, int mode,
                     double* pd, double* pd_sd, double* pd_cov, double* ice);

/* ---- closed-form Sobol indices under a product measure (no reference counterpart) ----------------------------------------------------
 * The variance-based answer to "which inputs matter": the variance V of a sample function under a stated input distribution, the
 * main-effect variances Vmain[d] = Var(E[f | x_d]) and the total-effect variances Vtot[d] = E[Var(f | x_-d)]; S_d = Vmain[d] / V and
 * T_d = Vtot[d] / V are the first-order and total Sobol indices.  A phase is linear in x, so with phi(x) = s [cos z | sin z], z_j = sum_e
 * x_e Om[e][j] + b_j (Om: rows 0..D-1 of F_all, b: its row D; J = S + M) and a_j = s (w_j - i w_{J+j}) a sample function is f(x) = Re sum_j
 * a_j e^{i z_j(x)}, and under a product measure mu = prod_d mu_d over the SCALED inputs with characteristic functions psi_d(om) = E e^{i om x}
 *     kind 0, uniform on [p0, p1]:   psi(om) = e^{i om (p0 + p1) / 2} sinc(om (p1 - p0) / 2)     (p0 == p1: a point mass)
 *     kind 1, normal(p0, p1^2):       psi(om) = e^{i om p0 - (om p1)^2 / 2}                         (exactly 0 from |om| p1 of about 39 on)
 * every moment factorises over the inputs: no pool, no row sweep, no Monte-Carlo error.  With psi1[d][j] = psi_d(Om[d][j]), E_j = e^{i b_j}
 * prod_d psi1[d][j], E_j^{-d} the same product without factor d and, for a pair (j, k) and a sign (conjugation (+-) follows the sign),
 *     P+-_all       = e^{i(b_j +- b_k)} prod_e psi_e(Om[e][j] +- Om[e][k])
 *     P+-_main(d)   = E_j^{-d} (E_k^{-d})^(+-) psi_d(Om[d][j] +- Om[d][k])
 *     P+-_closed(d) = e^{i(b_j +- b_k)} psi1[d][j] (psi1[d][k])^(+-) prod_{e != d} psi_e(Om[e][j] +- Om[e][k])
 * the centred coefficients are C+-_u = P+-_u - E_j E_k^(+-), the centred form is Q_u(w) = 1/2 Re sum_{j,k} [a_j a_k C+_u + a_j conj(a_k)
 * C-_u], and f0 = Re sum_j a_j E_j, V = Q_all, Vmain[d] = Q_main(d), Vtot[d] = V - Q_closed(d), phibar = s (Re E | Im E) = E_mu phi(x) in
 * alpha's layout (f0 = phibar^T w; Bayesian quadrature: int f dmu ~ N(phibar^T alpha, kappa |Li phibar|^2)).  The difference is taken per
 * coefficient, never as w^T M w - f0^2, so f0^2 >> V does not cancel; a leave-one-out product is a prefix times a suffix, never a
 * quotient, so a factor that is exactly 0 is harmless.
 * kind (D entries, NULL: all uniform), p0, p1 (D each); W (K x nw, row-major: what scfgp_sample_weights returns, or any K-vectors; nw = 1
 * with W = alpha gives the posterior mean), 1 <= nw <= 1024; f0, V (nw each), Vmain, Vtot (nw x D, row-major), phibar (K).  Any output
 * may be NULL, at least one must be given; a NULL Vtot skips the closed-set work, a NULL Vmain the main-effect work, f0 and phibar alone
 * run no pair work at all; W may be NULL (and nw is then ignored) when only phibar is asked for.  The variances are returned, not the
 * ratios: V may be 0.  Everything is fp64 in every context (the K x K stage convention, as in scfgp_forget) and uses the context's current
 * parameters only: no alpha, no Li, no rows, no scaler; the training state of the context survives.  D is not limited: the pair kernel
 * takes the inputs in groups of 16 (option test_sobol_group can only lower that) and re-evaluates psi outside the group.
 * Promises, bit for bit: (1) the same outputs on every run; (2) column w of every output depends on W[:, w] and the parameters only, not
 * on nw or on the other columns: a call with fewer columns returns a prefix; (3) every output is the same whichever other outputs are
 * asked for; (4) contexts of all three compute modes agree (F_all and the scalars are formed by the same fp64 kernels in each); (5) the
 * group size does not change any output.
 * SCFGP_EARG (with a scfgp_last_error text "sobol: ...", before any device work, in this order) for a NULL p0 or p1; no output asked for;
 * W == NULL while f0, V, Vmain or Vtot is wanted; nw out of range (when W is used); a kind outside {0, 1}; p1 < p0 on a uniform input or
 * p1 < 0 on a normal one (the text names the first such input); parameters not set.  SCFGP_ENONFINITE for a non-finite p0, p1 or W.  The
 * outputs are untouched in both cases.
 * The domain of the measure.  Every phase goes through the feature map's sin / cos (csrc/sincos.h), which is exact to 0.77 * 2^-53 for
 * |z| < 2^31 pi/2 = 3.37e9 and returns finite values with the wrong quadrant beyond.  The pair coefficients evaluate psi_d at Om[d][j] +-
 * Om[d][k], twice the frequencies of the feature map, so the phases of input d reach
 *     R_d = 2 max_j |Om[d][j]| (|p0 + p1| / 2 + (p1 - p0) / 2)  on a uniform input (the sinc takes a sine at (Om_j +- Om_k) (p1 - p0) / 2),
 *     R_d = 2 max_j |Om[d][j]| |p0|                             on a normal one (its amplitude takes no sin / cos).
 * A call with any R_d >= 3.37e9 is refused: SCFGP_EARG, "sobol: input d: the measure's phases leave the sin/cos domain (2 max|Om| |x| <
 * 3.37e9)", naming the first such input (an index into the SCALED inputs, the d of kind, p0, p1), behind the refusals above and one small
 * kernel that reads max_j |Om[d][j]| back, before any table, pair or output; it does not depend on which outputs are asked for.  An
 * input whose frequencies are all zero passes whatever its measure; finite bounds of the order of DBL_MAX are refused wherever a
 * frequency is not zero, they do not overflow.  Inside the domain the refusal changes no bit.
 * Out of scope: second-order and higher interaction indices, empirical marginals, dependent inputs, raw-y units, a row-sharded form
 * (there are no rows), weights kept on the device between calls, and pair phases formed as products of table values, which would widen
 * the domain to the feature map's. */
int scfgp_sobol(scfgp_ctx* ctx, const int32_t* kind, const double* p0, const double* p1, const double* W, int nw,
                double* f0, double* V, double* Vmain, double* Vtot, double* phibar);

/* ---- greedy maximum-information choice of m rows from a pool (no reference counterpart) ----------------------------------------------
 * Which rows should be observed next?  The posterior of a Fourier-feature model is a Bayesian linear model in K weights, and the
 * posterior variance after an observation does not depend on the observed value, so the exact greedy batch needs neither targets nor
 * a refit per pick.  With Li of a fit, kappa = softplus(c), pool rows Xc (T x D), C = Phi_c Li^T (T x K) and d_i^(0) = |c_i|^2
 * (scfgp_predict_cov's diagonal divided by kappa), step j = 0 .. m-1 does
 *     p_j = argmax over the rows not yet taken with w_i > 0 of  w_i d_i^(j)                 (ties: the lowest index)
 *     t   = c_p - sum_{l<j} u_l (u_l . c_p)        dp = c_p . t        u_j = t / sqrt(1 + dp)
 *     d_i^(j+1) = max(d_i^(j) - (c_i . u_j)^2, 0)   for every i
 * kappa d_i^(j) is the posterior variance of f(x_i) given noisy observations (noise variance kappa, as scfgp_predict) at p_0 .. p_{j-1}:
 * (I + C_S^T C_S)^-1 = I - sum_l u_l u_l^T by Sherman-Morrison, one rank per pick.  sqrt(kappa (1 + d_i^(m))) is exactly what
 * scfgp_predict returns as std after scfgp_condition has absorbed the picked rows, whatever their targets are, and
 * sum_j log1p(dp_j) / 2 = log det(I + C_S C_S^T) / 2 is the information gain of the batch, of which the greedy choice is a (1 - 1/e)
 * maximiser (submodularity).
 * Xc (T x D): the pool; mode 0: scaled rows (as scfgp_predict), 1: column-selected raw rows through the registered X scaler (as
 * scfgp_predict_raw).  w (T, may be NULL = ones): non-negative weights of the criterion; w_i = 0 excludes row i from being picked (its
 * std_after is still reported).  Li as scfgp_eval returns it (entries above the diagonal are not read); alpha is not needed.  Points that
 * are pending (chosen, not yet observed) are handled by conditioning on them first with ANY targets (scfgp_condition): only Li' is used.
 * Outputs: idx (m): the picks in order, indices into the pool; var (m, may be NULL): kappa dp_j, the posterior variance of f at pick j
 * when it was picked; gain (m, may be NULL): log1p(dp_j) / 2; std_after (T, may be NULL): sqrt(kappa (1 + d_i^(m))) of every pool row.
 * Bounds: 1 <= m <= min(4096, number of rows with w_i > 0), 1 <= T <= 2^20, K <= 8192 (u_j is held in LDS).  The call owns a T x Kp
 * buffer of C in the context's type for its duration (a failed allocation is SCFGP_EHIP with the size in the message) and m x Kp
 * doubles of the u_l; nothing stays resident between calls.
 * Guarantees: the picks of a call with m1 < m2 are a prefix of those with m2, bit for bit, in idx, var and gain (step j does the same
 * arithmetic whatever m is).  A row's c_i . u has one summation order whatever T is and wherever the row sits, so appending rows with
 * w = 0 changes nothing and std_after of the original rows keeps its bits.  C runs in the context's precision (SCFGP_F16X3 contexts run
 * fp32 mode's kernels and agree with it bit for bit); d, t, dp, u and every sum over k are fp64, C is converted on load.  No step
 * returns to the host: m picks are eager launches on the context's stream, fetched once at the end.  The training state of the context
 * survives (resident rows, exchange buffers, optimiser state, precision level).
 * SCFGP_EARG (with a scfgp_last_error text, before any device work) for NULL pointers, a bad m, T or mode, a missing X scaler in mode 1,
 * parameters not set, a negative weight, or fewer than m rows with a positive weight; SCFGP_ENONFINITE for non-finite rows, weights or
 * factors: the outputs are untouched in both cases.  Integrated-variance criteria (ALC / A-optimal): scfgp_select_iv.  Out of scope: a row-sharded pool,
 * raw-y units (the criterion is in scaled-y units), and factors kept on the device between calls. */
int scfgp_select(scfgp_ctx* ctx, const double* Xc, int64_t T, const double* w, const double* Li, int m, int mode, int64_t* idx,
                 double* var, double* gain, double* std_after);

/* ---- greedy choice of m pool rows by integrated variance reduction (ALC / A-optimal; no reference counterpart) -------------------------
 * scfgp_select asks where the model is most uncertain; this entry point asks which observation most reduces the uncertainty WHERE THE
 * MODEL WILL BE USED: a reference set Xr (R x D) with non-negative weights omega.  Notation as scfgp_select: C = Phi_c Li^T of the pool,
 * d_i = |c_i|^2, u_l the Sherman-Morrison directions of the picks so far, P = I - sum_{l<j} u_l u_l^T.  With C_R = Phi_r Li^T,
 * Q = C_R^T diag(omega) C_R (K x K, symmetric positive semi-definite, formed once) and a_i = c_i^T P Q P c_i, observing pool row i with
 * noise kappa lowers sum_r omega_r Var[f(x_r)] by kappa a_i / (1 + d_i), and the integrated variance itself is kappa tr(P Q).  Step j:
 *     p_j = argmax over the rows not yet taken with w_i > 0 of  w_i a_i / (1 + d_i)           (ties: the lowest index)
 *     t, dp, u_j exactly as scfgp_select
 *     h = Q u_j       q = u_j . h                       (q = a_p / (1 + d_p): the reduction achieved, in units of kappa)
 *     g = h - sum_{l<j} u_l (u_l . h)                   (= P Q u_j, with P from before this pick)
 *     v = g - (q / 2) u_j
 *     for every i:  s_i = c_i . u_j,  z_i = c_i . v,   a_i <- max(a_i - 2 s_i z_i, 0),   d_i <- max(d_i - s_i^2, 0)
 * from a_i^(0) = c_i^T Q c_i, d_i^(0) = |c_i|^2: with P' = P - u u^T, c^T P' Q P' c = a - 2 s (c . P Q u) + s^2 q = a - 2 s (c . v).
 * Xc, T, w, Li, m, mode, idx, var (= kappa dp_j) and std_after (= sqrt(kappa (1 + d_i^(m)))) mean what they mean in scfgp_select.  Xr
 * (R x D, same mode as Xc): the reference rows; Xr == NULL: the pool is its own reference (R is ignored; wr, if given, has T entries).
 * wr (may be NULL = ones): non-negative finite weights omega, at least one positive.  R >= 1 without limit: the reference rows go through
 * the chunk pipeline and only Q is kept.  Outputs: red (m, may be NULL): kappa q_j, the reduction of the integrated variance by pick j;
 * ivar (2 doubles, may be NULL): [0] kappa tr(Q), the integrated variance before the picks (noise excluded), [1] = [0] - sum_j red[j],
 * subtracted in pick order by one thread.
 * Bounds: 1 <= m <= min(4096, number of rows with w_i > 0), 1 <= T <= 2^20, K <= 4096 (u_j and v are held in LDS together).  The call
 * owns a T x Kp buffer of C in the context's type, Kp x Kp doubles of Q (and a copy in the context's type), (4 + Kp / 128) T doubles
 * per-row state and m x Kp doubles of the u_l for its duration; it shares scfgp_condition's Gram slabs.
 * Guarantees: the picks of a call with m1 < m2 are a prefix of those with m2, bit for bit, in idx, red and var.  With an explicit Xr,
 * appending pool rows of weight 0 changes no bit of idx, red, var, or std_after of the original rows: a_i, s_i and z_i depend on row i,
 * Kp and Q only (a_i^(0) is the sum of its Kp / 128 column-tile shares in tile order; s_i and z_i have scfgp_select's summation order).
 * With Xr == NULL the appended rows enter Q, so nothing is claimed.  C and the product C Q of the start values run in the context's
 * precision (SCFGP_F16X3 contexts run fp32 mode's kernels and agree with it bit for bit; the weights omega are rounded to fp32 by fp32
 * mode's Gram); Q is summed over the chunks in fp64, and a, d, h, g, v and every sum over k of the picks are fp64.  Nothing returns to
 * the host between picks.  The training state of the context survives.
 * SCFGP_EARG (with a scfgp_last_error text, before any device work) as scfgp_select, and for a negative wr, an all-zero wr, R < 1 with
 * Xr given, or K above the bound; SCFGP_ENONFINITE for non-finite rows, weights or factors: the outputs are untouched in both cases.
 * Out of scope: a row-sharded pool or reference, raw-y units, factors or Q kept on the device between calls, K above the LDS bound.
 * Continuous optimisation: the criterion itself has no gradient entry; candidates found by following sample functions off the pool
 * (scfgp_sample_grad) can be appended to Xc. */
int scfgp_select_iv(scfgp_ctx* ctx, const double* Xc, int64_t T, const double* w, const double* Xr, int64_t R, const double* wr,
                    const double* Li, int m, int mode, int64_t* idx, double* red, double* var, double* ivar, double* std_after);

/* ---- greedy Monte-Carlo batch expected improvement over a pool (q-EI; no reference counterpart) ------------------------------------------
 * scfgp_select_qei: which m pool rows should be tried together, for improvement over the incumbent?  A sample function of this model is a
 * function (K weights; the same seed gives the same functions on any rows), so joint draws over the whole pool are exact and cost one
 * product Phi* W: no T x T covariance is formed.  With F[t][s] = f_s(x_t) what scfgp_sample(Xc, .., nsamp, seed, mode, noise = 0) returns,
 * bit for bit, sgn = +1, or -1 when `minimize` is set, u_ts = sgn F[t][s] and b = sgn best + xi (scaled-y units, as scfgp_acquire), the
 * Monte-Carlo q-EI of a batch B is
 *     qEI(B) = (1 / nsamp) sum_s max( max_{t in B} u_ts - b, 0 )
 * It is monotone and submodular in B (each term is a max over a set), so the greedy batch is a (1 - 1/e) maximiser, the argument
 * scfgp_select rests on.  Row t is eligible iff w == NULL or w[t] > 0 (scfgp_sample_argmax's meaning and host-side checks).
 *     start      m_s = b; with pending rows Xp (np x D, same mode; np = 0: none, Xp may then be NULL): m_s = max(b, max_r sgn f_s(xp_r)), the
 *                maximum being what scfgp_sample_argmax on Xp returns in val (its product and merge kernels: scfgp_sample's bits)
 *     step j     score_t = (1 / nsamp) sum_s max(u_ts - m_s, 0)   for every row t
 *                p_j = the lowest eligible, not yet taken t at which score_t is largest (scfgp_sample_argmax's merge rule)
 *                gain[j] = score_{p_j}        m_s <- max(m_s, u_{p_j, s})
 * Pending rows (chosen, not yet observed) enter through their sampled values: the fantasy treatment of asynchronous optimisation.  When
 * every remaining score is 0 (no sample can still improve), the picks go to the lowest eligible untaken indices and their gain is 0;
 * that is not an error.
 * Outputs: idx (m): the picks in order, indices into the pool; gain (m, may be NULL); score0 (T, may be NULL): the scores of step 0 of
 * every row, eligible or not -- the Monte-Carlo one-point EI given the pending rows; mstate (nsamp, may be NULL): m after the last pick;
 * qei (2 doubles, may be NULL): [0] = (1 / nsamp) sum_s (m_s - b) at the start, the q-EI of the pending rows alone (0 without them), [1]
 * the same after the last pick, the q-EI of pending rows plus picks; each is added by one thread in sample order.
 * mode 0: scaled rows; 1: column-selected raw rows through the registered X scaler.  There is no raw-y mode (as scfgp_acquire) and no
 * noise argument (as scfgp_sample_argmax).
 * Bounds: 1 <= nsamp <= 1024, 1 <= m <= min(4096, number of eligible rows), 1 <= T <= 2^20, np >= 0 without limit (the pending rows go
 * through the chunk pipeline).  The call owns T x nsamp doubles of F for its duration (a failed allocation is SCFGP_EHIP with the size in
 * the message) and 2 T doubles of per-row state; nothing stays resident between calls.  Storing F costs 8 T nsamp bytes and makes a
 * pick one read of it; recomputing Phi* W instead would cost 2 T K nsamp flops per pick.
 * Guarantees: F is written by scfgp_sample's kernel and stays fp64 in every compute mode (SCFGP_F16X3 contexts run fp32 mode's kernels
 * and agree with it bit for bit).  A row's score depends on the row's F values, m and nsamp only -- not on T, the row's position, the
 * grid or w: a group of lanes whose width depends on nsamp alone (16 for nsamp <= 64, else 64) adds s = g, g + G, .. in ascending order,
 * a fixed xor butterfly follows, then one division by nsamp.  m is exact (max).  So the picks of m1 < m2 are a prefix, bit for bit, in
 * idx and gain; gain never increases; appending rows of weight 0, or duplicating the pool behind itself, changes nothing; and a later
 * call with the first picks passed as pending rows (and masked) continues the same sequence with the same bits.  No step returns to the
 * host: a pick is two eager launches on the context's stream; the host waits once after F is built (for the non-finite flag) and once
 * at the end.  The training state of the context survives.
 * SCFGP_EARG (with a scfgp_last_error text, before any device work) for NULL Xc, alpha, Li or idx, T, m, nsamp or mode out of range,
 * np < 0, np > 0 with NULL Xp, xi < 0, a missing X scaler in mode 1, parameters not set, a negative w, or fewer than m rows with a
 * positive w.  SCFGP_ENONFINITE for a non-finite best, xi or w (on the host, before any device work) and for a non-finite sampled value
 * of an eligible or pending row (found on the device); a non-finite row with w = 0 is not an error: its terms count as 0 in score0.
 * The outputs are untouched in every error case.
 * Out of scope: lazy-greedy pruning of the sweep, q-PI / q-UCB, gradients of q-EI in the inputs (continuous refinement goes through
 * scfgp_sample_grad), a row-sharded pool, raw-y units, and F, W or factors kept on the device between calls. */
int scfgp_select_qei(scfgp_ctx* ctx, const double* Xc, int64_t T, const double* w, const double* Xp, int64_t np,
                     const double* alpha, const double* Li, int nsamp, uint64_t seed, double best, double xi, int m, int mode,
                     int minimize, int64_t* idx, double* gain, double* score0, double* mstate, double* qei);

/* ---- staged evaluation for row-sharded data parallelism ---------------------------------
 * The objective needs three row sweeps separated by two K x K stages; with rows sharded
 * over ranks each sweep ends in one sum over ranks.  The host framework (torch.distributed
 * over RCCL) performs that sum in place on the device buffer scfgp_exchange() exposes:
 *
 *   scfgp_pass1   -> exchange 1 = [G, packed lower 128x128 tiles | Phi^T y (Kp) | y^T y ...]
 *   scfgp_factor     (replicated: Cholesky, Li, alpha, log det)
 *   scfgp_pass2   -> exchange 2 = [B W B = V^T diag(q) V, packed lower tiles | B Phi^T p = V^T p (Kp) | T2, kbar, sum q v, sum p mu ...]
 *                    (at precision level 2 of fp32 mode, scfgp_get_condition: [C^T diag(q) C | C^T p | ...], C = Phi Li^T --
 *                    still row sums, so the sum over ranks is the same operation)
 *   scfgp_adjoint    (replicated: Abar)                      [want_grad only]
 *   scfgp_pass3   -> exchange 3 = [X~^T Zbar | ...]          [want_grad only]  (d cost / d b is formed in closed form from the
 *                    summed exchanges 1 and 2: 2 tr(Abar G) + ut^T Phi^T y + 2 sum q v + sum p mu -- no row sweep, no slot here)
 *   scfgp_finish  -> outputs on the host
 *
 * These calls only enqueue work on the context's stream (asynchronous); scfgp_finish
 * synchronises.  scfgp_eval is exactly this sequence without the sums.
 *
 * Ranks decide together.  The last four of the 8 scalars that close every exchange buffer are a status word: each rank
 * writes 0 / 1 there, the sum over ranks turns them into COUNTS that every rank reads alike --
 *   [4] ranks whose pass 1 ran at precision level >= 1        [5] / [6] ranks that cannot reach level 1 / 2 (their row
 *   buffers were refused)            (exchange 1)             [7] ranks that failed in this sweep (exchanges 1, 2, 3).
 * After a precision level was raised (the decision comes from the summed matrix, so every rank tries in the same
 * evaluation) scfgp_factor reads the summed word once -- one stream synchronisation in that evaluation only -- and every
 * rank commits to the lowest level any rank can reach; if that changes the form of pass 1 on some rank, scfgp_factor
 * returns SCFGP_REDO on ALL ranks.  scfgp_get_condition()[1] then reports the common level, scfgp_last_error the refusal.
 * A rank whose sweep fails calls scfgp_fail_stage for that and every later exchange of the evaluation (stage 1..3; stage 3
 * only with want_grad): the buffer is marked, the sum still happens (inside the library with a communicator, else by the
 * host framework as usual), nobody waits in a collective for a rank that has left, and scfgp_finish returns SCFGP_EPEER on
 * every other rank.  scfgp_eval / scfgp_eval_rows / scfgp_train do this themselves when the sums run inside the library. */
int scfgp_pass1(scfgp_ctx* ctx);
int scfgp_factor(scfgp_ctx* ctx);
int scfgp_pass2(scfgp_ctx* ctx, int want_grad);
int scfgp_adjoint(scfgp_ctx* ctx);
int scfgp_pass3(scfgp_ctx* ctx);
int scfgp_finish(scfgp_ctx* ctx, int want_grad, double* cost, double* grad, double* alpha, double* Li);
int scfgp_fail_stage(scfgp_ctx* ctx, int stage, int want_grad);
/* optional, any time after scfgp_factor, best after the remaining stages are queued: copies alpha (K) and
 * Li (K*K) to the host on a second stream through pinned staging and returns once they are in the caller's
 * arrays.  It waits for the factor stage only, so the transfer and the host-side copy overlap passes 2 and 3
 * (then pass NULL for both to scfgp_finish). */
int scfgp_fetch_factors(scfgp_ctx* ctx, double* alpha, double* Li);
/* device pointer + length (in doubles) of exchange buffer `stage` (1..3) */
int scfgp_exchange(scfgp_ctx* ctx, int stage, void** dev_ptr, int64_t* count);
/* Ordering contract for the sums.  The library enqueues on ITS stream: the one handed to scfgp_create, or a
 * private one when that was NULL (torch's default stream is handle 0 == NULL, so a caller on torch's default
 * stream always gets a private library stream).  A collective issued by the host framework on another stream
 * must be fenced on both sides:
 *     scfgp_stream_fence(ctx, peer, 0)   peer waits for the library's queued work   (before the all-reduce)
 *     scfgp_stream_fence(ctx, peer, 1)   the library waits for peer's queued work   (after the all-reduce)
 * peer = the hipStream_t the collective runs on (NULL = legacy default stream).  Event based, asynchronous,
 * a no-op when peer is the library's own stream.  No reference counterpart (the reference is single-device). */
int scfgp_stream_fence(scfgp_ctx* ctx, void* peer_stream, int direction);

/* ---- the sums inside the library: RCCL all-reduce over xGMI (no reference counterpart: the reference is single-device) ----
 * One process per GPU.  Rank 0 calls scfgp_comm_unique_id and hands the 128 bytes to the other ranks by any means (MPI, a file,
 * torch.distributed.broadcast_object_list); every rank then calls scfgp_comm_init on its context (collective: ncclCommInitRank).
 * From then on the three sums of the row sums of SCFGP/SCFGP.py:104,108,126 and of the reverse sweep -- exchange buffers 1..3
 * above -- are ncclAllReduce(fp64, sum) calls the library enqueues itself on the context's stream at the end of scfgp_pass1 /
 * scfgp_pass2 / scfgp_pass3, so scfgp_eval and scfgp_eval_rows are complete sharded evaluations (set the rows of the rank with
 * scfgp_set_data(..., n_global = sum of the ranks' N)); the precision level is decided from the summed matrix and committed
 * through the status word above, alike on every rank.  scfgp_train runs its iterations with the three sums inside (every rank
 * applies the same deterministic rule to the same summed gradient: the parameter vectors stay bit-equal without a broadcast;
 * eager launches by default, the captured graph only with option "use_graph" = 2).  librccl.so is looked up at run time (a copy
 * the process already carries is reused, wherever it was loaded from): the library has no link-time dependency on it and
 * single-GPU users never load it.  A caller that prefers to run the sums in its own framework leaves the communicator out and
 * uses scfgp_exchange + scfgp_stream_fence as before.
 * STATUS: the communicator path has run on hardware with ONE rank only (the build pool hands out single GPUs); with two or
 * more ranks it is covered by construction and by the in-process / gloo rehearsals of the same protocol, not by a measurement. */
int scfgp_comm_unique_id(void* id128);
int scfgp_comm_init(scfgp_ctx* ctx, int nranks, int rank, const void* id128);
int scfgp_comm_destroy(scfgp_ctx* ctx);

/* ---- on-device update rule and multi-iteration residency -------------
 * The arithmetic of SCFGP/Optimizer.py as a device kernel behind the evaluation, so a training
 * iteration (SCFGP/SCFGP.py:237: train_iter_func) needs no host round trip; from the second
 * iteration on the whole iteration is ONE captured hipGraph launch.
 *   algo   0 sgd, 1 adagrad, 2 rmsprop, 3 adadelta, 4 adam, 5 adamax  (SCFGP/Optimizer.py:99-382)
 *   hyper  [learning_rate, beta1 (rho for rmsprop/adadelta), beta2, epsilon]
 *   momentum  Nesterov momentum as the reference applies it (SCFGP/Optimizer.py:62-97, on the FIRST
 *             state of the rule's update dictionary); negative = none
 * scfgp_train runs n_iters x (evaluate + update) on the resident rows (of this rank: see the communicator above), returns the cost
 * of every iteration (each at its pre-update parameters, like train_iter_func) and, if non-NULL,
 * alpha / Li of the LAST evaluation; the updated vector is read with scfgp_get_params.
 * scfgp_opt_state copies optimiser state to (set=0) or from (set=1) the host: which 0,1 = the rule's
 * two state vectors, 2 = Nesterov velocity (P doubles each), 3 = step counter (1 double). */
int scfgp_opt_init(scfgp_ctx* ctx, int algo, const double* hyper, int nhyper, double momentum);
int scfgp_opt_state(scfgp_ctx* ctx, int set, int which, double* buf);
/* one step of the device rule with a caller-supplied gradient (P doubles, host): parameters and state advance as inside
 * scfgp_train, no evaluation (for gradients formed elsewhere; the rule's known-answer tests drive it) */
int scfgp_opt_step(scfgp_ctx* ctx, const double* grad, int P);
int scfgp_train(scfgp_ctx* ctx, int n_iters, double* cost_hist, double* alpha, double* Li);

/* ---- conditioning and precision level (no reference counterpart) -----------------------------------
 * The reference computes in float64 throughout (SCFGP/SCFGP.py:95-96) and factors A = Phi^T Phi + (e^{2a}+1e-6) I
 * (SCFGP/SCFGP.py:104-107) whatever its conditioning.  In SCFGP_F32 mode the Gram products carry a
 * relative error of ~6e-8, which reaches alpha and Li multiplied by the condition of A (measured: about 3e-7 times the
 * estimate below).  The K x K stage therefore reports a condition estimate with every evaluation, and by default (option
 * "gram64" = 2, auto) the library raises the precision of the two Gram products when it is high:
 *   level 1 (estimate > 10):   pass 1 -- G and Phi^T y by the fp64 kernels from fp64 features; alpha and Li then equal fp64
 *                               mode's bit for bit, cost / mu* / sigma* to ~1e-8
 *   level 2 (estimate > 1000): also pass 2 in the reference's own factor form (SCFGP/SCFGP.py:112): C = Phi Li^T,
 *                               v = rowsum(C^2), V = C Li, all in fp32 MFMA; EXCHANGE BUFFER 2 THEN CARRIES C^T diag(q) C AND
 *                               C^T p (not B W B and u): the K x K stage forms B W B = Li^T (C^T diag(q) C) Li and
 *                               u = Li^T (C^T p) after the sum over ranks.  Rounding errors are amplified by sqrt(cond A)
 *                               instead of cond A (gradient blocks to ~1e-4)
 * "gram64" = 0 never (plain fp32: the caller reads out[3] to know what alpha is worth), 1 / 3 = always level 1 / 2.
 * out (n >= 4, up to 9 values): [0] condition estimate max_i L_ii^2 * max_j (A^-1)_jj of the last finished evaluation (a lower
 * bound of cond_2(A)), [1] level it ran at, [2] 1 if G was formed in fp64 from fp64 features, [3] predicted relative error
 * of alpha / Li for an fp32 Gram at this estimate, [4] / [5] thresholds of levels 1 / 2, [6..8] min L_ii^2, max L_ii^2,
 * max_j (A^-1)_jj. */
int scfgp_get_condition(scfgp_ctx* ctx, double* out, int n);

/* ---- introspection ------------------------------------------------------------------------ */
/* padded sizes the device buffers use: out[0]=K, out[1]=Kp, out[2]=Jp, out[3]=Dp, out[4]=Np, out[5]=P, out[6]=tile (n >= 7),
 * out[7]=rows made resident by scfgp_set_data, 0 without any (n >= 8) */
int scfgp_get_dims(scfgp_ctx* ctx, int64_t* out, int n);
/* profiling: enable per-stage hipEvent timing; after an evaluation read back up to n
 * (name, milliseconds) pairs.  Returns the number of stages recorded. */
int scfgp_set_profiling(scfgp_ctx* ctx, int enable);
int scfgp_get_timings(scfgp_ctx* ctx, double* ms, const char** names, int n);
/* copy an internal device buffer to the host for tests ("Phi","V","G","W","XZ","Li","B","Abar",
 * "p","q","vecs","Fall","Lall","Rall","Xt","Tt","scalars"); returns the number of bytes copied or <0.  "Lall" (Dp x round_up(Sp,64))
 * and "Rall" (Sp x Jp) are the factors of the rank-S projection, defined only where it runs (Sp < Dp).  "G" is exchange buffer 1 unpacked
 * (the summed Gram, Phi^T y, y^T y and the status word) at any stage; "W" is exchange buffer 2 as the adjoint stage left it.
 * "Xt" holds the resident training rows only; "pXt" is the packed chunk of the last posterior call (scfgp_predict* and the other
 * entry points that take test or pool rows): the rows of its last chunk after the X scaler, round_up(rows, 256) x Dp doubles with a
 * column of ones at d = D and zeros elsewhere in the padding; an error before the first such call.
 * Compute mode SCFGP_F16X3 only (elsewhere an error with a message): "Phi16", "V16g", "qV16g" the Np x Kp plane-form arrays of
 * Phi, V and diag(q) V (4 bytes per element, per 16 columns 16 fp16 h's then 16 l's; without the padding behind them); "B16"
 * the K x K operand of the apply products in plane form (Kp x Kp x 4 bytes, row j = column j); "f16scale" its 4 floats
 * (scale[0] = 2^-(e_Phi + e_operand), scale[1] = 2^e_operand); "f16tmp" the 8 floats of bounds and scales (0: bound of |Phi|,
 * 2..4: 2^-e, 2^-e_w and the Gram scale of the last split pass, 5: bound of |V|, 6: max |q| (1 + 1e-6)) */
int64_t scfgp_debug_read(scfgp_ctx* ctx, const char* name, void* host, int64_t max_bytes);
/* options (name, value):
 *   "gram_nsplit"  row-split units of the Gram products (0 = default)
 *   "gram_taper"   1: the last unit of every XCD group is cut into 1/2, 1/4, 1/8, 1/8; t >= 2: into t + 3 pieces down to 1/2^(t+2)
 *   "gram_chunk"   fp32 mode: rows between two flushes of the fp32 accumulators into the fp64 slabs (default 4096; f16x3 mode:
 *                  half the rows of a Gram job)
 *   "f16_gram"     f16x3 mode: 1 (default) the two Gram products on the fp16 pipe too, 0 keep fp32 mode's
 *   "xtz_nsplit"   row splits of X~^T Zbar (0 = default)
 *   "use_graph"    0: scfgp_train launches every iteration eagerly instead of replaying a captured hipGraph (1, default: the
 *                  graph unless a communicator is attached; 2: the graph with a communicator too)
 *   "apply_dma"    the tiles of the apply products staged by LDS-DMA (global_load_lds) instead of through registers:
 *                  -1 automatic (K > 256 and >= 16384 rows: 128-wide tiles; fp32 from K >= 1024 and 65536 rows: 256-wide), 0 off,
 *                  1 = 128-wide tiles, 2 = 256-wide tiles (fp32; fp64 stays 128 wide)
 *   "gram64"       precision level policy of fp32 mode (scfgp_get_condition): 0 never, 1 always level 1, 2 auto, 3 always level 2
 *   "cond_threshold" / "cond_threshold_w"   the two thresholds of the auto policy
 *   "factor_form"  -1 auto (= precision level 2), 0 never, 1 always: pass 2 as C = Phi Li^T, V = C Li
 *   "lowrank_bwd"  -1 auto (D+1 >= 4 (S+1), padded), 0 never, 1 whenever it can (the forward projection goes through the S
 *                  columns and U fits): the reverse sweep of F = l_F r_F^T through T~^T Zbar and X~^T (Zbar_L + Zbar_M r_F)
 *                  instead of the dense X~^T Zbar; exchange buffer 3 then holds those two
 *   "roctx"        1: push a roctx range per stage for `rocprofv3 --marker-trace` (off by default; also SCFGP_ROCTX=1)
 *   "test_deny_level" / "test_fail_stage"   fault injection for the tests of "ranks decide together": precision levels >= value
 *                  are refused as if their buffers could not be allocated / the next sweep `value` (1..3) fails before it enqueues
 * Experiments of earlier rounds that measured equal or slower (feature map fused into the Gram loaders, lock-step Gram
 * schedule, pass 3 in row parts on two streams, Zbar written by the Phibar product, 8-wave and hand-pipelined LDS-DMA
 * tiles, the bf16x3 split-precision dtype) are no longer part of the library: profiles/r02_tuning.md, r03_tuning.md hold
 * their measurements, git history (tag of round 3: commit 757ac97) their code. */
int scfgp_set_option(scfgp_ctx* ctx, const char* name, int64_t value);

/* Box probe (no reference counterpart; bench.py's `secondary.box`): ~100 ms of device work on `device`, no context needed.
 * out[0] = fp32 MFMA TFLOP/s of a register-only v_mfma_f32_16x16x4_f32 loop (best of 1, 2, 8 waves per SIMD; n >= 6: each
 * in out[3..5]), out[1] = shader clock it held (GHz), out[2] = GB/s of a 1 GiB -> 1 GiB streaming copy (read + write), n >= 7:
 * out[6] = GB/s of a read-only stream over the same 2 GiB (the ceiling of the sweeps that only read).
 * Lets two timings from two devices be normalised. */
int scfgp_box_probe(int device, double* out, int n);

/* host-only self-test of the row splits of the Gram products (how the N rows are cut into the splits whose partial
 * sums the reduction adds; `nsplit` 0 = default, `taper` as the option): returns 0 when the splits tile [0, Np) in
 * order on 256-row blocks.  Needs no GPU. */
int scfgp_selftest_row_splits(int D, int S, int M, int64_t N, int dtype, int nsplit, int taper);

#ifdef __cplusplus
}
#endif
#endif /* SCFGP_HIP_H */
