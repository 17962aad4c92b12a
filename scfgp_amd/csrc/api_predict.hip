// C ABI of libscfgp_hip.so, the predict family: scfgp_predict, _raw, _y, _grad and the scaler setters, scfgp_predict_cov,
// scfgp_predict_gradcov, scfgp_predict_pd and scfgp_sobol.
#include "api_chunks.h"

// chunk bodies of this file's entry points; those that other files call too are ChunkImpl's (api_chunks.h)
template <typename T> struct PredictImpl : ChunkImpl<T> {
    typedef SweepKernels<T> SK;
    using ChunkImpl<T>::features;
    static void cov_panel(scfgp_ctx* c, const void* Ca, const void* Cb, int64_t nrows, int64_t Tb, int64_t row_base, int noise, double* out) {
        predcov<T>(c->g, (const T*)Ca, (const T*)Cb, nrows, Tb, row_base, noise, c->d_sc, out, c->st);
    }
    // scfgp_predict_gradcov (gradcov.hip).  Qt: the typed direction basis, once per call
    static void gradcov_basis(scfgp_ctx* c, void* Qt) { gradcov_operand<T>(c->g, c->d_params, c->d_Fall, (T*)Qt, c->st); }
    // a chunk of g.N points: dmu by predict_grad's own kernel (mean only) and chain rule, so that it has scfgp_predict_grad's bits; then
    // the g.N q derivative rows Psi into p_V, C' = Psi Li^T into p_C (its by-products land in the chunk's partials and are ignored), the
    // block kernel and, rec != NULL, the ordered sum of its records.  x: the chunk's raw rows (xmode != 0: gfac <- the scaler's factors)
    static int gradcov_chunk(scfgp_ctx* c, const Geom& g, const void* LiT, const void* Qt, const double* x, int xmode, double* gfac,
                             const double* wgt, double* dmu, double* dvar, double* dcov, double* rec, double* acc) {
        const int q = std::min(g.D, g.S);
        features(c, g);
        { ProfScope ps(c, "gradcov_dmu");
          predgrad<T>(g, (const T*)c->p_Phi, (const T*)c->p_V, c->alpha_pred(), (const T*)c->p_FT, nullptr, c->d_sc, dmu, nullptr, c->st);
          if (xmode) {
              gradcov_ones(gfac, g.N * g.D, c->st);
              xgrad_chunk(x, g.N, g.D, xmode, c->d_xscale, dmu, gfac, c->st);
          } }
        if (dvar || dcov || rec) {
            const Geom gr = chunk_geom(g, g.N * q);
            { ProfScope ps(c, "gradfeat"); gradfeat<T>(gr, g, (const T*)c->p_Phi, (const T*)Qt, (T*)c->p_V, c->st); }
            { ProfScope ps(c, "gradcov_apply_c");
              SK::apply_c(gr, (const T*)c->p_V, (const T*)LiT, (const T*)c->p_Li, (T*)c->p_C, c->p_vpart, c->alpha_pred(), c->alpha_pred(),
                          c->p_mupart, c->st, 0); }
            { ProfScope ps(c, "gradcov_block");
              gradcov_blocks<T>(gr, g, (const T*)c->p_C, c->d_params, c->d_sc, xmode ? gfac : nullptr, dmu, wgt, dvar, dcov, rec, c->st); }
            if (rec) { ProfScope ps(c, "gradcov_reduce"); gradcov_reduce(rec, g.N, g.D, acc, c->st); }
        }
        HIPCHK(c, hipGetLastError());
        return SCFGP_OK;
    }
    // scfgp_predict_pd (pd.hip).  The sums of a chunk's packed rows for ng dimensions, added into the call's running sums
    static int pd_sums_chunk(scfgp_ctx* c, const Geom& g, const double* wgt, const int* dims, int ng, double* rec, double* acc) {
        ProfScope ps(c, "pd_sums");
        pd_sums<T>(g, c->p_Xt, c->d_Fall, c->d_sc, wgt, dims, ng, rec, acc, c->st);
        HIPCHK(c, hipGetLastError());
        return SCFGP_OK;
    }
    // the curves of ng dimensions: their stacked mean rows Phibar into p_Phi (gr: the geometry in those rows), Cbar = Phibar Li^T into p_C;
    // pd = the sum of mupart in rowpredict's order, sd = sqrt(kappa sum vpart) by kg_sigma's arithmetic.  pd, scratch, sd: gr.Np each
    static int pd_curves(scfgp_ctx* c, const Geom& gr, const void* LiT, const double* acc, double W, const int* dims, const double* grid, int ng,
                         int G, double* pd, double* scratch, double* sd) {
        ProfScope ps(c, "pd_curves");
        pd_mean_rows<T>(gr, c->g, acc, W, c->d_Fall, dims, grid, ng, G, (T*)c->p_Phi, c->st);
        SK::apply_c(gr, (const T*)c->p_Phi, (const T*)LiT, (const T*)c->p_Li, (T*)c->p_C, c->p_vpart, c->alpha_pred(), c->alpha_pred(),
                    c->p_mupart, c->st, 0);
        SK::rowpredict(gr, c->p_mupart, c->p_vpart, c->d_sc, pd, scratch, c->st);
        kg_sigma(gr, ApplyKernels<T>::partials(gr), c->p_vpart, c->d_sc, 0, sd, c->st);
        HIPCHK(c, hipGetLastError());
        return SCFGP_OK;
    }
    // the covariance of dimension number a of the last pd_curves: predcov on its own rows of p_C twice, so the result is symmetric bit for bit
    static int pd_cov_dim(scfgp_ctx* c, int a, int G, double* out) {
        const T* Ca = (const T*)c->p_C + (int64_t)a * pd_grid_rows(G) * c->g.Kp;
        predcov<T>(c->g, Ca, Ca, G, G, 0, 0, c->d_sc, out, c->st);
        HIPCHK(c, hipGetLastError());
        return SCFGP_OK;
    }
    // the ICE block of dimension d over the chunk's packed rows: column d of p_Xt is cleared for the feature map and put back
    static int pd_ice_chunk(scfgp_ctx* c, const Geom& g, int d, const double* grid_d, int G, void* R, double* keep, double* out) {
        pd_column(g, c->p_Xt, d, 1, keep, c->st);
        { ProfScope ps(c, "pd_ice_featuremap"); features(c, g); }
        { ProfScope ps(c, "pd_ice_product");
          pd_ice_weights<T>(c->g, c->alpha_pred(), c->d_Fall, d, grid_d, G, (T*)R, c->st);
          sample_product<T>(g, (const T*)c->p_Phi, (const T*)R, G, 0, 0, 0, -1, c->d_yscale, c->d_sc, out, c->st); }
        pd_column(g, c->p_Xt, d, 0, keep, c->st);
        HIPCHK(c, hipGetLastError());
        return SCFGP_OK;
    }
};
#define DISPATCH(c, fn, ...) DISPATCH_TO(PredictImpl, c, fn, __VA_ARGS__)

// raw_mode: apply the registered X scaler while packing; post: y-scaler backward transform of the outputs on
// the device and, with targets ys, the six validation metrics; dmu != NULL: also the gradients of mu (and, dstd != NULL, of std) in
// the inputs, T x D each (scfgp_predict_grad).  mu and sd of all T rows stay on the device until the end.
static int predict_impl(scfgp_ctx* c, const double* Xs, int64_t T, const double* alpha, const double* Li,
                        double* mu, double* sd, int raw_mode, int post = 0, const double* ys = nullptr,
                        double* metrics = nullptr, double* dmu = nullptr, double* dstd = nullptr) {
    if (!c || !Xs || !alpha || !Li || !mu || !sd || T < 1) { if (c) c->err = "predict: bad arguments"; return SCFGP_EARG; }
    int rc;
    if ((rc = need_model({c, "predict"}, false))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const Geom& g0 = c->g;
    if ((rc = ensure_pred_chunk(c))) return rc;
    const bool grad = dmu != nullptr;
    if (grad && (rc = ensure_pred_grad(c, dstd != nullptr))) return rc;
    RowFeed feed; DevTmp d_out, d_ys, d_part;                     // Li / two chunks of Xs | mu, sd of all T rows | targets, mean, metrics | chunk partials
    if ((rc = feed.open(c, PRED_ROWS * g0.D, (int64_t)g0.K * g0.K))) return rc;
    if ((rc = dmalloc(c, &d_out.p, sizeof(double) * 2 * T))) return rc;
    double* d_mu = d_out; double* d_sd = d_out + T;
    // the sweep operand is Li^T itself: sigma* needs rowsum((Phi* Li^T)^2) (SCFGP/SCFGP.py:144), a triangular product
    const void* LiT;
    if ((rc = load_factor(c, feed, Li, pad_square, false, alpha, &LiT))) return rc;
    DevTmp d_grad;                                                // dmu | dstd of all T rows (T x D each)
    if (grad) {
        if ((rc = dmalloc(c, &d_grad.p, sizeof(double) * T * g0.D * (dstd ? 2 : 1)))) return rc;
        DISPATCH(c, grad_operand, c);
        if (dstd) DISPATCH(c, type_factor, c, c->d_T1, nullptr, c->p_Li);      // p_Li exists with the std gradient only
    }
    double* d_dmu = d_grad; double* d_dsd = grad && dstd ? d_grad + T * g0.D : nullptr;
    HIPCHK(c, hipStreamSynchronize(c->st));                     // raw is reused below
    const RowJobs jobs = {Xs, nullptr, T, PRED_ROWS};
    const int nchunks = (int)jobs.count();
    if (post && ys) {
        if ((rc = dmalloc(c, &d_ys.p, sizeof(double) * (T + 8)))) return rc;
        if ((rc = dmalloc(c, &d_part.p, sizeof(double) * 4 * YPOST_BLOCKS * nchunks))) return rc;
        HIPCHK(c, hipMemcpyAsync(d_ys, ys, sizeof(double) * T, hipMemcpyHostToDevice, c->st));
        ypost_mean(d_ys, T, d_ys + T, c->st);
    }
    if ((rc = feed.upload(0, jobs))) return rc;
    for (int64_t i = 0; i < nchunks; ++i) {
        const int64_t t0 = jobs.row0(i);
        const Geom g = chunk_geom(g0, jobs.rows(i));
        const double* x;
        if ((rc = feed.acquire(i, &x))) return rc;
        pack_chunk(c, g, x, nullptr, nullptr, nullptr, raw_mode ? c->xs_mode : 0, c->d_xscale);
        if (!grad && (rc = feed.release(i))) return rc;
        if ((rc = DISPATCH(c, predict_chunk, c, g, LiT, d_mu + t0, d_sd + t0))) return rc;
        if (grad) {
            // the gradients in x~, then the scalers' chain rules: the X scaler's at the raw inputs (still in the feed's half: it is
            // released after them), the y scaler's at the scaled mu, sigma (before ypost_chunk transforms them in place)
            double* gm = d_dmu + t0 * g0.D; double* gs = d_dsd ? d_dsd + t0 * g0.D : nullptr;
            if ((rc = DISPATCH(c, predict_grad_chunk, c, g, LiT, d_sd + t0, gm, gs))) return rc;
            if (raw_mode && c->xs_mode) xgrad_chunk(x, g.N, g0.D, c->xs_mode, c->d_xscale, gm, gs, c->st);
            if (post) ygrad_chunk(d_mu + t0, d_sd + t0, g.N, g0.D, c->ys_mode, c->d_yscale, gm, gs, c->st);
            if ((rc = feed.release(i))) return rc;
        }
        if (post)
            ypost_chunk(d_mu + t0, d_sd + t0, d_ys.p ? d_ys + t0 : nullptr, g.N, c->ys_mode, c->d_yscale, d_ys.p ? d_ys + T : nullptr,
                        d_part.p ? d_part + 4 * YPOST_BLOCKS * i : nullptr, c->st);
        if (i + 1 < nchunks && (rc = feed.upload(i + 1, jobs))) return rc;
    }
    HIPCHK(c, hipMemcpyAsync(mu, d_mu, sizeof(double) * T, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(sd, d_sd, sizeof(double) * T, hipMemcpyDeviceToHost, c->st));
    if (grad) HIPCHK(c, hipMemcpyAsync(dmu, d_dmu, sizeof(double) * T * g0.D, hipMemcpyDeviceToHost, c->st));
    if (grad && dstd) HIPCHK(c, hipMemcpyAsync(dstd, d_dsd, sizeof(double) * T * g0.D, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (post && ys) {
        ypost_metrics(d_part, YPOST_BLOCKS * nchunks, T, d_ys + T + 1, c->st);
        HIPCHK(c, hipMemcpyAsync(metrics, d_ys + T + 1, sizeof(double) * 6, hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipStreamSynchronize(c->st));
    }
    HIPCHK(c, hipGetLastError());
    return SCFGP_OK;
}

extern "C" int scfgp_predict(scfgp_ctx* c, const double* Xs, int64_t T, const double* alpha, const double* Li,
                             double* mu, double* sd) {
    return predict_impl(c, Xs, T, alpha, Li, mu, sd, 0);
}

// SCFGP.predict feeds pred_func with X_scaler.forward_transform(Xs) (SCFGP/SCFGP.py:279); for large test
// sets that element-wise host pass dominates, so the same transform can run inside the packing kernel.
extern "C" int scfgp_set_x_scaler(scfgp_ctx* c, int mode, const double* mn, const double* mx, const double* boxcox,
                                  const double* mu, const double* sd) {
    if (!c || mode < 0 || mode > 5) return SCFGP_EARG;
    HIPCHK(c, hipSetDevice(c->device));
    const int D = c->g.D;
    std::vector<double> h(5 * D, 0.0);
    const double* src[5] = {mn, mx, boxcox, mu, sd};
    for (int k = 0; k < 5; ++k)
        if (src[k]) std::copy(src[k], src[k] + D, h.begin() + k * D);
    if (!c->d_xscale) { if (int rc = dmalloc(c, &c->d_xscale, sizeof(double) * 5 * D)) return rc; }
    HIPCHK(c, hipMemcpy(c->d_xscale, h.data(), sizeof(double) * 5 * D, hipMemcpyHostToDevice));
    c->xs_mode = mode;
    return SCFGP_OK;
}
extern "C" int scfgp_predict_raw(scfgp_ctx* c, const double* Xs, int64_t T, const double* alpha, const double* Li,
                                 double* mu, double* sd) {
    if (c && c->xs_mode && !c->d_xscale) { c->err = "predict_raw: no scaler set"; return SCFGP_EARG; }
    return predict_impl(c, Xs, T, alpha, Li, mu, sd, 1);
}

// The rest of SCFGP.predict (SCFGP/SCFGP.py:281-293): y_scaler.backward_transform of mu and of the mu +- std
// band, std_y = half the transformed band, and with targets the metrics MAE, NMAE, MSE, NMSE, MNLP, SCORE.
extern "C" int scfgp_set_y_scaler(scfgp_ctx* c, int mode, double mn, double mx, double boxcox, double mu, double sd) {
    if (!c || mode < 0 || mode > 5) return SCFGP_EARG;
    HIPCHK(c, hipSetDevice(c->device));
    const double h[5] = {mn, mx, boxcox, mu, sd};
    if (!c->d_yscale) { if (int rc = dmalloc(c, &c->d_yscale, sizeof(double) * 5)) return rc; }
    HIPCHK(c, hipMemcpy(c->d_yscale, h, sizeof(h), hipMemcpyHostToDevice));
    c->ys_mode = mode;
    return SCFGP_OK;
}
extern "C" int scfgp_predict_y(scfgp_ctx* c, const double* Xs, int64_t T, const double* alpha, const double* Li,
                               const double* ys, double* mu_y, double* std_y, double* metrics) {
    if (c && ((c->xs_mode && !c->d_xscale) || !c->d_yscale)) { c->err = "predict_y: scalers not set"; return SCFGP_EARG; }
    if (c && ys && !metrics) { c->err = "predict_y: targets given without a metrics buffer"; return SCFGP_EARG; }
    return predict_impl(c, Xs, T, alpha, Li, mu_y, std_y, 1, 1, ys, metrics);
}

// Gradients of the predictive mean and std in the inputs (predgrad.hip).  mu, std are those of scfgp_predict (mode 0),
// scfgp_predict_raw (1) or scfgp_predict_y (2), bit for bit: the same chunks, kernels and order.
extern "C" int scfgp_predict_grad(scfgp_ctx* c, const double* Xs, int64_t T, const double* alpha, const double* Li, int mode,
                                  double* mu, double* sd, double* dmu, double* dstd) {
    if (!c) return SCFGP_EARG;
    if (!Xs || !alpha || !Li || !mu || !sd || !dmu || T < 1 || mode < 0 || mode > 2) { c->err = "predict_grad: bad arguments"; return SCFGP_EARG; }
    if (mode >= 1 && !c->d_xscale) { c->err = "predict_grad: no X scaler set"; return SCFGP_EARG; }
    if (mode == 2 && !c->d_yscale) { c->err = "predict_grad: no y scaler set"; return SCFGP_EARG; }
    return predict_impl(c, Xs, T, alpha, Li, mu, sd, mode >= 1 ? 1 : 0, mode == 2 ? 1 : 0, nullptr, nullptr, dmu, dstd);
}

// ----------------------------------------------------------------------------------------------
// joint posterior covariance between test points (predcov.hip; contract in include/scfgp_hip.h)
// ----------------------------------------------------------------------------------------------
// The chunk pipeline (RowFeed, OutRing) with the X scaler in mode 1; the chunk body is C = Phi* Li^T.  Cb (the rows of Xb) is formed
// once, into p_V, by job 0 of the feed; each chunk of Xa gives Ca in p_C; in the symmetric case (Ta <= PRED_ROWS) Ca is both operands.
// A chunk's rows of the result are computed in panels of R rows x Tb, full rows in the symmetric case too (its symmetry comes from the
// commutativity of the products, predcov.hip); the ring's slots are panels, not chunks: device memory does not grow with Ta x Tb.
static constexpr int64_t COV_PANEL_BYTES = (int64_t)128 << 20;   // per staging panel: the size scfgp_sample stages per chunk at 512 samples
extern "C" int scfgp_predict_cov(scfgp_ctx* c, const double* Xa, int64_t Ta, const double* Xb, int64_t Tb, const double* Li, int mode,
                                 int noise, double* cov) {
    if (!c) return SCFGP_EARG;
    if (!Xa || !Li || !cov || mode < 0 || mode > 1) { c->err = "predict_cov: bad arguments"; return SCFGP_EARG; }
    const bool sym = Xb == nullptr;
    if (sym) Tb = Ta;
    const Fail fail = {c, "predict_cov"};
    if (Ta < 1) return fail.arg("Ta must be at least 1");
    if (Tb < 1 || Tb > PRED_ROWS) return fail.arg(sym ? "the symmetric form takes 1..32768 rows" : "Tb must lie in 1..32768");
    if (!sym && noise) return fail.arg("noise is defined for the symmetric form (Xb == NULL) only");
    int rc;
    if ((rc = need_model(fail, mode == 1))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const Geom& g0 = c->g;
    const int64_t Kp = g0.Kp;
    const size_t ts = c->tsize();
    if ((rc = ensure_pred_chunk(c))) return rc;
    if ((rc = ensure_pred_factor(c))) return rc;
    // panel height: whole 128-row tiles within COV_PANEL_BYTES, no more than a chunk holds
    const int64_t R = std::min<int64_t>(round_up(std::min<int64_t>(Ta, PRED_ROWS), 128),
                                        std::max<int64_t>(128, COV_PANEL_BYTES / ((int64_t)sizeof(double) * Tb) / 128 * 128));
    RowFeed feed; OutRing ring; DevTmp stage;                     // Li / two chunks of X | two panels of the result
    if ((rc = feed.open(c, PRED_ROWS * g0.D, (int64_t)g0.K * g0.K))) return rc;
    if ((rc = dmalloc(c, &stage.p, sizeof(double) * 2 * R * Tb))) return rc;
    const void* LiT;
    if ((rc = load_factor(c, feed, Li, pad_square, true, nullptr, &LiT))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->st));                     // raw is reused below
    if ((rc = ring.open(c))) return rc;
    const RowJobs jobs = {Xa, nullptr, Ta, PRED_ROWS, Xb, Tb};       // job 0 is Xb in the cross form, the chunks of Xa follow
    const int64_t njobs = jobs.count();
    // panel p: rows [row0, row0 + n) of the result
    struct Panel { int64_t row0, n; };
    auto slot = [&](int64_t p) { return stage + (p & 1) * R * Tb; };
    auto download = [&](int64_t p, Panel pn) {
        return ring.drain(p, [&]() -> int {
            HIPCHK(c, hipMemcpyAsync(cov + pn.row0 * Tb, slot(p), sizeof(double) * pn.n * Tb, hipMemcpyDeviceToHost, c->copy_st));
            return SCFGP_OK;
        });
    };
    int64_t npanel = 0;
    Panel prev = {0, 0};
    if ((rc = feed.upload(0, jobs))) return rc;
    for (int64_t job = 0; job < njobs; ++job) {
        const Geom g = chunk_geom(g0, jobs.rows(job));
        const double* x;
        if ((rc = feed.acquire(job, &x))) return rc;
        pack_chunk(c, g, x, nullptr, nullptr, nullptr, mode == 1 ? c->xs_mode : 0, c->d_xscale);
        if ((rc = feed.release(job))) return rc;
        if ((rc = DISPATCH(c, cov_factor_chunk, c, g, LiT, jobs.lead(job) ? c->p_V : c->p_C))) return rc;
        if (job + 1 < njobs && (rc = feed.upload(job + 1, jobs))) return rc;
        if (jobs.lead(job)) continue;
        const int64_t t0 = jobs.row0(job);
        const void* Cb = sym ? c->p_C : c->p_V;
        for (int64_t r0 = 0; r0 < g.N; r0 += R, ++npanel) {
            const Panel pn = {t0 + r0, std::min<int64_t>(R, g.N - r0)};
            if ((rc = ring.acquire(npanel))) return rc;
            DISPATCH(c, cov_panel, c, (const char*)c->p_C + ts * r0 * Kp, Cb, pn.n, Tb, pn.row0, noise, slot(npanel));
            HIPCHK(c, hipGetLastError());
            if ((rc = ring.computed(npanel))) return rc;
            if (npanel >= 1 && (rc = download(npanel - 1, prev))) return rc;
            prev = pn;
        }
    }
    if ((rc = download(npanel - 1, prev))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->copy_st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    return SCFGP_OK;
}

// ----------------------------------------------------------------------------------------------
// posterior covariance of the input gradient (gradcov.hip; derivation and promises in include/scfgp_hip.h)
// ----------------------------------------------------------------------------------------------
static constexpr int GRADCOV_MAX_Q = 64;                          // a point's q rows lie in one 64-row group of the block kernel
static constexpr int64_t GRADCOV_SLOT_BYTES = (int64_t)64 << 20;  // per-point D x D arrays of a chunk (a dcov slot, the records)
// points per chunk (the formula of the header): whole groups of (64 / q) points in the 32 768-row chunk buffers and, where a chunk
// carries a D x D array per point, no more points than the slot budget holds
static int64_t gradcov_points(const Geom& g, bool want_cov) {
    const int q = std::min(g.D, g.S), ppg = 64 / q;
    int64_t np = PRED_ROWS / (ppg * q) * ppg;
    if (want_cov) np = std::min(np, std::max<int64_t>(1, GRADCOV_SLOT_BYTES / (8 * (int64_t)g.D * g.D)));
    return np;
}
// The chunk pipeline (RowFeed, OutRing) with the weights behind the rows of their chunk.  dmu | dvar | dcov of a chunk leave through the
// two slots of `stage`; the records and the running D x D sums stay on the device, the sums are fetched once, at the end.
extern "C" int scfgp_predict_gradcov(scfgp_ctx* c, const double* Xs, int64_t T, const double* w, const double* alpha, const double* Li,
                                     int mode, double* dmu, double* dvar, double* dcov, double* asub) {
    if (!c) return SCFGP_EARG;
    if (!Xs || !alpha || !Li || T < 1 || mode < 0 || mode > 1) { c->err = "predict_gradcov: bad arguments"; return SCFGP_EARG; }
    if (!dmu && !dvar && !dcov && !asub) { c->err = "predict_gradcov: no output requested"; return SCFGP_EARG; }
    const Fail fail = {c, "predict_gradcov"};
    int rc;
    if ((rc = need_model(fail, mode == 1))) return rc;
    const Geom& g0 = c->g;
    const int D = g0.D, q = std::min(g0.D, g0.S);
    if (q > GRADCOV_MAX_Q) return fail.arg("min(D, S) must be at most 64");
    double sw = (double)T;
    if (asub && w) {
        const WeightScan ws = scan_weights(w, T);
        if (ws.first_bad() >= 0) return fail.arg("weight " + std::to_string(ws.first_bad()) + " is negative or not finite");
        sw = ws.sum;
        if (!(sw > 0.0)) return fail.arg("the weights sum to zero");
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (c->prof) { c->recs.clear(); c->pool_used = 0; }          // timings describe this call's chunks (tools/predict_gradcov_time.py)
    if ((rc = ensure_pred_chunk(c))) return rc;
    if ((rc = ensure_pred_grad(c, false))) return rc;
    if ((rc = ensure_pred_factor(c))) return rc;
    const bool feed_w = asub && w;
    const int xmode = mode == 1 ? c->xs_mode : 0;
    const int64_t DD = (int64_t)D * D;
    const RowJobs jobs = {Xs, feed_w ? w : nullptr, T, gradcov_points(g0, dcov || asub)};
    const int64_t nchunks = jobs.count(), rows = std::min(T, jobs.CH);
    const int64_t slot_len = rows * D * 2 + (dcov ? rows * DD : 0);
    RowFeed feed; OutRing ring; DevTmp qt, gfac, stage, rec, acc;  // Li / two chunks of [Xs | w] | Q | g_t | two slots | records | sums
    if ((rc = feed.open(c, PRED_ROWS * (D + 1), (int64_t)g0.K * g0.K))) return rc;
    if ((rc = dmalloc(c, &qt.p, c->tsize() * q * g0.Jp))) return rc;
    if (xmode && (rc = dmalloc(c, &gfac.p, sizeof(double) * rows * D))) return rc;
    if ((rc = dmalloc(c, &stage.p, sizeof(double) * 2 * slot_len))) return rc;
    if (asub && ((rc = dmalloc(c, &rec.p, sizeof(double) * rows * DD)) || (rc = dmalloc(c, &acc.p, sizeof(double) * DD)))) return rc;
    const void* LiT;
    if ((rc = load_factor(c, feed, Li, pad_square, true, alpha, &LiT))) return rc;
    DISPATCH(c, grad_operand, c);
    DISPATCH(c, gradcov_basis, c, qt.p);
    if (asub) HIPCHK(c, hipMemsetAsync(acc.p, 0, sizeof(double) * DD, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));                     // raw is reused below
    if ((rc = ring.open(c))) return rc;
    auto slot_dmu = [&](int64_t i) { return stage + (i & 1) * slot_len; };
    auto slot_dvar = [&](int64_t i) { return stage + (i & 1) * slot_len + rows * D; };
    auto slot_dcov = [&](int64_t i) { return stage + (i & 1) * slot_len + 2 * rows * D; };
    auto download = [&](int64_t i) {
        return ring.drain(i, [&]() -> int {
            const int64_t t0 = jobs.row0(i), n = jobs.rows(i);
            if (dmu) HIPCHK(c, hipMemcpyAsync(dmu + t0 * D, slot_dmu(i), sizeof(double) * n * D, hipMemcpyDeviceToHost, c->copy_st));
            if (dvar) HIPCHK(c, hipMemcpyAsync(dvar + t0 * D, slot_dvar(i), sizeof(double) * n * D, hipMemcpyDeviceToHost, c->copy_st));
            if (dcov) HIPCHK(c, hipMemcpyAsync(dcov + t0 * DD, slot_dcov(i), sizeof(double) * n * DD, hipMemcpyDeviceToHost, c->copy_st));
            return SCFGP_OK;
        });
    };
    if ((rc = feed.upload(0, jobs))) return rc;
    for (int64_t i = 0; i < nchunks; ++i) {
        const Geom g = chunk_geom(g0, jobs.rows(i));
        const double *x, *wi;
        if ((rc = feed.acquire(i, &x, &wi))) return rc;
        pack_chunk(c, g, x, nullptr, nullptr, nullptr, xmode, c->d_xscale);
        if ((rc = ring.acquire(i))) return rc;
        // the raw rows and the weights stay in the feed's half until the block kernel has read them
        if ((rc = DISPATCH(c, gradcov_chunk, c, g, LiT, qt.p, x, xmode, gfac.p, feed_w ? wi : nullptr, slot_dmu(i), dvar ? slot_dvar(i) : nullptr,
                           dcov ? slot_dcov(i) : nullptr, rec.p, acc.p)))
            return rc;
        if ((rc = feed.release(i))) return rc;
        if ((rc = ring.computed(i))) return rc;
        if (i + 1 < nchunks && (rc = feed.upload(i + 1, jobs))) return rc;
        if (i >= 1 && (rc = download(i - 1))) return rc;
    }
    if ((rc = download(nchunks - 1))) return rc;
    std::vector<double> sums;
    if (asub) {
        sums.resize(DD);
        HIPCHK(c, hipMemcpyAsync(sums.data(), acc.p, sizeof(double) * DD, hipMemcpyDeviceToHost, c->st));
    }
    HIPCHK(c, hipStreamSynchronize(c->copy_st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    if (asub)                                                     // one division per entry of the lower triangle, mirrored
        for (int d = 0; d < D; ++d)
            for (int e = 0; e <= d; ++e) asub[(int64_t)d * D + e] = asub[(int64_t)e * D + d] = sums[(int64_t)d * D + e] / sw;
    return SCFGP_OK;
}

// ----------------------------------------------------------------------------------------------
// partial dependence and ICE curves over a pool (pd.hip; derivation and promises in include/scfgp_hip.h)
// ----------------------------------------------------------------------------------------------
static constexpr int PD_MAX_G = SAMPLE_MAX;                       // the ICE block is sample_product's shape
static constexpr int64_t PD_RECORD_BYTES = GRADCOV_SLOT_BYTES;    // block records of one launch of the sums kernel
// Two passes of the chunk pipeline.  The first (pd, pd_sd or pd_cov wanted) feeds [Xs | w] and leaves the running sums of the zeroed-column
// features on the device, the dimensions in groups whose block records fit PD_RECORD_BYTES; the sums are checked, then the curves come
// from the stacked mean rows in groups of dimensions that fit the chunk buffers.  The second (ice wanted) feeds Xs again and sends one
// T_chunk x G block per (chunk, dimension) through the two slots of an OutRing.  No output is written before the last refusal is past.
extern "C" int scfgp_predict_pd(scfgp_ctx* c, const double* Xs, int64_t T, const double* w, const double* alpha, const double* Li,
                                const int* dims, int ndim, const double* grid, int G, int mode, double* pd, double* pd_sd, double* pd_cov,
                                double* ice) {
    if (!c) return SCFGP_EARG;
    if (!Xs || !alpha || !Li || !dims || !grid) { c->err = "predict_pd: bad arguments"; return SCFGP_EARG; }
    if (!pd && !pd_sd && !pd_cov && !ice) { c->err = "predict_pd: no output requested"; return SCFGP_EARG; }
    const Geom& g0 = c->g;
    const int D = g0.D;
    if (T < 1) { c->err = "predict_pd: T must be at least 1"; return SCFGP_EARG; }
    if (G < 1 || G > PD_MAX_G) { c->err = "predict_pd: G must lie in 1..1024"; return SCFGP_EARG; }
    if (ndim < 1 || ndim > D) { c->err = "predict_pd: ndim must lie in 1..D"; return SCFGP_EARG; }
    if (mode < 0 || mode > 1) { c->err = "predict_pd: bad mode"; return SCFGP_EARG; }
    {
        std::vector<char> seen(D, 0);
        for (int a = 0; a < ndim; ++a) {
            if (dims[a] < 0 || dims[a] >= D) { c->err = "predict_pd: dimension " + std::to_string(dims[a]) + " is out of range"; return SCFGP_EARG; }
            if (seen[dims[a]]) { c->err = "predict_pd: dimension " + std::to_string(dims[a]) + " is given twice"; return SCFGP_EARG; }
            seen[dims[a]] = 1;
        }
    }
    const Fail fail = {c, "predict_pd"};
    int rc;
    if ((rc = need_model(fail, mode == 1))) return rc;
    double W = (double)T;
    if (w) {
        const WeightScan ws = scan_weights(w, T);
        if (ws.first_negative >= 0) return fail.arg("negative weight at row " + std::to_string(ws.first_negative));
        W = ws.sum;
        if (ws.first_nonfinite >= 0 || !std::isfinite(W)) return fail.nonfinite("non-finite weights");
        if (!ws.positive) return fail.arg("no row has a positive weight");
    }
    const int xmode = mode == 1 ? c->xs_mode : 0;
    const int64_t NG = (int64_t)ndim * G;
    if (!xmode)
        for (int64_t e = 0; e < NG; ++e)
            if (!std::isfinite(grid[e])) return fail.nonfinite("non-finite grid value");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->prof) { c->recs.clear(); c->pool_used = 0; }          // timings describe this call's chunks (tools/pd_time.py)
    if ((rc = ensure_pred_chunk(c))) return rc;
    if ((rc = ensure_pred_factor(c))) return rc;
    const bool curves = pd || pd_sd || pd_cov;
    const RowJobs jobs = {Xs, w, T, PRED_ROWS}, rows_only = {Xs, nullptr, T, PRED_ROWS};      // pass 1 | pass 2
    const int64_t rows = std::min<int64_t>(T, PRED_ROWS), nchunks = jobs.count(), Jp2 = 2 * (int64_t)g0.Jp;
    const int Gp = pd_grid_rows(G);
    DevTmp d_dims, d_grid, wchunk;                                // dims | the (transformed) grid | w of the chunk, padded
    if ((rc = dmalloc(c, &d_dims.p, sizeof(int) * ndim))) return rc;
    if ((rc = dmalloc(c, &d_grid.p, sizeof(double) * NG))) return rc;
    if (w && curves && (rc = dmalloc(c, &wchunk.p, sizeof(double) * PRED_ROWS))) return rc;
    const int* dv = (const int*)d_dims.p;
    HIPCHK(c, hipMemcpyAsync(d_dims.p, dims, sizeof(int) * ndim, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemcpyAsync(d_grid.p, grid, sizeof(double) * NG, hipMemcpyHostToDevice, c->st));
    if (xmode) {
        std::vector<double> hg(NG);
        pd_grid(d_grid, dv, ndim, G, D, xmode, c->d_xscale, c->st);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(hg.data(), d_grid.p, sizeof(double) * NG, hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipStreamSynchronize(c->st));
        for (int64_t e = 0; e < NG; ++e)
            if (!std::isfinite(hg[e])) { c->err = "predict_pd: non-finite grid value after the X scaler"; return SCFGP_ENONFINITE; }
    }
    RowFeed feed;                                                 // Li / two chunks of [Xs | w], for both passes
    if ((rc = feed.open(c, PRED_ROWS * (D + 1), (int64_t)g0.K * g0.K))) return rc;
    const void* LiT;
    if ((rc = load_factor(c, feed, Li, pad_square, true, alpha, &LiT))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->st));                     // raw is reused below
    std::vector<double> h_pd, h_sd;
    if (curves) {
        // ---- pass 1: the running sums, ndim x 2 x Jp ----
        const Geom gmax = chunk_geom(g0, rows);
        int ngs = (int)std::min<int64_t>(ndim, std::max<int64_t>(1, PD_RECORD_BYTES / (int64_t)sizeof(double) / pd_record_len(gmax, 1)));
        if (c->test_pd_group > 0) ngs = std::min(ngs, c->test_pd_group);
        DevTmp rec, acc, flag;
        if ((rc = dmalloc(c, &rec.p, sizeof(double) * pd_record_len(gmax, ngs)))) return rc;
        if ((rc = dmalloc(c, &acc.p, sizeof(double) * ndim * Jp2))) return rc;
        if ((rc = dmalloc(c, &flag.p, sizeof(int) * 4))) return rc;
        HIPCHK(c, hipMemsetAsync(acc.p, 0, sizeof(double) * ndim * Jp2, c->st));
        HIPCHK(c, hipMemsetAsync(flag.p, 0, sizeof(int) * 4, c->st));
        if ((rc = feed.upload(0, jobs))) return rc;
        for (int64_t i = 0; i < nchunks; ++i) {
            const Geom g = chunk_geom(g0, jobs.rows(i));
            const double *x, *wraw;
            if ((rc = feed.acquire(i, &x, &wraw))) return rc;
            pack_chunk(c, g, x, w ? wraw : nullptr, nullptr, wchunk.p, xmode, c->d_xscale);
            if ((rc = feed.release(i))) return rc;
            for (int a0 = 0; a0 < ndim; a0 += ngs)
                if ((rc = DISPATCH(c, pd_sums_chunk, c, g, wchunk.p, dv + a0, std::min(ngs, ndim - a0), rec.p, acc + a0 * Jp2))) return rc;
            if (i + 1 < nchunks && (rc = feed.upload(i + 1, jobs))) return rc;
        }
        update_check_finite(acc, ndim * Jp2, (int*)flag.p, c->st);
        int hflag[4];
        HIPCHK(c, hipMemcpyAsync(hflag, flag.p, sizeof(hflag), hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipStreamSynchronize(c->copy_st));
        HIPCHK(c, hipStreamSynchronize(c->st));
        HIPCHK(c, hipGetLastError());
        if (hflag[1]) { c->err = "predict_pd: non-finite weighted sum of the features"; return SCFGP_ENONFINITE; }
        // ---- the curves: groups of dimensions whose stacked rows fit the chunk buffers ----
        int ngc = (int)std::min<int64_t>(ndim, PRED_ROWS / Gp);
        if (c->test_pd_group > 0) ngc = std::min(ngc, c->test_pd_group);
        const int64_t GG = (int64_t)G * G;
        DevTmp cur, stage; OutRing ring;                          // pd | scratch | sd of a group | two slots of G x G
        if ((rc = dmalloc(c, &cur.p, sizeof(double) * 3 * PRED_ROWS))) return rc;
        if (pd_cov && (rc = dmalloc(c, &stage.p, sizeof(double) * 2 * GG))) return rc;
        if ((rc = ring.open(c))) return rc;
        h_pd.resize(NG); h_sd.resize(NG);
        int64_t nslot = 0, prev = 0;
        auto download = [&](int64_t k, int64_t a) {
            return ring.drain(k, [&]() -> int {
                HIPCHK(c, hipMemcpyAsync(pd_cov + a * GG, stage + (k & 1) * GG, sizeof(double) * GG, hipMemcpyDeviceToHost, c->copy_st));
                return SCFGP_OK;
            });
        };
        for (int a0 = 0; a0 < ndim; a0 += ngc) {
            const int ng = std::min(ngc, ndim - a0);
            const Geom gr = chunk_geom(g0, (int64_t)ng * Gp);
            if ((rc = DISPATCH(c, pd_curves, c, gr, LiT, acc + a0 * Jp2, W, dv + a0, d_grid + (int64_t)a0 * G, ng, G, cur.p, cur + PRED_ROWS,
                               cur + 2 * PRED_ROWS)))
                return rc;
            HIPCHK(c, hipMemcpy2DAsync(h_pd.data() + (int64_t)a0 * G, sizeof(double) * G, cur.p, sizeof(double) * Gp, sizeof(double) * G, ng,
                                       hipMemcpyDeviceToHost, c->st));
            HIPCHK(c, hipMemcpy2DAsync(h_sd.data() + (int64_t)a0 * G, sizeof(double) * G, cur + 2 * PRED_ROWS, sizeof(double) * Gp,
                                       sizeof(double) * G, ng, hipMemcpyDeviceToHost, c->st));
            if (pd_cov)
                for (int a = 0; a < ng; ++a, ++nslot) {
                    if ((rc = ring.acquire(nslot))) return rc;
                    if ((rc = DISPATCH(c, pd_cov_dim, c, a, G, stage + (nslot & 1) * GG))) return rc;
                    if ((rc = ring.computed(nslot))) return rc;
                    if (nslot >= 1 && (rc = download(nslot - 1, prev))) return rc;
                    prev = a0 + a;
                }
            // the copies out of cur and predcov's reads of p_C are on the context's stream, ahead of the next group's kernels
        }
        if (pd_cov && nslot >= 1 && (rc = download(nslot - 1, prev))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->copy_st));
        HIPCHK(c, hipStreamSynchronize(c->st));
        HIPCHK(c, hipGetLastError());
    }
    if (ice) {
        // ---- pass 2: one T_chunk x G block per (chunk, dimension) ----
        OutRing ring; DevTmp stage, R, keep;                      // two blocks | the rotated weights | the saved column
        // The rows go through the feed of pass 1 again.  Both streams have drained, so its events are all past; the jobs go on from an
        // even number, so that the halves alternate as before and a wait for reuse meets a recorded (or never used) event.
        const int64_t j0 = curves ? (nchunks + 1) / 2 * 2 : 0;
        if ((rc = dmalloc(c, &stage.p, sizeof(double) * 2 * rows * G))) return rc;
        if ((rc = dmalloc(c, &R.p, c->tsize() * sample_w_rows(g0.K) * sample_w_cols(G)))) return rc;
        if ((rc = dmalloc(c, &keep.p, sizeof(double) * PRED_ROWS))) return rc;
        if ((rc = ring.open(c))) return rc;
        auto slot = [&](int64_t k) { return stage + (k & 1) * rows * G; };
        auto download = [&](int64_t k) {
            const int64_t i = k / ndim, a = k % ndim;
            return ring.drain(k, [&]() -> int {
                HIPCHK(c, hipMemcpyAsync(ice + (a * T + jobs.row0(i)) * G, slot(k), sizeof(double) * jobs.rows(i) * G, hipMemcpyDeviceToHost,
                                         c->copy_st));
                return SCFGP_OK;
            });
        };
        if ((rc = feed.upload(0, rows_only, j0))) return rc;
        int64_t k = 0;
        for (int64_t i = 0; i < nchunks; ++i) {
            const Geom g = chunk_geom(g0, jobs.rows(i));
            const double* x;
            if ((rc = feed.acquire(j0 + i, &x))) return rc;
            pack_chunk(c, g, x, nullptr, nullptr, nullptr, xmode, c->d_xscale);
            if ((rc = feed.release(j0 + i))) return rc;
            for (int a = 0; a < ndim; ++a, ++k) {
                if ((rc = ring.acquire(k))) return rc;
                if ((rc = DISPATCH(c, pd_ice_chunk, c, g, dims[a], d_grid + (int64_t)a * G, G, R.p, keep.p, slot(k)))) return rc;
                if ((rc = ring.computed(k))) return rc;
                if (a == 0 && i + 1 < nchunks && (rc = feed.upload(i + 1, rows_only, j0))) return rc;
                if (k >= 1 && (rc = download(k - 1))) return rc;
            }
        }
        if ((rc = download(k - 1))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->copy_st));
        HIPCHK(c, hipStreamSynchronize(c->st));
        HIPCHK(c, hipGetLastError());
    }
    if (pd) memcpy(pd, h_pd.data(), sizeof(double) * NG);
    if (pd_sd) memcpy(pd_sd, h_sd.data(), sizeof(double) * NG);
    return SCFGP_OK;
}

// ----------------------------------------------------------------------------------------------
// closed-form Sobol indices under a product measure (sobol.hip; derivation in include/scfgp_hip.h)
// ----------------------------------------------------------------------------------------------
static constexpr int SOBOL_MAX_NW = SAMPLE_MAX;
static constexpr int64_t SOBOL_RECORD_BYTES = GRADCOV_SLOT_BYTES;  // the workgroups' records of one pass over a block of columns
// No rows, no factors, no scaler: the tables from Fall / Scal, then the columns of W in passes whose records fit SOBOL_RECORD_BYTES.  The
// schedule of the pair kernel (api_host.h) depends on J and D only, so a column has one summation order whatever nw is.
extern "C" int scfgp_sobol(scfgp_ctx* c, const int32_t* kind, const double* p0, const double* p1, const double* W, int nw, double* f0,
                           double* V, double* Vmain, double* Vtot, double* phibar) {
    if (!c) return SCFGP_EARG;
    const Fail f = {c, "sobol"};
    const Geom& g = c->g;
    const int D = g.D, J = g.J, K = g.K;
    const bool cols = f0 || V || Vmain || Vtot;
    if (!p0 || !p1) return f.arg("p0 and p1 are needed");
    if (!cols && !phibar) return f.arg("no output asked for");
    if (cols && !W) return f.arg("W is needed for f0, V, Vmain and Vtot");
    if (cols && (nw < 1 || nw > SOBOL_MAX_NW)) return f.arg("nw must lie in 1..1024");
    if (int d = sobol_first_bad_kind(kind, D); d >= 0) return f.arg("kind[" + std::to_string(d) + "] must be 0 (uniform) or 1 (normal)");
    if (int d = sobol_first_bad_range(kind, p0, p1, D); d >= 0)
        return f.arg("input " + std::to_string(d) + (kind && kind[d] == 1 ? ": p1 (the standard deviation) is negative" : ": p1 < p0 on a uniform input"));
    if (int rc = need_model(f, false)) return rc;
    if (int d = sobol_first_nonfinite(p0, p1, D); d >= 0) return f.nonfinite("non-finite measure at input " + std::to_string(d));
    if (cols)
        for (int64_t i = 0; i < (int64_t)K * nw; ++i)
            if (!std::isfinite(W[i])) return f.nonfinite("non-finite W");
    HIPCHK(c, hipSetDevice(c->device));
    if (!cols) nw = 0;

    const int Jt = (int)round_up(J, SOBOL_T), nb = Jt / SOBOL_T, nsets = 1 + 2 * D;
    const int flags = (V || Vtot ? 1 : 0) | (Vmain ? 2 : 0) | (Vtot ? 4 : 0);
    std::vector<int> units;
    int pass = 0;
    if (flags) {
        sobol_units(nb, sobol_kseg(nb, nsets, SOBOL_COLS, SOBOL_RECORD_BYTES), units);
        pass = std::min<int>((int)round_up(nw, SOBOL_COLS), sobol_pass_cols((int64_t)units.size() / 3, nsets, SOBOL_COLS, SOBOL_RECORD_BYTES));
    }
    const int64_t nunits = (int64_t)units.size() / 3;
    int G = std::min(D, SOBOL_GROUP);
    if (c->test_sobol_group > 0) G = std::min(G, c->test_sobol_group);
    // one allocation: meas | omax | psi1 | Ed | E | Eb | phibar | W | A | f0 | sums | units | rec
    const int64_t n_meas = 3 * D, n_tab = 2 * (int64_t)D * Jt, n_e = 2 * Jt, n_w = (int64_t)K * nw, n_a = 2 * (int64_t)Jt * nw,
                  n_sums = (int64_t)nsets * nw, n_units = (3 * nunits + 1) / 2, n_rec = nunits * nsets * pass;
    DevTmp buf;
    if (int rc = dmalloc(c, &buf.p, sizeof(double) * (n_meas + D + 2 * n_tab + 2 * n_e + K + n_w + n_a + nw + n_sums + n_units + n_rec))) return rc;
    double* d_meas = buf.p; double* d_omax = d_meas + n_meas; double* d_psi1 = d_omax + D; double* d_Ed = d_psi1 + n_tab; double* d_E = d_Ed + n_tab;
    double* d_Eb = d_E + n_e; double* d_phibar = d_Eb + n_e; double* d_W = d_phibar + K; double* d_A = d_W + n_w; double* d_f0 = d_A + n_a;
    double* d_sums = d_f0 + nw; int* d_units = (int*)(d_sums + n_sums); double* d_rec = d_sums + n_sums + n_units;

    std::vector<double> h(std::max<int64_t>(n_meas, K + nw + n_sums));
    sobol_measure(kind, p0, p1, D, h.data());
    HIPCHK(c, hipMemcpyAsync(d_meas, h.data(), sizeof(double) * n_meas, hipMemcpyHostToDevice, c->st));
    if (cols) HIPCHK(c, hipMemcpyAsync(d_W, W, sizeof(double) * n_w, hipMemcpyHostToDevice, c->st));
    if (nunits) HIPCHK(c, hipMemcpyAsync(d_units, units.data(), sizeof(int) * 3 * nunits, hipMemcpyHostToDevice, c->st));
    // the largest frequency of every input, read back with the same wait: the measure is held against the domain of sin / cos before
    // any table or pair is formed
    std::vector<double> h_omax(D);
    sobol_omax(g, c->d_Fall, d_omax, c->st);
    HIPCHK(c, hipMemcpyAsync(h_omax.data(), d_omax, sizeof(double) * D, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));                      // h is reused for the results
    if (int d = sobol_first_out_of_domain(h.data(), h_omax.data(), D); d >= 0)
        return f.arg("input " + std::to_string(d) + ": the measure's phases leave the sin/cos domain (2 max|Om| |x| < 3.37e9)");
    { ProfScope ps(c, "sobol_tables"); sobol_tables(g, c->d_Fall, c->d_sc, d_meas, Jt, d_psi1, d_Ed, d_E, d_Eb, d_phibar, c->st); }
    if (cols) { ProfScope ps(c, "sobol_weights"); sobol_weights(g, d_W, c->d_sc, d_E, Jt, nw, d_A, d_f0, c->st); }
    for (int w0 = 0; flags && w0 < nw; w0 += pass) {
        const int ncols = std::min(pass, nw - w0);
        { ProfScope ps(c, "sobol_pairs");
          sobol_pairs(g, c->d_Fall, d_meas, d_psi1, d_Ed, d_E, d_Eb, d_A, d_units, (int)nunits, Jt, nw, w0, ncols, G, flags, d_rec, c->st); }
        { ProfScope ps(c, "sobol_reduce"); sobol_reduce(d_rec, (int)nunits, D, ncols, nw, w0, flags, d_sums, c->st); }
    }
    HIPCHK(c, hipGetLastError());
    // phibar | f0 | sums are adjacent on the device only up to W and A in between: three copies
    double* h_phibar = h.data(); double* h_f0 = h_phibar + K; double* h_sums = h_f0 + nw;
    HIPCHK(c, hipMemcpyAsync(h_phibar, d_phibar, sizeof(double) * K, hipMemcpyDeviceToHost, c->st));
    if (cols) HIPCHK(c, hipMemcpyAsync(h_f0, d_f0, sizeof(double) * nw, hipMemcpyDeviceToHost, c->st));
    if (flags) HIPCHK(c, hipMemcpyAsync(h_sums, d_sums, sizeof(double) * n_sums, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (phibar) memcpy(phibar, h_phibar, sizeof(double) * K);
    if (f0) memcpy(f0, h_f0, sizeof(double) * nw);
    if (V) memcpy(V, h_sums, sizeof(double) * nw);
    for (int w = 0; w < nw; ++w)
        for (int d = 0; d < D; ++d) {
            if (Vmain) Vmain[(int64_t)w * D + d] = h_sums[(int64_t)(1 + d) * nw + w];
            if (Vtot) Vtot[(int64_t)w * D + d] = h_sums[w] - h_sums[(int64_t)(1 + D + d) * nw + w];
        }
    return SCFGP_OK;
}
