// C ABI of libscfgp_hip.so, the sample functions and the entry points that sweep a pool of candidates: scfgp_sample_weights, _sample,
// _sample_argmax, _sample_grad, scfgp_acquire, _acquire_kg, scfgp_select, _select_iv and _select_qei.
#include "api_chunks.h"

// chunk bodies of this file's entry points; those that other files call too are ChunkImpl's (api_chunks.h)
template <typename T> struct PoolImpl : ChunkImpl<T> {
    typedef SweepKernels<T> SK;
    using ChunkImpl<T>::features;
    using ChunkImpl<T>::factor_c;
    static void pick_init(scfgp_ctx* c, const SelectBufs& b, const void* C) { select_init<T>(b, (const T*)C, c->st); }
    static void pick(scfgp_ctx* c, const SelectBufs& b, const void* C, int j) { select_step<T>(b, (const T*)C, j, c->d_sc, c->st); }
    // scfgp_select_iv: packed lower tiles of C^T diag(w) C of a chunk (w == NULL: C^T C) into `out`, by the Gram tiles update_chunk
    // uses, with the update's slabs (fp64 MFMA, or exact fp32 MFMA flushed into the fp64 slabs: never the fp16 split)
    static int iv_gram_chunk(scfgp_ctx* c, const Geom& g, const RowSplits& rs, const void* C, const double* w, double* out) {
        const int nts = g.Kp / g.tile, ntiles = nts * (nts + 1) / 2;
        double* sidepart = c->u_slabs + (size_t)rs.nsplit * ntiles * g.tile * g.tile;
        SK::gram(g, (const T*)C, w, nullptr, rs, sizeof(T) == 4 ? c->gram_chunk : 0, c->u_slabs, sidepart, c->u_flag + 8, c->u_ws2, c->st);
        reduce_tri_tiles(c->u_slabs, rs.nsplit, nts, g.tile, out, c->st);
        HIPCHK(c, hipGetLastError());
        return SCFGP_OK;
    }
    static void iv_init(scfgp_ctx* c, const SelectBufs& b, const SelectIvBufs& iv, const void* C, void* Qt) {
        SK::convert(iv.Q, (T*)Qt, c->g.K, c->g.Kp, c->st);
        select_iv_init<T>(b, iv, (const T*)C, (const T*)Qt, c->g.K, c->d_sc, c->st);
    }
    static void iv_pick(scfgp_ctx* c, const SelectBufs& b, const SelectIvBufs& iv, const void* C, int j) {
        select_iv_step<T>(b, iv, (const T*)C, j, c->d_sc, c->st);
    }
    // scfgp_sample: the weights of the sample functions (sample.hip), then per chunk out (N x nsamp) = Phi* W and the epilogue
    static void weights(scfgp_ctx* c, const double* Li, const double* alpha, int nsamp, uint64_t seed, double* Z, double* W, void* Wt) {
        sample_weights<T>(c->g, Li, alpha, c->d_sc, nsamp, seed, Z, W, (T*)Wt, c->st);
    }
    static int sample_chunk(scfgp_ctx* c, const Geom& g, const void* Wt, int nsamp, int64_t t0, uint64_t seed, int noise, int ymode,
                            double* out) {
        features(c, g);
        sample_product<T>(g, (const T*)c->p_Phi, (const T*)Wt, nsamp, t0, seed, noise, ymode, c->d_yscale, c->d_sc, out, c->st);
        HIPCHK(c, hipGetLastError());
        return SCFGP_OK;
    }
    // scfgp_sample_argmax: the same product, reduced per sample column in its epilogue and merged into the call's running best
    static int sample_argmax_chunk(scfgp_ctx* c, const Geom& g, const void* Wt, int nsamp, const double* w, int minimize, int64_t t0,
                                   const SampleArgmaxBufs& b) {
        features(c, g);
        sample_argmax_product<T>(g, (const T*)c->p_Phi, (const T*)Wt, nsamp, w, minimize, t0, t0 == 0, b, c->st);
        HIPCHK(c, hipGetLastError());
        return SCFGP_OK;
    }
    // scfgp_acquire: predict_chunk with acquire.hip's row kernels in rowpredict's place (the same partials in the same order, so mu has
    // scfgp_predict's bits), then the chunk's best eligible row into the call's running best
    static int acquire_chunk(scfgp_ctx* c, const Geom& g, const void* LiT, const AcquireSpec& a, const double* w, int64_t t0, const AcquireBufs& b) {
        features(c, g);
        SK::apply_predict(g, (const T*)c->p_Phi, (const T*)LiT, c->p_vpart, c->alpha_pred(), c->p_mupart, c->st);
        acquire_rows(g, ApplyKernels<T>::partials(g), c->p_mupart, c->p_vpart, c->d_sc, a, b, c->st);
        acquire_argmax(g, w, t0, t0 == 0, b, c->st);
        HIPCHK(c, hipGetLastError());
        return SCFGP_OK;
    }
    // scfgp_acquire_kg, the reference job: predict_chunk's product on the R reference rows, whose partials give u_r with scfgp_predict's
    // bits (kg.hip: d_r and the per-call constants of the nodes), then Cb = Phi Li^T into p_V, where it stays for the call
    static int kg_ref_chunk(scfgp_ctx* c, const Geom& g, const void* LiT, int minimize, const double* z, int J, const KgBufs& b, int* flag) {
        features(c, g);
        SK::apply_predict(g, (const T*)c->p_Phi, (const T*)LiT, c->p_vpart, c->alpha_pred(), c->p_mupart, c->st);
        kg_reference(ApplyKernels<T>::partials(g), c->p_mupart, g.Np, g.N, minimize, z, J, b.d, b.zf, flag, c->st);
        factor_c(c, g, (const T*)LiT, c->alpha_pred(), (T*)c->p_V);
        HIPCHK(c, hipGetLastError());
        return SCFGP_OK;
    }
    // a chunk of candidates: sigma from predict_chunk's product (scfgp_acquire's bits), Ca = Phi Li^T into p_C, then the fused product
    // with the node reduction and the two sums (kg.hip)
    static int kg_chunk(scfgp_ctx* c, const Geom& g, const void* LiT, int64_t R, int J, int noise, const KgBufs& b) {
        features(c, g);
        SK::apply_predict(g, (const T*)c->p_Phi, (const T*)LiT, c->p_vpart, c->alpha_pred(), c->p_mupart, c->st);
        kg_sigma(g, ApplyKernels<T>::partials(g), c->p_vpart, c->d_sc, noise, b.sd, c->st);
        factor_c(c, g, (const T*)LiT, c->alpha_pred(), (T*)c->p_C);
        kg_nodes<T>(g, (const T*)c->p_C, (const T*)c->p_V, R, J, b, c->d_sc, c->st);
        HIPCHK(c, hipGetLastError());
        return SCFGP_OK;
    }
    // scfgp_sample_grad: f and d f / d x~ of the chunk's rows, each under its own sample's weights (samplegrad.hip; FT: grad_operand)
    static int sample_grad_chunk(scfgp_ctx* c, const Geom& g, const double* WT, const double* sidx, int64_t t0, int nsamp, double* val,
                                 double* grad) {
        features(c, g);
        samplegrad<T>(g, (const T*)c->p_Phi, WT, sidx, t0, nsamp, (const T*)c->p_FT, val, grad, c->st);
        HIPCHK(c, hipGetLastError());
        return SCFGP_OK;
    }
};
#define DISPATCH(c, fn, ...) DISPATCH_TO(PoolImpl, c, fn, __VA_ARGS__)

// ----------------------------------------------------------------------------------------------
// posterior sample functions (sample.hip; derivation and random-number contract in include/scfgp_hip.h)
// ----------------------------------------------------------------------------------------------
// the weights of nsamp sample functions on the device: W (fp64) and Wt (the context's type), sample_w_rows(K) x sample_w_cols(nsamp)
struct SampleW { DevTmp z, w, wt; };
static int sample_weights_dev(scfgp_ctx* c, const double* alpha, const double* Li, int nsamp, uint64_t seed, SampleW& sw) {
    const Geom& g = c->g;
    const int64_t n = sample_w_rows(g.K) * sample_w_cols(nsamp);
    DevTmp dli, dal;
    int rc;
    if ((rc = dmalloc(c, &dli.p, sizeof(double) * g.K * g.K))) return rc;
    if ((rc = dmalloc(c, &dal.p, sizeof(double) * g.K))) return rc;
    if ((rc = dmalloc(c, &sw.z.p, sizeof(double) * n))) return rc;
    if ((rc = dmalloc(c, &sw.w.p, sizeof(double) * n))) return rc;
    if ((rc = dmalloc(c, &sw.wt.p, c->tsize() * n))) return rc;
    HIPCHK(c, hipMemcpyAsync(dli, Li, sizeof(double) * g.K * g.K, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemcpyAsync(dal, alpha, sizeof(double) * g.K, hipMemcpyHostToDevice, c->st));
    DISPATCH(c, weights, c, dli.p, dal.p, nsamp, seed, sw.z.p, sw.w.p, sw.wt.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->st));                     // dli, dal are released on return
    return SCFGP_OK;
}
static int sample_check(scfgp_ctx* c, bool ptrs_ok, int nsamp, const char* who) {
    if (!ptrs_ok) { c->err = std::string(who) + ": bad arguments"; return SCFGP_EARG; }
    if (nsamp < 1 || nsamp > SAMPLE_MAX) { c->err = std::string(who) + ": nsamp must lie in 1..1024"; return SCFGP_EARG; }
    return SCFGP_OK;
}

extern "C" int scfgp_sample_weights(scfgp_ctx* c, const double* alpha, const double* Li, int nsamp, uint64_t seed, double* W) {
    if (!c) return SCFGP_EARG;
    if (int rc = sample_check(c, alpha && Li && W, nsamp, "sample_weights")) return rc;
    if (int rc = need_model({c, "sample_weights"}, false)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    SampleW sw;
    if (int rc = sample_weights_dev(c, alpha, Li, nsamp, seed, sw)) return rc;
    HIPCHK(c, hipMemcpy2DAsync(W, sizeof(double) * nsamp, sw.w, sizeof(double) * sample_w_cols(nsamp), sizeof(double) * nsamp, c->g.K,
                               hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SCFGP_OK;
}

// The chunk pipeline (RowFeed, OutRing) with the X scaler in modes 1, 2; per chunk Phi* W into one of two staging buffers: device memory
// is two chunks of samples whatever T is.
extern "C" int scfgp_sample(scfgp_ctx* c, const double* Xs, int64_t T, const double* alpha, const double* Li, int nsamp, uint64_t seed,
                            int mode, int noise, double* out) {
    if (!c) return SCFGP_EARG;
    int rc;
    if ((rc = sample_check(c, Xs && alpha && Li && out && T >= 1 && mode >= 0 && mode <= 2, nsamp, "sample"))) return rc;
    if ((rc = need_model({c, "sample"}, mode >= 1, mode == 2))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const Geom& g0 = c->g;
    if ((rc = ensure_pred_chunk(c))) return rc;
    SampleW sw;
    if ((rc = sample_weights_dev(c, alpha, Li, nsamp, seed, sw))) return rc;
    const RowJobs jobs = {Xs, nullptr, T, PRED_ROWS};
    const int64_t rows = std::min<int64_t>(T, PRED_ROWS), nchunks = jobs.count();
    RowFeed feed; OutRing ring; DevTmp stage;                     // two chunks of Xs | two chunks of samples
    if ((rc = feed.open(c, PRED_ROWS * g0.D))) return rc;
    if ((rc = dmalloc(c, &stage.p, sizeof(double) * 2 * rows * nsamp))) return rc;
    if ((rc = ring.open(c))) return rc;
    auto slot = [&](int64_t i) { return stage + (i & 1) * rows * nsamp; };
    auto download = [&](int64_t i) {
        return ring.drain(i, [&]() -> int {
            HIPCHK(c, hipMemcpyAsync(out + jobs.row0(i) * nsamp, slot(i), sizeof(double) * jobs.rows(i) * nsamp, hipMemcpyDeviceToHost, c->copy_st));
            return SCFGP_OK;
        });
    };
    const int ymode = mode == 2 ? c->ys_mode : -1;
    if ((rc = feed.upload(0, jobs))) return rc;
    for (int64_t i = 0; i < nchunks; ++i) {
        const Geom g = chunk_geom(g0, jobs.rows(i));
        const double* x;
        if ((rc = feed.acquire(i, &x))) return rc;
        pack_chunk(c, g, x, nullptr, nullptr, nullptr, mode >= 1 ? c->xs_mode : 0, c->d_xscale);
        if ((rc = feed.release(i))) return rc;
        if ((rc = ring.acquire(i))) return rc;
        if ((rc = DISPATCH(c, sample_chunk, c, g, sw.wt.p, nsamp, jobs.row0(i), seed, noise, ymode, slot(i)))) return rc;
        if ((rc = ring.computed(i))) return rc;
        if (i + 1 < nchunks && (rc = feed.upload(i + 1, jobs))) return rc;
        if (i >= 1 && (rc = download(i - 1))) return rc;
    }
    if ((rc = download(nchunks - 1))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->copy_st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    return SCFGP_OK;
}

// scfgp_sample's pipeline without the OutRing: the weights w travel as the feed's targets and reach the product's epilogue through
// pack_data's zero-padded copy; per chunk the workgroups' records (two slots, alternating) are merged into nsamp running (value, row)
// pairs on the device.  The run owns its buffers: `best` (n = nsamp) is valid once the context's stream has drained.  xraw: the rows go
// through the registered X scaler.
struct SampleArgmaxRun {
    RowFeed feed; DevTmp wchunk, rec;                             // two chunks of [Xs | w] | w of the chunk, padded | records, running best, flag
    BestBlock best;
};
static int sample_argmax_run(scfgp_ctx* c, const double* Xs, int64_t T, const double* w, const void* Wt, int nsamp, bool xraw, int minimize,
                             SampleArgmaxRun& r) {
    const Geom& g0 = c->g;
    int rc;
    const RowJobs jobs = {Xs, w, T, PRED_ROWS};
    const int64_t nchunks = jobs.count();
    const int64_t nrec = sample_blocks(round_up(std::min<int64_t>(T, PRED_ROWS), 256), c->tsize()) * nsamp;      // records of a chunk
    if ((rc = r.feed.open(c, PRED_ROWS * (g0.D + (w ? 1 : 0))))) return rc;
    if (w && (rc = dmalloc(c, &r.wchunk.p, sizeof(double) * PRED_ROWS))) return rc;
    if ((rc = dmalloc(c, &r.rec.p, sizeof(double) * BestBlock::doubles(nsamp, nrec)))) return rc;
    r.best.carve(r.rec, nsamp, nrec);
    const BestBlock& best = r.best;
    if ((rc = best.clear(c))) return rc;
    if ((rc = r.feed.upload(0, jobs))) return rc;
    for (int64_t i = 0; i < nchunks; ++i) {
        const Geom g = chunk_geom(g0, jobs.rows(i));
        const double *x, *wraw;
        if ((rc = r.feed.acquire(i, &x, &wraw))) return rc;
        pack_chunk(c, g, x, w ? wraw : nullptr, nullptr, r.wchunk.p, xraw ? c->xs_mode : 0, c->d_xscale);
        if ((rc = r.feed.release(i))) return rc;
        const SampleArgmaxBufs b = {best.rec_v(i), best.rec_t(i), best.v(), best.t(), best.flag()};
        if ((rc = DISPATCH(c, sample_argmax_chunk, c, g, Wt, nsamp, r.wchunk.p, minimize, jobs.row0(i), b))) return rc;
        if (i + 1 < nchunks && (rc = r.feed.upload(i + 1, jobs))) return rc;
    }
    return SCFGP_OK;
}

// sample_argmax_run; the running best is all that the host fetches, once, with the non-finite flag.  w is checked on the host before
// any device work, as scfgp_select does.
extern "C" int scfgp_sample_argmax(scfgp_ctx* c, const double* Xs, int64_t T, const double* w, const double* alpha, const double* Li, int nsamp,
                                   uint64_t seed, int mode, int minimize, int64_t* idx, double* val) {
    if (!c) return SCFGP_EARG;
    int rc;
    if ((rc = sample_check(c, Xs && alpha && Li && idx && T >= 1 && mode >= 0 && mode <= 2, nsamp, "sample_argmax"))) return rc;
    const Fail fail = {c, "sample_argmax"};
    if ((rc = need_model(fail, mode >= 1, mode == 2))) return rc;
    if (w) {
        const WeightScan ws = scan_weights(w, T);
        if (ws.first_negative >= 0) return fail.arg("negative weight at row " + std::to_string(ws.first_negative));
        if (ws.first_nonfinite >= 0) return fail.nonfinite("non-finite rows, weights or factors");
        if (!ws.positive) return fail.arg("no row has a positive weight");
    }
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure_pred_chunk(c))) return rc;
    SampleW sw;
    if ((rc = sample_weights_dev(c, alpha, Li, nsamp, seed, sw))) return rc;
    SampleArgmaxRun run;
    if ((rc = sample_argmax_run(c, Xs, T, w, sw.wt.p, nsamp, mode >= 1, minimize, run))) return rc;
    if (mode == 2 && val) sample_argmax_finalize(run.best.v(), nsamp, c->ys_mode, c->d_yscale, c->d_sc, c->st);
    HIPCHK(c, hipGetLastError());
    std::vector<double> h(2 * nsamp + 1);                         // the outputs are written on success only
    if ((rc = run.best.fetch(c, h.data()))) return rc;
    if (run.best.host_flag(h.data())) return fail.nonfinite("non-finite rows, weights or factors");
    memcpy(idx, &h[nsamp], sizeof(int64_t) * nsamp);
    if (val) memcpy(val, h.data(), sizeof(double) * nsamp);
    return SCFGP_OK;
}

// predict_impl's pipeline (the factor pass, the feed of [Xs | w], mu / sd / acq of all T rows on the device until the end) with
// acquire.hip's kernels in rowpredict's place and scfgp_sample_argmax's running best and non-finite flag.  With grad, predict_grad_chunk
// gets the sigma in use as its sd, so its d sigma / d x is that sigma's; the combine runs before the X scaler's chain rule, which is
// linear per column.  par, fstar and w are checked on the host before any device work; the outputs are written on success only.
static constexpr int ACQUIRE_MAX_STAR = 1024;
extern "C" int scfgp_acquire(scfgp_ctx* c, const double* Xs, int64_t T, const double* w, const double* alpha, const double* Li, int kind,
                             const double* par, int npar, const double* fstar, int nstar, int mode, int noise, int minimize, double* acq,
                             int64_t* idx, double* val, double* mu, double* sd, double* grad) {
    if (!c) return SCFGP_EARG;
    const Fail fail = {c, "acquire"};
    if (!Xs || !alpha || !Li) return fail.arg("NULL Xs, alpha or Li");
    if (T < 1) return fail.arg("T must be at least 1");
    if (kind < 0 || kind > 4) return fail.arg("kind must lie in 0..4");
    if (mode < 0 || mode > 1) return fail.arg("mode must be 0 or 1 (there is no raw-y mode)");
    const int need = kind == 0 ? 1 : (kind == 4 ? 0 : 2);
    if (npar != need) return fail.arg("npar does not match the kind");
    if (need && !par) return fail.arg("NULL par");
    if (kind == 4 && (!fstar || nstar < 1 || nstar > ACQUIRE_MAX_STAR)) return fail.arg("MES needs fstar with 1 <= nstar <= 1024");
    if (kind != 4 && (fstar || nstar)) return fail.arg("fstar given for a kind other than MES");
    if (!acq && !idx && !grad) return fail.arg("no output requested (acq, idx and grad are all NULL)");
    if (val && !idx) return fail.arg("val without idx");
    int rc;
    if ((rc = need_model(fail, mode == 1))) return rc;
    AcquireSpec spec = {kind, {0.0, 0.0}, nullptr, kind == 4 ? nstar : 0, noise ? 1 : 0, minimize ? 1 : 0};
    bool nonfinite = false;
    for (int i = 0; i < need; ++i) { spec.par[i] = par[i]; if (!std::isfinite(par[i])) nonfinite = true; }
    for (int i = 0; i < spec.nstar; ++i) if (!std::isfinite(fstar[i])) nonfinite = true;
    if (!nonfinite && kind == 0 && par[0] < 0.0) return fail.arg("beta must not be negative");
    if (!nonfinite && (kind >= 1 && kind <= 3) && par[1] < 0.0) return fail.arg("xi must not be negative");
    if (w) {
        const WeightScan ws = scan_weights(w, T);
        if (ws.first_negative >= 0) return fail.arg("negative weight at row " + std::to_string(ws.first_negative));
        if (ws.first_nonfinite >= 0) nonfinite = true;
        if (!nonfinite && !ws.positive) return fail.arg("no row has a positive weight");
    }
    if (nonfinite) return fail.nonfinite("non-finite par, fstar or weights");
    HIPCHK(c, hipSetDevice(c->device));
    const Geom& g0 = c->g;
    if ((rc = ensure_pred_chunk(c))) return rc;
    if (grad && (rc = ensure_pred_grad(c, true))) return rc;
    const RowJobs jobs = {Xs, w, T, PRED_ROWS};
    const int64_t nchunks = jobs.count();
    const int64_t nrec = acquire_blocks(PRED_ROWS);
    RowFeed feed; DevTmp d_out, d_grad, work;     // Li / two chunks of [Xs | w] | mu, sd, acq of all T rows | grad of all T rows | chunk scratch
    if ((rc = feed.open(c, PRED_ROWS * (g0.D + (w ? 1 : 0)), (int64_t)g0.K * g0.K))) return rc;
    if ((rc = dmalloc(c, &d_out.p, sizeof(double) * 3 * T))) return rc;
    // work: w of the chunk, padded | a_u | a_sigma | d sigma / d x of the chunk | records of two chunks | running best, flag | fstar
    const int64_t n_dsd = grad ? PRED_ROWS * g0.D : 0;
    if ((rc = dmalloc(c, &work.p, sizeof(double) * (3 * PRED_ROWS + n_dsd + BestBlock::doubles(1, nrec) + ACQUIRE_MAX_STAR)))) return rc;
    double* d_mu = d_out; double* d_sd = d_out + T; double* d_acq = d_out + 2 * T;
    double* d_w = work; double* d_au = work + PRED_ROWS; double* d_as = work + 2 * PRED_ROWS; double* d_dsd = work + 3 * PRED_ROWS;
    BestBlock best;
    best.carve(d_dsd + n_dsd, 1, nrec);
    double* d_fstar = best.rec + BestBlock::doubles(1, nrec);
    if ((rc = best.clear(c))) return rc;
    if (kind == 4) {
        HIPCHK(c, hipMemcpyAsync(d_fstar, fstar, sizeof(double) * nstar, hipMemcpyHostToDevice, c->st));
        spec.fstar = d_fstar;
    }
    const void* LiT;
    if ((rc = load_factor(c, feed, Li, pad_square, false, alpha, &LiT))) return rc;
    if (grad) {
        if ((rc = dmalloc(c, &d_grad.p, sizeof(double) * T * g0.D))) return rc;
        DISPATCH(c, grad_operand, c);
        DISPATCH(c, type_factor, c, c->d_T1, nullptr, c->p_Li);
    }
    HIPCHK(c, hipStreamSynchronize(c->st));                     // raw is reused below
    if ((rc = feed.upload(0, jobs))) return rc;
    for (int64_t i = 0; i < nchunks; ++i) {
        const int64_t t0 = jobs.row0(i);
        const Geom g = chunk_geom(g0, jobs.rows(i));
        const double *x, *wraw;
        if ((rc = feed.acquire(i, &x, &wraw))) return rc;
        pack_chunk(c, g, x, w ? wraw : nullptr, nullptr, w ? d_w : nullptr, mode == 1 ? c->xs_mode : 0, c->d_xscale);
        if (!grad && (rc = feed.release(i))) return rc;
        const AcquireBufs b = {d_mu + t0, d_sd + t0, d_acq + t0, d_au, d_as, best.rec_v(i), best.rec_t(i), best.v(), best.t(), best.flag()};
        if ((rc = DISPATCH(c, acquire_chunk, c, g, LiT, spec, w ? d_w : nullptr, t0, b))) return rc;
        if (grad) {
            double* gm = d_grad + t0 * g0.D;
            if ((rc = DISPATCH(c, predict_grad_chunk, c, g, LiT, d_sd + t0, gm, d_dsd))) return rc;
            acquire_grad(g, b, spec.minimize, d_dsd, gm, c->st);
            if (mode == 1 && c->xs_mode) xgrad_chunk(x, g.N, g0.D, c->xs_mode, c->d_xscale, gm, nullptr, c->st);
            if ((rc = feed.release(i))) return rc;
        }
        if (i + 1 < nchunks && (rc = feed.upload(i + 1, jobs))) return rc;
    }
    HIPCHK(c, hipGetLastError());
    double h[3];                                                  // the running best and the flag first: the outputs are written on success only
    if ((rc = best.fetch(c, h))) return rc;
    if (best.host_flag(h)) return fail.nonfinite("an eligible row has a non-finite mu, sigma or value, or sigma = 0");
    if (acq) HIPCHK(c, hipMemcpyAsync(acq, d_acq, sizeof(double) * T, hipMemcpyDeviceToHost, c->st));
    if (mu) HIPCHK(c, hipMemcpyAsync(mu, d_mu, sizeof(double) * T, hipMemcpyDeviceToHost, c->st));
    if (sd) HIPCHK(c, hipMemcpyAsync(sd, d_sd, sizeof(double) * T, hipMemcpyDeviceToHost, c->st));
    if (grad) HIPCHK(c, hipMemcpyAsync(grad, d_grad, sizeof(double) * T * g0.D, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (idx) memcpy(idx, &h[1], sizeof(int64_t));
    if (val) val[0] = h[0];
    return SCFGP_OK;
}

// scfgp_acquire's pipeline with scfgp_predict_cov's first job: job 0 of the feed is the reference rows (Cb stays in p_V, d_r on the
// device), the chunks of [Xc | w] follow; each chunk's kg / kg_hi (and node table) join the call's T-sized arrays, its best eligible row
// the running best, through acquire.hip's argmax kernels (kg_hi in mu's place: an eligible row's kg, kg_hi and sigma must be finite,
// sigma not 0).  The symmetric form is the call with Xr = Xc.  z and w are checked on the host before any device work; the outputs are
// written on success only.
static constexpr int KG_MAX_NODES = 32;
extern "C" int scfgp_acquire_kg(scfgp_ctx* c, const double* Xc, int64_t T, const double* w, const double* Xr, int64_t R, const double* alpha,
                                const double* Li, const double* z, int J, int mode, int noise, int minimize, double* kg, double* kg_hi,
                                int64_t* idx, double* val, double* m, double* s) {
    if (!c) return SCFGP_EARG;
    const Fail fail = {c, "acquire_kg"};
    if (!Xc || !alpha || !Li || !z) return fail.arg("NULL Xc, alpha, Li or z");
    if (T < 1) return fail.arg("T must be at least 1");
    if (!Xr) {
        if (T > PRED_ROWS) return fail.arg("the symmetric form (Xr == NULL) takes 1..32768 rows");
        Xr = Xc; R = T;
    } else if (R < 1 || R > PRED_ROWS) return fail.arg("R must lie in 1..32768");
    if (J < 3 || J > KG_MAX_NODES) return fail.arg("J must lie in 3..32");
    if (mode < 0 || mode > 1) return fail.arg("mode must be 0 or 1 (there is no raw-y mode)");
    if (!kg && !kg_hi && !idx && !m && !s) return fail.arg("no output requested (kg, kg_hi, idx, m and s are all NULL)");
    if (val && !idx) return fail.arg("val without idx");
    int rc;
    if ((rc = need_model(fail, mode == 1))) return rc;
    bool nonfinite = false;
    for (int j = 0; j < J; ++j) if (!std::isfinite(z[j])) nonfinite = true;
    if (!nonfinite) {
        int zeros = z[0] == 0.0 ? 1 : 0;
        for (int j = 1; j < J; ++j) {
            if (!(z[j] > z[j - 1])) return fail.arg("the nodes must be strictly increasing");
            if (z[j] == 0.0) ++zeros;
        }
        if (zeros != 1) return fail.arg("exactly one node must be 0.0");
    }
    if (w) {
        const WeightScan ws = scan_weights(w, T);
        if (ws.first_negative >= 0) return fail.arg("negative weight at row " + std::to_string(ws.first_negative));
        if (ws.first_nonfinite >= 0) nonfinite = true;
        if (!nonfinite && !ws.positive) return fail.arg("no row has a positive weight");
    }
    if (nonfinite) return fail.nonfinite("non-finite nodes or weights");
    HIPCHK(c, hipSetDevice(c->device));
    const Geom& g0 = c->g;
    if ((rc = ensure_pred_chunk(c))) return rc;
    if ((rc = ensure_pred_factor(c))) return rc;
    const RowJobs jobs = {Xc, w, T, PRED_ROWS, Xr, R};              // job 0: the reference rows
    const int64_t njobs = jobs.count();
    const int64_t nrec = acquire_blocks(PRED_ROWS), SR = kg_state_rows();
    const bool table = m || s;
    RowFeed feed; DevTmp d_out, work;             // Li / two jobs of [X | w] | kg, kg_hi (and m, s) of all T rows | chunk scratch
    if ((rc = feed.open(c, PRED_ROWS * (g0.D + (w ? 1 : 0)), (int64_t)g0.K * g0.K))) return rc;
    if ((rc = dmalloc(c, &d_out.p, sizeof(double) * T * (2 + (table ? 2 * J : 0))))) return rc;
    // work: w of the chunk, padded | sigma of the chunk | d_r | z as given | nodes and h(-|z|) | records of two chunks | running best, flags |
    // bmin, bmax and the (m, s) states per row and column split
    if ((rc = dmalloc(c, &work.p, sizeof(double) * (3 * PRED_ROWS + 96 + BestBlock::doubles(1, nrec) + SR * (2 + 2 * J))))) return rc;
    double* d_kg = d_out; double* d_hi = d_out + T; double* d_m = table ? d_out + 2 * T : nullptr; double* d_s = table ? d_m + T * J : nullptr;
    double* d_w = work; double* d_sd = work + PRED_ROWS; double* d_d = work + 2 * PRED_ROWS; double* d_z = work + 3 * PRED_ROWS;
    double* d_zf = d_z + 32;
    BestBlock best;                                               // flag [0]: a candidate (acquire_argmax); [1]: a reference row
    best.carve(d_zf + 64, 1, nrec);
    double* d_stb = best.rec + BestBlock::doubles(1, nrec); double* d_stm = d_stb + 2 * SR; double* d_sts = d_stm + SR * J;
    if ((rc = best.clear(c))) return rc;
    HIPCHK(c, hipMemcpyAsync(d_z, z, sizeof(double) * J, hipMemcpyHostToDevice, c->st));
    const void* LiT;
    if ((rc = load_factor(c, feed, Li, pad_square, true, alpha, &LiT))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->st));                     // raw is reused below
    if ((rc = feed.upload(0, jobs))) return rc;
    for (int64_t job = 0; job < njobs; ++job) {
        const Geom g = chunk_geom(g0, jobs.rows(job));
        const double *x, *wraw;
        if ((rc = feed.acquire(job, &x, &wraw))) return rc;
        const bool cand = !jobs.lead(job);
        pack_chunk(c, g, x, cand && w ? wraw : nullptr, nullptr, cand && w ? d_w : nullptr, mode == 1 ? c->xs_mode : 0, c->d_xscale);
        if ((rc = feed.release(job))) return rc;
        const int64_t i = jobs.chunk(job), t0 = i * PRED_ROWS;
        const KgBufs b = {d_d, d_zf, d_sd, d_stm, d_sts, d_stb, cand ? d_kg + t0 : nullptr, cand ? d_hi + t0 : nullptr,
                          cand && table ? d_m + t0 * J : nullptr, cand && table ? d_s + t0 * J : nullptr};
        if (!cand) {
            if ((rc = DISPATCH(c, kg_ref_chunk, c, g, LiT, minimize ? 1 : 0, d_z, J, b, best.flag()))) return rc;
        } else {
            if ((rc = DISPATCH(c, kg_chunk, c, g, LiT, R, J, noise ? 1 : 0, b))) return rc;
            const AcquireBufs ab = {b.kg_hi, d_sd, b.kg, nullptr, nullptr, best.rec_v(i), best.rec_t(i), best.v(), best.t(), best.flag()};
            acquire_argmax(g, w ? d_w : nullptr, t0, i == 0, ab, c->st);
        }
        if (job + 1 < njobs && (rc = feed.upload(job + 1, jobs))) return rc;
    }
    HIPCHK(c, hipGetLastError());
    double h[3];                                                  // the running best and the flags first: the outputs are written on success only
    if ((rc = best.fetch(c, h))) return rc;
    if (best.host_flag(h, 1)) return fail.nonfinite("a reference row has a non-finite mean");
    if (best.host_flag(h, 0)) return fail.nonfinite("an eligible candidate has a non-finite value or sigma, or sigma = 0");
    if (kg) HIPCHK(c, hipMemcpyAsync(kg, d_kg, sizeof(double) * T, hipMemcpyDeviceToHost, c->st));
    if (kg_hi) HIPCHK(c, hipMemcpyAsync(kg_hi, d_hi, sizeof(double) * T, hipMemcpyDeviceToHost, c->st));
    if (m) HIPCHK(c, hipMemcpyAsync(m, d_m, sizeof(double) * T * J, hipMemcpyDeviceToHost, c->st));
    if (s) HIPCHK(c, hipMemcpyAsync(s, d_s, sizeof(double) * T * J, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (idx) memcpy(idx, &h[1], sizeof(int64_t));
    if (val) val[0] = h[0];
    return SCFGP_OK;
}

// scfgp_sample's pipeline (RowFeed, OutRing) with the weights given: W is uploaded and transposed once, the rows' sample indices travel
// as the feed's targets (doubles: exact below 1024) and reach the kernel through pack_data's zero-padded copy, and each chunk leaves
// [grad (rows x D) | val (rows)] in one of two staging slots.  W and sidx are checked on the host before any device work.
extern "C" int scfgp_sample_grad(scfgp_ctx* c, const double* Xs, int64_t T, const double* W, int nsamp, const int64_t* sidx, int mode,
                                 double* val, double* grad) {
    if (!c) return SCFGP_EARG;
    int rc;
    if ((rc = sample_check(c, Xs && W && grad && T >= 1 && mode >= 0 && mode <= 2, nsamp, "sample_grad"))) return rc;
    const Fail fail = {c, "sample_grad"};
    if ((rc = need_model(fail, mode >= 1, mode == 2))) return rc;
    const Geom& g0 = c->g;
    std::vector<double> hs;                                       // sidx as the feed's targets
    if (sidx) {
        hs.resize(T);
        for (int64_t t = 0; t < T; ++t) {
            if (sidx[t] < 0 || sidx[t] >= nsamp)
                return fail.arg("sample index " + std::to_string(sidx[t]) + " at row " + std::to_string(t) + " is outside [0, nsamp)");
            hs[t] = (double)sidx[t];
        }
    }
    for (int64_t e = 0, n = (int64_t)g0.K * nsamp; e < n; ++e)
        if (!std::isfinite(W[e])) return fail.nonfinite("non-finite weights");
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure_pred_chunk(c))) return rc;
    if ((rc = ensure_pred_grad(c, false))) return rc;
    DevTmp wraw, wt, schunk, stage;                               // W as uploaded | its transpose | sidx of the chunk, padded | two slots
    const int ldw = samplegrad_w_ld(g0.K);
    if ((rc = dmalloc(c, &wraw.p, sizeof(double) * g0.K * nsamp))) return rc;
    if ((rc = dmalloc(c, &wt.p, sizeof(double) * (int64_t)nsamp * ldw))) return rc;
    if (sidx && (rc = dmalloc(c, &schunk.p, sizeof(double) * PRED_ROWS))) return rc;
    HIPCHK(c, hipMemcpyAsync(wraw, W, sizeof(double) * g0.K * nsamp, hipMemcpyHostToDevice, c->st));
    samplegrad_weights(wraw, g0.K, nsamp, wt, c->st);
    DISPATCH(c, grad_operand, c);
    const RowJobs jobs = {Xs, sidx ? hs.data() : nullptr, T, PRED_ROWS};
    const int64_t rows = std::min<int64_t>(T, PRED_ROWS), nchunks = jobs.count(), slot_len = rows * (g0.D + 1);
    RowFeed feed; OutRing ring;
    if ((rc = feed.open(c, PRED_ROWS * (g0.D + (sidx ? 1 : 0))))) return rc;
    if ((rc = dmalloc(c, &stage.p, sizeof(double) * 2 * slot_len))) return rc;
    if ((rc = ring.open(c))) return rc;
    auto slot_grad = [&](int64_t i) { return stage + (i & 1) * slot_len; };
    auto slot_val = [&](int64_t i) { return stage + (i & 1) * slot_len + rows * g0.D; };
    auto download = [&](int64_t i) {
        return ring.drain(i, [&]() -> int {
            const int64_t t0 = jobs.row0(i), n = jobs.rows(i);
            HIPCHK(c, hipMemcpyAsync(grad + t0 * g0.D, slot_grad(i), sizeof(double) * n * g0.D, hipMemcpyDeviceToHost, c->copy_st));
            if (val) HIPCHK(c, hipMemcpyAsync(val + t0, slot_val(i), sizeof(double) * n, hipMemcpyDeviceToHost, c->copy_st));
            return SCFGP_OK;
        });
    };
    const int xmode = mode >= 1 ? c->xs_mode : 0;
    if ((rc = feed.upload(0, jobs))) return rc;
    for (int64_t i = 0; i < nchunks; ++i) {
        const Geom g = chunk_geom(g0, jobs.rows(i));
        const double *x, *sraw;
        if ((rc = feed.acquire(i, &x, &sraw))) return rc;
        pack_chunk(c, g, x, sidx ? sraw : nullptr, nullptr, schunk.p, xmode, c->d_xscale);
        if ((rc = ring.acquire(i))) return rc;
        if ((rc = DISPATCH(c, sample_grad_chunk, c, g, wt.p, schunk.p, jobs.row0(i), nsamp, slot_val(i), slot_grad(i)))) return rc;
        // the scalers' chain rules: the X scaler's at the raw inputs (still in the feed's half: it is released after them), the y
        // scaler's at the scaled value, which its backward transform then replaces
        if (xmode) xgrad_chunk(x, g.N, g0.D, xmode, c->d_xscale, slot_grad(i), nullptr, c->st);
        if ((rc = feed.release(i))) return rc;
        if (mode == 2) {
            ygrad_chunk(slot_val(i), nullptr, g.N, g0.D, c->ys_mode, c->d_yscale, slot_grad(i), nullptr, c->st);
            sample_argmax_finalize(slot_val(i), (int)g.N, c->ys_mode, c->d_yscale, c->d_sc, c->st);
        }
        if ((rc = ring.computed(i))) return rc;
        if (i + 1 < nchunks && (rc = feed.upload(i + 1, jobs))) return rc;
        if (i >= 1 && (rc = download(i - 1))) return rc;
    }
    if ((rc = download(nchunks - 1))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->copy_st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    return SCFGP_OK;
}

// ----------------------------------------------------------------------------------------------
// greedy maximum-information choice of m rows from a pool (select.hip; derivation in include/scfgp_hip.h)
// ----------------------------------------------------------------------------------------------
static constexpr int SELECT_MAX_M = 4096;
static constexpr int64_t SELECT_MAX_T = (int64_t)1 << 20;
static constexpr int SELECT_MAX_KP = 8192;                        // u_j lives in LDS as fp64: 64 KB dynamic beside the sweep's 128 B static
                                                                  // (65 664 B: gfx950 launches it without an opt-in, tests/test_gpu_select_bounds.py)
// The chunk pipeline (RowFeed) with the X scaler in mode 1; the chunk body is C = Phi_c Li^T, each chunk's C written to its place in a
// T x Kp buffer that this call owns.  Then d = rowsum(C^2) and m picks, every one of them a handful of eager launches on the context's
// stream (select.hip); the host waits once before the picks (for the non-finite flag of d) and once after them.  idx / var / gain are
// fetched at the end, std_after leaves on the copy stream.
extern "C" int scfgp_select(scfgp_ctx* c, const double* Xc, int64_t T, const double* w, const double* Li, int m, int mode, int64_t* idx,
                            double* var, double* gain, double* std_after) {
    if (!c) return SCFGP_EARG;
    if (!Xc || !Li || !idx || mode < 0 || mode > 1) { c->err = "select: bad arguments"; return SCFGP_EARG; }
    if (T < 1 || T > SELECT_MAX_T) { c->err = "select: T must lie in 1..1048576"; return SCFGP_EARG; }
    if (m < 1 || m > SELECT_MAX_M) { c->err = "select: m must lie in 1..4096"; return SCFGP_EARG; }
    const Fail fail = {c, "select"};
    int rc;
    if ((rc = need_model(fail, mode == 1))) return rc;
    if (c->g.Kp > SELECT_MAX_KP) return fail.arg("K above 8192 is not supported");
    int64_t eligible = T;
    if (w) {
        const WeightScan ws = scan_weights(w, T);
        if (ws.first_negative >= 0) return fail.arg("negative weight at row " + std::to_string(ws.first_negative));
        if (ws.first_nonfinite >= 0) return fail.nonfinite("non-finite rows, weights or factors");
        eligible = ws.positive;
    }
    if (m > eligible) return fail.arg("m = " + std::to_string(m) + " but only " + std::to_string(eligible) + " rows have a positive weight");
    HIPCHK(c, hipSetDevice(c->device));
    const Geom& g0 = c->g;
    const int64_t Kp = g0.Kp;
    const size_t ts = c->tsize();
    const RowJobs jobs = {Xc, nullptr, T, PRED_ROWS};
    const int64_t nchunks = jobs.count();
    // the last chunk's product writes whole 256-row blocks
    const int64_t Crows = jobs.row0(nchunks - 1) + round_up(jobs.rows(nchunks - 1), 256);
    if ((rc = ensure_pred_chunk(c))) return rc;
    if ((rc = ensure_pred_factor(c))) return rc;
    RowFeed feed; DevTmp Cbuf, rows, picks;                       // Li / two chunks of X | C | w, d, std, partials | U, cp, a, part, idx, var, gain, flag
    Events<1> sd_done;                                            // std_after is computed
    if ((rc = feed.open(c, PRED_ROWS * g0.D, (int64_t)g0.K * g0.K))) return rc;
    if (hipMalloc((void**)&Cbuf.p, ts * Crows * Kp) != hipSuccess) {
        (void)hipGetLastError();
        return fail.set("no device memory for the pool's factor (" + std::to_string(Crows) + " x " + std::to_string(Kp) + " x " +
                        std::to_string(ts) + " = " + std::to_string((unsigned long long)(ts * Crows * Kp)) + " bytes)", SCFGP_EHIP);
    }
    const int npart = select_partials(T), nlchunk = (m + 63) / 64;
    const int64_t npp = round_up(npart, 8), mp = round_up(m, 8);
    if ((rc = dmalloc(c, &rows.p, sizeof(double) * (3 * T + 2 * npp)))) return rc;
    if ((rc = dmalloc(c, &picks.p, sizeof(double) * ((int64_t)m * Kp + Kp + (int64_t)nlchunk * Kp + 4 * mp + 8)))) return rc;
    SelectBufs b;
    b.Kp = (int)Kp; b.Trows = T;
    b.w = rows; b.d = rows + T; double* d_sd = rows + 2 * T; b.pval = rows + 3 * T; b.pidx = (long long*)(rows + 3 * T + npp);
    b.U = picks; b.cp = b.U + (int64_t)m * Kp; b.part = b.cp + Kp; b.a = b.part + (int64_t)nlchunk * Kp;
    b.idx = (long long*)(b.a + mp); b.var = b.a + 2 * mp; b.gain = b.a + 3 * mp; b.flag = (int*)(b.a + 4 * mp);
    HIPCHK(c, hipMemsetAsync(Cbuf.p, 0, ts * Crows * Kp, c->st));   // the product leaves the padding columns K.. as they are: zero
    HIPCHK(c, hipMemsetAsync(b.flag, 0, sizeof(double), c->st));
    if (w) HIPCHK(c, hipMemcpyAsync(b.w, w, sizeof(double) * T, hipMemcpyHostToDevice, c->st));
    else select_ones(b.w, T, c->st);
    const void* LiT;
    if ((rc = load_factor(c, feed, Li, update_load_factor, true, nullptr, &LiT))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->st));                     // raw is reused below
    if ((rc = sd_done.create(c))) return rc;
    if ((rc = feed.upload(0, jobs))) return rc;
    for (int64_t i = 0; i < nchunks; ++i) {
        const Geom g = chunk_geom(g0, jobs.rows(i));
        const double* x;
        if ((rc = feed.acquire(i, &x))) return rc;
        pack_chunk(c, g, x, nullptr, nullptr, nullptr, mode == 1 ? c->xs_mode : 0, c->d_xscale);
        if ((rc = feed.release(i))) return rc;
        if ((rc = DISPATCH(c, cov_factor_chunk, c, g, LiT, (char*)Cbuf.p + ts * (size_t)jobs.row0(i) * Kp))) return rc;
        if (i + 1 < nchunks && (rc = feed.upload(i + 1, jobs))) return rc;
    }
    DISPATCH(c, pick_init, c, b, Cbuf.p);
    HIPCHK(c, hipGetLastError());
    int flag = 0;
    HIPCHK(c, hipMemcpyAsync(&flag, b.flag, sizeof(int), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->copy_st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (flag) { c->err = "select: non-finite rows, weights or factors"; return SCFGP_ENONFINITE; }
    for (int j = 0; j < m; ++j) DISPATCH(c, pick, c, b, Cbuf.p, j);
    HIPCHK(c, hipGetLastError());
    if (std_after) {
        select_std(b, c->d_sc, d_sd, c->st);
        HIPCHK(c, hipEventRecord(sd_done.e[0], c->st));
    }
    HIPCHK(c, hipMemcpyAsync(&flag, b.flag, sizeof(int), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    if (flag) { c->err = "select: non-finite rows, weights or factors"; return SCFGP_ENONFINITE; }
    if (std_after) {
        HIPCHK(c, hipStreamWaitEvent(c->copy_st, sd_done.e[0], 0));
        HIPCHK(c, hipMemcpyAsync(std_after, d_sd, sizeof(double) * T, hipMemcpyDeviceToHost, c->copy_st));
    }
    HIPCHK(c, hipMemcpyAsync(idx, b.idx, sizeof(int64_t) * m, hipMemcpyDeviceToHost, c->st));
    if (var) HIPCHK(c, hipMemcpyAsync(var, b.var, sizeof(double) * m, hipMemcpyDeviceToHost, c->st));
    if (gain) HIPCHK(c, hipMemcpyAsync(gain, b.gain, sizeof(double) * m, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->copy_st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SCFGP_OK;
}

// ----------------------------------------------------------------------------------------------
// greedy choice of m pool rows by integrated variance reduction (select.hip; derivation in include/scfgp_hip.h)
// ----------------------------------------------------------------------------------------------
static constexpr int SELECT_IV_MAX_KP = 4096;                     // u_j and v live in LDS as fp64: 64 KB
// scfgp_select's pipeline with one more product per chunk: the chunks of the reference rows (their weights travel as the feed's
// targets) go C = Phi_r Li^T -> packed C^T diag(omega) C, summed in fp64 over the chunks into Q; with Xr == NULL the pool's own chunks
// do, in the pass that fills the pool's C.  Then d, a = rowsum((C Q) o C) and m picks of eager launches (select.hip); the host waits
// once before the picks (for the non-finite flags) and once after them.
extern "C" int scfgp_select_iv(scfgp_ctx* c, const double* Xc, int64_t T, const double* w, const double* Xr, int64_t R, const double* wr,
                               const double* Li, int m, int mode, int64_t* idx, double* red, double* var, double* ivar, double* std_after) {
    if (!c) return SCFGP_EARG;
    if (!Xc || !Li || !idx || mode < 0 || mode > 1) { c->err = "select_iv: bad arguments"; return SCFGP_EARG; }
    if (T < 1 || T > SELECT_MAX_T) { c->err = "select_iv: T must lie in 1..1048576"; return SCFGP_EARG; }
    if (m < 1 || m > SELECT_MAX_M) { c->err = "select_iv: m must lie in 1..4096"; return SCFGP_EARG; }
    if (Xr && R < 1) { c->err = "select_iv: R must be at least 1"; return SCFGP_EARG; }
    const Fail fail = {c, "select_iv"};
    int rc;
    if ((rc = need_model(fail, mode == 1))) return rc;
    if (c->g.Kp > SELECT_IV_MAX_KP) return fail.arg("K above 4096 is not supported");
    const int64_t Rn = Xr ? R : T;
    bool nonfinite = false;
    int64_t eligible = T;
    if (w) {
        const WeightScan ws = scan_weights(w, T);
        if (ws.first_negative >= 0) return fail.arg("negative weight at row " + std::to_string(ws.first_negative));
        if (ws.first_nonfinite >= 0) nonfinite = true;
        eligible = ws.positive;
    }
    if (wr) {
        const WeightScan ws = scan_weights(wr, Rn);
        if (ws.first_negative >= 0) return fail.arg("negative reference weight at row " + std::to_string(ws.first_negative));
        if (ws.first_nonfinite >= 0) nonfinite = true;
        if (!nonfinite && !ws.positive) return fail.arg("no reference row has a positive weight");
    }
    if (nonfinite) return fail.nonfinite("non-finite rows, weights or factors");
    if (m > eligible) return fail.arg("m = " + std::to_string(m) + " but only " + std::to_string(eligible) + " rows have a positive weight");
    HIPCHK(c, hipSetDevice(c->device));
    const Geom& g0 = c->g;
    const int64_t Kp = g0.Kp, K2 = Kp * Kp;
    const size_t ts = c->tsize();
    // jobs 0 .. nref - 1: the chunks of the reference rows (their weights as targets); then the pool's, which carry wr where the pool is
    // its own reference
    const RowJobs ref = {Xr, wr, Xr ? R : 0, PRED_ROWS}, pool = {Xc, Xr ? nullptr : wr, T, PRED_ROWS};
    const int64_t npool = pool.count(), nref = ref.count(), njobs = nref + npool;
    const int64_t nqchunks = (Rn + PRED_ROWS - 1) / PRED_ROWS;
    // the last chunk's product writes whole 256-row blocks
    const int64_t Crows = pool.row0(npool - 1) + round_up(pool.rows(npool - 1), 256);
    if ((rc = ensure_pred_chunk(c))) return rc;
    if ((rc = ensure_pred_factor(c))) return rc;
    const int nts = (int)(Kp / g0.tile), ntiles = nts * (nts + 1) / 2;
    {   // slabs of the widest split among the chunk shapes of the reference rows (full chunks and the ragged last one)
        size_t need = 0;
        for (int64_t np : {round_up(std::min<int64_t>(Rn, PRED_ROWS), 256), round_up(Rn - (nqchunks - 1) * PRED_ROWS, 256)})
            need = std::max(need, sizeof(double) * (size_t)update_splits(c, np).nsplit * ((size_t)ntiles * g0.tile * g0.tile + Kp));
        if ((rc = ensure_update(c, need))) return rc;
    }
    RowFeed feed; DevTmp Cbuf, Qbuf, rows, picks;                 // Li / two chunks of [X | omega] | C | Q, typed Q | per row | per pick
    Events<1> sd_done;                                            // std_after is computed
    if ((rc = feed.open(c, PRED_ROWS * (g0.D + 1), (int64_t)g0.K * g0.K))) return rc;
    if (hipMalloc((void**)&Cbuf.p, ts * Crows * Kp) != hipSuccess) {
        (void)hipGetLastError();
        return fail.set("no device memory for the pool's factor (" + std::to_string(Crows) + " x " + std::to_string(Kp) + " x " +
                        std::to_string(ts) + " = " + std::to_string((unsigned long long)(ts * Crows * Kp)) + " bytes)", SCFGP_EHIP);
    }
    if ((rc = dmalloc(c, &Qbuf.p, (sizeof(double) + ts) * K2))) return rc;
    const int npart = select_partials(T), nlchunk = (m + 63) / 64;
    const int64_t npp = round_up(npart, 8), mp = round_up(m, 8), nat = select_iv_tiles((int)Kp);   // nat: the rows of apart
    if ((rc = dmalloc(c, &rows.p, sizeof(double) * ((4 + nat) * T + 2 * npp)))) return rc;
    if ((rc = dmalloc(c, &picks.p, sizeof(double) * ((int64_t)m * Kp + 3 * Kp + (int64_t)nlchunk * Kp + 5 * mp + 16)))) return rc;
    SelectBufs b; SelectIvBufs iv;
    b.Kp = (int)Kp; b.Trows = T;
    b.w = rows; b.d = rows + T; double* d_sd = rows + 2 * T; iv.a = rows + 3 * T; iv.apart = rows + 4 * T;
    b.pval = rows + (4 + nat) * T; b.pidx = (long long*)(b.pval + npp);
    b.U = picks; b.cp = b.U + (int64_t)m * Kp; iv.h = b.cp + Kp; iv.v = iv.h + Kp; b.part = iv.v + Kp; b.a = b.part + (int64_t)nlchunk * Kp;
    b.idx = (long long*)(b.a + mp); b.var = b.a + 2 * mp; b.gain = b.a + 3 * mp; iv.red = b.a + 4 * mp; iv.ivar = b.a + 5 * mp;
    b.flag = (int*)(iv.ivar + 8);                                 // [0]: select.hip's bits, [1]: update_check_finite's
    iv.Q = Qbuf;
    void* Qt = (void*)(Qbuf.p + K2);
    HIPCHK(c, hipMemsetAsync(Cbuf.p, 0, ts * Crows * Kp, c->st));   // the product leaves the padding columns K.. as they are: zero
    HIPCHK(c, hipMemsetAsync(b.flag, 0, sizeof(double), c->st));
    if (w) HIPCHK(c, hipMemcpyAsync(b.w, w, sizeof(double) * T, hipMemcpyHostToDevice, c->st));
    else select_ones(b.w, T, c->st);
    const void* LiT;
    if ((rc = load_factor(c, feed, Li, update_load_factor, true, nullptr, &LiT))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->st));                     // raw is reused below
    if ((rc = sd_done.create(c))) return rc;
    auto upload = [&](int64_t job) { return job < nref ? feed.upload(job, ref) : feed.upload(job - nref, pool, nref); };
    if ((rc = upload(0))) return rc;
    int64_t nq = 0;                                               // chunks summed into Q so far
    for (int64_t job = 0; job < njobs; ++job) {
        const Geom g = chunk_geom(g0, job < nref ? ref.rows(job) : pool.rows(job - nref));
        const bool in_q = job < nref || !Xr, weighted = in_q && wr;
        const double *x, *om;
        if ((rc = feed.acquire(job, &x, &om))) return rc;
        pack_chunk(c, g, x, weighted ? om : nullptr, nullptr, weighted ? c->u_y : nullptr, mode == 1 ? c->xs_mode : 0, c->d_xscale);
        if ((rc = feed.release(job))) return rc;
        void* Cj = job < nref ? c->p_C : (void*)((char*)Cbuf.p + ts * (size_t)((job - nref) * PRED_ROWS) * Kp);
        if ((rc = DISPATCH(c, cov_factor_chunk, c, g, LiT, Cj))) return rc;
        if (in_q) {
            if ((rc = DISPATCH(c, iv_gram_chunk, c, g, update_splits(c, g.Np), Cj, weighted ? c->u_y : nullptr, nq == 0 ? c->u_acc : c->u_part)))
                return rc;
            if (nq > 0) update_accumulate(c->u_acc, c->u_part, c->n_pk, c->st);
            ++nq;
        }
        if (job + 1 < njobs && (rc = upload(job + 1))) return rc;
    }
    // non-finite reference rows have reached Q by now; the pool's show in d and a
    update_check_finite(c->u_acc, c->n_pk, b.flag, c->st);
    unpack_tri_tiles(c->u_acc, nts, g0.tile, Qbuf, Kp, c->st);
    DISPATCH(c, iv_init, c, b, iv, Cbuf.p, Qt);
    HIPCHK(c, hipGetLastError());
    int flags[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(flags, b.flag, sizeof(flags), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->copy_st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (flags[0] || flags[1]) { c->err = "select_iv: non-finite rows, weights or factors"; return SCFGP_ENONFINITE; }
    for (int j = 0; j < m; ++j) DISPATCH(c, iv_pick, c, b, iv, Cbuf.p, j);
    HIPCHK(c, hipGetLastError());
    if (std_after) {
        select_std(b, c->d_sc, d_sd, c->st);
        HIPCHK(c, hipEventRecord(sd_done.e[0], c->st));
    }
    HIPCHK(c, hipMemcpyAsync(flags, b.flag, sizeof(flags), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    if (flags[0] || flags[1]) { c->err = "select_iv: non-finite rows, weights or factors"; return SCFGP_ENONFINITE; }
    if (std_after) {
        HIPCHK(c, hipStreamWaitEvent(c->copy_st, sd_done.e[0], 0));
        HIPCHK(c, hipMemcpyAsync(std_after, d_sd, sizeof(double) * T, hipMemcpyDeviceToHost, c->copy_st));
    }
    HIPCHK(c, hipMemcpyAsync(idx, b.idx, sizeof(int64_t) * m, hipMemcpyDeviceToHost, c->st));
    if (red) HIPCHK(c, hipMemcpyAsync(red, iv.red, sizeof(double) * m, hipMemcpyDeviceToHost, c->st));
    if (var) HIPCHK(c, hipMemcpyAsync(var, b.var, sizeof(double) * m, hipMemcpyDeviceToHost, c->st));
    if (ivar) HIPCHK(c, hipMemcpyAsync(ivar, iv.ivar, sizeof(double) * 2, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->copy_st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SCFGP_OK;
}

// ----------------------------------------------------------------------------------------------
// greedy Monte-Carlo batch expected improvement over a pool (selectqei.hip; formulas in include/scfgp_hip.h)
// ----------------------------------------------------------------------------------------------
// The pending rows go through sample_argmax_run (their per-sample best values are the start of m); the pool goes through scfgp_sample's
// chunk body with each chunk's block written to its place in a T x nsamp buffer that this call owns.  Then m picks of two eager launches
// each on the context's stream (selectqei.hip); the host waits once after the first sweep (for the non-finite flags) and once at the end.
extern "C" int scfgp_select_qei(scfgp_ctx* c, const double* Xc, int64_t T, const double* w, const double* Xp, int64_t np, const double* alpha,
                                const double* Li, int nsamp, uint64_t seed, double best, double xi, int m, int mode, int minimize,
                                int64_t* idx, double* gain, double* score0, double* mstate, double* qei) {
    if (!c) return SCFGP_EARG;
    const Fail fail = {c, "select_qei"};
    if (!Xc || !alpha || !Li || !idx) return fail.arg("NULL Xc, alpha, Li or idx");
    if (T < 1 || T > SELECT_MAX_T) return fail.arg("T must lie in 1..1048576");
    if (m < 1 || m > SELECT_MAX_M) return fail.arg("m must lie in 1..4096");
    if (nsamp < 1 || nsamp > SAMPLE_MAX) return fail.arg("nsamp must lie in 1..1024");
    if (mode < 0 || mode > 1) return fail.arg("mode must be 0 or 1 (there is no raw-y mode)");
    if (np < 0) return fail.arg("np must not be negative");
    if (np > 0 && !Xp) return fail.arg("np > 0 with NULL Xp");
    int rc;
    if ((rc = need_model(fail, mode == 1))) return rc;
    bool nonfinite = !std::isfinite(best) || !std::isfinite(xi);
    if (!nonfinite && xi < 0.0) return fail.arg("xi must not be negative");
    int64_t eligible = T;
    if (w) {
        const WeightScan ws = scan_weights(w, T);
        if (ws.first_negative >= 0) return fail.arg("negative weight at row " + std::to_string(ws.first_negative));
        if (ws.first_nonfinite >= 0) nonfinite = true;
        eligible = ws.positive;
    }
    if (nonfinite) return fail.nonfinite("non-finite best, xi or weights");
    if (m > eligible) return fail.arg("m = " + std::to_string(m) + " but only " + std::to_string(eligible) + " rows have a positive weight");
    HIPCHK(c, hipSetDevice(c->device));
    const Geom& g0 = c->g;
    if ((rc = ensure_pred_chunk(c))) return rc;
    SampleW sw;
    if ((rc = sample_weights_dev(c, alpha, Li, nsamp, seed, sw))) return rc;
    RowFeed feed; DevTmp Fbuf, state;                             // two chunks of Xc | F | w, score0, m, records, idx, gain, qei, flag
    if ((rc = feed.open(c, PRED_ROWS * g0.D))) return rc;
    if (hipMalloc((void**)&Fbuf.p, sizeof(double) * T * nsamp) != hipSuccess) {
        (void)hipGetLastError();
        return fail.set("no device memory for the pool's samples (" + std::to_string(T) + " x " + std::to_string(nsamp) + " x 8 = " +
                        std::to_string((unsigned long long)(sizeof(double) * T * nsamp)) + " bytes)", SCFGP_EHIP);
    }
    const int64_t nblk = selectqei_blocks(T), mp = round_up(m, 8);
    if ((rc = dmalloc(c, &state.p, sizeof(double) * (2 * T + nsamp + 2 * nblk + 2 * mp + 3)))) return rc;
    SelectQeiBufs b;
    b.F = Fbuf; b.T = T; b.nsamp = nsamp; b.sgn = minimize ? -1.0 : 1.0;
    b.w = state; b.score0 = b.w + T; b.ms = b.score0 + T; b.pval = b.ms + nsamp; b.pidx = (long long*)(b.pval + nblk);
    b.idx = (long long*)(b.pval + 2 * nblk); b.gain = b.pval + 2 * nblk + mp; b.qei = b.gain + mp; b.flag = (int*)(b.qei + 2);
    HIPCHK(c, hipMemsetAsync(b.flag, 0, sizeof(double), c->st));
    if (w) HIPCHK(c, hipMemcpyAsync(b.w, w, sizeof(double) * T, hipMemcpyHostToDevice, c->st));
    else select_ones(b.w, T, c->st);
    SampleArgmaxRun pend;                                         // the pending rows: every one of them is eligible
    if (np > 0 && (rc = sample_argmax_run(c, Xp, np, nullptr, sw.wt.p, nsamp, mode == 1, minimize, pend))) return rc;
    const RowJobs jobs = {Xc, nullptr, T, PRED_ROWS};
    const int64_t nchunks = jobs.count();
    if ((rc = feed.upload(0, jobs))) return rc;
    for (int64_t i = 0; i < nchunks; ++i) {
        const Geom g = chunk_geom(g0, jobs.rows(i));
        const double* x;
        if ((rc = feed.acquire(i, &x))) return rc;
        pack_chunk(c, g, x, nullptr, nullptr, nullptr, mode == 1 ? c->xs_mode : 0, c->d_xscale);
        if ((rc = feed.release(i))) return rc;
        if ((rc = DISPATCH(c, sample_chunk, c, g, sw.wt.p, nsamp, jobs.row0(i), seed, 0, -1, Fbuf + jobs.row0(i) * nsamp))) return rc;
        if (i + 1 < nchunks && (rc = feed.upload(i + 1, jobs))) return rc;
    }
    const double base = b.sgn * best + xi;
    selectqei_state(b, np > 0 ? pend.best.v() : nullptr, base, 1, c->st);
    selectqei_sweep(b, 0, c->st);
    HIPCHK(c, hipGetLastError());
    int flags[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(&flags[0], b.flag, sizeof(int), hipMemcpyDeviceToHost, c->st));
    if (np > 0) HIPCHK(c, hipMemcpyAsync(&flags[1], pend.best.flag(), sizeof(int), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->copy_st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (flags[0] || flags[1]) { c->err = "select_qei: a non-finite sampled value at an eligible or pending row"; return SCFGP_ENONFINITE; }
    for (int j = 0; j < m; ++j) {
        if (j) selectqei_sweep(b, j, c->st);
        selectqei_commit(b, j, c->st);
    }
    selectqei_state(b, nullptr, base, 0, c->st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(idx, b.idx, sizeof(int64_t) * m, hipMemcpyDeviceToHost, c->st));
    if (gain) HIPCHK(c, hipMemcpyAsync(gain, b.gain, sizeof(double) * m, hipMemcpyDeviceToHost, c->st));
    if (score0) HIPCHK(c, hipMemcpyAsync(score0, b.score0, sizeof(double) * T, hipMemcpyDeviceToHost, c->st));
    if (mstate) HIPCHK(c, hipMemcpyAsync(mstate, b.ms, sizeof(double) * nsamp, hipMemcpyDeviceToHost, c->st));
    if (qei) HIPCHK(c, hipMemcpyAsync(qei, b.qei, sizeof(double) * 2, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SCFGP_OK;
}
