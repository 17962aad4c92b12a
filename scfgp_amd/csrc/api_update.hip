// C ABI of libscfgp_hip.so, the entry points that change or leave out observations of a fitted posterior: scfgp_condition,
// scfgp_condition_grad, scfgp_forget and scfgp_loo.
#include "api_chunks.h"

// typed operands of the first pass of scfgp_condition / scfgp_forget (UpdateImpl::update_chunk): Phi and C of a chunk (PRED_ROWS x Kp,
// padding columns zero), the factor's transpose and the factor (Kp x Kp)
struct UpdateOperands { void *Phi, *C, *LiT, *Li; };

// chunk bodies of this file's entry points; those that other files call too are ChunkImpl's (api_chunks.h)
template <typename T> struct UpdateImpl : ChunkImpl<T> {
    typedef SweepKernels<T> SK;
    using ChunkImpl<T>::features;
    using ChunkImpl<T>::factor_c;
    // scfgp_condition, scfgp_forget: C = Phi_n Li^T with the update's own factor and alpha (o.LiT / o.Li, u_vec), the residual
    // r = y - Phi_n alpha, then [packed lower tiles of C^T C | C^T r] of the chunk into `out` by the evaluation's Gram tiles on the
    // chunk's geometry with the update's own slabs: fp64 MFMA, or exact fp32 MFMA flushed into the fp64 slabs every gram_chunk rows
    // (never the fp16 split: an f16x3 context runs fp32 mode's kernels here).  The typed operands come with the call (UpdateOperands):
    // scfgp_forget runs the fp64 arm on buffers of its own in an fp32 context.
    // have_rows: o.Phi and u_y already hold the chunk's rows and targets (scfgp_condition_grad: gradobs_chunk)
    static int update_chunk(scfgp_ctx* c, const Geom& g, const RowSplits& rs, const UpdateOperands& o, double* out, bool have_rows = false) {
        if (!have_rows) SK::featuremap(g, c->p_Xt, Projection{c->d_Fall, c->d_Lall, c->d_Rall, c->p_Tt}, c->d_sc, (T*)o.Phi, c->st);
        SK::apply_c(g, (const T*)o.Phi, (const T*)o.LiT, (const T*)o.Li, (T*)o.C, c->p_vpart, c->u_vec, c->u_vec, c->p_mupart, c->st, 0);
        SK::rowresidual(g, c->p_mupart, c->u_y, c->u_r, c->st);
        const int nts = g.Kp / g.tile, ntiles = nts * (nts + 1) / 2;
        double* sidepart = c->u_slabs + (size_t)rs.nsplit * ntiles * g.tile * g.tile;
        SK::gram(g, (const T*)o.C, nullptr, c->u_r, rs, sizeof(T) == 4 ? c->gram_chunk : 0, c->u_slabs, sidepart, c->u_flag + 8, c->u_ws2, c->st);
        reduce_tri_tiles(c->u_slabs, rs.nsplit, nts, g.tile, out, c->st);
        reduce_side(sidepart, rs.nsplit, g.Kp, g.gfull * g.tile + g.gstrip * 64, out + c->n_pk, c->st);
        HIPCHK(c, hipGetLastError());
        return SCFGP_OK;
    }
    // scfgp_condition_grad (condgrad.hip): Phi of the chunk's g.N packed points into o.C (which the product that follows overwrites), then
    // their gr.N observation rows into o.Phi and the rows' targets into u_y, where update_chunk (have_rows) finds them
    static int gradobs_chunk(scfgp_ctx* c, const Geom& g, const Geom& gr, const UpdateOperands& o, const GradObs& a) {
        { ProfScope ps(c, "gradobs_featuremap");
          SK::featuremap(g, c->p_Xt, Projection{c->d_Fall, c->d_Lall, c->d_Rall, c->p_Tt}, c->d_sc, (T*)o.C, c->st); }
        { ProfScope ps(c, "gradobs_rows"); gradobs_rows<T>(gr, g, (const T*)o.C, c->d_Fall, a, (T*)o.Phi, c->u_y, c->st); }
        HIPCHK(c, hipGetLastError());
        return SCFGP_OK;
    }
    // scfgp_loo: C = Phi_I Li^T and r = y - Phi_I alpha of the chunk's rows, then the block kernel and the ordered sum of its records
    // (loo.hip)
    static int loo_chunk(scfgp_ctx* c, const Geom& g, const void* LiT, int block, int64_t blk0, double* mu, double* sd, double* lev) {
        features(c, g);
        factor_c(c, g, (const T*)LiT, c->alpha_pred(), (T*)c->p_C);
        SK::rowresidual(g, c->p_mupart, c->l_y, c->l_r, c->st);
        loo_blocks<T>(g, (const T*)c->p_C, c->l_r, c->l_y, block, blk0, c->d_sc, mu, sd, lev, c->l_rec, c->l_acc, c->l_bad, c->st);
        HIPCHK(c, hipGetLastError());
        return SCFGP_OK;
    }
};
#define DISPATCH(c, fn, ...) DISPATCH_TO(UpdateImpl, c, fn, __VA_ARGS__)

// ----------------------------------------------------------------------------------------------
// absorbing new observations into a fitted posterior (kernels_kstage.hip: kstage_update; derivation in include/scfgp_hip.h)
// ----------------------------------------------------------------------------------------------
// The first pass of scfgp_condition and scfgp_forget: the chunk pipeline (RowFeed) with the targets behind the rows of their chunk and
// the X scaler in mode 1.  The factors are loaded into the update's buffers (u_Li, u_LiT, alpha at u_vec), then each chunk adds its
// C^T C and C^T r to a running fp64 sum in u_acc and, rr != NULL, its r^T r to rr[0].  u_flag[0..3] are cleared first; u_flag[1] tells
// of non-finite rows, targets or factors.  `feed` is opened here and stays open for the caller.  wide != NULL (fp32 contexts only): the
// pass runs the fp64 kernels on these operands.
//
// How a chunk's rows and targets are produced is the caller's: produce(i, g, x, targets, ops, &have_rows) packs job i (g: its geometry
// in points; x, targets: its place in the feed), releases the feed's half when the raw rows have been read, and either leaves the
// feature map to update_chunk (the packed rows ARE the update's rows, targets in u_y) or writes the rows of the update itself into
// ops.Phi and u_y (have_rows; rpp of them per point: scfgp_condition_grad).
template <typename Produce>
static int update_gather(scfgp_ctx* c, RowFeed& feed, const RowJobs& jobs, int64_t rpp, const double* alpha, const double* Li, double* rr,
                         const UpdateOperands* wide, Produce produce) {
    const Geom& g0 = c->g;
    const int64_t Kp = g0.Kp;
    const int64_t nchunks = jobs.count(), n = jobs.n * rpp, CHR = jobs.CH * rpp;      // the update's rows: in all, per full chunk
    int rc;
    if ((rc = ensure_pred_chunk(c))) return rc;
    if ((rc = ensure_pred_factor(c))) return rc;
    {   // slabs of the widest split among the call's chunk shapes (full chunks and the ragged last one)
        const int nts = Kp / g0.tile, ntiles = nts * (nts + 1) / 2;
        size_t need = 0;
        for (int64_t np : {round_up(std::min<int64_t>(n, CHR), 256), round_up(n - (nchunks - 1) * CHR, 256)})
            need = std::max(need, sizeof(double) * (size_t)update_splits(c, np, wide).nsplit * ((size_t)ntiles * g0.tile * g0.tile + Kp));
        if ((rc = ensure_update(c, need))) return rc;
    }
    const UpdateOperands own = {c->p_Phi, c->p_C, c->u_LiT, c->p_Li};
    const UpdateOperands& ops = wide ? *wide : own;
    // Li in host layout (in, then out) / two chunks of [X | y]
    if ((rc = feed.open(c, PRED_ROWS * g0.D + jobs.CH * std::max<int64_t>(1, jobs.target_width()), (int64_t)g0.K * g0.K))) return rc;
    HIPCHK(c, hipMemsetAsync(c->u_flag, 0, sizeof(int) * 4, c->st));
    if (rr) HIPCHK(c, hipMemsetAsync(rr, 0, sizeof(double), c->st));
    if ((rc = load_factor(c, feed.raw, Li, update_load_factor, c->u_Li, wide ? nullptr : ops.LiT, wide ? nullptr : ops.Li, alpha, c->u_vec,
                          c->u_flag))) return rc;
    if (wide) UpdateImpl<double>::type_factor(c, c->u_Li, ops.LiT, ops.Li);
    HIPCHK(c, hipStreamSynchronize(c->st));                     // raw is reused below
    if ((rc = feed.upload(0, jobs))) return rc;
    for (int64_t i = 0; i < nchunks; ++i) {
        const Geom gp = chunk_geom(g0, jobs.rows(i));
        const double *x, *yi;
        if ((rc = feed.acquire(i, &x, &yi))) return rc;
        bool have_rows = false;
        if ((rc = produce(i, gp, x, yi, ops, &have_rows))) return rc;
        const Geom g = have_rows ? chunk_geom(g0, jobs.rows(i) * rpp) : gp;
        double* out = i == 0 ? c->u_acc : c->u_part;
        if ((rc = wide ? UpdateImpl<double>::update_chunk(c, g, update_splits(c, g.Np, true), ops, out, have_rows)
                       : DISPATCH(c, update_chunk, c, g, update_splits(c, g.Np), ops, out, have_rows))) return rc;
        if (i > 0) update_accumulate(c->u_acc, c->u_part, c->n_pk + Kp, c->st);
        if (rr) update_sumsq(c->u_r, g.N, rr, c->st);
        if (i + 1 < nchunks && (rc = feed.upload(i + 1, jobs))) return rc;
    }
    // non-finite rows or targets have reached C^T C or C^T r by now
    update_check_finite(c->u_acc, c->n_pk + Kp, c->u_flag, c->st);
    return SCFGP_OK;
}
// scfgp_condition, scfgp_forget: the n rows (X, y) in chunks of PRED_ROWS are the update's rows
static int update_gather(scfgp_ctx* c, RowFeed& feed, const double* X, const double* y, int64_t n, const double* alpha, const double* Li,
                         int mode, double* rr, const UpdateOperands* wide = nullptr) {
    const RowJobs jobs = {X, y, n, PRED_ROWS};
    return update_gather(c, feed, jobs, 1, alpha, Li, rr, wide,
                         [&](int64_t i, const Geom& g, const double* x, const double* yi, const UpdateOperands&, bool*) {
                             pack_chunk(c, g, x, yi, nullptr, c->u_y, mode == 1 ? c->xs_mode : 0, c->d_xscale);
                             return feed.release(i);
                         });
}
static KUpdate update_buffers(scfgp_ctx* c) {
    const int64_t Kp = c->g.Kp;
    KUpdate k;
    k.K = c->g.K; k.Kp = c->g.Kp; k.packed = c->u_acc; k.n_pk = c->n_pk; k.Li = c->u_Li; k.alpha = c->u_vec; k.S = c->u_S; k.Lm = c->u_Lm;
    k.Mi = c->u_Mi; k.Si = c->u_Si; k.gamma = c->u_vec + Kp; k.alpha_out = c->u_vec + 2 * Kp; k.part = c->u_vec + 3 * Kp; k.flag = c->u_flag;
    return k;
}

// One K x K stage turns the first pass's sum into the new factors, which leave through the feed's buffer.  The outputs are fetched only
// when the stage succeeded.  who, what: the entry point and its name for the targets in the error texts
static int update_finish(scfgp_ctx* c, RowFeed& feed, const char* who, const char* what, double* alpha_out, double* Li_out) {
    const Geom& g0 = c->g;
    const int64_t Kp = g0.Kp, K2 = Kp * Kp;
    const Fail fail = {c, who};
    const KUpdate k = update_buffers(c);
    kstage_update(k, c->st);
    // u_flag[1]: what went in; u_flag[2]: what came out, as in scfgp_forget: a factorisation that failed leaves NaN behind, which is
    // u_flag[0]'s to tell (an fp32 context's C^T C is off by eps32 |S|, which reaches the unit eigenvalues of S once |S| nears 1 / eps32)
    update_check_finite(c->u_S, K2, c->u_flag + 1, c->st);
    update_check_finite(k.alpha_out, Kp, c->u_flag + 1, c->st);
    update_store_factor(c->u_S, g0.K, g0.Kp, feed.raw, c->st);
    HIPCHK(c, hipGetLastError());
    int flags[3] = {0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(flags, c->u_flag, sizeof(flags), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (flags[1]) return fail.nonfinite(std::string("non-finite rows, ") + what + " or factors");
    if (flags[0]) return fail.set("I + C^T C is not positive definite", SCFGP_ENOTPD);
    if (flags[2]) return fail.nonfinite("the updated factors are not finite");
    HIPCHK(c, hipMemcpyAsync(Li_out, feed.raw, sizeof(double) * g0.K * g0.K, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(alpha_out, k.alpha_out, sizeof(double) * g0.K, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SCFGP_OK;
}
extern "C" int scfgp_condition(scfgp_ctx* c, const double* Xn, const double* yn, int64_t n, const double* alpha, const double* Li, int mode,
                               double* alpha_out, double* Li_out) {
    if (!c) return SCFGP_EARG;
    if (!Xn || !yn || !alpha || !Li || !alpha_out || !Li_out || mode < 0 || mode > 1) { c->err = "condition: bad arguments"; return SCFGP_EARG; }
    if (n < 1) { c->err = "condition: n must be at least 1"; return SCFGP_EARG; }
    int rc;
    if ((rc = need_model({c, "condition"}, mode == 1))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    RowFeed feed;
    if ((rc = update_gather(c, feed, Xn, yn, n, alpha, Li, mode, nullptr))) return rc;
    return update_finish(c, feed, "condition", "targets", alpha_out, Li_out);
}

// ----------------------------------------------------------------------------------------------
// absorbing derivative observations into a fitted posterior (condgrad.hip; derivation and promises in include/scfgp_hip.h)
// ----------------------------------------------------------------------------------------------
// scfgp_condition's path with another producer of a chunk's rows: a chunk holds whole points, np = PRED_ROWS / nb of them (GradBlocks,
// api_host.h), whose features are expanded into nb observation rows each (UpdateImpl::gradobs_chunk).  A job uploads [X | yn | Gn | rho] of its
// points; the raw rows stay in the feed's half until the scaler's factors g_t have been formed from them (mode 1) and the targets
// until the row kernel has read them.  In fp32 contexts the first pass is the fp64 one on scfgp_forget's buffers, as there: a derivative
// row is |F_all[d, :]| sqrt(rho / J) times as long as a value row, the rounding errors of the fp32 products grow with its square, and
// the predictions feel them (DESIGN 4.20 has the measured ratios).
static int ensure_forget(scfgp_ctx* c);
extern "C" int scfgp_condition_grad(scfgp_ctx* c, const double* Xn, int64_t n, const int32_t* dims, int nd, const double* Gn, const double* rho,
                                    const double* yn, const double* alpha, const double* Li, int mode, double* alpha_out, double* Li_out) {
    if (!c) return SCFGP_EARG;
    const Fail fail = {c, "condition_grad"};
    if (!Xn || !Gn || !alpha || !Li || !alpha_out || !Li_out) return fail.arg("bad arguments");
    if (n < 1) return fail.arg("n must be at least 1");
    const Geom& g0 = c->g;
    const int D = g0.D;
    if (nd < 1 || nd > D) return fail.arg("nd must lie in 1..D");
    const GradBlocks gb = {nd, yn != nullptr, rho != nullptr};
    if (gb.nb() > PRED_ROWS) return fail.arg("the rows of a point (nd, and one for its value) must not exceed 32768");
    if (!dims && nd != D) return fail.arg("dims == NULL needs nd == D");
    if (dims) {
        std::vector<char> seen(D);
        const int j = first_bad_dim(dims, nd, D, seen.data());
        if (j >= 0) return fail.arg("dims[" + std::to_string(j) + "] is out of range or repeated");
    }
    if (mode < 0 || mode > 1) return fail.arg("bad mode");
    int rc;
    if ((rc = need_model(fail, mode == 1))) return rc;
    if (rho) {
        const WeightScan ws = scan_weights(rho, n * nd);
        auto at = [&](int64_t e) { return "rho[" + std::to_string(e / nd) + ", " + std::to_string(e % nd) + "]"; };
        if (ws.first_negative >= 0) return fail.arg(at(ws.first_negative) + " is negative");
        if (ws.first_nonfinite >= 0) return fail.nonfinite(at(ws.first_nonfinite) + " is not finite");
        if (!yn && ws.positive == 0) return fail.arg("every rho is zero and no values are given");
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (c->prof) { c->recs.clear(); c->pool_used = 0; }          // timings describe this call's chunks (tools/condition_grad_time.py)
    const int xmode = mode == 1 ? c->xs_mode : 0;
    const RowJobs jobs = gb.jobs(Xn, yn, Gn, rho, n, PRED_ROWS);
    DevTmp d_dims, gfac;                                          // dims | g_t of a chunk's points
    if (dims) {
        if ((rc = dmalloc(c, &d_dims.p, sizeof(int) * nd))) return rc;
        HIPCHK(c, hipMemcpyAsync(d_dims.p, dims, sizeof(int) * nd, hipMemcpyHostToDevice, c->st));
    }
    if (xmode && (rc = dmalloc(c, &gfac.p, sizeof(double) * std::min(n, jobs.CH) * D))) return rc;
    const int64_t Kp = g0.Kp, K2 = Kp * Kp;
    if (c->dtype == SCFGP_F32 && (rc = ensure_forget(c))) return rc;
    const UpdateOperands wide = {c->f_w, c->f_w + PRED_ROWS * Kp, c->f_w + 2 * PRED_ROWS * Kp, c->f_w + 2 * PRED_ROWS * Kp + K2};
    RowFeed feed;
    auto produce = [&](int64_t i, const Geom& g, const double* x, const double* tg, const UpdateOperands& ops, bool* have_rows) -> int {
        pack_chunk(c, g, x, nullptr, nullptr, nullptr, xmode, c->d_xscale);
        if (xmode) {
            gradcov_ones(gfac.p, g.N * D, c->st);
            xgrad_chunk(x, g.N, D, xmode, c->d_xscale, gfac.p, nullptr, c->st);
        }
        const GradObs obs = {(const int*)d_dims.p, nd, xmode ? gfac.p : nullptr, yn ? tg + jobs.seg_off(0) : nullptr, tg + jobs.seg_off(1),
                             rho ? tg + jobs.seg_off(2) : nullptr};
        const Geom gr = chunk_geom(g0, g.N * gb.nb());
        if (int r = UpdateImpl<double>::gradobs_chunk(c, g, gr, ops, obs)) return r;      // fp64 operands in every context
        *have_rows = true;
        return feed.release(i);
    };
    if ((rc = update_gather(c, feed, jobs, gb.nb(), alpha, Li, nullptr, c->dtype == SCFGP_F32 ? &wide : nullptr, produce))) return rc;
    return update_finish(c, feed, "condition_grad", "observations", alpha_out, Li_out);
}

// ----------------------------------------------------------------------------------------------
// removing observations from a fitted posterior (kernels_kstage.hip: kstage_downdate; derivation in include/scfgp_hip.h)
// ----------------------------------------------------------------------------------------------
static int ensure_forget(scfgp_ctx* c) {
    if (c->f_out) return SCFGP_OK;
    const int64_t Kp = c->g.Kp;
    int rc;
    if (c->dtype == SCFGP_F32) {
        const size_t bytes = sizeof(double) * 2 * (PRED_ROWS * Kp + Kp * Kp);
        if ((rc = dmalloc(c, &c->f_w, bytes))) return rc;
        HIPCHK(c, hipMemsetAsync(c->f_w, 0, bytes, c->st));               // the padding columns of Phi and C stay zero
    }
    return dmalloc(c, &c->f_out, sizeof(double) * (7 * PRED_ROWS + 8));
}
// scfgp_condition's first pass over the rows (plus r^T r), the K x K stage in its downdate form, then -- mu != NULL -- a second pass of
// the same feed over the rows: predict_chunk on the typed transpose of the device's Li', mu | std leaving through two staging halves
// (OutRing), the stats' sums formed on the device.  The host learns whether the stage succeeded before anything is written.
extern "C" int scfgp_forget(scfgp_ctx* c, const double* Xo, const double* yo, int64_t n, const double* alpha, const double* Li, int mode,
                            double* alpha_out, double* Li_out, double* mu, double* sd, double* stats) {
    if (!c) return SCFGP_EARG;
    if (!Xo || !yo || !alpha || !Li || mode < 0 || mode > 1) { c->err = "forget: bad arguments"; return SCFGP_EARG; }
    if ((!alpha_out) != (!Li_out)) { c->err = "forget: alpha_out and Li_out go together"; return SCFGP_EARG; }
    if ((!mu) != (!sd)) { c->err = "forget: mu and std go together"; return SCFGP_EARG; }
    if (stats && !mu) { c->err = "forget: stats need mu and std"; return SCFGP_EARG; }
    if (!alpha_out && !mu) { c->err = "forget: no output asked for"; return SCFGP_EARG; }
    if (n < 1) { c->err = "forget: n must be at least 1"; return SCFGP_EARG; }
    int rc;
    if ((rc = need_model({c, "forget"}, mode == 1))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const Geom& g0 = c->g;
    const int64_t Kp = g0.Kp, K2 = Kp * Kp;
    const RowJobs jobs = {Xo, yo, n, PRED_ROWS};
    const int64_t nchunks = jobs.count();
    if ((rc = ensure_forget(c))) return rc;
    double* rec = c->f_out + 4 * PRED_ROWS; double* acc = c->f_out + 7 * PRED_ROWS;
    // In fp32 contexts the first pass is the fp64 one: the error of C^T C is divided by lam_min(S) here, and what the fp32 chains of the
    // Gram launch add to it (~1e-6 of its entries) is felt in the predictions once most of a fit is removed.
    const UpdateOperands wide = {c->f_w, c->f_w + PRED_ROWS * Kp, c->f_w + 2 * PRED_ROWS * Kp, c->f_w + 2 * PRED_ROWS * Kp + K2};
    RowFeed feed;
    if ((rc = update_gather(c, feed, Xo, yo, n, alpha, Li, mode, acc + 3, c->dtype == SCFGP_F32 ? &wide : nullptr))) return rc;
    const KUpdate k = update_buffers(c);
    kstage_downdate(k, acc + 3, (double)n, c->d_sc, acc + 4, c->st);
    // u_flag[1]: what went in; u_flag[2]: what came out (a factorisation that failed leaves NaN behind, which is u_flag[0]'s to tell)
    update_check_finite(c->u_S, K2, c->u_flag + 1, c->st);
    update_check_finite(k.alpha_out, Kp, c->u_flag + 1, c->st);
    HIPCHK(c, hipGetLastError());
    int flags[3] = {0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(flags, c->u_flag, sizeof(flags), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (flags[1]) { c->err = "forget: non-finite rows, targets or factors"; return SCFGP_ENONFINITE; }
    if (flags[0]) { c->err = "forget: I - C^T C is not positive definite: these rows were not in this fit"; return SCFGP_ENOTPD; }
    if (flags[2]) { c->err = "forget: the downdated factors are not finite"; return SCFGP_ENONFINITE; }
    if (mu) {
        // the operands predict would build from the returned factors: the typed Li'^T (over the old one) and alpha', zero-padded
        DISPATCH(c, type_factor, c, c->u_S, c->u_LiT, nullptr);
        HIPCHK(c, hipMemsetAsync(c->alpha_pred(), 0, sizeof(double) * Kp, c->st));
        HIPCHK(c, hipMemcpyAsync(c->alpha_pred(), k.alpha_out, sizeof(double) * g0.K, hipMemcpyDeviceToDevice, c->st));
        HIPCHK(c, hipMemsetAsync(acc, 0, sizeof(double) * 3, c->st));
        OutRing ring;
        if ((rc = ring.open(c))) return rc;
        // the feed's jobs go on counting behind the first pass's (base nchunks), so its halves and events keep their order
        auto slot = [&](int64_t i) { return c->f_out + (i & 1) * 2 * PRED_ROWS; };
        auto download = [&](int64_t i) {
            return ring.drain(i, [&]() -> int {
                const int64_t t0 = jobs.row0(i), m = jobs.rows(i);
                const double* o = slot(i);
                HIPCHK(c, hipMemcpyAsync(mu + t0, o, sizeof(double) * m, hipMemcpyDeviceToHost, c->copy_st));
                HIPCHK(c, hipMemcpyAsync(sd + t0, o + PRED_ROWS, sizeof(double) * m, hipMemcpyDeviceToHost, c->copy_st));
                return SCFGP_OK;
            });
        };
        if ((rc = feed.upload(0, jobs, nchunks))) return rc;
        for (int64_t i = 0; i < nchunks; ++i) {
            const Geom g = chunk_geom(g0, jobs.rows(i));
            const double *x, *yi;
            if ((rc = feed.acquire(nchunks + i, &x, &yi))) return rc;
            pack_chunk(c, g, x, yi, nullptr, c->u_y, mode == 1 ? c->xs_mode : 0, c->d_xscale);
            if ((rc = feed.release(nchunks + i))) return rc;
            if ((rc = ring.acquire(i))) return rc;
            double* o = slot(i);
            if ((rc = DISPATCH(c, predict_chunk, c, g, c->u_LiT, o, o + PRED_ROWS))) return rc;
            if (stats) forget_stats(o, o + PRED_ROWS, c->u_y, g.N, PRED_ROWS, rec, acc, c->st);
            if ((rc = ring.computed(i))) return rc;
            if (i + 1 < nchunks && (rc = feed.upload(i + 1, jobs, nchunks))) return rc;
            if (i >= 1 && (rc = download(i - 1))) return rc;
        }
        if ((rc = download(nchunks - 1))) return rc;
    }
    double h_acc[6];
    if (stats) HIPCHK(c, hipMemcpyAsync(h_acc, acc, sizeof(h_acc), hipMemcpyDeviceToHost, c->st));
    if (alpha_out) {
        update_store_factor(c->u_S, g0.K, g0.Kp, c->u_Si, c->st);          // S^-1 is done with: Li' in host layout
        HIPCHK(c, hipMemcpyAsync(Li_out, c->u_Si, sizeof(double) * g0.K * g0.K, hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipMemcpyAsync(alpha_out, k.alpha_out, sizeof(double) * g0.K, hipMemcpyDeviceToHost, c->st));
    }
    HIPCHK(c, hipStreamSynchronize(c->copy_st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    if (stats) {
        stats[0] = (double)n; stats[1] = h_acc[0]; stats[2] = h_acc[1]; stats[3] = h_acc[2]; stats[4] = h_acc[4]; stats[5] = h_acc[5];
        stats[6] = 1.0; stats[7] = 0.0;
    }
    return SCFGP_OK;
}

// ----------------------------------------------------------------------------------------------
// exact leave-one-out / leave-block-out predictions of rows that are in the fit (loo.hip; derivation in include/scfgp_hip.h)
// ----------------------------------------------------------------------------------------------
static constexpr int LOO_MAX_BLOCK = 64;
static int ensure_loo(scfgp_ctx* c) {
    if (c->l_bad) return SCFGP_OK;
    int rc;
    if ((rc = dmalloc(c, &c->l_y, sizeof(double) * PRED_ROWS)) || (rc = dmalloc(c, &c->l_r, sizeof(double) * PRED_ROWS)) ||
        (rc = dmalloc(c, &c->l_rec, sizeof(double) * 5 * PRED_ROWS)) || (rc = dmalloc(c, &c->l_out, sizeof(double) * 6 * PRED_ROWS)) ||
        (rc = dmalloc(c, &c->l_acc, sizeof(double) * 8)) || (rc = dmalloc(c, &c->l_bad, sizeof(unsigned long long) * 2)))
        return rc;
    return SCFGP_OK;
}

// The chunk pipeline (RowFeed, OutRing) with the targets behind the rows of their chunk; resident rows bypass the feed and are read
// where they lie (d_Xraw / d_yraw, never the evaluation's working set).  Per chunk C = Phi_I Li^T, the residual and the block kernel.  A
// chunk holds floor(32768 / block) whole blocks, so no block straddles two chunks.  mu | std | lev leave through the two halves of
// l_out; the stats and the flags are fetched once, at the end.
extern "C" int scfgp_loo(scfgp_ctx* c, const double* X, const double* y, int64_t n, const double* alpha, const double* Li, int mode,
                         int block, double* mu, double* sd, double* lev, double* stats) {
    if (!c) return SCFGP_EARG;
    const bool resident = !X && !y;
    if ((!X) != (!y) || !alpha || !Li || !mu || !sd || mode < 0 || mode > 1) { c->err = "loo: bad arguments"; return SCFGP_EARG; }
    if (block < 1 || block > LOO_MAX_BLOCK) { c->err = "loo: block must lie in 1..64"; return SCFGP_EARG; }
    if (resident) {
        if (mode != 0) { c->err = "loo: resident rows are scaled rows (mode must be 0)"; return SCFGP_EARG; }
        if (!c->have_data || c->Nstore < 1) { c->err = "loo: no resident rows (scfgp_set_data)"; return SCFGP_EARG; }
        n = c->Nstore;
    }
    if (n < 1) { c->err = "loo: n must be at least 1"; return SCFGP_EARG; }
    int rc;
    if ((rc = need_model({c, "loo"}, mode == 1))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const Geom& g0 = c->g;
    const int64_t CH = PRED_ROWS / block * block;               // rows per chunk: whole blocks
    const RowJobs jobs = {X, y, n, CH};
    const int64_t nchunks = jobs.count();
    if ((rc = ensure_pred_chunk(c))) return rc;
    if ((rc = ensure_pred_factor(c))) return rc;
    if ((rc = ensure_loo(c))) return rc;
    RowFeed feed; OutRing ring;                                   // Li in host layout / two chunks of [X | y] (resident rows: Li only)
    if ((rc = feed.open(c, resident ? 0 : PRED_ROWS * (g0.D + 1), (int64_t)g0.K * g0.K))) return rc;
    const void* LiT;
    if ((rc = load_factor(c, feed, Li, pad_square, true, alpha, &LiT))) return rc;
    const unsigned long long bad0[2] = {0ull, ~0ull};
    HIPCHK(c, hipMemsetAsync(c->l_acc, 0, sizeof(double) * 8, c->st));
    HIPCHK(c, hipMemcpyAsync(c->l_bad, bad0, sizeof(bad0), hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));                     // raw is reused below
    if ((rc = ring.open(c))) return rc;
    auto slot = [&](int64_t i) { return c->l_out + (i & 1) * 3 * PRED_ROWS; };
    auto download = [&](int64_t i) {
        return ring.drain(i, [&]() -> int {
            const int64_t t0 = jobs.row0(i), m = jobs.rows(i);
            const double* o = slot(i);
            HIPCHK(c, hipMemcpyAsync(mu + t0, o, sizeof(double) * m, hipMemcpyDeviceToHost, c->copy_st));
            HIPCHK(c, hipMemcpyAsync(sd + t0, o + PRED_ROWS, sizeof(double) * m, hipMemcpyDeviceToHost, c->copy_st));
            if (lev) HIPCHK(c, hipMemcpyAsync(lev + t0, o + 2 * PRED_ROWS, sizeof(double) * m, hipMemcpyDeviceToHost, c->copy_st));
            return SCFGP_OK;
        });
    };
    if (!resident && (rc = feed.upload(0, jobs))) return rc;    // resident rows are read where they lie: nothing is uploaded
    for (int64_t i = 0; i < nchunks; ++i) {
        const int64_t t0 = jobs.row0(i);
        const Geom g = chunk_geom(g0, jobs.rows(i));
        if (resident) {
            pack_chunk(c, g, c->d_Xraw + t0 * g0.D, c->d_yraw + t0, nullptr, c->l_y);
        } else {
            const double *xi, *yi;
            if ((rc = feed.acquire(i, &xi, &yi))) return rc;
            pack_chunk(c, g, xi, yi, nullptr, c->l_y, mode == 1 ? c->xs_mode : 0, c->d_xscale);
            if ((rc = feed.release(i))) return rc;
        }
        if ((rc = ring.acquire(i))) return rc;
        double* o = slot(i);
        if ((rc = DISPATCH(c, loo_chunk, c, g, LiT, block, t0 / block, o, o + PRED_ROWS, o + 2 * PRED_ROWS))) return rc;
        if ((rc = ring.computed(i))) return rc;
        if (!resident && i + 1 < nchunks && (rc = feed.upload(i + 1, jobs))) return rc;
        if (i >= 1 && (rc = download(i - 1))) return rc;
    }
    if ((rc = download(nchunks - 1))) return rc;
    double acc[8]; unsigned long long bad[2];
    HIPCHK(c, hipMemcpyAsync(acc, c->l_acc, sizeof(acc), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(bad, c->l_bad, sizeof(bad), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->copy_st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    if (bad[0]) { c->err = "loo: non-finite rows, targets or factors"; return SCFGP_ENONFINITE; }
    if (bad[1] != ~0ull) {
        const long long j = (long long)bad[1];
        c->err = "loo: I - H of block " + std::to_string(j) + " (rows " + std::to_string(j * block) + ".." +
                 std::to_string(std::min<long long>((j + 1) * block, n) - 1) + ") is not positive definite: these rows are not in the fit";
        return SCFGP_ENOTPD;
    }
    if (stats) {
        stats[0] = (double)n; stats[1] = acc[0]; stats[2] = acc[1]; stats[3] = acc[2]; stats[4] = acc[3]; stats[5] = acc[4];
        stats[6] = (double)((n + block - 1) / block); stats[7] = 0.0;
    }
    return SCFGP_OK;
}
