// Internal to csrc/: what the source files of the posterior and pool entry points (api_predict.hip, api_update.hip, api_pool.hip)
// share -- the chunk buffers, the chunk bodies that more than one of them calls (ChunkImpl), the chunk pipeline, and the update's
// row splits and buffers (scfgp_condition's family and scfgp_select_iv).  A helper that one file uses lives in that file.
#pragma once
#include "api_ctx.h"

// the chunk buffers of the predict family and of scfgp_sample (first call only); the padding columns of Phi* stay zero
static int ensure_pred_chunk(scfgp_ctx* c) {
    const Geom& g0 = c->g;
    const int64_t Kp = g0.Kp;
    const size_t ts = c->tsize();
    int rc;
    if (!c->p_Xt) {
        if ((rc = dmalloc(c, &c->p_Xt, sizeof(double) * PRED_ROWS * g0.Dp))) return rc;
        if (g0.lowrank && (rc = dmalloc(c, &c->p_Tt, sizeof(double) * PRED_ROWS * g0.Sp))) return rc;
        if ((rc = dmalloc(c, &c->p_vpart, sizeof(double) * PRED_ROWS * (Kp / 64)))) return rc;
        if ((rc = dmalloc(c, &c->p_mupart, sizeof(double) * PRED_ROWS * (Kp / 64)))) return rc;
        if ((rc = dmalloc(c, &c->p_Phi, ts * PRED_ROWS * Kp))) return rc;
        HIPCHK(c, hipMemsetAsync(c->p_Phi, 0, ts * PRED_ROWS * Kp, c->st));
    }
    return SCFGP_OK;
}

// the factor-form buffers that the std gradient of scfgp_predict_grad and scfgp_predict_cov share (first call of either only): the
// typed Li and two PRED_ROWS x Kp typed arrays (C = Phi* Li^T and V = C Li there; Ca and Cb here), padding columns zero
static int ensure_pred_factor(scfgp_ctx* c) {
    if (c->p_V) return SCFGP_OK;
    const int64_t Kp = c->g.Kp;
    const size_t ts = c->tsize();
    int rc;
    if ((rc = dmalloc(c, &c->p_Li, ts * Kp * Kp))) return rc;
    if ((rc = dmalloc(c, &c->p_C, ts * PRED_ROWS * Kp))) return rc;
    if ((rc = dmalloc(c, &c->p_V, ts * PRED_ROWS * Kp))) return rc;
    HIPCHK(c, hipMemsetAsync(c->p_C, 0, ts * PRED_ROWS * Kp, c->st));
    HIPCHK(c, hipMemsetAsync(c->p_V, 0, ts * PRED_ROWS * Kp, c->st));
    return SCFGP_OK;
}

// buffers of scfgp_predict_grad beside predict's own (first call only; the std gradient's on its first call)
static int ensure_pred_grad(scfgp_ctx* c, bool want_std) {
    const Geom& g = c->g;
    const size_t ts = c->tsize();
    int rc;
    if (!c->p_FT && (rc = dmalloc(c, &c->p_FT, ts * round_up(g.J, 16) * predgrad_ft_cols(g.D)))) return rc;
    if (want_std && (rc = ensure_pred_factor(c))) return rc;
    return SCFGP_OK;
}

// The chunk bodies that more than one source file calls.  Each file's own wrapper template (PredictImpl, UpdateImpl, PoolImpl) derives
// from this one, only so that the file's one-line DISPATCH and its own bodies reach these members under the names they always had.
template <typename T> struct ChunkImpl {
    typedef SweepKernels<T> SK;
    // ---- chunk bodies of the posterior entry points (the pipeline that feeds them is described at RowFeed below) ----
    // typed operands arrive as void*: both arms of DISPATCH get the same arguments
    // Phi of the chunk's packed rows (p_Xt -> p_Phi)
    static void features(scfgp_ctx* c, const Geom& g) {
        SK::featuremap(g, c->p_Xt, Projection{c->d_Fall, c->d_Lall, c->d_Rall, c->p_Tt}, c->d_sc, (T*)c->p_Phi, c->st);
    }
    // C = Phi Li^T by pass 2's level-2 product (loader-staged tiles); its by-products land in the chunk's partials: vpart (slices of
    // rowsum(C^2)) and mupart (slices of Phi avec)
    static void factor_c(scfgp_ctx* c, const Geom& g, const T* LiT, const double* avec, T* C) {
        SK::apply_c(g, (const T*)c->p_Phi, LiT, (const T*)c->p_Li, C, c->p_vpart, avec, avec, c->p_mupart, c->st, 0);
    }
    // typed copies of a padded fp64 factor: its transpose into LiT and / or the factor itself into Li (either may be NULL)
    static void type_factor(scfgp_ctx* c, const double* L64, void* LiT, void* Li) {
        if (LiT) SK::convert_transposed(L64, (T*)LiT, c->g.K, c->g.Kp, c->st);
        if (Li) SK::convert(L64, (T*)Li, c->g.K, c->g.Kp, c->st);
    }
    static int predict_chunk(scfgp_ctx* c, const Geom& g, const void* LiT, double* mu, double* sd) {
        features(c, g);
        SK::apply_predict(g, (const T*)c->p_Phi, (const T*)LiT, c->p_vpart, c->alpha_pred(), c->p_mupart, c->st);
        SK::rowpredict(g, c->p_mupart, c->p_vpart, c->d_sc, mu, sd, c->st);
        HIPCHK(c, hipGetLastError());
        return SCFGP_OK;
    }
    // FT = F_all^T in the context's type, the operand of predict_grad_chunk (once per call)
    static void grad_operand(scfgp_ctx* c) { predgrad_operand(c->g, c->d_Fall, (T*)c->p_FT, c->st); }
    // after predict_chunk: d mu / d x~ and (dstd != NULL) d sigma / d x~ of the chunk's rows (predgrad.hip).  V* = Phi* B in the factor
    // form C = Phi* Li^T, V = C Li: its rounding errors grow with sqrt(cond(A)) where those of V = Phi* B formed directly grow with
    // cond(A).  factor_c's by-products land in the chunk's partials, which rowpredict has consumed.
    static int predict_grad_chunk(scfgp_ctx* c, const Geom& g, const void* LiT, const double* sd, double* dmu, double* dstd) {
        if (dstd) {
            factor_c(c, g, (const T*)LiT, c->alpha_pred(), (T*)c->p_C);
            SK::apply_vc(g, (const T*)c->p_C, (const T*)c->p_Li, (const T*)LiT, (T*)c->p_V, c->st, 0);
        }
        predgrad<T>(g, (const T*)c->p_Phi, (const T*)c->p_V, c->alpha_pred(), (const T*)c->p_FT, sd, c->d_sc, dmu, dstd, c->st);
        HIPCHK(c, hipGetLastError());
        return SCFGP_OK;
    }
    // scfgp_predict_cov, scfgp_select: C = Phi* Li^T of the chunk's rows (the by-products are ignored)
    static int cov_factor_chunk(scfgp_ctx* c, const Geom& g, const void* LiT, void* C) {
        features(c, g);
        factor_c(c, g, (const T*)LiT, c->alpha_pred(), (T*)C);
        HIPCHK(c, hipGetLastError());
        return SCFGP_OK;
    }
    // workgroups per row split of the Gram launch on the context's geometry (update_splits)
    static int gram_jobs(const scfgp_ctx* c) { return SK::gram_jobs(c->g); }
};

// ----------------------------------------------------------------------------------------------
// the chunk pipeline of the posterior entry points: the predict family, scfgp_sample, scfgp_sample_argmax, scfgp_predict_cov,
// scfgp_condition, scfgp_condition_grad, scfgp_forget, scfgp_loo, scfgp_predict_gradcov, scfgp_predict_pd, scfgp_select, scfgp_select_qei and scfgp_acquire_kg
// ----------------------------------------------------------------------------------------------
// Rows come from pageable host memory in jobs of at most PRED_ROWS rows.  Job i + 1 is uploaded on the copy stream (the call blocks
// the host while it stages) after the kernels of job i have been enqueued on the context's stream, so the copy runs beside them.  A
// RowFeed owns the two halves that the uploads alternate between and the events that order a half between the streams: up (the rows
// are there: st waits before pack_data reads them) and fre (they have been read: the copy stream waits before job i + 2 overwrites
// them).  The caller places release(): right after pack_data, or after the last kernel that still reads the raw rows.
// Results that do not stay on the device leave through two staging slots of the caller, ordered by an OutRing: done (slot k is
// computed: the copy stream waits before it copies the slot out) and copied (st waits before slot k + 2 overwrites it).  Each loop
// enqueues in the order "compute slot k, upload job k + 1, drain slot k - 1" and drains the last slot behind the loop: the host's
// blocking copies in both directions fall under the next chunk's kernels, and device memory does not grow with the row count.
// The waits for reuse run from the third job or slot on.
//
// Around it the entry points share (the parts that need no HIP are in api_host.h; each is described where it is defined): RowJobs, the
// job schedule that RowFeed::upload(job, jobs) stages from (`base` shifts the feed's job number behind an earlier schedule; the loops stay
// in the entry points, since where release, ring.acquire, ring.computed and the downloads fall differs); scan_weights, one pass over a
// weight vector (all callers report the first negative row even behind a non-finite one, scfgp_predict_gradcov the first entry that is
// either); Fail and need_model, the one way to refuse a call; load_factor's short form; BestBlock, the running best of a pool sweep.
// Not through these helpers, and why:
//   scfgp_loo with resident rows      the rows are read where they lie on the device: its loop skips the uploads and the feed
//   scfgp_select_iv                   two schedules in a row (the reference chunks, then the pool): a one-line lambda picks a job's
//   scfgp_condition, _condition_grad, scfgp_forget    load_factor's long form (update_gather): other buffers, and the finite check
//   scfgp_predict_grad, _raw, _y      scaler checks under their own names and texts, apart from predict_impl's parameter check
//   scfgp_select, _select_iv, _qei    bare int flags, fetched twice under two different synchronisations: a helper would not be shorter
// scfgp_forget's second phase and scfgp_predict_pd's second pass use RowJobs through `base`: their feed goes on counting.
template <int N> struct Events {                                  // call-scoped events: released on every return path
    hipEvent_t e[N] = {};
    int create(scfgp_ctx* c) {
        for (hipEvent_t& x : e) HIPCHK(c, hipEventCreateWithFlags(&x, hipEventDisableTiming));
        return SCFGP_OK;
    }
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};
struct RowFeed {
    scfgp_ctx* c = nullptr;
    DevTmp raw;                                                   // two halves of `stride` doubles: rows (n x D), targets at PRED_ROWS * D
    int64_t stride = 0;
    Events<4> ev;                                                 // up[2] | fre[2]
    // also_holds: what else the buffer is used for (the host layout of Li, before the first job); stride 0: no rows will be fed
    int open(scfgp_ctx* c_, int64_t stride_, int64_t also_holds = 0) {
        c = c_; stride = stride_;
        if (int rc = dmalloc(c, &raw.p, sizeof(double) * std::max<int64_t>(also_holds, 2 * stride))) return rc;
        return ev.create(c);
    }
    int upload(int64_t job, const double* X, const double* y, int64_t rows) {
        const int h = (int)(job & 1);
        if (job >= 2) HIPCHK(c, hipStreamWaitEvent(c->copy_st, ev.e[2 + h], 0));
        HIPCHK(c, hipMemcpyAsync(raw + h * stride, X, sizeof(double) * rows * c->g.D, hipMemcpyHostToDevice, c->copy_st));
        if (y) HIPCHK(c, hipMemcpyAsync(raw + h * stride + PRED_ROWS * c->g.D, y, sizeof(double) * rows, hipMemcpyHostToDevice, c->copy_st));
        HIPCHK(c, hipEventRecord(ev.e[h], c->copy_st));
        return SCFGP_OK;
    }
    // a job of a schedule, as the feed's job base + job.  A schedule with further target arrays (RowJobs::y1, y2: scfgp_condition_grad)
    // stages every segment at its place in the block behind the rows; its stride is PRED_ROWS * D + CH * target_width() doubles
    int upload(int64_t job, const RowJobs& j, int64_t base = 0) {
        if (!j.y1 && !j.y2) return upload(base + job, j.x(job, c->g.D), j.targets(job), j.rows(job));
        const int h = (int)((base + job) & 1);
        const int64_t rows = j.rows(job);
        if (base + job >= 2) HIPCHK(c, hipStreamWaitEvent(c->copy_st, ev.e[2 + h], 0));
        HIPCHK(c, hipMemcpyAsync(raw + h * stride, j.x(job, c->g.D), sizeof(double) * rows * c->g.D, hipMemcpyHostToDevice, c->copy_st));
        for (int k = 0; k < RowJobs::SEGS; ++k)
            if (const double* src = j.seg(job, k))
                HIPCHK(c, hipMemcpyAsync(raw + h * stride + PRED_ROWS * c->g.D + j.seg_off(k), src, sizeof(double) * rows * j.seg_width(k),
                                         hipMemcpyHostToDevice, c->copy_st));
        HIPCHK(c, hipEventRecord(ev.e[h], c->copy_st));
        return SCFGP_OK;
    }
    int acquire(int64_t job, const double** x, const double** y = nullptr) {
        const int h = (int)(job & 1);
        HIPCHK(c, hipStreamWaitEvent(c->st, ev.e[h], 0));
        *x = raw + h * stride;
        if (y) *y = raw + h * stride + PRED_ROWS * c->g.D;
        return SCFGP_OK;
    }
    int release(int64_t job) {
        HIPCHK(c, hipEventRecord(ev.e[2 + (int)(job & 1)], c->st));
        return SCFGP_OK;
    }
};
struct OutRing {
    scfgp_ctx* c = nullptr;
    Events<4> ev;                                                 // done[2] | copied[2]
    int open(scfgp_ctx* c_) { c = c_; return ev.create(c); }
    int acquire(int64_t k) {
        if (k >= 2) HIPCHK(c, hipStreamWaitEvent(c->st, ev.e[2 + (int)(k & 1)], 0));
        return SCFGP_OK;
    }
    int computed(int64_t k) {
        HIPCHK(c, hipEventRecord(ev.e[(int)(k & 1)], c->st));
        return SCFGP_OK;
    }
    // copies: the caller's hipMemcpyAsync calls on the copy stream (pageable: the host waits in them while the next slot computes)
    template <typename F> int drain(int64_t k, F copies) {
        const int h = (int)(k & 1);
        HIPCHK(c, hipStreamWaitEvent(c->copy_st, ev.e[h], 0));
        if (int rc = copies()) return rc;
        HIPCHK(c, hipEventRecord(ev.e[2 + h], c->copy_st));
        return SCFGP_OK;
    }
};
static Geom chunk_geom(const Geom& g0, int64_t rows) {
    Geom g = g0;
    g.N = rows; g.Np = round_up(rows, 256);
    return g;
}
// pack_data of one chunk of a posterior call into p_Xt; the chunk's padded row count is kept for debug_read("pXt")
static void pack_chunk(scfgp_ctx* c, const Geom& g, const double* Xraw, const double* yraw, const int64_t* idx, double* y,
                       int mode = 0, const double* sp = nullptr) {
    c->p_rows = g.Np;
    pack_data(g, Xraw, yraw, idx, c->p_Xt, y, c->st, mode, sp);
}
// The factor pass.  Li (K x K, host) -> raw -> L64 (Kp x Kp fp64) by `pad` (pad_square: identity padding; update_load_factor: the
// lower triangle only, so that entries above the diagonal are never read) -> the typed Li^T into LiT and, Li_typed != NULL, the typed
// Li.  alpha != NULL: zero-padded into avec.  finite != NULL: scfgp_condition's checks of what was loaded.  raw may be reused once the
// stream has been synchronised.
typedef void (*PadFn)(const double*, int, int, double*, hipStream_t);
static int load_factor(scfgp_ctx* c, double* raw, const double* Li, PadFn pad, double* L64, void* LiT, void* Li_typed,
                       const double* alpha = nullptr, double* avec = nullptr, int* finite = nullptr) {
    const Geom& g = c->g;
    HIPCHK(c, hipMemcpyAsync(raw, Li, sizeof(double) * g.K * g.K, hipMemcpyHostToDevice, c->st));
    pad(raw, g.K, g.Kp, L64, c->st);
    if (alpha) {
        HIPCHK(c, hipMemsetAsync(avec, 0, sizeof(double) * g.Kp, c->st));
        HIPCHK(c, hipMemcpyAsync(avec, alpha, sizeof(double) * g.K, hipMemcpyHostToDevice, c->st));
    }
    if (finite) {
        update_check_finite(L64, (int64_t)g.Kp * g.Kp, finite, c->st);
        update_check_finite(avec, g.Kp, finite, c->st);
    }
    DISPATCH_TO(ChunkImpl, c, type_factor, c, L64, LiT, Li_typed);
    return SCFGP_OK;
}
// The usual operands: L64 is d_T1, the typed Li^T goes to d_AbarT (scratch outside adjoint..pass3) and is handed back in *LiT, the
// typed Li to p_Li (typed_Li), alpha to alpha_pred().  The caller synchronises the stream before the feed's buffer is reused.
static int load_factor(scfgp_ctx* c, RowFeed& feed, const double* Li, PadFn pad, bool typed_Li, const double* alpha, const void** LiT) {
    *LiT = c->d_AbarT;
    return load_factor(c, feed.raw, Li, pad, c->d_T1, c->d_AbarT, typed_Li ? c->p_Li : nullptr, alpha, alpha ? c->alpha_pred() : nullptr);
}

// One way to refuse a call: "<who>: <what>" is the context's error text.
struct Fail {
    scfgp_ctx* c; const char* who;
    int set(const std::string& what, int code) const { c->err = std::string(who) + ": " + what; return code; }
    int arg(const std::string& what) const { return set(what, SCFGP_EARG); }
    int nonfinite(const std::string& what) const { return set(what, SCFGP_ENONFINITE); }
};
// what a posterior entry point needs of the context before it reads its other arguments' values
static int need_model(const Fail& f, bool x_scaler, bool y_scaler = false) {
    if (x_scaler && !f.c->d_xscale) return f.arg("no X scaler set");
    if (y_scaler && !f.c->d_yscale) return f.arg("no y scaler set");
    if (!f.c->have_params) return f.arg("parameters not set");
    return SCFGP_OK;
}

// The running best of a pool sweep: n (value, row) pairs and one double that holds the call's int flags, behind the workgroups' records
// of two chunks (values of slot 0, of slot 1, then the rows of each; chunk i writes slot i & 1): 4 * nrec + 2 * n + 1 doubles.
struct BestBlock {
    double* rec = nullptr; int64_t n = 0, nrec = 0;
    static int64_t doubles(int64_t n, int64_t nrec) { return 4 * nrec + 2 * n + 1; }
    void carve(double* base, int64_t n_, int64_t nrec_) { rec = base; n = n_; nrec = nrec_; }
    double* v() const { return rec + 4 * nrec; }
    long long* t() const { return (long long*)(v() + n); }
    int* flag() const { return (int*)(v() + 2 * n); }
    double* rec_v(int64_t i) const { return rec + (i & 1) * nrec; }
    long long* rec_t(int64_t i) const { return (long long*)(rec + (2 + (i & 1)) * nrec); }
    int clear(scfgp_ctx* c) const { HIPCHK(c, hipMemsetAsync(flag(), 0, sizeof(double), c->st)); return SCFGP_OK; }
    // host: 2 * n + 1 doubles, [v | t | flags]; both streams have drained on return, so the caller can refuse before it writes an output
    int fetch(scfgp_ctx* c, double* host) const {
        HIPCHK(c, hipMemcpyAsync(host, v(), sizeof(double) * (2 * n + 1), hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipStreamSynchronize(c->copy_st));
        HIPCHK(c, hipStreamSynchronize(c->st));
        return SCFGP_OK;
    }
    int host_flag(const double* host, int k = 0) const { int f[2]; memcpy(f, host + 2 * n, sizeof(f)); return f[k]; }
};

// Here, not in api_update.hip, because scfgp_select_iv (api_pool.hip) forms its Gram products with them too; ChunkImpl::gram_jobs likewise.
// row splits of the update's Gram product over a chunk of Np rows, and the slabs they need
static RowSplits update_splits(const scfgp_ctx* c, int64_t Np, bool wide = false) {
    if (wide) return gram_row_splits(ChunkImpl<double>::gram_jobs(c), Np, false, 0, 1);     // the fp64 job list in an fp32 context
    return gram_row_splits(DISPATCH_TO(ChunkImpl, c, gram_jobs, c), Np, c->dtype == SCFGP_F32, 0, 1);
}
// the update stage's own buffers (first call only; the slabs grow to what the call's chunks need)
static int ensure_update(scfgp_ctx* c, size_t slabs_bytes) {
    const int64_t Kp = c->g.Kp, K2 = Kp * Kp;
    int rc;
    if (!c->u_flag) {
        if ((rc = dmalloc(c, &c->u_Li, sizeof(double) * K2)) || (rc = dmalloc(c, &c->u_S, sizeof(double) * K2)) ||
            (rc = dmalloc(c, &c->u_Lm, sizeof(double) * K2)) || (rc = dmalloc(c, &c->u_Mi, sizeof(double) * K2)) ||
            (rc = dmalloc(c, &c->u_Si, sizeof(double) * K2)) || (rc = dmalloc(c, &c->u_LiT, c->tsize() * K2)) ||
            (rc = dmalloc(c, &c->u_vec, sizeof(double) * 35 * Kp)) || (rc = dmalloc(c, &c->u_acc, sizeof(double) * (c->n_pk + Kp))) ||
            (rc = dmalloc(c, &c->u_part, sizeof(double) * (c->n_pk + Kp))) || (rc = dmalloc(c, &c->u_y, sizeof(double) * PRED_ROWS)) ||
            (rc = dmalloc(c, &c->u_r, sizeof(double) * PRED_ROWS)) || (rc = dmalloc(c, &c->u_ws2, sizeof(float) * 2 * (PRED_ROWS + 32))))
            return rc;
        HIPCHK(c, hipMemsetAsync(c->u_Mi, 0, sizeof(double) * K2, c->st));       // its blocks above the diagonal stay zero for good
        HIPCHK(c, hipMemsetAsync(c->u_ws2, 0, sizeof(float) * 2 * (PRED_ROWS + 32), c->st));
        if ((rc = dmalloc(c, &c->u_flag, sizeof(int) * 16))) return rc;
    }
    if (slabs_bytes > c->u_slabs_bytes) {
        HIPCHK(c, hipStreamSynchronize(c->st));
        dfree(c->u_slabs); c->u_slabs_bytes = 0;
        if ((rc = dmalloc(c, &c->u_slabs, slabs_bytes))) return rc;
        c->u_slabs_bytes = slabs_bytes;
    }
    return SCFGP_OK;
}

// most sample functions, grid points or weight columns a call takes (scfgp_sample's family; scfgp_predict_pd and scfgp_sobol follow it)
static constexpr int SAMPLE_MAX = 1024;
