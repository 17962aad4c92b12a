// C ABI of libscfgp_hip.so (declared in include/scfgp_hip.h): context, device memory,
// the staged evaluation  pass1 | factor | pass2 | adjoint | pass3 | finish  and predict.
#include "../../include/scfgp_hip.h"
#include "kernels.h"
#include "api_host.h"

#include <dlfcn.h>
// RCCL: types and prototypes only -- the library is looked up at run time (scfgp_comm_init), no link-time dependency.  A ROCm
// install without the RCCL development headers still builds: the handful of declarations used here are then spelled out
// (they are RCCL's public, NCCL-compatible ABI).
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
extern "C" {
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclFloat64 = 8 } ncclDataType_t;
typedef enum { ncclSum = 0 } ncclRedOp_t;
ncclResult_t ncclGetUniqueId(ncclUniqueId*);
ncclResult_t ncclCommInitRank(ncclComm_t*, int, ncclUniqueId, int);
ncclResult_t ncclAllReduce(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
ncclResult_t ncclCommDestroy(ncclComm_t);
const char* ncclGetErrorString(ncclResult_t);
}
#endif

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define HIPCHK(ctx, call)                                                                           \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                         \
            return SCFGP_EHIP;                                                                      \
        }                                                                                           \
    } while (0)

static constexpr int XT = 128;              // tile of the X~^T Zbar product and padding unit of J (kernels_sweep.hip)
static constexpr int64_t PRED_ROWS = 32768; // predict processes test rows in chunks of this size
// Thresholds of the automatic precision escalation and the error model behind them (profiles/r03_c3_owner.md): with the
// fp32 Gram products (4096-row flush interval, relative error ~6e-8) the relative error of alpha / Li, and of the frequency
// gradient blocks, against fp64 mode is about SCFGP_ERR_PER_COND times the condition estimate (measured 7e-8 .. 2e-6 times
// the estimate at estimates 4 .. 6.4e3: the estimate is a lower bound of cond_2 of varying tightness).  Level 1 keeps the predicted alpha error under 3e-6 (north star: 1e-5), level 2
// the predicted gradient error under 3e-4 (SURVEY App. E acceptance: 1e-3 per block).
#ifndef SCFGP_COND_THRESHOLD
#define SCFGP_COND_THRESHOLD 10.0
#endif
#ifndef SCFGP_COND_THRESHOLD_W
#define SCFGP_COND_THRESHOLD_W 1000.0
#endif
#ifndef SCFGP_ERR_PER_COND
#define SCFGP_ERR_PER_COND 3.0e-7
#endif
static void derive_geom(Geom& g, int D, int S, int M);
static Geom chunk_geom(const Geom& g0, int64_t rows);

thread_local bool g_scfgp_capturing = false;

// roctx ranges around every stage (visible in `rocprofv3 --marker-trace`): OPT-IN (environment SCFGP_ROCTX=1 at context
// creation or option "roctx"); only then is the profiler's roctx library looked up, at run time, so the product has no
// link-time dependency on the profiler SDK and an ordinary process never loads it
struct Roctx {
    int (*push)(const char*) = nullptr; int (*pop)() = nullptr;
    Roctx() {
        void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_LAZY | RTLD_LOCAL);
        if (!h) h = dlopen("libroctx64.so", RTLD_LAZY | RTLD_LOCAL);
        if (!h) return;
        push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
        pop = (int (*)())dlsym(h, "roctxRangePop");
        if (!push || !pop) { push = nullptr; pop = nullptr; }
    }
};
static Roctx& roctx() { static Roctx r; return r; }

// RCCL, resolved at run time the first time a communicator is asked for: a process that already carries a copy (the host
// framework's, e.g. torch's librccl.so) is served by that copy, otherwise ROCm's is loaded.  Single-GPU users never load it.
struct Rccl {
    void* h = nullptr;
    decltype(&ncclGetUniqueId) get_id = nullptr; decltype(&ncclCommInitRank) init_rank = nullptr;
    decltype(&ncclAllReduce) all_reduce = nullptr; decltype(&ncclCommDestroy) destroy = nullptr;
    decltype(&ncclGetErrorString) err_string = nullptr;
    bool resolved = false;
    bool bind(void* from) {
        get_id = (decltype(get_id))dlsym(from, "ncclGetUniqueId"); init_rank = (decltype(init_rank))dlsym(from, "ncclCommInitRank");
        all_reduce = (decltype(all_reduce))dlsym(from, "ncclAllReduce"); destroy = (decltype(destroy))dlsym(from, "ncclCommDestroy");
        err_string = (decltype(err_string))dlsym(from, "ncclGetErrorString");
        return get_id && init_rank && all_reduce && destroy && err_string;
    }
    Rccl() {
        // a copy the process already carries, WHEREVER it was loaded from (a host framework bundles its own librccl under its
        // own path and may have loaded it RTLD_GLOBAL): the global symbol scope first, then an already-mapped copy by soname
        // (RTLD_NOLOAD; never promoted to RTLD_GLOBAL), and only then ROCm's copy, privately
        if (dlsym(RTLD_DEFAULT, "ncclAllReduce") && bind(RTLD_DEFAULT)) { resolved = true; return; }
        const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"};
        for (const char* n : names) if (!h) h = dlopen(n, RTLD_NOW | RTLD_NOLOAD | RTLD_LOCAL);
        for (const char* n : names) if (!h) h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        if (bind(h)) resolved = true;
        else { dlclose(h); h = nullptr; }
    }
    bool ok() const { return resolved; }
};
static Rccl& rccl() { static Rccl r; return r; }

struct ProfRec { std::string name; hipEvent_t e0, e1; };

struct scfgp_ctx {
    Geom g{};
    int dtype = 0, device = 0;
    hipStream_t st = nullptr; bool own_stream = false;
    hipStream_t copy_st = nullptr; hipEvent_t ev_factor = nullptr;          // alpha/Li D2H beside pass 2/3 ...
    // rank-S form of the backward projection: exchange 3 = [T~^T Zbar (Spp x Jp) ... | 8 scalars at Dpp*Jp | X~^T U (Dpp x Sq)]
    int lowrank_bwd = -1; int Spp = 0, Sq = 0; bool last_lrb = false;
    bool want_lrb() const {
        // T~ = [X l_F | 1] exists only when the forward projection goes through the S columns (g.lowrank), and U needs room in
        // Phibar's dead sine half
        const bool fits = g.lowrank && g.Jp + (int)round_up(g.S, 64) <= g.Kp;
        return fits && (lowrank_bwd == 1 || (lowrank_bwd < 0 && g.Dp >= 4 * g.Sp));
    }
    double* x3_scalars() { return d_x3 + (int64_t)Dpp * g.Jp; }
    double* xs1() { return d_xp1 + n_pk + g.Kp; }                           // the 8 scalars that close exchange buffers 1 and 2
    double* xs2() { return d_xp2 + n_pk + g.Kp; }
    // Ranks decide together (common.h: XS_*).  `unsettled`: a precision level was raised (or refused) since the last sum over
    // ranks, so the next exchange 1 carries every rank's attainable level and scfgp_factor commits to the lowest before pass 2
    // runs; cap(): the highest level this rank can run at.  test_*: fault injection for the tests (scfgp_set_option).
    bool unsettled = false; int test_deny_level = 0, test_fail_stage = 0, test_pd_group = 0, test_sobol_group = 0;
    int cap() const { return esc_denied > 0 ? esc_denied - 1 : 2; }
    double* x3_xu() { return d_x3 + (int64_t)Dpp * g.Jp + 8; }
    hipEvent_t ev_fence = nullptr;                                          // scfgp_stream_fence
    ncclComm_t comm = nullptr; int comm_ranks = 0, comm_rank = 0;           // scfgp_comm_init: the three sums run inside the library
    double* h_pin = nullptr;                                                // ... through pinned staging (K*K + K doubles)
    int64_t Ncap = 0, Nglobal = 0, Nglobal_full = 0;        // Nglobal_full: n_global given to scfgp_set_data
    bool have_params = false, have_data = false;
    int stage = 0, last_want_grad = 0;
    std::vector<double> h_params;
    // parameters
    double *d_params = nullptr, *d_F = nullptr, *d_Fall = nullptr, *d_Lall = nullptr, *d_Rall = nullptr; Scal* d_sc = nullptr;
    double *d_Tt = nullptr, *p_Tt = nullptr;                     // T~ = X~ Lall of the rank-S projection (rows / predict chunk)
    // dataset store (raw rows as uploaded) and the working set the sweeps run on
    double *d_Xraw = nullptr, *d_yraw = nullptr; int64_t Nstore = 0, store_cap = 0; bool work_full = false;
    int64_t* d_idx = nullptr; int64_t idx_cap = 0;
    // rows
    double *d_Xt = nullptr, *d_y = nullptr, *d_p = nullptr, *d_q = nullptr, *d_mu = nullptr, *d_vpart = nullptr;
    void *d_Phi = nullptr, *d_V = nullptr;
    // compute mode SCFGP_F16X3 (apply_f16.hip): fp32 mode whose two square apply products run as a three-term fp16 split wherever
    // fp32 mode would use its 256-wide LDS-DMA tiles; Phi16 = Phi in plane form (kernels.h), B16 = the K x K operand in plane form
    bool split16 = false; unsigned* d_Phi16 = nullptr; char* d_B16 = nullptr; float* d_f16scale = nullptr;
    // ... and the two Gram products too (gram_f16.hip): pass 1's on Phi16, pass 2's on the plane forms of V and of diag(q) V; block
    // partials of the side vectors; 8 floats of bounds and scales
    unsigned* d_V16g = nullptr; unsigned* d_qV16g = nullptr; double* d_f16side = nullptr; float* d_f16tmp = nullptr;
    int f16gram = 1;                                             // tuning knob "f16_gram": 0 keeps the fp32 Gram in this mode
    bool f16_on() const { return split16 && dma() == 2; }
    // rows per job and per slab set of the fp16 Gram (its fp32 chains end every 512 rows whatever this is): twice the fp32 Gram's flush
    // interval, less where that would leave fewer than 512 jobs = two rounds of the chip
    int64_t f16_chunk() const {
        const int64_t top = gram_chunk > 0 ? 2 * gram_chunk : 8192, fill = g.Np * F16x3Kernels::gram_tiles(g) / 512 / 512 * 512;
        return std::max<int64_t>(std::min(top, fill), 1024);
    }
    bool f16_gram() const { return f16_on() && f16gram && !last_cform; }      // factor form (level 2) keeps its fp32 products
    F16Operands f16ops() const { return F16Operands{d_Phi16, d_B16, d_f16scale, nullptr, d_f16tmp + 5}; }
    // exchange buffers and K-stage
    // exchange buffers xp1/xp2 = [packed lower tiles | vector Kp | 8 scalars], x3 = [X~^T Zbar | 8 scalars];
    // x1/x2 = the same matrices unpacked to full Kp x Kp (+ vector) for the K x K stage
    double *d_xp1 = nullptr, *d_xp2 = nullptr; int64_t n_xp = 0, n_pk = 0;
    double *d_x1 = nullptr, *d_x2 = nullptr, *d_x3 = nullptr; int64_t n_x1 = 0, n_x2 = 0, n_x3 = 0; int Dpp = 0;
    double *d_Li = nullptr, *d_B = nullptr, *d_T1 = nullptr, *d_T2 = nullptr, *d_Abar = nullptr;
    void *d_BT = nullptr, *d_AbarT = nullptr;                      // sweep operands: typed copies of B (or Li) and Abar (or Li^T)
    int apply_dma = -1;                                            // option: -1 = by problem size, 0 off, 1 = 128-wide tiles, 2 = 256-wide (fp32)
    double *d_vecs = nullptr;            // beta, alpha, u, ut, alpha_pred (Kp each)
    double *d_scalars = nullptr, *d_yy = nullptr; int* d_flag = nullptr;
    float* d_ws2 = nullptr;                                        // fp32 mode: packed (weight, side multiplier) rows of the Gram launches (kernels.h)
    double *d_slabs = nullptr; size_t slabs_bytes = 0;
    double *d_partial = nullptr; int64_t n_partial = 0;
    double *d_work = nullptr, *d_grad = nullptr;
    int xs_mode = 0; double* d_xscale = nullptr;                 // X scaler for scfgp_predict_raw (5*D doubles)
    int ys_mode = 0; double* d_yscale = nullptr;                 // y scaler for scfgp_predict_y (5 doubles)
    // predict chunk buffers
    double *p_Xt = nullptr, *p_vpart = nullptr, *p_mupart = nullptr; void *p_Phi = nullptr;
    int64_t p_rows = 0;                                          // padded rows of the chunk p_Xt holds (debug_read "pXt")
    // ... and those of scfgp_predict_grad, allocated by its first call: FT = Fall^T typed; with the std gradient C = Phi* Li^T, V = C Li
    // (PRED_ROWS x Kp each, typed) and the typed Li
    void *p_FT = nullptr, *p_C = nullptr, *p_V = nullptr, *p_Li = nullptr;
    // ... and those of scfgp_condition, allocated by its first call (ensure_update): the update stage's own K x K matrices (fp64: the old
    // factor, S / Li', M, M^-1, S^-1; typed: Li^T), its vectors [alpha | gamma | alpha' | 32 partial sums] (Kp each), the summed and the
    // per-chunk [packed C^T C | C^T r], targets and residuals of a chunk, the Gram launch's slabs, row weights and queue heads
    // (u_flag: [0] Cholesky flag, [1] non-finite flag, [8..15] queue heads)
    double *u_Li = nullptr, *u_S = nullptr, *u_Lm = nullptr, *u_Mi = nullptr, *u_Si = nullptr, *u_vec = nullptr, *u_acc = nullptr, *u_part = nullptr;
    double *u_y = nullptr, *u_r = nullptr, *u_slabs = nullptr; size_t u_slabs_bytes = 0;
    void* u_LiT = nullptr; float* u_ws2 = nullptr; int* u_flag = nullptr;
    // ... and those of scfgp_loo, allocated by its first call (ensure_loo): targets and residuals of a chunk, one record per block of a
    // chunk, two staging halves of [mu | std | lev], the running stats ([0..3] sums, [4] max h) and the flags ([0] non-finite, [1] first
    // block without a Cholesky factor)
    double *l_y = nullptr, *l_r = nullptr, *l_rec = nullptr, *l_out = nullptr, *l_acc = nullptr; unsigned long long* l_bad = nullptr;
    // ... and those of scfgp_forget beyond scfgp_condition's, allocated by its first call (ensure_forget): two staging halves of
    // [mu | std], the stats' terms of a chunk (3 x PRED_ROWS) and the scalars ([0..2] running sums, [3] r^T r, [4] joint, [5] min M_ii^2)
    // In fp32 contexts its first pass runs in fp64 (the fp64 features, C and Gram of precision level 1) on f_w: [Phi | C] (PRED_ROWS x Kp
    // each) and [Li^T | Li] (Kp x Kp each), all fp64
    double *f_out = nullptr, *f_w = nullptr;
    // on-device optimiser + captured training iteration
    int opt_algo = -1; OptHyper opt_h{}; double *d_opt = nullptr, *d_tctr = nullptr, *d_hist = nullptr; int hist_cap = 0;
    hipGraph_t graph = nullptr; hipGraphExec_t gexec = nullptr; int64_t graph_N = -1; bool in_train = false, warm = false;
    int use_graph = 1;
    // options
    int gram_nsplit = 0, gram_taper = 1, xtz_nsplit = 0; int64_t gram_chunk = 4096;
    RowSplits splits{};
    // Precision escalation (fp32 mode; profiles/r03_c3_owner.md).  The fp32 Gram products carry a relative error
    // of ~6e-8 that reaches alpha / Li (pass 1) and the gradient (pass 2's V^T diag(q) V) multiplied by the condition of A,
    // so the K x K stage's free condition estimate decides how the two TN products are formed:
    //   level 0  both in fp32 MFMA (fp64 across 4096-row chunks)
    //   level 1  pass 1: G = Phi^T Phi and Phi^T y by the fp64 kernels from fp64 features (alpha, Li, cost, mu*, sigma* then
    //            equal fp64 mode's to ~1e-8; alpha and Li bit for bit)
    //   level 2  also pass 2 in its factor form (C = Phi Li^T, v = rowsum(C^2), B W B = Li^T (C^T diag(q) C) Li, V = C Li):
    //            rounding errors amplified by sqrt(cond) instead of cond (gradient blocks)
    // option gram64: 0 never, 1 always level 1, 2 auto (default), 3 always level 2.  Auto is sticky: when the estimate of a
    // finished evaluation asks for a higher level that evaluation is repeated (scfgp_finish returns SCFGP_REDO; scfgp_eval
    // does so itself) and the following ones start at that level; the level drops when the estimate falls below a quarter
    // of the threshold.  Inside one scfgp_train call the level is fixed (the iteration may be a captured graph).
    int gram64 = 2, esc_level = 0, esc_denied = 0; double esc_thr = SCFGP_COND_THRESHOLD, escw_thr = SCFGP_COND_THRESHOLD_W; bool last_used64 = false;
    int last_level = 0; bool cond_valid = false;               // cond_valid: cond[] describes the current parameters and rows
    double cond[3] = {0, 0, 0};                                         // min L_ii^2, max L_ii^2, max_j (A^-1)_jj of the last factorisation
    void* d_Phi64 = nullptr; int64_t phi64_cap = 0; RowSplits splits64{};
    // factor form of pass 2 (C = Phi Li^T, V = C Li: SweepKernels::apply_c): -1 auto (precision level 2), 0 never, 1 always
    int factor_form = -1; bool last_cform = false; void* d_C = nullptr; int64_t c_cap = 0;
    bool want_cform() const { return factor_form == 1 || (factor_form < 0 && level() >= 2); }
    int level() const { return dtype != SCFGP_F32 || gram64 == 0 ? 0 : (gram64 == 1 ? 1 : (gram64 == 3 ? 2 : esc_level)); }
    bool use64() const { return level() >= 1; }
    double cond_est() const { return cond[1] * cond[2]; }
    // predicted relative error of alpha / Li behind an fp32 Gram: SCFGP_ERR_PER_COND x estimate.  The estimate is a lower bound
    // of cond_2(A) whose tightness varies (cond_2 / estimate: 30 .. 330 over the measured cases), so the prediction is an order
    // of magnitude: measured error / prediction lies in 0.2 .. 7 (profiles/r03_c3_owner.md)
    double alpha_err_fp32() const { return SCFGP_ERR_PER_COND * cond_est(); }
    int want_level(double est, double slack) const { return est > escw_thr * slack ? 2 : (est > esc_thr * slack ? 1 : 0); }
    // profiling
    bool roctx_on = false;
    bool prof = false; std::vector<ProfRec> recs; std::vector<hipEvent_t> pool; size_t pool_used = 0;
    std::string err;

    double* beta() { return d_vecs; }
    double* alpha() { return d_vecs + g.Kp; }
    // the apply products by LDS-DMA (apply.hip: apply_dma_kernel).  Auto: whenever the column plan has 128-wide tiles (K > 256)
    // and there are >= 16384 rows -- measured at K = 544 and 992, 16384 .. 100000 rows, both dtypes: 128-wide LDS-DMA tiles are
    // 4-13 % ahead of the loader-staged ones per product, 256-wide ones behind at these sizes (profiles/r04_tuning.md); fp32
    // 256-wide tiles from K >= 1024 and 65536 rows (equal to 128-wide at H since both are pipelined, 2/3 of the fabric traffic).
    // Below that the loader-staged tiles, whose single 64-wide launch per product matters more there
    int dma() const {
        const int auto_dma = g.K > 256 && g.Np >= 16384 ? (dtype == SCFGP_F32 && g.K >= 1024 && g.Np >= 65536 ? 2 : 1) : 0;
        return apply_dma < 0 ? auto_dma : apply_dma;
    }
    double* u() { return d_vecs + 2 * g.Kp; }
    double* ut() { return d_vecs + 3 * g.Kp; }
    double* alpha_pred() { return d_vecs + 4 * g.Kp; }
    size_t tsize() const { return dtype == SCFGP_F32 ? 4 : 8; }
    KStage kstage() {
        KStage k; k.K = g.K; k.Kp = g.Kp; k.A = d_x1; k.Li = d_Li; k.B = d_B; k.T1 = d_T1; k.T2 = d_T2;
        k.g = d_x1 + (int64_t)g.Kp * g.Kp; k.beta = beta(); k.alpha = alpha(); k.h = d_x2 + (int64_t)g.Kp * g.Kp;
        k.u = u(); k.ut = ut(); k.scalars = d_scalars; k.flag = d_flag;
        return k;
    }
};

struct ProfScope {
    scfgp_ctx* c; size_t idx = (size_t)-1; bool ranged = false;
    ProfScope(scfgp_ctx* c_, const char* name) : c(c_) {
        if (g_scfgp_capturing) return;
        if (c->roctx_on && roctx().push) { roctx().push(name); ranged = true; }
        if (!c->prof) return;
        auto get = [&]() {
            if (c->pool_used == c->pool.size()) { hipEvent_t e; hipEventCreate(&e); c->pool.push_back(e); }
            return c->pool[c->pool_used++];
        };
        ProfRec r; r.name = name; r.e0 = get(); r.e1 = get();
        hipEventRecord(r.e0, c->st);
        c->recs.push_back(r); idx = c->recs.size() - 1;
    }
    ~ProfScope() {
        if (idx != (size_t)-1) hipEventRecord(c->recs[idx].e1, c->st);
        if (ranged) roctx().pop();
    }
};

template <typename P> static int dmalloc(scfgp_ctx* c, P** p, size_t bytes) {
    HIPCHK(c, hipMalloc((void**)p, bytes ? bytes : 16));
    return SCFGP_OK;
}
template <typename P> static void dfree(P*& p) { if (p) { hipFree((void*)p); p = nullptr; } }
// call-scoped device buffer: released on every return path
struct DevTmp {
    double* p = nullptr;
    ~DevTmp() { if (p) hipFree(p); }
    operator double*() const { return p; }
};

// Row splits of the X~^T Zbar grid (few output tiles, equally long workgroups, two per CU): ONE round of the 512 resident
// workgroups.  The former "about 1152 workgroups" were 2.25 rounds at the headline shape (9 tiles x 128 splits) -- a third
// round a quarter full: 4.00 ms against 3.24 at 56 splits = 504 workgroups, 3.28-3.32 at two to six full rounds
// (profiles/r05_tuning.md).
static int xtz_split(int ntiles, int64_t Np) {
    int64_t s = std::max(1, 512 / ntiles);
    int64_t smax = std::max<int64_t>(Np / 2048, 1);
    if (ntiles * smax < 256) smax = std::max<int64_t>(Np / 64, 1);      // small problems: short dependent k-loops instead of few long ones
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    return (int)s;
}

static void free_rows(scfgp_ctx* c) {
    dfree(c->d_Xt); dfree(c->d_y); dfree(c->d_p); dfree(c->d_q); dfree(c->d_ws2); dfree(c->d_mu); dfree(c->d_vpart); dfree(c->d_Tt);
    dfree(c->d_Phi); dfree(c->d_V); dfree(c->d_Phi16); dfree(c->d_V16g); dfree(c->d_qV16g); dfree(c->d_f16side); dfree(c->d_slabs);
    c->Ncap = 0; c->slabs_bytes = 0;
}

// optional row buffers (fp64 features of an escalated pass 1, C of the factor form): sized
// for the current working set, allocated HERE and never inside a pass -- a pass may be running under graph capture
static int ensure_aux_rows(scfgp_ctx* c) {
    const Geom& g = c->g;
    if (c->use64() && c->phi64_cap < g.Np) {
        dfree(c->d_Phi64); c->phi64_cap = 0;
        if (int rc = dmalloc(c, &c->d_Phi64, sizeof(double) * g.Np * g.Kp)) return rc;
        HIPCHK(c, hipMemsetAsync(c->d_Phi64, 0, sizeof(double) * g.Np * g.Kp, c->st));      // columns >= K stay zero
        c->phi64_cap = g.Np;
    }
    if (c->want_cform() && c->c_cap < g.Np) {
        dfree(c->d_C); c->c_cap = 0;
        if (int rc = dmalloc(c, &c->d_C, c->tsize() * g.Np * g.Kp)) return rc;
        HIPCHK(c, hipMemsetAsync(c->d_C, 0, c->tsize() * g.Np * g.Kp, c->st));
        c->c_cap = g.Np;
    }
    return SCFGP_OK;
}

// (re)allocate every buffer whose size depends on the number of local rows
static int ensure_rows(scfgp_ctx* c, int64_t N) {
    Geom& g = c->g;
    if (c->gexec) { hipGraphExecDestroy(c->gexec); c->gexec = nullptr; }      // captured pointers/sizes may change
    if (c->graph) { hipGraphDestroy(c->graph); c->graph = nullptr; }
    const int64_t Np = round_up(N > 0 ? N : 1, 256);
    g.N = N; g.Np = Np;
    const int nts = g.Kp / g.tile, ntiles = nts * (nts + 1) / 2;
    const int ntx = ((g.Dp + XT - 1) / XT) * (g.Jp / XT);
    const int gjobs = c->dtype == SCFGP_F32 ? SweepKernels<float>::gram_jobs(g) : SweepKernels<double>::gram_jobs(g);
    c->splits = gram_row_splits(gjobs, Np, c->dtype == SCFGP_F32, c->gram_nsplit, c->gram_taper);
    int gs = c->splits.nsplit;
    if (c->dtype == SCFGP_F32 && c->gram64 != 0) {              // the fp64 job list of an escalated pass 1 has its own row splits
        c->splits64 = gram_row_splits(SweepKernels<double>::gram_jobs(g), Np, false, c->gram_nsplit, c->gram_taper);
        gs = std::max(gs, c->splits64.nsplit);
    }
    const int xs = c->xtz_nsplit > 0 ? (int)std::min<int64_t>(c->xtz_nsplit, Np / 64) : xtz_split(ntx, Np);
    // Gram slabs are followed by the per-split side-vector partials (gs x Kp)
    // the two row-contracted products of the rank-S backward projection (pass3): (Spp x Jp) and (Dpp x Sq) tile grids
    const int nt1 = (c->Spp / XT) * (g.Jp / XT), nt2 = (c->Dpp / XT) * (c->Sq / XT);
    const size_t lrb = std::max<size_t>((size_t)xtz_split(nt1, Np) * nt1, (size_t)xtz_split(nt2, Np) * nt2);
    if (c->split16) gs = std::max(gs, F16x3Kernels::gram_chunks(g, c->f16_chunk()));       // the f16x3 Gram: one set of slabs per row chunk
    const size_t need = sizeof(double) * std::max<size_t>((size_t)gs * ntiles * g.tile * g.tile + (size_t)gs * g.Kp,
                                                          std::max<size_t>((size_t)xs * ntx, lrb) * XT * XT);
    if (need > c->slabs_bytes) {
        dfree(c->d_slabs);
        if (int rc = dmalloc(c, &c->d_slabs, need)) return rc;
        c->slabs_bytes = need;
    }
    if (int rc = ensure_aux_rows(c)) return rc;
    if (Np <= c->Ncap) return SCFGP_OK;
    dfree(c->d_Xt); dfree(c->d_y); dfree(c->d_p); dfree(c->d_q); dfree(c->d_ws2); dfree(c->d_mu); dfree(c->d_vpart); dfree(c->d_Tt);
    dfree(c->d_Phi); dfree(c->d_V); dfree(c->d_Phi16); dfree(c->d_V16g); dfree(c->d_qV16g); dfree(c->d_f16side);
    c->Ncap = 0;
    const size_t ts = c->tsize();
    int rc;
    if ((rc = dmalloc(c, &c->d_Xt, sizeof(double) * Np * g.Dp))) return rc;
    if (g.lowrank && (rc = dmalloc(c, &c->d_Tt, sizeof(double) * Np * g.Sp))) return rc;
    if ((rc = dmalloc(c, &c->d_y, sizeof(double) * Np))) return rc;
    if ((rc = dmalloc(c, &c->d_p, sizeof(double) * Np))) return rc;
    if ((rc = dmalloc(c, &c->d_q, sizeof(double) * Np))) return rc;
    if (c->dtype == SCFGP_F32 && (rc = dmalloc(c, &c->d_ws2, sizeof(float) * 2 * (Np + 32)))) return rc;
    if ((rc = dmalloc(c, &c->d_mu, sizeof(double) * Np * (g.Kp / 64)))) return rc;           // mupart, like vpart
    if ((rc = dmalloc(c, &c->d_vpart, sizeof(double) * Np * (g.Kp / 64)))) return rc;          // <= one entry per 64 columns
    if ((rc = dmalloc(c, &c->d_Phi, ts * Np * g.Kp))) return rc;
    if ((rc = dmalloc(c, &c->d_V, ts * Np * g.Kp))) return rc;
    if (c->split16) {
        const size_t plane = sizeof(unsigned) * Np * g.Kp + F16x3Kernels::F16_PAD;
        if ((rc = dmalloc(c, &c->d_Phi16, plane)) || (rc = dmalloc(c, &c->d_V16g, plane)) || (rc = dmalloc(c, &c->d_qV16g, plane))) return rc;
        if ((rc = dmalloc(c, &c->d_f16side, sizeof(double) * F16x3Kernels::side_blocks(g) * g.Kp))) return rc;
        HIPCHK(c, hipMemsetAsync(c->d_Phi16, 0, plane, c->st));           // the padding is read (into tiles nobody stores): keep it finite
        HIPCHK(c, hipMemsetAsync(c->d_V16g, 0, plane, c->st));
        HIPCHK(c, hipMemsetAsync(c->d_qV16g, 0, plane, c->st));
    }
    HIPCHK(c, hipMemsetAsync(c->d_Phi, 0, ts * Np * g.Kp, c->st));       // padding columns >= K stay zero forever
    HIPCHK(c, hipMemsetAsync(c->d_V, 0, ts * Np * g.Kp, c->st));         // columns >= K are never written
    c->Ncap = Np;
    return SCFGP_OK;
}

extern "C" int scfgp_create(scfgp_ctx** out, int D, int S, int M, int dtype, int device, void* stream) {
    if (!out || D < 1 || S < 1 || M < 1 || (dtype != SCFGP_F64 && dtype != SCFGP_F32 && dtype != SCFGP_F16X3)) return SCFGP_EARG;
    scfgp_ctx* c = new scfgp_ctx();
    *out = c;
    c->split16 = dtype == SCFGP_F16X3;                            // fp32 mode in everything but the two square apply products
    if (c->split16) dtype = SCFGP_F32;
    c->dtype = dtype; c->device = device;
    Geom& g = c->g;
    derive_geom(g, D, S, M);
    if (const char* e = getenv("SCFGP_LOWRANK")) g.lowrank = atoi(e) != 0;                       // tuning override
    if (const char* e = getenv("SCFGP_ROCTX")) c->roctx_on = atoi(e) != 0;
    c->Dpp = (int)round_up(g.Dp, XT);
    HIPCHK(c, hipSetDevice(device));
    if (stream) c->st = (hipStream_t)stream;
    else { HIPCHK(c, hipStreamCreate(&c->st)); c->own_stream = true; }
    HIPCHK(c, hipStreamCreateWithFlags(&c->copy_st, hipStreamNonBlocking));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_factor, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_fence, hipEventDisableTiming));
    const int64_t Kp = g.Kp, K2 = Kp * Kp;
    c->Spp = (int)round_up(g.Sp, XT); c->Sq = (int)round_up(g.S, XT);
    c->n_x1 = K2 + Kp + 8; c->n_x2 = K2 + Kp + 8; c->n_x3 = (int64_t)std::max(c->Dpp, c->Spp) * g.Jp + 8 + (int64_t)c->Dpp * c->Sq;
    { const int64_t nts = Kp / g.tile; c->n_pk = nts * (nts + 1) / 2 * g.tile * g.tile; c->n_xp = c->n_pk + Kp + 8; }
    int rc;
    if ((rc = dmalloc(c, &c->d_params, sizeof(double) * g.P))) return rc;
    if ((rc = dmalloc(c, &c->d_F, sizeof(double) * D * M))) return rc;
    if ((rc = dmalloc(c, &c->d_Fall, sizeof(double) * g.Dp * g.Jp))) return rc;
    if ((rc = dmalloc(c, &c->d_Lall, sizeof(double) * g.Dp * round_up(g.Sp, 64)))) return rc;
    if ((rc = dmalloc(c, &c->d_Rall, sizeof(double) * g.Sp * g.Jp))) return rc;
    if ((rc = dmalloc(c, &c->d_sc, sizeof(Scal)))) return rc;
    if ((rc = dmalloc(c, &c->d_xp1, sizeof(double) * c->n_xp))) return rc;
    if ((rc = dmalloc(c, &c->d_xp2, sizeof(double) * c->n_xp))) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_xp1, 0, sizeof(double) * c->n_xp, c->st));
    HIPCHK(c, hipMemsetAsync(c->d_xp2, 0, sizeof(double) * c->n_xp, c->st));
    if ((rc = dmalloc(c, &c->d_x1, sizeof(double) * c->n_x1))) return rc;
    if ((rc = dmalloc(c, &c->d_x2, sizeof(double) * c->n_x2))) return rc;
    if ((rc = dmalloc(c, &c->d_x3, sizeof(double) * c->n_x3))) return rc;
    if ((rc = dmalloc(c, &c->d_Li, sizeof(double) * K2))) return rc;
    if ((rc = dmalloc(c, &c->d_B, sizeof(double) * K2))) return rc;
    if ((rc = dmalloc(c, &c->d_T1, sizeof(double) * K2))) return rc;
    if ((rc = dmalloc(c, &c->d_T2, sizeof(double) * K2))) return rc;
    if ((rc = dmalloc(c, &c->d_Abar, sizeof(double) * K2))) return rc;
    if ((rc = dmalloc(c, &c->d_BT, c->tsize() * K2))) return rc;        // sweep operands: typed, padding zeroed
    if ((rc = dmalloc(c, &c->d_AbarT, c->tsize() * K2))) return rc;
    if (c->split16) {
        if ((rc = dmalloc(c, &c->d_B16, 4 * (size_t)K2))) return rc;
        if ((rc = dmalloc(c, &c->d_f16scale, sizeof(float) * 4))) return rc;
        if ((rc = dmalloc(c, &c->d_f16tmp, sizeof(float) * 8))) return rc;
    }
    if ((rc = dmalloc(c, &c->d_vecs, sizeof(double) * 5 * Kp))) return rc;
    if ((rc = dmalloc(c, &c->d_scalars, sizeof(double) * 32))) return rc;
    if ((rc = dmalloc(c, &c->d_yy, sizeof(double) * 8))) return rc;
    if ((rc = dmalloc(c, &c->d_flag, sizeof(int) * 16))) return rc;         // [0..3] not-positive-definite flag, [8..15] the Gram's queue heads
    c->n_partial = 16384;                                             // block partials of the scalar reductions
    if ((rc = dmalloc(c, &c->d_partial, sizeof(double) * c->n_partial))) return rc;
    if ((rc = dmalloc(c, &c->d_work, sizeof(double) * (4 * D + 4 + (int64_t)D * M)))) return rc;
    if ((rc = dmalloc(c, &c->d_grad, sizeof(double) * g.P))) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_x1, 0, sizeof(double) * c->n_x1, c->st));
    HIPCHK(c, hipMemsetAsync(c->d_x2, 0, sizeof(double) * c->n_x2, c->st));
    HIPCHK(c, hipMemsetAsync(c->d_x3, 0, sizeof(double) * c->n_x3, c->st));
    HIPCHK(c, hipMemsetAsync(c->d_Li, 0, sizeof(double) * K2, c->st));          // its upper blocks stay zero for good (kstage_factor)
    HIPCHK(c, hipMemsetAsync(c->d_vecs, 0, sizeof(double) * 5 * Kp, c->st));
    HIPCHK(c, hipMemsetAsync(c->d_scalars, 0, sizeof(double) * 32, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SCFGP_OK;
}

extern "C" void scfgp_destroy(scfgp_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->st) hipStreamSynchronize(c->st);
    free_rows(c);
    dfree(c->d_Phi64); dfree(c->d_C); dfree(c->d_Xraw); dfree(c->d_yraw); dfree(c->d_idx); dfree(c->d_xscale); dfree(c->d_yscale);
    dfree(c->d_params); dfree(c->d_F); dfree(c->d_Fall); dfree(c->d_Lall); dfree(c->d_Rall); dfree(c->d_sc); dfree(c->p_Tt);
    dfree(c->d_xp1); dfree(c->d_xp2); dfree(c->d_x1); dfree(c->d_x2); dfree(c->d_x3); dfree(c->d_Li); dfree(c->d_B); dfree(c->d_T1); dfree(c->d_T2);
    dfree(c->d_Abar); dfree(c->d_BT); dfree(c->d_AbarT); dfree(c->d_B16); dfree(c->d_f16scale); dfree(c->d_f16tmp); dfree(c->d_vecs); dfree(c->d_scalars); dfree(c->d_yy);
    dfree(c->d_flag); dfree(c->d_partial); dfree(c->d_work); dfree(c->d_grad);
    dfree(c->p_Xt); dfree(c->p_vpart); dfree(c->p_mupart); dfree(c->p_Phi);
    dfree(c->p_FT); dfree(c->p_C); dfree(c->p_V); dfree(c->p_Li);
    dfree(c->u_Li); dfree(c->u_S); dfree(c->u_Lm); dfree(c->u_Mi); dfree(c->u_Si); dfree(c->u_vec); dfree(c->u_acc); dfree(c->u_part);
    dfree(c->u_y); dfree(c->u_r); dfree(c->u_slabs); dfree(c->u_LiT); dfree(c->u_ws2); dfree(c->u_flag);
    dfree(c->l_y); dfree(c->l_r); dfree(c->l_rec); dfree(c->l_out); dfree(c->l_acc); dfree(c->l_bad);
    dfree(c->f_out); dfree(c->f_w);
    if (c->gexec) hipGraphExecDestroy(c->gexec);
    if (c->graph) hipGraphDestroy(c->graph);
    dfree(c->d_opt); dfree(c->d_tctr); dfree(c->d_hist);
    for (hipEvent_t e : c->pool) hipEventDestroy(e);
    if (c->copy_st) { hipStreamSynchronize(c->copy_st); hipStreamDestroy(c->copy_st); }
    if (c->comm && rccl().ok()) rccl().destroy(c->comm);
    if (c->ev_factor) hipEventDestroy(c->ev_factor);
    if (c->ev_fence) hipEventDestroy(c->ev_fence);
    if (c->h_pin) hipHostFree(c->h_pin);
    if (c->own_stream && c->st) hipStreamDestroy(c->st);
    delete c;
}

extern "C" const char* scfgp_last_error(const scfgp_ctx* c) { return c ? c->err.c_str() : "null context"; }

extern "C" int scfgp_set_params(scfgp_ctx* c, const double* params, int P) {
    if (!c || !params || P != c->g.P) { if (c) c->err = "set_params: wrong parameter count"; return SCFGP_EARG; }
    HIPCHK(c, hipSetDevice(c->device));
    c->h_params.assign(params, params + P);
    HIPCHK(c, hipMemcpyAsync(c->d_params, c->h_params.data(), sizeof(double) * P, hipMemcpyHostToDevice, c->st));
    unpack_params(c->g, c->d_params, c->d_F, c->d_Fall, c->d_Lall, c->d_Rall, c->d_sc, c->st);
    HIPCHK(c, hipGetLastError());
    c->have_params = true; c->cond_valid = false;
    return SCFGP_OK;
}

extern "C" int scfgp_get_params(scfgp_ctx* c, double* params, int P) {
    if (!c || !params || P != c->g.P || !c->have_params) return SCFGP_EARG;
    memcpy(params, c->h_params.data(), sizeof(double) * P);
    return SCFGP_OK;
}

// working set := rows of the store selected by idx (NULL = all rows, in order)
static int load_working_set(scfgp_ctx* c, const int64_t* d_idx, int64_t n, int64_t n_global) {
    if (int rc = ensure_rows(c, n)) return rc;
    c->Nglobal = n_global > 0 ? n_global : n;
    pack_data(c->g, c->d_Xraw, c->d_yraw, d_idx, c->d_Xt, c->d_y, c->st);
    sum_squares(c->d_y, c->g.Np, c->d_yy, 0, c->d_partial, c->st);
    HIPCHK(c, hipGetLastError());
    c->work_full = d_idx == nullptr;
    c->have_data = true; c->stage = 0; c->cond_valid = false; c->esc_denied = 0;
    return SCFGP_OK;
}

extern "C" int scfgp_set_data(scfgp_ctx* c, const double* X, const double* y, int64_t N, int64_t n_global) {
    if (!c || !X || !y || N < 1) { if (c) c->err = "set_data: bad arguments"; return SCFGP_EARG; }
    HIPCHK(c, hipSetDevice(c->device));
    if (N > c->store_cap) {
        HIPCHK(c, hipStreamSynchronize(c->st));
        dfree(c->d_Xraw); dfree(c->d_yraw); c->store_cap = 0;
        if (int rc = dmalloc(c, &c->d_Xraw, sizeof(double) * N * c->g.D)) return rc;
        if (int rc = dmalloc(c, &c->d_yraw, sizeof(double) * N)) return rc;
        c->store_cap = N;
    }
    c->Nstore = N; c->Nglobal_full = n_global > 0 ? n_global : N;
    HIPCHK(c, hipMemcpyAsync(c->d_Xraw, X, sizeof(double) * N * c->g.D, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemcpyAsync(c->d_yraw, y, sizeof(double) * N, hipMemcpyHostToDevice, c->st));
    if (int rc = load_working_set(c, nullptr, N, n_global)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->st));            // the caller may reuse X, y as soon as we return
    return SCFGP_OK;
}

// ----------------------------------------------------------------------------------------------
// staged evaluation
// ----------------------------------------------------------------------------------------------
// summed exchange buffer [packed | vec | scalars] -> full symmetric matrix + vector for the K x K stage
static void unpack_exchange(scfgp_ctx* c, const double* xp, double* x) {
    const Geom& g = c->g;
    unpack_tri_tiles(xp, g.Kp / g.tile, g.tile, x, g.Kp, c->st);
    hipMemcpyAsync(x + (int64_t)g.Kp * g.Kp, xp + c->n_pk, sizeof(double) * (g.Kp + 8), hipMemcpyDeviceToDevice, c->st);
}

// typed operands of the first pass of scfgp_condition / scfgp_forget (Impl::update_chunk): Phi and C of a chunk (PRED_ROWS x Kp, padding
// columns zero), the factor's transpose and the factor (Kp x Kp)
struct UpdateOperands { void *Phi, *C, *LiT, *Li; };
template <typename T> struct Impl {
    typedef SweepKernels<T> SK;
    // out = [packed lower tiles of M^T diag(w) M | M^T side (Kp)],  M = Phi (pass 1) or V = Phi B (pass 2)
    static void gram_to(scfgp_ctx* c, const T* Mx, const double* w, const double* side, double* out, const char* name) {
        const Geom& g = c->g;
        const int nts = g.Kp / g.tile, ntiles = nts * (nts + 1) / 2;
        if constexpr (sizeof(T) == 4) {
            if (c->f16_gram()) {
                // f16x3 mode: a split pass over the operand (which also leaves the side vector's block partials), then the fp16 Gram
                // whose row chunks are the "splits" of the shared reduction
                const int nch = F16x3Kernels::gram_chunks(g, c->f16_chunk());
                { ProfScope ps(c, w ? "split_v" : "split_phi");
                  // V's own planes were written by the epilogue of V = Phi B (pass2) -- unless fp32 mode's register tiles formed V (K <= 256)
                  if (w) F16x3Kernels::split_v(g, (const float*)Mx, w, side, F16x3Kernels::apply_runs(g) ? nullptr : c->d_V16g, c->d_qV16g,
                                               c->d_f16side, c->d_f16tmp, c->st);
                  else F16x3Kernels::split_phi(g, (const float*)Mx, side, c->d_sc, c->d_Phi16, c->d_f16side, c->d_f16tmp, c->st); }
                { ProfScope ps(c, name);
                  F16x3Kernels::gram(g, w ? c->d_V16g : c->d_Phi16, w ? c->d_qV16g : c->d_Phi16, c->d_f16tmp + 4, c->f16_chunk(), c->d_slabs, c->st); }
                { ProfScope ps(c, "reduce_tiles"); reduce_tri_tiles(c->d_slabs, nch, nts, g.tile, out, c->st);
                  reduce_side(c->d_f16side, F16x3Kernels::side_blocks(g), g.Kp, g.gfull * g.tile + g.gstrip * 64, out + c->n_pk, c->st); }
                return;
            }
        }
        const int gs = c->splits.nsplit;
        double* sidepart = c->d_slabs + (size_t)gs * ntiles * g.tile * g.tile;
        { ProfScope ps(c, name);
          SK::gram(g, Mx, w, side, c->splits, c->dtype == SCFGP_F32 ? c->gram_chunk : 0, c->d_slabs, sidepart, c->d_flag + 8, c->d_ws2, c->st); }
        { ProfScope ps(c, "reduce_tiles"); reduce_tri_tiles(c->d_slabs, gs, nts, g.tile, out, c->st);
          reduce_side(sidepart, gs, g.Kp, g.gfull * g.tile + g.gstrip * 64, out + c->n_pk, c->st); }
    }
    static int pass1(scfgp_ctx* c) {
        const Geom& g = c->g;
        if (!c->in_train) HIPCHK(c, hipMemsetAsync(c->d_flag, 0, sizeof(int) * 4, c->st));
        const bool use64 = sizeof(T) == 4 && c->use64();
        c->last_cform = c->want_cform();
        if ((use64 && c->phi64_cap < g.Np) || (c->last_cform && c->c_cap < g.Np)) {
            c->err = "pass1: auxiliary row buffer missing"; return SCFGP_EARG;
        }
        const Projection proj{c->d_Fall, c->d_Lall, c->d_Rall, c->d_Tt};
        if constexpr (sizeof(T) == 4) {
            if (use64) {                                       // escalated pass 1: fp64 features, fp64 Gram and Phi^T y
                typedef SweepKernels<double> SK64;
                const int nts = g.Kp / g.tile, ntiles = nts * (nts + 1) / 2, gs = c->splits64.nsplit;
                double* sidepart = c->d_slabs + (size_t)gs * ntiles * g.tile * g.tile;
                { ProfScope ps(c, "featuremap64"); SK64::featuremap(g, c->d_Xt, proj, c->d_sc, (double*)c->d_Phi64, c->st); }
                { ProfScope ps(c, "gram64");
                  SK64::gram(g, (const double*)c->d_Phi64, nullptr, c->d_y, c->splits64, 0, c->d_slabs, sidepart, c->d_flag + 8, nullptr, c->st); }
                { ProfScope ps(c, "reduce_tiles"); reduce_tri_tiles(c->d_slabs, gs, nts, g.tile, c->d_xp1, c->st);
                  reduce_side(sidepart, gs, g.Kp, g.gfull * g.tile + g.gstrip * 64, c->d_xp1 + c->n_pk, c->st); }
            }
        }
        { ProfScope ps(c, "featuremap"); SK::featuremap(g, c->d_Xt, proj, c->d_sc, (T*)c->d_Phi, c->st); }
        if constexpr (sizeof(T) == 4) {
            // f16x3 mode: the apply tiles' packed pairs; with the fp16 Gram they come out of gram_to's split pass instead
            if (c->f16_on() && (use64 || !c->f16_gram())) {
                ProfScope ps(c, "split_phi");
                F16x3Kernels::split_phi(g, (const float*)c->d_Phi, c->d_y, c->d_sc, c->d_Phi16, c->d_f16side, c->d_f16tmp, c->st);
            }
        }
        if (!use64) gram_to(c, (const T*)c->d_Phi, nullptr, c->d_y, c->d_xp1, "gram");
        c->last_used64 = use64 || sizeof(T) == 8; c->last_level = sizeof(T) == 8 ? 0 : c->level();
        HIPCHK(c, hipMemcpyAsync(c->xs1(), c->d_yy, sizeof(double), hipMemcpyDeviceToDevice, c->st));
        write_status(c->xs1(), c->last_level >= 1 ? 1.0 : 0.0, c->cap() < 1 ? 1.0 : 0.0, c->cap() < 2 ? 1.0 : 0.0, 0.0, c->st);
        HIPCHK(c, hipGetLastError());
        return SCFGP_OK;
    }
    static int factor(scfgp_ctx* c) {
        const Geom& g = c->g;
        { ProfScope ps(c, "kstage_factor");
          hipMemcpyAsync(c->d_x1 + (int64_t)g.Kp * g.Kp, c->d_xp1 + c->n_pk, sizeof(double) * (g.Kp + 8), hipMemcpyDeviceToDevice, c->st);
          kstage_factor(c->kstage(), c->d_xp1, c->d_sc, c->st); }
        if (c->last_cform) {                                   // factor form: the typed operands are Li (in B's place) and Li^T (scratch)
            SK::convert(c->d_Li, (T*)c->d_BT, g.K, g.Kp, c->st);
            SK::convert_transposed(c->d_Li, (T*)c->d_AbarT, g.K, g.Kp, c->st);
        } else {
            SK::convert(c->d_B, (T*)c->d_BT, g.K, g.Kp, c->st);
            if (c->f16_on()) {
                F16x3Kernels::split_operand(g, c->d_B, c->d_B16, c->d_f16scale, c->d_partial, c->d_sc, c->st);
                F16x3Kernels::v_bound(g, c->d_B, c->d_sc, c->d_f16tmp, c->st);
            }
        }
        HIPCHK(c, hipGetLastError());
        return SCFGP_OK;
    }
    static int pass2(scfgp_ctx* c, int want_grad) {
        const Geom& g = c->g;
        if (c->last_cform) {
            // triangular products: 128-wide LDS-DMA tiles wherever the square products use LDS-DMA.  With the column tile rotated
            // by the row block (apply.hip: the shader engines' round-robin) they beat the loader-staged tiles that pair a long
            // and a short column tile per workgroup: C3 34.4 / 33.5 ms against 40.0 / 34.9 (profiles/r05_tuning.md)
            const int dma = c->dma() ? 1 : 0;
            { ProfScope ps(c, "apply_c");
              SK::apply_c(g, (const T*)c->d_Phi, (const T*)c->d_AbarT, (const T*)c->d_BT, (T*)c->d_C, c->d_vpart, c->alpha(), c->beta(), c->d_mu, c->st, dma); }
            { ProfScope ps(c, "apply_vc");
              SK::apply_vc(g, (const T*)c->d_C, (const T*)c->d_BT, (const T*)c->d_AbarT, (T*)c->d_V, c->st, dma); }
        } else {
            ProfScope ps(c, "apply_v");
            F16Operands f16 = c->f16ops();
            if (want_grad && c->f16_gram()) f16.V16 = c->d_V16g;      // the weighted Gram's operand, from this product's epilogue
            SK::apply_v(g, (const T*)c->d_Phi, (const T*)c->d_BT, (T*)c->d_V, c->d_vpart, c->alpha(), c->d_mu, c->st, c->dma(), c->f16_on() ? &f16 : nullptr);
        }
        const int nb = (int)std::min<int64_t>(g.Np / 4, 2048);
        { ProfScope ps(c, "rowstats");
          SK::rowstats(g, c->d_mu, c->d_vpart, c->d_y, c->d_sc, c->d_p, c->d_q, c->d_partial, nb, c->st);
          reduce_scalars(c->d_partial, nb, 4, c->xs2(), 0, c->st);       // T2, kbar, sum q v, sum p mu
          write_status(c->xs2(), 0.0, 0.0, 0.0, 0.0, c->st); }
        if (want_grad) {
            // factor form: C^T diag(q) C and C^T p (the K x K stage turns them into B W B and u); else V^T diag(q) V = B W B, V^T p = u
            gram_to(c, c->last_cform ? (const T*)c->d_C : (const T*)c->d_V, c->d_q, c->d_p, c->d_xp2, "gram_w");
        }
        HIPCHK(c, hipGetLastError());
        return SCFGP_OK;
    }
    static int adjoint(scfgp_ctx* c) {
        const Geom& g = c->g;
        { ProfScope ps(c, "kstage_adjoint"); unpack_exchange(c, c->d_xp2, c->d_x2);
          if (c->last_cform) kstage_adjoint_factor_form(c->kstage(), c->d_x2, c->d_Abar, c->d_sc, c->st);
          else kstage_adjoint(c->kstage(), c->d_x2, c->d_Abar, c->d_sc, c->st);
          // the K x K part of bbar from the summed G (exchange buffer 1 is intact until the next pass 1) and Abar
          kstage_bbar(c->kstage(), c->d_xp1, c->d_Abar, c->d_partial, c->st); }
        SK::convert(c->d_Abar, (T*)c->d_AbarT, g.K, g.Kp, c->st);
        if (c->f16_on()) F16x3Kernels::split_operand(g, c->d_Abar, c->d_B16, c->d_f16scale, c->d_partial, c->d_sc, c->st);
        HIPCHK(c, hipGetLastError());
        return SCFGP_OK;
    }
    static int pass3(scfgp_ctx* c) {
        const Geom& g = c->g;
        { ProfScope ps(c, "apply_phibar");
          const F16Operands f16 = c->f16ops();
          SK::apply_phibar(g, (const T*)c->d_Phi, (const T*)c->d_AbarT, (T*)c->d_V, c->d_p, c->d_q, c->d_y, c->alpha(), c->ut(), c->st, c->dma(),
                           c->f16_on() ? &f16 : nullptr);
          write_status(c->x3_scalars(), 0.0, 0.0, 0.0, 0.0, c->st); }
        const int ntm = c->Dpp / XT, ntn = g.Jp / XT;
        const int64_t chunk = c->dtype == SCFGP_F32 ? c->gram_chunk : 0;
        c->last_lrb = c->want_lrb();
        if (c->last_lrb) {
            // rank-S form of the backward projection (F = l_F r_F^T, SCFGP.py:83,100): Zbar once, in place over Phibar's cosine half;
            // T~^T Zbar (T~ = [X l_F | 1] is resident from the forward projection); U = Zbar_L + Zbar_M r_F into Phibar's dead
            // sine half; X~^T U.  2 N (S+1) J + 2 N J S + 2 N (D+1) S flops instead of 2 N (D+1) J.
            ProfScope ps(c, "xtz");
            T* Zb = (T*)c->d_V; T* U = (T*)c->d_V + g.Jp;
            SK::zbar_inplace(g, (const T*)c->d_Phi, Zb, c->st);
            SK::rsel(g, c->d_params, (T*)c->d_AbarT, c->st);                       // Abar's typed copy is dead after the product above
            SK::apply_plain(g, Zb, (const T*)c->d_AbarT, U, g.J, g.S, c->st);
            const int nt1 = (c->Spp / XT) * ntn, xs1 = xtz_split(nt1, g.Np);
            SK::tn_plain(c->d_Tt, g.Sp, Zb, g.Kp, g.J, g.Np, xs1, chunk, c->d_slabs, c->st);
            reduce_full_tiles(c->d_slabs, xs1, c->Spp / XT, ntn, c->d_x3, g.Jp, c->st);
            const int nt2 = ntm * (c->Sq / XT), xs2 = xtz_split(nt2, g.Np);
            SK::tn_plain(c->d_Xt, g.Dp, U, g.Kp, g.S, g.Np, xs2, chunk, c->d_slabs, c->st);
            reduce_full_tiles(c->d_slabs, xs2, ntm, c->Sq / XT, c->x3_xu(), c->Sq, c->st);
            HIPCHK(c, hipGetLastError());
            return SCFGP_OK;
        }
        const int xs = c->xtz_nsplit > 0 ? (int)std::min<int64_t>(c->xtz_nsplit, g.Np / 64) : xtz_split(ntm * ntn, g.Np);
        { ProfScope ps(c, "xtz");
          SK::xtz(g, c->d_Xt, (const T*)c->d_Phi, (const T*)c->d_V, xs, chunk, c->d_slabs, c->st);
          reduce_full_tiles(c->d_slabs, xs, ntm, ntn, c->d_x3, g.Jp, c->st); }
        HIPCHK(c, hipGetLastError());
        return SCFGP_OK;
    }
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
    static void cov_panel(scfgp_ctx* c, const void* Ca, const void* Cb, int64_t nrows, int64_t Tb, int64_t row_base, int noise, double* out) {
        predcov<T>(c->g, (const T*)Ca, (const T*)Cb, nrows, Tb, row_base, noise, c->d_sc, out, c->st);
    }
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
    // workgroups per row split of the Gram launch on the context's geometry (update_splits)
    static int gram_jobs(const scfgp_ctx* c) { return SK::gram_jobs(c->g); }
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

#define DISPATCH(c, fn, ...) ((c)->dtype == SCFGP_F32 ? Impl<float>::fn(__VA_ARGS__) : Impl<double>::fn(__VA_ARGS__))

static int ready(scfgp_ctx* c) {
    if (!c) return SCFGP_EARG;
    if (!c->have_params || !c->have_data) { c->err = "parameters and data must be set first"; return SCFGP_EARG; }
    if (hipSetDevice(c->device) != hipSuccess) { c->err = "hipSetDevice failed"; return SCFGP_EHIP; }
    return SCFGP_OK;
}

// scfgp_eval_rows leaves a gathered minibatch as the working set; every entry point that evaluates "the resident
// rows" (scfgp_eval with X == NULL, the staged path, scfgp_train) first brings all rows of the data set back,
// with the n_global it was uploaded with (the reference refits on all N rows after minibatch training, SCFGP.py:265)
static int restore_full_set(scfgp_ctx* c) {
    if (!c->have_data || c->work_full) return SCFGP_OK;
    return load_working_set(c, nullptr, c->Nstore, c->Nglobal_full);
}

// with a communicator attached (scfgp_comm_init) every sweep ends in its sum over the ranks, enqueued on the context's own
// stream right behind the sweep: no fences, no host in between
static int comm_sum(scfgp_ctx* c, int stage, const char* name) {
    if (!c->comm) return SCFGP_OK;
    void* p = nullptr; int64_t n = 0;
    if (int rc = scfgp_exchange(c, stage, &p, &n)) return rc;
    ProfScope ps(c, name);
    const ncclResult_t r = rccl().all_reduce(p, p, (size_t)n, ncclFloat64, ncclSum, c->comm, c->st);
    if (r != ncclSuccess) { c->err = std::string("ncclAllReduce: ") + rccl().err_string(r); return SCFGP_EHIP; }
    return SCFGP_OK;
}

// test-only fault injection (option "test_fail_stage"): the next call of sweep `stage` fails before it enqueues anything
static int injected_failure(scfgp_ctx* c, int stage) {
    if (c->test_fail_stage != stage) return SCFGP_OK;
    c->test_fail_stage = 0;
    c->err = "pass" + std::to_string(stage) + ": injected failure (option test_fail_stage)";
    return SCFGP_EHIP;
}

// Ranks commit to ONE precision level (auto policy of fp32 mode).  A level is raised when the condition estimate asks for it --
// the estimate comes from the summed matrix, so every rank tries at the same evaluation -- but whether the row buffers of the
// level can be allocated is a rank's own affair.  The evaluation after such an attempt therefore carries, in the scalar tail of
// exchange 1 (common.h: XS_CAP1, XS_CAP2, XS_RAN1), how many ranks cannot reach level 1 / level 2 and how many formed their
// pass-1 Gram in fp64; once the sum over ranks is there every rank reads the same counts and
//   * takes the lowest attainable level as its own limit (a refusal anywhere is then recorded everywhere),
//   * continues if pass 1 of every rank already had the form of that level (levels 1 and 2 share pass 1),
//   * else asks for the stages again (SCFGP_REDO) -- all ranks do, the refusing one included --
// before pass 2, whose exchange would otherwise sum C^T diag(q) C on one rank with B W B on another.  One stream
// synchronisation, in that evaluation only.  Without peers the counts are the context's own and nothing changes.
static int settle_level(scfgp_ctx* c) {
    if (!c->unsettled || c->dtype != SCFGP_F32 || c->gram64 != 2) { c->unsettled = false; return SCFGP_OK; }
    double xs[8];
    HIPCHK(c, hipMemcpyAsync(xs, c->xs1(), sizeof(xs), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    c->unsettled = false;
    const int agreed = xs[XS_CAP1] > 0.5 ? 0 : (xs[XS_CAP2] > 0.5 ? 1 : 2);
    if (agreed < c->cap()) {
        c->esc_denied = agreed + 1;
        c->err = "precision level " + std::to_string(agreed + 1) + " refused on another rank; every rank stays at level " + std::to_string(agreed) + " or below";
    }
    if (c->esc_level > agreed) {
        c->esc_level = agreed;
        if (c->gexec) { hipGraphExecDestroy(c->gexec); c->gexec = nullptr; }
        if (c->graph) { hipGraphDestroy(c->graph); c->graph = nullptr; }
        c->warm = false;
    }
    if (agreed < 1 && xs[XS_RAN1] > 0.5) { c->stage = 0; return SCFGP_REDO; }   // some rank's G is an fp64 one: everybody forms it again in fp32
    c->last_cform = c->want_cform(); c->last_level = c->level();               // pass 2 in the form of the agreed level
    return SCFGP_OK;
}

extern "C" int scfgp_pass1(scfgp_ctx* c) {
    if (int rc = ready(c)) return rc;
    if (int rc = restore_full_set(c)) return rc;
    if (c->prof) { c->recs.clear(); c->pool_used = 0; }
    if (int rc = injected_failure(c, 1)) return rc;
    if (int rc = DISPATCH(c, pass1, c)) return rc;
    c->stage = 1;
    return comm_sum(c, 1, "exchange1");
}
extern "C" int scfgp_factor(scfgp_ctx* c) {
    if (int rc = ready(c)) return rc;
    if (c->stage != 1) { c->err = "factor: call pass1 first"; return SCFGP_EARG; }
    if (int rc = settle_level(c)) return rc;                     // SCFGP_REDO: start again at scfgp_pass1
    if (int rc = DISPATCH(c, factor, c)) return rc;
    if (!g_scfgp_capturing) HIPCHK(c, hipEventRecord(c->ev_factor, c->st));
    c->stage = 2; return SCFGP_OK;
}
extern "C" int scfgp_pass2(scfgp_ctx* c, int want_grad) {
    if (int rc = ready(c)) return rc;
    if (c->stage != 2) { c->err = "pass2: call factor first"; return SCFGP_EARG; }
    if (int rc = injected_failure(c, 2)) return rc;
    if (int rc = DISPATCH(c, pass2, c, want_grad)) return rc;
    c->last_want_grad = want_grad; c->stage = 3;
    return comm_sum(c, 2, "exchange2");
}
extern "C" int scfgp_adjoint(scfgp_ctx* c) {
    if (int rc = ready(c)) return rc;
    if (c->stage != 3 || !c->last_want_grad) { c->err = "adjoint: call pass2(want_grad=1) first"; return SCFGP_EARG; }
    if (int rc = DISPATCH(c, adjoint, c)) return rc;
    c->stage = 4; return SCFGP_OK;
}
extern "C" int scfgp_pass3(scfgp_ctx* c) {
    if (int rc = ready(c)) return rc;
    if (c->stage != 4) { c->err = "pass3: call adjoint first"; return SCFGP_EARG; }
    if (int rc = injected_failure(c, 3)) return rc;
    if (int rc = DISPATCH(c, pass3, c)) return rc;
    c->stage = 5;
    return comm_sum(c, 3, "exchange3");
}

// A rank that cannot compute sweep `stage` of the evaluation in progress still owes its peers the sum that ends the sweep:
// this marks exchange buffer `stage` as failed (XS_FAIL; its other contents are whatever they were) and, with a communicator
// attached, enqueues the all-reduce.  Called for every remaining exchange of the evaluation (want_grad sizes exchange 2 and
// decides whether there is a third), it lets the peers run to their scfgp_finish, where the summed XS_FAIL makes all of them
// return SCFGP_EPEER -- nobody waits in a collective for a rank that has left.  A sticky HIP error
// (a faulted kernel) cannot be helped this way: the calls below fail too.
extern "C" int scfgp_fail_stage(scfgp_ctx* c, int stage, int want_grad) {
    if (!c || stage < 1 || stage > 3 || (stage == 3 && !want_grad)) return SCFGP_EARG;
    const std::string keep = c->err;                             // the caller still wants the message of what failed
    if (hipSetDevice(c->device) != hipSuccess) return SCFGP_EHIP;
    c->last_want_grad = want_grad;
    double* xs = stage == 1 ? c->xs1() : (stage == 2 ? c->xs2() : c->x3_scalars());
    write_status(xs, 0.0, c->cap() < 1 ? 1.0 : 0.0, c->cap() < 2 ? 1.0 : 0.0, 1.0, c->st);
    const int rc = comm_sum(c, stage, stage == 1 ? "exchange1" : (stage == 2 ? "exchange2" : "exchange3"));
    c->stage = 0;
    if (rc == SCFGP_OK) c->err = keep;
    return rc;
}
// the exchanges of the evaluation in progress that have not been summed yet, all failed (native sums: scfgp_eval, scfgp_train)
static void fail_rest(scfgp_ctx* c, int want_grad) {
    const int st = c->stage, next = st < 1 ? 1 : (st < 3 ? 2 : (st < 5 ? 3 : 4));
    for (int s = next; s <= (want_grad ? 3 : 2); ++s)
        if (scfgp_fail_stage(c, s, want_grad) != SCFGP_OK) return;
}

extern "C" int scfgp_exchange(scfgp_ctx* c, int stage, void** dev_ptr, int64_t* count) {
    if (!c || !dev_ptr || !count) return SCFGP_EARG;
    if (stage == 1) { *dev_ptr = c->d_xp1; *count = c->n_xp; }
    else if (stage == 2) {
        if (c->last_want_grad) { *dev_ptr = c->d_xp2; *count = c->n_xp; }
        else { *dev_ptr = c->d_xp2 + c->n_pk + c->g.Kp; *count = 8; }    // forward only: just (T2, kbar)
    }
    else if (stage == 3) { *dev_ptr = c->d_x3; *count = c->n_x3; }
    else return SCFGP_EARG;
    return SCFGP_OK;
}

// Explicit ordering between the library's stream and the stream the host framework issues its collective on:
//   direction 0: `peer` waits for everything queued on the library's stream (call before the all-reduce)
//   direction 1: the library's stream waits for everything queued on `peer` (call after the all-reduce)
// A no-op when both are the same stream.  peer == NULL names the legacy default stream.
extern "C" int scfgp_stream_fence(scfgp_ctx* c, void* peer_stream, int direction) {
    if (!c || (direction != 0 && direction != 1)) return SCFGP_EARG;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t peer = (hipStream_t)peer_stream;
    if (peer == c->st) return SCFGP_OK;
    hipStream_t from = direction == 0 ? c->st : peer, to = direction == 0 ? peer : c->st;
    HIPCHK(c, hipEventRecord(c->ev_fence, from));
    HIPCHK(c, hipStreamWaitEvent(to, c->ev_fence, 0));
    return SCFGP_OK;
}

// alpha and Li are final once scfgp_factor has run; their copy to the host (K^2 doubles, 35.7 MB at
// K = 2112) goes on a second stream so it overlaps passes 2 and 3 instead of trailing the evaluation
extern "C" int scfgp_fetch_factors(scfgp_ctx* c, double* alpha, double* Li) {
    if (int rc = ready(c)) return rc;
    if (c->stage < 2) { c->err = "fetch_factors: call factor first"; return SCFGP_EARG; }
    const Geom& g = c->g;
    // The factors are final once the factor stage is done.  They cross PCIe on the copy stream into pinned memory
    // while the sweeps already queued behind the factor stage keep the GPU busy, and the host moves them on into the
    // caller's (pageable) arrays during those sweeps instead of after the last one.
    const size_t K = (size_t)g.K;
    if (!c->h_pin) HIPCHK(c, hipHostMalloc((void**)&c->h_pin, sizeof(double) * (K * K + K), hipHostMallocDefault));
    HIPCHK(c, hipStreamWaitEvent(c->copy_st, c->ev_factor, 0));
    if (alpha) HIPCHK(c, hipMemcpyAsync(c->h_pin + K * K, c->alpha(), sizeof(double) * K, hipMemcpyDeviceToHost, c->copy_st));
    if (Li) HIPCHK(c, hipMemcpy2DAsync(c->h_pin, sizeof(double) * K, c->d_Li, sizeof(double) * g.Kp, sizeof(double) * K, K,
                                       hipMemcpyDeviceToHost, c->copy_st));
    HIPCHK(c, hipStreamSynchronize(c->copy_st));
    if (alpha) memcpy(alpha, c->h_pin + K * K, sizeof(double) * K);
    if (Li) memcpy(Li, c->h_pin, sizeof(double) * K * K);
    return SCFGP_OK;
}

static void enqueue_epilogue(scfgp_ctx* c, int want_grad) {
    const Geom& g = c->g;
    ProfScope ps(c, "epilogue");
    if (want_grad && c->last_lrb)
        grad_epilogue(g, c->d_params, c->d_F, nullptr, 0, c->d_work, c->d_scalars, c->Nglobal, c->d_grad, c->st, c->d_x3, g.Jp, c->x3_xu(), c->Sq);
    else
        grad_epilogue(g, c->d_params, c->d_F, c->d_x3, g.Jp, c->d_work, c->d_scalars, c->Nglobal, want_grad ? c->d_grad : nullptr, c->st);
    finalize_cost(g, c->d_sc, c->d_scalars, c->xs1(), c->xs2(), c->Nglobal, c->d_grad, want_grad, c->st);
}

// Automatic precision level for the NEXT evaluation from the condition estimate of the one just finished (and, when that
// one ran below the level its own estimate asks for, SCFGP_REDO).  A Cholesky that failed on the fp32 Gram is retried on
// the fp64 one before it is reported.
static int update_level(scfgp_ctx* c, bool notpd, bool want_grad, bool may_redo = true) {
    if (c->dtype != SCFGP_F32 || c->gram64 != 2) return SCFGP_OK;
    const double est = c->cond_est();
    int want = notpd || !std::isfinite(est) ? 2 : c->want_level(est, 1.0);
    const int top = c->esc_denied > 0 ? std::min(want, c->esc_denied - 1) : want;     // levels refused before are not tried again
    if (top > c->esc_level) {
        // the buffers of the higher level first; the level is committed only when they exist.  If they cannot be allocated
        // (~17 GB at the headline shape for level 1, N Kp 4 bytes more for level 2) the context stays usable at the level below:
        // scfgp_get_condition keeps reporting the estimate and the predicted error, last_error says what was refused.  Row
        // shards: every rank is at this point in the same evaluation (the estimate is the summed matrix's), and the next
        // exchange 1 tells them all what each could allocate (settle_level) -- until then the level is `unsettled`.
        const int old = c->esc_level;
        c->unsettled = true;
        for (int lvl = top; lvl > old; --lvl) {                  // level 2 refused: level 1 may still fit
            c->esc_level = lvl;
            if (!(c->test_deny_level > 0 && lvl >= c->test_deny_level) && ensure_aux_rows(c) == SCFGP_OK) break;
            if (c->test_deny_level > 0 && lvl >= c->test_deny_level) c->err = "refused by option test_deny_level";
            (void)hipGetLastError();
            c->esc_level = lvl - 1; c->esc_denied = lvl;
            c->err = "precision level " + std::to_string(lvl) + " refused (auxiliary row buffers could not be allocated); staying at level " +
                     std::to_string(lvl - 1) + ": " + c->err;
        }
    }
    // Whether the evaluation is repeated depends on `top` -- the demand of the summed estimate under the limit the ranks last agreed
    // on, the same number on every rank -- and NOT on what this rank could allocate just now: a rank whose buffers were refused
    // repeats with the others (at its lower level) and tells them in the next exchange 1 (settle_level); deciding from its own
    // outcome it would return while they wait for it in that exchange.
    want = top;
    // level 2 only serves the gradient: a forward-only evaluation at level 1 is final
    if (may_redo && (want_grad ? want : std::min(want, 1)) > c->last_level) {
        if (c->gexec) { hipGraphExecDestroy(c->gexec); c->gexec = nullptr; }
        if (c->graph) { hipGraphDestroy(c->graph); c->graph = nullptr; }
        c->warm = false;
        if (int rc = ensure_aux_rows(c)) return rc;
        if (notpd) HIPCHK(c, hipMemsetAsync(c->d_flag, 0, sizeof(int) * 4, c->st));
        return SCFGP_REDO;
    }
    if ((c->use64() && c->phi64_cap < c->g.Np) || (c->want_cform() && c->c_cap < c->g.Np)) {   // level raised without a repeat (scfgp_train, forward-only)
        if (c->gexec) { hipGraphExecDestroy(c->gexec); c->gexec = nullptr; }
        if (c->graph) { hipGraphDestroy(c->graph); c->graph = nullptr; }
        c->warm = false;
        if (int rc = ensure_aux_rows(c)) return rc;
    }
    if (!notpd) {
        const int keep = c->want_level(est, 0.25);             // hysteresis: drop only well below the threshold
        if (keep < c->esc_level) {
            c->esc_level = keep;
            if (c->gexec) { hipGraphExecDestroy(c->gexec); c->gexec = nullptr; }
            if (c->graph) { hipGraphDestroy(c->graph); c->graph = nullptr; }
            c->warm = false;
        }
    }
    return SCFGP_OK;
}

extern "C" int scfgp_finish(scfgp_ctx* c, int want_grad, double* cost, double* grad, double* alpha, double* Li) {
    if (int rc = ready(c)) return rc;
    if ((want_grad && c->stage != 5) || (!want_grad && c->stage != 3)) { c->err = "finish: evaluation incomplete"; return SCFGP_EARG; }
    const Geom& g = c->g;
    enqueue_epilogue(c, want_grad);
    double h_cost = 0, h_fail[3] = {0, 0, 0}; int h_flag[4] = {0, 0, 0, 0};
    {
        ProfScope ps(c, "d2h");
        HIPCHK(c, hipMemcpyAsync(&h_fail[0], c->xs1() + XS_FAIL, sizeof(double), hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipMemcpyAsync(&h_fail[1], c->xs2() + XS_FAIL, sizeof(double), hipMemcpyDeviceToHost, c->st));
        if (want_grad) HIPCHK(c, hipMemcpyAsync(&h_fail[2], c->x3_scalars() + XS_FAIL, sizeof(double), hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipMemcpyAsync(&h_cost, c->d_scalars + R_COST, sizeof(double), hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipMemcpyAsync(c->cond, c->d_scalars + R_LMIN2, sizeof(double) * 3, hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipMemcpyAsync(h_flag, c->d_flag, sizeof(int) * 4, hipMemcpyDeviceToHost, c->st));
        if (want_grad && grad) HIPCHK(c, hipMemcpyAsync(grad, c->d_grad, sizeof(double) * g.P, hipMemcpyDeviceToHost, c->st));
        if (alpha) HIPCHK(c, hipMemcpyAsync(alpha, c->alpha(), sizeof(double) * g.K, hipMemcpyDeviceToHost, c->st));
        if (Li) HIPCHK(c, hipMemcpy2DAsync(Li, sizeof(double) * g.K, c->d_Li, sizeof(double) * g.Kp, sizeof(double) * g.K, g.K,
                                           hipMemcpyDeviceToHost, c->st));
    }
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    c->stage = 0; c->warm = true;
    if (cost) *cost = h_cost;
    if (h_fail[0] + h_fail[1] + h_fail[2] > 0.5) {              // summed over the ranks: the same verdict everywhere, no level decision from it
        c->cond_valid = false;
        c->err = "a rank failed in this evaluation (exchange 1 / 2 / 3: " + std::to_string((int)h_fail[0]) + " / " + std::to_string((int)h_fail[1]) +
                 " / " + std::to_string((int)h_fail[2]) + " ranks): its results are not valid on any rank";
        return SCFGP_EPEER;
    }
    if (int rc = update_level(c, h_flag[0] != 0, want_grad != 0)) return rc;    // SCFGP_REDO: repeat the evaluation at the higher level
    c->cond_valid = true;
    if (h_flag[0]) { c->err = "Phi^T Phi + (e^{2a}+1e-6) I is not positive definite"; return SCFGP_ENOTPD; }
    if (!std::isfinite(h_cost)) { c->err = "non-finite cost"; return SCFGP_ENONFINITE; }
    return SCFGP_OK;
}

static int pass1_current(scfgp_ctx* c) {                  // pass 1 on the working set as it stands (full or gathered)
    if (int rc = ready(c)) return rc;
    if (c->prof) { c->recs.clear(); c->pool_used = 0; }
    if (int rc = injected_failure(c, 1)) return rc;
    if (int rc = DISPATCH(c, pass1, c)) return rc;
    c->stage = 1;
    return comm_sum(c, 1, "exchange1");
}
static int run_eval(scfgp_ctx* c, int want_grad, double* cost, double* grad, double* alpha, double* Li, bool subset = false) {
    int rc = SCFGP_OK;
    // with the sums inside the library a rank that fails still posts the remaining all-reduces of the evaluation (fail_rest)
    const auto leave = [&](int code) { if (code < 0 && c->comm) fail_rest(c, want_grad); return code; };
    for (int attempt = 0; attempt < 5; ++attempt) {              // at most two escalations (levels 0 -> 1 -> 2) and their settling
        if ((rc = subset ? pass1_current(c) : scfgp_pass1(c))) return leave(rc);
        if ((rc = scfgp_factor(c)) == SCFGP_REDO) continue;       // the ranks agreed on a lower level than some of them ran pass 1 at
        if (rc) return leave(rc);
        if ((rc = scfgp_pass2(c, want_grad))) return leave(rc);
        if (want_grad) {
            if ((rc = scfgp_adjoint(c))) return leave(rc);
            if ((rc = scfgp_pass3(c))) return leave(rc);
        }
        // everything is queued: the factor outputs now stream to the host beside passes 2 and 3
        if ((alpha || Li) && (rc = scfgp_fetch_factors(c, alpha, Li))) return rc;
        rc = scfgp_finish(c, want_grad, cost, grad, nullptr, nullptr);
        if (rc != SCFGP_REDO) return rc;
    }
    return rc;
}

extern "C" int scfgp_eval(scfgp_ctx* c, const double* X, const double* y, int64_t N, int want_grad,
                          double* cost, double* grad, double* alpha, double* Li) {
    if (!c) return SCFGP_EARG;
    int rc;
    if (X) { if ((rc = scfgp_set_data(c, X, y, N, N))) return rc; }
    return run_eval(c, want_grad, cost, grad, alpha, Li);      // scfgp_pass1 brings all rows back after a row subset
}

extern "C" int scfgp_eval_rows(scfgp_ctx* c, const int64_t* idx, int64_t n, int want_grad,
                               double* cost, double* grad, double* alpha, double* Li) {
    if (!c || !idx || n < 1) { if (c) c->err = "eval_rows: bad arguments"; return SCFGP_EARG; }
    if (!c->have_data || c->Nstore < 1) { c->err = "eval_rows: no resident data set"; return SCFGP_EARG; }
    for (int64_t i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= c->Nstore) { c->err = "eval_rows: index out of range"; return SCFGP_EARG; }
    HIPCHK(c, hipSetDevice(c->device));
    if (n > c->idx_cap) {
        HIPCHK(c, hipStreamSynchronize(c->st));
        dfree(c->d_idx);
        if (int rc = dmalloc(c, &c->d_idx, sizeof(int64_t) * n)) return rc;
        c->idx_cap = n;
    }
    HIPCHK(c, hipMemcpyAsync(c->d_idx, idx, sizeof(int64_t) * n, hipMemcpyHostToDevice, c->st));
    if (int rc = load_working_set(c, c->d_idx, n, n)) return rc;       // per-batch N, as SCFGP.py:126,128
    return run_eval(c, want_grad, cost, grad, alpha, Li, true);
}

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
    DISPATCH(c, type_factor, c, L64, LiT, Li_typed);
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
// posterior sample functions (sample.hip; derivation and random-number contract in include/scfgp_hip.h)
// ----------------------------------------------------------------------------------------------
static constexpr int SAMPLE_MAX = 1024;
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
// absorbing new observations into a fitted posterior (kernels_kstage.hip: kstage_update; derivation in include/scfgp_hip.h)
// ----------------------------------------------------------------------------------------------
// row splits of the update's Gram product over a chunk of Np rows, and the slabs they need
static RowSplits update_splits(const scfgp_ctx* c, int64_t Np, bool wide = false) {
    if (wide) return gram_row_splits(Impl<double>::gram_jobs(c), Np, false, 0, 1);     // the fp64 job list in an fp32 context
    return gram_row_splits(DISPATCH(c, gram_jobs, c), Np, c->dtype == SCFGP_F32, 0, 1);
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
    if (wide) Impl<double>::type_factor(c, c->u_Li, ops.LiT, ops.Li);
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
        if ((rc = wide ? Impl<double>::update_chunk(c, g, update_splits(c, g.Np, true), ops, out, have_rows)
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
    update_check_finite(c->u_S, K2, c->u_flag, c->st);
    update_check_finite(k.alpha_out, Kp, c->u_flag, c->st);
    update_store_factor(c->u_S, g0.K, g0.Kp, feed.raw, c->st);
    HIPCHK(c, hipGetLastError());
    int flags[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(flags, c->u_flag, sizeof(flags), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (flags[1]) return fail.nonfinite(std::string("non-finite rows, ") + what + " or factors");
    if (flags[0]) return fail.set("I + C^T C is not positive definite", SCFGP_ENOTPD);
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
// api_host.h), whose features are expanded into nb observation rows each (Impl::gradobs_chunk).  A job uploads [X | yn | Gn | rho] of its
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
        if (int r = Impl<double>::gradobs_chunk(c, g, gr, ops, obs)) return r;      // fp64 operands in every context
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
    // one allocation: meas | psi1 | Ed | E | Eb | phibar | W | A | f0 | sums | units | rec
    const int64_t n_meas = 3 * D, n_tab = 2 * (int64_t)D * Jt, n_e = 2 * Jt, n_w = (int64_t)K * nw, n_a = 2 * (int64_t)Jt * nw,
                  n_sums = (int64_t)nsets * nw, n_units = (3 * nunits + 1) / 2, n_rec = nunits * nsets * pass;
    DevTmp buf;
    if (int rc = dmalloc(c, &buf.p, sizeof(double) * (n_meas + 2 * n_tab + 2 * n_e + K + n_w + n_a + nw + n_sums + n_units + n_rec))) return rc;
    double* d_meas = buf.p; double* d_psi1 = d_meas + n_meas; double* d_Ed = d_psi1 + n_tab; double* d_E = d_Ed + n_tab;
    double* d_Eb = d_E + n_e; double* d_phibar = d_Eb + n_e; double* d_W = d_phibar + K; double* d_A = d_W + n_w; double* d_f0 = d_A + n_a;
    double* d_sums = d_f0 + nw; int* d_units = (int*)(d_sums + n_sums); double* d_rec = d_sums + n_sums + n_units;

    std::vector<double> h(std::max<int64_t>(n_meas, K + nw + n_sums));
    sobol_measure(kind, p0, p1, D, h.data());
    HIPCHK(c, hipMemcpyAsync(d_meas, h.data(), sizeof(double) * n_meas, hipMemcpyHostToDevice, c->st));
    if (cols) HIPCHK(c, hipMemcpyAsync(d_W, W, sizeof(double) * n_w, hipMemcpyHostToDevice, c->st));
    if (nunits) HIPCHK(c, hipMemcpyAsync(d_units, units.data(), sizeof(int) * 3 * nunits, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));                      // h is reused for the results
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

// ----------------------------------------------------------------------------------------------
// on-device optimiser and the captured training iteration
// ----------------------------------------------------------------------------------------------
extern "C" int scfgp_opt_init(scfgp_ctx* c, int algo, const double* hyper, int nhyper, double momentum) {
    if (!c || algo < 0 || algo > 5 || !hyper || nhyper < 4) { if (c) c->err = "opt_init: bad arguments"; return SCFGP_EARG; }
    HIPCHK(c, hipSetDevice(c->device));
    const int P = c->g.P;
    if (!c->d_opt) {
        if (int rc = dmalloc(c, &c->d_opt, sizeof(double) * 3 * P)) return rc;
        if (int rc = dmalloc(c, &c->d_tctr, sizeof(double) * 8)) return rc;
    }
    HIPCHK(c, hipMemsetAsync(c->d_opt, 0, sizeof(double) * 3 * P, c->st));
    HIPCHK(c, hipMemsetAsync(c->d_tctr, 0, sizeof(double) * 8, c->st));
    c->opt_algo = algo;
    c->opt_h = OptHyper{hyper[0], hyper[1], hyper[2], hyper[3], momentum};
    if (c->gexec) { hipGraphExecDestroy(c->gexec); c->gexec = nullptr; }
    if (c->graph) { hipGraphDestroy(c->graph); c->graph = nullptr; }
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SCFGP_OK;
}

// which: 0 = s1, 1 = s2, 2 = velocity (P doubles each), 3 = step counter t (1 double)
extern "C" int scfgp_opt_state(scfgp_ctx* c, int set, int which, double* buf) {
    if (!c || !buf || c->opt_algo < 0 || which < 0 || which > 3) return SCFGP_EARG;
    HIPCHK(c, hipSetDevice(c->device));
    double* dev = which == 3 ? c->d_tctr : c->d_opt + (int64_t)which * c->g.P;
    const size_t bytes = sizeof(double) * (which == 3 ? 1 : c->g.P);
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (set) HIPCHK(c, hipMemcpy(dev, buf, bytes, hipMemcpyHostToDevice));
    else HIPCHK(c, hipMemcpy(buf, dev, bytes, hipMemcpyDeviceToHost));
    return SCFGP_OK;
}

// One step of the device rule with a caller-supplied gradient (P doubles on the host): the parameter vector and the rule's
// state advance exactly as inside scfgp_train, without an evaluation -- for callers that form the gradient elsewhere and for
// known-answer tests of the rule itself (tests/golden/optimizer_kats.npz).
extern "C" int scfgp_opt_step(scfgp_ctx* c, const double* grad, int P) {
    if (!c || !grad || P != c->g.P) { if (c) c->err = "opt_step: wrong gradient length"; return SCFGP_EARG; }
    if (c->opt_algo < 0 || !c->have_params) { c->err = "opt_step: call scfgp_set_params and scfgp_opt_init first"; return SCFGP_EARG; }
    if (c->stage != 0) { c->err = "opt_step: a staged evaluation is in progress (finish it first: its later stages would run on other parameters)"; return SCFGP_EARG; }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(c->d_grad, grad, sizeof(double) * P, hipMemcpyHostToDevice, c->st));
    opt_update(c->opt_algo, c->opt_h, P, c->d_params, c->d_grad, c->d_opt, c->d_tctr, c->d_scalars, nullptr, 0, c->st);
    unpack_params(c->g, c->d_params, c->d_F, c->d_Fall, c->d_Lall, c->d_Rall, c->d_sc, c->st);
    HIPCHK(c, hipMemcpyAsync(c->h_params.data(), c->d_params, sizeof(double) * P, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    c->cond_valid = false;
    return SCFGP_OK;
}

// One training iteration, enqueued.  With a communicator attached the three sums over ranks are part of it (ncclAllReduce on
// the context's stream right behind each sweep); every rank then applies the same deterministic rule to the same summed
// gradient, so the parameter vectors stay bit-equal without a broadcast.  c->stage follows the sweeps so that a failing rank
// can tell which exchanges it still owes (fail_rest).
static int enqueue_train_iter(scfgp_ctx* c) {
    int rc;
    c->stage = 0; c->last_want_grad = 1;
    if ((rc = injected_failure(c, 1))) return rc;
    if ((rc = DISPATCH(c, pass1, c))) return rc;
    c->stage = 1;
    if ((rc = comm_sum(c, 1, "exchange1"))) return rc;
    if ((rc = DISPATCH(c, factor, c))) return rc;
    c->stage = 2;
    if ((rc = injected_failure(c, 2))) return rc;
    if ((rc = DISPATCH(c, pass2, c, 1))) return rc;
    c->stage = 3;
    if ((rc = comm_sum(c, 2, "exchange2"))) return rc;
    if ((rc = DISPATCH(c, adjoint, c))) return rc;
    c->stage = 4;
    if ((rc = injected_failure(c, 3))) return rc;
    if ((rc = DISPATCH(c, pass3, c))) return rc;
    c->stage = 5;
    if ((rc = comm_sum(c, 3, "exchange3"))) return rc;
    enqueue_epilogue(c, 1);
    opt_update(c->opt_algo, c->opt_h, c->g.P, c->d_params, c->d_grad, c->d_opt, c->d_tctr, c->d_scalars, c->d_hist, c->hist_cap, c->st);
    unpack_params(c->g, c->d_params, c->d_F, c->d_Fall, c->d_Lall, c->d_Rall, c->d_sc, c->st);
    HIPCHK(c, hipGetLastError());
    return SCFGP_OK;
}

extern "C" int scfgp_train(scfgp_ctx* c, int n_iters, double* cost_hist, double* alpha, double* Li) {
    if (int rc = ready(c)) return rc;
    if (c->opt_algo < 0 || n_iters < 1) { c->err = "train: call scfgp_opt_init first"; return SCFGP_EARG; }
    if (int rc = restore_full_set(c)) return rc;
    if (!c->comm && c->Nglobal != c->g.N) {                      // a shard without its peers would train on its own rows' sums
        c->err = "train: the resident rows are a shard (n_global != N) but no communicator is attached (scfgp_comm_init); the "
                 "on-device loop needs the sums over ranks inside the library";
        return SCFGP_EARG;
    }
    const Geom& g = c->g;
    if (n_iters > c->hist_cap) {
        dfree(c->d_hist);
        if (int rc = dmalloc(c, &c->d_hist, sizeof(double) * n_iters)) return rc;
        c->hist_cap = n_iters;
        if (c->gexec) { hipGraphExecDestroy(c->gexec); c->gexec = nullptr; }
        if (c->graph) { hipGraphDestroy(c->graph); c->graph = nullptr; }
    }
    // auto precision level, condition of the current parameters unknown (no evaluation since they or the rows were set):
    // one pass 1 + factor stage as a probe, so that the iterations of this call run at the level their first one needs
    // (row shards: the probe ends in exchange 1 like any pass 1, and a level raised or refused since the last sum over ranks
    // is settled here, before the iterations -- possibly one captured graph -- are enqueued)
    for (int round = 0; round < 5 && c->dtype == SCFGP_F32 && c->gram64 == 2 && (!c->cond_valid || c->unsettled); ++round) {
        int rc;
        c->stage = 0;
        if ((rc = injected_failure(c, 1)) || (rc = DISPATCH(c, pass1, c))) {
            if (c->comm) (void)scfgp_fail_stage(c, 1, 1);         // the peers' probes wait in exchange 1; they read the mark and stop there too
            return rc;
        }
        c->stage = 1;
        if ((rc = comm_sum(c, 1, "exchange1"))) return rc;
        if ((rc = settle_level(c)) == SCFGP_REDO) continue;
        if (rc) return rc;
        if ((rc = DISPATCH(c, factor, c))) return rc;
        int h_flag[4] = {0, 0, 0, 0}; double h_fail = 0;
        HIPCHK(c, hipMemcpyAsync(c->cond, c->d_scalars + R_LMIN2, sizeof(double) * 3, hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipMemcpyAsync(h_flag, c->d_flag, sizeof(int) * 4, hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipMemcpyAsync(&h_fail, c->xs1() + XS_FAIL, sizeof(double), hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipStreamSynchronize(c->st));
        c->stage = 0;
        if (h_fail > 0.5) { c->err = "train: a rank failed in the probe evaluation"; return SCFGP_EPEER; }
        if ((rc = update_level(c, h_flag[0] != 0, true, false))) return rc;
        c->cond_valid = true;
    }
    if (c->unsettled) { c->err = "train: the ranks' precision level did not settle"; return SCFGP_EHIP; }
    HIPCHK(c, hipMemsetAsync(c->d_flag, 0, sizeof(int) * 4, c->st));
    HIPCHK(c, hipMemsetAsync(c->d_tctr + 1, 0, sizeof(double), c->st));
    c->in_train = true;
    int rc = SCFGP_OK, done = 0;
    // the captured iteration: always without a communicator; with one only on request (option use_graph = 2) -- capturing
    // ncclAllReduce is RCCL's business and has not run here with more than one rank, eager launches queue far ahead of the GPU anyway
    const bool graph_ok = c->use_graph && !c->prof && (!c->comm || c->use_graph >= 2);
    if (graph_ok && !c->warm) {                                  // first touch of every kernel: eager
        rc = enqueue_train_iter(c); done = 1;
        if (rc == SCFGP_OK) c->warm = true;
    }
    if (rc == SCFGP_OK && graph_ok && done < n_iters) {
        if (!c->gexec || c->graph_N != g.N) {
            if (c->gexec) { hipGraphExecDestroy(c->gexec); c->gexec = nullptr; }
            if (c->graph) { hipGraphDestroy(c->graph); c->graph = nullptr; }
            hipError_t e = hipStreamBeginCapture(c->st, hipStreamCaptureModeThreadLocal);
            if (e == hipSuccess) {
                g_scfgp_capturing = true;
                rc = enqueue_train_iter(c);
                g_scfgp_capturing = false;
                e = hipStreamEndCapture(c->st, &c->graph);
                if (rc == SCFGP_OK && e == hipSuccess) e = hipGraphInstantiate(&c->gexec, c->graph, nullptr, nullptr, 0);
            }
            if (e != hipSuccess || rc != SCFGP_OK) {                 // fall back to eager launches
                if (c->graph) { hipGraphDestroy(c->graph); c->graph = nullptr; }
                c->gexec = nullptr; (void)hipGetLastError(); rc = SCFGP_OK;
            } else c->graph_N = g.N;
        }
        if (c->gexec)
            for (; done < n_iters && rc == SCFGP_OK; ++done)
                if (hipGraphLaunch(c->gexec, c->st) != hipSuccess) { c->err = "hipGraphLaunch failed"; rc = SCFGP_EHIP; }
    }
    for (; done < n_iters && rc == SCFGP_OK; ++done) {
        if (c->prof) { c->recs.clear(); c->pool_used = 0; }      // timings describe the last eager iteration
        rc = enqueue_train_iter(c);
    }
    c->in_train = false;
    if (rc != SCFGP_OK) {
        // the peers are enqueueing all n_iters iterations: this rank owes them every remaining sum (XS_FAIL set), or they wait
        // in an all-reduce for good; they learn of it from the summed XS_FAIL when their call ends
        if (c->comm && rc < 0) {
            fail_rest(c, 1);
            for (; done < n_iters; ++done) { c->stage = 0; fail_rest(c, 1); }
        }
        c->stage = 0;
        return rc;
    }
    int h_flag[4] = {0, 0, 0, 0}; double h_fail[3] = {0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(&h_fail[0], c->xs1() + XS_FAIL, sizeof(double), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(&h_fail[1], c->xs2() + XS_FAIL, sizeof(double), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(&h_fail[2], c->x3_scalars() + XS_FAIL, sizeof(double), hipMemcpyDeviceToHost, c->st));
    if (cost_hist) HIPCHK(c, hipMemcpyAsync(cost_hist, c->d_hist, sizeof(double) * n_iters, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(c->h_params.data(), c->d_params, sizeof(double) * g.P, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(h_flag, c->d_flag, sizeof(int) * 4, hipMemcpyDeviceToHost, c->st));
    if (alpha) HIPCHK(c, hipMemcpyAsync(alpha, c->alpha(), sizeof(double) * g.K, hipMemcpyDeviceToHost, c->st));
    if (Li) HIPCHK(c, hipMemcpy2DAsync(Li, sizeof(double) * g.K, c->d_Li, sizeof(double) * g.Kp, sizeof(double) * g.K, g.K,
                                       hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(c->cond, c->d_scalars + R_LMIN2, sizeof(double) * 3, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    c->stage = 0;
    if (h_fail[0] + h_fail[1] + h_fail[2] > 0.5) {
        c->cond_valid = false;
        c->err = "train: a rank failed; parameters and optimiser state of this call are not valid on any rank";
        return SCFGP_EPEER;
    }
    // the precision level is fixed inside one call; the last iteration's condition estimate sets it for the next call
    if (int rc = update_level(c, h_flag[0] != 0, true, false)) return rc;
    c->cond_valid = true;
    if (h_flag[0]) { c->err = "Phi^T Phi + (e^{2a}+1e-6) I is not positive definite"; return SCFGP_ENOTPD; }
    if (cost_hist) for (int i = 0; i < n_iters; ++i) if (!std::isfinite(cost_hist[i])) { c->err = "non-finite cost"; return SCFGP_ENONFINITE; }
    return SCFGP_OK;
}

// ----------------------------------------------------------------------------------------------
// row-sharded evaluation with the sums inside the library (RCCL all-reduce over xGMI)
// ----------------------------------------------------------------------------------------------
extern "C" int scfgp_comm_unique_id(void* id128) {
    if (!id128) return SCFGP_EARG;
    if (!rccl().ok()) return SCFGP_EHIP;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    return rccl().get_id((ncclUniqueId*)id128) == ncclSuccess ? SCFGP_OK : SCFGP_EHIP;
}
extern "C" int scfgp_comm_init(scfgp_ctx* c, int nranks, int rank, const void* id128) {
    if (!c || !id128 || nranks < 1 || rank < 0 || rank >= nranks) { if (c) c->err = "comm_init: bad arguments"; return SCFGP_EARG; }
    if (c->comm) { c->err = "comm_init: this context already has a communicator"; return SCFGP_EARG; }
    if (!rccl().ok()) { c->err = "comm_init: librccl.so could not be loaded"; return SCFGP_EHIP; }
    HIPCHK(c, hipSetDevice(c->device));
    ncclUniqueId id; memcpy(&id, id128, sizeof(id));
    const ncclResult_t r = rccl().init_rank(&c->comm, nranks, id, rank);
    if (r != ncclSuccess) { c->comm = nullptr; c->err = std::string("ncclCommInitRank: ") + rccl().err_string(r); return SCFGP_EHIP; }
    c->comm_ranks = nranks; c->comm_rank = rank;
    if (c->gexec) { hipGraphExecDestroy(c->gexec); c->gexec = nullptr; }
    if (c->graph) { hipGraphDestroy(c->graph); c->graph = nullptr; }
    return SCFGP_OK;
}
extern "C" int scfgp_comm_destroy(scfgp_ctx* c) {
    if (!c) return SCFGP_EARG;
    if (c->comm) {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(c->st));
        rccl().destroy(c->comm); c->comm = nullptr; c->comm_ranks = 0;
    }
    return SCFGP_OK;
}

extern "C" int scfgp_get_dims(scfgp_ctx* c, int64_t* out, int n) {
    if (!c || !out || n < 6) return SCFGP_EARG;
    out[0] = c->g.K; out[1] = c->g.Kp; out[2] = c->g.Jp; out[3] = c->g.Dp; out[4] = c->g.Np; out[5] = c->g.P;
    if (n >= 7) out[6] = c->g.tile;
    if (n >= 8) out[7] = c->have_data ? c->Nstore : 0;          // rows made resident by scfgp_set_data
    return SCFGP_OK;
}

extern "C" int scfgp_set_profiling(scfgp_ctx* c, int enable) {
    if (!c) return SCFGP_EARG;
    c->prof = enable != 0; c->recs.clear(); c->pool_used = 0;
    return SCFGP_OK;
}

extern "C" int scfgp_get_timings(scfgp_ctx* c, double* ms, const char** names, int n) {
    if (!c) return SCFGP_EARG;
    hipStreamSynchronize(c->st);
    int k = 0;
    for (const ProfRec& r : c->recs) {
        if (k >= n) break;
        float t = 0;
        if (hipEventElapsedTime(&t, r.e0, r.e1) != hipSuccess) t = -1;
        if (ms) ms[k] = t;
        if (names) names[k] = r.name.c_str();
        ++k;
    }
    return k;
}

// host-only: geometry as scfgp_create derives it (the row-split self-test below runs without a GPU)
static void derive_geom(Geom& g, int D, int S, int M) {
    g.D = D; g.S = S; g.M = M; g.J = S + M; g.K = 2 * g.J; g.P = 3 + D * S + M * S + S + M;
    g.Dp = (int)round_up(D + 1, 16); g.Jp = (int)round_up(g.J, XT);
    g.Sp = (int)round_up(S + 1, 16); g.lowrank = g.Sp < g.Dp;     // F = l_F r_F^T: project through the S columns when that is narrower
    // Gram tile grid: 128-wide tiles cover K in 64-column blocks; an odd block count ends in a 64-high strip
    g.tile = 128;
    g.gfull = (int)(round_up(g.K, 64) / 128);
    g.gstrip = (int)(round_up(g.K, 64) / 64 % 2);
    g.Kp = (g.gfull + g.gstrip) * g.tile;
}
extern "C" int scfgp_selftest_row_splits(int D, int S, int M, int64_t N, int dtype, int nsplit, int taper) {
    if (D < 1 || S < 1 || M < 1 || N < 1) return SCFGP_EARG;
    Geom g{};
    derive_geom(g, D, S, M);
    g.N = N; g.Np = round_up(N, 256);
    const int jobs = dtype == SCFGP_F32 ? SweepKernels<float>::gram_jobs(g) : SweepKernels<double>::gram_jobs(g);
    const RowSplits rs = gram_row_splits(jobs, g.Np, dtype == SCFGP_F32, nsplit, taper);
    if (rs.nsplit < 1 || rs.nsplit != rs.groups * rs.per_group()) return 1;
    int64_t at = 0;
    for (int s = 0; s < rs.nsplit; ++s) {                       // the splits tile [0, Np) in order, on 256-row blocks
        int64_t r0, r1; rs.range(s, r0, r1);
        if (r0 != at || r1 < r0 || r0 % rs.gran || r1 % rs.gran || (rs.gran != 64 && rs.gran != 256)) return 2;
        at = r1;
    }
    return at == g.Np ? 0 : 3;
}

extern "C" int scfgp_set_option(scfgp_ctx* c, const char* name, int64_t value) {
    if (!c || !name) return SCFGP_EARG;
    const std::string s(name);
    if (s == "gram_nsplit") c->gram_nsplit = (int)value;
    else if (s == "gram_taper") c->gram_taper = (int)value;
    else if (s == "apply_dma") { if (value < -1 || value > 2) { c->err = "apply_dma: -1 auto, 0 off, 1 = 128-wide tiles, 2 = 256-wide (fp32)"; return SCFGP_EARG; }
                                 c->apply_dma = (int)value; }
    else if (s == "gram_chunk") c->gram_chunk = value;
    else if (s == "f16_gram") c->f16gram = (int)value;
    else if (s == "lowrank_bwd") c->lowrank_bwd = (int)value;
    else if (s == "xtz_nsplit") c->xtz_nsplit = (int)value;
    else if (s == "use_graph") c->use_graph = (int)value;
    else if (s == "gram64") { if (value < 0 || value > 3) { c->err = "gram64: 0 never, 1 always level 1, 2 auto, 3 always level 2"; return SCFGP_EARG; }
                              c->gram64 = (int)value; c->esc_level = 0; c->esc_denied = 0; }
    else if (s == "factor_form") { if (value < -1 || value > 1) { c->err = "factor_form: -1 auto, 0 never, 1 always"; return SCFGP_EARG; } c->factor_form = (int)value; }
    else if (s == "cond_threshold") c->esc_thr = (double)value;
    else if (s == "cond_threshold_w") c->escw_thr = (double)value;
    else if (s == "roctx") c->roctx_on = value != 0;
    else if (s == "test_deny_level") { c->test_deny_level = (int)value; return SCFGP_OK; }       // tests: levels >= value are refused as if out of memory
    else if (s == "test_pd_group") { c->test_pd_group = (int)value; return SCFGP_OK; }         // tests: scfgp_predict_pd takes at most `value` dimensions per group
    else if (s == "test_sobol_group") { c->test_sobol_group = (int)value; return SCFGP_OK; }   // tests: scfgp_sobol takes at most `value` inputs per workgroup
    else if (s == "test_fail_stage") { c->test_fail_stage = (int)value; return SCFGP_OK; }       // tests: the next sweep `value` (1..3) fails
    else { c->err = "unknown option " + s; return SCFGP_EARG; }
    // kernels not run so far, buffers not allocated so far: the next scfgp_train starts with an eager iteration again
    c->warm = false; c->cond_valid = false;
    if (c->gexec) { hipGraphExecDestroy(c->gexec); c->gexec = nullptr; }
    if (c->graph) { hipGraphDestroy(c->graph); c->graph = nullptr; }
    if (c->have_data) return ensure_rows(c, c->g.N);
    return SCFGP_OK;
}

// out[0] condition estimate of A = Phi^T Phi + lam I from the last finished evaluation: max_i L_ii^2 * max_j (A^-1)_jj, a
//        LOWER bound of cond_2(A) (>= the diagonal ratio max L_ii^2 / min L_ii^2)
// out[1] precision level that evaluation ran at (0, 1, 2: see scfgp_ctx; fp64 mode reports 0)
// out[2] 1 if its G and Phi^T y were formed in fp64 from fp64 features (always in fp64 mode), else 0
// out[3] predicted relative error of alpha / Li had the Gram been formed in fp32: SCFGP_ERR_PER_COND * out[0] (an order of
//        magnitude: measured / predicted = 0.2 .. 7)
// out[4] threshold of level 1, out[5] threshold of level 2 (auto policy), out[6] min L_ii^2, out[7] max L_ii^2, out[8] max_j (A^-1)_jj
extern "C" int scfgp_get_condition(scfgp_ctx* c, double* out, int n) {
    if (!c || !out || n < 4) return SCFGP_EARG;
    const double v[9] = {c->cond_est(), (double)c->last_level, c->last_used64 ? 1.0 : 0.0, c->alpha_err_fp32(),
                         c->esc_thr, c->escw_thr, c->cond[0], c->cond[1], c->cond[2]};
    for (int i = 0; i < n && i < 9; ++i) out[i] = v[i];
    return SCFGP_OK;
}

extern "C" int64_t scfgp_debug_read(scfgp_ctx* c, const char* name, void* host, int64_t max_bytes) {
    if (!c || !name || !host) return SCFGP_EARG;
    const Geom& g = c->g;
    const std::string s(name);
    if (s == "chol_trace") { if (hipStreamSynchronize(c->st) != hipSuccess) return SCFGP_EHIP; return chol_trace_read(host, max_bytes); }
    if (s == "apply_trace") { if (hipStreamSynchronize(c->st) != hipSuccess) return SCFGP_EHIP; return apply_trace_read(host, max_bytes); }
    if (s == "trace") { if (hipStreamSynchronize(c->st) != hipSuccess) return SCFGP_EHIP; return trace_read(host, max_bytes); }
    const int64_t K2 = (int64_t)g.Kp * g.Kp;
    const size_t ts = c->tsize();
    const void* src = nullptr; int64_t bytes = 0;
    DevTmp tmp;
    if (s == "Phi") { src = c->d_Phi; bytes = ts * g.Np * g.Kp; }
    else if (s == "V") { src = c->d_V; bytes = ts * g.Np * g.Kp; }
    else if (s == "G") {                                         // exchange buffer 1 unpacked into a buffer of its own: d_x1 is the
        if (dmalloc(c, &tmp.p, 8 * c->n_x1)) return SCFGP_EHIP;  // factorisation's working matrix from scfgp_factor on
        unpack_exchange(c, c->d_xp1, tmp.p); src = tmp.p; bytes = 8 * c->n_x1;
    }
    else if (s == "W") { if (c->stage == 3) unpack_exchange(c, c->d_xp2, c->d_x2); src = c->d_x2; bytes = 8 * c->n_x2; }
    else if (s == "XZ") { src = c->d_x3; bytes = 8 * c->n_x3; }
    else if (s == "Li") { src = c->d_Li; bytes = 8 * K2; }
    else if (s == "B") { src = c->d_B; bytes = 8 * K2; }
    else if (s == "Abar") { src = c->d_Abar; bytes = 8 * K2; }
    else if (s == "p") { src = c->d_p; bytes = 8 * g.Np; }
    else if (s == "q") { src = c->d_q; bytes = 8 * g.Np; }
    else if (s == "vecs") { src = c->d_vecs; bytes = 8 * 5 * g.Kp; }
    else if (s == "Fall") { src = c->d_Fall; bytes = 8 * (int64_t)g.Dp * g.Jp; }
    else if (s == "Lall") { src = c->d_Lall; bytes = 8 * (int64_t)g.Dp * round_up(g.Sp, 64); }   // factors of the rank-S form; written
    else if (s == "Rall") { src = c->d_Rall; bytes = 8 * (int64_t)g.Sp * g.Jp; }                  // only where it is used (Sp < Dp)
    else if (s == "Xt") { src = c->d_Xt; bytes = 8 * g.Np * g.Dp; }
    else if (s == "pXt") {                                       // the packed, scaled rows of the last chunk of the last posterior call
        if (!c->p_Xt || !c->p_rows) { c->err = "debug_read: pXt exists only after a posterior call"; return SCFGP_EARG; }
        src = c->p_Xt; bytes = 8 * c->p_rows * g.Dp;
    }
    else if (s == "scalars") { src = c->d_scalars; bytes = 8 * 32; }
    else if (s == "C") {                                         // factor form: C = Phi Li^T of the last pass 2 at level 2
        if (!c->d_C || c->c_cap < g.Np || !c->last_cform) { c->err = "debug_read: C exists only after a pass 2 in the factor form (level 2)"; return SCFGP_EARG; }
        src = c->d_C; bytes = ts * g.Np * g.Kp;
    }
    else if (s == "Phi64") {                                     // the fp64 features of an escalated pass 1 (levels 1 and 2)
        if (!c->d_Phi64 || c->phi64_cap < g.Np) { c->err = "debug_read: Phi64 exists only in fp32 mode at a raised level"; return SCFGP_EARG; }
        src = c->d_Phi64; bytes = 8 * g.Np * g.Kp;
    }
    else if (s == "Tt") {                                        // T~ = [X l_F | 1] of the rank-S projection, Np x Sp
        if (!c->d_Tt) { c->err = "debug_read: Tt exists only where the projection goes through the S columns"; return SCFGP_EARG; }
        src = c->d_Tt; bytes = 8 * g.Np * g.Sp;
    }
    else if (s == "Phi16" || s == "V16g" || s == "qV16g" || s == "B16" || s == "f16scale" || s == "f16tmp") {
        if (!c->split16) { c->err = "debug_read: " + s + " exists in compute mode SCFGP_F16X3 only"; return SCFGP_EARG; }
        const int64_t plane = 4 * g.Np * g.Kp;                  // the F16_PAD bytes behind the Np x Kp arrays are left out
        if (s == "Phi16") { src = c->d_Phi16; bytes = plane; }
        else if (s == "V16g") { src = c->d_V16g; bytes = plane; }
        else if (s == "qV16g") { src = c->d_qV16g; bytes = plane; }
        else if (s == "B16") { src = c->d_B16; bytes = 4 * K2; }
        else if (s == "f16scale") { src = c->d_f16scale; bytes = sizeof(float) * 4; }
        else { src = c->d_f16tmp; bytes = sizeof(float) * 8; }
    }
    else { c->err = "debug_read: unknown buffer " + s; return SCFGP_EARG; }
    if (!src) return SCFGP_EARG;
    if (bytes > max_bytes) bytes = max_bytes;
    if (hipStreamSynchronize(c->st) != hipSuccess) return SCFGP_EHIP;
    if (hipMemcpy(host, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) return SCFGP_EHIP;
    return bytes;
}
