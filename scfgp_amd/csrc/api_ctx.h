// Internal to csrc/: what every source file of the C ABI needs -- the context, HIPCHK, the profiling scopes and the device allocation
// helpers.  scfgp_api.hip holds the evaluation side; the posterior and pool entry points (api_predict.hip, api_update.hip,
// api_pool.hip) add the chunk pipeline of api_chunks.h.
#pragma once
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
inline Roctx& roctx() { static Roctx r; return r; }         // inline, not static: one Roctx and one dlopen for all source files

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
    // (u_flag: [0] Cholesky flag, [1] non-finite input, [2] non-finite output of the K x K stage, [8..15] queue heads)
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

// fn of the class template I at the context's type.  Every source file has a wrapper template of its own name and a one-line DISPATCH on
// it: static members of a class template are weak symbols, and two templates of one name in two files would be merged by the linker
#define DISPATCH_TO(I, c, fn, ...) ((c)->dtype == SCFGP_F32 ? I<float>::fn(__VA_ARGS__) : I<double>::fn(__VA_ARGS__))
