// Host-callable launchers for every device kernel of the scfgp HIP library.
// All launch asynchronously on `st`; none allocates or synchronises.
#pragma once
#include "common.h"

// geometry shared by all sweeps (device buffers are padded so kernels need no edge code)
struct Geom {
    int D, S, M, J, K, P;
    int Dp;      // round_up(D+1,16): X~ = [X | 1 | 0..]   (ones column carries the phase offsets)
    int Jp;      // round_up(J,128)
    int Sp;      // round_up(S+1,16): T~ = [X l_F | 1 | 0..] (N x Sp), the rank-S form of the projection
    int lowrank; // 1: Z = (X~ Lall) Rall = T~ Rall (chosen when Sp < Dp); 0: Z = X~ Fall
    int Kp;      // round_up(K,tile): leading dimension of Phi and of every K x K matrix
    int tile;    // 128: square tile of the Gram products and of the packed exchange layout
    int gfull;   // Gram tile grid: gfull rows of square tiles ...
    int gstrip;  // ... plus, for an odd number of 64-column blocks in K, one 64-high strip below them
    int64_t N;   // valid local rows
    int64_t Np;  // round_up(N,256)
};

// Row splits of the Gram products.  A job is (row split, output tile); the launch runs the jobs split-major and the
// XCD map hands each of the 8 XCD groups a contiguous run of splits, so the workgroups that are resident together
// work on the same rows (their re-reads of Phi are served by the Infinity Cache / L2 instead of HBM) while faster CUs
// simply take more jobs.  A launch ends when the last jobs of every group finish: with equal splits those are full-size
// jobs (5.2 ms of a 38.6 ms launch, 3.7 ms of it with part of the chip idle: profiles/r02_tuning.md), so the LAST
// unit of every group is cut into splits of 1/2, 1/4, 1/8, 1/8 of a unit (`taper`): the tail shrinks eightfold for
// three more slabs per group.
struct RowSplits {
    int nsplit;          // all splits
    int groups;          // 8 (one run of splits per XCD group) or 1
    int units;           // equal-size units per group; taper: the last unit is cut into taper + 1 splits
    int taper;           // 0, or t: the last unit of every group is cut into 1/2, 1/4, .., 1/2^t, 1/2^t
    int gran;            // row granule of the split boundaries: 256, or 64 for problems too small to fill the chip otherwise
    int64_t nrb;         // granules: Np / gran
    __host__ __device__ int per_group() const { return units + taper; }
    // rows [r0, r1) of split s (multiples of gran; may be empty)
    __host__ __device__ void range(int s, int64_t& r0, int64_t& r1) const {
        const int pg = per_group(), grp = s / pg, i = s % pg;
        const int64_t g0 = nrb * grp / groups, g1 = nrb * (grp + 1) / groups, len = g1 - g0;
        const int64_t den = (int64_t)1 << taper;                    // position in 2^-taper of a unit
        const int k = i - (units - 1);                              // 0..taper inside the last unit
        int64_t e0, e1;
        if (taper == 0 || k < 0) { e0 = den * i; e1 = e0 + den; }
        else {
            const int64_t base = den * (units - 1);
            e0 = base + den - (den >> k);                           // 0, 1/2, 3/4, ...
            e1 = k == taper ? base + den : base + den - (den >> (k + 1));
        }
        r0 = (g0 + len * e0 / (den * units)) * gran;
        r1 = (g0 + len * e1 / (den * units)) * gran;
    }
};
RowSplits gram_row_splits(int jobs_per_split, int64_t Np, bool f32, int nsplit_override, int taper);

// operands of the phase projection: Fall (Dp x Jp); Lall (Dp x round_up(Sp,64)) = [l_F | e_D], Rall (Sp x Jp) =
// [[I_S | r_F^T]; phase offsets], Tt (Np x Sp) scratch for T~
struct Projection { const double* Fall; const double* Lall; const double* Rall; double* Tt; };

// ---- fmap.hip: feature map and operand staging ---------------------------------------------------------------------
template <typename T>
struct FmapKernels {
    // Phi = s*[cos Z, sin Z], Z = X~ . Fall  or, F = l_F r_F^T being rank S (SCFGP.py:83), Z = (X~ . Lall) . Rall
    //                                                            (SCFGP.py:98-102 / :139-142)
    static void featuremap(const Geom& g, const double* Xt, const Projection& pr, const Scal* sc, T* Phi, hipStream_t st);
    // fp64 Kp x Kp matrix -> sweep operand (type T, rows/cols >= K zeroed)
    static void convert(const double* src, T* dst, int K, int Kp, hipStream_t st);
    static void convert_transposed(const double* src, T* dst, int K, int Kp, hipStream_t st);      // dst = src^T on the K x K block
};

// ---- gram.hip: TN products (contraction over the rows) ---------------------------------------------------------------
template <typename T>
struct GramKernels {
    // lower tiles of  Phi^T diag(w) Phi  into per-split fp64 slabs (SCFGP.py:104; weighted: backward of :111-113)
    // and, from the diagonal tiles, sidepart[split][Kp] = partials of Phi^T side (side = y: SCFGP.py:108)
    //   qhead: 8 ints of device scratch (the heads of the per-XCD job queues of the persistent launch)
    //   ws2:   2 (Np + 32) floats of device scratch (fp32 mode: the packed row weights / side multipliers of the LDS-DMA tiles;
    //          the 64 floats behind the last row are read, never used); unused in fp64 mode
    static void gram(const Geom& g, const T* Phi, const double* w, const double* side, const RowSplits& rs, int64_t chunk,
                     double* slabs, double* sidepart, int* qhead, float* ws2, hipStream_t st);
    static int gram_jobs(const Geom& g);        // workgroups per row split of gram() (sizes the row split)
    // X~^T Zbar into per-split fp64 slabs, Zbar[n][j] = Phi[n][j] Phibar[n][J+j] - Phi[n][J+j] Phibar[n][j]
    // formed inside the operand loader
    static void xtz(const Geom& g, const double* Xt, const T* Phi, const T* Phibar, int nsplit, int64_t chunk, double* slabs,
                    hipStream_t st);
    // ---- rank-S form of the backward projection (F = l_F r_F^T, SCFGP.py:83,100: the reverse sweep needs only
    //      T~^T Zbar (S+1 x J) and X~^T (Zbar_L + Zbar_M r_F) (D+1 x S) instead of X~^T Zbar (D+1 x J)) -------------
    // Zbar over the cosine half of Phibar, in place
    static void zbar_inplace(const Geom& g, const T* Phi, T* Phibar, hipStream_t st);
    // Rsel = [I_S ; r_F] as a typed Kp x Kp-strided operand (round_up(S,64) columns written)
    static void rsel(const Geom& g, const double* params, T* out, hipStream_t st);
    // A^T Bm over the rows into per-split slabs: A (Np x Dp fp64), Bm (Np x J live columns, leading dimension ldb)
    static void tn_plain(const double* A, int Dp, const T* Bm, int64_t ldb, int J, int64_t Np, int nsplit, int64_t chunk, double* slabs,
                         hipStream_t st);
};

// operands of one apply product in compute mode SCFGP_F16X3 (apply_f16.hip): Phi and the K x K operand in plane form (below), scale[0] =
// 2^-(e_Phi + e_operand) on the device.  V16 (may be NULL): V = Phi B's epilogue also writes V in plane form, scaled by 2^e with
// e = 14 - ilogb(vbound[0]) -- the array split_v would otherwise write
struct F16Operands { const unsigned* Phi16; const char* B16; const float* scale; unsigned* V16; const float* vbound; };

// ---- apply.hip: NT products (contraction over the feature columns) and the per-row statistics ------------------------
//   dma: 0 = operands staged through registers; 1 / 2 = the full 128-column tiles by LDS-DMA, 128 / 256 wide (256: fp32 only)
template <typename T>
struct ApplyKernels {
    // V = Phi . Bm, vpart[jt][n] = sum_{j in tile} Phi[n][j] V[n][j]    (SCFGP.py:112); column tile jt also forms
    // mupart[jt][n] = its slice of mu = Phi . alpha (SCFGP.py:111 / :143) from the rows it stages
    //   f16 (fp32 mode only, dma == 2): the 256-wide tiles by the three-term fp16 split instead (apply_f16.hip); the narrower tiles of
    //   the launch plan stay exact fp32
    static void apply_v(const Geom& g, const T* Phi, const T* Bm, T* V, double* vpart, const double* alpha, double* mupart,
                        hipStream_t st, int dma = 0, const F16Operands* f16 = nullptr);
    // predict: vpart[jt][n] = slices of v_n = || Li phi_n ||^2 (the reference's rowsum((Phi Li^T)^2), SCFGP.py:144) from the
    // triangular product Phi . LiT, LiT[k][j] = Li[j][k] (convert_transposed); mupart as apply_v.  Half the flops of apply_v.
    static void apply_predict(const Geom& g, const T* Phi, const T* LiT, double* vpart, const double* alpha, double* mupart,
                              hipStream_t st);
    // Factor form of pass 2 (the reference's own products, SCFGP/SCFGP.py:112: v = rowsum((Phi Li^T)^2)): C = Phi . LiT
    // (triangular: half the flops), vpart = slices of rowsum(C^2), mupart = slices of mu = Phi . alpha = C . beta (SCFGP.py:109-111:
    // alpha = Li^T beta, beta = Li Phi^T y; the LDS-DMA tiles use the second form); then V = C . Li = Phi B (triangular).
    // Li / LiT: the typed K x K copies of L^-1 and its transpose (padding zeroed).  Rounding errors of C are amplified by
    // cond(L) = sqrt(cond(A)) where those of V = Phi . B computed directly are amplified by cond(A)
    // (profiles/r03_c3_owner.md).
    static void apply_c(const Geom& g, const T* Phi, const T* LiT, const T* Li, T* C, double* vpart, const double* alpha,
                        const double* beta, double* mupart, hipStream_t st, int dma = 0);
    static void apply_vc(const Geom& g, const T* C, const T* Li, const T* LiT, T* V, hipStream_t st, int dma = 0);
    // Phibar = 2 Phi.Abar + 2 q V + p alpha^T + y ut^T  (in place over V)
    static void apply_phibar(const Geom& g, const T* Phi, const T* Abar, T* V, const double* p, const double* q,
                             const double* y, const double* alpha, const double* ut, hipStream_t st, int dma = 0, const F16Operands* f16 = nullptr);
    // Out = A . Bm over k < Kc for ncols columns (64-wide tiles, leading dimension Kp everywhere; Bm[k][c] = 0 for k < c)
    static void apply_plain(const Geom& g, const T* A, const T* Bm, T* Out, int Kc, int ncols, hipStream_t st);
    // per-row moments and adjoint scalars; block partials (4 per block) of T2, kbar, sum q v, sum p mu  (SCFGP.py:111-113,121-124)
    static void rowstats(const Geom& g, const double* mupart, const double* vpart, const double* y,
                         const Scal* sc, double* p, double* q, double* partial, int nblocks, hipStream_t st);
    // predictive mean / std                                          (SCFGP.py:143-144)
    static void rowpredict(const Geom& g, const double* mupart, const double* vpart, const Scal* sc, double* mu, double* sd,
                           hipStream_t st);
    // residual of new rows under the old mean (scfgp_condition): r[n] = y[n] - sum_jt mupart[jt][n] for n < N, 0 on the padding rows
    static void rowresidual(const Geom& g, const double* mupart, const double* y, double* r, hipStream_t st);
    // slices per row of vpart / mupart: the column tiles of the launch plan (depends on K alone)
    static int partials(const Geom& g);
};

// ---- apply_f16.hip, gram_f16.hip: compute mode SCFGP_F16X3 -- the big products as a three-term fp16 split (a labelled secondary mode) ----
// "Plane form": 4 bytes per element, per 16 consecutive columns the 16 h's and then the 16 l's ([16 x h | 16 x l], 64 bytes).  Operands of
// one apply product: Phi in plane form (Np x Kp), the K x K operand in plane form (row = output column), scale[0] = 2^-(e_Phi + e_operand)
// on the device
struct F16x3Kernels {
    // M: fp64, symmetric, K x K inside Kp x Kp; part: >= 512 doubles of scratch
    static void split_operand(const Geom& g, const double* M, char* B16, float* scale, double* part, const Scal* sc, hipStream_t st);
    // column tiles [col0, col0 + BN njt) (BN = 256, 128 or 64; vpart slots from slot0) of row blocks rb0 .. rb0 + nrb - 1, epilogue EPI 0
    // (V, row dots) or 1 (Phibar); returns the tile count
    template <int EPI, int BN>
    static int apply(const Geom& g, int njt, int col0, int slot0, const float* Phi, const F16Operands& f, float* V,
                     double* vpart, const double* p, const double* q, const double* y, const double* alpha, const double* ut, double* mu,
                     hipStream_t st, int64_t rb0, int64_t nrb);
    // apply.hip: whether the apply products run these tiles at all -- the launch plan has full 128-column blocks (K > 256); below
    // that fp32 mode's register tiles do, and V = Phi B's epilogue writes no planes
    static bool apply_runs(const Geom& g);
    // gram_f16.hip.  The Np x Kp plane-form arrays are allocated with F16_PAD bytes behind them (the Gram's last 256-column block may
    // stick out of Kp).  tmp: 8 floats on the device; after a split pass tmp + 4 is the scale of the Gram product that follows.
    // sidepart: side_blocks(g) x Kp doubles, the block partials of M^T w (reduce_side sums them).
    static constexpr size_t F16_PAD = 1024;
    static int side_blocks(const Geom& g);
    // Phi -> plane form (Phi16: the operand of the apply tiles and of pass 1's Gram); sidepart <- Phi^T y
    static void split_phi(const Geom& g, const float* Phi, const double* y, const Scal* sc, unsigned* Phi16, double* sidepart, float* tmp,
                          hipStream_t st);
    // tmp[5] <- a bound of |V| = |Phi B| from B alone (fp64, symmetric, ld Kp): before the product, whose epilogue writes V's planes with it
    static void v_bound(const Geom& g, const double* B, const Scal* sc, float* tmp, hipStream_t st);
    // V = Phi B -> plane form of diag(q) V (and of V itself unless V16g is NULL: the product's epilogue wrote it); sidepart <- V^T p
    static void split_v(const Geom& g, const float* V, const double* q, const double* p, unsigned* V16g, unsigned* qV16g, double* sidepart,
                        float* tmp, hipStream_t st);
    // slabs[chunk][tri(128-tile)][128 x 128] = scale[0] (A chunk)^T (B chunk) on the lower 128-tiles, every slab written; chunk rows per
    // chunk (rounded up to 256): gram_chunks(g, chunk) chunks, to be summed by reduce_tri_tiles with nsplit = that number
    static int gram_chunks(const Geom& g, int64_t chunk);
    static int gram_tiles(const Geom& g);                       // 256 x 128 tiles of one chunk
    static void gram(const Geom& g, const unsigned* A16g, const unsigned* B16g, const float* scale, int64_t chunk, double* slabs, hipStream_t st);
};

// everything that sweeps the rows, under one name
template <typename T> struct SweepKernels : FmapKernels<T>, GramKernels<T>, ApplyKernels<T> {};

// diagnostic builds only (-DSCFGP_TRACE): per-workgroup [start, end, xcc, kind] of the last Gram launch; -1 otherwise
int64_t trace_read(void* host, int64_t max_bytes);
int64_t apply_trace_read(void* host, int64_t max_bytes);    // per workgroup of the last LDS-DMA apply launch: [start, end, xcc]
int64_t chol_trace_read(void* host, int64_t max_bytes);     // per Cholesky step: 12 phase stamps of workgroup 0

// ---- reductions ------------------------------------------------------------
// packed lower tiles = sum over splits of the per-split lower-tile slabs (tile t = ti(ti+1)/2+tj, row-major)
void reduce_tri_tiles(const double* slabs, int nsplit, int nts, int tile, double* packed, hipStream_t st);
// packed lower tiles -> full symmetric Kp x Kp matrix
void unpack_tri_tiles(const double* packed, int nts, int tile, double* full, int64_t ld, hipStream_t st);
// out (ldo) = sum over splits of a full ntm x ntn tile grid of slabs
void reduce_full_tiles(const double* slabs, int nsplit, int ntm, int ntn, double* out, int64_t ldo, hipStream_t st);
// vec[j < ncov] = sum over splits of sidepart[split][j] (ld Kp), vec[ncov..Kp) = 0
void reduce_side(const double* sidepart, int nsplit, int Kp, int ncov, double* vec, hipStream_t st);
// scalars[slot0 + k] = sum_b partial[b*width + k], k < width (the partials are scratch: a large single-scalar sum is staged in place)
void reduce_scalars(double* partial, int nblocks, int width, double* scalars, int slot0, hipStream_t st);
// scalars[slot] = sum y^2
void sum_squares(const double* y, int64_t n, double* scalars, int slot, double* scratch, hipStream_t st);

// ---- parameter unpack / gradient epilogue -----------------------------------
void unpack_params(const Geom& g, const double* params, double* F, double* Fall, double* Lall, double* Rall, Scal* sc, hipStream_t st);
//   rank-S form (TZ != NULL): XZ is not used; TZ (ld ldtz) rows s < S hold l_F^T X^T Zbar and row S the column sums of Zbar,
//   XU (ld ldxu) holds X~^T (Zbar_L + Zbar_M r_F)
void grad_epilogue(const Geom& g, const double* params, const double* F, const double* XZ, int64_t ldxz,
                   double* work, double* scalars, int64_t Nglobal, double* grad, hipStream_t st,
                   const double* TZ = nullptr, int64_t ldtz = 0, const double* XU = nullptr, int64_t ldxu = 0);
// yy -> y^T y, t2kb -> (T2, kbar, sum q v, sum p mu): device scalars living in the exchange buffers (summed over ranks)
void finalize_cost(const Geom& g, const Scal* sc, double* scalars, const double* yy, const double* t2kb,
                   int64_t Nglobal, double* grad, int want_grad, hipStream_t st);
// xs[XS_RAN1 .. XS_FAIL] = the four status slots of an exchange buffer's scalar tail (common.h)
void write_status(double* xs, double ran1, double cap1, double cap2, double fail, hipStream_t st);
// Xt (Np x Dp) = [X[idx] | 1 | 0], zero rows >= N; y padded with zeros; idx == NULL: rows in order
// mode/sp: optional per-column input scaling (SCFGP/Scaler.py forward_transform) applied on the fly
void pack_data(const Geom& g, const double* Xraw, const double* yraw, const int64_t* idx, double* Xt, double* y, hipStream_t st,
               int mode = 0, const double* sp = nullptr);
// square K x K host-layout matrix (ld K) -> Kp x Kp with identity padding, and back
void pad_square(const double* src, int K, int Kp, double* dst, hipStream_t st);

// ---- prediction post-processing (SCFGP/SCFGP.py:281-293, SCFGP/Scaler.py:118-135) -------------
constexpr int YPOST_BLOCKS = 64;
// out[0] = mean(ys)
void ypost_mean(const double* ys, int64_t n, double* out, hipStream_t st);
// mu, sd (n) <- y-scaler backward transform of the mean and half the transformed +-1 std band, in place;
// ys != NULL: part[YPOST_BLOCKS][4] = block partials of the metric sums of this chunk
void ypost_chunk(double* mu, double* sd, const double* ys, int64_t n, int mode, const double* sp, const double* ymean,
                 double* part, hipStream_t st);
// out[6] = MAE, NMAE, MSE, NMSE, MNLP, SCORE from nparts x 4 partial sums over n targets
void ypost_metrics(const double* part, int nparts, int64_t n, double* out, hipStream_t st);

// ---- predgrad.hip, gradients of predict in its inputs (scfgp_predict_grad) ---------------------------------------------
// columns of the typed operand FT = Fall^T (rows d >= D zero): a multiple of 16 that the launches' column tiles cover
int predgrad_ft_cols(int D);
// FT (round_up(J,16) x predgrad_ft_cols(D), type T) from Fall; rows j >= J and columns d >= D zero
template <typename T> void predgrad_operand(const Geom& g, const double* Fall, T* FT, hipStream_t st);
// dmu[n][d] = sum_j Fall[d][j] (phi_c alpha_s - phi_s alpha_c)_nj and, dstd != NULL, dstd[n][d] = kappa / sd_n sum_j Fall[d][j]
// (phi_c V_s - phi_s V_c)_nj, V = Phi B; n < N, d < D (ld D)
template <typename T>
void predgrad(const Geom& g, const T* Phi, const T* V, const double* alpha, const T* FT, const double* sd, const Scal* sc, double* dmu,
              double* dstd, hipStream_t st);
// chain rules of the scalers, in place on n x D gradients (dstd may be NULL): xgrad_chunk multiplies column d by the derivative of
// the packing transform at the raw input Xraw[n][d] (modes of pack_data); ygrad_chunk turns d mu, d std into those of mu_y = bw(mu) and
// std_y = (bw(mu + std) - bw(mu - std)) / 2 (mu, sd: the scaled predictions of the same rows, before ypost_chunk)
void xgrad_chunk(const double* Xraw, int64_t n, int D, int mode, const double* sp, double* dmu, double* dstd, hipStream_t st);
void ygrad_chunk(const double* mu, const double* sd, int64_t n, int D, int mode, const double* sp, double* dmu, double* dstd, hipStream_t st);

// ---- sample.hip, posterior sample functions (scfgp_sample, scfgp_sample_weights) -----------------------------------------------------
// the weight arrays are sample_w_rows(K) x sample_w_cols(nsamp), zero outside K x nsamp
inline int64_t sample_w_rows(int K) { return round_up(K, 64); }
inline int sample_w_cols(int nsamp) { return (int)round_up(nsamp, 64); }
// Z (scratch) <- the normals of `seed`; W (fp64) and Wt (type T) <- alpha 1^T + sqrt(kappa) Li^T Z (Li: K x K device copy of the host
// matrix, lower triangular; alpha: K)
template <typename T>
void sample_weights(const Geom& g, const double* Li, const double* alpha, const Scal* sc, int nsamp, uint64_t seed, double* Z, double* W,
                    T* Wt, hipStream_t st);
// out (N x nsamp, row-major) = Phi Wt over the K features of the chunk's rows; noise: + sqrt(kappa) eps of rows t0 + n; ymode >= 0: then
// the y scaler's backward transform of that mode (sp: its 5 parameters)
template <typename T>
void sample_product(const Geom& g, const T* Phi, const T* Wt, int nsamp, int64_t t0, uint64_t seed, int noise, int ymode, const double* ysp,
                    const Scal* sc, double* out, hipStream_t st);
// scfgp_sample_argmax: the product's workgroups cover sample_block_rows rows each and leave one record per sample column
constexpr int sample_block_rows(size_t tsize) { return tsize == 4 ? 128 : 64; }
inline int64_t sample_blocks(int64_t Np, size_t tsize) { return Np / sample_block_rows(tsize); }
// pv, pt: the records of one chunk's workgroups (sample_blocks x nsamp: value, chunk-local row or -1 for none); bestv, bestt (nsamp): the
// running best over the chunks so far (value, row index in the call's Xs); flag: set where an eligible row's value is not finite
struct SampleArgmaxBufs { double* pv; long long* pt; double* bestv; long long* bestt; int* flag; };
// Phi Wt as sample_product forms it, reduced per sample column in the product's epilogue: over the rows n < N with w[n] > 0 (w == NULL:
// all; w: Np entries) the largest value (minimize: the smallest), ties to the lowest row; then the chunk's records are merged into
// bestv / bestt with rows counted from t0 (`first`: the running best starts empty)
template <typename T>
void sample_argmax_product(const Geom& g, const T* Phi, const T* Wt, int nsamp, const double* w, int minimize, int64_t t0, int first,
                           const SampleArgmaxBufs& b, hipStream_t st);
// bestv (nsamp) <- the y scaler's backward transform of mode ymode, by the kernel sample_product applies it with
void sample_argmax_finalize(double* bestv, int nsamp, int ymode, const double* ysp, const Scal* sc, hipStream_t st);

// ---- acquire.hip, acquisition functions over a pool (scfgp_acquire) ------------------------------------------------------------------------
// the call's scalars: kind 0 UCB (par = [beta]), 1 PI, 2 EI, 3 LOGEI (par = [best, xi]), 4 MES (fstar: nstar sampled maxima on the device)
struct AcquireSpec { int kind; double par[2]; const double* fstar; int nstar; int noise; int minimize; };
// workgroup records of the argmax over a chunk of Np rows
inline int64_t acquire_blocks(int64_t Np) { return Np / 256; }
// mu, sd, acq: the chunk's rows of the call's T-sized arrays; au, as (Np): the partials d acq / d u, d acq / d sigma of the chunk's rows;
// pv, pt: the records of the chunk's workgroups (value, chunk-local row or -1); bestv, bestt (1 each): the running best over the chunks so
// far; flag: set where an eligible row has a non-finite mu, sigma or value, or sigma = 0
struct AcquireBufs { double* mu; double* sd; double* acq; double* au; double* as; double* pv; long long* pt; double* bestv; long long* bestt; int* flag; };
// rows n < N from the chunk's partials (njt slices each, summed in rowpredict's order): mu, sd = sqrt(kappa v) or (noise) sqrt(kappa (1 + v)),
// the acquisition value and its partials
void acquire_rows(const Geom& g, int njt, const double* mupart, const double* vpart, const Scal* sc, const AcquireSpec& a, const AcquireBufs& b,
                  hipStream_t st);
// the chunk's best eligible row (w == NULL: all; else w[n] > 0; w: Np entries) merged into bestv / bestt with rows counted from t0
// (`first`: the running best starts empty); the largest value wins, ties go to the lowest row
void acquire_argmax(const Geom& g, const double* w, int64_t t0, int first, const AcquireBufs& b, hipStream_t st);
// grad (N x D, holding d mu / d x) <- sgn au grad + as dsd
void acquire_grad(const Geom& g, const AcquireBufs& b, int minimize, const double* dsd, double* grad, hipStream_t st);

// ---- kg.hip, knowledge gradient over a pool (scfgp_acquire_kg) ------------------------------------------------------------------------------
// d (round_up(R, 128)): d_r = u_r - max u of the reference rows; zf (64): the nodes and h(-|z_j|); sd (Np): sigma of the chunk's candidates;
// st_m, st_s (kg_state_rows() x J), st_b (kg_state_rows() x 2): the node states per row and column split; kg, kg_hi: the chunk's rows of
// the call's T-sized arrays; m, s: its rows of the T x J node tables, or NULL
struct KgBufs { double *d, *zf, *sd, *st_m, *st_s, *st_b, *kg, *kg_hi, *m, *s; };
int64_t kg_state_rows();
// after apply_predict on the R reference rows (njt partials per row, leading dimension Np): d, zf; flag[1] = 1 where a u_r is not finite
void kg_reference(int njt, const double* mupart, int64_t Np, int64_t R, int minimize, const double* z, int J, double* d, double* zf, int* flag,
                  hipStream_t st);
// sd[n < Np] = sqrt(kappa v) or (noise) sqrt(kappa (1 + v)) from the chunk's partials, by acquire_rows' arithmetic
void kg_sigma(const Geom& g, int njt, const double* vpart, const Scal* sc, int noise, double* sd, hipStream_t st);
// Ca (the chunk's g.N candidates), Cb (R reference rows): C = Phi Li^T as apply_c leaves it, as predcov takes them.  The node table of
// every candidate without the g.N x R matrix, then kg, kg_hi (and m, s) of the chunk's rows
template <typename T>
void kg_nodes(const Geom& g, const T* Ca, const T* Cb, int64_t R, int J, const KgBufs& b, const Scal* sc, hipStream_t st);

// ---- samplegrad.hip, values and input gradients of sample functions, one sample per row (scfgp_sample_grad) ----------------------------
// leading dimension of WT: a weight row is contiguous, 16-byte aligned and zero past K
int samplegrad_w_ld(int K);
// WT (nsamp x samplegrad_w_ld(K), fp64) <- the transpose of W (K x nsamp row-major: a device copy of the host array)
void samplegrad_weights(const double* W, int K, int nsamp, double* WT, hipStream_t st);
// chunk row n < N under sample s = sidx[n] (sidx: Np doubles holding integers in [0, nsamp); NULL: s = (t0 + n) % nsamp):
// val[n] = sum_j phi_c_nj w_s[j] + phi_s_nj w_s[J + j] (fp64) and grad[n][d] = sum_j Fall[d][j] (phi_c w_s[J + j] - phi_s w_s[j])_nj,
// d < D (ld D), by predgrad's arithmetic and launch plan; FT as predgrad_operand leaves it
template <typename T>
void samplegrad(const Geom& g, const T* Phi, const double* WT, const double* sidx, int64_t t0, int nsamp, const T* FT, double* val,
                double* grad, hipStream_t st);

// ---- predcov.hip, joint posterior covariance between test points (scfgp_predict_cov) ---------------------------------------------------
// out[n][j] (n < nrows, j < Tb; row-major, leading dimension Tb, fp64) = kappa sum_k Ca[n][k] Cb[j][k] over the K features, + kappa
// where row_base + n == j with `noise`.  Ca, Cb: C = Phi Li^T as apply_c leaves it (leading dimension Kp, columns K.. zero), with
// round_up(nrows, 128) and round_up(Tb, 128) readable rows.
template <typename T>
void predcov(const Geom& g, const T* Ca, const T* Cb, int64_t nrows, int64_t Tb, int64_t row_base, int noise, const Scal* sc, double* out,
             hipStream_t st);

// ---- on-device update rules (SCFGP/Optimizer.py) --------------------------------------------
struct OptHyper { double lr, b1, b2, eps, momentum; };   // b1 doubles as rho for rmsprop/adadelta; momentum < 0: no Nesterov
// theta <- rule(theta, grad); st = [s1 | s2 | velocity]; tctr[0] = step counter, tctr[1] = index into hist
void opt_update(int algo, const OptHyper& h, int P, double* theta, const double* grad, double* st, double* tctr,
                const double* scalars, double* hist, int hist_cap, hipStream_t stream);

// ---- K x K stage (fp64, all matrices Kp x Kp, leading dimension Kp) -----------
struct KStage {
    int K, Kp;
    double *A;      // in: G + lam I (full, symmetric); working matrix of the factorisation (the factor L goes to T2)
    double *Li;     // L^{-1} (lower, zero above)
    double *B;      // Li^T Li
    double *T1, *T2;// scratch Kp x Kp
    double *g, *beta, *alpha, *h, *u, *ut;   // Kp vectors
    double *scalars; int* flag;
};
// SCFGP.py:105-110,125; packed: the summed packed lower 128 x 128 tiles of G (exchange buffer 1); the upper blocks of Li stay as
// they are (zero from context creation: nothing ever writes them)
void kstage_factor(const KStage& k, const double* packed, const Scal* sc, hipStream_t st);
void kstage_adjoint(const KStage& k, const double* BWB, double* Abar, const Scal* sc, hipStream_t st);
void kstage_adjoint_factor_form(const KStage& k, double* McBWB, double* Abar, const Scal* sc, hipStream_t st);
// scalars[R_TRAG] = tr(Abar G), scalars[R_UTG] = ut^T Phi^T y from the summed packed G of exchange buffer 1 (after the adjoint)
void kstage_bbar(const KStage& k, const double* packed, const double* Abar, double* part, hipStream_t st);

// ---- posterior update (scfgp_condition): S = I + C^T C = M M^T, Li' = M^-1 Li, alpha' = alpha + Li^T S^-1 C^T r -----------------
// All matrices Kp x Kp fp64 with identity padding; none of them is a buffer of KStage.
struct KUpdate {
    int K, Kp;
    const double* packed;   // in: packed lower 128 x 128 tiles of C^T C, then C^T r (Kp) at packed + n_pk
    int64_t n_pk;
    const double* Li;       // in: the old factor (lower triangular, zeros above the diagonal: update_load_factor)
    const double* alpha;    // in: the old weights (Kp, padding zero)
    double *S;              // working matrix of the factorisation; on return Li' (lower triangular, zeros above the diagonal)
    double *Lm, *Mi, *Si;   // M (diagonal blocks), M^-1 (its blocks above the diagonal must be zero on entry and stay so), S^-1
    double *gamma, *alpha_out, *part;   // Kp, Kp, 32 Kp
    int* flag;              // flag[0] = 1: S not positive definite (or NaN)
};
void kstage_update(const KUpdate& k, hipStream_t st);
// scfgp_forget: the same stage with S = I - C^T C and alpha' = alpha - Li^T gamma (flag[0] = 1: the rows were not in the fit), then
// out[0] = log p(y_o | the other rows) from rr[0] = r^T r, |M^-1 C^T r|^2 and M's diagonal, out[1] = min_i M_ii^2.  k.part holds
// M^-1 C^T r on return.
void kstage_downdate(const KUpdate& k, const double* rr, double n, const Scal* sc, double* out, hipStream_t st);
// acc[0] += sum of r[0..n)^2 (one workgroup, fixed order)
void update_sumsq(const double* r, int64_t n, double* acc, hipStream_t st);
// acc[0..2] += sum e^2, sum |e|, sum log N(y_i; mu_i, sd_i^2) of n rows, e = y - mu: terms from the rounded mu / sd into rec (3 x ldr),
// added in row order by one lane per sum
void forget_stats(const double* mu, const double* sd, const double* y, int64_t n, int64_t ldr, double* rec, double* acc, hipStream_t st);
// host-layout K x K factor on the device (ld K, entries above the diagonal not read) <-> Kp x Kp lower triangular, identity padding
void update_load_factor(const double* Li_host_layout, int K, int Kp, double* Li, hipStream_t st);
void update_store_factor(const double* Li, int K, int Kp, double* Li_host_layout, hipStream_t st);
// flag[1] = 1 if any of x[0..n) is NaN or Inf;  acc[0..n) += part[0..n)
void update_check_finite(const double* x, int64_t n, int* flag, hipStream_t st);
void update_accumulate(double* acc, const double* part, int64_t n, hipStream_t st);

// ---- loo.hip: exact leave-block-out predictions of rows that are in the fit (scfgp_loo) ------------------------------------------
// C (typed, ld Kp) = Phi_I Li^T, r = y - Phi_I alpha and y of the chunk's g.N rows, whose first block has the call-wide index blk0:
// mu, sd, lev (may be NULL) of every row, one record of 5 doubles per block into rec, then the records added in block order into acc
// ([0..3] sums, [4] max h).  bad[0] != 0: a non-finite h, r or y; bad[1]: the smallest block index whose I - H has no Cholesky factor.
template <typename T>
void loo_blocks(const Geom& g, const T* C, const double* r, const double* y, int block, int64_t blk0, const Scal* sc, double* mu,
                double* sd, double* lev, double* rec, double* acc, unsigned long long* bad, hipStream_t st);

// ---- gradcov.hip: posterior covariance of the input gradient (scfgp_predict_gradcov) --------------------------------------------------
// q = min(D, S) directions per point; a chunk of g.N points has gr.N = g.N q derivative rows (gr: the chunk's geometry in those rows).
// Qt (q x Jp, type T): row i = Q[:, i] of the direction basis (dense D <= S: row i of Fall; latent D > S: [e_i | r_F[:, i]^T])
template <typename T> void gradcov_operand(const Geom& g, const double* params, const double* Fall, T* Qt, hipStream_t st);
// Psi (gr.Np x Kp): row t q + i = (-Phi_s[t] o Q[:, i] | Phi_c[t] o Q[:, i]), formed in fp64 and rounded once; padding columns and rows zero
template <typename T> void gradfeat(const Geom& gr, const Geom& g, const T* Phi, const T* Qt, T* Psi, hipStream_t st);
void gradcov_ones(double* x, int64_t n, hipStream_t st);
// C (typed, ld Kp) = Psi Li^T.  Per point t < g.N: Sigma_t = kappa P H_t P^T (H_t = C_t C_t^T; P = l_F read from params, or I), scaled
// on both sides by gfac[t] (g.N x D; NULL: none).  dvar (g.N x D), dcov (g.N x D x D), rec (g.N x D x D, lower triangle only:
// wgt[t] (m[t] m[t]^T + Sigma_t); wgt NULL: 1) may each be NULL
template <typename T>
void gradcov_blocks(const Geom& gr, const Geom& g, const T* C, const double* params, const Scal* sc, const double* gfac, const double* m,
                    const double* wgt, double* dvar, double* dcov, double* rec, hipStream_t st);
// acc (D x D, lower triangle) += rec[0..n) in point order, one lane per entry
void gradcov_reduce(const double* rec, int64_t n, int D, double* acc, hipStream_t st);

// ---- condgrad.hip: derivative observations as rows of the posterior update (scfgp_condition_grad) ------------------------------------
// what a chunk of g.N points observes: dims (nd device ints, NULL: 0..nd-1), gfac (g.N x D: the X scaler's derivative factors, NULL: 1), y
// (g.N values, NULL: none), G (g.N x nd derivatives), rho (g.N x nd precisions relative to the value noise, NULL: 1)
struct GradObs { const int* dims; int nd; const double *gfac, *y, *G, *rho; };
// Psi (gr.Np x Kp) and tg (gr.Np): a point's nb = nd + (y ? 1 : 0) observation rows and their targets at rows t nb + i -- the value row
// phi_t with target y_t, then sqrt(rho) gfac[d] (-Phi_s[t] o Fall[d] | Phi_c[t] o Fall[d]) with target sqrt(rho) G for d = dims[j], formed in
// fp64 and rounded once; an entry with rho = 0 gives exact zeros; the padding columns and the rows from g.N nb on are zero.  gr: the
// chunk's geometry in observation rows
template <typename T>
void gradobs_rows(const Geom& gr, const Geom& g, const T* Phi, const double* Fall, const GradObs& a, T* Psi, double* tg, hipStream_t st);

// ---- sobol.hip: closed-form Sobol indices under a product measure (scfgp_sobol) -------------------------------------------------------
constexpr int SOBOL_T = 8;                      // edge of a tile of pairs (j, k)
constexpr int SOBOL_COLS = 32;                  // weight columns per workgroup of the pair kernel
constexpr int SOBOL_GROUP = 16;                 // inputs per workgroup of the pair kernel, at most
// meas (3 x D): kind (0 uniform, 1 normal) | centre or mean | half width or standard deviation.  Jt = round_up(J, SOBOL_T).  psi1[d][j] =
// psi_d(Fall[d][j]) and Ed[d][j] = E_j without its factor d (D x Jt complex each), E_j = E_mu e^{i z_j}, Eb_j = e^{i b_j} (Jt complex
// each; entries j >= J are not written), phibar (K, or NULL) = s (Re E | Im E)
void sobol_tables(const Geom& g, const double* Fall, const Scal* sc, const double* meas, int Jt, double* psi1, double* Ed, double* E,
                  double* Eb, double* phibar, hipStream_t st);
// omax (D) = max_j |Fall[d][j]|: with the measure it bounds every phase the tables and the pair kernel hand to fast_sincos
void sobol_omax(const Geom& g, const double* Fall, double* omax, hipStream_t st);
// W (K x nw, row-major) -> A (Jt x nw complex) = s (W[j] - i W[J + j]), zero rows from J on; f0 (nw, or NULL) = Re sum_j A_j E_j
void sobol_weights(const Geom& g, const double* W, const Scal* sc, const double* E, int Jt, int nw, double* A, double* f0, hipStream_t st);
// The centred quadratic forms of columns w0 .. w0 + ncols of A.  units (3 ints each: block of j, first and one-past-last block of k, blocks
// of SOBOL_T); G <= SOBOL_GROUP inputs per workgroup; flags: 1 = the whole set, 2 = main effects, 4 = closed sets.  rec (nunits x (1 + 2 D)
// x ncols): per unit the partial sums of set 0 = all, 1 + d = main effect of d, 1 + D + d = closed set of d; what flags leave out is
// neither computed nor written
void sobol_pairs(const Geom& g, const double* Fall, const double* meas, const double* psi1, const double* Ed, const double* E,
                 const double* Eb, const double* A, const int* units, int nunits, int Jt, int nw, int w0, int ncols, int G, int flags,
                 double* rec, hipStream_t st);
// sums ((1 + 2 D) x nw): columns w0 .. w0 + ncols of the sets that flags name = the records added in unit order
void sobol_reduce(const double* rec, int nunits, int D, int ncols, int nw, int w0, int flags, double* sums, hipStream_t st);

// ---- pd.hip: partial dependence and ICE curves over a pool (scfgp_predict_pd) ----------------------------------------------------------
// rows that a dimension's G grid points take in the stacked operand Phibar: a multiple of 128, so that predcov finds its padded rows
inline int pd_grid_rows(int G) { return (int)round_up(G, 128); }
// doubles of the block records of one chunk with ng dimensions: one record of 2 Jp doubles per (128-row block, dimension)
int64_t pd_record_len(const Geom& g, int ng);
// acc (ng x 2 x Jp, fp64) += the sums over the chunk's live rows n (n < g.N, wgt[n] > 0; wgt: g.Np weights with zeros on the padding, or NULL
// for all 1) of wgt[n] phi0_n for the dimensions dims[0..ng): phi0 = the features at row n with coordinate d cleared, cosine half then sine
// half.  rec: pd_record_len(g, ng) doubles of scratch; the block records are added in block order.
template <typename T>
void pd_sums(const Geom& g, const double* Xt, const double* Fall, const Scal* sc, const double* wgt, const int* dims, int ng, double* rec,
             double* acc, hipStream_t st);
// grid (ndim x G) <- the X scaler's forward transform (mode, sp: as pack_data) of row a in column dims[a], in place
void pd_grid(double* grid, const int* dims, int ndim, int G, int D, int mode, const double* sp, hipStream_t st);
// Phibar (gr.Np x Kp, type T): row a pd_grid_rows(G) + i = (acc[a] / W) rotated by grid[a][i] Fall[dims[a]][.], a < ng, i < G; all other
// rows and the padding columns zero
template <typename T>
void pd_mean_rows(const Geom& gr, const Geom& g, const double* acc, double W, const double* Fall, const int* dims, const double* grid, int ng,
                  int G, T* Phibar, hipStream_t st);
// R (sample_w_rows(K) x sample_w_cols(G), type T, zero outside K x G): alpha rotated by grid_d[i] Fall[d][.], so that Phi0 R = the ICE block
template <typename T>
void pd_ice_weights(const Geom& g, const double* alpha, const double* Fall, int d, const double* grid_d, int G, T* R, hipStream_t st);
// save != 0: keep (g.Np) <- column d of Xt, which is cleared; save == 0: the column is put back
void pd_column(const Geom& g, double* Xt, int d, int save, double* keep, hipStream_t st);

// ---- select.hip: greedy maximum-information choice of m rows from a pool (scfgp_select) ---------------------------------------------
// C (typed, ld Kp, Trows rows) = Phi_c Li^T of the pool.  Device state of one call: w (Trows: the weights; a picked row's is set to 0),
// d (Trows: the running |c_i|^2 downdated by every pick), pval / pidx (select_partials(Trows) argmax partials of the last sweep), U
// (m x Kp: the u_l), cp (Kp: the picked row in fp64), a (m: u_l . c_p), part (ceil(m / 64) x Kp: chunk sums of the projection), idx /
// var / gain (m each), flag (bit 0: a non-finite |c_i|^2, bit 1: a step found no eligible row).
struct SelectBufs {
    int Kp; int64_t Trows;
    double *w, *d, *pval; long long* pidx;
    double *U, *cp, *a, *part;
    long long* idx; double *var, *gain; int* flag;
};
int select_partials(int64_t Trows);
void select_ones(double* w, int64_t Trows, hipStream_t st);
// d = rowsum(C^2) and the first argmax partials
template <typename T> void select_init(const SelectBufs& b, const T* C, hipStream_t st);
// pick j: idx[j], var[j] = kappa dp, gain[j] = log1p(dp) / 2, u_j into U, then the sweep that downdates d and leaves the next partials
template <typename T> void select_step(const SelectBufs& b, const T* C, int j, const Scal* sc, hipStream_t st);
// sd[i] = sqrt(kappa (1 + d[i]))
void select_std(const SelectBufs& b, const Scal* sc, double* sd, hipStream_t st);

// ---- select.hip: the integrated-variance criterion (scfgp_select_iv) ------------------------------------------------------------------
// Beside SelectBufs: Q (Kp x Kp fp64, symmetric: C_R^T diag(omega) C_R of the reference rows), a (Trows: the running c_i^T P Q P c_i),
// apart (select_iv_tiles(Kp) x Trows: the column-tile shares of the start values), h, v (Kp each), red (m), ivar (2: kappa tr(Q), and that minus
// the reductions so far).  SelectBufs::flag bit 0 also reports a non-finite start value.
struct SelectIvBufs {
    const double* Q;
    double *a, *apart, *h, *v, *red, *ivar;
};
int select_iv_tiles(int Kp);                                      // column tiles of the start values' product: the rows of apart
// d = rowsum(C^2), a = rowsum((C Qt) o C) (Qt: Q in C's type, K live columns), ivar, and the first argmax partials of w a / (1 + d)
template <typename T>
void select_iv_init(const SelectBufs& b, const SelectIvBufs& iv, const T* C, const T* Qt, int K, const Scal* sc, hipStream_t st);
// pick j: idx[j], var[j], u_j as select_step; red[j] = kappa u_j . Q u_j, ivar[1] -= red[j]; then the sweep that downdates a and d and
// leaves the next partials
template <typename T> void select_iv_step(const SelectBufs& b, const SelectIvBufs& iv, const T* C, int j, const Scal* sc, hipStream_t st);

// ---- selectqei.hip: greedy Monte-Carlo batch expected improvement over a pool (scfgp_select_qei) ----------------------------------------
// F (T x nsamp fp64, row pitch nsamp): scfgp_sample's values of the pool, sgn = +1 or -1 (minimize).  Device state of one call: w (T: a
// row is eligible iff w > 0; a picked row's is set to 0), ms (nsamp: the running per-sample maximum m of b, the pending rows and the
// picks, in units sgn f), score0 (T: the scores of pick 0), pval / pidx (selectqei_blocks(T) records of the last sweep), idx / gain (m
// each), qei (2), flag (an eligible row holds a non-finite value).
struct SelectQeiBufs {
    const double* F; int64_t T; int nsamp; double sgn;
    double *w, *ms, *score0, *pval; long long* pidx;
    long long* idx; double *gain, *qei; int* flag;
};
int selectqei_blocks(int64_t T);
// start != 0: ms[s] = max(base, sgn pend[s]) (pend NULL: base) and qei[0]; start == 0: qei[1] from ms as it stands.  qei[.] =
// (1 / nsamp) sum_s (ms[s] - base), by one thread in sample order
void selectqei_state(const SelectQeiBufs& b, const double* pend, double base, int start, hipStream_t st);
// the scores of every row against ms and the workgroups' records; j == 0 also writes score0 and raises the flag
void selectqei_sweep(const SelectQeiBufs& b, int j, hipStream_t st);
// folds the records: idx[j], gain[j], w[idx[j]] = 0, ms raised to the picked row
void selectqei_commit(const SelectQeiBufs& b, int j, hipStream_t st);
