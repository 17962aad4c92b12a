// Greedy maximum-information choice of m rows from a pool (scfgp_select; derivation in include/scfgp_hip.h).  With C = Phi_c Li^T (apply_c's
// triangular product) of the T pool rows and d_i = |c_i|^2, step j picks p = argmax w_i d_i over the rows not yet taken, forms
//     t = c_p - sum_{l<j} u_l (u_l . c_p),   dp = c_p . t,   u_j = t / sqrt(1 + dp)
// and downdates d_i <- max(d_i - (c_i . u_j)^2, 0) of every row.  Everything stays on the device between the picks: no step reads an index
// or a value back.
//
// select_sweep_kernel<T, INIT> is the pass over C (INIT: d_i = |c_i|^2; else the downdate by u_j, held in LDS as fp64).  A row belongs
// to one half-wave: lane h of the 32 reads the 16-byte slots h, h + 32, .. of the row (a half-wave reads 512 consecutive bytes per
// instruction), converts to fp64 on load and adds its products into ONE fp64 accumulator in slot order; the 32 accumulators are added by
// the xor butterfly 16, 8, 4, 2, 1.  That order depends on Kp alone: a row's c_i . u has the same bits whatever T is, wherever the row
// sits and whichever workgroup meets it.  Four slots are fetched before the first of them is used.  Lane 0 of the half-wave applies the
// downdate, the clamp and the weight (w_i = 0: not eligible; a picked row's weight is set to 0 by select_pick_kernel) and keeps the
// half-wave's best (score, row); the workgroup's 8 are reduced to one partial, the lowest row winning a tie.
// Rows >= T (the padding rows of the last chunk of the factor pass) are never read.
//
// Per pick: select_pick_kernel (one workgroup: the partials -> p, the lowest row winning a tie; marks the row; c_p in fp64),
// select_dot_kernel (a_l = u_l . c_p, one wave per earlier pick), select_proj_kernel (sum_l a_l u_l in chunks of SELECT_LCHUNK picks
// x 256 columns: the m x Kp array of the u_l is read by many workgroups, never by one), select_finish_kernel (one workgroup: t, dp, u_j,
// var[j] = kappa dp, gain[j] = log1p(dp) / 2), then the sweep.  The chunking of the projection depends on j alone, so step j does the same
// arithmetic whatever m is: the picks of a shorter call are a prefix of a longer one's bit for bit.
#include "kernels.h"
#include "tile_engine.h"

constexpr int SELECT_LCHUNK = 64;               // earlier picks per workgroup of the projection
constexpr long long SELECT_NOROW = 0x7fffffffffffffffLL;

// (va, ia) <- the better of (va, ia), (vb, ib): the larger score, the lower row on a tie
__device__ __forceinline__ void select_better(double& va, long long& ia, double vb, long long ib) {
    if (vb > va || (vb == va && ib < ia)) { va = vb; ia = ib; }
}

template <typename T, bool INIT>
__global__ __launch_bounds__(256) void select_sweep_kernel(const T* __restrict__ C, int Kp, int64_t Trows, int rpw,
                                                           const double* __restrict__ u, const double* __restrict__ w,
                                                           double* __restrict__ d, double* __restrict__ pval,
                                                           long long* __restrict__ pidx, int* __restrict__ flag) {
    typedef typename Vec16<T>::type vec_t;
    constexpr int VN = Vec16<T>::N;
    extern __shared__ double s_u[];                              // u_j (Kp doubles; not INIT)
    __shared__ double s_val[8];
    __shared__ long long s_idx[8];
    const int tid = threadIdx.x, h = tid & 31, grp = tid >> 5;
    if (!INIT) {
        for (int k = tid; k < Kp; k += 256) s_u[k] = u[k];
        __syncthreads();
    }
    const int64_t r0 = (int64_t)blockIdx.x * rpw, r1 = r0 + rpw < Trows ? r0 + rpw : Trows;
    const int nit = Kp / (VN * 32);                              // slots of a row per lane (Kp is a multiple of 128)
    double best_v = -1.0;
    long long best_i = SELECT_NOROW;
    for (int64_t i = r0 + grp; i < r1; i += 8) {
        const vec_t* __restrict__ row = reinterpret_cast<const vec_t*>(C + i * Kp) + h;
        double acc = 0.0;
        for (int it = 0; it < nit; it += 4) {
            vec_t v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (it + q < nit) v[q] = row[(it + q) * 32];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (it + q < nit) {
                    const double* uu = s_u + ((it + q) * 32 + h) * VN;
#pragma unroll
                    for (int e = 0; e < VN; ++e) {
                        const double x = (double)v[q][e];
                        acc = fma(x, INIT ? x : uu[e], acc);
                    }
                }
        }
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (h == 0) {
            double di;
            if (INIT) {
                di = acc;
                if (!isfinite(di)) atomicOr(flag, 1);
            } else {
#pragma clang fp contract(off)
                di = d[i] - acc * acc;
                di = di > 0.0 ? di : 0.0;
            }
            d[i] = di;
            const double wi = w[i];
            if (wi > 0.0) select_better(best_v, best_i, wi * di, (long long)i);
        }
    }
    if (h == 0) { s_val[grp] = best_v; s_idx[grp] = best_i; }
    __syncthreads();
    if (tid == 0) {
        for (int gI = 1; gI < 8; ++gI) select_better(best_v, best_i, s_val[gI], s_idx[gI]);
        pval[blockIdx.x] = best_v; pidx[blockIdx.x] = best_i;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void select_pick_kernel(const double* __restrict__ pval, const long long* __restrict__ pidx, int npart,
                                                          const T* __restrict__ C, int Kp, int64_t Trows, int j, double* __restrict__ w,
                                                          long long* __restrict__ idx, double* __restrict__ cp, int* __restrict__ flag) {
    __shared__ double s_val[256];
    __shared__ long long s_idx[256];
    const int tid = threadIdx.x;
    double bv = -1.0;
    long long bi = SELECT_NOROW;
    for (int k = tid; k < npart; k += 256) select_better(bv, bi, pval[k], pidx[k]);
    s_val[tid] = bv; s_idx[tid] = bi;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) {
            select_better(bv, bi, s_val[tid + s], s_idx[tid + s]);
            s_val[tid] = bv; s_idx[tid] = bi;
        }
        __syncthreads();
    }
    long long p = s_idx[0];
    if (p < 0 || p >= Trows) {                                   // no eligible row (scores of NaN): the host discards the call
        p = 0;
        if (tid == 0) atomicOr(flag, 2);
    }
    if (tid == 0) { idx[j] = p; w[p] = 0.0; }
    const T* __restrict__ row = C + p * Kp;
    for (int k = tid; k < Kp; k += 256) cp[k] = (double)row[k];
}

// a[l] = u_l . c_p for l < j: one wave per l, lane-strided products into one accumulator, xor butterfly
__global__ __launch_bounds__(256) void select_dot_kernel(const double* __restrict__ U, const double* __restrict__ cp, int Kp, int j,
                                                         double* __restrict__ a) {
    const int lane = threadIdx.x & 63, l = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= j) return;
    const double* __restrict__ ul = U + (int64_t)l * Kp;
    double acc = 0.0;
    for (int k = lane; k < Kp; k += 64) acc = fma(ul[k], cp[k], acc);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) a[l] = acc;
}

// part[s][k] = sum over the picks l of chunk s (l < j, in order) of a[l] u_l[k]
__global__ __launch_bounds__(256) void select_proj_kernel(const double* __restrict__ U, const double* __restrict__ a, int Kp, int j,
                                                          double* __restrict__ part) {
    const int k = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (k >= Kp) return;
    const int l0 = s * SELECT_LCHUNK, l1 = l0 + SELECT_LCHUNK < j ? l0 + SELECT_LCHUNK : j;
    double acc = 0.0;
#pragma unroll 8
    for (int l = l0; l < l1; ++l) acc = fma(a[l], U[(int64_t)l * Kp + k], acc);
    part[(int64_t)s * Kp + k] = acc;
}

// t = c_p - sum_s part[s] (in chunk order), dp = c_p . t, u_j = t / sqrt(1 + dp) into uj; var[j], gain[j]
__global__ __launch_bounds__(256) void select_finish_kernel(const double* __restrict__ cp, const double* __restrict__ part, int nchunk, int Kp,
                                                            int j, const Scal* __restrict__ sc, double* __restrict__ uj,
                                                            double* __restrict__ var, double* __restrict__ gain) {
    __shared__ double s_sum[256];
    const int tid = threadIdx.x;
    double dp = 0.0;
    for (int k = tid; k < Kp; k += 256) {
        const double c = cp[k];
        double t = c;
        for (int s = 0; s < nchunk; ++s) t -= part[(int64_t)s * Kp + k];
        uj[k] = t;
        dp = fma(c, t, dp);
    }
    s_sum[tid] = dp;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) s_sum[tid] += s_sum[tid + s];
        __syncthreads();
    }
    dp = s_sum[0];
    dp = dp > 0.0 ? dp : 0.0;
    const double den = sqrt(1.0 + dp);
    for (int k = tid; k < Kp; k += 256) uj[k] = uj[k] / den;    // a thread rescales the entries it wrote itself
    if (tid == 0) {
        var[j] = sc->kappa * dp;
        gain[j] = 0.5 * log1p(dp);
    }
}

__global__ __launch_bounds__(256) void select_init_weights_kernel(double* __restrict__ w, int64_t Trows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < Trows) w[i] = 1.0;
}

__global__ __launch_bounds__(256) void select_std_kernel(const double* __restrict__ d, int64_t Trows, const Scal* __restrict__ sc,
                                                         double* __restrict__ sd) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < Trows) sd[i] = sqrt(sc->kappa * (1.0 + d[i]));
}

int select_rows_per_group(int64_t Trows) {
    int rpw = 64;
    while ((Trows + rpw - 1) / rpw > 4096) rpw *= 2;
    return rpw;
}
int select_partials(int64_t Trows) {
    const int rpw = select_rows_per_group(Trows);
    return (int)((Trows + rpw - 1) / rpw);
}

void select_ones(double* w, int64_t Trows, hipStream_t st) {
    hipLaunchKernelGGL(select_init_weights_kernel, dim3((unsigned)((Trows + 255) / 256)), dim3(256), 0, st, w, Trows);
}

template <typename T>
void select_init(const SelectBufs& b, const T* C, hipStream_t st) {
    const int rpw = select_rows_per_group(b.Trows);
    hipLaunchKernelGGL((select_sweep_kernel<T, true>), dim3((unsigned)select_partials(b.Trows)), dim3(256), 0, st, C, b.Kp, b.Trows, rpw,
                       (const double*)nullptr, (const double*)b.w, b.d, b.pval, b.pidx, b.flag);
}

template <typename T>
void select_step(const SelectBufs& b, const T* C, int j, const Scal* sc, hipStream_t st) {
    const int rpw = select_rows_per_group(b.Trows), npart = select_partials(b.Trows);
    double* uj = b.U + (int64_t)j * b.Kp;
    hipLaunchKernelGGL(select_pick_kernel<T>, dim3(1), dim3(256), 0, st, (const double*)b.pval, (const long long*)b.pidx, npart, C, b.Kp,
                       b.Trows, j, b.w, b.idx, b.cp, b.flag);
    const int nchunk = (j + SELECT_LCHUNK - 1) / SELECT_LCHUNK;
    if (j > 0) {
        hipLaunchKernelGGL(select_dot_kernel, dim3((unsigned)((j + 3) / 4)), dim3(256), 0, st, (const double*)b.U, (const double*)b.cp, b.Kp, j,
                           b.a);
        hipLaunchKernelGGL(select_proj_kernel, dim3((unsigned)((b.Kp + 255) / 256), (unsigned)nchunk), dim3(256), 0, st, (const double*)b.U,
                           (const double*)b.a, b.Kp, j, b.part);
    }
    hipLaunchKernelGGL(select_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)b.cp, (const double*)b.part, nchunk, b.Kp, j, sc, uj,
                       b.var, b.gain);
    hipLaunchKernelGGL((select_sweep_kernel<T, false>), dim3((unsigned)npart), dim3(256), sizeof(double) * b.Kp, st, C, b.Kp, b.Trows, rpw,
                       (const double*)uj, (const double*)b.w, b.d, b.pval, b.pidx, b.flag);
}

void select_std(const SelectBufs& b, const Scal* sc, double* sd, hipStream_t st) {
    hipLaunchKernelGGL(select_std_kernel, dim3((unsigned)((b.Trows + 255) / 256)), dim3(256), 0, st, (const double*)b.d, b.Trows, sc, sd);
}

template void select_init<double>(const SelectBufs&, const double*, hipStream_t);
template void select_init<float>(const SelectBufs&, const float*, hipStream_t);
template void select_step<double>(const SelectBufs&, const double*, int, const Scal*, hipStream_t);
template void select_step<float>(const SelectBufs&, const float*, int, const Scal*, hipStream_t);

// ---- integrated-variance criterion (scfgp_select_iv; derivation in include/scfgp_hip.h) ------------------------------------------------
// The score of row i is w_i a_i / (1 + d_i) with a_i = c_i^T P Q P c_i, Q = C_R^T diag(omega) C_R of the reference rows (formed once by
// the weighted Gram tiles, fp64 Kp x Kp, symmetric) and P = I - sum_l u_l u_l^T.  A pick forms u_j as select_step does (the same four
// kernels), then h = Q u_j (select_iv_gemv_kernel: one wave per row of Q), q = u_j . h, g = h - sum_{l<j} u_l (u_l . h) (the dot and
// projection kernels again), v = g - (q / 2) u_j (select_iv_v_kernel, which also writes red[j] = kappa q and the running integrated
// variance), and select_iv_sweep_kernel downdates a_i by 2 (c_i . u_j)(c_i . v) and d_i by (c_i . u_j)^2 in ONE pass over C.
//
// select_iv_rowdot_kernel forms the start values a_i = c_i^T Q c_i = rowsum((C Q) o C): predcov.hip's NT tile product (Q is symmetric,
// so row k of Q is column k; the same LDS image, swizzle and double buffering, described there) of a 128-row panel of C with a
// 128-row panel of the typed Q, whose epilogue multiplies the accumulator tile with the matching 128 x 128 tile of C and adds along
// the row: the 4 MFMA tiles of a lane in column order, the 16 lanes of a row by the xor butterfly 8, 4, 2, 1, the wave of columns
// 64.. to the wave of columns 0.. through LDS.  E = C Q never exists in memory.  apart[jt][i] is the share of column tile jt;
// select_iv_init_kernel adds the shares in tile order, so a_i has one summation order whatever T is.
constexpr int SELIV_TILE = 128;
constexpr int SELIV_FLUSH = 128;

int select_iv_tiles(int Kp) { return Kp / SELIV_TILE; }

template <typename T>
__global__ __launch_bounds__(256) void select_iv_rowdot_kernel(const T* __restrict__ C, const T* __restrict__ Q, int Kp, int nkt,
                                                               int64_t Trows, double* __restrict__ apart) {
    typedef MT<T, 16> M;
    typedef typename Vec16<T>::type vec_t;                       // one 16-byte slot
    constexpr bool F32 = sizeof(T) == 4;
    constexpr int VN = Vec16<T>::N, BK = 8 * VN;                 // features per slot, per k-tile
    constexpr int SLOTS = SELIV_TILE * 8;                        // 16-byte slots of one panel image
    constexpr int FLUSH_KT = SELIV_FLUSH / BK;
    __shared__ vec_t lds[2][2][SLOTS];                           // [buffer][operand]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int64_t r0 = (int64_t)blockIdx.y * SELIV_TILE, c0 = (int64_t)blockIdx.x * SELIV_TILE;

    // staging: thread t moves slot t % 8 of rows t / 8 + 32 j of both panels (8 lanes: one 128-byte row segment)
    const int srow = tid >> 3, sslot = tid & 7;
    const vec_t* __restrict__ ga = reinterpret_cast<const vec_t*>(C + (r0 + srow) * Kp) + sslot;
    const vec_t* __restrict__ gb = reinterpret_cast<const vec_t*>(Q + (c0 + srow) * Kp) + sslot;
    const int64_t gstep = (int64_t)32 * Kp / VN;                 // 32 rows, in slots
    int soff[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = srow + 32 * j;
        soff[j] = r * 8 + (sslot ^ ((r >> 1) & 7));
    }
    vec_t pa[4], pb[4];
    auto fetch = [&](int kt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { pa[j] = ga[j * gstep + kt * 8]; pb[j] = gb[j * gstep + kt * 8]; }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { lds[buf][0][soff[j]] = pa[j]; lds[buf][1][soff[j]] = pb[j]; }
    };
    const int aoff = (wm + i) * 8, boff = (wn + i) * 8, swz = (i >> 1) & 7;

    typename M::acc_t acc[4][4];
    double part[F32 ? 4 : 1][4][4];                              // fp32 only: the fp64 sums of the flushed accumulators
#pragma unroll
    for (int tm = 0; tm < 4; ++tm)
#pragma unroll
        for (int tn = 0; tn < 4; ++tn)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                acc[tm][tn][r] = 0;
                if constexpr (F32) part[tm][tn][r] = 0.0;
            }

    fetch(0);
    stage(0);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nkt) fetch(kt + 1);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            vec_t a[4], b[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                a[t] = lds[buf][0][aoff + 128 * t + ((q + 4 * h) ^ swz)];
                b[t] = lds[buf][1][boff + 128 * t + ((q + 4 * h) ^ swz)];
            }
#pragma unroll
            for (int e = 0; e < VN; ++e)
#pragma unroll
                for (int tm = 0; tm < 4; ++tm)
#pragma unroll
                    for (int tn = 0; tn < 4; ++tn) M::mfma(acc[tm][tn], a[tm][e], b[tn][e]);
        }
        if constexpr (F32) {
            if ((kt + 1) % FLUSH_KT == 0 || kt + 1 == nkt) {
#pragma unroll
                for (int tm = 0; tm < 4; ++tm)
#pragma unroll
                    for (int tn = 0; tn < 4; ++tn)
#pragma unroll
                        for (int r = 0; r < 4; ++r) { part[tm][tn][r] += (double)acc[tm][tn][r]; acc[tm][tn][r] = 0; }
            }
        }
        // the other buffer was last read before the barrier that ended tile kt - 1
        if (kt + 1 < nkt) stage(buf ^ 1);
        __syncthreads();
    }

    // epilogue: rowsum(E o C) over the wave's 64 columns (rows below round_up(Trows, 128) are readable: zero beyond Trows); the
    // panel images are dead behind the loop's last barrier: their head carries the row sums of the columns 64.. of the tile
    double* s_half = reinterpret_cast<double*>(&lds[0][0][0]);
    double rs[4][4];
#pragma unroll
    for (int tm = 0; tm < 4; ++tm)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t n = r0 + wm + 16 * tm + M::crow(lane, r);
            const T* __restrict__ crow_p = C + n * Kp + c0 + wn + i;
            double s = 0.0;
#pragma unroll
            for (int tn = 0; tn < 4; ++tn) {
                double e;
                if constexpr (F32) e = part[tm][tn][r];
                else e = (double)acc[tm][tn][r];
                s = fma(e, (double)crow_p[16 * tn], s);
            }
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
            rs[tm][r] = s;
        }
    if (wn == 64 && i == 0) {
#pragma unroll
        for (int tm = 0; tm < 4; ++tm)
#pragma unroll
            for (int r = 0; r < 4; ++r) s_half[wm + 16 * tm + M::crow(lane, r)] = rs[tm][r];
    }
    __syncthreads();
    if (wn == 0 && i == 0) {
#pragma unroll
        for (int tm = 0; tm < 4; ++tm)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int nl = wm + 16 * tm + M::crow(lane, r);
                const int64_t n = r0 + nl;
                if (n < Trows) apart[(int64_t)blockIdx.x * Trows + n] = rs[tm][r] + s_half[nl];
            }
    }
}

// a_i = sum over the column tiles, in tile order, of apart[jt][i]; flag bit 0 for a non-finite a_i; the first argmax partials of the
// score w_i a_i / (1 + d_i) (block b: rows [b rpw, (b + 1) rpw), as the sweep)
__global__ __launch_bounds__(256) void select_iv_init_kernel(const double* __restrict__ apart, int ntile, int64_t Trows, int rpw,
                                                             const double* __restrict__ w, const double* __restrict__ d,
                                                             double* __restrict__ a, double* __restrict__ pval,
                                                             long long* __restrict__ pidx, int* __restrict__ flag) {
    __shared__ double s_val[256];
    __shared__ long long s_idx[256];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * rpw, r1 = r0 + rpw < Trows ? r0 + rpw : Trows;
    double bv = -1.0;
    long long bi = SELECT_NOROW;
    for (int64_t i = r0 + tid; i < r1; i += 256) {
        double ai = 0.0;
        for (int jt = 0; jt < ntile; ++jt) ai += apart[(int64_t)jt * Trows + i];
        if (!isfinite(ai)) atomicOr(flag, 1);
        a[i] = ai;
        const double wi = w[i];
        if (wi > 0.0) {
#pragma clang fp contract(off)
            select_better(bv, bi, wi * ai / (1.0 + d[i]), (long long)i);
        }
    }
    s_val[tid] = bv; s_idx[tid] = bi;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) {
            select_better(bv, bi, s_val[tid + s], s_idx[tid + s]);
            s_val[tid] = bv; s_idx[tid] = bi;
        }
        __syncthreads();
    }
    if (tid == 0) { pval[blockIdx.x] = bv; pidx[blockIdx.x] = bi; }
}

// ivar[0] = ivar[1] = kappa tr(Q): one workgroup, thread-strided diagonal, tree sum
__global__ __launch_bounds__(256) void select_iv_trace_kernel(const double* __restrict__ Q, int Kp, const Scal* __restrict__ sc,
                                                              double* __restrict__ ivar) {
    __shared__ double s_sum[256];
    const int tid = threadIdx.x;
    double t = 0.0;
    for (int k = tid; k < Kp; k += 256) t += Q[(int64_t)k * Kp + k];
    s_sum[tid] = t;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) s_sum[tid] += s_sum[tid + s];
        __syncthreads();
    }
    if (tid == 0) { ivar[0] = sc->kappa * s_sum[0]; ivar[1] = ivar[0]; }
}

// h[k] = Q[k] . u: one wave per row of Q (Kp is a multiple of 128), 16-byte loads, one accumulator per lane in column order, xor butterfly
__global__ __launch_bounds__(256) void select_iv_gemv_kernel(const double* __restrict__ Q, const double* __restrict__ u, int Kp,
                                                             double* __restrict__ h) {
    const int lane = threadIdx.x & 63, k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= Kp) return;
    const double* __restrict__ row = Q + (int64_t)k * Kp;
    double acc = 0.0;
#pragma unroll 4
    for (int l = 2 * lane; l < Kp; l += 128) {
        const v2d x = *reinterpret_cast<const v2d*>(row + l);
        const v2d y = *reinterpret_cast<const v2d*>(u + l);
        acc = fma(x[0], y[0], acc);
        acc = fma(x[1], y[1], acc);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) h[k] = acc;
}

// q = u_j . h; v = h - sum_s part[s] (in chunk order) - (q / 2) u_j; red[j] = kappa q; ivar[1] -= red[j] (one workgroup, thread 0 for
// the scalars: the running sum is formed in pick order)
__global__ __launch_bounds__(256) void select_iv_v_kernel(const double* __restrict__ uj, const double* __restrict__ h,
                                                          const double* __restrict__ part, int nchunk, int Kp, int j,
                                                          const Scal* __restrict__ sc, double* __restrict__ v, double* __restrict__ red,
                                                          double* __restrict__ ivar) {
    __shared__ double s_sum[256];
    const int tid = threadIdx.x;
    double q = 0.0;
    for (int k = tid; k < Kp; k += 256) q = fma(uj[k], h[k], q);
    s_sum[tid] = q;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) s_sum[tid] += s_sum[tid + s];
        __syncthreads();
    }
    q = s_sum[0];
    {
#pragma clang fp contract(off)
        const double hq = 0.5 * q;
        for (int k = tid; k < Kp; k += 256) {
            double gk = h[k];
            for (int s = 0; s < nchunk; ++s) gk -= part[(int64_t)s * Kp + k];
            v[k] = gk - hq * uj[k];
        }
        if (tid == 0) {
            const double r = sc->kappa * q;
            red[j] = r;
            ivar[1] = ivar[1] - r;
        }
    }
}

// select_sweep_kernel's pass over C with two vectors: the same row-to-half-wave mapping, slot order, four-slot prefetch and butterfly,
// two fp64 accumulators (s_i = c_i . u_j, z_i = c_i . v; u_j and v in LDS, 2 Kp doubles).  Lane 0 downdates a_i and d_i, clamps both
// and scores w_i a_i / (1 + d_i).  The 8 half-wave results are reduced through the head of the same LDS array once every row is done.
template <typename T>
__global__ __launch_bounds__(256) void select_iv_sweep_kernel(const T* __restrict__ C, int Kp, int64_t Trows, int rpw,
                                                              const double* __restrict__ u, const double* __restrict__ v,
                                                              const double* __restrict__ w, double* __restrict__ d, double* __restrict__ a,
                                                              double* __restrict__ pval, long long* __restrict__ pidx) {
    typedef typename Vec16<T>::type vec_t;
    constexpr int VN = Vec16<T>::N;
    extern __shared__ double s_uv[];                             // u_j | v (Kp doubles each)
    const int tid = threadIdx.x, h = tid & 31, grp = tid >> 5;
    for (int k = tid; k < Kp; k += 256) { s_uv[k] = u[k]; s_uv[Kp + k] = v[k]; }
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * rpw, r1 = r0 + rpw < Trows ? r0 + rpw : Trows;
    const int nit = Kp / (VN * 32);                              // slots of a row per lane (Kp is a multiple of 128)
    double best_v = -1.0;
    long long best_i = SELECT_NOROW;
    for (int64_t i = r0 + grp; i < r1; i += 8) {
        const vec_t* __restrict__ row = reinterpret_cast<const vec_t*>(C + i * Kp) + h;
        double accu = 0.0, accv = 0.0;
        for (int it = 0; it < nit; it += 4) {
            vec_t x4[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (it + q < nit) x4[q] = row[(it + q) * 32];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (it + q < nit) {
                    const double* uu = s_uv + ((it + q) * 32 + h) * VN;
                    const double* vv = uu + Kp;
#pragma unroll
                    for (int e = 0; e < VN; ++e) {
                        const double x = (double)x4[q][e];
                        accu = fma(x, uu[e], accu);
                        accv = fma(x, vv[e], accv);
                    }
                }
        }
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) {
            accu += __shfl_xor(accu, off, 64);
            accv += __shfl_xor(accv, off, 64);
        }
        if (h == 0) {
#pragma clang fp contract(off)
            double di = d[i] - accu * accu;
            di = di > 0.0 ? di : 0.0;
            double ai = a[i] - 2.0 * accu * accv;
            ai = ai > 0.0 ? ai : 0.0;
            d[i] = di; a[i] = ai;
            const double wi = w[i];
            if (wi > 0.0) select_better(best_v, best_i, wi * ai / (1.0 + di), (long long)i);
        }
    }
    __syncthreads();                                             // u_j and v are dead: their first 16 slots carry the reduction
    double* s_val = s_uv;
    long long* s_idx = reinterpret_cast<long long*>(s_uv + 8);
    if (h == 0) { s_val[grp] = best_v; s_idx[grp] = best_i; }
    __syncthreads();
    if (tid == 0) {
        for (int gI = 1; gI < 8; ++gI) select_better(best_v, best_i, s_val[gI], s_idx[gI]);
        pval[blockIdx.x] = best_v; pidx[blockIdx.x] = best_i;
    }
}

template <typename T>
void select_iv_init(const SelectBufs& b, const SelectIvBufs& iv, const T* C, const T* Qt, int K, const Scal* sc, hipStream_t st) {
    constexpr int BK = 8 * Vec16<T>::N;
    const int rpw = select_rows_per_group(b.Trows), npart = select_partials(b.Trows), ntile = select_iv_tiles(b.Kp);
    const int nkt = (int)(round_up(K, BK) / BK);                 // <= Kp / BK: Kp is a multiple of 128
    select_init<T>(b, C, st);                                    // d and its non-finite flag; the partials are replaced below
    hipLaunchKernelGGL(select_iv_trace_kernel, dim3(1), dim3(256), 0, st, iv.Q, b.Kp, sc, iv.ivar);
    const dim3 grid((unsigned)ntile, (unsigned)((b.Trows + SELIV_TILE - 1) / SELIV_TILE));
    hipLaunchKernelGGL(select_iv_rowdot_kernel<T>, grid, dim3(256), 0, st, C, Qt, b.Kp, nkt, b.Trows, iv.apart);
    hipLaunchKernelGGL(select_iv_init_kernel, dim3((unsigned)npart), dim3(256), 0, st, (const double*)iv.apart, ntile, b.Trows, rpw,
                       (const double*)b.w, (const double*)b.d, iv.a, b.pval, b.pidx, b.flag);
}

template <typename T>
void select_iv_step(const SelectBufs& b, const SelectIvBufs& iv, const T* C, int j, const Scal* sc, hipStream_t st) {
    const int rpw = select_rows_per_group(b.Trows), npart = select_partials(b.Trows);
    double* uj = b.U + (int64_t)j * b.Kp;
    // u_j: select_step's launches
    hipLaunchKernelGGL(select_pick_kernel<T>, dim3(1), dim3(256), 0, st, (const double*)b.pval, (const long long*)b.pidx, npart, C, b.Kp,
                       b.Trows, j, b.w, b.idx, b.cp, b.flag);
    const int nchunk = (j + SELECT_LCHUNK - 1) / SELECT_LCHUNK;
    const dim3 dgrid((unsigned)((j + 3) / 4)), pgrid((unsigned)((b.Kp + 255) / 256), (unsigned)nchunk);
    if (j > 0) {
        hipLaunchKernelGGL(select_dot_kernel, dgrid, dim3(256), 0, st, (const double*)b.U, (const double*)b.cp, b.Kp, j, b.a);
        hipLaunchKernelGGL(select_proj_kernel, pgrid, dim3(256), 0, st, (const double*)b.U, (const double*)b.a, b.Kp, j, b.part);
    }
    hipLaunchKernelGGL(select_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)b.cp, (const double*)b.part, nchunk, b.Kp, j, sc, uj,
                       b.var, b.gain);
    // h = Q u_j, g = P h (P from before this pick), v
    hipLaunchKernelGGL(select_iv_gemv_kernel, dim3((unsigned)((b.Kp + 3) / 4)), dim3(256), 0, st, iv.Q, (const double*)uj, b.Kp, iv.h);
    if (j > 0) {
        hipLaunchKernelGGL(select_dot_kernel, dgrid, dim3(256), 0, st, (const double*)b.U, (const double*)iv.h, b.Kp, j, b.a);
        hipLaunchKernelGGL(select_proj_kernel, pgrid, dim3(256), 0, st, (const double*)b.U, (const double*)b.a, b.Kp, j, b.part);
    }
    hipLaunchKernelGGL(select_iv_v_kernel, dim3(1), dim3(256), 0, st, (const double*)uj, (const double*)iv.h, (const double*)b.part, nchunk,
                       b.Kp, j, sc, iv.v, iv.red, iv.ivar);
    hipLaunchKernelGGL(select_iv_sweep_kernel<T>, dim3((unsigned)npart), dim3(256), sizeof(double) * 2 * b.Kp, st, C, b.Kp, b.Trows, rpw,
                       (const double*)uj, (const double*)iv.v, (const double*)b.w, b.d, iv.a, b.pval, b.pidx);
}

template void select_iv_init<double>(const SelectBufs&, const SelectIvBufs&, const double*, const double*, int, const Scal*, hipStream_t);
template void select_iv_init<float>(const SelectBufs&, const SelectIvBufs&, const float*, const float*, int, const Scal*, hipStream_t);
template void select_iv_step<double>(const SelectBufs&, const SelectIvBufs&, const double*, int, const Scal*, hipStream_t);
template void select_iv_step<float>(const SelectBufs&, const SelectIvBufs&, const float*, int, const Scal*, hipStream_t);
