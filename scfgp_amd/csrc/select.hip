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
