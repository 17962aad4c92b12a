// Partial dependence and ICE curves over a pool (scfgp_predict_pd; derivation and promises in include/scfgp_hip.h and DESIGN 4.19).
//   A phase is linear in x: z_j = sum_e x_e Fall[e][j] + b_j, so row t with coordinate d replaced by g has phase z0_tj + g Fall[d][j],
//   z0_tj = z_tj - x_td Fall[d][j], and its features are the zeroed-column features phi0_t rotated by g Fall[d][j] pair by pair.
//   The PD curve needs the weighted mean of phi0 over the pool alone (K numbers per dimension): pd_sums forms its sums without ever
//   writing Phi0; pd_rotate turns the mean into the rows Phibar_d[i] (the operand of apply_c and predcov) and alpha into the weight
//   matrix R_d of the ICE product (the operand of sample_product).
#include "kernels.h"
#include "tile_engine.h"
#include "sincos.h"

#define SMEM_DECL extern __shared__ __attribute__((aligned(16))) char smem_raw[]
typedef TileCfg<double, 128, 64, 16, 4, 2, 16, true> PdCfg;      // featuremap_kernel's tile (fmap.hip), restated

// --------------------------------------------------------------------------
// the sums: rec[rb][a][h][j] = sum over the live rows n of row block rb of w_n phi0^(d_a)_n, h = 0 cosine | 1 sine
// --------------------------------------------------------------------------
// One workgroup: 128 rows x the column tiles [jt0, jt0 + nseg) of Z = X~ Fall (fp64 MFMA), as featuremap_kernel runs them.  In place of
// that kernel's store, every finished 128 x 64 tile of Z goes through the call's dimensions: z0 = z - x_d Fall[d][j], sin / cos in the
// context's type, the scale s = s_hi + s_lo, times w_n in fp64, then the sum over the block's 128 rows in a fixed order:
//   a lane's 8 rows (tm, then r), the 4 lanes that share a column (lane ^ 16, then lane ^ 32), the 4 waves that share it (LDS, in wave order).
// A row with w_n == 0 (or n >= N) is selected away, not multiplied: its phase may be anything.
// wgt: Np weights, zero on the padding rows (pack_data's copy), or NULL for all 1.
template <typename T>
__global__ __launch_bounds__(PdCfg::THREADS) void pd_sums_kernel(
    const double* __restrict__ Xt, const double* __restrict__ Fall, const Scal* __restrict__ sc, const double* __restrict__ wgt,
    const int* __restrict__ dims, int ng, double* __restrict__ rec, int Dp, int Jp, int64_t N, int njt, int ncs) {
    typedef PdCfg Cfg;
    SMEM_DECL;
    __shared__ double red[2][2][Cfg::WGM][Cfg::BN];             // [parity of the dimension][cos | sin][wave row][column]
    double* smem = reinterpret_cast<double*>(smem_raw);
    const int cs = blockIdx.x % ncs;                            // column range of this workgroup
    const int64_t rb = blockIdx.x / ncs;
    const int per = (njt + ncs - 1) / ncs, jt0 = cs * per, nseg = (jt0 + per <= njt ? per : njt - jt0);
    if (nseg <= 0) return;
    const int nkt = Dp / Cfg::BK;
    TrLoader<double, double, Cfg::BM, Cfg::BK, Cfg::LDA, Cfg::THREADS, false, Cfg::SWZA> la(Xt + rb * Cfg::BM * Dp, Dp, threadIdx.x);
    NatLoader<double, double, Cfg::BN, Cfg::BK, Cfg::LDB, Cfg::THREADS, false, false> lb(Fall + jt0 * Cfg::BN, Jp, threadIdx.x);
    typename Cfg::MTr::acc_t acc[Cfg::TM][Cfg::TN];
    acc_zero<Cfg>(acc);
    const double s = sc->s;
    const T s_hi = (T)s, s_lo = (T)(s - (double)s_hi);
    AccCoord<Cfg> co;
    const int wm = (int)(threadIdx.x >> 6) / Cfg::WGN;
    // the weights of this lane's 8 rows; 0 = not live
    double wr[Cfg::TM][Cfg::MTr::NACC];
#pragma unroll
    for (int tm = 0; tm < Cfg::TM; ++tm)
#pragma unroll
        for (int r = 0; r < Cfg::MTr::NACC; ++r) {
            const int64_t n = rb * Cfg::BM + co.row(tm, r);
            wr[tm][r] = n < N ? (wgt ? wgt[n] : 1.0) : 0.0;
        }
    int par = 0;
    tile_mainloop_segments<Cfg>(la, lb, nkt, nseg, -(int64_t)Dp, (int64_t)Cfg::BN - (int64_t)Dp * Jp, acc, smem,
        [&](int seg, typename Cfg::MTr::acc_t (&a)[Cfg::TM][Cfg::TN]) {
            const int jb = (jt0 + seg) * Cfg::BN;
            for (int ai = 0; ai < ng; ++ai) {
                const int d = dims[ai];
                double xd[Cfg::TM][Cfg::MTr::NACC];
#pragma unroll
                for (int tm = 0; tm < Cfg::TM; ++tm)
#pragma unroll
                    for (int r = 0; r < Cfg::MTr::NACC; ++r) xd[tm][r] = Xt[(rb * Cfg::BM + co.row(tm, r)) * Dp + d];
#pragma unroll
                for (int tn = 0; tn < Cfg::TN; ++tn) {
                    const double f = Fall[(int64_t)d * Jp + jb + co.col(tn)];
                    double sumc = 0.0, sums = 0.0;
#pragma unroll
                    for (int tm = 0; tm < Cfg::TM; ++tm)
#pragma unroll
                        for (int r = 0; r < Cfg::MTr::NACC; ++r) {
                            T sn, cs_;
                            fast_sincos(a[tm][tn][r] - xd[tm][r] * f, sn, cs_);
                            const T vc = fma(cs_, s_hi, cs_ * s_lo), vs = fma(sn, s_hi, sn * s_lo);
                            const bool live = wr[tm][r] > 0.0;
                            sumc += live ? wr[tm][r] * (double)vc : 0.0;
                            sums += live ? wr[tm][r] * (double)vs : 0.0;
                        }
                    sumc += __shfl_xor(sumc, 16); sums += __shfl_xor(sums, 16);
                    sumc += __shfl_xor(sumc, 32); sums += __shfl_xor(sums, 32);
                    if (co.lane < 16) {
                        red[par][0][wm][co.col(tn)] = sumc;
                        red[par][1][wm][co.col(tn)] = sums;
                    }
                }
                __syncthreads();
                // one barrier per dimension: the next dimension writes the other half of red, and the one after that comes behind
                // the next barrier, which every reader of this half has passed
                if (threadIdx.x < 2 * Cfg::BN) {
                    const int h = threadIdx.x / Cfg::BN, j = threadIdx.x % Cfg::BN;
                    double v = red[par][h][0][j];
#pragma unroll
                    for (int m = 1; m < Cfg::WGM; ++m) v += red[par][h][m][j];
                    rec[((rb * ng + ai) * 2 + h) * Jp + jb + j] = v;
                }
                par ^= 1;
            }
        });
}

// acc[a][h][j] += rec[rb][a][h][j] over rb = 0 .. nrb - 1 in that order, one lane per entry (n = ng 2 Jp entries)
__global__ __launch_bounds__(256) void pd_reduce_kernel(const double* __restrict__ rec, int64_t nrb, int64_t n, double* __restrict__ acc) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    double a = acc[x];
    int64_t b = 0;
    for (; b + 8 <= nrb; b += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = rec[(b + u) * n + x];
#pragma unroll
        for (int u = 0; u < 8; ++u) a += v[u];
    }
    for (; b < nrb; ++b) a += rec[b * n + x];
    acc[x] = a;
}

// the X scaler's forward transform of pack_data (fmap.hip), restated for the grid values of a column
__device__ __forceinline__ double pd_scale_x(double x, int mode, const double* __restrict__ sp, int D, int d) {
    if (mode == 0) return x;
    const double mn = sp[d], mx = sp[D + d], lm = sp[2 * D + d], mu = sp[3 * D + d], sd = sp[4 * D + d];
    if (mode == 1) return (x - mn) / (mx - mn);
    if (mode == 2) return (x - mu) / sd;
    if (mode == 3) return 0.5 * erfc(-((x - mu) / sd) * 0.70710678118654752440);
    const double t = (x - mn) / (mx - mn);
    const double bc = ((t < 0 ? -1.0 : (t > 0 ? 1.0 : 0.0)) * pow(fabs(t), lm) - 1.0) / lm;       // sign(t)|t|^lm
    const double z = (bc - mu) / sd;
    return mode == 4 ? z : 0.5 * erfc(-z * 0.70710678118654752440);
}
__global__ void pd_grid_kernel(double* __restrict__ grid, const int* __restrict__ dims, int ndim, int G, int D, int mode,
                               const double* __restrict__ sp) {
    const int total = ndim * G;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) grid[e] = pd_scale_x(grid[e], mode, sp, D, dims[e / G]);
}

// Phibar (nrows x Kp, type T): row a Gp + i (a < ng, i < G) = the mean zeroed-column features acc[a] / W rotated by g_i Fall[d_a][.]; every
// other row, and the columns from 2 J on, zero.  fp64 throughout, rounded once.  One workgroup per row.
template <typename T>
__global__ __launch_bounds__(256) void pd_mean_rows_kernel(const double* __restrict__ acc, double W, const double* __restrict__ Fall,
                                                           const int* __restrict__ dims, const double* __restrict__ grid, int ng, int G,
                                                           int Gp, int J, int Jp, int Kp, T* __restrict__ Phibar) {
    const int64_t row = blockIdx.x;
    const int a = (int)(row / Gp), i = (int)(row % Gp);
    T* out = Phibar + row * Kp;
    if (a >= ng || i >= G) {
        for (int c = threadIdx.x; c < Kp; c += 256) out[c] = (T)0;
        return;
    }
    const double gi = grid[(int64_t)a * G + i];
    const double* f = Fall + (int64_t)dims[a] * Jp;
    const double* mc = acc + (int64_t)a * 2 * Jp;
    const double* ms = mc + Jp;
    for (int j = threadIdx.x; j < J; j += 256) {
        double sn, cs;
        fast_sincos(gi * f[j], sn, cs);
        const double c0 = mc[j] / W, s0 = ms[j] / W;
        out[j] = (T)(c0 * cs - s0 * sn);
        out[J + j] = (T)(s0 * cs + c0 * sn);
    }
    for (int c = 2 * J + threadIdx.x; c < Kp; c += 256) out[c] = (T)0;
}

// R (rows x cols, type T; sample_product's weight layout): R[j][i] = alpha_j c_ij + alpha_{J+j} s_ij, R[J+j][i] = alpha_{J+j} c_ij -
// alpha_j s_ij with (c, s)_ij = (cos, sin)(g_i Fall[d][j]); zero outside 2 J x G
template <typename T>
__global__ __launch_bounds__(256) void pd_ice_weights_kernel(const double* __restrict__ alpha, const double* __restrict__ Fall_d,
                                                             const double* __restrict__ grid_d, int G, int J, int64_t rows, int cols,
                                                             T* __restrict__ R) {
    const int64_t total = rows * cols;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t k = e / cols;
        const int i = (int)(e - k * cols);
        double v = 0.0;
        if (k < 2 * J && i < G) {
            const int j = (int)(k < J ? k : k - J);
            double sn, cs;
            fast_sincos(grid_d[i] * Fall_d[j], sn, cs);
            v = k < J ? alpha[j] * cs + alpha[J + j] * sn : alpha[J + j] * cs - alpha[j] * sn;
        }
        R[e] = (T)v;
    }
}

// save != 0: keep[n] = Xt[n][d], Xt[n][d] = 0; else Xt[n][d] = keep[n]  (n < Np)
__global__ void pd_column_kernel(double* __restrict__ Xt, int Dp, int d, int64_t Np, int save, double* __restrict__ keep) {
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < Np; n += (int64_t)gridDim.x * 256) {
        if (save) { keep[n] = Xt[n * Dp + d]; Xt[n * Dp + d] = 0.0; }
        else Xt[n * Dp + d] = keep[n];
    }
}

int64_t pd_record_len(const Geom& g, int ng) { return g.Np / PdCfg::BM * (int64_t)ng * 2 * g.Jp; }

template <typename T>
void pd_sums(const Geom& g, const double* Xt, const double* Fall, const Scal* sc, const double* wgt, const int* dims, int ng, double* rec,
             double* acc, hipStream_t st) {
    const int njt = g.Jp / PdCfg::BN;
    const int64_t nrb = g.Np / PdCfg::BM;
    // featuremap's column ranges: one per row block for large N, more for small N
    const int ncs = (int)std::min<int64_t>(njt, std::max<int64_t>(1, (6144 + nrb - 1) / nrb));
    allow_big_lds(pd_sums_kernel<T>, PdCfg::LDS_BYTES);
    hipLaunchKernelGGL(pd_sums_kernel<T>, dim3((unsigned)(ncs * nrb)), dim3(PdCfg::THREADS), PdCfg::LDS_BYTES, st, Xt, Fall, sc, wgt, dims, ng,
                       rec, g.Dp, g.Jp, g.N, njt, ncs);
    const int64_t n = (int64_t)ng * 2 * g.Jp;
    hipLaunchKernelGGL(pd_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, rec, nrb, n, acc);
}

void pd_grid(double* grid, const int* dims, int ndim, int G, int D, int mode, const double* sp, hipStream_t st) {
    hipLaunchKernelGGL(pd_grid_kernel, dim3((unsigned)((ndim * G + 255) / 256)), dim3(256), 0, st, grid, dims, ndim, G, D, mode, sp);
}

template <typename T>
void pd_mean_rows(const Geom& gr, const Geom& g, const double* acc, double W, const double* Fall, const int* dims, const double* grid, int ng,
                  int G, T* Phibar, hipStream_t st) {
    hipLaunchKernelGGL(pd_mean_rows_kernel<T>, dim3((unsigned)gr.Np), dim3(256), 0, st, acc, W, Fall, dims, grid, ng, G, pd_grid_rows(G), g.J,
                       g.Jp, g.Kp, Phibar);
}

template <typename T>
void pd_ice_weights(const Geom& g, const double* alpha, const double* Fall, int d, const double* grid_d, int G, T* R, hipStream_t st) {
    const int64_t rows = sample_w_rows(g.K);
    const int cols = sample_w_cols(G);
    const int64_t blocks = std::min<int64_t>((rows * cols + 255) / 256, 2048);
    hipLaunchKernelGGL(pd_ice_weights_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, alpha, Fall + (int64_t)d * g.Jp, grid_d, G, g.J, rows,
                       cols, R);
}

void pd_column(const Geom& g, double* Xt, int d, int save, double* keep, hipStream_t st) {
    hipLaunchKernelGGL(pd_column_kernel, dim3((unsigned)std::min<int64_t>((g.Np + 255) / 256, 1024)), dim3(256), 0, st, Xt, g.Dp, d, g.Np, save,
                       keep);
}

template void pd_sums<double>(const Geom&, const double*, const double*, const Scal*, const double*, const int*, int, double*, double*,
                              hipStream_t);
template void pd_sums<float>(const Geom&, const double*, const double*, const Scal*, const double*, const int*, int, double*, double*,
                             hipStream_t);
template void pd_mean_rows<double>(const Geom&, const Geom&, const double*, double, const double*, const int*, const double*, int, int, double*,
                                   hipStream_t);
template void pd_mean_rows<float>(const Geom&, const Geom&, const double*, double, const double*, const int*, const double*, int, int, float*,
                                  hipStream_t);
template void pd_ice_weights<double>(const Geom&, const double*, const double*, int, const double*, int, double*, hipStream_t);
template void pd_ice_weights<float>(const Geom&, const double*, const double*, int, const double*, int, float*, hipStream_t);
