// Input gradients of the predictive mean and std (scfgp_predict_grad; SCFGP/SCFGP.py:138-148 differentiated in Xs).
//   Phi = s [cos Z | sin Z], Z = X~ Fall: d phi_c_j / d z_j = -phi_s_j, d phi_s_j / d z_j = phi_c_j, so with alpha = [alpha_c | alpha_s]
//   and V = Phi B (B = Li^T Li, v = phi^T B phi = || Li phi ||^2):
//     d mu / d z_j  = phi_c_j alpha_s_j - phi_s_j alpha_c_j                      (Zbar_mu)
//     d v / d z_j   = 2 (phi_c_j V_s_j - phi_s_j V_c_j)                          (2 Zbar_v)
//     d mu / d x_d  = sum_j Fall[d][j] Zbar_mu_j,   d sigma / d x_d = kappa / sigma * sum_j Fall[d][j] Zbar_v_j   (sigma = sqrt(kappa (1 + v)))
//   The same Zbar = Phi_c o Phibar_s - Phi_s o Phibar_c form as gram.hip's xtz_kernel, here contracted over the features.
// Built on the MFMA traits of tile_engine.h; templated on the storage type T of Phi and V (fp64 MFMA in fp64 mode, exact fp32 in fp32 mode).
#include "kernels.h"
#include "tile_engine.h"

// FT (Jq x ldft, typed) = Fall^T on j < J, d < D; zero elsewhere (the ones row D of X~ carries the phase offsets: no x-gradient)
template <typename T>
__global__ void predgrad_ft_kernel(const double* __restrict__ Fall, int Jp, int J, int D, int Jq, int ldft, T* __restrict__ FT) {
    const int64_t total = (int64_t)Jq * ldft;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int j = (int)(e / ldft), d = (int)(e % ldft);
        FT[e] = (j < J && d < D) ? (T)Fall[(int64_t)d * Jp + j] : (T)0;
    }
}

// four consecutive elements p[0..3], those at or past `nvalid` zero; `al`: p is 16-byte aligned
__device__ __forceinline__ void load4(const float* __restrict__ p, int nvalid, bool al, double (&v)[4]) {
    if (nvalid >= 4 && al) {
        const v4f x = *reinterpret_cast<const v4f*>(p);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = x[e];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = e < nvalid ? (double)p[e] : 0.0;
    }
}
__device__ __forceinline__ void load4(const double* __restrict__ p, int nvalid, bool al, double (&v)[4]) {
    if (nvalid >= 4 && al) {
        const v2d x0 = *reinterpret_cast<const v2d*>(p), x1 = *reinterpret_cast<const v2d*>(p + 2);
        v[0] = x0[0]; v[1] = x0[1]; v[2] = x1[0]; v[3] = x1[1];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = e < nvalid ? p[e] : 0.0;
    }
}

// One wave: 16 TM rows x the NDT 16-wide column tiles [d0, d0 + 16 NDT) of the output, over all J features in steps of 16.  No LDS and no
// barriers: lane (i, q) = (lane % 16, lane / 16) stages features j0 + 4q .. j0 + 4q + 3 of its rows (one 16-byte load of each half of
// Phi, and of V) and forms Zbar in fp64 from them, rounded once to T; MFMA step e pairs k slot q with feature j0 + 4q + e in both operands.
// The B fragments FT[j][d0 + 16 tn + i] are re-read by every wave from L1 / L2 (FT is a few hundred KB at most).
template <typename T, int NDT, bool STD>
__global__ __launch_bounds__(256) void predgrad_zf_kernel(
    const T* __restrict__ Phi, const T* __restrict__ V, const double* __restrict__ alpha, const T* __restrict__ FT, int ldft, int d0,
    int J, int Kp, int D, int64_t N, const double* __restrict__ sd, const Scal* __restrict__ sc, double* __restrict__ dmu,
    double* __restrict__ dstd) {
    typedef MT<T, 16> M;
    constexpr int TM = sizeof(T) == 4 ? 2 : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * 16 * TM;
    const bool al_s = sizeof(T) == 4 ? (J & 3) == 0 : (J & 1) == 0;   // the sine half starts at column J
    typename M::acc_t am[TM][NDT], av[TM][NDT];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < NDT; ++tn)
#pragma unroll
            for (int r = 0; r < M::NACC; ++r) { am[tm][tn][r] = 0; av[tm][tn][r] = 0; }
    for (int j0 = 0; j0 < J; j0 += 16) {
        const int jl = j0 + 4 * q, nv = J - jl;                     // features jl .. jl + 3 of this lane; nv <= 0: none live
        double ac[4], as[4];
        load4(alpha + jl, nv, true, ac);
        load4(alpha + J + jl, nv, (J & 1) == 0, as);
        T b[4][NDT];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int tn = 0; tn < NDT; ++tn) b[e][tn] = FT[(int64_t)(jl + e) * ldft + d0 + tn * 16 + i];
        T zm[TM][4], zv[TM][4];
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
            const int64_t n = row0 + tm * 16 + i;
            double pc[4], ps[4];
            load4(Phi + n * Kp + jl, nv, true, pc);
            load4(Phi + n * Kp + J + jl, nv, al_s, ps);
#pragma unroll
            for (int e = 0; e < 4; ++e) zm[tm][e] = (T)(pc[e] * as[e] - ps[e] * ac[e]);
            if (STD) {
                double vc[4], vs[4];
                load4(V + n * Kp + jl, nv, true, vc);
                load4(V + n * Kp + J + jl, nv, al_s, vs);
#pragma unroll
                for (int e = 0; e < 4; ++e) zv[tm][e] = (T)(pc[e] * vs[e] - ps[e] * vc[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < NDT; ++tn) {
                    M::mfma(am[tm][tn], zm[tm][e], b[e][tn]);
                    if (STD) M::mfma(av[tm][tn], zv[tm][e], b[e][tn]);
                }
    }
    const double kappa = sc->kappa;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int r = 0; r < M::NACC; ++r) {
            const int64_t n = row0 + tm * 16 + M::crow(lane, r);
            if (n >= N) continue;
            const double ks = STD ? kappa / sd[n] : 0.0;
#pragma unroll
            for (int tn = 0; tn < NDT; ++tn) {
                const int d = d0 + tn * 16 + i;
                if (d >= D) continue;
                dmu[n * D + d] = (double)am[tm][tn][r];
                if (STD) dstd[n * D + d] = ks * (double)av[tm][tn][r];
            }
        }
}

// 16-wide column tiles of the next launch for `rem` tiles left: 8, 4, 2 or 1 (a launch may round up; FT's zero columns fill it)
static int predgrad_tiles(int rem) { return rem > 4 ? 8 : (rem > 2 ? 4 : rem); }
int predgrad_ft_cols(int D) {
    int w = 0;
    for (int rem = (D + 15) / 16; rem > 0;) { const int p = predgrad_tiles(rem); w += p; rem -= p < rem ? p : rem; }
    return 16 * w;
}

template <typename T>
void predgrad_operand(const Geom& g, const double* Fall, T* FT, hipStream_t st) {
    hipLaunchKernelGGL(predgrad_ft_kernel<T>, dim3(512), dim3(256), 0, st, Fall, g.Jp, g.J, g.D, (int)round_up(g.J, 16),
                       predgrad_ft_cols(g.D), FT);
}

template <typename T, bool STD>
static void predgrad_launch(const Geom& g, const T* Phi, const T* V, const double* alpha, const T* FT, const double* sd, const Scal* sc,
                            double* dmu, double* dstd, hipStream_t st) {
    constexpr int ROWS = 4 * 16 * (sizeof(T) == 4 ? 2 : 1);            // rows per workgroup: Np (a multiple of 256) is covered exactly
    const dim3 grid((unsigned)(g.Np / ROWS));
    const int ldft = predgrad_ft_cols(g.D);
    for (int rem = (g.D + 15) / 16, d0 = 0; rem > 0;) {
        const int p = predgrad_tiles(rem);
        const auto args = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, Phi, V, alpha, FT, ldft, d0, g.J, g.Kp, g.D, g.N, sd, sc, dmu, dstd);
        };
        if (p == 8) args(predgrad_zf_kernel<T, 8, STD>);
        else if (p == 4) args(predgrad_zf_kernel<T, 4, STD>);
        else if (p == 2) args(predgrad_zf_kernel<T, 2, STD>);
        else args(predgrad_zf_kernel<T, 1, STD>);
        d0 += 16 * p; rem -= p < rem ? p : rem;
    }
}

template <typename T>
void predgrad(const Geom& g, const T* Phi, const T* V, const double* alpha, const T* FT, const double* sd, const Scal* sc, double* dmu,
              double* dstd, hipStream_t st) {
    if (dstd) predgrad_launch<T, true>(g, Phi, V, alpha, FT, sd, sc, dmu, dstd, st);
    else predgrad_launch<T, false>(g, Phi, V, alpha, FT, sd, sc, dmu, dstd, st);
}

template void predgrad_operand<double>(const Geom&, const double*, double*, hipStream_t);
template void predgrad_operand<float>(const Geom&, const double*, float*, hipStream_t);
template void predgrad<double>(const Geom&, const double*, const double*, const double*, const double*, const double*, const Scal*,
                               double*, double*, hipStream_t);
template void predgrad<float>(const Geom&, const float*, const float*, const double*, const float*, const double*, const Scal*,
                              double*, double*, hipStream_t);
