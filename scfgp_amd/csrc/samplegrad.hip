// Values and input gradients of posterior sample functions, one sample per row (scfgp_sample_grad).
//   f_s(x) = phi(x)^T w_s with Phi = s [cos Z | sin Z], Z = X~ Fall and w_s = [w_c | w_s] in alpha's layout, so (predgrad.hip, with the
//   row's own weight vector in alpha's place)
//     d f / d z_j = phi_c_j w_s_j - phi_s_j w_c_j                                   (Zbar)
//     d f / d x_d = sum_j Fall[d][j] Zbar_j
//     f           = sum_j phi_c_j w_c_j + phi_s_j w_s_j
//   Row n is evaluated under sample sidx[n]; its weights come from WT, the fp64 transpose of W with one contiguous row per sample.
// The gradient is predgrad_zf_kernel<T, NDT, false>'s arithmetic: Zbar in fp64, rounded once to T, contracted with FT = Fall^T by the
// same MFMA steps in the same order -- with every row under the weights alpha the two kernels write the same bits.
#include "kernels.h"
#include "tile_engine.h"

// WT (nsamp x ldw fp64) = W^T (W: K x nsamp row-major, the host layout), columns k >= K zero
__global__ void samplegrad_wt_kernel(const double* __restrict__ W, int K, int nsamp, int ldw, double* __restrict__ WT) {
    const int64_t total = (int64_t)nsamp * ldw;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int s = (int)(e / ldw), k = (int)(e % ldw);
        WT[e] = k < K ? W[(int64_t)k * nsamp + s] : 0.0;
    }
}

// four consecutive elements p[0..3], those at or past `nvalid` zero; `al`: p is 16-byte aligned (as predgrad.hip's loads)
__device__ __forceinline__ void sg_load4(const float* __restrict__ p, int nvalid, bool al, double (&v)[4]) {
    if (nvalid >= 4 && al) {
        const v4f x = *reinterpret_cast<const v4f*>(p);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = x[e];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = e < nvalid ? (double)p[e] : 0.0;
    }
}
__device__ __forceinline__ void sg_load4(const double* __restrict__ p, int nvalid, bool al, double (&v)[4]) {
    if (nvalid >= 4 && al) {
        const v2d x0 = *reinterpret_cast<const v2d*>(p), x1 = *reinterpret_cast<const v2d*>(p + 2);
        v[0] = x0[0]; v[1] = x0[1]; v[2] = x1[0]; v[3] = x1[1];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = e < nvalid ? p[e] : 0.0;
    }
}

// One wave: 16 TM rows x the NDT 16-wide column tiles [d0, d0 + 16 NDT) of the gradient, over all J features in steps of 16; no LDS and
// no barriers.  Lane (i, q) = (lane % 16, lane / 16) stages features j0 + 4q .. j0 + 4q + 3 of its rows: one 16-byte load of each half
// of Phi and two 16-byte loads of each half of the row's weight vector (L2 hits where many rows share few samples).  sidx (Np doubles,
// exact integers in [0, nsamp); NULL: sample (t0 + n) % nsamp) names the sample of chunk row n; the rows n >= N of the last workgroup
// read sample 0 or their modulus, both valid, and write nothing.
// VAL (the launch with d0 = 0 only): f in fp64, each lane's features in ascending order by fused multiply-adds (cosine term, then sine
// term, per feature), then (q0 + q1) + (q2 + q3) over the four lanes of a row -- an order that depends on J alone.
template <typename T, int NDT, bool VAL>
__global__ __launch_bounds__(256) void samplegrad_zf_kernel(
    const T* __restrict__ Phi, const double* __restrict__ WT, int ldw, const double* __restrict__ sidx, int64_t t0, int nsamp,
    const T* __restrict__ FT, int ldft, int d0, int J, int Kp, int D, int64_t N, double* __restrict__ val, double* __restrict__ grad) {
    typedef MT<T, 16> M;
    constexpr int TM = sizeof(T) == 4 ? 2 : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * 16 * TM;
    const bool al_s = sizeof(T) == 4 ? (J & 3) == 0 : (J & 1) == 0;   // the sine half of Phi starts at column J
    const bool al_w = (J & 1) == 0;                                   // the sine half of a weight row (fp64) too
    const double* w[TM];
    double f[TM];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
        const int64_t n = row0 + tm * 16 + i;
        const int s = sidx ? (int)sidx[n] : (int)((t0 + n) % nsamp);
        w[tm] = WT + (int64_t)s * ldw;
        f[tm] = 0.0;
    }
    typename M::acc_t am[TM][NDT];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < NDT; ++tn)
#pragma unroll
            for (int r = 0; r < M::NACC; ++r) am[tm][tn][r] = 0;
    for (int j0 = 0; j0 < J; j0 += 16) {
        const int jl = j0 + 4 * q, nv = J - jl;                     // features jl .. jl + 3 of this lane; nv <= 0: none live
        T b[4][NDT];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int tn = 0; tn < NDT; ++tn) b[e][tn] = FT[(int64_t)(jl + e) * ldft + d0 + tn * 16 + i];
        T zm[TM][4];
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
            const int64_t n = row0 + tm * 16 + i;
            double ac[4], as[4], pc[4], ps[4];
            sg_load4(w[tm] + jl, nv, true, ac);
            sg_load4(w[tm] + J + jl, nv, al_w, as);
            sg_load4(Phi + n * Kp + jl, nv, true, pc);
            sg_load4(Phi + n * Kp + J + jl, nv, al_s, ps);
#pragma unroll
            for (int e = 0; e < 4; ++e) zm[tm][e] = (T)(pc[e] * as[e] - ps[e] * ac[e]);
            if (VAL) {
#pragma unroll
                for (int e = 0; e < 4; ++e) f[tm] = __builtin_fma(ps[e], as[e], __builtin_fma(pc[e], ac[e], f[tm]));
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < NDT; ++tn) M::mfma(am[tm][tn], zm[tm][e], b[e][tn]);
    }
    if (VAL) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
            double v = f[tm];
            v += __shfl_xor(v, 16);                                 // q0 + q1 | q2 + q3 (commutative: both lanes of a pair hold the same bits)
            v += __shfl_xor(v, 32);
            const int64_t n = row0 + tm * 16 + i;
            if (q == 0 && n < N) val[n] = v;
        }
    }
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int r = 0; r < M::NACC; ++r) {
            const int64_t n = row0 + tm * 16 + M::crow(lane, r);
            if (n >= N) continue;
#pragma unroll
            for (int tn = 0; tn < NDT; ++tn) {
                const int d = d0 + tn * 16 + i;
                if (d >= D) continue;
                grad[n * D + d] = (double)am[tm][tn][r];
            }
        }
}

int samplegrad_w_ld(int K) { return (int)round_up(K, 16); }

void samplegrad_weights(const double* W, int K, int nsamp, double* WT, hipStream_t st) {
    hipLaunchKernelGGL(samplegrad_wt_kernel, dim3(256), dim3(256), 0, st, W, K, nsamp, samplegrad_w_ld(K), WT);
}

// predgrad.hip's plan of the launches over D: 8, 4, 2 or 1 column tiles (a launch may round up; FT's zero columns fill it), so that
// predgrad_ft_cols(D) is this plan's width too
static int samplegrad_tiles(int rem) { return rem > 4 ? 8 : (rem > 2 ? 4 : rem); }

template <typename T>
void samplegrad(const Geom& g, const T* Phi, const double* WT, const double* sidx, int64_t t0, int nsamp, const T* FT, double* val,
                double* grad, hipStream_t st) {
    constexpr int ROWS = 4 * 16 * (sizeof(T) == 4 ? 2 : 1);            // rows per workgroup: Np (a multiple of 256) is covered exactly
    const dim3 grid((unsigned)(g.Np / ROWS));
    const int ldft = predgrad_ft_cols(g.D), ldw = samplegrad_w_ld(g.K);
    for (int rem = (g.D + 15) / 16, d0 = 0; rem > 0;) {
        const int p = samplegrad_tiles(rem);
        const auto args = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, Phi, WT, ldw, sidx, t0, nsamp, FT, ldft, d0, g.J, g.Kp, g.D, g.N, val, grad);
        };
        const auto pick = [&](auto ndt) {
            constexpr int NDT = decltype(ndt)::value;
            if (d0 == 0) args(samplegrad_zf_kernel<T, NDT, true>);
            else args(samplegrad_zf_kernel<T, NDT, false>);
        };
        if (p == 8) pick(std::integral_constant<int, 8>());
        else if (p == 4) pick(std::integral_constant<int, 4>());
        else if (p == 2) pick(std::integral_constant<int, 2>());
        else pick(std::integral_constant<int, 1>());
        d0 += 16 * p; rem -= p < rem ? p : rem;
    }
}

template void samplegrad<double>(const Geom&, const double*, const double*, const double*, int64_t, int, const double*, double*, double*,
                                 hipStream_t);
template void samplegrad<float>(const Geom&, const float*, const double*, const double*, int64_t, int, const float*, double*, double*,
                                hipStream_t);
