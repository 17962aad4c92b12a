// Posterior covariance of the input gradient (scfgp_predict_gradcov; derivation in include/scfgp_hip.h and DESIGN 4.18).
//   grad f(x) = J(x)^T w with w ~ N(alpha, kappa A^-1), so Cov[grad f(x_t)] = kappa J_t^T A^-1 J_t.  Every phase is z = x l_F [I | r_F^T] +
//   offset, so J_t^T = P Psi_t with q = min(D, S) directions:
//     Psi_t (q x K): row i = phi'_t o (Q[:, i] ; Q[:, i]),  phi' = (-phi_s | phi_c),  Fall[d][j] = sum_i P[d][i] Q[j][i]
//     dense  (D <= S): Q[j][i] = Fall[i][j], P = I;       latent (D > S): Q = [I_S | r_F^T]^T, P = l_F
//     C'_t = Psi_t Li^T (apply_c),  H_t = C'_t C'_t^T (q x q),  Sigma_t = kappa P H_t P^T
// The q derivative rows of a point are consecutive rows of the chunk (row t q + i), so a point is a "block" of b = q rows in the sense
// of loo.hip and the Gram part of gradcov_block_kernel is loo_block_kernel's (block_gram.h): groups of gs = (64 / q) q rows, the tiles
// that meet a point's diagonal block, the waves' tiles added into the LDS image in a fixed order.  An entry of H_t therefore has one
// summation order whatever the group, the chunk or the call.
#include "kernels.h"
#include "block_gram.h"

constexpr int GC_LD = BLOCK_GRAM_LD;            // doubles per row of the LDS image of H
constexpr int GC_TD = 32;                       // columns of Sigma per pass of the expansion
constexpr int GC_WLD = GC_TD + 1;

// Qt (q x Jp, typed): row i = Q[:, i]; columns j >= J zero
template <typename T>
__global__ void gradcov_q_kernel(const double* __restrict__ params, const double* __restrict__ Fall, int D, int S, int J, int Jp, int q,
                                 int latent, T* __restrict__ Qt) {
    const int total = q * Jp;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
        const int i = e / Jp, j = e % Jp;
        double v = 0.0;
        if (j < J) {
            if (!latent) v = Fall[(int64_t)i * Jp + j];
            else v = j < S ? (i == j ? 1.0 : 0.0) : params[3 + (int64_t)D * S + (int64_t)(j - S) * S + i];
        }
        Qt[e] = (T)v;
    }
}

// Psi (Np x Kp, typed): row r = t q + i < nrows is (-Phi_s[t][j] Q[j][i] | Phi_c[t][j] Q[j][i]), the product in fp64 rounded once; the
// padding columns and the rows from nrows on are zero.  One workgroup per row.
template <typename T>
__global__ __launch_bounds__(256) void gradfeat_kernel(const T* __restrict__ Phi, const T* __restrict__ Qt, int J, int Jp, int Kp, int q,
                                                       int64_t nrows, T* __restrict__ Psi) {
    const int64_t r = blockIdx.x;
    T* out = Psi + r * Kp;
    if (r >= nrows) {
        for (int c = threadIdx.x; c < Kp; c += 256) out[c] = (T)0;
        return;
    }
    const int64_t t = r / q;
    const int i = (int)(r - t * q);
    const T* ph = Phi + t * Kp;
    const T* qi = Qt + (int64_t)i * Jp;
    for (int c = threadIdx.x; c < Kp; c += 256) {
        double v = 0.0;
        if (c < J) v = -(double)ph[J + c] * (double)qi[c];
        else if (c < 2 * J) v = (double)ph[c - J] * (double)qi[c - J];
        out[c] = (T)v;
    }
}

__global__ void gradcov_ones_kernel(double* __restrict__ x, int64_t n) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) x[e] = 1.0;
}

// One workgroup of 4 waves per group of gs rows of C' = Psi Li^T (ld Kp): the points p0 .. of the chunk, q rows each.  P: l_F (D x q, ld
// q) or NULL for P = I (then D == q); gfac: the X scaler's factors g_t (n x D) or NULL; m: the (already chained) mean gradients (n x D)
// and wgt (n, or NULL for all 1) feed the records rec (n x D x D, lower triangle only) = w_t (m_t m_t^T + Sigma_t).  dvar (n x D), dcov
// (n x D x D) and rec may each be NULL.  Every entry of the lower triangle is computed once and mirrored.
template <typename T>
__global__ __launch_bounds__(256) void gradcov_block_kernel(const T* __restrict__ C, int Kp, int64_t nrows, int q, int gs, int D,
                                                            const double* __restrict__ P, const Scal* __restrict__ sc,
                                                            const double* __restrict__ gfac, const double* __restrict__ m,
                                                            const double* __restrict__ wgt, double* __restrict__ dvar,
                                                            double* __restrict__ dcov, double* __restrict__ rec) {
    __shared__ double Hs[64 * GC_LD];
    __shared__ double Ws[64 * GC_WLD];
    const int tid = threadIdx.x;
    const int64_t g0 = (int64_t)blockIdx.x * gs;                 // first row of the group (chunk-local)
    const int live = (int)(nrows - g0 < gs ? nrows - g0 : gs);   // live rows of the group: whole points, >= q

    block_gram<T>(C, Kp, g0, live, q, Hs);

    // ---- the tail, fp64: Sigma = kappa P H P^T of every point of the group, entries (d, e <= d); H is read from its lower triangle ----
    const double kappa = sc->kappa;
    const int64_t p0 = g0 / q;
    const int npts = live / q;
    const bool full = dcov != nullptr || rec != nullptr;         // else the diagonal only
    const int64_t DD = (int64_t)D * D;
    auto emit = [&](int64_t t, int d, int e, double h) {
        double v = kappa * h;
        if (gfac) v *= gfac[t * D + d] * gfac[t * D + e];
        if (d == e && dvar) dvar[t * D + d] = v;
        if (dcov) { dcov[t * DD + (int64_t)d * D + e] = v; dcov[t * DD + (int64_t)e * D + d] = v; }
        if (rec) rec[t * DD + (int64_t)d * D + e] = (wgt ? wgt[t] : 1.0) * (m[t * D + d] * m[t * D + e] + v);
    };
    if (!P) {                                                     // dense form: Sigma = kappa H (D == q)
        const int qq = q * q;
        for (int x = tid; x < npts * qq; x += 256) {
            const int p = x / qq, r = x - p * qq, d = r / q, e = r - d * q;
            if (e > d || (!full && e != d)) continue;
            emit(p0 + p, d, e, Hs[(p * q + d) * GC_LD + p * q + e]);
        }
        return;
    }
    for (int p = 0; p < npts; ++p) {                              // latent form: columns [e0, e0 + GC_TD) of W = H P^T, then P W below them
        const int o = p * q;
        const int64_t t = p0 + p;
        for (int e0 = 0; e0 < D; e0 += GC_TD) {
            const int ne = D - e0 < GC_TD ? D - e0 : GC_TD;
            for (int x = tid; x < q * ne; x += 256) {
                const int a = x / ne, e = x - a * ne;
                const double* pe = P + (int64_t)(e0 + e) * q;
                double s = 0.0;
                for (int b = 0; b < q; ++b) s += (a >= b ? Hs[(o + a) * GC_LD + o + b] : Hs[(o + b) * GC_LD + o + a]) * pe[b];
                Ws[a * GC_WLD + e] = s;
            }
            __syncthreads();
            const int nx = full ? (D - e0) * ne : ne;
            for (int x = tid; x < nx; x += 256) {
                const int dd = full ? x / ne : x, e = full ? x - dd * ne : x, d = e0 + dd;
                if (e0 + e > d) continue;
                const double* pd = P + (int64_t)d * q;
                double s = 0.0;
                for (int a = 0; a < q; ++a) s += pd[a] * Ws[a * GC_WLD + e];
                emit(t, d, e0 + e, s);
            }
            __syncthreads();
        }
    }
}

// acc (D x D) += the records of n points in point order, one lane per entry of the lower triangle
__global__ __launch_bounds__(256) void gradcov_reduce_kernel(const double* __restrict__ rec, int64_t n, int D, double* __restrict__ acc) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int64_t DD = (int64_t)D * D;
    if (x >= DD) return;
    const int d = x / D, e = x - d * D;
    if (e > d) return;
    double a = acc[x];
    int64_t t = 0;
    for (; t + 8 <= n; t += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = rec[(t + u) * DD + x];
#pragma unroll
        for (int u = 0; u < 8; ++u) a += v[u];
    }
    for (; t < n; ++t) a += rec[t * DD + x];
    acc[x] = a;
}

template <typename T>
void gradcov_operand(const Geom& g, const double* params, const double* Fall, T* Qt, hipStream_t st) {
    const int q = g.D < g.S ? g.D : g.S;
    hipLaunchKernelGGL(gradcov_q_kernel<T>, dim3(64), dim3(256), 0, st, params, Fall, g.D, g.S, g.J, g.Jp, q, g.D > g.S ? 1 : 0, Qt);
}

template <typename T>
void gradfeat(const Geom& gr, const Geom& g, const T* Phi, const T* Qt, T* Psi, hipStream_t st) {
    const int q = g.D < g.S ? g.D : g.S;
    hipLaunchKernelGGL(gradfeat_kernel<T>, dim3((unsigned)gr.Np), dim3(256), 0, st, Phi, Qt, g.J, g.Jp, g.Kp, q, gr.N, Psi);
}

void gradcov_ones(double* x, int64_t n, hipStream_t st) {
    hipLaunchKernelGGL(gradcov_ones_kernel, dim3((unsigned)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048)), dim3(256), 0, st, x, n);
}

template <typename T>
void gradcov_blocks(const Geom& gr, const Geom& g, const T* C, const double* params, const Scal* sc, const double* gfac, const double* m,
                    const double* wgt, double* dvar, double* dcov, double* rec, hipStream_t st) {
    const int q = g.D < g.S ? g.D : g.S, gs = 64 / q * q;
    const int64_t ngroups = (gr.N + gs - 1) / gs;
    const double* P = g.D > g.S ? params + 3 : nullptr;          // l_F (D x S row-major) heads the parameter vector behind its 3 scalars
    hipLaunchKernelGGL(gradcov_block_kernel<T>, dim3((unsigned)ngroups), dim3(256), 0, st, C, g.Kp, gr.N, q, gs, g.D, P, sc, gfac, m, wgt,
                       dvar, dcov, rec);
}

void gradcov_reduce(const double* rec, int64_t n, int D, double* acc, hipStream_t st) {
    hipLaunchKernelGGL(gradcov_reduce_kernel, dim3((unsigned)(((int64_t)D * D + 255) / 256)), dim3(256), 0, st, rec, n, D, acc);
}

template void gradcov_operand<double>(const Geom&, const double*, const double*, double*, hipStream_t);
template void gradcov_operand<float>(const Geom&, const double*, const double*, float*, hipStream_t);
template void gradfeat<double>(const Geom&, const Geom&, const double*, const double*, double*, hipStream_t);
template void gradfeat<float>(const Geom&, const Geom&, const float*, const float*, float*, hipStream_t);
template void gradcov_blocks<double>(const Geom&, const Geom&, const double*, const double*, const Scal*, const double*, const double*,
                                     const double*, double*, double*, double*, hipStream_t);
template void gradcov_blocks<float>(const Geom&, const Geom&, const float*, const double*, const Scal*, const double*, const double*,
                                    const double*, double*, double*, double*, hipStream_t);
