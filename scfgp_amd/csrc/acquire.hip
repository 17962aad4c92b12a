// Acquisition functions over a pool (scfgp_acquire; definitions, guarantees and errors in include/scfgp_hip.h).  With u = sgn mu*(x),
// sigma the latent (sqrt(kappa v)) or the predictive (sqrt(kappa (1 + v))) standard deviation, Phi / phi the standard normal CDF / PDF,
// lam = phi / Phi and h(g) = g Phi(g) + phi(g):
//     UCB    u + beta sigma                                         PI     Phi(g),            g = (u - sgn best - xi) / sigma
//     EI     sigma h(g)                                             LOGEI  log sigma + log h(g)
//     MES    (1 / n*) sum_s [ g_s lam(g_s) / 2 - log Phi(g_s) ],    g_s = (sgn f*_s - u) / sigma
// and the partials a_u = d acq / d u, a_s = d acq / d sigma that the gradient combine chains with predgrad's d mu / d x, d sigma / d x.
// Everything here is fp64 in every compute mode: mu and v are the fp64 sums of the chunk's partials, in rowstats_kernel<1>'s order.
//
// Tail forms (tests/acquire_ref.py restates them in numpy and pins them to 50-digit arithmetic).  With t = -g / sqrt 2 and erfcx the
// scaled complementary error function, Phi(g) = erfcx(t) exp(-g^2 / 2) / 2 for g < 0, so
//     log Phi = log(erfcx(t) / 2) - g^2 / 2,   lam = sqrt(2 / pi) / erfcx(t)                              (g < 0)
//     log Phi = log1p(-c),  c = erfcx(-t) exp(-g^2 / 2) / 2 = erfc(g / sqrt 2) / 2,   lam = phi / (1 - c)    (g >= 0)
//     h = phi r,  r = 1 - sqrt(pi) t erfcx(t)  (-50 <= g <= -1);  r = g^-2 (1 - 3 g^-2 + 15 g^-4 - 105 g^-6 + 945 g^-8)  (g < -50)
//     log h = -g^2 / 2 - log(2 pi) / 2 + log r,   Phi / h = sqrt(pi / 2) erfcx(t) / r,   phi / h = 1 / r       (g <= -1)
// r cancels to relative eps g^2 in its first form (2.8e-13 at -50, where the series' first dropped term is 1.1e-13) and so do the
// two g^2 / 2 of a MES term at very negative g (absolute eps g^2 on a value of order log |g|).
#include "kernels.h"
#include "argmax.h"
#include "acquire_math.h"                                         // phi, Phi, tail_r (shared with kg.hip); contraction off from here on

namespace {

// the acquisition value of kinds 0 - 3 and its partials in u and sigma
template <int KIND>
__device__ __forceinline__ void acquire_value(double u, double s, double p0, double p1, double& acq, double& au, double& as) {
    if (KIND == 0) { acq = u + p0 * s; au = 1.0; as = p0; return; }
    const double g = (u - p0 - p1) / s;                         // p0 = sgn best, p1 = xi
    if (KIND == 1) {
        const double ph = norm_pdf(g);
        acq = norm_cdf(g); au = ph / s; as = -g * ph / s;
        return;
    }
    if (g > -1.0) {
        const double P = norm_cdf(g), ph = norm_pdf(g), h = g * P + ph;
        if (KIND == 2) { acq = s * h; au = P; as = ph; }
        else { acq = log(s) + log(h); au = P / (s * h); as = ph / (s * h); }
    } else {
        const double e = erfcx(-g * INV_SQRT2), r = tail_r(g, e);
        if (KIND == 2) {
            const double ph = norm_pdf(g);
            acq = s * (ph * r); au = norm_cdf(g); as = ph;
        } else {
            acq = log(s) + (-0.5 * g * g - HALF_LOG_2PI + log(r));
            au = SQRT_PI_OVER_2 * e / r / s; as = 1.0 / r / s;
        }
    }
}

}  // namespace

// One thread per row: mu, v from the chunk's partials exactly as rowstats_kernel<1> sums them (so mu and, with noise, sd have
// scfgp_predict's bits), sigma, the acquisition value and its two partials.  Kinds 0 - 3.
template <int KIND>
__global__ __launch_bounds__(256) void acquire_rows_kernel(const double* __restrict__ mupart, const double* __restrict__ vpart, int njt,
                                                           const Scal* __restrict__ sc, int64_t N, int64_t Np, int noise, double sgn, double p0,
                                                           double p1, double* __restrict__ mu_o, double* __restrict__ sd_o,
                                                           double* __restrict__ acq_o, double* __restrict__ au_o, double* __restrict__ as_o) {
    const double kappa = sc->kappa;
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < N; n += (int64_t)gridDim.x * 256) {
        double v = 0, mu = 0;
        for (int t = 0; t < njt; ++t) { v += vpart[(int64_t)t * Np + n]; mu += mupart[(int64_t)t * Np + n]; }
        const double d = noise ? kappa * (v + 1.0) : kappa * v;
        const double s = sqrt(d);
        mu_o[n] = mu; sd_o[n] = s;
        if constexpr (KIND < 4) {
            double acq, au, as;
            acquire_value<KIND>(sgn * mu, s, p0, p1, acq, au, as);
            acq_o[n] = acq; au_o[n] = au; as_o[n] = as;
        }
    }
}

// MES.  ACQ_MES_LANES lanes share a row: lane l takes the samples l, l + 16, l + 32, ... in that order, then the lanes' partial sums
// meet in a butterfly of fixed shape -- the order of the sum depends on n* alone.  f* sits in LDS (the lanes of a row read consecutive
// entries, the four rows of a wave the same ones).  A 32768-row chunk is 2048 workgroups of 4 waves.
constexpr int ACQ_MES_LANES = 16;
constexpr int ACQ_MES_ROWS = 256 / ACQ_MES_LANES;
__global__ __launch_bounds__(256) void acquire_mes_kernel(const double* __restrict__ mu_i, const double* __restrict__ sd_i,
                                                          const double* __restrict__ fstar, int nstar, double sgn, int64_t N,
                                                          double* __restrict__ acq_o, double* __restrict__ au_o, double* __restrict__ as_o) {
    __shared__ double s_f[1024];
    for (int s = threadIdx.x; s < nstar; s += 256) s_f[s] = sgn * fstar[s];
    __syncthreads();
    const int l = threadIdx.x & (ACQ_MES_LANES - 1);
    const int64_t n = (int64_t)blockIdx.x * ACQ_MES_ROWS + (threadIdx.x >> 4);
    const bool live = n < N;
    const double u = live ? sgn * mu_i[n] : 0.0, sd = live ? sd_i[n] : 1.0;
    double sm = 0.0, sq = 0.0, sgq = 0.0;
    for (int s = l; s < nstar; s += ACQ_MES_LANES) {
        const double g = (s_f[s] - u) / sd;
        const double e = erfcx(fabs(g) * INV_SQRT2), hg2 = 0.5 * g * g;
        double logP, lam;
        if (g < 0.0) { logP = log(0.5 * e) - hg2; lam = SQRT_2_OVER_PI / e; }
        else {
            const double ex = exp(-hg2), c = 0.5 * e * ex;
            logP = log1p(-c); lam = INV_SQRT_2PI * ex / (1.0 - c);
        }
        const double q = 0.5 * lam * (1.0 + g * (g + lam));
        sm += 0.5 * g * lam - logP; sq += q; sgq += g * q;
    }
#pragma unroll
    for (int off = ACQ_MES_LANES / 2; off >= 1; off >>= 1) {
        sm += __shfl_xor(sm, off); sq += __shfl_xor(sq, off); sgq += __shfl_xor(sgq, off);
    }
    if (live && l == 0) {
        const double ns = (double)nstar;
        acq_o[n] = sm / ns; au_o[n] = sq / ns / sd; as_o[n] = sgq / ns / sd;
    }
}

// One record per workgroup of 256 rows: the best eligible row of the chunk's acq by argmax_beats (always maximising), lanes by
// shuffles, waves through LDS.  flag: an eligible row whose mu, sigma or value is not finite, or whose sigma is 0.
__global__ __launch_bounds__(256) void acquire_argmax_kernel(const double* __restrict__ acq, const double* __restrict__ mu,
                                                             const double* __restrict__ sd, const double* __restrict__ w, int64_t N,
                                                             double* __restrict__ pv, long long* __restrict__ pt, int* __restrict__ flag) {
    __shared__ double sv[4];
    __shared__ long long sl[4];
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double bv = 0.0;
    long long bt = -1;
    if (n < N && (!w || w[n] > 0.0)) {
        const double a = acq[n], s = sd[n];
        if (!isfinite(a) || !isfinite(mu[n]) || !isfinite(s) || s == 0.0) *flag = 1;
        bv = a; bt = n;
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double ov = __shfl_xor(bv, off);
        const long long ot = __shfl_xor(bt, off);
        if (argmax_beats(ov, ot, bv, bt, false)) { bv = ov; bt = ot; }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { sv[wave] = bv; sl[wave] = bt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = sv[0];
        long long t = sl[0];
        for (int k = 1; k < 4; ++k)
            if (argmax_beats(sv[k], sl[k], v, t, false)) { v = sv[k]; t = sl[k]; }
        pv[blockIdx.x] = v; pt[blockIdx.x] = t;
    }
}

// the chunk's records, in block order, into the running best (value, row index in the call's Xs) that stays on the device
__global__ void acquire_merge_kernel(const double* __restrict__ pv, const long long* __restrict__ pt, int nblocks, int64_t t0, int first,
                                     double* __restrict__ bestv, long long* __restrict__ bestt) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double v = first ? 0.0 : bestv[0];
    long long t = first ? -1 : bestt[0];
    for (int b = 0; b < nblocks; ++b) {
        const long long cl = pt[b], ct = cl < 0 ? -1 : t0 + cl;
        if (argmax_beats(pv[b], ct, v, t, false)) { v = pv[b]; t = ct; }
    }
    bestv[0] = v; bestt[0] = t;
}

// grad[n][d] = sgn a_u[n] dmu[n][d] + a_s[n] dsd[n][d], in place over dmu
__global__ __launch_bounds__(256) void acquire_grad_kernel(const double* __restrict__ au, const double* __restrict__ as,
                                                           const double* __restrict__ dsd, int64_t total, int D, double sgn,
                                                           double* __restrict__ dmu) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t n = e / D;
        dmu[e] = sgn * au[n] * dmu[e] + as[n] * dsd[e];
    }
}

void acquire_rows(const Geom& g, int njt, const double* mupart, const double* vpart, const Scal* sc, const AcquireSpec& a, const AcquireBufs& b,
                  hipStream_t st) {
    const dim3 grid((unsigned)(g.Np / 256));                          // Np: a multiple of 256
    const double sgn = a.minimize ? -1.0 : 1.0;
    const auto launch = [&](auto kernel, double p0, double p1) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, mupart, vpart, njt, sc, g.N, g.Np, a.noise, sgn, p0, p1, b.mu, b.sd, b.acq, b.au,
                           b.as);
    };
    switch (a.kind) {
    case 0: launch(acquire_rows_kernel<0>, a.par[0], 0.0); break;
    case 1: launch(acquire_rows_kernel<1>, sgn * a.par[0], a.par[1]); break;
    case 2: launch(acquire_rows_kernel<2>, sgn * a.par[0], a.par[1]); break;
    case 3: launch(acquire_rows_kernel<3>, sgn * a.par[0], a.par[1]); break;
    default:
        launch(acquire_rows_kernel<4>, 0.0, 0.0);
        hipLaunchKernelGGL(acquire_mes_kernel, dim3((unsigned)((g.N + ACQ_MES_ROWS - 1) / ACQ_MES_ROWS)), dim3(256), 0, st, b.mu, b.sd,
                           a.fstar, a.nstar, sgn, g.N, b.acq, b.au, b.as);
    }
}

void acquire_argmax(const Geom& g, const double* w, int64_t t0, int first, const AcquireBufs& b, hipStream_t st) {
    const int nblocks = (int)acquire_blocks(g.Np);
    hipLaunchKernelGGL(acquire_argmax_kernel, dim3(nblocks), dim3(256), 0, st, b.acq, b.mu, b.sd, w, g.N, b.pv, b.pt, b.flag);
    hipLaunchKernelGGL(acquire_merge_kernel, dim3(1), dim3(64), 0, st, b.pv, b.pt, nblocks, t0, first, b.bestv, b.bestt);
}

void acquire_grad(const Geom& g, const AcquireBufs& b, int minimize, const double* dsd, double* grad, hipStream_t st) {
    hipLaunchKernelGGL(acquire_grad_kernel, dim3(2048), dim3(256), 0, st, b.au, b.as, dsd, g.N * g.D, g.D, minimize ? -1.0 : 1.0, grad);
}
