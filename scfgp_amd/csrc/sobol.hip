// Closed-form Sobol indices under a product measure (scfgp_sobol; derivation in include/scfgp_hip.h and DESIGN 4.21).
//   f(x) = Re sum_j a_j e^{i z_j(x)},  z_j = sum_e x_e Om[e][j] + b_j,  a_j = s (w_j - i w_{J+j}),  mu = prod_d mu_d with characteristic
//   functions psi_d.  Every variance is 1/2 Re sum_{j,k} [a_j a_k C+_u(j,k) + a_j conj(a_k) C-_u(j,k)] with centred coefficients
//     C+-_all       = e^{i(b_j +- b_k)} prod_e psi_e(Om[e][j] +- Om[e][k])                                        - E_j E_k^(+-)
//     C+-_main(d)   = E_j^{-d} (E_k^{-d})^(+-) psi_d(Om[d][j] +- Om[d][k])                                        - E_j E_k^(+-)
//     C+-_closed(d) = e^{i(b_j +- b_k)} psi1[d][j] (psi1[d][k])^(+-) prod_{e != d} psi_e(Om[e][j] +- Om[e][k])   - E_j E_k^(+-)
//   ((+-): conjugated with the minus sign).  Only j <= k is formed, with weight 2 off the diagonal.
// Launch plan: sobol_tables (one lane per j) writes psi1, E, E^{-d}, e^{i b} and phibar; sobol_weights the a_j of every column;
// sobol_pairs (the hot path) runs one workgroup per (unit, block of 32 columns, group of <= 16 inputs), a unit being a block of 8 j and
// a run of blocks of 8 k: per tile of 8 x 8 pairs 128 lanes (pair, sign) evaluate psi along the inputs -- products before the group
// forwards from input 0, behind it backwards from input D-1, so a leave-one-out product is prefix * suffix, never a quotient, and has
// the same bits whatever the group size -- and leave the centred coefficients in LDS as the four real entries of the symmetric form
// (cos-cos, sin-sin, cos-sin, sin-cos); then 256 lanes (input of the group, pair of columns) contract them with the weights into
// register accumulators that live across the unit's tiles.  The workgroups' records are added in unit order by sobol_reduce.  No
// K x K matrix reaches memory, no atomics.  A column's sums run over units, tiles and pairs in one order, whatever else the call holds.
// Every product chain below is evaluated at more than one place (before, inside and behind a group; per column slot), and the promises of
// the header need the same bits at each: no contraction the source does not spell out, in fast_sincos too.
#pragma clang fp contract(off)
#include "kernels.h"
#include "sincos.h"

namespace {

struct cplx { double re, im; };
__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return {fma(a.re, b.re, -(a.im * b.im)), fma(a.re, b.im, a.im * b.re)}; }
__device__ __forceinline__ cplx cconj(cplx a, bool yes) { return {a.re, yes ? -a.im : a.im}; }

// sin t / t: its series where |t| < 1/2 (the term after t^14 / 15! is below 2^-64), 1 at 0
__device__ __forceinline__ double sinc(double t) {
    if (fabs(t) < 0.5) {
        const double u = t * t;
        double r = -1.0 / 1307674368000.0;
        r = fma(u, r, 1.0 / 6227020800.0); r = fma(u, r, -1.0 / 39916800); r = fma(u, r, 1.0 / 362880); r = fma(u, r, -1.0 / 5040);
        r = fma(u, r, 1.0 / 120); r = fma(u, r, -1.0 / 6);
        return fma(u, r, 1.0);
    }
    double sn, cs;
    fast_sincos(t, sn, cs);
    return sn / t;
}

// meas (3 x D): kind; uniform: centre and half width, normal: mean and standard deviation
__device__ __forceinline__ cplx psi(const double* __restrict__ meas, int D, int d, double om) {
    const double m0 = meas[D + d], m1 = meas[2 * D + d];
    double sn, cs;
    fast_sincos(om * m0, sn, cs);
    double amp;
    if (meas[d] == 0.0) amp = sinc(om * m1);
    else { const double t = om * m1; amp = exp(-0.5 * t * t); }
    return {cs * amp, sn * amp};
}

}  // namespace

// One lane per j < J.  psi1, Ed (D x Jt complex), E, Eb (Jt complex), phibar (K).  E = e^{ib} (psi_0 (psi_1 (... psi_{D-1}))), E^{-d} =
// e^{ib} (prefix_d suffix_{d+1}) with prefix_d = ((psi_0 psi_1) ...) psi_{d-1}: Ed holds the prefixes between the two passes.
__global__ __launch_bounds__(64) void sobol_tables_kernel(const double* __restrict__ Fall, const Scal* __restrict__ sc,
                                                          const double* __restrict__ meas, int D, int J, int Jp, int Jt,
                                                          double* __restrict__ psi1, double* __restrict__ Ed, double* __restrict__ E,
                                                          double* __restrict__ Eb, double* __restrict__ phibar) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= J) return;
    cplx pre = {1.0, 0.0};
    for (int d = 0; d < D; ++d) {
        const cplx p = psi(meas, D, d, Fall[(int64_t)d * Jp + j]);
        const int64_t o = 2 * ((int64_t)d * Jt + j);
        psi1[o] = p.re; psi1[o + 1] = p.im;
        Ed[o] = pre.re; Ed[o + 1] = pre.im;
        pre = cmul(pre, p);
    }
    cplx eb;
    fast_sincos(Fall[(int64_t)D * Jp + j], eb.im, eb.re);
    cplx suf = {1.0, 0.0};
    for (int d = D - 1; d >= 0; --d) {
        const int64_t o = 2 * ((int64_t)d * Jt + j);
        const cplx v = cmul(eb, cmul(cplx{Ed[o], Ed[o + 1]}, suf));
        Ed[o] = v.re; Ed[o + 1] = v.im;
        suf = cmul(cplx{psi1[o], psi1[o + 1]}, suf);
    }
    const cplx e = cmul(eb, suf);
    E[2 * j] = e.re; E[2 * j + 1] = e.im;
    Eb[2 * j] = eb.re; Eb[2 * j + 1] = eb.im;
    if (phibar) { phibar[j] = sc->s * e.re; phibar[J + j] = sc->s * e.im; }
}

// omax[d] = max_j |Fall[d][j]| over j < J, one wave per input: what scfgp_sobol holds the measure against before any psi is evaluated
// (api_host.h: sobol_first_out_of_domain).  A maximum has no order, so the shuffle tree is no part of any summation.
__global__ __launch_bounds__(64) void sobol_omax_kernel(const double* __restrict__ Fall, int J, int Jp, double* __restrict__ omax) {
    const int d = blockIdx.x;
    double m = 0.0;
    for (int j = threadIdx.x; j < J; j += 64) m = fmax(m, fabs(Fall[(int64_t)d * Jp + j]));
    for (int o = 32; o; o >>= 1) m = fmax(m, __shfl_xor(m, o));
    if (threadIdx.x == 0) omax[d] = m;
}

// A (Jt x nw complex): a_j of every column, zero for j >= J; f0 (nw, or NULL) = Re sum_j a_j E_j in index order
__global__ __launch_bounds__(256) void sobol_weights_kernel(const double* __restrict__ W, const Scal* __restrict__ sc,
                                                            const double* __restrict__ E, int J, int Jt, int nw, double* __restrict__ A,
                                                            double* __restrict__ f0) {
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= nw) return;
    const double s = sc->s;
    double acc = 0.0;
    for (int j = 0; j < Jt; ++j) {
        const double ar = j < J ? s * W[(int64_t)j * nw + w] : 0.0, ai = j < J ? -(s * W[(int64_t)(J + j) * nw + w]) : 0.0;
        A[2 * ((int64_t)j * nw + w)] = ar;
        A[2 * ((int64_t)j * nw + w) + 1] = ai;
        if (j < J) acc = fma(-ai, E[2 * j + 1], fma(ar, E[2 * j], acc));
    }
    if (f0) f0[w] = acc;
}

// LDS of the pair kernel, in doubles: the coefficients of a tile's 64 pairs for the G inputs of the group (8 per pair and input: the
// main and the closed form; a pair's block is padded by 4 doubles, so that the 128 lanes (pair, sign) of the first phase, which all write
// the same input at once, spread over the banks), those of the whole set (4 per pair), a_j and a_k of the block's 32 columns (8 x 32
// complex each)
__host__ __device__ static inline int sobol_pair_stride(int G) { return G * 8 + 4; }
__host__ __device__ static inline int sobol_lds_doubles(int G) { return 64 * sobol_pair_stride(G) + 64 * 4 + 2 * SOBOL_T * SOBOL_COLS * 2; }

// units (3 ints each): block of j, first and one-past-last block of k.  flags: 1 = the whole set, 2 = main effects, 4 = closed sets.
// rec (units x nsets x ncols), nsets = 1 + 2 D: set 0 = all, 1 + d = main, 1 + D + d = closed; only what flags ask for is written.
__global__ __launch_bounds__(256) void sobol_pairs_kernel(const double* __restrict__ Fall, const double* __restrict__ meas,
                                                          const double* __restrict__ psi1, const double* __restrict__ Ed,
                                                          const double* __restrict__ E, const double* __restrict__ Eb,
                                                          const double* __restrict__ A, const int* __restrict__ units, int D, int J, int Jp,
                                                          int Jt, int nw, int w0, int ncols, int G, int flags, double* __restrict__ rec) {
    extern __shared__ double lds[];
    const int PS = sobol_pair_stride(G);
    double* Mg = lds;                              // [pair][input of the group][8], PS doubles a pair
    double* Mall = Mg + 64 * PS;                   // [pair][4]
    double* Aj = Mall + 64 * 4;                    // [jl][column][2]
    double* Ak = Aj + SOBOL_T * SOBOL_COLS * 2;
    const int tid = threadIdx.x;
    const int unit = blockIdx.x, cb = blockIdx.y, grp = blockIdx.z;
    const int jb = units[3 * unit], kb0 = units[3 * unit + 1], kb1 = units[3 * unit + 2];
    const int g0 = grp * G, g1 = g0 + G < D ? g0 + G : D, ng = g1 - g0;
    const bool all = (flags & 1) && grp == 0, mains = flags & 2, closed = flags & 4;
    // contraction lanes: an input of the group and two columns
    const int es = tid & 15, cs = tid >> 4;
    const int col = cb * SOBOL_COLS + 2 * cs;      // of this launch's ncols
    double am[2] = {0.0, 0.0}, ac[2] = {0.0, 0.0}, aa[2] = {0.0, 0.0};

    for (int x = tid; x < SOBOL_T * SOBOL_COLS; x += 256) {
        const int jl = x / SOBOL_COLS, c = x - jl * SOBOL_COLS, cc = cb * SOBOL_COLS + c;
        const int64_t o = 2 * ((int64_t)(jb * SOBOL_T + jl) * nw + w0 + cc);
        Aj[2 * x] = cc < ncols ? A[o] : 0.0;
        Aj[2 * x + 1] = cc < ncols ? A[o + 1] : 0.0;
    }
    for (int kb = kb0; kb < kb1; ++kb) {
        __syncthreads();                           // the last tile's contraction is over
        for (int x = tid; x < SOBOL_T * SOBOL_COLS; x += 256) {
            const int kl = x / SOBOL_COLS, c = x - kl * SOBOL_COLS, cc = cb * SOBOL_COLS + c;
            const int64_t o = 2 * ((int64_t)(kb * SOBOL_T + kl) * nw + w0 + cc);
            Ak[2 * x] = cc < ncols ? A[o] : 0.0;
            Ak[2 * x + 1] = cc < ncols ? A[o + 1] : 0.0;
        }
        // ---- coefficients: lane (pair, sign); a pair beyond J or below the diagonal is evaluated at clamped indices and weighs 0 ----
        if (tid < 128) {
            const int p = tid >> 1, minus = tid & 1;
            const int jr = jb * SOBOL_T + (p >> 3), kr = kb * SOBOL_T + (p & 7);
            const int j = jr < J ? jr : J - 1, k = kr < J ? kr : J - 1;
            const double sg = minus ? -1.0 : 1.0;
            double* mine = Mg + p * PS + minus * 2;      // per input: [+main | -main | +closed | -closed], complex each
            cplx pre = {1.0, 0.0}, suf = {1.0, 0.0};
            if (closed)
                for (int e = 0; e < g0; ++e) pre = cmul(pre, psi(meas, D, e, Fall[(int64_t)e * Jp + j] + sg * Fall[(int64_t)e * Jp + k]));
            for (int e = g0; e < g1; ++e) {
                const cplx v = psi(meas, D, e, Fall[(int64_t)e * Jp + j] + sg * Fall[(int64_t)e * Jp + k]);
                double* m = mine + (e - g0) * 8;
                m[0] = v.re; m[1] = v.im;
                m[4] = pre.re; m[5] = pre.im;
                if (closed) pre = cmul(pre, v);
            }
            const cplx ej = {E[2 * j], E[2 * j + 1]}, ek = cconj(cplx{E[2 * k], E[2 * k + 1]}, minus);
            const cplx cen = cmul(ej, ek);
            const cplx eb = cmul(cplx{Eb[2 * j], Eb[2 * j + 1]}, cconj(cplx{Eb[2 * k], Eb[2 * k + 1]}, minus));
            if (closed || all)
                for (int e = D - 1; e >= g1; --e) suf = cmul(psi(meas, D, e, Fall[(int64_t)e * Jp + j] + sg * Fall[(int64_t)e * Jp + k]), suf);
            for (int e = g1 - 1; e >= g0; --e) {
                double* m = mine + (e - g0) * 8;
                const cplx v = {m[0], m[1]};
                const int64_t tj = 2 * ((int64_t)e * Jt + j), tk = 2 * ((int64_t)e * Jt + k);
                if (mains) {
                    const cplx pm = cmul(cmul(cplx{Ed[tj], Ed[tj + 1]}, cconj(cplx{Ed[tk], Ed[tk + 1]}, minus)), v);
                    m[0] = pm.re - cen.re; m[1] = pm.im - cen.im;
                }
                if (closed) {
                    const cplx loo = cmul(cplx{m[4], m[5]}, suf);
                    const cplx pc = cmul(cmul(eb, cmul(cplx{psi1[tj], psi1[tj + 1]}, cconj(cplx{psi1[tk], psi1[tk + 1]}, minus))), loo);
                    m[4] = pc.re - cen.re; m[5] = pc.im - cen.im;
                }
                if (closed || all) suf = cmul(v, suf);
            }
            if (all) {                                               // grp == 0: suf is the product over every input
                const cplx pa = cmul(eb, suf);
                Mall[p * 4 + minus * 2] = pa.re - cen.re;
                Mall[p * 4 + minus * 2 + 1] = pa.im - cen.im;
            }
        }
        __syncthreads();
        // ---- (C+, C-) -> the real form, weighted: 1/2 on the diagonal, 1 above it, 0 elsewhere ----
        for (int x = tid; x < 64 * (2 * ng + 1); x += 256) {
            const int p = x / (2 * ng + 1), r = x - p * (2 * ng + 1);
            const int jr = jb * SOBOL_T + (p >> 3), kr = kb * SOBOL_T + (p & 7);
            const double wt = jr >= J || kr >= J || jr > kr ? 0.0 : jr == kr ? 0.5 : 1.0;
            double* m = r < 2 * ng ? Mg + p * PS + (r >> 1) * 8 + (r & 1) * 4 : Mall + p * 4;
            if (r == 2 * ng && !all) continue;
            const double pr = m[0], pi = m[1], mr = m[2], mi = m[3];
            m[0] = wt * (pr + mr);                 // cos-cos
            m[1] = wt * (mr - pr);                 // sin-sin
            m[2] = wt * (mi - pi);                 // cos-sin
            m[3] = wt * (-pi - mi);                // sin-cos
        }
        __syncthreads();
        // ---- contraction: (a_j a_k, a_j conj a_k) against the coefficients, pairs in order ----
        // both forms are accumulated whatever the call asks for (what it does not ask for is not stored): a branch per form in this
        // loop costs more than the eight FMAs it saves
        if (es < ng || (all && es == 0)) {
            const bool grp_lane = es < ng, all_lane = all && es == 0;
#pragma unroll 4
            for (int p = 0; p < 64; ++p) {
                const double* xj = Aj + ((p >> 3) * SOBOL_COLS + 2 * cs) * 2;
                const double* yk = Ak + ((p & 7) * SOBOL_COLS + 2 * cs) * 2;
                const double* m = Mg + p * PS + (grp_lane ? es : 0) * 8;
                double rr[2], ii[2], ri[2], ir[2], mm[8];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const double xr = xj[2 * c], xi = xj[2 * c + 1], yr = yk[2 * c], yi = yk[2 * c + 1];
                    rr[c] = xr * yr; ii[c] = xi * yi; ri[c] = xr * yi; ir[c] = xi * yr;
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) mm[q] = m[q];
                if (grp_lane) {
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        am[c] = fma(ir[c], mm[3], fma(ri[c], mm[2], fma(ii[c], mm[1], fma(rr[c], mm[0], am[c]))));
                        ac[c] = fma(ir[c], mm[7], fma(ri[c], mm[6], fma(ii[c], mm[5], fma(rr[c], mm[4], ac[c]))));
                    }
                }
                if (all_lane) {
                    const double* ma = Mall + p * 4;
#pragma unroll
                    for (int c = 0; c < 2; ++c) aa[c] = fma(ir[c], ma[3], fma(ri[c], ma[2], fma(ii[c], ma[1], fma(rr[c], ma[0], aa[c]))));
                }
            }
        }
    }
    const int nsets = 1 + 2 * D;
    double* out = rec + (int64_t)unit * nsets * ncols;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if (col + c >= ncols) continue;
        if (es < ng && mains) out[(int64_t)(1 + g0 + es) * ncols + col + c] = am[c];
        if (es < ng && closed) out[(int64_t)(1 + D + g0 + es) * ncols + col + c] = ac[c];
        if (all && es == 0) out[col + c] = aa[c];
    }
}

// sums (nsets x nw): column w0 + c of set s = the records of the units in unit order, for the sets that flags name
__global__ __launch_bounds__(256) void sobol_reduce_kernel(const double* __restrict__ rec, int nunits, int D, int ncols, int nw, int w0,
                                                           int flags, double* __restrict__ sums) {
    const int nsets = 1 + 2 * D;
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= (int64_t)nsets * ncols) return;
    const int s = (int)(x / ncols), c = (int)(x - (int64_t)s * ncols);
    const int need = s == 0 ? 1 : s <= D ? 2 : 4;
    if (!(flags & need)) return;
    double a = 0.0;
    for (int u = 0; u < nunits; ++u) a += rec[((int64_t)u * nsets + s) * ncols + c];
    sums[(int64_t)s * nw + w0 + c] = a;
}

void sobol_tables(const Geom& g, const double* Fall, const Scal* sc, const double* meas, int Jt, double* psi1, double* Ed, double* E,
                  double* Eb, double* phibar, hipStream_t st) {
    hipLaunchKernelGGL(sobol_tables_kernel, dim3((unsigned)((g.J + 63) / 64)), dim3(64), 0, st, Fall, sc, meas, g.D, g.J, g.Jp, Jt, psi1, Ed,
                       E, Eb, phibar);
}

void sobol_omax(const Geom& g, const double* Fall, double* omax, hipStream_t st) {
    hipLaunchKernelGGL(sobol_omax_kernel, dim3((unsigned)g.D), dim3(64), 0, st, Fall, g.J, g.Jp, omax);
}

void sobol_weights(const Geom& g, const double* W, const Scal* sc, const double* E, int Jt, int nw, double* A, double* f0, hipStream_t st) {
    hipLaunchKernelGGL(sobol_weights_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, W, sc, E, g.J, Jt, nw, A, f0);
}

void sobol_pairs(const Geom& g, const double* Fall, const double* meas, const double* psi1, const double* Ed, const double* E,
                 const double* Eb, const double* A, const int* units, int nunits, int Jt, int nw, int w0, int ncols, int G, int flags,
                 double* rec, hipStream_t st) {
    const int bytes = sobol_lds_doubles(G) * (int)sizeof(double);
    allow_big_lds(sobol_pairs_kernel, bytes);
    const int ngroups = flags & 6 ? (g.D + G - 1) / G : 1;
    hipLaunchKernelGGL(sobol_pairs_kernel, dim3((unsigned)nunits, (unsigned)((ncols + SOBOL_COLS - 1) / SOBOL_COLS), (unsigned)ngroups),
                       dim3(256), bytes, st, Fall, meas, psi1, Ed, E, Eb, A, units, g.D, g.J, g.Jp, Jt, nw, w0, ncols, G, flags, rec);
}

void sobol_reduce(const double* rec, int nunits, int D, int ncols, int nw, int w0, int flags, double* sums, hipStream_t st) {
    const int64_t n = (int64_t)(1 + 2 * D) * ncols;
    hipLaunchKernelGGL(sobol_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, rec, nunits, D, ncols, nw, w0, flags, sums);
}
