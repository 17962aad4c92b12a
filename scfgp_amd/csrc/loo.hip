// Exact leave-block-out predictions of rows that are IN the fit (scfgp_loo; derivation in include/scfgp_hip.h).  With C = Phi_I Li^T
// (apply_c's triangular product) and r = y_I - Phi_I alpha (rowresidual) of a block I of b <= 64 consecutive rows,
//     H = C C^T,  I - H = R R^T,  W = R^-1,  t = W r,  e = W^T t = (I - H)^-1 r,  d_i = sum_k W[k][i]^2 = [(I - H)^-1]_ii
//     mu_i = y_i - e_i,  sigma_i = sqrt(kappa d_i),  h_i = H_ii,  log p(y_I | rest) = -1/2 [ |t|^2 / kappa + b log(2 pi kappa) - 2 sum log R_ii ]
//
// One workgroup of 4 waves owns a GROUP of gs = (64 / b) b rows: whole blocks, one at b = 64.  H of the group is a 64 x 64 fp64 tile
// formed by fp64 MFMA (16 x 16 x 4) from the rows of C, converted on load in fp32 contexts; only the 16 x 16 tiles of its lower half that
// meet a diagonal b x b block are multiplied.  The Kp features are dealt to the waves in quarters; inside its quarter lane (i, q) reads the
// 16-byte slots q, q + 4, .. of row i of each of the four 16-row fragments (the four lanes of a row read 64 consecutive bytes), and MFMA
// step e pairs the e-th elements of the lanes' slots: a permutation of the reduction index that both operands share.  The waves add
// their tiles into the LDS image one after the other, so an entry's sum has one order whatever the group, the chunk or the call: a row's
// outputs depend on the rows of its own block only, bit for bit.  Rows past the call's last one are never loaded: their rows of H are zero,
// their rows of I - H the identity (ragged last block, ragged last group).
//
// The tail is fp64 in LDS and runs on the first wave: lane l is row l of the group, all blocks of the group advance in lockstep.  The
// image has 65 doubles per row (a lane's own row and a column across lanes are both conflict-free).  Left-looking Cholesky of I - H in
// the lower triangles; W = R^-1 column by column, column c into the UPPER triangle of row c (its diagonal stays in a register); t, e, d
// from W.  A pivot that is not positive (NaN included) records its block in bad[1] (the smallest index wins), a non-finite h or r sets
// bad[0]; nothing else happens: the arithmetic goes on with whatever it has and the host discards the call.
// One record per block goes to rec: sum e^2, sum |e|, sum log N(y_i; mu_i, sigma_i^2), the joint log density, max h -- from the ROUNDED
// outputs (e = y - mu, sigma^2 = sigma sigma), so a host that recomputes them from mu, std, lev meets the same terms.  For b = 1 the
// joint density of a block IS the marginal of its row and is copied, not recomputed.  loo_reduce_kernel adds the records in block order.
#include "kernels.h"
#include "block_gram.h"

constexpr int LOO_LD = BLOCK_GRAM_LD;           // doubles per row of the LDS image
constexpr int LOO_REC = 5;                      // doubles per block record

template <typename T>
__global__ __launch_bounds__(256) void loo_block_kernel(const T* __restrict__ C, int Kp, const double* __restrict__ rvec,
                                                        const double* __restrict__ y, int64_t N, int b, int gs, int64_t blk0,
                                                        const Scal* __restrict__ sc, double* __restrict__ mu, double* __restrict__ sd,
                                                        double* __restrict__ lev, double* __restrict__ rec,
                                                        unsigned long long* __restrict__ bad) {
    __shared__ double Hs[64 * LOO_LD];
    __shared__ double s_r[64], s_t[64], s_a[64], s_b[64], s_c[64], s_h[64], s_l[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t g0 = (int64_t)blockIdx.x * gs;                 // first row of the group (chunk-local)
    const int live = (int)(N - g0 < gs ? N - g0 : gs);           // live rows of the group (>= 1)

    block_gram<T>(C, Kp, g0, live, b, Hs);
    if (wave != 0) return;

    // ---- the tail: lane = row of the group; no workgroup barrier from here on (one wave: fences order its LDS traffic) ----------
#define LOO_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
    const int l = lane;
    const bool in_group = l < gs;                                // lanes past the group's blocks (gs < 64) idle
    const bool alive = l < live;
    const int ib = l % b, o = l - ib;                            // row in the block, first row of the block
    double* row = Hs + l * LOO_LD + o;                           // row[j] = image entry (l, o + j)
    const double h = row[ib];
    const double rr = alive ? rvec[g0 + l] : 0.0;
    const double yy = alive ? y[g0 + l] : 0.0;
    s_r[l] = rr;
    if (alive && !(isfinite(h) && isfinite(rr) && isfinite(yy))) atomicOr(&bad[0], 1ull);
    if (in_group)
        for (int j = 0; j <= ib; ++j) row[j] = (j == ib ? 1.0 : 0.0) - row[j];
    LOO_SYNC();
    for (int j = 0; j < b; ++j) {
        double s = 0.0;
        if (in_group && ib >= j) {
            const double* rj = Hs + (o + j) * LOO_LD + o;
            s = row[j];
            for (int k = 0; k < j; ++k) s -= row[k] * rj[k];
            if (ib == j) {
                if (!(s > 0.0)) atomicMin(&bad[1], (unsigned long long)(blk0 + (g0 + o) / b));
                row[j] = sqrt(s);
            }
        }
        LOO_SYNC();
        if (in_group && ib > j) row[j] = s / Hs[(o + j) * LOO_LD + o + j];
        LOO_SYNC();
    }
    // W = R^-1: lane l owns column ib of its block; W[k][ib] (k > ib) goes to the upper triangle, entry (l, o + k)
    const double dg = row[ib];
    const double wcc = 1.0 / dg;
    if (in_group)
        for (int k = ib + 1; k < b; ++k) {
            const double* rk = Hs + (o + k) * LOO_LD + o;
            double a = rk[ib] * wcc;
            for (int m = ib + 1; m < k; ++m) a += rk[m] * row[m];
            row[k] = -a / rk[k];
        }
    LOO_SYNC();
    double t = wcc * rr;
    if (in_group)
        for (int m = 0; m < ib; ++m) t += Hs[(o + m) * LOO_LD + l] * s_r[o + m];
    s_t[l] = t;
    LOO_SYNC();
    double e = wcc * t, d = wcc * wcc;
    if (in_group)
        for (int k = ib + 1; k < b; ++k) { e += row[k] * s_t[o + k]; d += row[k] * row[k]; }
    const double kappa = sc->kappa;
    const double TWO_PI = 6.283185307179586476925286766559;
    double m_out = 0, s_out = 0;
    if (alive) {
#pragma clang fp contract(off)
        m_out = yy - e;
        s_out = sqrt(kappa * d);
        mu[g0 + l] = m_out; sd[g0 + l] = s_out;
        if (lev) lev[g0 + l] = h;
        // the record's terms from the rounded outputs, as a host recomputes them
        const double er = yy - m_out, var = s_out * s_out;
        const double e2 = er * er;
        s_a[l] = e2; s_b[l] = fabs(er); s_c[l] = -0.5 * (e2 / var + log(TWO_PI * var));
    }
    s_h[l] = h; s_l[l] = log(dg);
    LOO_SYNC();
    if (alive && ib == 0) {
        const int nb = live - o < b ? live - o : b;              // live rows of this block
        double a1 = 0, a2 = 0, a3 = 0, tt = 0, ld = 0, hm = s_h[l];
        for (int k = 0; k < nb; ++k) {
            a1 += s_a[l + k]; a2 += s_b[l + k]; a3 += s_c[l + k];
            tt += s_t[l + k] * s_t[l + k]; ld += s_l[l + k];
            hm = s_h[l + k] > hm ? s_h[l + k] : hm;
        }
        const double joint = b == 1 ? a3 : -0.5 * (tt / kappa + nb * log(TWO_PI * kappa) - 2.0 * ld);
        double* out = rec + ((g0 + o) / b) * LOO_REC;
        out[0] = a1; out[1] = a2; out[2] = a3; out[3] = joint; out[4] = hm;
    }
#undef LOO_SYNC
}

// acc[0..3] += the records' four sums in block order, acc[4] = max(acc[4], max h): one lane per number, one after the other
__global__ __launch_bounds__(64) void loo_reduce_kernel(const double* __restrict__ rec, int64_t nblk, double* __restrict__ acc) {
    const int s = threadIdx.x;
    if (s >= LOO_REC) return;
    double a = acc[s];
    int64_t j = 0;
    for (; j + 8 <= nblk; j += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = rec[(j + u) * LOO_REC + s];
#pragma unroll
        for (int u = 0; u < 8; ++u) a = s < 4 ? a + v[u] : (v[u] > a ? v[u] : a);
    }
    for (; j < nblk; ++j) {
        const double v = rec[j * LOO_REC + s];
        a = s < 4 ? a + v : (v > a ? v : a);
    }
    acc[s] = a;
}

template <typename T>
void loo_blocks(const Geom& g, const T* C, const double* r, const double* y, int block, int64_t blk0, const Scal* sc, double* mu,
                double* sd, double* lev, double* rec, double* acc, unsigned long long* bad, hipStream_t st) {
    const int gs = 64 / block * block;
    const int64_t ngroups = (g.N + gs - 1) / gs, nblk = (g.N + block - 1) / block;
    hipLaunchKernelGGL(loo_block_kernel<T>, dim3((unsigned)ngroups), dim3(256), 0, st, C, g.Kp, r, y, g.N, block, gs, blk0, sc, mu, sd, lev,
                       rec, bad);
    hipLaunchKernelGGL(loo_reduce_kernel, dim3(1), dim3(64), 0, st, rec, nblk, acc);
}

template void loo_blocks<double>(const Geom&, const double*, const double*, const double*, int, int64_t, const Scal*, double*, double*,
                                 double*, double*, double*, unsigned long long*, hipStream_t);
template void loo_blocks<float>(const Geom&, const float*, const double*, const double*, int, int64_t, const Scal*, double*, double*,
                                double*, double*, double*, unsigned long long*, hipStream_t);
