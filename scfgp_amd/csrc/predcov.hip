// Joint posterior covariance between test points (scfgp_predict_cov): with C = Phi* Li^T (apply_c's triangular product),
//     Cov[f(a_i), f(b_j)] = kappa phi(a_i)^T A^-1 phi(b_j) = kappa sum_k Ca[i][k] Cb[j][k]        (A^-1 = Li^T Li)
// an NT product of two row-major arrays whose reduction index is the contiguous one.  Built on the MFMA traits of tile_engine.h;
// templated on the storage type T of C (fp64 MFMA in fp64 mode, exact fp32 MFMA with fp64 partial sums in fp32 and f16x3 contexts).
#include "kernels.h"
#include "tile_engine.h"

// A workgroup of 2 x 2 waves owns a 128 x 128 output tile; a wave 64 x 64 of it (4 x 4 MFMA tiles of 16 x 16).  Both operand panels
// go through LDS in k-tiles of 128 bytes per row (32 fp32 / 16 fp64 features), in the global layout (row-major, k contiguous): a
// panel image is [128 rows][8 slots of 16 bytes], slot s of row r stored at slot s ^ ((r >> 1) & 7).  Lane (i, q) = (lane % 16,
// lane / 16) reads slots q and q + 4 of its rows by ds_read_b128; with that XOR the 16 lanes of each of the instruction's four lane
// groups fall on 16 different 16-byte slots of the 256-byte bank row (rows of one parity share its half; their 8 lanes carry the 8
// different values of (r >> 1) & 7 xor'ed into two q that differ in one bit), and the 8 lanes of a ds_write_b128 group fill one row.
// MFMA step e pairs k slot q with the e-th element of the lane's slot in A and in B alike: a permutation of the reduction index
// that both operands share.  Two LDS buffers per operand (64 KB in all): the next k-tile's global loads are issued before the
// current tile's MFMAs and stored after them, one barrier per k-tile.
// The k loop of an element is the same in every tile and every launch: its value depends on neither Ta, Tb, the panel nor the
// chunk it falls in, and, the products being commutative, Out[i][j] of (A, B) equals Out[j][i] of (B, A) bit for bit.
// fp32: the accumulators are added into fp64 partial sums every PREDCOV_FLUSH features (as sample_fw_kernel does).
// Epilogue: x kappa in fp64, + kappa where the global row equals the column (noise); rows < nrows and columns < Tb only.
constexpr int PREDCOV_TILE = 128;
constexpr int PREDCOV_FLUSH = 128;

template <typename T>
__global__ __launch_bounds__(256) void predcov_kernel(const T* __restrict__ Ca, const T* __restrict__ Cb, int Kp, int nkt, int64_t nrows,
                                                      int64_t Tb, int64_t row_base, int noise, const Scal* __restrict__ sc,
                                                      double* __restrict__ out) {
    typedef MT<T, 16> M;
    typedef typename Vec16<T>::type vec_t;                       // one 16-byte slot
    constexpr bool F32 = sizeof(T) == 4;
    constexpr int VN = Vec16<T>::N, BK = 8 * VN;                 // features per slot, per k-tile
    constexpr int SLOTS = PREDCOV_TILE * 8;                      // 16-byte slots of one panel image
    constexpr int FLUSH_KT = PREDCOV_FLUSH / BK;
    __shared__ vec_t lds[2][2][SLOTS];                           // [buffer][operand]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int64_t r0 = (int64_t)blockIdx.y * PREDCOV_TILE, c0 = (int64_t)blockIdx.x * PREDCOV_TILE;

    // staging: thread t moves slot t % 8 of rows t / 8 + 32 j of both panels (8 lanes: one 128-byte row segment)
    const int srow = tid >> 3, sslot = tid & 7;
    const vec_t* __restrict__ ga = reinterpret_cast<const vec_t*>(Ca + (r0 + srow) * Kp) + sslot;
    const vec_t* __restrict__ gb = reinterpret_cast<const vec_t*>(Cb + (c0 + srow) * Kp) + sslot;
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
    // fragment reads: rows wm + 16 t + i of A, wn + 16 t + i of B
    // (the XOR of a row is that of i: wm, wn and 16 t are multiples of 16)
    const int aoff = (wm + i) * 8, boff = (wn + i) * 8, swz = (i >> 1) & 7;

    typename M::acc_t acc[4][4];
    double part[4][4][4];                                        // fp32 only
#pragma unroll
    for (int tm = 0; tm < 4; ++tm)
#pragma unroll
        for (int tn = 0; tn < 4; ++tn)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                acc[tm][tn][r] = 0;
                if (F32) part[tm][tn][r] = 0.0;
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
        if (F32 && ((kt + 1) % FLUSH_KT == 0 || kt + 1 == nkt)) {
#pragma unroll
            for (int tm = 0; tm < 4; ++tm)
#pragma unroll
                for (int tn = 0; tn < 4; ++tn)
#pragma unroll
                    for (int r = 0; r < 4; ++r) { part[tm][tn][r] += (double)acc[tm][tn][r]; acc[tm][tn][r] = 0; }
        }
        // the other buffer was last read before the barrier that ended tile kt - 1
        if (kt + 1 < nkt) stage(buf ^ 1);
        __syncthreads();
    }

    const double kappa = sc->kappa;
#pragma unroll
    for (int tm = 0; tm < 4; ++tm)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t n = r0 + wm + 16 * tm + M::crow(lane, r);
#pragma unroll
            for (int tn = 0; tn < 4; ++tn) {
                const int64_t j = c0 + wn + 16 * tn + i;
                if (n < nrows && j < Tb) {
#pragma clang fp contract(off)
                    // kappa s, then + kappa: two roundings, as the host would add it
                    double v = kappa * (F32 ? part[tm][tn][r] : (double)acc[tm][tn][r]);
                    if (noise && row_base + n == j) v = v + kappa;
                    out[n * Tb + j] = v;
                }
            }
        }
}

template <typename T>
void predcov(const Geom& g, const T* Ca, const T* Cb, int64_t nrows, int64_t Tb, int64_t row_base, int noise, const Scal* sc, double* out,
             hipStream_t st) {
    constexpr int BK = 8 * Vec16<T>::N;
    const int nkt = (int)(round_up(g.K, BK) / BK);               // <= Kp / BK: Kp is a multiple of 128
    const dim3 grid((unsigned)((Tb + PREDCOV_TILE - 1) / PREDCOV_TILE), (unsigned)((nrows + PREDCOV_TILE - 1) / PREDCOV_TILE));
    hipLaunchKernelGGL(predcov_kernel<T>, grid, dim3(256), 0, st, Ca, Cb, g.Kp, nkt, nrows, Tb, row_base, noise, sc, out);
}

template void predcov<double>(const Geom&, const double*, const double*, int64_t, int64_t, int64_t, int, const Scal*, double*, hipStream_t);
template void predcov<float>(const Geom&, const float*, const float*, int64_t, int64_t, int64_t, int, const Scal*, double*, hipStream_t);
