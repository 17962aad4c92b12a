// Posterior sample functions (scfgp_sample, scfgp_sample_weights).  The reference defines the marginals only (SCFGP/SCFGP.py:103-110,
// 138-148): A = Phi^T Phi + (sigma_n^2 + eps) I = L L^T, Li = L^-1, alpha = Li^T Li Phi^T y, kappa = softplus(c) and
//     mu*(x) = phi(x)^T alpha,   sigma*(x)^2 = kappa (1 + || Li phi(x) ||^2).
// A^-1 = Li^T Li, so the Gaussian over the K weights  w ~ N(alpha, kappa A^-1),  w_s = alpha + sqrt(kappa) Li^T z_s,  z_s ~ N(0, I_K)
// reproduces them exactly: f_s(x) = phi(x)^T w_s has mean mu*, variance sigma*^2 - kappa and covariance kappa phi(x)^T A^-1 phi(x') between
// two points; y_s(x) = f_s(x) + sqrt(kappa) eps (eps ~ N(0, 1)) has the marginal N(mu*, sigma*^2) that pred_func reports.
//
// The random numbers are counter-based and part of the contract, so a sample function is a function: the same seed gives the same
// functions on any rows, in any chunking, for any nsamp.  Philox4x64-10 (Random123) maps counter (c0, c1, 0, 0) and key (seed, stream)
// to four 64-bit words; U(u) = ((u >> 11) + 0.5) 2^-53; word pair p = (s & 3) >> 1 feeds Box-Muller in fp64,
// r = sqrt(-2 ln U(w_2p)), normal = r cos(2 pi U(w_2p+1)) for even s, r sin(...) for odd s.
//     z[k][s]    counter (k, s >> 2), stream 0      (k < K: alpha's layout, J cosine then J sine features)
//     eps[t][s]  counter (t, s >> 2), stream 1      (t: the row's index in the call's Xs)
//
// Kernels: Z from the generator; W = alpha 1^T + sqrt(kappa) Li^T Z in fp64 (LDS tiles, the triangle of Li only) with its typed copy;
// per chunk of test rows Out = Phi* W on the matrix pipe (fp64 MFMA in fp64 contexts, exact fp32 MFMA with fp64 partial sums
// otherwise) and an fp64 epilogue (observation noise, the y scaler's backward transform).
// scfgp_sample_argmax: the same product with a second epilogue that keeps, per sample column, the best (value, row) of the workgroup's
// rows instead of storing the block; sample_argmax_merge_kernel folds the workgroups' records into a running best across chunks.
#include <type_traits>
#include "kernels.h"
#include "tile_engine.h"
#include "yscale.h"
#include "argmax.h"

// Philox4x64-10 of counter (c0, c1, 0, 0) and key (k0, k1)
__device__ __forceinline__ void philox4x64_10(uint64_t c0, uint64_t c1, uint64_t k0, uint64_t k1, uint64_t (&o)[4]) {
    uint64_t c2 = 0, c3 = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B97F4A7C15ull; k1 += 0xBB67AE8584CAA73Bull; }
        const uint64_t hi0 = __umul64hi(0xD2E7470EE14C6C93ull, c0), lo0 = 0xD2E7470EE14C6C93ull * c0;
        const uint64_t hi1 = __umul64hi(0xCA5A826395121157ull, c2), lo1 = 0xCA5A826395121157ull * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}
__device__ __forceinline__ double philox_u01(uint64_t u) { return ((double)(u >> 11) + 0.5) * 0x1p-53; }
// the standard normal of index `idx` (k or t), sample s, stream 0 (weights) or 1 (observation noise)
__device__ double sample_normal(uint64_t idx, int s, uint64_t seed, uint64_t stream) {
    uint64_t w[4];
    philox4x64_10(idx, (uint64_t)(s >> 2), seed, stream, w);
    const bool hi = (s & 2) != 0;
    const double r = sqrt(-2.0 * log(philox_u01(hi ? w[2] : w[0])));
    const double th = 2.0 * M_PI * philox_u01(hi ? w[3] : w[1]);
    return (s & 1) ? r * sin(th) : r * cos(th);
}

// Z (Kw x ldw fp64): z[k][s] for k < K, s < nsamp, zero elsewhere
__global__ __launch_bounds__(256) void sample_z_kernel(int K, int nsamp, int64_t Kw, int ldw, uint64_t seed, double* __restrict__ Z) {
    const int64_t total = Kw * ldw;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int k = (int)(e / ldw), s = (int)(e % ldw);
        Z[e] = k < K && s < nsamp ? sample_normal((uint64_t)k, s, seed, 0) : 0.0;
    }
}

// W[k][s] = alpha[k] + sqrt(kappa) sum_{j >= k} Li[j][k] Z[j][s] (Li: K x K, ld K; entries above the diagonal are not read) on a 64 x 64
// output tile per workgroup, 4 x 4 per thread; j runs upwards from the tile's first row in steps of 16, so the summation order of an
// element depends on k alone.  Written for k < Kw, s < ldw (zero outside K x nsamp), in fp64 and as the typed operand Wt.
template <typename T>
__global__ __launch_bounds__(256) void sample_w_kernel(const double* __restrict__ Li, const double* __restrict__ Z, const double* __restrict__ alpha,
                                                       const Scal* __restrict__ sc, int K, int nsamp, int ldw, double* __restrict__ W,
                                                       T* __restrict__ Wt) {
    __shared__ double sl[16][64], sz[16][64];
    const int tid = threadIdx.x, tk = tid >> 4, ts = tid & 15;
    const int k0 = blockIdx.y * 64, s0 = blockIdx.x * 64;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    for (int j0 = k0; j0 < K; j0 += 16) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int idx = tid + 256 * e, jj = idx >> 6, cc = idx & 63, j = j0 + jj, k = k0 + cc;
            sl[jj][cc] = j < K && k < K && j >= k ? Li[(int64_t)j * K + k] : 0.0;
            sz[jj][cc] = j < K ? Z[(int64_t)j * ldw + s0 + cc] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < 16; ++jj)
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = fma(sl[jj][tk + 16 * a], sz[jj][ts + 16 * b], acc[a][b]);
        __syncthreads();
    }
    const double sk = sqrt(sc->kappa);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int k = k0 + tk + 16 * a;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int s = s0 + ts + 16 * b;
            const double w = k < K && s < nsamp ? fma(sk, acc[a][b], alpha[k]) : 0.0;
            W[(int64_t)k * ldw + s] = w;
            Wt[(int64_t)k * ldw + s] = (T)w;
        }
    }
}

template <typename T>
void sample_weights(const Geom& g, const double* Li, const double* alpha, const Scal* sc, int nsamp, uint64_t seed, double* Z, double* W,
                    T* Wt, hipStream_t st) {
    const int64_t Kw = sample_w_rows(g.K);
    const int ldw = sample_w_cols(nsamp);
    hipLaunchKernelGGL(sample_z_kernel, dim3(1024), dim3(256), 0, st, g.K, nsamp, Kw, ldw, seed, Z);
    hipLaunchKernelGGL(sample_w_kernel<T>, dim3((unsigned)(ldw / 64), (unsigned)(Kw / 64)), dim3(256), 0, st, Li, Z, alpha, sc, g.K, nsamp,
                       ldw, W, Wt);
}

// four consecutive elements of a Phi row (16-byte aligned: Kp and the offset are multiples of 4)
__device__ __forceinline__ void load_row4(const float* __restrict__ p, float (&v)[4]) {
    const v4f x = *reinterpret_cast<const v4f*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = x[e];
}
__device__ __forceinline__ void load_row4(const double* __restrict__ p, double (&v)[4]) {
    const v2d x0 = *reinterpret_cast<const v2d*>(p), x1 = *reinterpret_cast<const v2d*>(p + 2);
    v[0] = x0[0]; v[1] = x0[1]; v[2] = x1[0]; v[3] = x1[1];
}

// Out = Phi* W for 16 TM rows x the NST 16-wide column tiles [s0, s0 + 16 NST) per wave, after predgrad_zf_kernel's pattern: no LDS and
// no barriers; lane (i, q) = (lane % 16, lane / 16) loads features k0 + 4q .. k0 + 4q + 3 of its rows (16-byte loads) and the matching
// rows of W (re-read by every wave from L1 / L2); MFMA step e pairs k slot q with feature k0 + 4q + e in both operands.  The loop over
// the features is the same for every column tile, so the value of an element depends neither on nsamp nor on the launch plan.  fp32:
// the accumulators are added into fp64 partial sums every SAMPLE_FLUSH features (exact fp32 products, fp32 sums over 128 features
// only).  out: the chunk's N x nsamp block, row-major, in fp64; noise and the y scaler follow in sample_post_kernel (in the product's
// own epilogue the generator and the transform cost the main loop its registers).
// Out selects the epilogue: double* is that store; SampleArgmaxOut is scfgp_sample_argmax's reduction (below).  The main loop is the
// same text for both, so the value of an element is the same bits in both.
constexpr int SAMPLE_FLUSH = 128;

// the argmax epilogue's destination: w the chunk's weights (NULL: every row is eligible; row n is eligible iff w[n] > 0), pv / pt the
// workgroups' records ([gridDim.x][nsamp]: value, chunk-local row or -1), flag set where an eligible row's value is not finite
struct SampleArgmaxOut {
    const double* w;
    double* pv;
    long long* pt;
    int* flag;
    int minimize;
};

// the kernel's last parameter: the store epilogue keeps its restrict qualifier
template <typename Out> struct SampleDst { typedef Out type; };
template <> struct SampleDst<double*> { typedef double* __restrict__ type; };

template <typename T, int NST, typename Out>
__global__ __launch_bounds__(256) void sample_fw_kernel(const T* __restrict__ Phi, const T* __restrict__ Wt, int ldw, int s0, int Kq, int Kp,
                                                        int64_t N, int nsamp, typename SampleDst<Out>::type dst) {
    typedef MT<T, 16> M;
    constexpr bool F32 = sizeof(T) == 4;
    constexpr int TM = F32 ? 2 : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * 16 * TM;
    typename M::acc_t acc[TM][NST];
    double part[TM][NST][4];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < NST; ++tn)
#pragma unroll
            for (int r = 0; r < 4; ++r) { acc[tm][tn][r] = 0; part[tm][tn][r] = 0.0; }
    const T* __restrict__ wcol = Wt + s0 + i;
    for (int k0 = 0; k0 < Kq; k0 += 16) {
        const int kl = k0 + 4 * q;
        T b[4][NST];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int tn = 0; tn < NST; ++tn) b[e][tn] = wcol[(int64_t)(kl + e) * ldw + tn * 16];
        T a[TM][4];
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) load_row4(Phi + (row0 + tm * 16 + i) * Kp + kl, a[tm]);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < NST; ++tn) M::mfma(acc[tm][tn], a[tm][e], b[e][tn]);
        if (F32 && ((k0 + 16) % SAMPLE_FLUSH == 0 || k0 + 16 >= Kq)) {
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < NST; ++tn)
#pragma unroll
                    for (int r = 0; r < 4; ++r) { part[tm][tn][r] += (double)acc[tm][tn][r]; acc[tm][tn][r] = 0; }
        }
    }
    if constexpr (std::is_same<Out, double*>::value) {
        double* __restrict__ out = dst;                           // scfgp_sample's store, unchanged
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t n = row0 + tm * 16 + M::crow(lane, r);
#pragma unroll
                for (int tn = 0; tn < NST; ++tn) {
                    const int s = s0 + tn * 16 + i;
                    if (n < N && s < nsamp) out[n * nsamp + s] = F32 ? part[tm][tn][r] : (double)acc[tm][tn][r];
                }
            }
    } else {
        // the lane's 4 TM rows of each column tile -> the four q-groups of a column (lanes i, i + 16, i + 32, i + 48) by shuffles -> the
        // four waves through LDS -> one record per column of the workgroup
        const bool mini = dst.minimize != 0;
        __shared__ double sv[4][16 * NST];
        __shared__ long long sl[4][16 * NST];
        bool eligible[TM][4];
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t n = row0 + tm * 16 + M::crow(lane, r);
                eligible[tm][r] = n < N && (!dst.w || dst.w[n] > 0.0);
            }
        bool bad = false;
#pragma unroll
        for (int tn = 0; tn < NST; ++tn) {                          // one column tile at a time: one record live per lane
            const bool live = s0 + tn * 16 + i < nsamp;
            double bv = 0.0;
            long long bt = -1;
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double v = F32 ? part[tm][tn][r] : (double)acc[tm][tn][r];
                    const long long n = row0 + tm * 16 + M::crow(lane, r);
                    if (eligible[tm][r] && live) {
                        bad |= !isfinite(v);
                        if (argmax_beats(v, n, bv, bt, mini)) { bv = v; bt = n; }
                    }
                }
#pragma unroll
            for (int off = 16; off <= 32; off <<= 1) {
                const double ov = __shfl_xor(bv, off);
                const long long ot = __shfl_xor(bt, off);
                if (argmax_beats(ov, ot, bv, bt, mini)) { bv = ov; bt = ot; }
            }
            if (q == 0) { sv[wave][tn * 16 + i] = bv; sl[wave][tn * 16 + i] = bt; }
        }
        __syncthreads();
        const int col = threadIdx.x, s = s0 + col;
        if (col < 16 * NST && s < nsamp) {
            double v = sv[0][col];
            long long t = sl[0][col];
#pragma unroll
            for (int wv = 1; wv < 4; ++wv)
                if (argmax_beats(sv[wv][col], sl[wv][col], v, t, mini)) { v = sv[wv][col]; t = sl[wv][col]; }
            dst.pv[(int64_t)blockIdx.x * nsamp + s] = v;
            dst.pt[(int64_t)blockIdx.x * nsamp + s] = t;
        }
        if (bad) *dst.flag = 1;
    }
}

// One thread per sample column folds the chunk's workgroup records, in block order, into the running best (bestv, bestt: value, row
// index in the call's Xs) that stays on the device across chunks; `first`: the running best starts empty.  t0: the chunk's first row.
__global__ __launch_bounds__(256) void sample_argmax_merge_kernel(const double* __restrict__ pv, const long long* __restrict__ pt, int nblocks,
                                                                  int nsamp, int64_t t0, int first, int minimize, double* __restrict__ bestv,
                                                                  long long* __restrict__ bestt) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nsamp) return;
    const bool mini = minimize != 0;
    double v = first ? 0.0 : bestv[s];
    long long t = first ? -1 : bestt[s];
#pragma unroll 8
    for (int b = 0; b < nblocks; ++b) {
        const double cv = pv[(int64_t)b * nsamp + s];
        const long long cl = pt[(int64_t)b * nsamp + s], ct = cl < 0 ? -1 : t0 + cl;
        if (argmax_beats(cv, ct, v, t, mini)) { v = cv; t = ct; }
    }
    bestv[s] = v;
    bestt[s] = t;
}

// the epilogue of the product, in place on the chunk's N x nsamp block (fp64): + sqrt(kappa) eps[t0 + n][s] (noise), then the y scaler's
// backward transform (ymode >= 0)
__global__ __launch_bounds__(256) void sample_post_kernel(double* __restrict__ out, int64_t total, int nsamp, int64_t t0, uint64_t seed,
                                                          int noise, int ymode, const double* __restrict__ ysp, const Scal* __restrict__ sc) {
    const double sk = sqrt(sc->kappa);
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t n = e / nsamp;
        const int s = (int)(e - n * nsamp);
        double v = out[e];
        if (noise) v += sk * sample_normal((uint64_t)(t0 + n), s, seed, 1);
        if (ymode >= 0) v = y_backward(v, ymode, ysp);
        out[e] = v;
    }
}

// 16-wide column tiles of the next launch for `rem` tiles left: the largest of 8 (fp64) or 4 (fp32), 2, 1 that fits -- the launches
// cover exactly round_up(nsamp, 16) columns
template <typename T> static int sample_tiles(int rem) {
    const int top = sizeof(T) == 4 ? 4 : 8;
    return rem >= top ? top : (rem >= 4 ? 4 : (rem >= 2 ? 2 : 1));
}

// the launch plan of Phi* W, shared by both epilogues (dst: double* or SampleArgmaxOut)
template <typename T, typename Out>
static void sample_launches(const Geom& g, const T* Phi, const T* Wt, int nsamp, Out dst, hipStream_t st) {
    static_assert(sample_block_rows(sizeof(T)) == 4 * 16 * (sizeof(T) == 4 ? 2 : 1), "rows per workgroup: 4 waves x 16 TM");
    const dim3 grid((unsigned)sample_blocks(g.Np, sizeof(T)));          // Np (a multiple of 256) is covered exactly
    const int ldw = sample_w_cols(nsamp), Kq = (int)round_up(g.K, 16);
    for (int rem = (nsamp + 15) / 16, s0 = 0; rem > 0;) {
        const int p = sample_tiles<T>(rem);
        const auto args = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, Phi, Wt, ldw, s0, Kq, g.Kp, g.N, nsamp, dst);
        };
        if (p == 8) args(sample_fw_kernel<T, sizeof(T) == 4 ? 4 : 8, Out>);      // p == 8 in fp64 only
        else if (p == 4) args(sample_fw_kernel<T, 4, Out>);
        else if (p == 2) args(sample_fw_kernel<T, 2, Out>);
        else args(sample_fw_kernel<T, 1, Out>);
        s0 += 16 * p; rem -= p;
    }
}

template <typename T>
void sample_product(const Geom& g, const T* Phi, const T* Wt, int nsamp, int64_t t0, uint64_t seed, int noise, int ymode, const double* ysp,
                    const Scal* sc, double* out, hipStream_t st) {
    sample_launches<T>(g, Phi, Wt, nsamp, out, st);
    if (noise || ymode >= 0)
        hipLaunchKernelGGL(sample_post_kernel, dim3(2048), dim3(256), 0, st, out, g.N * nsamp, nsamp, t0, seed, noise, ymode, ysp, sc);
}

template <typename T>
void sample_argmax_product(const Geom& g, const T* Phi, const T* Wt, int nsamp, const double* w, int minimize, int64_t t0, int first,
                           const SampleArgmaxBufs& b, hipStream_t st) {
    sample_launches<T>(g, Phi, Wt, nsamp, SampleArgmaxOut{w, b.pv, b.pt, b.flag, minimize}, st);
    hipLaunchKernelGGL(sample_argmax_merge_kernel, dim3((unsigned)((nsamp + 255) / 256)), dim3(256), 0, st, b.pv, b.pt,
                       (int)sample_blocks(g.Np, sizeof(T)), nsamp, t0, first, minimize, b.bestv, b.bestt);
}
// the y scaler's backward transform of the nsamp winning values, by the kernel that applies it to scfgp_sample's block: the same bits
void sample_argmax_finalize(double* bestv, int nsamp, int ymode, const double* ysp, const Scal* sc, hipStream_t st) {
    hipLaunchKernelGGL(sample_post_kernel, dim3(4), dim3(256), 0, st, bestv, (int64_t)nsamp, nsamp, (int64_t)0, (uint64_t)0, 0, ymode, ysp, sc);
}

template void sample_weights<double>(const Geom&, const double*, const double*, const Scal*, int, uint64_t, double*, double*, double*, hipStream_t);
template void sample_weights<float>(const Geom&, const double*, const double*, const Scal*, int, uint64_t, double*, double*, float*, hipStream_t);
template void sample_product<double>(const Geom&, const double*, const double*, int, int64_t, uint64_t, int, int, const double*, const Scal*,
                                     double*, hipStream_t);
template void sample_product<float>(const Geom&, const float*, const float*, int, int64_t, uint64_t, int, int, const double*, const Scal*,
                                    double*, hipStream_t);
template void sample_argmax_product<double>(const Geom&, const double*, const double*, int, const double*, int, int64_t, int,
                                            const SampleArgmaxBufs&, hipStream_t);
template void sample_argmax_product<float>(const Geom&, const float*, const float*, int, const double*, int, int64_t, int,
                                           const SampleArgmaxBufs&, hipStream_t);
