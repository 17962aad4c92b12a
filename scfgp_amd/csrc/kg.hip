// Knowledge gradient over a pool (scfgp_acquire_kg; definitions, guarantees and errors in include/scfgp_hip.h).  With candidates i,
// reference rows r, d_r = u_r - max u <= 0 and b_ir = kappa <Li phi(x_i), Li phi(x_r)> / sigma_i, the caller's nodes z_1 < .. < z_J give
//     m_ij = max_r (d_r + b_ir z_j)      s_ij = b_ir at the maximiser (ties: lowest r)      bmin_i, bmax_i = min_r, max_r b_ir
// and from these two closed-form numbers per candidate, kg <= KG_i <= kg_hi (kg_finish_kernel).  b_ir is an element of predcov's
// product: the kernel below is predcov_kernel with the node reduction in the place of its store, so the T x R matrix never exists.
#include "kernels.h"
#include "tile_engine.h"
#include "apply_epilogue.h"                                       // dpp_mov_f64: a 16-lane row group is one DPP row
#include "acquire_math.h"                                         // norm_h; contraction off from here on

// The node arithmetic is fp64 and written without contraction: t = b z, then d + t, two roundings (as predcov's epilogue adds its
// kappa), so that numpy restates m and s bit for bit (tests/kg_ref.py: node_table).
#pragma clang fp contract(off)

constexpr int KG_TILE = 128;
constexpr int KG_FLUSH = 128;                                     // predcov's PREDCOV_FLUSH: the fp32 sums must have predict_cov's bits

// One workgroup, after the reference job's apply_predict: u_r = sgn mu_r from the chunk's partials in rowstats_kernel<1>'s order (so
// u has scfgp_predict's bits), u* = max_r u_r (exact and order-free), d_r = u_r - u* for r < R and 0 up to Rp; zf = [z (32) | h(-|z_j|)
// (32)], the per-call constants of the upper bound.  flag[1] = 1: a non-finite u_r.
__global__ __launch_bounds__(1024) void kg_ref_kernel(const double* __restrict__ mupart, int njt, int64_t Np, int64_t R, int64_t Rp, double sgn,
                                                      const double* __restrict__ z, int J, double* __restrict__ d, double* __restrict__ zf,
                                                      int* __restrict__ flag) {
    __shared__ double s_max[16];
    const int tid = threadIdx.x;
    const auto u_of = [&](int64_t n) {
        double mu = 0;
        for (int t = 0; t < njt; ++t) mu += mupart[(int64_t)t * Np + n];
        return sgn * mu;
    };
    double best = -INFINITY;
    for (int64_t n = tid; n < R; n += 1024) {
        const double u = u_of(n);
        if (!isfinite(u)) flag[1] = 1;
        best = fmax(best, u);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) best = fmax(best, __shfl_xor(best, off));
    if ((tid & 63) == 0) s_max[tid >> 6] = best;
    __syncthreads();
    double ustar = s_max[0];
    for (int k = 1; k < 16; ++k) ustar = fmax(ustar, s_max[k]);
    for (int64_t n = tid; n < Rp; n += 1024) d[n] = n < R ? u_of(n) - ustar : 0.0;
    if (tid < 32) {
        const double zj = tid < J ? z[tid] : 0.0;
        zf[tid] = zj; zf[32 + tid] = norm_h(-fabs(zj));
    }
}

// sigma of the chunk's candidates from its partials, with acquire_rows_kernel's arithmetic (scfgp_acquire's sd bit for bit); all Np rows
__global__ __launch_bounds__(256) void kg_sigma_kernel(const double* __restrict__ vpart, int njt, const Scal* __restrict__ sc, int64_t Np,
                                                       int noise, double* __restrict__ sd_o) {
    const double kappa = sc->kappa;
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < Np; n += (int64_t)gridDim.x * 256) {
        double v = 0;
        for (int t = 0; t < njt; ++t) v += vpart[(int64_t)t * Np + n];
        const double dd = noise ? kappa * (v + 1.0) : kappa * v;
        sd_o[n] = sqrt(dd);
    }
}

// A pair (a, b) of every lane merged over the 16 lanes of its DPP row (the lanes that hold one output row of a 16 x 16 MFMA tile), the
// result in every lane: two quad permutes, row_half_mirror, row_mirror -- apply_epilogue.h's row16_sum with `merge` in the place of
// its +.  merge must be commutative and associative (max / min; larger value, then lower column: a total order on distinct columns).
template <int CTRL> __device__ __forceinline__ double kg_dpp(double x) { return dpp_mov_f64<CTRL>(x); }
template <int CTRL> __device__ __forceinline__ int kg_dpp(int x) { return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, true); }
template <typename B, typename F> __device__ __forceinline__ void kg_row16(double& a, B& b, F merge) {
    merge(a, b, kg_dpp<0xB1>(a), kg_dpp<0xB1>(b));                // quad_perm [1,0,3,2]
    merge(a, b, kg_dpp<0x4E>(a), kg_dpp<0x4E>(b));                // quad_perm [2,3,0,1]
    merge(a, b, kg_dpp<0x141>(a), kg_dpp<0x141>(b));              // row_half_mirror
    merge(a, b, kg_dpp<0x140>(a), kg_dpp<0x140>(b));              // row_mirror
}

// The fused product.  predcov_kernel's 128 x 128 tile, LDS images (slot s of row r at s ^ ((r >> 1) & 7), two buffers per operand) and k
// loop: an element's sum is formed by the same MFMA steps in the same order, fp32 flushed into fp64 every KG_FLUSH features, so
// kappa x sum has scfgp_predict_cov's bits.  The four waves are stacked 4 x 1 (32 rows x 128 columns each, 2 x 8 MFMA tiles) where
// predcov has 2 x 2: the 16 lanes of a row group then hold all 128 columns of their row, a wave owns its 32 rows of the node state,
// and the epilogue needs no barrier.  blockIdx.y: the 128-row strip of candidates; blockIdx.x: a contiguous run of tps column tiles
// of the reference rows (the column split).
// Epilogue per tile, per row of the lane (8) and node: the lane's 8 columns in rising order (strict >: the lowest column wins a tie),
// then (value, column) through kg_row16 over the row group's 16 lanes (larger value, then lower column), and the lane that holds the
// winner updates the strip's LDS state [128][J] of (m, s) where its value is strictly larger: tiles are walked in rising column
// order, so a tie keeps the lowest r.  bmin / bmax likewise.  Rows >= nrows compute on whatever the padding holds and are never read;
// columns >= R take no part.  Dynamic LDS: 64 KB of operand images + 128 J 16 B of state + 3 KB (at J = 32: 131 KB of the CU's 160).
// Output: the strip's state per split, st_m / st_s [row][split][J] and st_b [row][split][2]; kg_finish_kernel merges the splits in
// order by the same strict >, so the result is that of one walk over all columns whatever the split.
template <typename T>
__global__ __launch_bounds__(256) void kg_node_kernel(const T* __restrict__ Ca, const T* __restrict__ Cb, int Kp, int nkt, int64_t R, int ntiles,
                                                      int tps, const double* __restrict__ dref, const double* __restrict__ sd,
                                                      const double* __restrict__ zf, int J, const Scal* __restrict__ sc,
                                                      double* __restrict__ st_m, double* __restrict__ st_s, double* __restrict__ st_b) {
    typedef MT<T, 16> M;
    typedef typename Vec16<T>::type vec_t;                       // one 16-byte slot
    constexpr bool F32 = sizeof(T) == 4;
    constexpr int VN = Vec16<T>::N, BK = 8 * VN;                 // features per slot, per k-tile
    constexpr int SLOTS = KG_TILE * 8;                           // 16-byte slots of one panel image
    constexpr int FLUSH_KT = KG_FLUSH / BK;
    extern __shared__ __attribute__((aligned(16))) char kg_smem[];
    vec_t* lds = reinterpret_cast<vec_t*>(kg_smem);              // [buffer][operand][SLOTS]
    double* s_m = reinterpret_cast<double*>(kg_smem + 4 * SLOTS * 16);   // [128][J]
    double* s_s = s_m + KG_TILE * J;                              // [128][J]
    double* s_b = s_s + KG_TILE * J;                              // [128][2]: bmin, bmax
    double* s_sd = s_b + 2 * KG_TILE;                             // [128]
    double* s_z = s_sd + KG_TILE;                                 // [32]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
    const int wm = wave * 32;
    const int64_t r0 = (int64_t)blockIdx.y * KG_TILE;
    const int split = blockIdx.x, nsplit = gridDim.x;
    const int ct0 = split * tps, ct1 = min(ct0 + tps, ntiles);

    // the wave's rows of the state, sigma of the strip, the nodes
    for (int e = lane; e < 32 * J; e += 64) { s_m[wm * J + e] = -INFINITY; s_s[wm * J + e] = 0.0; }
    if (lane < 32) { s_b[2 * (wm + lane)] = INFINITY; s_b[2 * (wm + lane) + 1] = -INFINITY; }
    if (tid < KG_TILE) s_sd[tid] = sd[r0 + tid];
    if (tid < 32) s_z[tid] = zf[tid];

    // staging: thread t moves slot t % 8 of rows t / 8 + 32 j of both panels (8 lanes: one 128-byte row segment)
    const int srow = tid >> 3, sslot = tid & 7;
    const vec_t* __restrict__ ga = reinterpret_cast<const vec_t*>(Ca + (r0 + srow) * Kp) + sslot;
    const int64_t gstep = (int64_t)32 * Kp / VN;                 // 32 rows, in slots
    int soff[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = srow + 32 * j;
        soff[j] = r * 8 + (sslot ^ ((r >> 1) & 7));
    }
    // fragment reads: rows wm + 16 t + i of A, 16 t + i of B (the XOR of a row is that of i: wm and 16 t are multiples of 16)
    const int aoff = (wm + i) * 8, boff = i * 8, swz = (i >> 1) & 7;
    const double kappa = sc->kappa;

    for (int ct = ct0; ct < ct1; ++ct) {
        const int64_t c0 = (int64_t)ct * KG_TILE;
        const vec_t* __restrict__ gb = reinterpret_cast<const vec_t*>(Cb + (c0 + srow) * Kp) + sslot;
        vec_t pa[4], pb[4];
        auto fetch = [&](int kt) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { pa[j] = ga[j * gstep + kt * 8]; pb[j] = gb[j * gstep + kt * 8]; }
        };
        auto stage = [&](int buf) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { lds[(buf * 2 + 0) * SLOTS + soff[j]] = pa[j]; lds[(buf * 2 + 1) * SLOTS + soff[j]] = pb[j]; }
        };
        typename M::acc_t acc[2][8];
        double part[2][8][4];                                    // fp32 only
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int tn = 0; tn < 8; ++tn)
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
                vec_t a[2], b[8];
#pragma unroll
                for (int t = 0; t < 2; ++t) a[t] = lds[(buf * 2 + 0) * SLOTS + aoff + 128 * t + ((q + 4 * h) ^ swz)];
#pragma unroll
                for (int t = 0; t < 8; ++t) b[t] = lds[(buf * 2 + 1) * SLOTS + boff + 128 * t + ((q + 4 * h) ^ swz)];
#pragma unroll
                for (int e = 0; e < VN; ++e)
#pragma unroll
                    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                        for (int tn = 0; tn < 8; ++tn) M::mfma(acc[tm][tn], a[tm][e], b[tn][e]);
            }
            if (F32 && ((kt + 1) % FLUSH_KT == 0 || kt + 1 == nkt)) {
#pragma unroll
                for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                    for (int tn = 0; tn < 8; ++tn)
#pragma unroll
                        for (int r = 0; r < 4; ++r) { part[tm][tn][r] += (double)acc[tm][tn][r]; acc[tm][tn][r] = 0; }
            }
            // the other buffer was last read before the barrier that ended tile kt - 1
            if (kt + 1 < nkt) stage(buf ^ 1);
            __syncthreads();
        }

        // ---- node epilogue ----
        double dcol[8];
        bool live[8];
#pragma unroll
        for (int tn = 0; tn < 8; ++tn) {
            const int64_t j = c0 + 16 * tn + i;
            live[tn] = j < R;
            dcol[tn] = live[tn] ? dref[j] : 0.0;
        }
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rl = wm + 16 * tm + M::crow(lane, r);
                const double sig = s_sd[rl];
                double b[8], lo = INFINITY, hi = -INFINITY;
#pragma unroll
                for (int tn = 0; tn < 8; ++tn) {
                    // kappa x sum: scfgp_predict_cov's element; then / sigma_i
                    const double num = kappa * (F32 ? part[tm][tn][r] : (double)acc[tm][tn][r]);
                    b[tn] = num / sig;
                    if (live[tn]) { lo = fmin(lo, b[tn]); hi = fmax(hi, b[tn]); }
                }
                kg_row16(lo, hi, [](double& a, double& c, double oa, double oc) { a = fmin(a, oa); c = fmax(c, oc); });
                if (i == 0) {
                    s_b[2 * rl] = fmin(s_b[2 * rl], lo);
                    s_b[2 * rl + 1] = fmax(s_b[2 * rl + 1], hi);
                }
                for (int j = 0; j < J; ++j) {
                    const double zj = s_z[j];
                    double best = -INFINITY, bs = 0.0;
                    int mine = 128;                              // the lane's winning column within the tile; 128: none
#pragma unroll
                    for (int tn = 0; tn < 8; ++tn) {
                        const double t = b[tn] * zj;
                        const double cand = dcol[tn] + t;
                        if (live[tn] && cand > best) { best = cand; bs = b[tn]; mine = 16 * tn + i; }
                    }
                    double gv = best;
                    int gc = mine;
                    kg_row16(gv, gc, [](double& v, int& c, double ov, int oc) { if (ov > v || (ov == v && oc < c)) { v = ov; c = oc; } });
                    if (mine < 128 && mine == gc && best > s_m[rl * J + j]) { s_m[rl * J + j] = best; s_s[rl * J + j] = bs; }
                }
            }
        // the next tile's first barrier (or the one below) orders this tile's state updates before the next reads of them
    }
    __syncthreads();
    for (int e = tid; e < KG_TILE * J; e += 256) {
        const int rl = e / J, j = e - rl * J;
        const int64_t o = ((r0 + rl) * nsplit + split) * J + j;
        st_m[o] = s_m[e]; st_s[o] = s_s[e];
    }
    for (int e = tid; e < 2 * KG_TILE; e += 256) st_b[((r0 + (e >> 1)) * nsplit + split) * 2 + (e & 1)] = s_b[e];
}

// One thread per candidate: the splits merged in order (strict >: the lowest r keeps a tie), then the two sums.
//   kg: the expected maximum of the J tangents (m_j, s_j).  Their slopes do not decrease (the envelope is convex); a slope that is not
//       larger than the last kept one merges with it.  The tangents kept at nodes j' < j cross at c = (icpt' - icpt_j) / (s_j - s'),
//       icpt = m - s z, clamped into [z_{j-1}, z_j] where it lies in exact arithmetic; kg = sum (s_j - s') h(-|c|).
//   kg_hi: the chord interpolant through (z_j, m_j), continued by bmin and bmax: sum_j max(q_j - q_{j-1}, 0) h(-|z_j|) with q_j the
//       chord slope over [z_j, z_{j+1}], clamped into [s_j, s_{j+1}] where it lies in exact arithmetic (a chord of a convex function
//       between its end slopes; with one reference row every q is then b itself and the sum is 0 exactly), q_0 = bmin, q_J = bmax.
// Every term is >= 0.  m_o, s_o (N x J, may be NULL): the node table.
__global__ __launch_bounds__(256) void kg_finish_kernel(const double* __restrict__ st_m, const double* __restrict__ st_s,
                                                        const double* __restrict__ st_b, int nsplit, int J, const double* __restrict__ zf,
                                                        int64_t N, double* __restrict__ kg_o, double* __restrict__ hi_o,
                                                        double* __restrict__ m_o, double* __restrict__ s_o) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const auto node = [&](int j, double& m, double& s) {
        m = st_m[(n * nsplit) * J + j]; s = st_s[(n * nsplit) * J + j];
        for (int p = 1; p < nsplit; ++p) {
            const double om = st_m[(n * nsplit + p) * J + j];
            if (om > m) { m = om; s = st_s[(n * nsplit + p) * J + j]; }
        }
        if (m_o) { m_o[n * J + j] = m; s_o[n * J + j] = s; }
    };
    double bmin = st_b[(n * nsplit) * 2], bmax = st_b[(n * nsplit) * 2 + 1];
    for (int p = 1; p < nsplit; ++p) {
        bmin = fmin(bmin, st_b[(n * nsplit + p) * 2]);
        bmax = fmax(bmax, st_b[(n * nsplit + p) * 2 + 1]);
    }
    double mp, sp;                                                // node j - 1
    node(0, mp, sp);
    double sk = sp, ik = mp - sp * zf[0];                         // the last tangent kept
    double qp = bmin, kg = 0.0, hi = 0.0;
    for (int j = 1; j < J; ++j) {
        double mj, sj;
        node(j, mj, sj);
        const double zl = zf[j - 1], zr = zf[j];
        double qj = (mj - mp) / (zr - zl);
        qj = fmin(fmax(qj, sp), sj);
        hi += fmax(qj - qp, 0.0) * zf[32 + j - 1];
        qp = qj;
        if (sj > sk) {
            const double ij = mj - sj * zr;
            double c = (ik - ij) / (sj - sk);
            c = fmin(fmax(c, zl), zr);
            kg += (sj - sk) * norm_h(-fabs(c));
            sk = sj; ik = ij;
        }
        mp = mj; sp = sj;
    }
    hi += fmax(bmax - qp, 0.0) * zf[32 + J - 1];
    kg_o[n] = kg; hi_o[n] = hi;
}

// rows x splits of the largest launch: 128 nstrips nsplit <= 128 max(nstrips, 512), nstrips <= 256
int64_t kg_state_rows() { return 128 * 512; }

// the column split of a chunk of N candidates against R reference rows: about 512 workgroups where the strips alone give fewer; returns
// the number of splits, *tps = column tiles per split (no split is empty)
static int kg_plan(int64_t N, int64_t R, int* tps) {
    const int nstrips = (int)((N + KG_TILE - 1) / KG_TILE), ntiles = (int)((R + KG_TILE - 1) / KG_TILE);
    const int want = std::min(ntiles, std::max(1, 512 / nstrips));
    *tps = (ntiles + want - 1) / want;
    return (ntiles + *tps - 1) / *tps;
}

void kg_reference(int njt, const double* mupart, int64_t Np, int64_t R, int minimize, const double* z, int J, double* d, double* zf, int* flag,
                  hipStream_t st) {
    hipLaunchKernelGGL(kg_ref_kernel, dim3(1), dim3(1024), 0, st, mupart, njt, Np, R, round_up(R, KG_TILE), minimize ? -1.0 : 1.0, z, J, d, zf,
                       flag);
}

void kg_sigma(const Geom& g, int njt, const double* vpart, const Scal* sc, int noise, double* sd, hipStream_t st) {
    hipLaunchKernelGGL(kg_sigma_kernel, dim3((unsigned)(g.Np / 256)), dim3(256), 0, st, vpart, njt, sc, g.Np, noise, sd);
}

template <typename T>
void kg_nodes(const Geom& g, const T* Ca, const T* Cb, int64_t R, int J, const KgBufs& b, const Scal* sc, hipStream_t st) {
    constexpr int BK = 8 * Vec16<T>::N;
    const int nkt = (int)(round_up(g.K, BK) / BK);               // <= Kp / BK: Kp is a multiple of 128
    const int ntiles = (int)((R + KG_TILE - 1) / KG_TILE), nstrips = (int)((g.N + KG_TILE - 1) / KG_TILE);
    int tps;
    const int nsplit = kg_plan(g.N, R, &tps);
    const int lds_bytes = 4 * KG_TILE * 8 * 16 + (int)sizeof(double) * (2 * KG_TILE * J + 3 * KG_TILE + 32);
    allow_big_lds(kg_node_kernel<T>, lds_bytes);
    hipLaunchKernelGGL(kg_node_kernel<T>, dim3(nsplit, nstrips), dim3(256), lds_bytes, st, Ca, Cb, g.Kp, nkt, R, ntiles, tps, b.d, b.sd, b.zf, J,
                       sc, b.st_m, b.st_s, b.st_b);
    hipLaunchKernelGGL(kg_finish_kernel, dim3((unsigned)((g.N + 255) / 256)), dim3(256), 0, st, b.st_m, b.st_s, b.st_b, nsplit, J, b.zf, g.N, b.kg,
                       b.kg_hi, b.m, b.s);
}

template void kg_nodes<double>(const Geom&, const double*, const double*, int64_t, int, const KgBufs&, const Scal*, hipStream_t);
template void kg_nodes<float>(const Geom&, const float*, const float*, int64_t, int, const KgBufs&, const Scal*, hipStream_t);
