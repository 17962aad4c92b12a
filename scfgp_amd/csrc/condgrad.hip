// Observation rows of derivative observations (scfgp_condition_grad; derivation in include/scfgp_hip.h and DESIGN 4.20).
//   grad f(x) = J(x)^T w is linear in the weights, so "d f / d x_d at x_t was observed as G with noise kappa / rho" is a linear
//   observation of w with the row and the target
//     psi = sqrt(rho) g_t[d] (-phi_s o Fall[d, :] | phi_c o Fall[d, :])          sqrt(rho) G
//   (g_t: the X scaler's derivative factors of raw mode).  A point brings nb = nd (+ 1 with its value, whose row is phi_t itself) rows,
//   which are consecutive rows of the chunk (row t nb + i): the operand scfgp_condition's products read as Phi.
// The kernel is write-bound (np nb Kp elements out for np Kp in): a workgroup owns GO_PTS points and a slab of 256 x 16 bytes of
// columns, keeps the points' phi' in registers across the loop over the derivative rows, loads a row of Fall once for its points and
// stores 16 bytes per lane, a row's slab being one contiguous 4 KiB run.  A chunk has few points when nb is large (504 at nb = 65), so
// the derivative rows are also split into groups of GO_ROWS across the grid's z: without it the launch is 2 waves per SIMD at the
// headline shape.
#include "kernels.h"

constexpr int GO_PTS = 4;                       // points per workgroup
constexpr int GO_ROWS = 16;                     // derivative rows of a point per workgroup

template <typename T> struct GoVec;
template <> struct GoVec<double> { typedef double2 V; static constexpr int N = 2; };

template <typename T, int N> struct GoPack { T v[N]; };

// Phi (npts x Kp, typed): the features of the chunk's points.  Psi (nrows_pad x Kp, typed) and tg (nrows_pad): the observation rows and
// their targets; rows from npts nb on and the padding columns are zero.  grid: (ceil(npts / GO_PTS) + padding rows, column slabs,
// ceil(nd / GO_ROWS)); the value rows and the padding rows belong to z = 0.
template <typename T>
__global__ __launch_bounds__(256) void gradobs_rows_kernel(const T* __restrict__ Phi, const double* __restrict__ Fall,
                                                           const int* __restrict__ dims, const double* __restrict__ gfac,
                                                           const double* __restrict__ yv, const double* __restrict__ G,
                                                           const double* __restrict__ rho, int D, int J, int Jp, int Kp, int nd,
                                                           int64_t npts, T* __restrict__ Psi, double* __restrict__ tg) {
    typedef typename GoVec<T>::V V;
    constexpr int VN = GoVec<T>::N;
    const int hv = yv ? 1 : 0, nb = nd + hv;
    const int64_t nrows = npts * nb, ngroups = (npts + GO_PTS - 1) / GO_PTS;
    const int c0 = ((int)blockIdx.y * 256 + (int)threadIdx.x) * VN;          // the lane's VN columns: Kp is a multiple of 128
    const bool first = blockIdx.y == 0 && threadIdx.x == 0;                   // the lane that writes the targets
    auto store = [&](int64_t row, const GoPack<T, VN>& o) {
        V v;
        if constexpr (VN == 4) { v.x = o.v[0]; v.y = o.v[1]; v.z = o.v[2]; v.w = o.v[3]; }
        else { v.x = o.v[0]; v.y = o.v[1]; }
        *reinterpret_cast<V*>(Psi + row * Kp + c0) = v;
    };
    if (c0 >= Kp) return;                                                     // (the lane that writes the targets has column 0)
    if ((int64_t)blockIdx.x >= ngroups) {                                     // one padding row per workgroup
        if (blockIdx.z != 0) return;
        const int64_t r = nrows + ((int64_t)blockIdx.x - ngroups);
        GoPack<T, VN> z;
        for (int v = 0; v < VN; ++v) z.v[v] = (T)0;
        store(r, z);
        if (first) tg[r] = 0.0;
        return;
    }
    const int64_t t0 = (int64_t)blockIdx.x * GO_PTS;
    const int np = (int)(npts - t0 < GO_PTS ? npts - t0 : GO_PTS);
    // phi' = (-phi_s | phi_c) and phi at the lane's columns, and the column of Fall each of them meets
    double dp[GO_PTS][VN];
    T ph[GO_PTS][VN];
    int fc[VN];
    bool live[VN];
#pragma unroll
    for (int v = 0; v < VN; ++v) {
        const int c = c0 + v;
        live[v] = c < 2 * J;
        fc[v] = c < J ? c : (live[v] ? c - J : 0);
#pragma unroll
        for (int p = 0; p < GO_PTS; ++p) {
            dp[p][v] = 0.0; ph[p][v] = (T)0;
            if (p < np && live[v]) {
                const T* row = Phi + (t0 + p) * Kp;
                dp[p][v] = c < J ? -(double)row[J + c] : (double)row[c - J];
                ph[p][v] = row[c];
            }
        }
    }
    if (yv && blockIdx.z == 0) {                                              // the value rows: phi_t as it stands, target y_t
#pragma unroll
        for (int p = 0; p < GO_PTS; ++p) {
            if (p >= np) continue;
            const int64_t r = (t0 + p) * nb;
            GoPack<T, VN> o;
            for (int v = 0; v < VN; ++v) o.v[v] = ph[p][v];
            store(r, o);
            if (first) tg[r] = yv[t0 + p];
        }
    }
    const int j0 = (int)blockIdx.z * GO_ROWS, j1 = j0 + GO_ROWS < nd ? j0 + GO_ROWS : nd;
    for (int j = j0; j < j1; ++j) {
        const int d = dims ? dims[j] : j;
        double f[VN];
#pragma unroll
        for (int v = 0; v < VN; ++v) f[v] = live[v] ? Fall[(int64_t)d * Jp + fc[v]] : 0.0;
#pragma unroll
        for (int p = 0; p < GO_PTS; ++p) {
            if (p >= np) continue;
            const int64_t t = t0 + p, r = t * nb + hv + j;
            const double rh = rho ? rho[t * nd + j] : 1.0;
            const double sq = sqrt(rh);                                        // sqrt(1) = 1: rho of all ones has rho == NULL's bits
            const double s = gfac ? sq * gfac[t * D + d] : sq;
            GoPack<T, VN> o;
#pragma unroll
            for (int v = 0; v < VN; ++v) o.v[v] = rh == 0.0 || !live[v] ? (T)0 : (T)(dp[p][v] * f[v] * s);   // fp64, rounded once
            store(r, o);
            if (first) tg[r] = rh == 0.0 ? 0.0 : sq * G[t * nd + j];           // rho = 0: exact zeros whatever G holds
        }
    }
}

template <typename T>
void gradobs_rows(const Geom& gr, const Geom& g, const T* Phi, const double* Fall, const GradObs& a, T* Psi, double* tg, hipStream_t st) {
    constexpr int VN = GoVec<T>::N;
    const int64_t nb = a.nd + (a.y ? 1 : 0), ngroups = (g.N + GO_PTS - 1) / GO_PTS, npad = gr.Np - g.N * nb;
    const dim3 grid((unsigned)(ngroups + npad), (unsigned)((g.Kp + 256 * VN - 1) / (256 * VN)), (unsigned)((a.nd + GO_ROWS - 1) / GO_ROWS));
    hipLaunchKernelGGL(gradobs_rows_kernel<T>, grid, dim3(256), 0, st, Phi, Fall, a.dims, a.gfac, a.y, a.G, a.rho, g.D, g.J, g.Jp, g.Kp, a.nd,
                       g.N, Psi, tg);
}

// the update's first pass is fp64 in every context (api_update.hip: scfgp_condition_grad), so this is the instantiation that runs
template void gradobs_rows<double>(const Geom&, const Geom&, const double*, const double*, const GradObs&, double*, double*, hipStream_t);
