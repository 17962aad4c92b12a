// Greedy Monte-Carlo batch expected improvement over a pool (scfgp_select_qei; formulas in include/scfgp_hip.h).  F (T x nsamp, fp64,
// row pitch nsamp) holds scfgp_sample's values of the pool, written by sample_fw_kernel's store epilogue; m (nsamp) is the running
// per-sample maximum of b, the pending rows and the picks so far, in units u = sgn f.  A pick is two launches:
//     selectqei_sweep_kernel   score_t = (1 / nsamp) sum_s max(sgn F[t][s] - m_s, 0) of every row, and per workgroup the best eligible,
//                              untaken (score, row) record by argmax.h's rule: one read of F, nothing else of size T x nsamp
//     selectqei_commit_kernel  one workgroup folds the records, writes idx[j] and gain[j], marks the row taken in the device copy of w
//                              and raises m to the picked row's values
// selectqei_state_kernel forms the start m and the two q-EI sums, each summed by one thread in sample order.
#include "kernels.h"
#include "argmax.h"

constexpr int QEI_BLOCK_ROWS = 128;                               // rows per workgroup of the sweep: one record each
int selectqei_blocks(int64_t T) { return (int)((T + QEI_BLOCK_ROWS - 1) / QEI_BLOCK_ROWS); }
// the lane group that sums a row: a function of nsamp alone, so a row's score does not depend on T, its position or the grid
static int selectqei_group(int nsamp) { return nsamp <= 64 ? 16 : 64; }

// A group of G lanes per row, 256 / G rows at a time (consecutive rows: a wave's loads are runs of G doubles, 8-byte aligned whatever
// the pitch is).  Lane g adds s = g, g + G, .. in ascending order, a xor butterfly from G / 2 down to 1 leaves the row's sum in every
// lane of the group, then one division by nsamp.  A term that is not > 0 (a NaN among them) counts as 0.  FIRST (pick 0): score0 of
// every row, and the flag where an eligible row holds a non-finite value.
template <int G, bool FIRST>
__global__ __launch_bounds__(256) void selectqei_sweep_kernel(const double* __restrict__ F, const double* __restrict__ w,
                                                              const double* __restrict__ ms, int64_t T, int nsamp, double sgn,
                                                              double* __restrict__ score0, double* __restrict__ pval,
                                                              long long* __restrict__ pidx, int* __restrict__ flag) {
    constexpr int NG = 256 / G;
    __shared__ double sm[1024];
    __shared__ double gv[NG];
    __shared__ long long gt[NG];
    for (int s = threadIdx.x; s < nsamp; s += 256) sm[s] = ms[s];
    __syncthreads();
    const int grp = threadIdx.x / G, g = threadIdx.x % G;
    const int64_t base = (int64_t)blockIdx.x * QEI_BLOCK_ROWS;
    const double dn = (double)nsamp;
    double bv = 0.0;
    long long bt = -1;
    bool bad = false;
    for (int k = 0; k < QEI_BLOCK_ROWS / NG; ++k) {
        const int64_t t = base + k * NG + grp;                    // the same for the G lanes of a group
        const bool live = t < T, eligible = live && w[t] > 0.0;
        double acc = 0.0;
        if (live) {
            const double* __restrict__ row = F + t * nsamp;
#pragma unroll 4
            for (int s = g; s < nsamp; s += G) {
                const double f = row[s];
                if (FIRST && eligible) bad |= !isfinite(f);
                const double d = sgn * f - sm[s];                 // sgn = +-1: the product is exact
                acc += d > 0.0 ? d : 0.0;
            }
        }
#pragma unroll
        for (int off = G / 2; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, G);
        const double score = acc / dn;
        if (FIRST && live && g == 0) score0[t] = score;
        if (eligible && argmax_beats(score, t, bv, bt, false)) { bv = score; bt = t; }
    }
    if (g == 0) { gv[grp] = bv; gt[grp] = bt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = gv[0];
        long long t = gt[0];
#pragma unroll
        for (int i = 1; i < NG; ++i)
            if (argmax_beats(gv[i], gt[i], v, t, false)) { v = gv[i]; t = gt[i]; }
        pval[blockIdx.x] = v;
        pidx[blockIdx.x] = t;
    }
    if (FIRST && bad) *flag = 1;
}

// One workgroup: thread i folds a run of consecutive records, thread 0 the 256 runs in order; idx[j], gain[j], w[p] = 0, and
// m_s <- max(m_s, sgn F[p][s]).  No record (never with m <= the eligible rows): idx[j] = -1 and m stays.
__global__ __launch_bounds__(256) void selectqei_commit_kernel(const double* __restrict__ F, const double* __restrict__ pval,
                                                               const long long* __restrict__ pidx, int nblocks, int nsamp, double sgn, int j,
                                                               double* __restrict__ w, double* __restrict__ ms, long long* __restrict__ idx,
                                                               double* __restrict__ gain) {
    __shared__ double sv[256];
    __shared__ long long sl[256];
    __shared__ long long picked;
    const int per = (nblocks + 255) / 256, b0 = threadIdx.x * per, b1 = min(b0 + per, nblocks);
    double v = 0.0;
    long long t = -1;
    for (int b = b0; b < b1; ++b)
        if (argmax_beats(pval[b], pidx[b], v, t, false)) { v = pval[b]; t = pidx[b]; }
    sv[threadIdx.x] = v; sl[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 256; ++i)
            if (argmax_beats(sv[i], sl[i], v, t, false)) { v = sv[i]; t = sl[i]; }
        idx[j] = t;
        gain[j] = t < 0 ? 0.0 : v;
        if (t >= 0) w[t] = 0.0;
        picked = t;
    }
    __syncthreads();
    const long long p = picked;
    if (p < 0) return;
    for (int s = threadIdx.x; s < nsamp; s += 256) {
        const double u = sgn * F[p * nsamp + s];
        if (u > ms[s]) ms[s] = u;
    }
}

// start != 0: m_s = max(base, sgn pend[s]) (pend: the pending rows' per-sample best values, NULL: none) is written first.  Then
// *out = (1 / nsamp) sum_s (m_s - base), added by one thread in sample order.
__global__ __launch_bounds__(256) void selectqei_state_kernel(const double* __restrict__ pend, double base, double sgn, int nsamp, int start,
                                                              double* __restrict__ ms, double* __restrict__ out) {
    __shared__ double sm[1024];
    for (int s = threadIdx.x; s < nsamp; s += 256) {
        double v = ms[s];
        if (start) {
            v = base;
            if (pend) { const double u = sgn * pend[s]; if (u > v) v = u; }
            ms[s] = v;
        }
        sm[s] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (int s = 0; s < nsamp; ++s) acc += sm[s] - base;
        *out = acc / (double)nsamp;
    }
}

void selectqei_state(const SelectQeiBufs& b, const double* pend, double base, int start, hipStream_t st) {
    hipLaunchKernelGGL(selectqei_state_kernel, dim3(1), dim3(256), 0, st, pend, base, b.sgn, b.nsamp, start, b.ms, b.qei + (start ? 0 : 1));
}

void selectqei_sweep(const SelectQeiBufs& b, int j, hipStream_t st) {
    const dim3 grid((unsigned)selectqei_blocks(b.T));
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, b.F, b.w, b.ms, b.T, b.nsamp, b.sgn, b.score0, b.pval, b.pidx, b.flag);
    };
    if (selectqei_group(b.nsamp) == 16) { if (j == 0) launch(selectqei_sweep_kernel<16, true>); else launch(selectqei_sweep_kernel<16, false>); }
    else { if (j == 0) launch(selectqei_sweep_kernel<64, true>); else launch(selectqei_sweep_kernel<64, false>); }
}

void selectqei_commit(const SelectQeiBufs& b, int j, hipStream_t st) {
    hipLaunchKernelGGL(selectqei_commit_kernel, dim3(1), dim3(256), 0, st, b.F, b.pval, b.pidx, selectqei_blocks(b.T), b.nsamp, b.sgn, j, b.w,
                       b.ms, b.idx, b.gain);
}
