// The Gram part that loo_block_kernel (loo.hip) and gradcov_block_kernel (gradcov.hip) share: H = C C^T of a GROUP of at most 64
// consecutive rows of C (typed, ld Kp), restricted to the diagonal b x b blocks of the group, as a 64 x 64 fp64 image in LDS.
//
// A workgroup of 4 waves owns the group.  H is formed by fp64 MFMA (16 x 16 x 4) from the rows of C, converted on load in fp32 contexts;
// only the 16 x 16 tiles of its lower half that meet a diagonal b x b block are multiplied.  The Kp features are dealt to the waves in
// quarters; inside its quarter lane (i, q) reads the 16-byte slots q, q + 4, .. of row i of each of the four 16-row fragments (the four
// lanes of a row read 64 consecutive bytes), and MFMA step e pairs the e-th elements of the lanes' slots: a permutation of the
// reduction index that both operands share.  The waves add their tiles into the LDS image one after the other, so an entry's sum has one
// order whatever the group, the chunk or the call.  Rows from `live` on are never loaded: their rows of H are zero.
#pragma once
#include "tile_engine.h"

constexpr int BLOCK_GRAM_LD = 65;               // doubles per row of the LDS image (a lane's own row and a column across lanes are
                                                // both conflict-free)

// Hs: 64 x BLOCK_GRAM_LD doubles of LDS.  g0: first row of the group, live: its live rows (>= 1), b: rows per diagonal block.  All 256
// threads call it; it ends behind a workgroup barrier with the image complete (entries outside the multiplied tiles are zero).
template <typename T>
__device__ __forceinline__ void block_gram(const T* __restrict__ C, int Kp, int64_t g0, int live, int b, double* __restrict__ Hs) {
    typedef MT<double, 16> M;
    typedef typename Vec16<T>::type vec_t;
    constexpr int VN = Vec16<T>::N;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;

    for (int x = tid; x < 64 * BLOCK_GRAM_LD; x += 256) Hs[x] = 0.0;

    // lower 16 x 16 tiles (tm, tn <= tm) that meet a diagonal block: the first row of tm and the last row of tn lie in one block
    unsigned need = 0;
    {
        int t = 0;
        for (int tm = 0; tm < 4; ++tm)
            for (int tn = 0; tn <= tm; ++tn, ++t)
                if (tn == tm || (16 * tm) / b == (16 * tn + 15) / b) need |= 1u << t;
    }
    typename M::acc_t acc[10];
#pragma unroll
    for (int t = 0; t < 10; ++t) acc[t] = 0;

    const int nslot = Kp / 4 / VN;                               // 16-byte slots of a wave's quarter of a row (a multiple of 8)
    const vec_t* src[4]; bool on[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        on[f] = 16 * f + i < live;
        src[f] = reinterpret_cast<const vec_t*>(C + (g0 + (on[f] ? 16 * f + i : 0)) * Kp) + wave * nslot + q;
    }
    for (int s = 0; s < nslot; s += 4) {
        vec_t v[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            if (on[f]) v[f] = src[f][s];
            else v[f] = 0;
        }
#pragma unroll
        for (int e = 0; e < VN; ++e) {
            double a[4];
#pragma unroll
            for (int f = 0; f < 4; ++f) a[f] = (double)v[f][e];
            int t = 0;
#pragma unroll
            for (int tm = 0; tm < 4; ++tm)
#pragma unroll
                for (int tn = 0; tn <= tm; ++tn, ++t)
                    if (need >> t & 1) M::mfma(acc[t], a[tm], a[tn]);
        }
    }
    __syncthreads();
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
            int t = 0;
#pragma unroll
            for (int tm = 0; tm < 4; ++tm)
#pragma unroll
                for (int tn = 0; tn <= tm; ++tn, ++t)
                    if (need >> t & 1) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) Hs[(16 * tm + M::crow(lane, r)) * BLOCK_GRAM_LD + 16 * tn + i] += acc[t][r];
                    }
        }
        __syncthreads();
    }
}
