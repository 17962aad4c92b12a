// Host-side helpers of the posterior and pool entry points (api_predict.hip, api_update.hip, api_pool.hip): plain C++17, no HIP, so
// that a stand-alone program can check them (tests/host/api_host_check.cpp; scfgp_condition_grad's part:
// tests/host/condgrad_host_check.cpp; scfgp_sobol's: tests/host/sobol_host_check.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

// One pass over a weight vector, in index order.  It decides nothing: every caller keeps its own messages and its own order of tests.
struct WeightScan {
    int64_t first_negative = -1;                                  // first w[i] < 0 (-inf included), -1: none
    int64_t first_nonfinite = -1;                                 // first NaN or +-inf, -1: none
    int64_t positive = 0;                                         // finite entries above 0
    double sum = 0.0;                                             // ((0 + w[0]) + w[1]) + ...
    int64_t first_bad() const {                                   // the first entry that is either, -1: none
        return first_negative < 0 || first_nonfinite < 0 ? std::max(first_negative, first_nonfinite) : std::min(first_negative, first_nonfinite);
    }
};
inline WeightScan scan_weights(const double* w, int64_t n) {
    WeightScan s;
    for (int64_t i = 0; i < n; ++i) {
        if (w[i] < 0.0 && s.first_negative < 0) s.first_negative = i;
        if (!std::isfinite(w[i])) { if (s.first_nonfinite < 0) s.first_nonfinite = i; }
        else if (w[i] > 0.0) ++s.positive;
        s.sum += w[i];
    }
    return s;
}

// The job schedule of a feed: an optional leading block (X0: n0 rows, no targets, one job) and then the rows of X (n x D, targets
// beside them or NULL) in chunks of CH rows, the last one ragged.
struct RowJobs {
    const double* X; const double* y; int64_t n, CH;
    const double* X0 = nullptr; int64_t n0 = 0;
    int64_t count() const { return (X0 ? 1 : 0) + (n + CH - 1) / CH; }
    bool lead(int64_t job) const { return X0 && job == 0; }
    int64_t chunk(int64_t job) const { return lead(job) ? -1 : job - (X0 ? 1 : 0); }      // -1: the leading job
    int64_t row0(int64_t job) const { return lead(job) ? 0 : chunk(job) * CH; }
    int64_t rows(int64_t job) const { return lead(job) ? n0 : std::min(CH, n - row0(job)); }
    const double* x(int64_t job, int D) const { return lead(job) ? X0 : X + row0(job) * D; }
    const double* targets(int64_t job) const { return lead(job) || !y ? nullptr : y + row0(job); }
    // The target block of a job: up to three arrays behind the rows, segment 0 = y (1 double per row), segments 1 and 2 = y1, y2 (w1, w2
    // doubles per row; NULL: absent).  In the feed's half the segments that are present follow one another, each CH rows long, so a
    // segment's place does not depend on the job: seg_off(k) doubles behind the start of the block, target_width() * CH in all.
    const double* y1 = nullptr; int64_t w1 = 0;
    const double* y2 = nullptr; int64_t w2 = 0;
    static constexpr int SEGS = 3;
    const double* seg_base(int k) const { return k == 0 ? y : k == 1 ? y1 : y2; }
    int64_t seg_width(int k) const { return !seg_base(k) ? 0 : k == 0 ? 1 : k == 1 ? w1 : w2; }
    int64_t seg_off(int k) const { int64_t o = 0; for (int i = 0; i < k; ++i) o += seg_width(i) * CH; return o; }
    int64_t target_width() const { return seg_width(0) + seg_width(1) + seg_width(2); }
    const double* seg(int64_t job, int k) const { return lead(job) || !seg_base(k) ? nullptr : seg_base(k) + row0(job) * seg_width(k); }
};

// scfgp_condition_grad: a point brings a block of nb = nd + (values ? 1 : 0) observation rows, and a chunk holds whole points.
struct GradBlocks {
    int nd; bool values, weights;                                 // derivative columns; yn given; rho given
    int64_t nb() const { return nd + (values ? 1 : 0); }
    int64_t points(int64_t chunk_rows) const { return chunk_rows / nb(); }       // per chunk of chunk_rows observation rows (0: none fit)
    int64_t target_width() const { return (values ? 1 : 0) + (int64_t)nd * (weights ? 2 : 1); }
    // the schedule: n points in chunks of points(chunk_rows), targets [yn | Gn | rho] behind them
    RowJobs jobs(const double* X, const double* yn, const double* Gn, const double* rho, int64_t n, int64_t chunk_rows) const {
        RowJobs j = {X, values ? yn : nullptr, n, points(chunk_rows)};
        j.y1 = Gn; j.w1 = nd;
        j.y2 = weights ? rho : nullptr; j.w2 = weights ? nd : 0;
        return j;
    }
};

// dims (nd entries): the position of the first entry that is out of 0..D-1 or repeats an earlier one, -1: none.  seen: D bytes of scratch
inline int first_bad_dim(const int32_t* dims, int nd, int D, char* seen) {
    std::fill(seen, seen + D, 0);
    for (int j = 0; j < nd; ++j) {
        if (dims[j] < 0 || dims[j] >= D || seen[dims[j]]) return j;
        seen[dims[j]] = 1;
    }
    return -1;
}

// ---- scfgp_sobol: the measure (kind NULL: all uniform; p0, p1: D entries each) and the schedule of the pair kernel -------------------
inline int sobol_first_bad_kind(const int32_t* kind, int D) {         // first kind outside {0, 1}, -1: none
    if (kind) for (int d = 0; d < D; ++d) if (kind[d] != 0 && kind[d] != 1) return d;
    return -1;
}
// first input with p1 < p0 (uniform) or p1 < 0 (normal), -1: none; a NaN compares false and is left to sobol_first_nonfinite
inline int sobol_first_bad_range(const int32_t* kind, const double* p0, const double* p1, int D) {
    for (int d = 0; d < D; ++d) if (kind && kind[d] == 1 ? p1[d] < 0.0 : p1[d] < p0[d]) return d;
    return -1;
}
inline int sobol_first_nonfinite(const double* p0, const double* p1, int D) {
    for (int d = 0; d < D; ++d) if (!std::isfinite(p0[d]) || !std::isfinite(p1[d])) return d;
    return -1;
}
// meas (3 x D) as the kernels take it: kind | centre or mean | half width or standard deviation.  The halves are taken before the sum
// and the difference, so bounds near DBL_MAX do not overflow here: the centre and the half width come out finite.  That says nothing
// about the phases -- a measure that far out is refused by sobol_first_out_of_domain wherever its input has a nonzero frequency.
inline void sobol_measure(const int32_t* kind, const double* p0, const double* p1, int D, double* meas) {
    for (int d = 0; d < D; ++d) {
        const bool normal = kind && kind[d] == 1;
        meas[d] = normal ? 1.0 : 0.0;
        meas[D + d] = normal ? p0[d] : 0.5 * p0[d] + 0.5 * p1[d];
        meas[2 * D + d] = normal ? p1[d] : 0.5 * p1[d] - 0.5 * p0[d];
    }
}
// The domain of fast_sincos (sincos.h): |z| < 2^31 pi/2 = 3.373e9, stated as 3.37e9.  The pair kernel evaluates psi_d at Om[d][j] +-
// Om[d][k], so the phases of input d reach R_d = 2 omax[d] (|centre| + half width) on a uniform input (the sinc takes its sine at
// (Om_j +- Om_k) half width) and 2 omax[d] |mean| on a normal one, whose amplitude takes no sin / cos.  First input with R_d at or beyond
// the limit, -1: none.  The two products are formed apart, so that an input with omax = 0 passes whatever its measure (0, never 0 x inf),
// and a sum that overflows is +inf and refused.  meas as sobol_measure leaves it, omax (D) = max_j |Om[d][j]|, both finite.
constexpr double SOBOL_PHASE_LIMIT = 3.37e9;
inline int sobol_first_out_of_domain(const double* meas, const double* omax, int D) {
    for (int d = 0; d < D; ++d) {
        const double r = 2.0 * (omax[d] * std::fabs(meas[D + d]) + (meas[d] == 0.0 ? omax[d] * meas[2 * D + d] : 0.0));
        if (!(r < SOBOL_PHASE_LIMIT)) return d;
    }
    return -1;
}
// The work units of the pair kernel: the blocks (jb, kb), jb <= kb < nb, of the upper triangle in row-major order, a row cut into runs
// of at most kseg blocks; a unit is (jb, kb0, kb1).  A column's sum visits the units in this order, so the schedule may depend on the
// geometry only, never on the number of columns: kseg is the smallest of 16, 32, 64, ... at which the records of one block of `cols`
// columns (units x nsets x cols doubles) fit `budget` bytes, or one unit per row where none does.
inline int64_t sobol_unit_count(int nb, int kseg) {
    int64_t n = 0;
    for (int jb = 0; jb < nb; ++jb) n += (nb - jb + kseg - 1) / kseg;
    return n;
}
inline int sobol_kseg(int nb, int64_t nsets, int cols, int64_t budget) {
    int kseg = 16;
    while (kseg < nb && sobol_unit_count(nb, kseg) * nsets * cols * 8 > budget) kseg *= 2;
    return kseg;
}
inline void sobol_units(int nb, int kseg, std::vector<int>& units) {
    units.clear();
    for (int jb = 0; jb < nb; ++jb)
        for (int kb = jb; kb < nb; kb += kseg) { units.push_back(jb); units.push_back(kb); units.push_back(std::min(kb + kseg, nb)); }
}
// columns per pass: as many blocks of `cols` as fit the budget, at least one
inline int sobol_pass_cols(int64_t nunits, int64_t nsets, int cols, int64_t budget) {
    const int64_t blocks = budget / (nunits * nsets * cols * 8);
    return (int)(std::max<int64_t>(1, std::min<int64_t>(blocks, 1 << 10)) * cols);
}
