// Host-side helpers of the posterior and pool entry points (scfgp_api.hip): plain C++17, no HIP, so that a stand-alone program can
// check them (tests/host/api_host_check.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

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
};
