// Stand-alone check of scfgp_amd/csrc/api_host.h (plain C++17, no HIP): scan_weights on the weight vectors of the entry points' refusals,
// RowJobs against a walk over the rows.  Built and run by tests/test_api_host.py, plain and under -fsanitize=address,undefined.
#include "../../scfgp_amd/csrc/api_host.h"

#include <cstdio>
#include <limits>
#include <vector>

static int failures = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static void check_scan() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    {
        const double w[5] = {1, -1, nan, 1, 1};
        const WeightScan s = scan_weights(w, 5);
        CHECK(s.first_negative == 1 && s.first_nonfinite == 2 && s.positive == 3 && s.first_bad() == 1 && s.sum != s.sum);
    }
    {
        const double w[5] = {nan, -1, 1, 1, 1};
        const WeightScan s = scan_weights(w, 5);
        CHECK(s.first_negative == 1 && s.first_nonfinite == 0 && s.positive == 3 && s.first_bad() == 0);
    }
    {
        const double w[5] = {1, inf, 1, 1, 1};
        const WeightScan s = scan_weights(w, 5);
        CHECK(s.first_negative == -1 && s.first_nonfinite == 1 && s.positive == 4 && s.first_bad() == 1 && s.sum == inf);
    }
    {
        const double w[5] = {1, -inf, 1, 1, 1};                  // negative and non-finite at once
        const WeightScan s = scan_weights(w, 5);
        CHECK(s.first_negative == 1 && s.first_nonfinite == 1 && s.positive == 4 && s.first_bad() == 1);
    }
    {
        const double w[5] = {0, 0, 0, 0, 0};
        const WeightScan s = scan_weights(w, 5);
        CHECK(s.first_negative == -1 && s.first_nonfinite == -1 && s.positive == 0 && s.first_bad() == -1 && s.sum == 0.0);
    }
    {
        const double w[5] = {0, 1, 0, 0, 0};
        const WeightScan s = scan_weights(w, 5);
        CHECK(s.first_negative == -1 && s.first_nonfinite == -1 && s.positive == 1 && s.sum == 1.0);
    }
    {
        const WeightScan s = scan_weights(nullptr, 0);
        CHECK(s.first_negative == -1 && s.first_nonfinite == -1 && s.positive == 0 && s.sum == 0.0);
    }
    {
        const double big = std::numeric_limits<double>::max();
        const double w[3] = {big, big, 1};                        // finite entries, a sum that is not
        const WeightScan s = scan_weights(w, 3);
        CHECK(s.first_negative == -1 && s.first_nonfinite == -1 && s.positive == 3 && s.sum == inf);
    }
    {
        const double w[4] = {0.1, 0.2, 0.3, 0.4};                 // the sum is the left-to-right one, bit for bit
        const WeightScan s = scan_weights(w, 4);
        double ref = 0.0;
        for (double v : w) ref += v;
        CHECK(s.sum == ref && s.positive == 4);
    }
}

static void check_jobs(int64_t n, int64_t CH, bool lead, bool with_targets) {
    const int D = 3;
    const int64_t n0 = 5;
    std::vector<double> X(n * D), y(n), X0(n0 * D);
    const RowJobs jobs = {X.data(), with_targets ? y.data() : nullptr, n, CH, lead ? X0.data() : nullptr, lead ? n0 : 0};
    int64_t job = 0, total = 0;
    if (lead) {
        CHECK(jobs.lead(0) && jobs.chunk(0) == -1 && jobs.rows(0) == n0 && jobs.row0(0) == 0);
        CHECK(jobs.x(0, D) == X0.data() && jobs.targets(0) == nullptr);
        ++job;
    }
    for (int64_t r = 0, i = 0; r < n; ++i, ++job) {               // the walk: chunk i takes the next min(CH, rows left) rows
        int64_t m = 0;
        while (m < CH && r + m < n) ++m;
        CHECK(!jobs.lead(job) && jobs.chunk(job) == i && jobs.row0(job) == r && jobs.rows(job) == m);
        CHECK(jobs.x(job, D) == X.data() + r * D);
        CHECK(jobs.targets(job) == (with_targets ? y.data() + r : nullptr));
        total += m;
        r += m;
    }
    CHECK(jobs.count() == job && total == n);
}

int main() {
    check_scan();
    for (int64_t CH : {(int64_t)7, (int64_t)32768})
        for (int64_t n : {(int64_t)1, CH - 1, CH, CH + 1, 2 * CH, 2 * CH + 300})
            for (int lead = 0; lead < 2; ++lead)
                for (int tg = 0; tg < 2; ++tg) check_jobs(n, CH, lead != 0, tg != 0);
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("ok\n");
    return failures ? 1 : 0;
}
