// Stand-alone check of the host arithmetic that scfgp_condition_grad adds to scfgp_amd/csrc/api_host.h (plain C++17, no HIP): the point
// blocks of a chunk (GradBlocks), the target segments of its job schedule (RowJobs::seg, seg_off) against a walk over the points, and
// first_bad_dim.  Built and run by tests/test_condgrad_host.py, plain and under -fsanitize=address,undefined.
#include "../../scfgp_amd/csrc/api_host.h"

#include <cstdio>
#include <vector>

static int failures = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static constexpr int64_t CHUNK = 32768;

// n points with nd derivative columns, with or without values and precisions: every job's rows and the source and place of its segments
static void check_schedule(int nd, bool values, bool weights, int64_t n) {
    const int D = 3;
    const GradBlocks gb = {nd, values, weights};
    const int64_t nb = nd + (values ? 1 : 0), np = CHUNK / nb;
    CHECK(gb.nb() == nb && gb.points(CHUNK) == np && np >= 1 && np * nb <= CHUNK && (np + 1) * nb > CHUNK);
    CHECK(gb.target_width() == (values ? 1 : 0) + (int64_t)nd * (weights ? 2 : 1));
    std::vector<double> X(n * D), y(n), G(n * nd), rho(n * nd);   // full size: every address the schedule forms lies inside its array
    // yn and rho are handed over even where the call has none: jobs() must drop them
    const RowJobs jobs = gb.jobs(X.data(), y.data(), G.data(), rho.data(), n, CHUNK);
    CHECK(jobs.CH == np && jobs.n == n && jobs.X0 == nullptr);
    CHECK(jobs.target_width() == gb.target_width());
    CHECK(jobs.seg_width(0) == (values ? 1 : 0) && jobs.seg_width(1) == nd && jobs.seg_width(2) == (weights ? nd : 0));
    CHECK(jobs.seg_off(0) == 0 && jobs.seg_off(1) == (values ? np : 0) && jobs.seg_off(2) == jobs.seg_off(1) + np * nd);
    CHECK(jobs.seg_off(2) + jobs.seg_width(2) * np == jobs.target_width() * np);                     // the block's length
    int64_t job = 0, total = 0;
    for (int64_t t = 0; t < n; ++job) {                            // the walk: a job takes the next min(np, points left) points
        int64_t m = 0;
        while (m < np && t + m < n) ++m;
        CHECK(!jobs.lead(job) && jobs.chunk(job) == job && jobs.row0(job) == t && jobs.rows(job) == m);
        CHECK(jobs.rows(job) * nb <= CHUNK);                       // a chunk's observation rows fit the chunk buffers
        CHECK(jobs.x(job, D) == X.data() + t * D);
        CHECK(jobs.targets(job) == (values ? y.data() + t : nullptr) && jobs.seg(job, 0) == jobs.targets(job));
        CHECK(jobs.seg(job, 1) == G.data() + t * nd);
        CHECK(jobs.seg(job, 2) == (weights ? rho.data() + t * nd : nullptr));
        total += m;
        t += m;
    }
    CHECK(jobs.count() == job && total == n && job == (n + np - 1) / np);
}

// the schedules of the older entry points are what they were: no further segments, y at offset 0
static void check_plain_jobs() {
    std::vector<double> X(30), y(10);
    const RowJobs a = {X.data(), y.data(), 10, 4};
    CHECK(a.y1 == nullptr && a.y2 == nullptr && a.target_width() == 1 && a.seg_off(0) == 0 && a.seg(1, 0) == y.data() + 4);
    CHECK(a.seg(1, 1) == nullptr && a.seg(1, 2) == nullptr && a.seg_width(1) == 0 && a.seg_width(2) == 0);
    const RowJobs b = {X.data(), nullptr, 10, 4, X.data(), 2};
    CHECK(b.target_width() == 0 && b.seg(0, 0) == nullptr && b.seg(1, 0) == nullptr && b.count() == 4);
}

static void check_dims() {
    std::vector<char> seen(5);
    { const int32_t d[5] = {4, 0, 3, 1, 2}; CHECK(first_bad_dim(d, 5, 5, seen.data()) == -1); }
    { const int32_t d[1] = {3}; CHECK(first_bad_dim(d, 1, 5, seen.data()) == -1); }
    { const int32_t d[3] = {0, 5, 1}; CHECK(first_bad_dim(d, 3, 5, seen.data()) == 1); }
    { const int32_t d[3] = {-1, 5, 1}; CHECK(first_bad_dim(d, 3, 5, seen.data()) == 0); }
    { const int32_t d[4] = {2, 0, 1, 0}; CHECK(first_bad_dim(d, 4, 5, seen.data()) == 3); }
    { const int32_t d[4] = {2, 2, 9, 0}; CHECK(first_bad_dim(d, 4, 5, seen.data()) == 1); }      // the first of two bad entries
    { const int32_t d[2] = {1, 1}; CHECK(first_bad_dim(d, 2, 5, seen.data()) == 1); CHECK(first_bad_dim(d, 1, 5, seen.data()) == -1); }   // scratch is cleared
    { const int32_t d[1] = {0}; CHECK(first_bad_dim(d, 1, 1, seen.data()) == -1); }
}

int main() {
    check_plain_jobs();
    check_dims();
    for (int nb : {1, 2, 71, 32768})
        for (int values = 0; values < 2; ++values) {
            const int nd = nb - values;
            if (nd < 1) continue;                                   // nb = 1 with a value row has no derivative column
            const int64_t np = CHUNK / nb;
            for (int64_t n : {(int64_t)1, np - 1, np, np + 1, 2 * np + 3}) {
                if (n < 1) continue;                                // np = 1: np - 1 points is no call
                for (int weights = 0; weights < 2; ++weights) check_schedule(nd, values != 0, weights != 0, n);
            }
        }
    // a point that does not fit a chunk: the entry point refuses on nb() before it asks for points()
    { const GradBlocks gb = {32768, true, false}; CHECK(gb.nb() == 32769 && gb.points(CHUNK) == 0); }
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("ok\n");
    return failures ? 1 : 0;
}
