// Stand-alone check of the host arithmetic that scfgp_sobol adds to scfgp_amd/csrc/api_host.h (plain C++17, no HIP): the scans of the
// measure, its device form, the test of its phases against the domain of sin / cos, and the schedule of the pair kernel -- every block (jb, kb) of the upper triangle in exactly one unit, in
// row-major order, the run length and the columns per pass against the record budget.  Built and run by tests/test_sobol_host.py, plain
// and under -fsanitize=address,undefined.
#include "../../scfgp_amd/csrc/api_host.h"

#include <cfloat>
#include <cstdio>
#include <limits>
#include <vector>

static int failures = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static constexpr int64_t BUDGET = (int64_t)64 << 20;
static constexpr int COLS = 32;

static void check_measure() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    { const int32_t k[4] = {0, 1, 1, 0}; CHECK(sobol_first_bad_kind(k, 4) == -1); CHECK(sobol_first_bad_kind(nullptr, 4) == -1); }
    { const int32_t k[4] = {0, 2, -1, 0}; CHECK(sobol_first_bad_kind(k, 4) == 1); CHECK(sobol_first_bad_kind(k, 1) == -1); }
    const double p0[4] = {0.0, 0.5, -1.0, 2.0}, p1[4] = {1.0, 0.0, -1.0, 3.0};
    CHECK(sobol_first_bad_range(nullptr, p0, p1, 4) == 1);                       // all uniform: 0 < 0.5
    { const int32_t k[4] = {0, 1, 0, 0}; CHECK(sobol_first_bad_range(k, p0, p1, 4) == -1); }      // sd 0; a point mass at -1
    { const int32_t k[4] = {0, 1, 1, 0}; CHECK(sobol_first_bad_range(k, p0, p1, 4) == 2); }       // sd -1
    { const double q1[4] = {1.0, nan, -1.0, 1.0}; const int32_t k[4] = {0, 0, 0, 0};
      CHECK(sobol_first_bad_range(k, p0, q1, 4) == 3);                           // a NaN compares false: left to the finite scan
      CHECK(sobol_first_nonfinite(p0, q1, 4) == 1); }
    { const double q0[4] = {0.0, 0.5, -inf, 2.0}; CHECK(sobol_first_nonfinite(q0, p1, 4) == 2); }
    CHECK(sobol_first_nonfinite(p0, p1, 4) == -1);
    const int32_t k[4] = {0, 1, 0, 1};
    const double a0[4] = {-1.0, 0.5, -DBL_MAX, 2.0}, a1[4] = {3.0, 0.25, DBL_MAX, 0.0};
    double meas[12];
    sobol_measure(k, a0, a1, 4, meas);
    CHECK(meas[0] == 0.0 && meas[1] == 1.0 && meas[2] == 0.0 && meas[3] == 1.0);
    CHECK(meas[4] == 1.0 && meas[8] == 2.0);                                     // uniform: centre, half width
    CHECK(meas[5] == 0.5 && meas[9] == 0.25);                                    // normal: as given
    CHECK(meas[6] == 0.0 && meas[10] == DBL_MAX);                                // no overflow at the ends of the range
    CHECK(meas[7] == 2.0 && meas[11] == 0.0);
    sobol_measure(nullptr, a0, a1, 1, meas);
    CHECK(meas[0] == 0.0 && meas[1] == 1.0 && meas[2] == 2.0);
}

// the domain of sin / cos: R_d = 2 omax (|centre| + half width) or 2 omax |mean| against 3.37e9, the first input at or beyond it
static void check_domain() {
    const double two30 = 1073741824.0;
    {   // the case that was found: centre 2.5 * 2^30, half width 1/8, max |Om| = 1 -> R = 5.4e9; 1.5 * 2^30 -> 3.2e9 passes
        const double om[1] = {1.0};
        double meas[3] = {0.0, 2.5 * two30, 0.125};
        CHECK(sobol_first_out_of_domain(meas, om, 1) == 0);
        meas[1] = 1.5 * two30; CHECK(sobol_first_out_of_domain(meas, om, 1) == -1);
        meas[1] = -2.5 * two30; CHECK(sobol_first_out_of_domain(meas, om, 1) == 0);       // |centre|
        meas[1] = two30; meas[2] = 0.0; CHECK(sobol_first_out_of_domain(meas, om, 1) == -1);     // R = 2^31 = 2.1e9
        meas[2] = two30; CHECK(sobol_first_out_of_domain(meas, om, 1) == 0);               // R = 2^32: the half width counts
    }
    {   // either side of the limit, R formed exactly: omax = 1/2, so R = |centre| + half width
        const double om[1] = {0.5};
        double meas[3] = {0.0, 3.37e9, 0.0};
        CHECK(sobol_first_out_of_domain(meas, om, 1) == 0);                                // R == limit is outside
        meas[1] = std::nextafter(3.37e9, 0.0); CHECK(sobol_first_out_of_domain(meas, om, 1) == -1);
        meas[1] = 3.37e9 - 1.0; meas[2] = 1.0; CHECK(sobol_first_out_of_domain(meas, om, 1) == 0);      // the half width counts ...
        meas[0] = 1.0; CHECK(sobol_first_out_of_domain(meas, om, 1) == -1);                // ... on a uniform input only
        meas[2] = 1e300; CHECK(sobol_first_out_of_domain(meas, om, 1) == -1);              // a normal's sd takes no sin / cos
    }
    {   // the first of several; an input without frequencies passes whatever its measure; the ends of the range refuse, never NaN
        const double om[4] = {1.0, 0.0, 3.0, 1e-290};
        const int32_t k[4] = {0, 0, 1, 0};
        const double p0[4] = {0.0, -DBL_MAX / 2, 2e9, -DBL_MAX / 2}, p1[4] = {1.0, DBL_MAX / 2, 1.0, DBL_MAX / 2};
        double meas[12];
        sobol_measure(k, p0, p1, 4, meas);
        CHECK(sobol_first_out_of_domain(meas, om, 4) == 2);                                // 2 * 3 * 2e9
        const double p0b[4] = {0.0, 0.9 * DBL_MAX, 1e8, -DBL_MAX / 2};
        const double p1b[4] = {1.0, DBL_MAX, 1.0, DBL_MAX / 2};
        sobol_measure(k, p0b, p1b, 4, meas);
        CHECK(std::isfinite(meas[5]) && std::isfinite(meas[9]));
        CHECK(sobol_first_out_of_domain(meas, om, 4) == 3);                                // input 1: omax 0; input 3: 2e-290 * 9e307
        const double big[4] = {1.0, 2.0, 3.0, 2.0};
        CHECK(sobol_first_out_of_domain(meas, big, 4) == 1);                               // 2 * 2 * 0.95 DBL_MAX = +inf: refused
        const double none[4] = {0.0, 0.0, 0.0, 0.0};
        CHECK(sobol_first_out_of_domain(meas, none, 4) == -1);
    }
}

// every block of the triangle once, in row-major order; no run longer than kseg; the count agrees
static void check_units(int nb, int kseg) {
    std::vector<int> u;
    sobol_units(nb, kseg, u);
    CHECK(u.size() % 3 == 0 && (int64_t)u.size() / 3 == sobol_unit_count(nb, kseg));
    int jb = 0, kb = 0;                                                          // the next block the walk expects
    for (size_t i = 0; i < u.size(); i += 3) {
        CHECK(u[i] == jb && u[i + 1] == kb && u[i + 2] > u[i + 1] && u[i + 2] - u[i + 1] <= kseg && u[i + 2] <= nb);
        kb = u[i + 2];
        if (kb == nb) { ++jb; kb = jb; }
    }
    CHECK(jb == nb);
}

static void check_schedule() {
    for (int nb : {1, 2, 15, 16, 17, 38, 132})
        for (int kseg : {1, 16, 32, 1024}) check_units(nb, kseg);
    // the run length depends on the geometry only and starts at 16
    CHECK(sobol_kseg(1, 3, COLS, BUDGET) == 16 && sobol_kseg(132, 129, COLS, BUDGET) == 16);
    CHECK(sobol_unit_count(132, 16) * 129 * COLS * 8 <= BUDGET);
    {   // K = 16384 at D = 64: the records of 16-block runs would not fit, longer runs do
        const int nb = 1024, nsets = 129;
        const int kseg = sobol_kseg(nb, nsets, COLS, BUDGET);
        CHECK(kseg > 16 && (kseg & (kseg - 1)) == 0);
        CHECK(sobol_unit_count(nb, kseg) * nsets * COLS * 8 <= BUDGET || kseg >= nb);
        CHECK(kseg == 16 * 2 || sobol_unit_count(nb, kseg / 2) * nsets * COLS * 8 > BUDGET);
    }
    CHECK(sobol_kseg(64, (int64_t)1 << 40, COLS, BUDGET) == 64);                 // nothing fits: one unit per row, and the loop ends
    // columns per pass: whole blocks of COLS, at least one, within the budget where one block fits
    for (int64_t nunits : {(int64_t)1, (int64_t)610, (int64_t)40000})
        for (int64_t nsets : {(int64_t)3, (int64_t)129}) {
            const int pass = sobol_pass_cols(nunits, nsets, COLS, BUDGET);
            CHECK(pass >= COLS && pass % COLS == 0 && pass <= 1024 * COLS);
            if (nunits * nsets * COLS * 8 <= BUDGET) {
                CHECK(nunits * nsets * pass * 8 <= BUDGET);
                CHECK(pass == 1024 * COLS || nunits * nsets * (pass + COLS) * 8 > BUDGET);
            } else CHECK(pass == COLS);
        }
}

int main() {
    check_measure();
    check_domain();
    check_schedule();
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("ok\n");
    return failures ? 1 : 0;
}
