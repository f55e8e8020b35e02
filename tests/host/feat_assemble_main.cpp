// Stand-alone host check of l3_feat_assemble's planning (csrc/feat_assemble.h): the segment checks, the table and its prefix of
// output rows, then the copy the table describes, done by a host loop that walks it as the kernel does.  Built with
// -fsanitize=address,undefined and run by tests/test_foldbank_host.py; exit status 0 and "OK" when every case holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../l3embedding_amd/csrc/feat_assemble.h"

using namespace l3;

static int failures = 0;

static void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

static void expect_error(int device, const std::vector<FeatSegView>& segs, int64_t n_segs, const char* needle, const char* what) {
    AssemblePlan plan;
    std::string err;
    const bool ok = plan_assemble(device, segs.empty() ? nullptr : segs.data(), n_segs, &plan, &err);
    expect(!ok, what);
    if (!ok && err.find(needle) == std::string::npos) {
        std::printf("FAILED: %s: message '%s' lacks '%s'\n", what, err.c_str(), needle);
        ++failures;
    }
}

int main() {
    const int64_t D = 5;
    std::vector<float> a(7 * D), b(1 * D), c(3 * 4);
    for (size_t i = 0; i < a.size(); ++i) a[i] = (float)i;
    for (size_t i = 0; i < b.size(); ++i) b[i] = 100.f + (float)i;
    const FeatSegView A{true, 0, 7, D, a.data(), 0, 7}, B{true, 0, 1, D, b.data(), 0, 1};

    // a valid list: a source used twice, empty segments in between, an odd first row
    {
        std::vector<FeatSegView> segs = {A, B, A, B, A};
        segs[0].lo = 3, segs[0].hi = 5;
        segs[1].lo = 1, segs[1].hi = 1;          // empty, at the end of its source
        segs[2].lo = 0, segs[2].hi = 0;          // empty
        segs[4].lo = 6, segs[4].hi = 7;
        AssemblePlan plan;
        std::string err;
        expect(plan_assemble(0, segs.data(), (int64_t)segs.size(), &plan, &err), "valid list");
        expect(plan.rows == 4 && plan.D == D && plan.table.size() == 4, "valid list: shape");
        expect(plan.table[0].first == 0 && plan.table[1].first == 2 && plan.table[2].first == 3 && plan.table[3].first == 4 &&
                   plan.table[3].src == nullptr,
               "valid list: prefix and sentinel");
        std::vector<float> y((size_t)(plan.rows * D), -1.f);
        for (int64_t r = 0, s = 0; r < plan.rows; ++r) {          // the kernel's walk, a row at a time
            while (r >= plan.table[s + 1].first) ++s;
            std::memcpy(&y[(size_t)(r * D)], plan.table[s].src + (r - plan.table[s].first) * D, sizeof(float) * D);
        }
        const float want[4] = {15.f, 20.f, 100.f, 30.f};          // first entries of a's rows 3, 4, b's row 0, a's row 6
        for (int r = 0; r < 4; ++r) expect(y[(size_t)(r * D)] == want[r] && y[(size_t)(r * D + 4)] == want[r] + 4.f, "valid list: rows");
    }

    // every refusal
    expect_error(0, {}, 0, "at least one segment", "n_segs 0");
    expect_error(0, {A}, -3, "at least one segment", "n_segs negative");
    expect_error(0, {}, 2, "at least one segment", "NULL list");
    {
        FeatSegView g = B;
        g.present = false;
        expect_error(0, {A, g}, 2, "segment 1: the source is NULL", "NULL source");
    }
    {
        FeatSegView g = B;
        g.device = 1;
        expect_error(0, {A, A, g}, 3, "segment 2: the source is on device 1", "other device");
        expect_error(1, {g, A}, 2, "segment 1: the source is on device 0", "other device, second segment");
    }
    {
        const FeatSegView g{true, 0, 3, 4, c.data(), 0, 3};
        expect_error(0, {A, g}, 2, "segment 1: the source has 4 columns", "other width");
    }
    {
        FeatSegView g = A;
        g.lo = -1;
        expect_error(0, {g}, 1, "segment 0: rows [-1, 7) outside", "lo negative");
        g.lo = 0, g.hi = 8;
        expect_error(0, {A, g}, 2, "segment 1: rows [0, 8) outside", "hi past the end");
        g.lo = 5, g.hi = 4;
        expect_error(0, {g}, 1, "segment 0: rows [5, 4) outside", "hi below lo");
        g.lo = INT64_MIN, g.hi = INT64_MAX;
        expect_error(0, {g}, 1, "segment 0: rows [", "extreme range");
    }
    {
        FeatSegView g = A;
        g.hi = 0;
        expect_error(0, {g, g, g}, 3, "hold 0 rows in total", "no rows");
    }
    {
        // 2^31 - 1 rows are allowed, one more is not: a huge source that is only described, never read
        const int64_t big = FEAT_MAX_ROWS;
        const FeatSegView G{true, 0, big, D, a.data(), 0, big - 1};
        AssemblePlan plan;
        std::string err;
        const std::vector<FeatSegView> fits = {G, B};
        expect(plan_assemble(0, fits.data(), 2, &plan, &err) && plan.rows == big, "2^31 - 1 rows");
        expect_error(0, {G, B, B}, 3, "segment 2: the total passes 2^31 - 1 rows", "2^31 rows");
        expect_error(0, {G, G}, 2, "segment 1: the total passes 2^31 - 1 rows", "2^32 rows");
    }
    std::printf(failures ? "%d FAILED\n" : "OK\n", failures);
    return failures ? 1 : 0;
}
