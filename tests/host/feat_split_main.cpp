// Stand-alone host check of l3_feat_split's planning (csrc/feat_split.h): the checks of the two index tables, the launch geometry, then
// the copy the plan describes, done by a host loop that cuts the output rows into the waves' spans as the kernel does.  Built with
// -fsanitize=address,undefined and run by tests/test_param_split_host.py; exit status 0 and "OK" when every case holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../l3embedding_amd/csrc/feat_split.h"

using namespace l3;

static int failures = 0;

static void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

struct Call {
    bool has_src = true;
    int64_t n = 9, D = 5;
    const int64_t* rows_a = nullptr;
    int64_t n_a = 0;
    const int64_t* rows_b = nullptr;
    int64_t n_b = 0;
    bool has_out_a = true, has_out_b = false;
};

static bool run(const Call& c, SplitPlan* plan, std::string* err) {
    return plan_split(c.has_src, c.n, c.D, c.rows_a, c.n_a, c.rows_b, c.n_b, c.has_out_a, c.has_out_b, plan, err);
}

static void expect_error(const Call& c, const char* needle, const char* what) {
    SplitPlan plan;
    std::string err;
    const bool ok = run(c, &plan, &err);
    expect(!ok, what);
    if (!ok && err.find(needle) == std::string::npos) {
        std::printf("FAILED: %s: message '%s' lacks '%s'\n", what, err.c_str(), needle);
        ++failures;
    }
}

// the kernel's walk on the host: wave w owns the output rows [w * rows_per_wave, ...), A's rows first, then B's
static void copy_by_plan(const SplitPlan& p, const float* x, const int64_t* rows_a, const int64_t* rows_b, float* ya, float* yb) {
    const int64_t n_out = p.n_a + p.n_b;
    for (int64_t w = 0; w < (int64_t)p.blocks * (SPLIT_BLOCK / 64); ++w) {
        const int64_t r0 = w * p.rows_per_wave;
        if (r0 >= n_out) continue;
        const int64_t r1 = r0 + p.rows_per_wave < n_out ? r0 + p.rows_per_wave : n_out;
        for (int64_t o = r0; o < r1; ++o) {
            const int64_t from = o < p.n_a ? rows_a[o] : rows_b[o - p.n_a];
            std::memcpy(o < p.n_a ? ya + o * p.D : yb + (o - p.n_a) * p.D, x + from * p.D, sizeof(float) * (size_t)p.D);
        }
    }
}

int main() {
    const int64_t n = 9, D = 5;
    std::vector<float> x((size_t)(n * D));
    for (size_t i = 0; i < x.size(); ++i) x[i] = (float)i;
    // exactly sized tables: a read past either end is the address sanitizer's to find
    std::vector<int64_t> a = {8, 0, 3, 3, 7, 1, 8}, b = {2, 0};

    // a valid cut, with repeats and the first and last source rows on both sides
    {
        Call c;
        c.rows_a = a.data(), c.n_a = (int64_t)a.size(), c.rows_b = b.data(), c.n_b = (int64_t)b.size(), c.has_out_b = true;
        SplitPlan plan;
        std::string err;
        expect(run(c, &plan, &err), "valid cut");
        expect(plan.n_a == 7 && plan.n_b == 2 && plan.D == D && plan.vec == 1, "valid cut: shape");
        expect(plan.rows_per_wave == SPLIT_WAVE_FLOATS / 5 && plan.waves == 1 && plan.blocks == 1, "valid cut: geometry");
        std::vector<float> ya(a.size() * D, -1.f), yb(b.size() * D, -1.f);
        copy_by_plan(plan, x.data(), a.data(), b.data(), ya.data(), yb.data());
        for (size_t r = 0; r < a.size(); ++r)
            expect(ya[r * D] == (float)(a[r] * D) && ya[r * D + 4] == (float)(a[r] * D + 4), "valid cut: rows of A");
        for (size_t r = 0; r < b.size(); ++r)
            expect(yb[r * D] == (float)(b[r] * D) && yb[r * D + 4] == (float)(b[r] * D + 4), "valid cut: rows of B");
    }
    // the two forms of an empty B: no table and no output at all is a plain take; anything else with n_b = 0 is refused
    {
        Call c;
        c.rows_a = a.data(), c.n_a = (int64_t)a.size();
        SplitPlan plan;
        std::string err;
        expect(run(c, &plan, &err) && plan.n_b == 0 && plan.waves == 1, "plain take");
        std::vector<float> ya(a.size() * D, -1.f);
        copy_by_plan(plan, x.data(), a.data(), nullptr, ya.data(), nullptr);
        expect(ya[0] == 40.f && ya[6 * D + 4] == 44.f, "plain take: rows");
        c.rows_b = b.data();
        expect_error(c, "n_b = 0 does not match rows_b (given) and out_b (NULL)", "n_b 0 with a table");
        c.rows_b = nullptr, c.has_out_b = true;
        expect_error(c, "n_b = 0 does not match rows_b (NULL) and out_b (given)", "n_b 0 with an output");
    }
    // indices outside [0, n): the message names the table and the position
    {
        Call c;
        c.rows_a = a.data(), c.n_a = (int64_t)a.size(), c.rows_b = b.data(), c.n_b = (int64_t)b.size(), c.has_out_b = true;
        a[4] = -1;
        expect_error(c, "rows_a[4] = -1 outside [0, 9)", "-1 in A");
        a[4] = n;
        expect_error(c, "rows_a[4] = 9 outside [0, 9)", "n in A");
        a[4] = 7, b[1] = -1;
        expect_error(c, "rows_b[1] = -1 outside [0, 9)", "-1 in B");
        b[1] = n;
        expect_error(c, "rows_b[1] = 9 outside [0, 9)", "n in B");
        b[1] = INT64_MIN;
        expect_error(c, "rows_b[1] = ", "extreme index");
        b[1] = 0;
    }
    // counts and missing arguments
    {
        Call c;
        c.rows_a = a.data(), c.n_a = 0;
        expect_error(c, "need 1 <= n_a", "n_a 0");
        c.n_a = -2;
        expect_error(c, "need 1 <= n_a", "n_a negative");
        c.n_a = SPLIT_MAX_ROWS + 1;          // refused before any entry is read
        expect_error(c, "need 1 <= n_a", "n_a 2^31");
        c.n_a = 7, c.n_b = 2, c.rows_b = nullptr, c.has_out_b = true;
        expect_error(c, "n_b = 2 does not match rows_b (NULL) and out_b (given)", "n_b > 0 with a NULL table");
        c.rows_b = b.data(), c.has_out_b = false;
        expect_error(c, "n_b = 2 does not match rows_b (given) and out_b (NULL)", "n_b > 0 with a NULL output");
        c.has_out_b = true, c.n_b = -1;
        expect_error(c, "need 0 <= n_b", "n_b negative");
        c.n_b = 2, c.rows_a = nullptr;
        expect_error(c, "NULL argument", "NULL rows_a");
        c.rows_a = a.data(), c.has_out_a = false;
        expect_error(c, "NULL argument", "NULL out_a");
        c.has_out_a = true, c.has_src = false;
        expect_error(c, "NULL argument", "NULL src");
    }
    // geometry: the shortest and the longest row, and the most rows two outputs can have
    {
        SplitPlan p = split_geometry(1, 5000, 3192);
        expect(p.vec == 1 && p.rows_per_wave == 4096 && p.waves == 2 && p.blocks == 1, "D = 1");
        p = split_geometry(1, 4096 * 4, 1);
        expect(p.waves == 5 && p.blocks == 2, "D = 1: one row past a block");
        p = split_geometry((int64_t)1 << 21, 3, 2);
        expect(p.vec == 4 && p.rows_per_wave == 1 && p.waves == 5 && p.blocks == 2, "D = 2^21");
        p = split_geometry(6144, 55706, 9830);
        expect(p.vec == 4 && p.rows_per_wave == 1 && p.waves == 65536 && p.blocks == 16384, "D = 6144");
        p = split_geometry(24, 85, 15);
        expect(p.vec == 4 && p.rows_per_wave == 170 && p.waves == 1 && p.blocks == 1, "D = 24");
        p = split_geometry(4100, SPLIT_MAX_ROWS, SPLIT_MAX_ROWS);
        expect(p.rows_per_wave == 1 && p.waves == 2 * SPLIT_MAX_ROWS && p.blocks == (1u << 30), "2^32 - 2 rows");
        // every output row belongs to exactly one wave, and the last wave is not empty
        for (int64_t D2 : {1, 5, 8, 24, 2047, 2048, 2049, 4096, 4097, 6144})
            for (int64_t rows : {1, 63, 64, 170, 171, 4096, 4097, 70000}) {
                p = split_geometry(D2, rows, 0);
                expect(p.waves * p.rows_per_wave >= rows && (p.waves - 1) * p.rows_per_wave < rows &&
                           (int64_t)p.blocks * (SPLIT_BLOCK / 64) >= p.waves && ((int64_t)p.blocks - 1) * (SPLIT_BLOCK / 64) < p.waves,
                       "cover");
            }
    }
    std::printf(failures ? "%d FAILED\n" : "OK\n", failures);
    return failures ? 1 : 0;
}
