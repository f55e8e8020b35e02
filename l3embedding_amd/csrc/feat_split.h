// feat_split.h -- the host half of l3_feat_split (featprep.hip): the two index tables are checked and the launch geometry of the row
// copy is worked out.  Plain C++ with no HIP in it, as feat_assemble.h, so that it also compiles into a stand-alone host program
// (tests/host/feat_split_main.cpp, run under the address and undefined-behaviour sanitizers).
#pragma once
#include <stdint.h>

#include <string>

namespace l3 {

constexpr int64_t SPLIT_MAX_ROWS = INT32_MAX;      // of each output
constexpr int SPLIT_BLOCK = 256;                   // four waves
constexpr int SPLIT_WAVE_FLOATS = 4096;            // what one wave moves when rows are shorter than that (featprep.hip's ASM_WAVE_FLOATS)

// the output rows 0 .. n_a + n_b - 1 (A's, then B's) in spans of rows_per_wave, one wave per span, SPLIT_BLOCK / 64 waves per block
struct SplitPlan {
    int64_t n_a = 0, n_b = 0, D = 0;
    int vec = 1;                 // floats per lane and access: 4 when D % 4 == 0, else 1
    int rows_per_wave = 1;
    int64_t waves = 0;
    unsigned blocks = 0;
};

// the geometry alone: 1 <= D <= 2^21, 1 <= n_a, 0 <= n_b, both at most SPLIT_MAX_ROWS
inline SplitPlan split_geometry(int64_t D, int64_t n_a, int64_t n_b) {
    SplitPlan p;
    p.n_a = n_a, p.n_b = n_b, p.D = D;
    p.vec = D % 4 == 0 ? 4 : 1;
    p.rows_per_wave = (int)(SPLIT_WAVE_FLOATS / D > 1 ? SPLIT_WAVE_FLOATS / D : 1);
    p.waves = (n_a + n_b + p.rows_per_wave - 1) / p.rows_per_wave;          // <= 2^32 - 2
    const int64_t per_block = SPLIT_BLOCK / 64;
    p.blocks = (unsigned)((p.waves + per_block - 1) / per_block);           // <= 2^30
    return p;
}

// the source has n rows of D floats.  -> true and *plan, or false and *err, which names the table and the position.  Nothing is
// read past rows_a[n_a - 1] / rows_b[n_b - 1].  has_src / has_out_a / has_out_b: whether the caller passed those pointers.
inline bool plan_split(bool has_src, int64_t n, int64_t D, const int64_t* rows_a, int64_t n_a, const int64_t* rows_b, int64_t n_b,
                       bool has_out_a, bool has_out_b, SplitPlan* plan, std::string* err) {
    const std::string fn = "l3_feat_split: ";
    if (!has_src || !rows_a || !has_out_a) {
        *err = fn + "NULL argument (src, rows_a and out_a are needed)";
        return false;
    }
    if (n_a < 1 || n_a > SPLIT_MAX_ROWS) {
        *err = fn + "need 1 <= n_a <= 2^31 - 1 rows (n_a = " + std::to_string(n_a) + ")";
        return false;
    }
    if (n_b < 0 || n_b > SPLIT_MAX_ROWS) {
        *err = fn + "need 0 <= n_b <= 2^31 - 1 rows (n_b = " + std::to_string(n_b) + ")";
        return false;
    }
    if (n_b == 0 ? (rows_b != nullptr || has_out_b) : (!rows_b || !has_out_b)) {
        *err = fn + "n_b = " + std::to_string(n_b) + " does not match rows_b (" + (rows_b ? "given" : "NULL") + ") and out_b (" +
               (has_out_b ? "given" : "NULL") + "): both NULL with n_b = 0, both given otherwise";
        return false;
    }
    const struct { const char* name; const int64_t* rows; int64_t count; } tables[2] = {{"rows_a", rows_a, n_a}, {"rows_b", rows_b, n_b}};
    for (const auto& t : tables)
        for (int64_t i = 0; i < t.count; ++i)
            if (t.rows[i] < 0 || t.rows[i] >= n) {
                *err = fn + t.name + "[" + std::to_string(i) + "] = " + std::to_string(t.rows[i]) + " outside [0, " + std::to_string(n) + ")";
                return false;
            }
    *plan = split_geometry(D, n_a, n_b);
    return true;
}

}  // namespace l3
