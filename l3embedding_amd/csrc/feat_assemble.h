// feat_assemble.h -- the host half of l3_feat_assemble (featprep.hip): the segment list is checked and turned into the table the copy
// kernel reads.  Plain C++ with no HIP in it, so that it also compiles into a stand-alone host program (tests/host/feat_assemble_main.cpp,
// run under the address and undefined-behaviour sanitizers).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace l3 {

// what the plan reads of one segment: its source handle's fields (present == false: a NULL handle) and the rows [lo, hi) taken
struct FeatSegView {
    bool present;
    int device;
    int64_t n, D;
    const float* x;
    int64_t lo, hi;
};

// one non-empty segment as the kernel sees it: the address of its first source row and its first output row.  The table ends with
// a sentinel {nullptr, rows}, so entry s covers the output rows [first[s], first[s + 1]).
struct AssembleEntry {
    const float* src;
    int64_t first;
};

struct AssemblePlan {
    std::vector<AssembleEntry> table;          // the non-empty segments in order, then the sentinel
    int64_t rows = 0, D = 0;
};

constexpr int64_t FEAT_MAX_ROWS = INT32_MAX;

// -> true and *plan, or false and *err (which names the segment).  Nothing of *plan is meaningful after a failure.
inline bool plan_assemble(int device, const FeatSegView* segs, int64_t n_segs, AssemblePlan* plan, std::string* err) {
    const std::string fn = "l3_feat_assemble: ";
    if (n_segs < 1 || !segs) {
        *err = fn + "need at least one segment (n_segs = " + std::to_string(n_segs) + ")";
        return false;
    }
    plan->table.clear();
    plan->rows = 0, plan->D = 0;
    for (int64_t i = 0; i < n_segs; ++i) {
        const FeatSegView& g = segs[i];
        const std::string at = fn + "segment " + std::to_string(i) + ": ";
        if (!g.present) {
            *err = at + "the source is NULL";
            return false;
        }
        if (g.device != device) {
            *err = at + "the source is on device " + std::to_string(g.device) + ", not on device " + std::to_string(device);
            return false;
        }
        if (i == 0) plan->D = g.D;
        if (g.D != plan->D) {
            *err = at + "the source has " + std::to_string(g.D) + " columns, segment 0 has " + std::to_string(plan->D);
            return false;
        }
        if (g.lo < 0 || g.hi < g.lo || g.hi > g.n) {
            *err = at + "rows [" + std::to_string(g.lo) + ", " + std::to_string(g.hi) + ") outside the source's [0, " +
                   std::to_string(g.n) + ")";
            return false;
        }
        if (g.hi == g.lo) continue;
        // g.hi - g.lo <= g.n <= 2^31 - 1 and plan->rows <= 2^31 - 1: the sum cannot overflow before it is tested
        if (plan->rows + (g.hi - g.lo) > FEAT_MAX_ROWS) {
            *err = at + "the total passes 2^31 - 1 rows (" + std::to_string(plan->rows) + " before it, " + std::to_string(g.hi - g.lo) +
                   " in it)";
            return false;
        }
        plan->table.push_back(AssembleEntry{g.x + g.lo * g.D, plan->rows});
        plan->rows += g.hi - g.lo;
    }
    if (plan->rows == 0) {
        *err = fn + "segments 0 to " + std::to_string(n_segs - 1) + " hold 0 rows in total";
        return false;
    }
    plan->table.push_back(AssembleEntry{nullptr, plan->rows});
    return true;
}

}  // namespace l3
