// Host side of sss_linear_grouped_bf16 (linear_bf16.hip): the argument checks and the tile bookkeeping of a launch, with
// no device type in it, so that a stand-alone host program can drive it under a sanitizer.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "../../include/sss.h"

namespace sss {

constexpr int BF_T = 128;    // k_linear_grouped_bf16: output tile rows (X rows) and columns (W rows)

// Checks `nprob` problems against the limits of include/lowp/sss_linear_bf16.h and lays their tiles out in one grid:
// tiles_m[i] the column tiles of problem i, tile_begin[i] its first workgroup, *total the workgroups of the launch.
// Returns true, or false with the reason in msg (at most cap bytes).  Slots nprob..3 are not touched.
inline bool linear_bf16_plan(const sss_linear_problem* p, int nprob, int k, int tiles_m[4], int tile_begin[4], int* total, char* msg,
                             size_t cap) {
    if (!p || nprob < 1 || nprob > 4) { snprintf(msg, cap, "linear_grouped_bf16: 1..4 problems (got %d)", nprob); return false; }
    if (k <= 0 || k % 32) { snprintf(msg, cap, "linear_grouped_bf16: need k > 0 and k %% 32 == 0 (k = %d)", k); return false; }
    int64_t sum = 0;
    for (int i = 0; i < nprob; ++i) {
        const sss_linear_problem& q = p[i];
        const char* bad = nullptr;
        if (q.ids || q.table || q.xcopy) bad = "no gather mode here: ids, table and xcopy must be NULL";
        else if (q.act < 0 || q.act > 5) bad = "act must be 0..5";
        else if ((q.post_scale == nullptr) != (q.post_shift == nullptr)) bad = "post_scale / post_shift come together";
        else if (q.n < 0 || q.m <= 0) bad = "need n >= 0 and m > 0";
        else if (q.ldw % 8 || q.ldw < k) bad = "need ldw % 8 == 0 and ldw >= k (in bf16 elements)";
        else if (q.ldx % 4 || q.ldx < k) bad = "need ldx % 4 == 0 and ldx >= k";
        else if (q.ldy < q.m) bad = "need ldy >= m";
        if (bad) { snprintf(msg, cap, "linear_grouped_bf16: problem %d: %s", i, bad); return false; }
        tiles_m[i] = (q.m - 1) / BF_T + 1;                           // m <= 2^31 - 1: no overflow before the division
        tile_begin[i] = (int)sum;
        const int64_t tiles_n = q.n / BF_T + (q.n % BF_T != 0);     // any n >= 0, no overflow
        if (tiles_n > INT32_MAX / tiles_m[i] || (sum += tiles_n * tiles_m[i]) > INT32_MAX) {
            snprintf(msg, cap, "linear_grouped_bf16: problem %d: the launch would need more than 2^31 - 1 tiles", i);
            return false;
        }
    }
    *total = (int)sum;
    return true;
}

}  // namespace sss
