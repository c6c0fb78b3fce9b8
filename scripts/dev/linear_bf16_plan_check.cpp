// Host-only driver of csrc/linear_bf16_plan.h (the argument checks and tile bookkeeping of sss_linear_grouped_bf16), meant
// to be built with a sanitizer; no device, no HIP:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/dev/linear_bf16_plan_check.cpp \
//         -o /tmp/linear_bf16_plan_check && /tmp/linear_bf16_plan_check
// Walks shapes around the 128-tile edges and the integer limits, checks every plan against plain arithmetic and prints the
// number of plans checked; any mismatch aborts.
#include <stdlib.h>
#include <string.h>

#include "../../sessionsimilaritysearch_amd/csrc/linear_bf16_plan.h"

static sss_linear_problem problem(int64_t n, int32_t m, int k) {
    sss_linear_problem p;
    memset(&p, 0, sizeof p);
    p.x = (const float*)16; p.w = (const float*)16; p.y = (float*)16;        // never dereferenced
    p.ldx = k; p.ldw = k; p.ldy = m; p.n = n; p.m = m;
    return p;
}

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); abort(); } } while (0)

int main() {
    const int64_t ns[] = {0, 1, 127, 128, 129, 255, 256, 257, 32768, 1000003, INT32_MAX, (int64_t)1 << 40, INT64_MAX};
    const int32_t ms[] = {1, 2, 127, 128, 129, 768, 2304, 3072, 1 << 20, INT32_MAX};
    const int ks[] = {32, 64, 96, 3072};
    char msg[160];
    long plans = 0, refused = 0;
    for (int k : ks)
        for (int nprob = 1; nprob <= 4; ++nprob)
            for (size_t a = 0; a < sizeof ns / sizeof *ns; ++a)
                for (size_t b = 0; b < sizeof ms / sizeof *ms; ++b) {
                    sss_linear_problem p[4];
                    __int128 want = 0;
                    for (int i = 0; i < nprob; ++i) {                                   // a different shape in every slot
                        p[i] = problem(ns[(a + 3 * i) % (sizeof ns / sizeof *ns)], ms[(b + i) % (sizeof ms / sizeof *ms)], k);
                        want += ((__int128)p[i].n + 127) / 128 * (((__int128)p[i].m + 127) / 128);
                    }
                    int tiles_m[4] = {-1, -1, -1, -1}, tile_begin[4] = {-1, -1, -1, -1}, total = -1;
                    const bool ok = sss::linear_bf16_plan(p, nprob, k, tiles_m, tile_begin, &total, msg, sizeof msg);
                    ++plans;
                    if (!ok) { ++refused; REQUIRE(strstr(msg, "tiles") && want > INT32_MAX); continue; }
                    REQUIRE(want <= INT32_MAX && total == (int)want);
                    int begin = 0;
                    for (int i = 0; i < nprob; ++i) {
                        REQUIRE(tiles_m[i] == (int)(((int64_t)p[i].m + 127) / 128) && tile_begin[i] == begin);
                        begin += (int)((p[i].n + 127) / 128) * tiles_m[i];
                    }
                    REQUIRE(begin == total);
                    for (int i = nprob; i < 4; ++i) REQUIRE(tiles_m[i] == -1 && tile_begin[i] == -1);
                }
    // the rejections, each with its message
    int tm[4], tb[4], total;
    sss_linear_problem q = problem(5, 16, 64);
    REQUIRE(!sss::linear_bf16_plan(nullptr, 1, 64, tm, tb, &total, msg, sizeof msg));
    REQUIRE(!sss::linear_bf16_plan(&q, 0, 64, tm, tb, &total, msg, sizeof msg) && !sss::linear_bf16_plan(&q, 5, 64, tm, tb, &total, msg, sizeof msg));
    REQUIRE(!sss::linear_bf16_plan(&q, 1, 48, tm, tb, &total, msg, sizeof msg) && !sss::linear_bf16_plan(&q, 1, 0, tm, tb, &total, msg, sizeof msg));
    q.ldw = 68; REQUIRE(!sss::linear_bf16_plan(&q, 1, 64, tm, tb, &total, msg, sizeof msg) && strstr(msg, "ldw"));
    q = problem(5, 16, 64); q.ids = (const int64_t*)16;
    REQUIRE(!sss::linear_bf16_plan(&q, 1, 64, tm, tb, &total, msg, sizeof msg) && strstr(msg, "gather"));
    q = problem(5, 16, 64); q.act = 6;
    REQUIRE(!sss::linear_bf16_plan(&q, 1, 64, tm, tb, &total, msg, 8) && strlen(msg) == 7);     // a short buffer is respected
    printf("linear_bf16_plan: %ld plans checked, %ld of them refused for their tile count\n", plans, refused);
    return 0;
}
