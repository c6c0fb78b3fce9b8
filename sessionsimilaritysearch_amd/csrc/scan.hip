// Query x corpus inner-product CANDIDATE scan with fused running top-k (gfx950 / CDNA4): f32, bf16, f16, int8 rows,
// split-bf16 (three passes over an f32 corpus) and scaled f16 (one pass over an f32 corpus).
//
// Replaces what the reference asks of faiss at test_amazon_filterd.py:578
// (`D, I = index.search(normalize(emb), K)`, faiss.IndexFlatIP).
// The scan's scores never reach the output: select.hip re-scores the candidates in float64 from the
// stored rows and proves, per query, that nothing outside them could matter (error bound per scan
// type: select_dev.h err_bound).
//
// k_scan<RB, TR, DT, NW, THR, AP>  -- the dominant kernel (DESIGN.md "scoring kernel"); RB = bytes per scanned
// corpus row (256 / 512 / 1024), TR = rows per LDS tile (64 / 128 / 256), DT = element type (scan.h),
// NW = waves per workgroup:
//   * one workgroup = 8 waves (2 per SIMD) = 256 queries x one contiguous corpus split (1024-byte
//     rows: 4 waves, one per SIMD, 128 queries);
//   * each wave keeps its 32 queries resident in RB/8 VGPRs as the B operand of
//     v_mfma_f32_32x32x2_f32 (DT_F32: an exact k-ordered f32 fma chain), v_mfma_f32_32x32x16_bf16
//     (DT_BF16; DT_SPLIT: hi*hi + hi*lo + lo*hi of rows stored [hi | lo]) or v_mfma_f32_32x32x16_f16
//     (DT_F16: f32 queries scaled by their own power of two and rounded in the prologue; DT_H16: stored f16 rows
//     and f16 queries as they are) or v_mfma_i32_32x32x32_i8 (DT_I8: stored int8 rows and int8 queries, 16 elements
//     per 16-byte chunk, exact int32 sums converted to float32 keys once per 64-row step), so the query tile is read
//     from HBM once;
//   * corpus rows stream HBM -> LDS with global_load_lds_dwordx4 (no VGPR staging), double
//     buffered, one burst per tile, 16-byte chunks XOR-swizzled on the SOURCE address so the
//     ds_read_b128 fragment reads are bank-conflict free.  Rows of equal BYTES stage and read
//     identically whatever they hold: lane half h reads chunk 2u+h, which is the k-permuted A operand
//     of four f32 MFMAs or the natural A operand of one 16-bit MFMA;
//   * the score matrix is never written: each lane owns one query column of the 32x32
//     accumulators and keeps a sorted top-KP list (scores + row ids) in registers.  The scan runs
//     in 64-row steps: a HOT loop (MFMAs, one v_max3 tree, one compare) that never writes the list
//     state, left for a RARE insert path only when some lane's step maximum beats its threshold.  (The f32 list form
//     for 512-byte rows decides the two 32-row halves of a step apart, each under the other half's MFMAs and across
//     the step boundary: two exits, one per half -- scan_kernel.h, "F32S");
//   * ADMISSION THRESHOLD shared by all workgroups of a query: every lane list belongs to one of J
//     classes (J >= K2); slot[q][class] holds, by atomic max, the best score any list of that class
//     has seen (cert == 1) or the largest cert-th best of such a list (cert > 1).  Classes
//     partition the corpus rows, so tau = min over slots is a score that at least J * cert >= K2
//     distinct rows reach, and a row scoring below tau can never be among the best K2.  With
//     cert == 1 (K2 <= 16) all 16 slots are distinct classes and tau is RANK-SELECTED: the K2-th largest
//     class maximum (scan_dev.h: tau_select16) -- K2 distinct rows reach it as well, and it sits near the
//     ~21st best row seen instead of the ~37th of "min over K2 classes".  The first tile of every split is
//     scanned twice: once max-only to publish (bootstrap: publish, then a bounded wait for the other
//     workgroups), and again at the end with the lists live, so no row is lost and the expensive "early
//     phase" of a running top-k (every row beats an empty list) never happens.  (More than one max-only
//     tile -- B tiles put B x as many rows behind the first live threshold -- was built and measured in
//     round 4: candidates fall further, the time does not: the extra tiles cost what they save.)  Slots
//     only ever hold scores of real rows and only grow, so a stale read merely admits extra candidates:
//     speed, never correctness;
//   * at the end each lane appends its real entries to the query's compact candidate array
//     (one atomic add per lane) for k_select_* (select.hip, select_thr.hip);
//   * AP = true, the APPEND form (k <= 16 on 256-byte rows of a 16-bit scan, with the bootstrap): the shared
//     threshold alone decides what is kept, so a lane needs no sorted list -- a 4-entry unsorted register
//     buffer, flushed to the candidate array when full and at the end.  128 VGPRs instead of 223: TWO
//     workgroups per CU (four waves per SIMD) on twice the splits.
#include "scan_kernel.h"

namespace sss {

__device__ unsigned g_boot_expired;              // (declared in scan_kernel.h)

// ------------------------------------------------------------------------------ host side
// Number of waves, since the last reset, whose bootstrap wait ran out (synchronises the device: a debugging / bench aid).
extern "C" int sss_scan_boot_expired(int reset) {
    unsigned v = 0, zero = 0;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_boot_expired), sizeof(v)) != hipSuccess) { set_error("scan_boot_expired: read failed"); return SSS_EHIP; }
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_boot_expired), &zero, sizeof(zero)) != hipSuccess) { set_error("scan_boot_expired: reset failed"); return SSS_EHIP; }
    return (int)(v > 0x7fffffffu ? 0x7fffffffu : v);
}

int current_device() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    return dev < 0 || dev >= MAX_DEVICES ? 0 : dev;
}

static int pick_splits(long n, int G, int tr) {
    // S*G workgroups, one per CU (256 CUs); S a multiple of 8 (XCD remap); >= one tile a split.
    int S = (256 / G) & ~7;
    if (S < 8) S = 8;
    while (S > 8 && (long)S * tr > n) S -= 8;
    return S;
}

constexpr int TR256_MIN_TILES = 24;     // splits at least this many 256-row tiles long use them (256-byte rows)

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

static ScanPlan make_plan_for(long nq, long n, int d, int k, int dtype, bool want_append);

// The append form's bootstrap hand-shake needs all 2 x 256 workgroups resident at once: ask the runtime, once per
// device, whether two of its workgroups (80 KB of LDS, 128 VGPRs each) fit a CU and the chip has the CUs -- otherwise
// (another LDS carve-out, a smaller part) the plan keeps the list form.
static bool append_form_fits() {
    static int cached[MAX_DEVICES] = {};                 // 0 unknown, 1 yes, 2 no
    const int dev = current_device();
    if (cached[dev] == 0) {
        constexpr int lds = 2 * 128 * 256 + 8 * 2048;
        const void* fn = reinterpret_cast<const void*>(&k_scan<256, 128, DT_F16, 8, false, true>);
        int blocks = 0, cus = 0;
        bool ok = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess &&
                  hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, fn, 512, lds) == hipSuccess &&
                  hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess;
        (void)hipGetLastError();
        cached[dev] = (ok && blocks >= 2 && cus >= 256) ? 1 : 2;
    }
    return cached[dev] == 1;
}

ScanPlan make_plan(long nq, long n, int d, int k, int dtype) {
    // The append form (k <= 16 on 256-byte rows of a 16-bit scan: no lane lists, half the registers) runs TWO
    // workgroups per CU on twice the splits; it needs the bootstrap (a shared threshold from the first live row on) and
    // splits long enough to be worth it -- otherwise the plan with lane lists.
    const int rb = d * elem_bytes(dtype);
    if (rb == 256 && dtype != DT_F32 && k <= KP && append_form_fits()) {
        const ScanPlan a = make_plan_for(nq, n, d, k, dtype, true);
        if (a.append) return a;
    }
    return make_plan_for(nq, n, d, k, dtype, false);
}
static ScanPlan make_plan_for(long nq, long n, int d, int k, int dtype, bool want_append) {
    ScanPlan p;
    const int rb = d * elem_bytes(dtype);
    const int wgq = rb == 1024 ? 128 : WG_QUERIES;      // queries per workgroup (k_scan's NW * 32)
    p.G = (int)((nq + wgq - 1) / wgq);
    // 128-row tiles (one barrier per 128 rows) for long splits; 64-row tiles keep the split
    // granularity (and the once-repeated bootstrap tile) small when a split is only a few tiles.
    int tr = rb <= 512 ? 128 : 64;
    int S = pick_splits(n, p.G, tr);
    if (rb == 512 && (n + (long)S * 128 - 1) / ((long)S * 128) < 48) { tr = 64; S = pick_splits(n, p.G, tr); }
    // 256-byte rows: 256-row tiles (one barrier and one threshold refresh per 256 rows, the next tile's
    // DMA a whole tile ahead) once a split is long enough to amortise the twice-scanned bootstrap tile
    if (rb == 256 && dtype != DT_F32 && n / ((long)S * 256) >= TR256_MIN_TILES) tr = 256;
    if (want_append) {                                    // 2 S splits of 128-row tiles, S * G <= 256
        tr = 128;
        S = pick_splits(n, p.G, tr);
        // (>= 7 tiles a split after doubling: measured round 4 -- 125 k rows, one of eight shards of the 1M corpus, 0.122 ->
        //  0.110 ms with the append form; 100 k rows the same either way, below that the list form)
        if ((long)S * p.G > 256 || (long)2 * S * tr * 7 > n) want_append = false;
        else S *= 2;
        if (!want_append) { ScanPlan none; none.append = 0; return none; }
    }
    p.tile_rows = tr;
    p.S = S;
    p.L = 2 * S;
    // k <= 14: K2 = max(k + 2, 8) (class maxima + bootstrap; the select kernel's second chance widens the candidate
    // set where the slack K2 - k is too thin for a query -- as it always had to for k = 15, 16, where K2 = 16 = KP
    // leaves none); larger k: k + 12.  A small K2 pays twice: the shared threshold certifies only K2 rows, and
    // "min over K2 class maxima" sits nearer the top the fewer classes there are (it tracks roughly the 35th best
    // row seen with 12 classes, the 50th with 16): a third fewer candidates to insert, re-score and carry.
    p.K2 = k + 2 <= KP ? (k + 2 < 8 ? 8 : k + 2) : k <= KP ? KP : k + 12;
    if ((long)p.L * KP < p.K2) p.K2 = p.L * KP;
    p.total_tiles = (int)((n + tr - 1) / tr);
    p.tiles_per_split = (p.total_tiles + S - 1) / S;
    p.cap = p.L * KP;
    // threshold slots: J classes x cert entries certify J * cert >= K2 rows (scan.hip header).
    // K2 <= 16: 16 classes of class maxima (cert 1, with the bootstrap; refreshed through LDS-DMA
    // every iteration).  Larger K2: 16 (64 beyond K2 = 128) classes certify `cert` rows each with
    // their lists' cert-th best -- measured faster than one class per row, whose 7+ slot loads per
    // refresh have to be synchronous.
    const int active_splits = (p.total_tiles + p.tiles_per_split - 1) / p.tiles_per_split;
    p.J = p.K2 <= 128 ? 16 : 64;
    p.cert = 1;
    while (p.J * p.cert < p.K2 && p.cert < KP) p.cert *= 2;
    // cert == 1 (K2 <= 16): all 16 slots are distinct classes and the threshold is the K2-th largest class maximum
    // (tau_skip = 16 - K2 words allowed below it; scan_dev.h: tau_select16)
    p.Ju = p.J;
    p.tau_skip = (p.cert == 1 && p.J == 16) ? 16 - p.K2 : 0;
    // cert == 1: a query's lane pairs publish per SPLIT, into class (split + split / 16) & 15 -- with fewer than 16 active
    // splits only classes 0 .. active_splits - 1 ever publish.  The scan's rank pick (scan_dev.h tau_select16) takes,
    // per half of the 16 slots, its (skip / 2 + 1)-th smallest word (half 0: + 1 more for an odd skip) and the min of
    // the two: each half may hold no more unpublished (zero) words than that, or the threshold stays 0 for the whole
    // scan and every wave sits out its bootstrap wait (8 splits: > 4096 queries per call, or a corpus of a few thousand
    // rows).  cert > 1 lists publish per lane ((2 split + h) % Ju).  Too few classes, or a tiny corpus: no threshold.
    bool classes_ok = 2 * active_splits >= p.Ju;
    if (p.cert == 1 && p.J == 16 && active_splits < 16) {
        const int zero0 = active_splits < 8 ? 8 - active_splits : 0, zero1 = active_splits < 8 ? 8 : 16 - active_splits;
        classes_ok = zero0 <= (p.tau_skip >> 1) + (p.tau_skip & 1) && zero1 <= (p.tau_skip >> 1);
    }
    if (p.J * p.cert < p.K2 || !classes_ok) { p.J = 0; p.Ju = 0; p.tau_skip = 0; }
    p.boot = (p.J > 0 && p.cert == 1) ? 1 : 0;
    p.append = (want_append && p.boot) ? 1 : 0;
    if (want_append && !p.append) return p;               // (the caller falls back to the list plan)
    if (p.append) p.cap = 2048;                            // candidates per query the select kernels stage (FS_CAP)
    p.total_bytes = align256((size_t)nq * p.cap * 8);
    return p;
}

// Plan of the threshold form: G groups of compact queries x S corpus splits, 128-row tiles (64 for
// 1024-byte rows), no threshold slots; cap = candidates kept per query.
ScanPlan make_thr_plan(long nsel, long n, int d, int scan_dtype, int cap) {
    ScanPlan p = {};
    const int rb = d * elem_bytes(scan_dtype);
    const int wgq = rb == 1024 ? 128 : WG_QUERIES;
    p.G = (int)((nsel + wgq - 1) / wgq);
    p.tile_rows = rb <= 512 ? 128 : 64;
    p.S = pick_splits(n, p.G, p.tile_rows);
    p.L = 2 * p.S;
    p.total_tiles = (int)((n + p.tile_rows - 1) / p.tile_rows);
    p.tiles_per_split = (p.total_tiles + p.S - 1) / p.S;
    p.cap = cap;
    p.total_bytes = align256((size_t)nsel * cap * 8);
    return p;
}

int launch_scan(int dtype, int d, int tile_rows, const ScanArgs& a, hipStream_t st) {
    const int rb = d * elem_bytes(dtype);
    if (a.bias != nullptr) return launch_scan_l2(dtype, d, tile_rows, a, st);      // a row bias is given: the L2 kernels (scan_l2.hip)
    int rc = 1;                                                  // (1: nothing launched)
    with_dtype<true>(dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        rc = launch_shape<DT, 0>(rb, tile_rows, a, st);
    });
    if (rc != 1) return rc;
    set_error("scan: unsupported row size %d bytes", rb);
    return SSS_EINVAL;
}

}  // namespace sss
