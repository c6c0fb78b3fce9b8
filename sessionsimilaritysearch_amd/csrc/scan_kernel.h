// k_scan, the candidate scan kernel, and its launch templates: included by the two translation units that instantiate
// it -- scan.hip (the inner-product scans, MET = 0, and the host side) and scan_l2.hip (the L2 scans, MET = 1) -- so the
// two sets of kernels compile side by side.  The kernel's description is at the top of scan.hip.  gfx950 only.
#pragma once
#include <type_traits>
#include "scan.h"
#include "scan_dev.h"

namespace sss {

// NW = waves per workgroup: 8 (two per SIMD, 256 VGPRs each) or, for 1024-byte rows whose resident
// queries alone take 128 VGPRs, 4 (one per SIMD, 512 VGPRs: no spills; NW * 32 queries per workgroup).
// THR = true is the THRESHOLD form (the rung between the fused search and the exhaustive kernels,
// ip_topk.hip: sss_ip_topk_threshold): the queries are the compact list A.qsel, every lane compares against
// its query's FIXED threshold A.thr[] (scan domain) instead of a running list, and every row above it is
// appended to the query's candidate array -- no lists, no shared threshold, no bootstrap.
// waves whose bootstrap wait expired before the threshold existed (read + reset through sss_scan_boot_expired)
extern __device__ unsigned g_boot_expired;       // (defined in scan.hip; counted by the inner-product scans only: MET = 0)

// MET = 1 is the L2 form: the scan key of (query, row) is q.c - |c|^2 / 2 -- the rows nearest to q in L2 are the rows with
// the largest such key (|q - c|^2 = |q|^2 - 2 key) -- so every accumulator starts from its row's bias A.bias[row] instead
// of zero and everything downstream (lists, append form, shared threshold, bootstrap, candidate arrays) sees keys as
// before.  The bias enters ON THE MATRIX CORES: one v_mfma_f32_32x32x2_f32 per accumulator, A = the 32 rows' biases in
// the k = 0 column (zeros in k = 1), B = 1 -- or, DT_F16, the power of two 2^(corpus shift + the lane's query shift) the
// scaled scan's keys live in: an exact product, landed in the accumulator layout by the unit itself.  A lane needs ONE
// float per 32 rows for that; a tile's 2 H of them are fetched during the PREVIOUS tile's end (tile_end: before the wait
// that retires the tile DMA, so the hot loop gains no counted load and no wait of its own).  The inner-product
// instantiations (MET = 0) compile to what they were: every L2 statement sits under `if constexpr (MET)`.
template <int RB, int TR, int DT, int NW, bool THR = false, bool AP = false, int MET = 0>
__global__ __launch_bounds__(NW * 64, AP ? 2 * (NW / 4) : NW / 4) void k_scan(const ScanArgs A) {
    constexpr int H = TR / 64;                        // 64-row sub-steps per tile
    constexpr int CH = RB / 16;                       // 16-byte chunks per row
    constexpr int NU = RB / 32;                       // k-groups per row (one b128 fragment each)
    constexpr int TILE_BYTES = TR * RB;
    constexpr int LOADS_PER_WAVE = TR * CH / 64 / NW; // LDS-DMA wave-instructions per wave per tile
    constexpr int WGQ = NW * 32;                      // queries per workgroup
    constexpr bool PRECOMP = RB <= 512 && !AP;        // keep the DMA lane offsets in VGPRs (register budget; not at 128 VGPRs)
    constexpr int TAU_LDS = 2 * TILE_BYTES;           // [8 waves][32 queries][16 slots] u32 behind the two tile buffers
    constexpr bool F32S = DT == DT_F32 && !AP && !THR && RB == 512;   // (the loop is in front of the split loop, below)
    static_assert(CH <= 64, "row longer than one LDS-DMA instruction");
    static_assert(LOADS_PER_WAVE >= 1, "a tile is at least one DMA piece per wave");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int nq = A.nq, n = A.n, S = A.S, G = A.G, J = A.J;
    const char* __restrict__ Qb = reinterpret_cast<const char*>(A.Q);
    const char* __restrict__ Cb = reinterpret_cast<const char*>(A.C);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;

    // XCD-aware remap: blocks b and b+8 share an XCD (and its L2); the G query groups that
    // stream the same corpus split are given consecutive slots of ONE XCD so the split is
    // fetched from HBM once and re-read from that L2.  Speed only, never correctness.
    const int bid = blockIdx.x;
    const int xcd = bid & 7, slot = bid >> 3;
    const int split = xcd * (S >> 3) + slot / G;
    const int g = slot % G;

    // ---- resident queries: lane (r, h) holds 16-byte chunk 2u + h of its query row in qc[u]
    const int q_local = wave * 32 + r;
    const int q_glob = g * WGQ + q_local;
    int q_ld = q_glob < nq ? q_glob : nq - 1;
    if constexpr (THR) q_ld = A.qsel[q_ld];             // row of Q this lane's (compact) query lives in
    f32x4 qc[NU];                                       // (loaded after the first tiles' DMA has been issued, below)

    // Lane list, sorted descending; empty slots are (-inf, -1).  thr = max(list tail, tau) is the
    // one value the hot path compares against.
    float ls[KP];
    int li[KP];
#pragma unroll
    for (int i = 0; i < KP; ++i) { ls[i] = -INFINITY; li[i] = -1; }
    float pend_s = -INFINITY;   // one parked candidate per lane (see the epilogue)
    int pend_i = -1;
    // AP (append form: K2 <= 16 with the bootstrap, 256-byte rows): the shared threshold alone decides what is kept,
    // so a lane needs no sorted list -- passing rows go into a small unsorted register buffer that is handed to the
    // query's candidate array when it is full and at the end (ls / li / pend_* are dead in this form).  Half the
    // registers: TWO workgroups per CU, four waves per SIMD.
    constexpr int E = 4;
    float es[E];
    int ei[E];
    int ecnt = 0;
#pragma unroll
    for (int i = 0; i < E; ++i) { es[i] = -INFINITY; ei[i] = -1; }
    float tau = -INFINITY, thr = -INFINITY;
    if constexpr (THR) thr = q_glob < nq ? A.thr[q_glob] : INFINITY;    // padding lanes never emit
    float rmax = -INFINITY;     // best score this lane has seen (published when cert == 1)
    float pub = -INFINITY;      // last value this lane published

    int tile_lo = split * A.tiles_per_split;
    int tile_hi = tile_lo + A.tiles_per_split;
    if (tile_hi > A.total_tiles) tile_hi = A.total_tiles;
    const int ntiles = tile_lo < tile_hi ? tile_hi - tile_lo : 0;
    const bool use_tau = !THR && J > 0;
    // bootstrap: the first tile of the split is scanned max-only first (iteration 0) and again, live, at the end
    // (iteration ntiles)
    const bool boot = use_tau && A.boot && ntiles > 0;
    const int nb = boot ? 1 : 0;
    const int niter = ntiles + nb;
    auto tile_of = [&](int i) { return i < ntiles ? tile_lo + i : tile_lo; };
    const int skip = A.tau_skip;                 // rank-selected threshold (cert == 1, J == 16): 16 - K2

    bool slots_seen = false;                     // the LDS copy of the slots has been filled at least once
    const unsigned* my_half = nullptr;
    unsigned cls_live = 0;                       // class of this lane's rows
    // cert == 1: a class is a set of SPLITS (split & 15; both lanes of a query's (h = 0, 1) pair belong to it), so the
    // pair publishes ONE value -- the better of its two lane maxima, by lane h = 0: half the agent-scope atomics (at the
    // bootstrap 128 instead of 256 per query line, which all arrive within a microsecond and serialise at the line's
    // memory channel).  cert > 1: a class per lane list, as the lists certify `cert` rows each.
    const bool pair_pub = A.cert == 1;
    if (use_tau) {
        // (split + split / 16: with the append form's 128 splits the low four bits of `split` alone would put the workgroups
        //  dispatched first -- the lower half of the grid, one per CU -- in classes 0-7 and their co-resident partners,
        //  which lose the SIMD arbitration and reach the end of the bootstrap tile ~10 us later, in classes 8-15: every
        //  wave then waits for the slow half before it has a threshold.  Mixed, each class has members of both halves.)
        cls_live = pair_pub ? (unsigned)(split + (split >> 4)) & 15u : (unsigned)(2 * split + h) % (unsigned)A.Ju;
        my_half = A.slots + (size_t)q_ld * SLOT_STRIDE + h * (J >> 1);
    }
    // Threshold word of the query from its J slots.  Synchronous form (bootstrap wait; J > 16): each lane of the
    // (h = 0, 1) pair reads half with agent-scope loads.  J == 16 with a rank: the (skip + 1)-th smallest; else the min.
    auto tau_ord = [&]() -> unsigned {
        if (J == 16 && skip > 0) {
            unsigned v[8];
            load8_sc1(my_half, v);
            return tau_select16(v, skip, h);
        }
        unsigned m = 0xFFFFFFFFu;
        for (int v = 0; v < (J >> 1); v += 8) m = min(m, min8_sc1(my_half + v));
        return min(m, (unsigned)__shfl_xor((int)m, 32));
    };
    // Asynchronous form (J == 16, every iteration): the wave's 32 queries x 64 B of slots are
    // fetched by two LDS-DMA instructions (agent scope) at the top of an iteration, land under the
    // MFMAs, are retired by the iteration's vmcnt(0) and read back by their owner lanes: no
    // stall, no registers held.
    const unsigned tau_lds = (unsigned)(unsigned long)(lptr_c)smem + TAU_LDS + wave * 2048;
    auto tau_fetch = [&]() {
        // (the lane offsets are recomputed from an OPAQUE copy of the lane id at every refresh: as loop invariants the
        //  compiler kept them in registers for the whole scan -- at the append form's register limit, in scratch, with a
        //  reload + vmcnt(0) in front of each of the two DMA instructions, which serialised them)
        int ln = lane;
        asm volatile("" : "+v"(ln));
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            int qi = g * WGQ + wave * 32 + 16 * j + (ln >> 2);
            if (qi > nq - 1) qi = nq - 1;
            const unsigned off = (unsigned)qi * (unsigned)(SLOT_STRIDE * 4) + (unsigned)(ln & 3) * 16u;
            const unsigned dst = __builtin_amdgcn_readfirstlane(tau_lds + j * 1024);
            lds_dma16<true>(off, dst, A.slots);
        }
    };
    auto tau_read = [&]() -> unsigned {
        const u32x4* p = reinterpret_cast<const u32x4*>(smem + TAU_LDS + wave * 2048 + r * 64 + h * 32);
        const u32x4 a = p[0], b = p[1];
        if (skip > 0) {
            unsigned v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            return tau_select16(v, skip, h);
        }
        const unsigned m = min(min(min(a.x, a.y), min(a.z, a.w)), min(min(b.x, b.y), min(b.z, b.w)));
        return min(m, (unsigned)__shfl_xor((int)m, 32));
    };
    auto set_tau = [&](unsigned m) {
        if (m > ORD_NEG_INF) tau = fmaxf(tau, ord2f(m - 1));     // the float just below the min slot
        thr = AP ? tau : fmaxf(ls[KP - 1], tau);
    };
    auto publish = [&](unsigned cls) {
        float val = rmax;
        bool ok = true;
        if (A.cert > 1) {
            // copies made opaque: a select chain over ls[] / li[] would be folded into a
            // runtime-indexed load and send both lists to scratch
            float v2 = ls[1], v4 = ls[3], v8 = ls[7], v16 = ls[KP - 1];
            int i2 = li[1], i4 = li[3], i8 = li[7], i16 = li[KP - 1];
            asm volatile("" : "+v"(v2), "+v"(v4), "+v"(v8), "+v"(v16), "+v"(i2), "+v"(i4), "+v"(i8), "+v"(i16));
            const int c = A.cert;
            val = c == 2 ? v2 : c == 4 ? v4 : c == 8 ? v8 : v16;
            ok = (c == 2 ? i2 : c == 4 ? i4 : c == 8 ? i8 : i16) >= 0;
        }
        // A lane's new best only matters if it beats its CLASS's best -- which ~10 lists share, so most lane records
        // are not class records.  The last fetched copy of the slots (LDS, J == 16) tells: without this filter the
        // early tiles, where every lane sets records all the time, spend most of their time waiting for some
        // hundred agent-scope atomics per query line to drain (vmcnt(0) at the end of the tile).
        if (pair_pub) { val = fmaxf(val, __shfl_xor(val, 32)); ok = h == 0; }
        unsigned cur = 0u;
        if (J == 16 && slots_seen) cur = *reinterpret_cast<const unsigned*>(smem + TAU_LDS + wave * 2048 + r * 64 + cls * 4u);
        if (ok && val > pub && val > tau && f2ord(val) > cur && q_glob < nq) {     // at or below tau it cannot raise the threshold
            // (the slot address is rebuilt from an opaque copy of the query index: a 64-bit per-lane pointer kept across the
            //  scan costs two registers the append form does not have -- it was spilled and reloaded here)
            int qq = THR ? q_ld : q_glob;
            asm volatile("" : "+v"(qq));
            __hip_atomic_fetch_max(A.slots + ((size_t)(unsigned)qq * (unsigned)SLOT_STRIDE + cls), f2ord(val), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            pub = val;
        }
    };

    // LDS-DMA staging (global_load_lds_dwordx4, 1 KiB per wave-instruction).  Written as inline
    // asm so hipcc neither counts it nor drains vmcnt(0) at the next ds_read: the next tile
    // stays in flight under this tile's MFMAs and is retired by the explicit vmcnt(0) that
    // precedes the barrier at the end of the iteration (cdna_hip_programming.md section 5.7).
    // Slot p of the tile (16 B each) holds chunk (p % CH) ^ (row & 15) of row p / CH: the
    // swizzle is on the SOURCE address, the LDS image is lane-linear.
    const unsigned lds_base = (unsigned)(unsigned long)(lptr_c)smem;
    auto slot_row = [&](int i) { return ((wave * LOADS_PER_WAVE + i) * 64 + lane) / CH; };
    auto slot_off = [&](int i) {                    // byte offset of this lane's chunk inside the tile
        const int p = (wave * LOADS_PER_WAVE + i) * 64 + lane;
        const int tr = p / CH, sc = p % CH;
        return (unsigned)(tr * RB + ((sc ^ (tr & 15)) * 16));
    };
    unsigned lane_off[PRECOMP ? LOADS_PER_WAVE : 1];
    if (PRECOMP) {
#pragma unroll
        for (int i = 0; i < LOADS_PER_WAVE; ++i) lane_off[i] = slot_off(i);
    }
    // One LDS-DMA wave-instruction (piece i of this wave's share of a tile).
    auto stage_piece = [&](int buf, int tile_idx, int i) {
        const long row0 = (long)tile_idx * TR;
        const bool inside = row0 + TR <= (long)n;          // wave-uniform
        const char* tile_src = Cb + (size_t)row0 * RB;      // wave-uniform -> SGPR pair
        const unsigned dst = __builtin_amdgcn_readfirstlane(
            lds_base + buf * TILE_BYTES + (wave * LOADS_PER_WAVE + i) * 1024);
        unsigned off = PRECOMP ? lane_off[PRECOMP ? i : 0] : slot_off(i);
        if (!inside) {                                       // ragged last tile: clamp the row
            const int lr = slot_row(i);
            long grow = row0 + lr;
            if (grow > (long)n - 1) grow = (long)n - 1;
            off = (unsigned)((grow - row0) * RB) + (off - (unsigned)(lr * RB));
        }
        lds_dma16(off, dst, tile_src);
    };
    auto stage = [&](int buf, int tile_idx) {
#pragma unroll
        for (int i = 0; i < LOADS_PER_WAVE; ++i) stage_piece(buf, tile_idx, i);
    };

    // per-lane LDS read swizzle term of chunk (2u + h) of row r
    const int x = h ^ (r & 15);
    f32x16 acc0 = {0}, acc1 = {0};
    // L2: bias of row (32 s + r) of the current tile, s = 0 .. 2 H - 1, in the lanes h = 0 (the k = 0 column of the seeding
    // MFMA's A operand; lanes h = 1 hold its k = 1 column: zeros); rows at and beyond n read row n - 1's and are masked
    // by the ragged-tile test like every other score of such a row
    [[maybe_unused]] float bcur[MET ? 2 * H : 1];
    [[maybe_unused]] float bscale = 1.f;
    [[maybe_unused]] auto bias_fetch = [&](int tile_idx) {
#pragma unroll
        for (int s = 0; s < 2 * H; ++s) {
            long row = (long)tile_idx * TR + s * 32 + r;
            if (row > (long)n - 1) row = (long)n - 1;
            bcur[s] = h == 0 ? A.bias[row] : 0.f;
        }
    };
    // ... retired HERE (the counted wait hipcc puts in front of the first use), where nothing else is in flight
    [[maybe_unused]] auto bias_land = [&]() {
#pragma unroll
        for (int s = 0; s < 2 * H; ++s) asm volatile("" : "+v"(bcur[s]));
    };

    auto mfma_sub = [&](int buf, int sub, int next_tile) {
        const char* tile = smem + buf * TILE_BYTES + sub * (64 * RB);
        // The next tile's DMA (all of this wave's pieces in one burst, once per tile): with a single
        // sub-step per tile it has to go out before this step's MFMAs to have time to land; otherwise
        // it follows the first sub-step's MFMAs, issuing while they execute, and has the rest of the
        // tile to land.  (One piece per k-group, as before, cost ~20 scalar instructions and a branch
        // per group in every step: the scan was bound by instruction issue, not by the matrix pipe.)
        if constexpr (H == 1) { if (next_tile >= 0) stage(buf ^ 1, next_tile); }
        auto lda = [&](int u) -> const f32x4* {
            const int c = (2 * u) ^ x;                          // == (2u + h) ^ (r & 15)
            return reinterpret_cast<const f32x4*>(tile + (r * CH + c) * 16);
        };
        // A fragments PF k-groups ahead of their MFMAs: the f32 MFMA spends 512 cycles on a group, one
        // group ahead covers the LDS latency; the 16-bit MFMAs spend 64-128, so their reads run further
        // ahead (all of a 256-byte row's fragments at once -- the registers are there).
        constexpr int PF = DT == DT_F32 ? 1 : AP ? 1 : (RB == 256 ? NU : RB == 512 ? 4 : 2);
        f32x4 as0[NU], as1[NU];
#pragma unroll
        for (int u = 0; u < PF && u < NU; ++u) { const f32x4* p = lda(u); as0[u] = p[0]; as1[u] = p[32 * CH]; }
        const f32x16 zero = {0};
        if constexpr (MET) {
            // (bias_of() written out: through the helper the kernels with four sub-steps a tile compile differently)
            float b0 = bcur[0], b1 = bcur[1];
#pragma unroll
            for (int s = 1; s < H; ++s) { b0 = sub == s ? bcur[2 * s] : b0; b1 = sub == s ? bcur[2 * s + 1] : b1; }
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(b0, bscale, zero, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(b1, bscale, zero, 0, 0, 0);
        } else {
            acc0 = zero; acc1 = zero;
        }
        [[maybe_unused]] i32x16 ia0 = {0}, ia1 = {0};       // DT_I8: the step's int32 accumulators
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            if (u + PF < NU) { const f32x4* p = lda(u + PF); as0[u + PF] = p[0]; as1[u + PF] = p[32 * CH]; }
            const f32x4 a0 = as0[u], a1 = as1[u];
            __builtin_amdgcn_sched_barrier(0);   // keep the prefetch ABOVE this group's MFMAs
            if constexpr (DT == DT_F32) {
                mfma_f32_group(acc0, acc1, a0, a1, qc[u]);
            } else if constexpr (DT == DT_BF16) {
                const bf16x8 qb = __builtin_bit_cast(bf16x8, qc[u]);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a0), qb, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a1), qb, acc1, 0, 0, 0);
            } else if constexpr (DT == DT_F16 || DT == DT_H16) {
                const f16x8 qb = __builtin_bit_cast(f16x8, qc[u]);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a0), qb, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a1), qb, acc1, 0, 0, 0);
            } else if constexpr (DT == DT_I8) {
                // (lane half h holds the same 16 k values of chunk 2u + h on the A and on the B side: whatever order the
                //  unit gives the 16 bytes of a lane, a row's byte j meets the query's byte j)
                const i32x4 qb = __builtin_bit_cast(i32x4, qc[u]);
                ia0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(i32x4, a0), qb, ia0, 0, 0, 0);
                ia1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(i32x4, a1), qb, ia1, 0, 0, 0);
            } else {
                // split f32: chunks of the hi half meet q_hi and q_lo, chunks of the lo half meet q_hi
                const bf16x8 A0 = __builtin_bit_cast(bf16x8, a0), A1 = __builtin_bit_cast(bf16x8, a1);
                const bf16x8 qh = __builtin_bit_cast(bf16x8, qc[u < NU / 2 ? u : u - NU / 2]);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A0, qh, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A1, qh, acc1, 0, 0, 0);
                if (u < NU / 2) {
                    const bf16x8 ql = __builtin_bit_cast(bf16x8, qc[u + NU / 2]);
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A0, ql, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A1, ql, acc1, 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (DT == DT_I8) {
            // |sum| <= RB * 2^14 <= 2^24: the conversion is exact, the float32 key is the score itself
            acc0 = __builtin_convertvector(ia0, f32x16);
            acc1 = __builtin_convertvector(ia1, f32x16);
        }
        if constexpr (H > 1) { if (sub == 0 && next_tile >= 0) stage(buf ^ 1, next_tile); }
    };

    auto block_max = [&](const f32x16& a, float& q0, float& q1, float& q2, float& q3) {
        q0 = fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3]));
        q1 = fmaxf(fmaxf(a[4], a[5]), fmaxf(a[6], a[7]));
        q2 = fmaxf(fmaxf(a[8], a[9]), fmaxf(a[10], a[11]));
        q3 = fmaxf(fmaxf(a[12], a[13]), fmaxf(a[14], a[15]));
        return fmaxf(fmaxf(q0, q1), fmaxf(q2, q3));
    };
    // Rare path of the top-k epilogue of one 32x32 accumulator: a[j] is (corpus row base + (j&3) +
    // 8*(j>>2), query r).  Only the quarters (rows 8g..8g+3 of this lane's 16) that hold a passing
    // score are walked.  A passing score parks in the lane's one pending slot; the 80-instruction
    // sorted insert runs only when some lane needs its slot again (then every lane's pending entry
    // goes in with that same pass).  thr may therefore lag behind -- it only admits extra
    // candidates, never drops one.
    auto insert_block = [&](const f32x16& a, int base) {
        float q0, q1, q2, q3;
        const float m = block_max(a, q0, q1, q2, q3);
        if (__builtin_amdgcn_ballot_w64(m > thr) == 0) return;
        auto walk = [&](float qm, int j0) {
            if (__builtin_amdgcn_ballot_w64(qm > thr) == 0) return;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int j = j0 + jj;
                const bool pass = a[j] > thr;
                if (__builtin_amdgcn_ballot_w64(pass) != 0) {
                    if (__builtin_amdgcn_ballot_w64(pass && pend_i >= 0) != 0) {
                        list_insert<KP>(ls, li, pend_s, pend_i);
                        pend_s = -INFINITY; pend_i = -1;
                        thr = fmaxf(ls[KP - 1], tau);
                    }
                    const bool still = a[j] > thr;
                    pend_s = still ? a[j] : pend_s;
                    pend_i = still ? base + acc_row(j) : pend_i;
                }
            }
        };
        walk(q0, 0); walk(q1, 4); walk(q2, 8); walk(q3, 12);     // ascending row order per lane
    };
    // AP: lanes flagged `need` hand their buffered rows to the query's candidate array (one atomic add per lane; what
    // does not fit the capacity is remembered as the largest lost key, exactly like the tail of a full list).
    auto flush = [&](bool need) {
        if (need && q_glob < nq) {
            const unsigned at = atomicAdd(A.cnt + q_glob, (unsigned)ecnt);
            unsigned long long* dst = A.cand + (size_t)q_glob * A.cap;
            unsigned long long lost = 0ull;
#pragma unroll
            for (int i = 0; i < E; ++i) {
                if (i < ecnt) {
                    const unsigned long long key = make_key(es[i], ei[i]);
                    if (at + (unsigned)i < (unsigned)A.cap) dst[at + i] = key;
                    else lost = lost > key ? lost : key;
                }
            }
            if (lost != 0ull && A.maxlast != nullptr) atomicMax(A.maxlast + q_glob, lost);   // (threshold form: the count alone tells)
        }
        ecnt = need ? 0 : ecnt;
    };
    auto append_block = [&](const f32x16& a, int base) {
        float q0, q1, q2, q3;
        const float m = block_max(a, q0, q1, q2, q3);
        if (__builtin_amdgcn_ballot_w64(m > thr) == 0) return;
        auto walk = [&](float qm, int j0) {
            if (__builtin_amdgcn_ballot_w64(qm > thr) == 0) return;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int j = j0 + jj;
                const bool pass = a[j] > thr;
                if (__builtin_amdgcn_ballot_w64(pass) != 0) {
                    const bool full = pass && ecnt == E;
                    if (__builtin_amdgcn_ballot_w64(full) != 0) flush(full);
#pragma unroll
                    for (int i = E - 1; i > 0; --i) { es[i] = pass ? es[i - 1] : es[i]; ei[i] = pass ? ei[i - 1] : ei[i]; }
                    es[0] = pass ? a[j] : es[0];
                    ei[0] = pass ? base + acc_row(j) : ei[0];
                    ecnt += pass ? 1 : 0;
                }
            }
        };
        walk(q0, 0); walk(q1, 4); walk(q2, 8); walk(q3, 12);
    };
    // THR: every score above the lane's fixed threshold goes straight to the query's candidate array
    // (rare by construction: the threshold sits an error bound below the k-th best score already known).
    auto emit_block = [&](const f32x16& a, int base) {
        float q0, q1, q2, q3;
        const float m = block_max(a, q0, q1, q2, q3);
        if (__builtin_amdgcn_ballot_w64(m > thr) == 0) return;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (a[j] > thr) {
                const unsigned pos = atomicAdd(A.cnt + q_glob, 1u);
                if (pos < (unsigned)A.cap) A.cand[(size_t)q_glob * A.cap + pos] = make_key(a[j], base + acc_row(j));
            }
        }
    };
    // Prologue: the first TWO tiles' DMA goes out before anything else (both buffers are free; from a cold start a tile
    // takes ~4 us to land, far longer than the bootstrap tile takes to scan), then the query rows are fetched and
    // converted under it.
    const bool two_ahead = H > 1 && niter > 1;          // (H == 1 issues a tile's successor before its MFMAs anyway)
    if (ntiles > 0) stage(0, tile_lo);
    if (two_ahead) stage(1, tile_of(1));
    if constexpr (MET) {
        int q_shift = 0;
        load_queries<RB, DT>(Qb, q_ld, h, qc, &q_shift);
        if constexpr (DT == DT_F16) {
            // (clamped to the normal range: beyond it the select kernels' bound is infinite and the query unproven anyway,
            //  select_dev.h query_bound -- but 0 x inf in the seeding MFMA would be a NaN)
            const int e = A.corpus_shift + q_shift;
            bscale = ldexpf(1.f, e < -126 ? -126 : e > 127 ? 127 : e);
        }
        bias_fetch(tile_of(0));
    } else {
        load_queries<RB, DT>(Qb, q_ld, h, qc);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if constexpr (MET) bias_land();

    // The scan advances in 64-row steps, t = tile iteration * H + sub-step.  The loop is split in two
    // so that the HOT loop (MFMAs, one max tree and one compare per step) never writes the list
    // state: a step whose maximum beats some lane's threshold leaves the hot loop, runs the rare
    // insert path on the still-live accumulators and re-enters.  (Written as one loop with the rare
    // path inside, the register allocator cannot keep the 35 state registers in place and pays
    // ~70 v_mov per step on the hot path.)
    const int T = niter * H;
    long row0_of_step = 0;                      // first corpus row of the current step
    // The threshold moves fast at first and then ever more slowly, and a stale one only admits extra candidates.  A
    // refresh is not cheap: its two LDS-DMA instructions (and the publish's atomic) queue behind the tile traffic of the
    // CU's memory pipe -- ~3 k cycles per wave, half a 128-row tile of a 16-bit scan (per-tile stamps).
    // With tau near the R-th best of the i tiles' rows seen so far, ~R / i rows per query pass per tile-time and a
    // threshold stale by D tiles admits ~R D / i^2 more: the cost of refreshing every D tiles, c_r / D + c_p D / i^2
    // per tile, is least at D ~ i -- so every scan refreshes at i = 2, 3, 4 and then at 2 and 3 times the powers of
    // two (6, 8, 12, 16, 24, ...: 12 refreshes of a 61-tile split instead of 21, 18 of 610 instead of 158).  The f32
    // scan (15 us per tile) refreshed every tile until round 4; the same schedule takes 2 % off it (4 % at 125 k rows).
    constexpr bool TAU_EVERY_TILE = TR >= 512;
    auto refresh_at = [&](int i) {
        // (no refresh in the tile right behind the bootstrap: the wave has just polled its threshold, and the first DMA
        //  fetch of the slot lines -- while every CU's bootstrap atomics are still draining at the memory side -- took
        //  ~25 k cycles to issue: per-tile stamps, round 4)
        if (i == 1 && boot && !TAU_EVERY_TILE) return false;
        if (TAU_EVERY_TILE || i <= 4) return true;
        const int sh = 30 - __builtin_clz(i);              // i = (2 or 3) << sh  <=>  its low sh bits are zero
        return (i & ((1 << sh) - 1)) == 0;
    };
    auto tile_top = [&](int i) {                // threshold refresh at the start of tile iteration i > 0
        if (!use_tau || i == 0) return;
        if (J == 16) {
            if (!refresh_at(i)) return;
            publish(cls_live);                  // (before the fetch: an atomic behind the two DMA instructions waits for them)
            tau_fetch();                        // lands under this tile's MFMAs
            return;
        }
        // J > 16 (k > 116): synchronous loads, rarely, staggered between the two waves of a
        // SIMD (waves 4-7 one tile later) so the partner keeps the matrix pipe busy meanwhile.
        const int ii = i - (wave >= 4 ? 1 : 0);        // (NW == 4: no SIMD partner, nothing to stagger)
        if (ii >= 2 && (ii <= 8 || (ii & (ii - 1)) == 0 || (ii & 15) == 0)) set_tau(tau_ord());
        publish(cls_live);                      // completes under this tile's MFMAs
    };
    auto tile_end = [&](int i) {
        const bool pre = boot && i == 0;
        if (pre) publish(cls_live);
        if constexpr (MET) { if (i + 1 < niter) bias_fetch(tile_of(i + 1)); }      // (this tile's biases are dead: its last step has been seeded)
        // this wave's share of the next tile landed (after the bootstrap tile: its own atomics did -- skipping this wait
        // there only moves it into the polling loop below, measured slower)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (use_tau && J == 16 && i > 0 && refresh_at(i)) { set_tau(tau_read()); slots_seen = true; }   // ... and so did its slots (own region: no barrier needed)
        __syncthreads();                                   // ... everyone's did, and this buffer is free
        if (pre) {
            // Wait (bounded) until every class of this wave's queries has published its bootstrap
            // maximum.  All workgroups of a launch are normally co-resident and reach this point
            // within a microsecond of each other; if not, the bound expires and the scan simply
            // runs with a weaker (or no) threshold -- correctness never depends on it.
            unsigned m = 0;
            // (the append form has nothing but the threshold to hold rows back: it waits much longer before it gives up)
            for (int it = 0; it < (AP ? 1024 : 24); ++it) {
                m = tau_ord();
                if (__builtin_amdgcn_ballot_w64(m == 0) == 0) break;
                __builtin_amdgcn_s_sleep(16);
            }
            // (debug counter, sss_scan_boot_expired: the wait ran out before K2 classes of every query had published --
            //  the workgroups of the launch were not co-resident; correct all the same, but the append form then floods)
            if constexpr (!MET) {
                if (lane == 0 && __builtin_amdgcn_ballot_w64(m == 0 && q_glob < nq) != 0) atomicAdd(&g_boot_expired, 1u);
            }
            set_tau(m);
        }
        if constexpr (MET) bias_land();
    };
    // MFMAs of step t into acc0 / acc1 (acc[j] is (corpus row row0 + (j&3) + 8*(j>>2) + 4h, query r),
    // acc1 32 rows further); score_tree() returns the lane's maximum over both.
    auto score_mfma = [&](int t) {
        const int i = (int)((unsigned)t / (unsigned)H), sub = (int)((unsigned)t % (unsigned)H);   // (unsigned: shifts, not the signed-division sequence)
        if (sub == 0) tile_top(i);
        const int next_tile = (i + 1 < niter && !(two_ahead && i == 0)) ? tile_of(i + 1) : -1;
        mfma_sub(i & 1, sub, next_tile);
        row0_of_step = (long)tile_of(i) * TR + sub * 64;
        if (row0_of_step + 64 > n) mask_rows(acc0, acc1, (int)row0_of_step + 4 * h, n);     // wave-uniform, last tile only
    };
    auto score_tree = [&]() -> float {
        // 16 v_max3 (as asm: fmaxf() adds a canonicalising v_max x, x per MFMA result it touches)
        float m0, m1;
        acc_max15(acc0, acc1, m0, m1);
        const float m = vmax3(m0, m1, acc0[15]);
        const float mm = vmax3(m, acc1[15], rmax);
        rmax = mm;
        return vmax3(m, acc1[15], acc1[15]);
    };
    const int t_live = nb * H;                  // steps of the bootstrap tile: lane maximum only
    // STAGGER (MI355X_MICROARCH.md, two waves per SIMD, item 9): the two waves of a SIMD run the same program and
    // leave every barrier together -- both into their MFMAs, then both into their max trees, the matrix pipe idle
    // meanwhile.  Waves 4-7 (the SIMD partners of waves 0-3) therefore take the end of a tile -- wait, threshold
    // refresh, barrier -- BEFORE the epilogue of its last step instead of after it (the accumulators simply stay
    // live across the barrier): after every barrier one partner starts with matrix work, the other with vector work.
    // Measured (same device, alternating builds): split scan -3.5 %, bf16 C5 -1.3 % time; f16 and f32 scans unchanged
    // to +1 % (their partners drift apart by themselves), so those keep the plain order.
    // (DT_H16 -- stored f16 rows -- and DT_I8 -- stored int8 rows -- are the bf16 kernel with another MFMA: they take the
    //  bf16 order)
    const bool defer = NW == 8 && (DT == DT_SPLIT || DT == DT_BF16 || DT == DT_H16 || DT == DT_I8) && wave >= 4;
    int t = 0;
    if constexpr (AP || THR) {
        // The forms WITHOUT lane lists (append, threshold) have no list state to keep out of the hot loop, so theirs is the
        // plain nest: tiles x (compile-time) sub-steps, the rare path an ordinary side branch.  What that buys is SCALAR
        // instructions: a SIMD issues one scalar instruction per 4 cycles, and the split loop below spends ~90 per
        // 64-row step on t / H, t % H, tile-of-iteration, 64-bit row arithmetic and the ragged-tile test -- with four
        // waves per SIMD that is ~70 % of the scalar issue slots of a step, the append form's real limit (the matrix
        // pipe is ~70 % busy, the two co-resident workgroups together finish in the same time however the SIMDs
        // arbitrate between them: section 5.1).  Here the per-tile values are computed once per tile.
        t = T;                                                  // (the split loop below is not entered)
        for (int i = 0; i < niter; ++i) {
            tile_top(i);
            const int tile = tile_of(i);
            const int next_tile = (i + 1 < niter && !(two_ahead && i == 0)) ? tile_of(i + 1) : -1;
            const int row_base = tile * TR;
            const bool ragged = row_base + TR > n;              // wave-uniform, last tile of the corpus only
            const bool live = i >= nb;
            if constexpr (THR) {
                // a wave whose 32 query slots are all padding (the rung's compact query list rarely fills the 256 slots of
                // a workgroup: ~100 unproven queries of a 1024-query batch leave waves 4-7 empty) stages its share of the
                // tiles and keeps the barriers, nothing else: the three-pass split scan of the rung is bound by the matrix
                // pipe, and an empty wave was taking half of its SIMD's
                if (g * WGQ + wave * 32 >= nq) {
                    if (next_tile >= 0) stage((i & 1) ^ 1, next_tile);
                    tile_end(i);
                    continue;
                }
            }
            // (unrolled: a single copy of the sub-step -- `#pragma unroll 1`, 6.4 k lines of ISA instead of 11.3 k, the
            //  rare path's ~20 KB of code once instead of twice -- measured the same at 1M rows and 5 % SLOWER at 10M)
#pragma unroll
            for (int sub = 0; sub < H; ++sub) {
                mfma_sub(i & 1, sub, next_tile);
                const int row0 = row_base + sub * 64;
                if (ragged) {
                    // (mask_rows(acc0, acc1, row0 + 4 * h, n) written out: through the helper, or with acc_row() for the row
                    //  term, hipcc compiles every append and threshold kernel differently -- DESIGN.md 5.1, the refactor's table)
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const int rr = row0 + 4 * h + (j & 3) + 8 * (j >> 2);
                        if (rr >= n) acc0[j] = -INFINITY;
                        if (rr + 32 >= n) acc1[j] = -INFINITY;
                    }
                }
                const float m = score_tree();
                if (live && __builtin_amdgcn_ballot_w64(m > thr) != 0) {
                    // (the threshold form used to hand every passing row to the candidate array with an atomic add of its own
                    //  -- fine for the rung's few queries and tight thresholds; the sampled large-k search keeps thousands of
                    //  rows per query: the append form's 4-entry register buffer, one atomic add per flush, serves both)
                    append_block(acc0, row0 + 4 * h);
                    append_block(acc1, row0 + 32 + 4 * h);
                }
            }
            tile_end(i);
        }
    }
    if constexpr (F32S) {
        // The f32 list form's own step order (512-byte rows).  One k-group of this scan is 8 v_mfma_f32_32x32x2_f32 = 512
        // matrix-pipe cycles during which the wave's issue port is idle, so everything a step needs besides its MFMAs is
        // issued BETWEEN the k-groups, in that shadow, instead of between the last MFMA of a step and the first of the
        // next (where the 16-bit scans, bound by instruction issue, want it):
        //  * the fragments of k-group 0 of the NEXT step are read during the last k-group of this one (nf0 / nf1 carry them
        //    over the step boundary and through the rare path): the first MFMA of a step waits for no LDS round trip;
        //  * the step's scalar values (tile, next tile, DMA source and destination, first row, ragged flag) and the
        //    threshold refresh of tile_top() follow the MFMAs of k-group 0, which need none of them;
        //  * the next tile's DMA pieces go out one per k-group, behind the MFMAs of k-groups 1 .. LOADS_PER_WAVE of the
        //    tile's first step (a ragged next tile -- the last tile of the corpus -- keeps the clamped burst);
        //  * the last k-group issues acc0's four MFMAs first, so acc0's half of the max tree runs under acc1's (the k order
        //    of each accumulator's chain is what it was: every score keeps its bits);
        //  * THE TILE HAND-OVER (tile_end: wait for the own DMA share, barrier) sits in front of the last k-group's MFMAs
        //    of the tile's last step, not behind the step.  Why that is enough: the fragments of that last k-group were
        //    read one group earlier and the wait for them (lgkmcnt) precedes the barrier, so a wave that arrives there has
        //    received every LDS read it will ever make of the current buffer; and its vmcnt(0) retired its share of the
        //    next tile.  Behind the barrier, therefore, (a) the current buffer is free for the DMA of the tile after the
        //    next -- which goes out during the NEXT tile's first step, i.e. behind this barrier -- and (b) everybody's share
        //    of the next tile has landed: exactly what the barrier at the end of the step guaranteed.  The last k-group's
        //    512 cycles then cover the next tile's first fragment reads and the threshold read-back.
        //    The bootstrap tile keeps the old order (publish behind its tree, wait, barrier, bounded poll): once a launch.
        //  * THE HALF-STEP SKEW: each accumulator's tree, compare and rare path run under the OTHER accumulator's
        //    MFMAs, across the step boundary.  acc0(t)'s tree and compare sit behind the second of acc1's last four MFMAs
        //    of step t; acc0's four MFMAs of k-group 0 of step t + 1 then overwrite it (its decision is made) and acc1(t)'s
        //    tree and compare sit behind the second of THOSE -- at least 128 pipe cycles after acc1's last MFMA was issued,
        //    so no wait states -- followed by acc1's four MFMAs of k-group 0.  Between the last MFMA of a step and the first
        //    of the next the plain path issues scalar instructions only.  The hot loop has two exits, one per half
        //    (insert_block of that accumulator alone; it re-enters where it left); every accumulator's k order is what it
        //    was.  The bootstrap tile's steps keep the whole step (nothing of them is compared); the last step's second
        //    half is drained behind the loop.
        static_assert(LOADS_PER_WAVE + 1 < NU, "a DMA piece per k-group, behind k-groups 1 .. LOADS_PER_WAVE");
        const unsigned frag_lane = (unsigned)(r * CH) * 16u;          // (the chunk term is added per k-group: compile-time xor)
        f32x4 nf0 = {0}, nf1 = {0};
        [[maybe_unused]] float nb0 = 0.f;                         // L2: the bias acc0 starts the next step from
        auto frag_ptr = [&](unsigned step_off, int u) -> const f32x4* {
            const int c = (2 * u) ^ x;                          // == (2u + h) ^ (r & 15)
            return reinterpret_cast<const f32x4*>(smem + step_off + frag_lane + c * 16);
        };
        // first fragments of the step at step_off, sub-step nsub of its tile (whose biases bcur holds by now)
        auto read_first = [&](unsigned step_off, [[maybe_unused]] int nsub) {
            const f32x4* p = frag_ptr(step_off, 0); nf0 = p[0]; nf1 = p[32 * CH];
            if constexpr (MET) nb0 = bias_of<H>(bcur, nsub, 0);
        };
        float tm0 = -INFINITY;                                    // acc0's half of the tree, taken under acc1's last MFMAs
        bool hit = false;                                         // some lane of the half just decided passes
        // The skew's first half: acc0's four MFMAs of k-group 0 of the step that follows step `row0_of_step`, and behind the second
        // of them the decision on that step's acc1 (whose last MFMA is two MFMA times back at the least)
        auto head = [&]() {
            const f32x4 a0 = nf0;
            const f32x16 zero = {0};
            const bool ragged_prev = row0_of_step + 64 > n;
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (MET) acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(nb0, bscale, zero, 0, 0, 0);
            else acc0 = zero;
            mfma_f32_pair(acc0, a0.x, a0.y, qc[0].x, qc[0].y);
            __builtin_amdgcn_sched_barrier(0);
            if (ragged_prev) mask_rows(acc1, (int)row0_of_step + 32 + 4 * h, n);
            float m1 = acc_max15(acc1);
            rmax = vmax3(m1, acc1[15], rmax);
            m1 = vmax3(m1, acc1[15], acc1[15]);
            hit = __builtin_amdgcn_ballot_w64(m1 > thr) != 0;
            __builtin_amdgcn_sched_barrier(0);
            mfma_f32_pair(acc0, a0.z, a0.w, qc[0].z, qc[0].w);
            __builtin_amdgcn_sched_barrier(0);
        };
        // MFMAs of step t (and, inside its last k-group, the hand-over when it ends a tile).  Whole (the bootstrap tile): the
        // lane's maximum over both accumulators goes into rmax, nothing is compared.
        // TAIL: the step behind head(), which has issued acc0's share of k-group 0 -- up to the decision on acc0, which it
        // leaves in `hit`; acc1 stays undecided.  (No caller reads the float it returns; it stays because a void step compiles
        // to another register assignment in the four kernels of this loop.)
        auto step = [&](int t, auto tail_c) -> float {
            constexpr bool TAIL = decltype(tail_c)::value;
            const int i = (int)((unsigned)t / (unsigned)H), sub = (int)((unsigned)t % (unsigned)H);
            const unsigned off = (unsigned)((i & 1) * TILE_BYTES + sub * (64 * RB));
            f32x4 as0[NU], as1[NU];
            as0[0] = nf0; as1[0] = nf1;
            const f32x16 zero = {0};
            if constexpr (MET) {
                if constexpr (!TAIL) acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(bias_of<H>(bcur, sub, 0), bscale, zero, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(bias_of<H>(bcur, sub, 1), bscale, zero, 0, 0, 0);
            } else {
                if constexpr (!TAIL) acc0 = zero;
                acc1 = zero;
            }
            auto fetch = [&](int u) { const f32x4* p = frag_ptr(off, u); as0[u] = p[0]; as1[u] = p[32 * CH]; };
            auto mfma8 = [&](int u) {
                const f32x4 a0 = as0[u], a1 = as1[u];
                __builtin_amdgcn_sched_barrier(0);   // keep the prefetch ABOVE this group's MFMAs
                mfma_f32_group(acc0, acc1, a0, a1, qc[u]);
                __builtin_amdgcn_sched_barrier(0);
            };
            // ---- k-group 0: its fragments came with the previous step; behind its MFMAs, whatever the step needs besides
            fetch(1);
            if constexpr (!TAIL) {
                mfma8(0);
            } else {
                const f32x4 a1 = as1[0];
                __builtin_amdgcn_sched_barrier(0);
                mfma_f32_pair(acc1, a1.x, a1.y, qc[0].x, qc[0].y);
                mfma_f32_pair(acc1, a1.z, a1.w, qc[0].z, qc[0].w);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (sub == 0) tile_top(i);
            const int next_tile = (sub == 0 && i + 1 < niter && !(two_ahead && i == 0)) ? tile_of(i + 1) : -1;
            const long nrow0 = (long)next_tile * TR;
            const bool dma_plain = next_tile >= 0 && nrow0 + TR <= (long)n;
            const char* dma_src = Cb + (size_t)nrow0 * RB;
            const unsigned dma_dst = __builtin_amdgcn_readfirstlane(lds_base + ((i & 1) ^ 1) * TILE_BYTES + wave * LOADS_PER_WAVE * 1024);
            row0_of_step = (long)tile_of(i) * TR + sub * 64;
            const bool ragged_step = row0_of_step + 64 > n;                 // wave-uniform, last tile only
            const bool ends_tile = sub == H - 1 && !(boot && i == 0);       // (the bootstrap tile's end comes behind its tree)
            if (next_tile >= 0 && !dma_plain) stage((i & 1) ^ 1, next_tile);
            // ---- k-groups 1 .. NU - 2, a DMA piece behind each of the first LOADS_PER_WAVE
#pragma unroll
            for (int u = 1; u < NU - 1; ++u) {
                fetch(u + 1);
                mfma8(u);
                if (u <= LOADS_PER_WAVE && dma_plain) lds_dma16(lane_off[u - 1], dma_dst + (u - 1) * 1024, dma_src);
            }
            // ---- the last k-group: the hand-over in front of its MFMAs when it ends a tile (see above)
            constexpr int u = NU - 1;
            if (ends_tile) {
                asm volatile("" : "+v"(as0[u]), "+v"(as1[u]));      // every LDS read this wave makes of the buffer has landed
                tile_end(i);
            }
            if (t + 1 < T && (sub < H - 1 || ends_tile))
                read_first(sub == H - 1 ? (unsigned)(((i + 1) & 1) * TILE_BYTES) : off + 64 * RB, sub == H - 1 ? 0 : sub + 1);
            // acc0's chain first (back to back on one accumulator is free: 64-cycle issue = the dependent latency); its
            // half of the tree goes in behind acc1's SECOND MFMA -- two MFMA times after acc0's last one was issued
            const f32x4 a0 = as0[u], a1 = as1[u];
            __builtin_amdgcn_sched_barrier(0);
            mfma_f32_pair(acc0, a0.x, a0.y, qc[u].x, qc[u].y);
            mfma_f32_pair(acc0, a0.z, a0.w, qc[u].z, qc[u].w);
            __builtin_amdgcn_sched_barrier(0);   // (acc0's last MFMA strictly in front of acc1's two: see the tree below)
            mfma_f32_pair(acc1, a1.x, a1.y, qc[u].x, qc[u].y);
            __builtin_amdgcn_sched_barrier(0);
            // (the tree is inline asm, which hipcc does not pad against the MFMA that wrote its operands: what keeps
            //  acc0's readers clear of acc0's last MFMA is the order -- acc1's second MFMA cannot issue before the
            //  first has had the pipe for its 64 cycles, and that one not before acc0's last has: 128 cycles, against
            //  the 19 wait states (76 cycles) a 16-pass MFMA's result needs before a VALU reads it)
            if (ragged_step) mask_rows(acc0, (int)row0_of_step + 4 * h, n);
            tm0 = acc_max15(acc0);
            if constexpr (TAIL) {       // acc0 is decided here; head() overwrites it
                rmax = vmax3(tm0, acc0[15], rmax);
                hit = __builtin_amdgcn_ballot_w64(vmax3(tm0, acc0[15], acc0[15]) > thr) != 0;
            }
            __builtin_amdgcn_sched_barrier(0);
            mfma_f32_pair(acc1, a1.z, a1.w, qc[u].z, qc[u].w);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (TAIL) return 0.f;
            if (ragged_step) mask_rows(acc1, (int)row0_of_step + 32 + 4 * h, n);
            const float m1 = acc_max15<true>(acc1);                   // (acc1's last MFMA is the instruction in front of it)
            const float m = vmax3(tm0, m1, acc0[15]);
            rmax = vmax3(m, acc1[15], rmax);
            return vmax3(m, acc1[15], acc1[15]);
        };
        constexpr std::false_type whole{};
        constexpr std::true_type tail{};
        if (T > 0) read_first(0, 0);
        for (; t < t_live; ++t) {           // bootstrap tile: lane maximum only; its end in the old order
            step(t, whole);
            if (t == t_live - 1) {
                tile_end(0);
                if (t + 1 < T) read_first((unsigned)TILE_BYTES, 0);
            }
        }
        if (t < T) {
#pragma unroll
            for (int j = 0; j < 16; ++j) acc1[j] = -INFINITY;     // no second half waits for its decision yet
            head();                         // (decides nothing: the hot loop is entered at its second half)
            for (;;) {
                int rare = 0;
                for (;;) {                  // ---- hot loop (never writes the list state)
                    step(t, tail);
                    ++t;
                    if (hit) { rare = 2; break; }
                    if (t == T) break;
                    head();
                    if (hit) { rare = 1; break; }
                }
                // (row0_of_step is the first row of the step both exits decide on: it moves behind k-group 0)
                if (rare == 2) {
                    insert_block(acc0, (int)row0_of_step + 4 * h);
                    if (t == T) break;
                    head();                 // outside the hot loop this once
                    if (hit) rare = 1;
                }
                if (rare == 1) insert_block(acc1, (int)row0_of_step + 32 + 4 * h);
                if (t == T) break;
            }
            // the last step's second half (insert_block tests it itself)
            if (row0_of_step + 64 > n) mask_rows(acc1, (int)row0_of_step + 32 + 4 * h, n);
            insert_block(acc1, (int)row0_of_step + 32 + 4 * h);
        }
    }
    while (!F32S && t < T) {
        bool rare = false;
        for (; t < T; ++t) {                    // ---- hot loop
            const bool last = (unsigned)t % (unsigned)H == H - 1;
            const bool early = defer && t >= t_live;        // (not on the bootstrap tile: its end publishes the tile's maxima)
            score_mfma(t);
            if (early && last) tile_end((int)((unsigned)t / (unsigned)H));
            const float m = score_tree();
            if (t >= t_live && __builtin_amdgcn_ballot_w64(m > thr) != 0) { rare = true; break; }
            if (!early && last) tile_end((int)((unsigned)t / (unsigned)H));
        }
        if (!rare) break;
        if constexpr (THR) {
            emit_block(acc0, (int)row0_of_step + 4 * h);
            emit_block(acc1, (int)row0_of_step + 32 + 4 * h);
        } else if constexpr (AP) {
            append_block(acc0, (int)row0_of_step + 4 * h);
            append_block(acc1, (int)row0_of_step + 32 + 4 * h);
        } else {
            insert_block(acc0, (int)row0_of_step + 4 * h);
            insert_block(acc1, (int)row0_of_step + 32 + 4 * h);
        }
        if (!defer && (unsigned)t % (unsigned)H == H - 1) tile_end((int)((unsigned)t / (unsigned)H));    // (rare implies t >= t_live)
        ++t;
    }
    if constexpr (THR) { flush(ecnt > 0); return; }
    if constexpr (AP) flush(ecnt > 0);
    list_insert<KP>(ls, li, pend_s, pend_i);   // no-op for lanes with an empty slot (-inf)
    // ---- append the real entries to the query's compact candidate array (none in the append form: li stayed -1)
    if (!AP && q_glob < nq) {
        int nreal = 0;
#pragma unroll
        for (int i = 0; i < KP; ++i) nreal += li[i] >= 0 ? 1 : 0;
        if (nreal > 0) {
            const unsigned base = atomicAdd(A.cnt + q_glob, (unsigned)nreal);
            unsigned long long* dst = A.cand + (size_t)q_glob * A.cap + base;
#pragma unroll
            for (int i = 0; i < KP; ++i)
                if (i < nreal) dst[i] = make_key(ls[i], li[i]);
            if (nreal == KP) atomicMax(A.maxlast + q_glob, (unsigned long long)make_key(ls[KP - 1], li[KP - 1]));
        }
    }
}

// ------------------------------------------------------------------------------ launch
template <int RB, int TR, int DT, int NW, int MET, bool THR, bool AP = false>
static int launch_form(const ScanArgs& a, hipStream_t st) {
    const size_t lds = 2 * (size_t)TR * RB + NW * 2048;      // two tile buffers + the threshold-slot staging
    const int rc = opt_in_lds(reinterpret_cast<const void*>(&k_scan<RB, TR, DT, NW, THR, AP, MET>), "k_scan", lds);
    if (rc) return rc;
    hipLaunchKernelGGL((k_scan<RB, TR, DT, NW, THR, AP, MET>), dim3(a.S * a.G), dim3(NW * 64), lds, st, a);
    return check_launch("k_scan");
}
template <int RB, int TR, int DT, int NW, int MET>
static int launch_one(const ScanArgs& a, hipStream_t st) {
    // the threshold form is compiled for one tile shape per row size (make_thr_plan picks it)
    if (a.thr != nullptr) {
        if constexpr (TR == (RB <= 512 ? 128 : 64)) return launch_form<RB, TR, DT, NW, MET, true>(a, st);
        set_error("scan: threshold form not built for %d-row tiles of %d-byte rows", TR, RB);
        return SSS_EINVAL;
    }
    if (a.append) {
        if constexpr (RB == 256 && TR == 128 && DT != DT_F32) return launch_form<RB, TR, DT, NW, MET, false, true>(a, st);
        set_error("scan: append form not built for this shape");
        return SSS_EINVAL;
    }
    return launch_form<RB, TR, DT, NW, MET, false>(a, st);
}
// the kernel of one (element type, metric) for the row size and tile shape of the plan; 1: no such row size
template <int DT, int MET>
static int launch_shape(int rb, int tile_rows, const ScanArgs& a, hipStream_t st) {
    if (rb == 256) return tile_rows == 256 ? launch_one<256, 256, DT, 8, MET>(a, st) : launch_one<256, 128, DT, 8, MET>(a, st);
    if (rb == 512) return tile_rows == 128 ? launch_one<512, 128, DT, 8, MET>(a, st) : launch_one<512, 64, DT, 8, MET>(a, st);
    if (rb == 1024) return launch_one<1024, 64, DT, 4, MET>(a, st);
    return 1;
}

}  // namespace sss
