// The WordPiece tokenizer: BERT input ids out of the code points of a string table (the reference's
// tokenizer(strings, padding='max_length', max_length=20, truncation=True), util_amazon_filtered.py:19-20, 120-121).
// C ABI, the score of record and the table formats: include/tok/sss_wordpiece.h; DESIGN.md section 5.14.
//
//   k_wordpiece   one wave per string, four strings per 256-thread workgroup.  Every phase ends at a __syncthreads all four
//                 waves reach exactly once (a wave without a string walks the phases with nothing to do).
//                 1. MAP.  64 code points at a time through the two-level character map; a wave prefix sum of the 0 to 3
//                    mapped characters per code point places them, packed with their class, in the wave's LDS row (at most
//                    3 x 1024 of them, 12 KiB).  A code point outside [0, 0x10FFFF] is never looked up.
//                 2. WORDS.  64 mapped characters at a time: a character starts a word if it is PUNCT, or OTHER after a
//                    character that is not; it ends one if it is PUNCT, or OTHER before a character that is not (a SPACE
//                    sentinel follows the last).  Two ballot compactions keep the first T - 2 starts and ends -- the k-th
//                    end belongs to the k-th start.  A later word can never reach the output: every word emits a piece.
//                 3. PIECES.  One lane per kept word.  From each piece start the end is extended one character at a time,
//                    the FNV state updated incrementally and the table probed at every length; the last confirmed hit is
//                    the longest match.  A piece id overwrites a character of its own word the lane has already consumed
//                    (the k-th piece of a word starts at or after its k-th character), so emission needs no LDS of its own.
//                 4. FRAME.  A wave prefix sum over the words' piece counts places the pieces in a 64-entry row; lane t
//                    writes ids[row][t]: coalesced.
//                 Vector loads and stores only; the error word is one atomicOr per offending string.
#include "sss_common.h"
#include "../../include/ext/sss_seqsim.h"
#include "../../include/tok/sss_wordpiece.h"

namespace sss {

constexpr int WP_WAVES = 4;
constexpr int WP_MAXC = 3 * SSS_STR_MAX_CHARS;            // mapped characters of one string
constexpr int WP_CP = 0x1FFFFF;                           // a packed mapped character: code point | class << 24
constexpr int WP_CLS_SHIFT = 24;
constexpr int WP_CHAR = WP_CP | (3 << WP_CLS_SHIFT);
constexpr int WP_OTHER = 0, WP_SPACE = 1, WP_PUNCT = 2;
constexpr int WP_SPACE_CHAR = 0x20 | (WP_SPACE << WP_CLS_SHIFT);
static_assert(SSS_WP_MAX_T == 64 && SSS_WP_CONT == WP_CP + 1 && SSS_WP_PAGES * 256 == 0x110000, "the header's constants");

__device__ __forceinline__ int wp_cls(int c) { return (c >> WP_CLS_SHIFT) & 3; }

__device__ __forceinline__ int wp_incl_scan(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

__device__ __forceinline__ unsigned wp_finish(unsigned h) {
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    return h;
}

// The id of the piece m[p .. q) (its first element marked with `first_mark`), or -1: linear probing from hash & mask to
// the first empty slot, a hit confirmed against the stored key.  At most table_slots probes, whatever the table holds.
__device__ __forceinline__ int wp_lookup(const int2* __restrict__ slots, unsigned mask, const int* __restrict__ piece_ptr,
                                         const int* __restrict__ piece_chars, int vocab_size, unsigned hash, const int* m, int p,
                                         int q, int first_mark) {
    unsigned slot = hash & mask;
    for (unsigned t = 0; t <= mask; ++t) {
        const int2 s = slots[slot];
        if (s.x < 0) return -1;
        if ((unsigned)s.y == hash && s.x < vocab_size) {
            const int a = piece_ptr[s.x], b = piece_ptr[s.x + 1];
            if (b - a == q - p) {
                bool same = (piece_chars[a] == ((m[p] & WP_CP) | first_mark));
                for (int k = 1; same && k < q - p; ++k) same = piece_chars[a + k] == (m[p + k] & WP_CP);
                if (same) return s.x;
            }
        }
        slot = (slot + 1) & mask;
    }
    return -1;
}

__global__ __launch_bounds__(WP_WAVES * 64) void k_wordpiece(
    const long* __restrict__ str_ptr, const int* __restrict__ str_chars, long n, long n_chars, const int* __restrict__ map_page,
    const int* __restrict__ map_entry, int n_pages, const int* __restrict__ map_ext, int n_ext, const int2* __restrict__ slots,
    unsigned slot_mask, const int* __restrict__ piece_ptr, const int* __restrict__ piece_chars, int vocab_size, int max_piece_len,
    int max_word_chars, int unk_id, int cls_id, int sep_id, int pad_id, int T, int* __restrict__ ids, int* __restrict__ n_tok,
    int* __restrict__ err) {
    __shared__ int s_m[WP_WAVES][WP_MAXC + 1];            // (+1: the sentinel after the last mapped character)
    __shared__ int s_ws[WP_WAVES][64], s_we[WP_WAVES][64], s_out[WP_WAVES][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * WP_WAVES + wave;
    const bool active = row < n;
    int* m = s_m[wave];
    int* ws = s_ws[wave];
    int* we = s_we[wave];
    int* out = s_out[wave];
    const int Tm2 = T - 2;

    // ---- 1. map
    int errbits = 0, len = 0, total = 0;
    long base = 0;
    if (active) {
        const long p0 = str_ptr[row], p1 = str_ptr[row + 1];
        if (p0 < 0 || p1 < p0 || p1 > n_chars || p1 - p0 > SSS_STR_MAX_CHARS) {
            errbits |= SSS_WP_ERR_LENGTH;
        } else {
            base = p0;
            len = (int)(p1 - p0);
        }
    }
    for (int c0 = 0; c0 < len; c0 += 64) {
        const int i = c0 + lane;
        int cnt = 0, nn = 0, e = 0, cp = 0;
        bool bad = false;
        if (i < len) {
            cp = str_chars[base + i];
            if ((unsigned)cp > 0x10FFFFu) {
                bad = true;
            } else {
                int page = map_page[cp >> 8];
                if ((unsigned)page >= (unsigned)n_pages) page = 0;
                e = map_entry[page * 256 + (cp & 255)];
                nn = (e >> 28) & 3;
                if (nn >= 2 && (e & 0xFFFFFF) + nn > n_ext) nn = 0;
                cnt = nn + ((nn <= 1 && ((e >> 26) & 1)) ? 2 : 0);
            }
        }
        if (__ballot(bad)) errbits |= SSS_WP_ERR_CODEPOINT;
        const int incl = wp_incl_scan(cnt, lane);
        const int pos = total + incl - cnt;
        if (cnt && pos + cnt <= WP_MAXC) {
            if (nn >= 2) {
                const int off = e & 0xFFFFFF;
                for (int k = 0; k < nn; ++k) m[pos + k] = map_ext[off + k] & WP_CHAR;
            } else {
                int at = pos;
                const bool spaced = (e >> 26) & 1;
                if (spaced) m[at++] = WP_SPACE_CHAR;
                if (nn == 1) m[at++] = ((cp + (e & WP_CP)) & WP_CP) | (e & (3 << WP_CLS_SHIFT));
                if (spaced) m[at] = WP_SPACE_CHAR;
            }
        }
        total += __shfl(incl, 63, 64);
    }
    if (total > WP_MAXC) total = WP_MAXC;                 // (3 per code point at most: never taken)
    if (errbits) total = 0;                               // the row is [CLS] [SEP]
    if (lane == 0) m[total] = WP_SPACE_CHAR;
    __syncthreads();

    // ---- 2. words
    int nst = 0, nen = 0;
    for (int j0 = 0; j0 < total && nen < Tm2; j0 += 64) {
        const int j = j0 + lane;
        bool st = false, en = false;
        if (j < total) {
            const int c = wp_cls(m[j]), before = j ? wp_cls(m[j - 1]) : WP_SPACE, after = wp_cls(m[j + 1]);
            st = c == WP_PUNCT || (c == WP_OTHER && before != WP_OTHER);
            en = c == WP_PUNCT || (c == WP_OTHER && after != WP_OTHER);
        }
        const unsigned long long bs = __ballot(st), be = __ballot(en), below = (1ull << lane) - 1ull;
        if (st) {
            const int k = nst + __popcll(bs & below);
            if (k < Tm2) ws[k] = j;
        }
        if (en) {
            const int k = nen + __popcll(be & below);
            if (k < Tm2) we[k] = j + 1;
        }
        nst += __popcll(bs);
        nen += __popcll(be);
    }
    const int nw = nst < Tm2 ? nst : Tm2;                  // (each has its end: the loop stops at the text's end or at T - 2 ends)
    __syncthreads();

    // ---- 3. pieces
    int cnt = 0, s = 0;
    if (lane < nw) {
        s = ws[lane];
        const int e = we[lane];
        bool unk = e - s > max_word_chars;
        int p = s;
        while (!unk && p < e) {
            unsigned h = 2166136261u;
            int best = -1, best_end = p;
            const int first_mark = p > s ? SSS_WP_CONT : 0;
            const int lim = e - p < max_piece_len ? e : p + max_piece_len;
            for (int q = p; q < lim; ++q) {
                h = (h ^ (unsigned)((m[q] & WP_CP) | (q == p ? first_mark : 0))) * 16777619u;
                const int id = wp_lookup(slots, slot_mask, piece_ptr, piece_chars, vocab_size, wp_finish(h), m, p, q + 1, first_mark);
                if (id >= 0) {
                    best = id;
                    best_end = q + 1;
                }
            }
            if (best < 0) {
                unk = true;
            } else {
                m[s + cnt++] = best;                       // s + cnt <= p < best_end: a character this lane is done with
                p = best_end;
            }
        }
        if (unk) {
            m[s] = unk_id;
            cnt = 1;
        }
    }

    // ---- 4. frame
    const int incl = wp_incl_scan(cnt, lane);
    const int off = incl - cnt;
    int pieces = __shfl(incl, 63, 64);
    if (pieces > Tm2) pieces = Tm2;
    for (int k = 0; k < cnt && off + k < Tm2; ++k) out[1 + off + k] = m[s + k];
    __syncthreads();
    if (active) {
        if (lane < T) {
            const int v = lane == 0 ? cls_id : lane <= pieces ? out[lane] : lane == pieces + 1 ? sep_id : pad_id;
            ids[row * T + lane] = v;
        }
        if (lane == 0) {
            n_tok[row] = pieces + 2;
            if (errbits) atomicOr(err, errbits);
        }
    }
}

// ------------------------------------------------------------------------------ host launcher
extern "C" int sss_wordpiece_encode(const int64_t* str_ptr, const int32_t* str_chars, int64_t n, int64_t n_chars,
                                    const int32_t* map_page, const int32_t* map_entry, int n_pages, const int32_t* map_ext, int n_ext,
                                    const int32_t* slots, int64_t table_slots, const int32_t* piece_ptr, const int32_t* piece_chars,
                                    int64_t vocab_size, int max_piece_len, int max_word_chars, int unk_id, int cls_id, int sep_id,
                                    int pad_id, int T, int32_t* ids, int32_t* n_tok, int32_t* err, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n < 0 || n >= (1L << 31) || n_chars < 0) {
        set_error("wordpiece_encode: need 0 <= n < 2^31 and 0 <= n_chars");
        return SSS_EINVAL;
    }
    if (T < 2 || T > SSS_WP_MAX_T) {
        set_error("wordpiece_encode: need 2 <= T <= 64, got %d", T);
        return SSS_EINVAL;
    }
    if (n_pages <= 0 || n_pages > SSS_WP_PAGES || n_ext < 0 || n_ext >= (1 << 24)) {
        set_error("wordpiece_encode: need 0 < n_pages <= 4352 and 0 <= n_ext < 2^24");
        return SSS_EINVAL;
    }
    if (vocab_size <= 0 || table_slots <= vocab_size || table_slots > (1L << 30) || (table_slots & (table_slots - 1))) {
        set_error("wordpiece_encode: table_slots must be a power of two with 0 < vocab_size < table_slots <= 2^30");
        return SSS_EINVAL;
    }
    if (max_piece_len < 1 || max_word_chars < 1) {
        set_error("wordpiece_encode: need 1 <= max_piece_len and 1 <= max_word_chars");
        return SSS_EINVAL;
    }
    const int special[4] = {unk_id, cls_id, sep_id, pad_id};
    for (int i = 0; i < 4; ++i)
        if (special[i] < 0 || special[i] >= vocab_size) {
            set_error("wordpiece_encode: a special id (unk, cls, sep, pad) lies outside [0, vocab_size): %d", special[i]);
            return SSS_EINVAL;
        }
    if (!str_ptr || !str_chars || !map_page || !map_entry || !map_ext || !slots || !piece_ptr || !piece_chars || !ids || !n_tok || !err) {
        set_error("wordpiece_encode: a null pointer (the string table, the character map, the vocabulary tables, ids, n_tok and err "
                  "are required)");
        return SSS_EINVAL;
    }
    if (reinterpret_cast<uintptr_t>(slots) & 7) {
        set_error("wordpiece_encode: slots must be aligned to 8 bytes (it is read a pair at a time)");
        return SSS_EINVAL;
    }
    if (n == 0) return SSS_OK;
    if (hipMemsetAsync(err, 0, sizeof(int), st) != hipSuccess) {
        set_error("wordpiece_encode: memset failed");
        return SSS_EHIP;
    }
    const unsigned nb = (unsigned)((n + WP_WAVES - 1) / WP_WAVES);
    hipLaunchKernelGGL(k_wordpiece, dim3(nb), dim3(WP_WAVES * 64), 0, st, str_ptr, str_chars, n, n_chars, map_page, map_entry, n_pages,
                       map_ext, n_ext, reinterpret_cast<const int2*>(slots), (unsigned)(table_slots - 1), piece_ptr, piece_chars,
                       (int)vocab_size, max_piece_len, max_word_chars, unk_id, cls_id, sep_id, pad_id, T, ids, n_tok, err);
    return check_launch("k_wordpiece");
}

}  // namespace sss
