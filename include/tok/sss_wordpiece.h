/* libsss, the WordPiece tokenizer -- the reference's tokenizer(strings, padding='max_length', max_length=20,
 * truncation=True) (util_amazon_filtered.py:19-20, 120-121: every query node and every product title of sequence_to_graph)
 * for the strings of a string table, on the device: BERT input ids out of code points.  Same library (libsss.so) and the
 * same conventions as sss.h; this header lives in include/tok/ and is bound through _lib.TOK_HEADERS.  Python:
 * sessionsimilaritysearch_amd/wordpiece.py (the tables below are built there); DESIGN.md section 5.14.
 *
 * Conventions:
 *   - all buffers are CALLER-OWNED DEVICE pointers (tensor.data_ptr()); nothing is allocated
 *     or freed here and there is no host synchronisation: work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream);
 *   - return 0 on success, -1 bad argument, -3 HIP error (there is no workspace, so no -2);
 *     sss_last_error() (sss.h) returns the thread-local message of the last failure;
 *   - re-entrant per stream; no global state except the error string;
 *   - arguments are validated before anything is launched.
 *
 * THE SCORE OF RECORD: the single-sentence pipeline of a BERT tokenizer (integers; the result is bit-exact).
 *
 *   1. THE CHARACTER MAP.  Every input code point becomes 0 to 3 MAPPED CHARACTERS, each with a class -- OTHER (0),
 *      SPACE (1) or PUNCT (2) -- by a table lookup; no rule looks at a neighbour (no final sigma, no canonical reordering
 *      of the marks that survive).  The host builds the table from the Unicode character database:
 *        - U+0000, U+FFFD and the categories Cc / Cf / Co are dropped, except \t \n \r, which become a space;
 *        - Zs becomes a space;
 *        - otherwise, under strip_accents: the canonical decomposition (NFD) with its Mn characters dropped; then, under
 *          do_lower_case: each remaining code point through the single-character lower-casing (strip_accents = None
 *          follows do_lower_case);
 *        - under tokenize_chinese_chars a code point of the CJK ranges gets a space on either side of its mapped form
 *          (the compatibility ideographs U+F900-FAFF and U+2F800-2FA1F are decomposed and still spaced);
 *        - unassigned code points (Cn) are kept as they are, OTHER;
 *        - classes of a mapped character: SPACE for U+0020 and the categories Zl / Zp; PUNCT for the ASCII ranges 33-47,
 *          58-64, 91-96, 123-126 and every category P*; OTHER for the rest.
 *   2. WORDS.  A word is a maximal run of OTHER characters; every PUNCT character is a word of its own.
 *   3. WORDPIECE.  A word of more than max_word_chars mapped characters is one unk_id.  Otherwise pieces are matched
 *      greedily from the left, the longest first; a piece that does not start its word is looked up as a CONTINUATION piece
 *      (the vocabulary's "##" entries).  A position no piece starts at makes the whole word one unk_id.
 *   4. FRAMING.  ids[u] = cls_id, the first T - 2 pieces of the string, sep_id, then pad_id up to T;  n_tok[u] = the
 *      positions before the padding, cls_id and sep_id included (the attention mask is 1 on exactly those).
 *
 * THE TABLES (int32, built by the host; the kernel trusts their internal offsets and bounds what it reads by the sizes
 * passed with them):
 *   map_page  [SSS_WP_PAGES]   the page of code points 256 p .. 256 p + 255, in [0, n_pages); equal pages are stored once
 *   map_entry [n_pages, 256]   bits 28-29: n, the number of mapped characters (0 to 3);
 *                              n <= 1: bits 0-20 delta -- the mapped code point is (cp + delta) mod 2^21 --, bits 24-25 its
 *                                      class, bit 26: a space on either side (the CJK rule);
 *                              n >= 2: bits 0-23 the offset of the n mapped characters in map_ext
 *   map_ext   [n_ext]          mapped characters: bits 0-20 the code point, bits 24-25 the class
 *   slots     [table_slots, 2] the vocabulary, open addressing with linear probing: (token id, or -1 for an empty slot;
 *                              the key hash of the token).  table_slots is a power of two greater than vocab_size, so a
 *                              probe sequence always ends at an empty slot.
 *   piece_ptr [vocab_size + 1], piece_chars: token t's KEY is piece_chars[piece_ptr[t] .. piece_ptr[t + 1]): its code
 *                              points without the "##" of a continuation piece, SSS_WP_CONT OR-ed into the first key
 *                              element of a continuation piece.
 *   THE KEY HASH of a key k[0 .. len) (32-bit unsigned arithmetic, the same on the host and on the device):
 *       h = 2166136261;   for i in 0 .. len - 1:  h = (h ^ k[i]) * 16777619;          (FNV-1a over whole elements)
 *       h = h ^ (h >> 15);   h = h * 0x2C1B3C6D;   h = h ^ (h >> 12);                  hash = h
 *     The first slot probed is hash & (table_slots - 1), the next one slot further (wrapping).  A slot is a hit only if its
 *     hash equals AND the stored key equals the candidate, element by element: a hash collision costs a probe and can never
 *     change a result.
 *
 * ERRORS IN THE DATA never fault and never truncate: err (int32 [1], zeroed by the call) gets SSS_WP_ERR_CODEPOINT OR-ed
 * in for a string with a code point outside [0, 0x10FFFF] and SSS_WP_ERR_LENGTH for a string of more than
 * SSS_STR_MAX_CHARS (include/ext/sss_seqsim.h: 1024) code points or one whose extent leaves [0, n_chars); such a row is
 * written as cls_id, sep_id and padding (n_tok = 2) and every other row is unaffected.
 */
#ifndef SSS_WORDPIECE_H
#define SSS_WORDPIECE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SSS_WP_PAGES 4352             /* 0x110000 / 256 */
#define SSS_WP_CONT 2097152           /* 1 << 21: marks the first key element of a continuation piece */
#define SSS_WP_MAX_T 64               /* one lane per output position */
#define SSS_WP_ERR_CODEPOINT 1
#define SSS_WP_ERR_LENGTH 2

/* ids int32 [n, T] and n_tok int32 [n] of the n strings of the string table (str_ptr int64 [n + 1], str_chars int32
 * [n_chars]: the layout of include/ext/sss_seqsim.h), as the score of record above states them.
 * 0 <= n < 2^31 (n == 0 returns 0 and touches nothing); 0 <= n_chars; 0 < n_pages <= SSS_WP_PAGES; 0 <= n_ext < 2^24;
 * 0 < vocab_size < table_slots <= 2^30, table_slots a power of two; 1 <= max_piece_len; 1 <= max_word_chars; the four
 * special ids in [0, vocab_size); 2 <= T <= SSS_WP_MAX_T.  No pointer may be NULL (an empty chars or map_ext array is still
 * an allocation). */
int sss_wordpiece_encode(const int64_t* str_ptr, const int32_t* str_chars, int64_t n, int64_t n_chars, const int32_t* map_page,
                         const int32_t* map_entry, int n_pages, const int32_t* map_ext, int n_ext, const int32_t* slots,
                         int64_t table_slots, const int32_t* piece_ptr, const int32_t* piece_chars, int64_t vocab_size,
                         int max_piece_len, int max_word_chars, int unk_id, int cls_id, int sep_id, int pad_id, int T,
                         int32_t* ids, int32_t* n_tok, int32_t* err, void* stream);

#ifdef __cplusplus
}
#endif
#endif
