/* Oracle: exact flat inner-product search in plain C.  TEST INFRASTRUCTURE ONLY.
 *
 * CPU restatement of what the reference asks of faiss at test_amazon_filterd.py:578
 * (IndexFlatIP.search; semantics SURVEY.md Appendix A.5) under the canonical contract of
 * score(a,b) = sum_{k=0..d-1} q[a][k]*c[b][k] accumulated sequentially in double
 * (each float*float product is exact in double) and rounded once to float; results ordered by
 * (score descending, id ascending); missing results id -1, score -FLT_MAX.
 * PARITY UNPINNED: faiss is not installed and the reference holds no fixture for this path.
 *
 * Also the grouped GEMM's k-ordered float32 fma chain (oracle_linear_chain, see there).
 *
 * Built by oracle/Makefile into oracle/libsss_oracle.so; loaded by oracle/search_ref.py.
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#ifdef _OPENMP
#include <omp.h>
#endif

/* insert (s,id) into a list sorted by (score desc, id asc); ids arrive ascending per query,
 * so a strict '>' keeps equal scores in id order. */
static inline void insert_sorted(float* D, int64_t* I, int k, float s, int64_t id) {
    if (I[k - 1] >= 0 && !(s > D[k - 1])) return; /* full list and not better than its tail */
    int p = k - 1;                                /* empty slots (id -1) lose to any entry */
    while (p > 0 && (I[p - 1] < 0 || s > D[p - 1])) {
        D[p] = D[p - 1];
        I[p] = I[p - 1];
        --p;
    }
    D[p] = s;
    I[p] = id;
}

static int search_impl(const float* q, int64_t nq, const float* c, int64_t n, int d, int k,
                       int64_t id_offset, float* D, int64_t* I, int threads, int mode) {
#ifdef _OPENMP
    if (threads > 0) omp_set_num_threads(threads);
#endif
#pragma omp parallel for schedule(dynamic, 4)
    for (int64_t a = 0; a < nq; ++a) {
        float* Da = D + a * k;
        int64_t* Ia = I + a * k;
        for (int j = 0; j < k; ++j) { Da[j] = -FLT_MAX; Ia[j] = -1; }
        const float* qa = q + a * d;
        for (int64_t b = 0; b < n; ++b) {
            const float* cb = c + b * d;
            float s;
            if (mode == 0) {
                double acc = 0.0;
                for (int t = 0; t < d; ++t) acc += (double)qa[t] * (double)cb[t];
                s = (float)acc;
            } else {
                float acc = 0.0f; /* k-ordered float fma chain == gfx950 f32 MFMA numerics */
                for (int t = 0; t < d; ++t) acc = fmaf(qa[t], cb[t], acc);
                s = acc;
            }
            insert_sorted(Da, Ia, k, s, b + id_offset);
        }
    }
    return 0;
}

int oracle_search_exact(const float* q, int64_t nq, const float* c, int64_t n, int d, int k,
                        int64_t id_offset, float* D, int64_t* I, int threads) {
    return search_impl(q, nq, c, n, d, k, id_offset, D, I, threads, 0);
}

int oracle_search_fp32(const float* q, int64_t nq, const float* c, int64_t n, int d, int k,
                       int64_t id_offset, float* D, int64_t* I, int threads) {
    return search_impl(q, nq, c, n, d, k, id_offset, D, I, threads, 1);
}

/* The gfx950 grouped GEMM's arithmetic (k_linear_grouped, linear.hip), element by element:
 * out[r][c] = fl(chain(r, c) + bias[c]) with chain one correctly rounded fmaf per k, starting from +0,
 * in the kernel's k order.  Per 32-wide K chunk k0 the kernel issues, for u = 0..3, four
 * v_mfma_f32_32x32x2_f32 steps (a.x, a.y, a.z, a.w); the lanes with h = 0 hold k0+8u+0..3 and the
 * lanes with h = 1 hold k0+8u+4..7, and one step accumulates its h = 0 product first.  So:
 *   for k0, for u in 0..3, for i in 0..3:  k0+8u+i,  then  k0+8u+4+i.
 * The bias is a separate float32 add (no fma).  K % 32 == 0; strides in floats. */
int oracle_linear_chain(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, int64_t n, int m,
                        int K, float* out, int64_t ldo) {
    if (K <= 0 || K % 32 || n < 0 || m < 0) return -1;
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t r = 0; r < n; ++r) {
        const float* xr = x + r * ldx;
        for (int c = 0; c < m; ++c) {
            const float* wc = w + (int64_t)c * ldw;
            float acc = 0.0f;
            for (int k0 = 0; k0 < K; k0 += 32)
                for (int u = 0; u < 4; ++u)
                    for (int i = 0; i < 4; ++i) {
                        const int ka = k0 + 8 * u + i, kb = ka + 4;
                        acc = fmaf(xr[ka], wc[ka], acc);
                        acc = fmaf(xr[kb], wc[kb], acc);
                    }
            out[r * ldo + c] = acc + (bias ? bias[c] : 0.0f);
        }
    }
    return 0;
}

/* fmaf element-wise, for checking the chain's single step against exact rational arithmetic. */
void oracle_fmaf(const float* a, const float* b, const float* c, float* out, int64_t n) {
    for (int64_t i = 0; i < n; ++i) out[i] = fmaf(a[i], b[i], c[i]);
}
