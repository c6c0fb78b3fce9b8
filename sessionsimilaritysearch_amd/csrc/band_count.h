// Internal: the band kernels of the ground-truth kinds (k_jaccard_bands in jaccard.hip, k_ptype_bands in ptype.hip).  Both
// walk csr_walk.h's rows, turn every (query, row) pair into one float64 score (their Kind's pair), and need, per query, the
// rows of every band and the lowest row in it.  The frame (csr_bands), the ballot and the flush are here, once.
//
//   per query one ballot per band over the wave (the popcount is the count; the lowest set lane is the lowest row, rows
//   ascend with the lane); the four waves' words of BD_QRUN queries meet in LDS and one thread per (query, band) adds the
//   workgroup's total with integer atomics.  No floating-point atomics: the totals do not depend on the launch geometry.
#pragma once
#include <math.h>

#include "csr_walk.h"

namespace sss {

constexpr int BD_QRUN = 32;           // queries between two flushes: 256 threads = 32 queries x 8 bands
constexpr int BD_MAX_EDGES = 7;
constexpr int BD_BANDS = BD_MAX_EDGES + 1;
static_assert(CSR_ROWS == BD_QRUN * BD_BANDS, "the flush maps one thread to one (query, band)");

struct BandEdges { double e[BD_MAX_EDGES]; };   // unused edges are +inf: no score reaches them

// (rows of the band in the wave) << 8 | its lowest lane; 0: none.  One per workgroup, in LDS.
using BandWords = int[CSR_ROWS / 64][BD_QRUN][BD_BANDS];

// band_ballot: the band of the thread's score (the number of edges it reaches, a float64 >=), one ballot per band over the
// wave, lane b keeping band b's word in the run's slot.  `live`: the thread's row exists.
__device__ __forceinline__ void band_ballot(BandWords& s_tot, int slot, bool live, double s, const BandEdges& E, int nb) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int band = 0;
#pragma unroll
    for (int e = 0; e < BD_MAX_EDGES; ++e) band += s >= E.e[e] ? 1 : 0;
    int mine = 0;                                                // lane b: band b's word for this wave
    for (int b = 0; b < nb; ++b) {
        const unsigned long long m = __builtin_amdgcn_ballot_w64(live && band == b);
        if (lane == b && m) mine = (__builtin_popcountll(m) << 8) | __builtin_ctzll(m);
    }
    if (lane < BD_BANDS) s_tot[wv][slot][lane] = mine;
}

// band_flush: the run's words of the four waves meet; one thread per (query, band) adds the workgroup's total to global
// memory.  row0: the workgroup's first row.  counts / first_out: [nq][nb] with nb = edges + 1, zeroed / set to all ones
// (int64 -1 = the largest unsigned value, so an unsigned atomicMin of row + id_offset >= 0 leaves -1 exactly where a band has
// no row) by the entry point.
__device__ __forceinline__ void band_flush(BandWords& s_tot, int f0, int fe, int nb, long row0, long id_offset,
                                           unsigned long long* __restrict__ counts, unsigned long long* __restrict__ first_out) {
    const int tid = threadIdx.x;
    __syncthreads();
    const int q = tid >> 3, b = tid & 7;                         // one thread per (query, band)
    if (f0 + q < fe && b < nb) {
        int cnt = 0, lo = -1;
        for (int w = 0; w < CSR_ROWS / 64; ++w) {                // waves ascend with the rows: the first hit is the lowest
            const int t = s_tot[w][q][b];
            if (t) {
                cnt += t >> 8;
                if (lo < 0) lo = w * 64 + (t & 255);
            }
        }
        if (cnt) {
            const size_t at = (size_t)(f0 + q) * nb + b;
            atomicAdd(&counts[at], (unsigned long long)cnt);
            atomicMin(&first_out[at], (unsigned long long)(row0 + lo + id_offset));
        }
    }
    __syncthreads();
}

// THE BAND FRAME: the band counts and first rows of the workgroup's rows and queries under Kind::pair, the queries in runs
// of BD_QRUN (workgroup-uniform bounds: band_flush's barriers are met by all).  grid: csr_grid's.
template <class Kind>
__device__ __forceinline__ void csr_bands(const CsrSets& Q, int nq, int q_per, const CsrSets& C, long n, const BandEdges& E, int nb,
                                          long id_offset, unsigned long long* __restrict__ counts,
                                          unsigned long long* __restrict__ first_out) {
    __shared__ int cols[CSR_LDS_WORDS];
    __shared__ BandWords s_tot;
    const long row0 = (long)blockIdx.x * CSR_ROWS, row = row0 + threadIdx.x;
    const auto R = csr_stage<Kind>(cols, C, row, n);
    const auto state = Kind::row_state(R);
    int f_lo;
    const int f_hi = csr_query_range(nq, q_per, &f_lo);
    for (int f0 = f_lo; f0 < f_hi; f0 += BD_QRUN) {
        const int fe = f0 + BD_QRUN < f_hi ? f0 + BD_QRUN : f_hi;
        R.each_space([&](auto V) {
            for (int f = f0; f < fe; ++f) {
                const long q0 = Q.ptr[f];
                band_ballot(s_tot, f - f0, row < n, Kind::pair(Q, q0, csr_len(q0, Q.ptr[f + 1]), V, state), E, nb);
            }
        });
        band_flush(s_tot, f0, fe, nb, row0, id_offset, counts, first_out);
    }
}

// ------------------------------------------------------------------------------ host (defined in jaccard.hip)
// A kind's band kernel: (qptr, qitems, qw, nq, q_per, cptr, citems, cw, n, E, nb, id_offset, counts, first), on csr_grid's grid.
using BandKernel = void (*)(const long*, const int*, const float*, int, int, const long*, const int*, const float*, long, BandEdges, int,
                            long, unsigned long long*, unsigned long long*);
// A *_bands entry point: csr_args_ok, the band arguments (1..7 finite ascending edges, no null pointer, an id_offset that
// leaves -1 free), counts / first initialised on the stream, the launch of `kernel` (`name`) and its status.  Messages start
// with `what`.
int band_counts(const char* what, const char* name, BandKernel kernel, const CsrSets& Q, long nq, const CsrSets& C, long n, bool weighted,
                const double* edges, int n_edges, long id_offset, int64_t* counts, int64_t* first, hipStream_t st);

}  // namespace sss
