// sss_topk_merge of the C ABI (include/sss.h; gfx950): k-way merge of per-shard results (after the RCCL all-gather):
// [shards][nq][k] -> [nq][k] by (score desc, id asc); ids < 0 are padding.  One thread per query (k*shards is tiny).
#include "scan.h"

namespace sss {

__global__ void k_topk_merge(const float* __restrict__ D_in, long d_stride, const long* __restrict__ I_in,
                             long i_stride, int shards, int nq, int k, float* __restrict__ D_out,
                             long* __restrict__ I_out) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    int pos[64];
    for (int s = 0; s < shards; ++s) pos[s] = 0;
    for (int o = 0; o < k; ++o) {
        int bs = -1; float bd = 0.f; long bi = 0;
        for (int s = 0; s < shards; ++s) {
            if (pos[s] >= k) continue;
            const size_t a = (size_t)q * k + pos[s];
            const long id = I_in[(size_t)s * i_stride + a];
            if (id < 0) { pos[s] = k; continue; }
            const float dd = D_in[(size_t)s * d_stride + a];
            if (bs < 0 || dd > bd || (dd == bd && id < bi)) { bs = s; bd = dd; bi = id; }
        }
        if (bs < 0) { D_out[(size_t)q * k + o] = -3.4028234663852886e38f; I_out[(size_t)q * k + o] = -1; }
        else { D_out[(size_t)q * k + o] = bd; I_out[(size_t)q * k + o] = bi; ++pos[bs]; }
    }
}

extern "C" int sss_topk_merge(const float* D_in, int64_t d_shard_stride, const int64_t* I_in, int64_t i_shard_stride, int shards,
                              int64_t nq, int k, float* D_out, int64_t* I_out, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (shards < 1 || shards > 64 || nq <= 0 || k <= 0 || d_shard_stride < nq * k || i_shard_stride < nq * k) {
        set_error("topk_merge: bad arguments");
        return SSS_EINVAL;
    }
    hipLaunchKernelGGL(k_topk_merge, dim3((unsigned)((nq + 127) / 128)), dim3(128), 0, st, D_in, d_shard_stride, I_in,
                       i_shard_stride, shards, (int)nq, k, D_out, I_out);
    return check_launch("k_topk_merge");
}

}  // namespace sss
