// What the two HeteroGGNN translation units share: gnn.hip (the per-op path) and gnn_fused.hip (the fused <= 256-wide path).
#pragma once
#include "lane_group.h"

namespace sss {

__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + expf(-v)); }

// The launch of k_segment_pool (defined, and instantiated, in gnn.hip alone): sss_segment_pool, and the rows wider than
// 256 floats of sss_pool_attention in gnn_fused.hip.  Arguments already checked, n_graphs > 0.
int launch_segment_pool(const float* node, long ld_node, const int* pptr, const int* qptr, long n_clicks, long n_graphs, int d,
                        const float* a, long ld_a, const float* bcoarse, long ld_b, const float* watt, float* out, long ld_out,
                        int reduce_sum, hipStream_t st);

}  // namespace sss
