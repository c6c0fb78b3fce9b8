// The L2 instantiations of the candidate scan (scan_kernel.h: k_scan<..., MET = 1>): float32 rows scanned as they are
// (DT_F32) or through their bf16 hi|lo (DT_SPLIT) or scaled float16 (DT_F16) image, scan keys q.c - |c|^2 / 2.  A
// translation unit of its own, so these kernels compile beside the inner-product ones of scan.hip.  gfx950 only.
#include "scan_kernel.h"

namespace sss {

int launch_scan_l2(int dtype, int d, int tile_rows, const ScanArgs& a, hipStream_t st) {
    const int rb = d * elem_bytes(dtype);
    int rc = 1;                                                  // (1: nothing launched)
    if (dtype == DT_F32) rc = launch_shape<DT_F32, 1>(rb, tile_rows, a, st);
    else if (dtype == DT_SPLIT) rc = launch_shape<DT_SPLIT, 1>(rb, tile_rows, a, st);
    else if (dtype == DT_F16) rc = launch_shape<DT_F16, 1>(rb, tile_rows, a, st);
    if (rc != 1) return rc;
    set_error("scan: no L2 scan of type %d for rows of %d bytes", dtype, rb);
    return SSS_EINVAL;
}

}  // namespace sss
