// Shared device/host helpers for libsss (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

// The whole C ABI: every entry point is DEFINED, extern "C", in the translation unit that implements it, and every
// translation unit sees every declaration -- a definition that differs from its header does not compile.
#include "../../include/sss.h"
#include "../../include/sss_eval.h"
#include "../../include/sss_graph.h"
#include "../../include/sss_l2.h"
#include "../../include/sss_l2_long.h"
#include "../../include/sss_pad.h"
#include "../../include/sss_sparse.h"

static_assert(std::is_same<int64_t, long>::value, "the kernels take the ABI's int64_t arrays as long");

#define SSS_OK 0
#define SSS_EINVAL (-1)
#define SSS_EWORKSPACE (-2)
#define SSS_EHIP (-3)

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace sss {

void set_error(const char* fmt, ...);
int check_launch(const char* what);
// Opt `kernel` in to `bytes` of dynamic LDS on the current device, once per (device, kernel); SSS_EHIP, with the HIP
// error cleared and a message naming `name` and the bytes, when the runtime refuses.
int opt_in_lds(const void* kernel, const char* name, size_t bytes);

// per-device host state is indexed by current_device() (defined in scan.hip)
constexpr int MAX_DEVICES = 64;
int current_device();

// workspace sections start on 256-byte boundaries
static inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

// float -> uint32 whose unsigned order equals the float order (-inf lowest, +inf highest).
__device__ __host__ __forceinline__ uint32_t f2ord(float f) {
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __host__ __forceinline__ float ord2f(uint32_t o) {
    uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    return __builtin_bit_cast(float, u);
}
// 64-bit selection key: larger key == better candidate == (higher score, then lower id).
// id -1 (empty slot) with score -inf gives the smallest key any slot can have; 0 is below all.
__device__ __host__ __forceinline__ uint64_t make_key(float s, int32_t id) {
    return ((uint64_t)f2ord(s) << 32) | (uint32_t)(~(uint32_t)id);
}
__device__ __host__ __forceinline__ float key_score(uint64_t k) { return ord2f((uint32_t)(k >> 32)); }
__device__ __host__ __forceinline__ int32_t key_id(uint64_t k) { return (int32_t)(~(uint32_t)k); }

// Exact GELU (torch's approximate='none', HF's "gelu"): k_hgt_aggregate's way out and act = 5 of k_linear_grouped.
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }

}  // namespace sss
