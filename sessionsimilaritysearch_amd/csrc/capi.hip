// Error plumbing of libsss and its two host-only queries.  Every other entry point of the C ABI (include/*.h, seen by
// every translation unit through sss_common.h) is defined, extern "C", in the translation unit that implements it.
#include <stdarg.h>
#include <stdio.h>

#include <mutex>
#include <set>
#include <utility>

#include "sss_common.h"

namespace sss {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return SSS_EHIP;
    }
    return SSS_OK;
}

int opt_in_lds(const void* kernel, const char* name, size_t bytes) {
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;          // (kernel, device) pairs opted in
    const std::pair<const void*, int> key(kernel, current_device());
    std::lock_guard<std::mutex> lock(mu);
    if (done.count(key)) return SSS_OK;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: opting in to %zu bytes of LDS failed: %s", name, bytes, hipGetErrorString(e));
        return SSS_EHIP;
    }
    done.insert(key);
    return SSS_OK;
}

}  // namespace sss

extern "C" int sss_version(void) { return 250; }
extern "C" const char* sss_last_error(void) { return sss::g_err; }
