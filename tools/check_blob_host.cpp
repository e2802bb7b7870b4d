// Host-only check of vtts::check_blob (viettts_amd/csrc/vtts_internal.h) under the address and undefined-behaviour sanitizers.  It links
// nothing of the HIP runtime (upload_blob is inline and not called) and needs no GPU:
//
//   clang++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/check_blob_host.cpp -o /tmp/check_blob_host && /tmp/check_blob_host
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../viettts_amd/csrc/vtts_internal.h"

static char g_msg[512];

namespace vtts {
int failf(int code, const char* fmt, ...) {  // engine.hip's, without its thread-local store
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace vtts

static int failures = 0;
static void expect(const char* what, int got, int want, const char* needle) {
    const bool ok = got == want && (!needle || strstr(g_msg, needle));
    printf("%-28s -> %d%s%s%s  %s\n", what, got, got ? " \"" : "", got ? g_msg : "", got ? "\"" : "", ok ? "ok" : "WRONG");
    failures += !ok;
}

int main() {
    using vtts::check_blob;
    const size_t need = 4096;
    void* const aligned = reinterpret_cast<void*>(uintptr_t(1) << 20);  // never dereferenced
    expect("NULL", check_blob(nullptr, need, need), VTTS_ERR_INVALID, "null");
    expect("need - 4 bytes", check_blob(aligned, need - 4, need), VTTS_ERR_NOMEM, "too small");
    expect("zero bytes", check_blob(aligned, 0, need), VTTS_ERR_NOMEM, "too small");
    expect("aligned to 64 only", check_blob(reinterpret_cast<void*>((uintptr_t(1) << 20) | 64), need, need), VTTS_ERR_INVALID, "aligned");
    expect("aligned to 1 only", check_blob(reinterpret_cast<void*>((uintptr_t(1) << 20) | 1), need, need), VTTS_ERR_INVALID, "aligned");
    expect("short AND misaligned", check_blob(reinterpret_cast<void*>(uintptr_t(260)), need - 4, need), VTTS_ERR_NOMEM, "too small");
    expect("exactly need", check_blob(aligned, need, need), VTTS_OK, nullptr);
    expect("need + 256", check_blob(aligned, need + 256, need), VTTS_OK, nullptr);
    expect("SIZE_MAX bytes", check_blob(aligned, ~size_t(0), need), VTTS_OK, nullptr);
    expect("top of the address space", check_blob(reinterpret_cast<void*>(~uintptr_t(0) & ~uintptr_t(255)), need, need), VTTS_OK, nullptr);
    expect("need of zero", check_blob(aligned, 0, 0), VTTS_OK, nullptr);
    return failures ? 1 : 0;
}
