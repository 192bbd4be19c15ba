// What the stand-in libraries (tests/cpp/h2v_stub*.cpp) share: the FNV-1a hash they print of every input array, read with the length
// the call itself passes, and the "name=length:hash" form of it.  tests/caller_harness.py's fnv() makes the same words.
#pragma once
#include <cinttypes>
#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace h2v_stub {
inline uint64_t fnv(const void* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { h ^= ((const uint8_t*)p)[i]; h *= 1099511628211ull; }
    return h;
}
inline void bytes(const char* name, const void* p, size_t n) {
    if (!p) printf(" %s=null", name); else printf(" %s=%zu:%016" PRIx64, name, n, fnv(p, n));
}
}  // namespace h2v_stub
