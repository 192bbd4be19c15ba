// h2v_draws.hpp — C++ mirror of include/h2v_draws.h: the draws of a 32-byte seed, on the host and into device memory.
//
//   draw(seed, i) = LE512(BLAKE2b-512(seed | LE64(i), digest 64, no key, personal "h2v-draws-v1")) mod r, 32 canonical bytes
//
// The seed comes from the OS RNG, is chosen independently of the proofs and is not revealed to provers before the verdict
// (h2v_draws.h has the contract).  Both calls are context-free and may be made from any number of threads.  Errors are thrown as
// halo2_verifier::Failure, as h2v.hpp throws them.
#pragma once
#include <array>
#include <cstdint>
#include <vector>
#include "h2v.hpp"
#include "h2v_draws.h"

namespace halo2_verifier {   // (h2v.hpp's alias: h2v::draws::expand)
namespace draws {

typedef std::array<uint8_t, 32> Seed;

// a seed for C++ callers: a canonical scalar from the library's OS generator (h2v_random_scalars)
inline Seed new_seed() {
    Seed s;
    check(h2v_random_scalars(s.data(), 1));
    return s;
}

// draw(seed, first) | .. | draw(seed, first + n - 1): n * 32 bytes, on the host
inline std::vector<uint8_t> expand(const Seed& seed, uint64_t first, size_t n) {
    std::vector<uint8_t> out(32 * n);
    check(h2v_draws_expand(seed.data(), first, n, out.data()));
    return out;
}

// the same values into 32 * n bytes of device memory at d_out32 (16-byte aligned), by a kernel enqueued on `stream` (a hipStream_t) of
// `device`; waits for nothing.  n <= H2V_DRAWS_DEVICE_MAX per call
inline void expand_device(int device, void* stream, const Seed& seed, uint64_t first, size_t n, void* d_out32) {
    check(h2v_draws_expand_device(device, stream, seed.data(), first, n, d_out32));
}

// The tail of a shard that starts at proof `lo` of `total` per group, group-major, into device memory: the whole stream is
// expand(seed, 0, groups * total), group g owns indices [g * total, (g + 1) * total).  d_out32 holds groups * (total - lo) draws.
inline void seeded_tail_device(int device, void* stream, const Seed& seed, size_t lo, size_t total, size_t groups, void* d_out32) {
    if (lo > total) throw Failure(H2V_ERR_BAD_ARGUMENT, "a shard starts inside its batch");
    const size_t per = total - lo;
    for (size_t g = 0; g < groups && per; ++g)
        expand_device(device, stream, seed, (uint64_t)(g * total + lo), per, static_cast<uint8_t*>(d_out32) + 32 * g * per);
}

}  // namespace draws
}  // namespace halo2_verifier
