// h2v_guards.hpp — C++ mirror of include/h2v_guards.h: every proof's Guard out of a launched staged batch.
//
// A staged batch (h2v_batch) runs verify_proof for all its proofs in one launch and leaves their terms resident; one kernel gathers
// any range [first, first + count) of them: term t of proof first + j at index j * T + t of a channel, T = T_L or T_R of shape().
// A scalar is the Guard's own times the product of the draws behind the proof inside its group; a proof with a status has zero
// scalars under all-zero bases; under GWC a commitment opened at several points occurs once with its scalars summed (h2v_guards.h has
// the definition).  The batch must be launched or finished, and its stage and results do not change.  Errors are thrown as
// halo2_verifier::Failure, as h2v.hpp throws them.  A batch is used from one thread at a time.
#pragma once
#include <cstdint>
#include <vector>
#include "h2v.hpp"
#include "h2v_guards.h"

namespace halo2_verifier {   // (h2v.hpp's alias: h2v::guards::to_host)
namespace guards {

struct Shape { size_t left_terms = 0, right_terms = 0; };
// the term counts of a proof's two channels under the plan of the batch's upload
inline Shape shape(const h2v_batch* b) {
    Shape s;
    check(h2v_batch_guard_shape(b, &s.left_terms, &s.right_terms));
    return s;
}

// The outputs of to_device, null = not wanted; each 16-byte aligned device memory of the batch's device
struct DeviceGuards {
    void* left_scalars = nullptr;    // 32 * count * T_L bytes
    void* left_bases = nullptr;      // 64 * count * T_L bytes
    void* right_scalars = nullptr;   // 32 * count * T_R bytes
    void* right_bases = nullptr;     // 64 * count * T_R bytes
    void* mult = nullptr;            // 32 * count bytes
    void* status = nullptr;          // count int32
};
// by kernels on the batch's stream; waits for nothing
inline void to_device(h2v_batch* b, size_t first, size_t count, const DeviceGuards& out) {
    for (const void* p : {out.left_scalars, out.left_bases, out.right_scalars, out.right_bases, out.mult, out.status})
        if (reinterpret_cast<uintptr_t>(p) % 16) throw Failure(H2V_ERR_BAD_ARGUMENT, "guards::to_device: a device pointer off a 16-byte boundary");
    check(h2v_batch_guards_device(b, first, count, out.left_scalars, out.left_bases, out.right_scalars, out.right_bases, out.mult, out.status));
}

// The Guards of a range on the host: the four term arrays of h2v.hpp's Guard for the whole range (proof after proof), the proofs'
// multipliers (32 bytes each) and statuses
struct HostGuards { Shape shape; size_t first = 0, count = 0; Guard terms; Bytes mult; std::vector<int> status; };
// one kernel per channel, one copy, one synchronise of the batch's stream
inline HostGuards to_host(h2v_batch* b, size_t first, size_t count) {
    HostGuards g;
    g.shape = shape(b);
    g.first = first; g.count = count;
    g.terms.left_scalars.resize(32 * count * g.shape.left_terms); g.terms.left_bases.resize(64 * count * g.shape.left_terms);
    g.terms.right_scalars.resize(32 * count * g.shape.right_terms); g.terms.right_bases.resize(64 * count * g.shape.right_terms);
    g.mult.resize(32 * count); g.status.resize(count);
    check(h2v_batch_guards(b, first, count, g.terms.left_scalars.data(), g.terms.left_bases.data(), g.terms.right_scalars.data(), g.terms.right_bases.data(),
                           g.mult.data(), g.status.data()));
    return g;
}
// proof first + j of a HostGuards as a Guard of its own
inline Guard guard_of(const HostGuards& g, size_t j) {
    if (j >= g.count) throw Failure(H2V_ERR_BAD_ARGUMENT, "guards::guard_of: a proof outside the range");
    const size_t tl = g.shape.left_terms, tr = g.shape.right_terms;
    auto cut = [](const Bytes& v, size_t lo, size_t n) { return Bytes(v.begin() + lo, v.begin() + lo + n); };
    return Guard{cut(g.terms.left_scalars, 32 * j * tl, 32 * tl), cut(g.terms.left_bases, 64 * j * tl, 64 * tl),
                 cut(g.terms.right_scalars, 32 * j * tr, 32 * tr), cut(g.terms.right_bases, 64 * j * tr, 64 * tr)};
}

// The range's left terms behind the end of `left`, its right terms behind the end of `right` (either may be null), in the objects' own
// form -> the proofs of the range with a non-zero status.  A Failure leaves both objects as they were.
inline size_t append(h2v_batch* b, size_t first, size_t count, Msm* left, Msm* right) {
    size_t failed = 0;
    check(h2v_batch_guards_append(b, first, count, left ? left->handle() : nullptr, right ? right->handle() : nullptr, &failed));
    return failed;
}

}  // namespace guards
}  // namespace halo2_verifier
