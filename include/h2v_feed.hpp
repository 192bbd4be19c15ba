// h2v_feed.hpp — C++ mirror of include/h2v_feed.h: feed a launched staged batch to a resident accumulator without a host wait.
//
// feed_batch is h2v_accumulator_process_batch ENQUEUED: the groups of the batch's last launch become legs of the accumulator on the
// device, behind the launch; the call waits for nothing, and the batch may be uploaded again at once.  settle waits for the
// accumulator's stream once, commits counters and journal entries of every feed since, and returns a Report per feed since the last
// settle.  feed_batch(b); settle equals process_batch(b) after a host finish of the same launch, bit for bit.  Every other
// h2v_accumulator_* call settles first and leaves the reports queued.  h2v_feed.h has the ordering, the lifetimes and the
// soundness argument.  Errors are thrown as halo2_verifier::Failure, as h2v.hpp throws them.
#pragma once
#include <cstddef>
#include <vector>
#include "h2v.hpp"
#include "h2v_feed.h"

namespace halo2_verifier {   // (h2v.hpp's alias: h2v::feed::settle)
namespace feed {

// rc: 0, or H2V_ERR_BAD_ARGUMENT for a feed the device dropped (a draw >= r in a tail uploaded from device memory: the points keep
// their value, no journal entry appears, n_failed == n_proofs)
struct Report { int rc = 0; size_t n_proofs = 0, n_failed = 0; };
struct Pending { size_t unsettled = 0, unreported = 0; };

// enqueue only: no synchronise, no copy
inline void feed_batch(h2v_accumulator* a, h2v_batch* b) { check(h2v_accumulator_feed_batch(a, b)); }

// host state only
inline Pending pending(const h2v_accumulator* a) {
    Pending p;
    check(h2v_accumulator_pending(a, &p.unsettled, &p.unreported));
    return p;
}

// waits for the accumulator's stream; the reports of every feed since the last settle, in feed order
inline std::vector<Report> settle(h2v_accumulator* a) {
    size_t n = 0;
    check(h2v_accumulator_settle(a, 0, &n, nullptr, nullptr, nullptr));
    std::vector<int> rc(n ? n : 1);
    std::vector<size_t> proofs(n ? n : 1), failed(n ? n : 1);
    check(h2v_accumulator_settle(a, n, &n, rc.data(), proofs.data(), failed.data()));
    std::vector<Report> out(n);
    for (size_t i = 0; i < n; ++i) { out[i].rc = rc[i]; out[i].n_proofs = proofs[i]; out[i].n_failed = failed[i]; }
    return out;
}

}  // namespace feed
}  // namespace halo2_verifier
