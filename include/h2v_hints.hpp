// h2v_hints.hpp — C++ mirror of include/h2v_hints.h: point hints for a staged batch.
//
// A hint is the claimed y coordinate of a compressed G1 point of a proof, 32 canonical little-endian bytes; a hint row holds the y of
// the Np points of one proof in byte order (point_offsets).  A staged batch (h2v_batch) that is given the hints of its upload checks
// each one (two squarings, a product, a comparison) instead of taking a square root, and takes the root where a hint does not hold:
// the results of a launch depend on the proofs, instances and draws only, and the hints change its time and nothing else
// (h2v_hints.h has the definition).  Errors are thrown as halo2_verifier::Failure, as h2v.hpp throws them.  A batch is used from one
// thread at a time.
#pragma once
#include <cstdint>
#include <vector>
#include "h2v.hpp"
#include "h2v_hints.h"

namespace halo2_verifier {   // (h2v.hpp's alias: h2v::hints::set)
namespace hints {

// the byte offsets of the Np compressed points inside a proof of the context's key, ascending
inline std::vector<size_t> point_offsets(const h2v_ctx* ctx) {
    size_t n = 0;
    check(h2v_hints_point_offsets(ctx, nullptr, 0, &n));
    std::vector<size_t> off(n);
    check(h2v_hints_point_offsets(ctx, off.data(), off.size(), &n));
    return off;
}

// host only, no device: the canonical y of k compressed points (32 zero bytes where G1Affine::from_bytes fails); decoded, if given,
// gets one byte per point
inline Bytes from_points(const Bytes& points32, std::vector<uint8_t>* decoded = nullptr) {
    if (points32.size() % 32) throw Failure(H2V_ERR_BAD_ARGUMENT, "hints::from_points: not a whole number of 32-byte points");
    const size_t k = points32.size() / 32;
    Bytes y(32 * k);
    if (decoded) decoded->assign(k, 0);
    check(h2v_hints_from_points(points32.data(), k, y.data(), decoded ? decoded->data() : nullptr));
    return y;
}

// the hint rows of n proofs of proof_len bytes each, their points at `offsets` -> n x offsets.size() x 32 bytes
inline Bytes for_proofs(const std::vector<size_t>& offsets, const Bytes& proofs_flat, size_t proof_len) {
    if (!proof_len || proofs_flat.size() % proof_len) throw Failure(H2V_ERR_BAD_ARGUMENT, "hints::for_proofs: not a whole number of proofs");
    const size_t n = proofs_flat.size() / proof_len;
    Bytes points;
    points.reserve(32 * n * offsets.size());
    for (size_t i = 0; i < n; ++i)
        for (size_t o : offsets) {
            if (o + 32 > proof_len) throw Failure(H2V_ERR_BAD_ARGUMENT, "hints::for_proofs: a point offset outside the proof");
            points.insert(points.end(), proofs_flat.begin() + i * proof_len + o, proofs_flat.begin() + i * proof_len + o + 32);
        }
    return from_points(points);
}

// the hints of the batch's current upload of n proofs, from host memory (n x Np x 32 bytes); drop: none
inline void set(h2v_batch* b, size_t n, const Bytes& y32) { check(h2v_batch_set_hints(b, n, y32.data())); }
inline void drop(h2v_batch* b, size_t n) { check(h2v_batch_set_hints(b, n, nullptr)); }
// from device memory: row i at d_y32 + i * row_stride; device -> device on the batch's stream, no host wait
inline void set_device(h2v_batch* b, size_t n, const void* d_y32, size_t row_stride) {
    if (reinterpret_cast<uintptr_t>(d_y32) % 16 || row_stride % 16) throw Failure(H2V_ERR_BAD_ARGUMENT, "hints::set_device: a device pointer or a stride off a 16-byte boundary");
    check(h2v_batch_set_hints_device(b, n, d_y32, row_stride));
}

// the canonical y of the points of proofs [first, first + count) of the last launch (zeros for a point that did not decode):
// n_points is Np of the batch's key (point_offsets(ctx).size()); waits for the batch's stream
inline Bytes of_launch(h2v_batch* b, size_t first, size_t count, size_t n_points) {
    Bytes y(32 * count * n_points);
    Bytes none(1);
    check(h2v_batch_hints(b, first, count, y.empty() ? none.data() : y.data()));
    return y;
}
// the same into device memory by one kernel on the batch's stream; waits for nothing
inline void of_launch_device(h2v_batch* b, size_t first, size_t count, void* d_y32, size_t row_stride) {
    if (reinterpret_cast<uintptr_t>(d_y32) % 16 || row_stride % 16) throw Failure(H2V_ERR_BAD_ARGUMENT, "hints::of_launch_device: a device pointer or a stride off a 16-byte boundary");
    check(h2v_batch_hints_device(b, first, count, d_y32, row_stride));
}

// of the last launch: n x Np; the same when the launch had hints, else 0; the hints that were not used
struct Stats { size_t points = 0, hinted = 0, missed = 0; };
inline Stats stats(h2v_batch* b) {
    Stats s;
    check(h2v_batch_hint_stats(b, &s.points, &s.hinted, &s.missed));
    return s;
}

}  // namespace hints
}  // namespace halo2_verifier
