// h2v_hints.hpp — C++ mirror of include/h2v_hints.h and include/h2v_hint_rows.h: point hints for a staged batch, and a hint row per
// proof (or none) for a staged batch, the one-shot calls and the resident accumulator.
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
#include "h2v_hint_rows.h"

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

// ---- a row per proof, or none (include/h2v_hint_rows.h).  A row is a proof's Np x 32 bytes (for_proofs of that one proof, Np of ITS
// key); an EMPTY Bytes stands for "this sender gave none".  The results are those of the calls without hints; only the time differs.
namespace detail {
// the char* array the C ABI takes: null for an empty row; every other row must hold 32 x n_points[i] bytes
inline std::vector<const uint8_t*> row_pointers(const std::vector<const Bytes*>& rows, const std::vector<size_t>& n_points) {
    std::vector<const uint8_t*> out(rows.size() ? rows.size() : 1, nullptr);
    for (size_t i = 0; i < rows.size(); ++i) {
        if (rows[i]->empty()) continue;
        if (rows[i]->size() != 32 * n_points[i]) throw Failure(H2V_ERR_BAD_ARGUMENT, "a hint row holds 32 bytes per point of its proof's key");
        out[i] = rows[i]->data();
    }
    return out;
}
inline size_t points_of(h2v_ctx* ctx) {
    size_t np = 0;
    check(h2v_ctx_proof_shape(ctx, nullptr, &np, nullptr, nullptr, nullptr));
    return np;
}
}  // namespace detail

// the hints of the batch's current upload from one row per proof (empty: none); n_points: Np of the batch's key
inline void set_rows(h2v_batch* b, const std::vector<Bytes>& rows, size_t n_points) {
    std::vector<const Bytes*> r;
    for (const Bytes& row : rows) r.push_back(&row);
    const std::vector<const uint8_t*> p = detail::row_pointers(r, std::vector<size_t>(rows.size(), n_points));
    check(h2v_batch_set_hint_rows(b, rows.size(), p.data()));
}

// h2v_verify_batch_keys_hinted: proofs of contexts[key] in call order, each with its row; rand32: one 32-byte draw per proof, or empty = OS RNG
struct Item { uint32_t key; Instances instances; Bytes proof; Bytes row; };
struct Result { bool ok = false; std::vector<int> statuses; Bytes left, right; Stats stats; };
namespace detail {
struct HintedCall {
    halo2_verifier::detail::Marshalled m;
    std::vector<const uint8_t*> rows;
    size_t stats[3] = {0, 0, 0};
    HintedCall(const std::vector<const Context*>& contexts, const std::vector<Item>& items, const Bytes& rand32, bool one_key = false) : m(one_key) {
        if (contexts.empty()) throw Failure(H2V_ERR_BAD_ARGUMENT, "at least one context");
        if (!rand32.empty() && rand32.size() != 32 * items.size()) throw Failure(H2V_ERR_BAD_ARGUMENT, "one 32-byte draw per proof");
        std::vector<size_t> np_of_key, np;
        for (const Context* c : contexts) { m.add_key(c->handle()); np_of_key.push_back(points_of(c->handle())); }
        std::vector<const Bytes*> r;
        for (const Item& it : items) { m.add(it.key, it.instances, it.proof); r.push_back(&it.row); np.push_back(np_of_key[it.key]); }
        rows = row_pointers(r, np);
    }
    Stats counted() const { Stats s; s.points = stats[0]; s.hinted = stats[1]; s.missed = stats[2]; return s; }
};
}  // namespace detail
inline Result verify_batch_keys(const std::vector<const Context*>& contexts, const std::vector<Item>& items, const Bytes& rand32 = Bytes()) {
    detail::HintedCall c(contexts, items, rand32);
    const size_t n = items.size();
    Result out;
    out.statuses.assign(n ? n : 1, 0); out.left.assign(64, 0); out.right.assign(64, 0);
    int ok = 0;
    check(h2v_verify_batch_keys_hinted(c.m.ctxs.data(), c.m.ctxs.size(), c.m.keys.data(), n, c.m.proofs.data(), c.m.lens.data(), c.rows.data(), c.m.insts.data(),
                                       c.m.ncols.data(), c.m.col_lens.data(), rand32.empty() ? nullptr : rand32.data(), out.statuses.data(), &ok, out.left.data(),
                                       out.right.data(), c.stats));
    out.ok = ok != 0; out.statuses.resize(n); out.stats = c.counted();
    return out;
}
// h2v_verify_batches_hinted: halo2_verifier::verify_batches with a row per proof (Item::key is 0); one instance shape per call
inline std::vector<Result> verify_batches(const Context& ctx, const std::vector<std::vector<Item>>& batches, const Bytes& rand32 = Bytes(), Stats* stats = nullptr) {
    std::vector<Item> all;
    std::vector<size_t> sizes;
    for (const auto& batch : batches) {
        if (batch.empty()) throw Failure(H2V_ERR_BAD_ARGUMENT, "a batch of no proofs");
        sizes.push_back(batch.size());
        all.insert(all.end(), batch.begin(), batch.end());
    }
    detail::HintedCall c({&ctx}, all, rand32, true);
    if (!c.m.uniform) throw Failure(H2V_ERR_BAD_ARGUMENT, "verify_batches takes one instance shape per call");
    const size_t n = all.size(), k = sizes.size();
    std::vector<int> st(n ? n : 1, 0), ok(k ? k : 1, 0);
    Bytes left(64 * (k ? k : 1), 0), right(64 * (k ? k : 1), 0);
    sizes.resize(k ? k : 1, 0);
    check(h2v_verify_batches_hinted(ctx.handle(), k, sizes.data(), c.m.proofs.data(), c.m.lens.data(), c.rows.data(), c.m.insts.data(), c.m.ncols[0], c.m.shape0(),
                                    rand32.empty() ? nullptr : rand32.data(), st.data(), ok.data(), left.data(), right.data(), c.stats));
    if (stats) *stats = c.counted();
    std::vector<Result> out(k);
    for (size_t g = 0, at = 0; g < k; at += sizes[g], ++g) {
        out[g].ok = ok[g] != 0;
        out[g].statuses.assign(st.begin() + at, st.begin() + at + sizes[g]);
        out[g].left.assign(left.begin() + 64 * g, left.begin() + 64 * g + 64);
        out[g].right.assign(right.begin() + 64 * g, right.begin() + 64 * g + 64);
    }
    return out;
}
// h2v_accumulator_process_hinted: Accumulator::process with a row per proof -> the statuses of this call's proofs; all_ok, if given, says
// whether all are 0 (the object's own all_ok() is not updated by this free function)
inline std::vector<int> process(Accumulator& acc, const std::vector<const Context*>& contexts, const std::vector<Item>& items, const Bytes& rand32 = Bytes(),
                                Stats* stats = nullptr, bool* all_ok = nullptr) {
    detail::HintedCall c(contexts, items, rand32);
    const size_t n = items.size();
    std::vector<int> st(n ? n : 1, 0);
    int ok = 0;
    check(h2v_accumulator_process_hinted(acc.handle(), c.m.ctxs.data(), c.m.ctxs.size(), c.m.keys.data(), n, c.m.proofs.data(), c.m.lens.data(), c.rows.data(),
                                         c.m.insts.data(), c.m.ncols.data(), c.m.col_lens.data(), rand32.empty() ? nullptr : rand32.data(), st.data(), &ok, c.stats));
    if (stats) *stats = c.counted();
    if (all_ok) *all_ok = ok != 0;
    st.resize(n);
    return st;
}

}  // namespace hints
}  // namespace halo2_verifier
