// The resident accumulator behind h2v_accumulator (include/h2v.h): an AccumulatorStrategy that lives across calls.
//
// The reference's AccumulatorStrategy is incremental: verify_proof takes a key and instances on every call and hands the strategy back
// (kzg/strategy.rs:125-136), finalize() runs the one pairing whenever the caller decides (:138-140), with(DualMSM) resumes an earlier
// accumulation (:76-78).  Here the strategy's DualMSM is two G1 points that stay in device memory.  A process call of n proofs with draws
// r_0 .. r_{n-1} is n x (scale by the draw, add the Guard):
//     (L, R) <- M (L, R) + sum_i (prod_{j > i} r_j) Guard_i,     M = r_0 r_1 .. r_{n-1}
// so process(A); process(B); finalize() equals one h2v_verify_batch_keys over A || B with the draws concatenated, for any cut.
//   - M (L, R) is k_accumulator_scale (msm.hip) on the accumulator's stream, enqueued first: it depends on the draws and the previous
//     accumulator only, and runs beside the groups' chains.  It writes a staging record, not the accumulator.
//   - the sum is the call's (key, shape) groups on their keys' scratch batches, each without a pairing, with the whole-sequence
//     multipliers (run_group_batches, oneshot.hip: what h2v_verify_batch_keys runs in front of its fold).
//   - one fold over [staging record, group records ..] writes the accumulator, as the last step: a call that fails before it leaves
//     the accumulator and the counters as they were.
// No pairing runs before finalize, and no accumulator point goes through host memory.
//
// The leg journal (h2v_accumulator_journal_begin; off by default, and then nothing below differs).  A proof that is wrong but decodes and
// passes its transcript poisons (L, R) with every status 0.  With the journal on, every successful call that changed the accumulator
// leaves an entry: its own sum (l, r) in a device slot of two points — one more fold over the call's group records WITHOUT the staging
// record — and on the host M and the call's counters.  Entry 0, the base, is the accumulator as it stood at journal_begin.  Invariant:
//     (L, R) = sum_e W_e sum_e,     W_e = prod_{f > e} M_f
//   - check_legs: one pairing_check_enqueue over the slots, a check per entry side by side.
//   - drop_legs: the host makes W_e of the kept entries, one k_accumulator_scale launch (an item per kept entry) writes W_e sum_e as
//     whole-point records, one fold over them writes the accumulator as the last step; the host's bookkeeping follows the synchronise.
// Entries never move in device memory: the host keeps entry -> slot and hands that map to the kernels, so a call that fails on the way
// leaves nothing half-moved.  A slot is written before its entry is visible (the commit rule of the accumulator, extended).
//
// Merging (h2v_accumulator_merge / _export_state / _merge_states): one pairing for K accumulators.  With draws c_1 .. c_K, none zero,
//     (L, R) <- (L, R) + sum_k c_k (L_k, R_k),     the counters += the sources'
// — per source DualMSM::scale then add_msm (poly/kzg/msm.rs:173-183) on a copy; dst is not scaled and the sources are not changed.  The
// sources' pairs reach a staging array of dst (device-to-device copies, or the lift of exported states from their bytes), one
// k_accumulator_scale launch of K workgroups writes c_k (L_k, R_k) as whole-point records, and one k_accumulator_merge_fold launch
// (util.hip) scatters them into the journal slots of K new entries (M = 1 each: the invariant holds as it stands) and writes the
// accumulator, as the last step.  Soundness: include/h2v.h.
//
// A finished staged batch as legs (h2v_accumulator_process_batch): process once per group of the batch, with the groups' sums S_g and
// the products M_g of their draws taken from what the launch left on the device:
//     (L, R) <- (prod_g M_g) (L, R) + sum_g W_g S_g,     W_g = prod_{f > g} M_f
// k_leg_weights (verify_kernels.hip) makes the scalars, one k_accumulator_scale launch of G + 1 items the records, k_accumulator_legs_fold
// (util.hip) the journal's G entries and the accumulator, as the last step.
//
// An enqueued feed (h2v_accumulator_feed_batch, include/h2v_feed.h): process_batch for a LAUNCHED batch, with no host wait.  The
// accumulator's stream waits for an event on the batch's stream; k_feed_gather and k_feed_weights read the batch into l_pairs / l_words
// and the batch's read event is recorded; k_accumulator_scale, k_accumulator_legs_fold and k_feed_report follow.  The host keeps a Feed
// per call: the journal slots it reserved at enqueue (out of free_slots, so that later calls cannot take them) and a pinned block
// with those slots for the fold and the report for h2v_accumulator_settle, which commits or releases them.  Every other entry point
// settles first (settle_feeds), so below this comment "idle" reads "idle, or holding only enqueued feeds".
#include "../../include/h2v.h"
#include "../../include/h2v_hint_rows.h"
#include "../../include/h2v_feed.h"
#include "batch.h"
#include "msm_object.h"
#include <string.h>
#include <algorithm>
#include <deque>
#include <functional>

using namespace h2v;

struct h2v_accumulator {
    h2v_ctx* ctx = nullptr;          // the params (same_srs for every context of a process call), the pairing tables, add_msm's MSMs
    hipStream_t stream = nullptr;    // its own, of the highest priority (h2v_accumulator_create); idle whenever a call returns, or holding only enqueued feeds
    DevBuf<G1J> acc;                 // [0] left, [1] right: whole Jacobian points
    DevBuf<uint8_t> records;         // [0] the staging record (the scaled accumulator), [1 ..] the records of a call's groups (at most H2V_MAX_SHAPES_PER_CALL)
    DevBuf<uint32_t> scalar;         // M of the call in flight, 8 canonical words
    DevBuf<uint32_t> words;          // [0] fold_failed, [1] the pairing's verdict, [2, 3] identity flags of the two points, [4, 5] add_msm's base flags, [6] an entry fold's fold_failed
    DevBuf<uint8_t> bytes;           // the affine bytes of the two points (read / finalize); add_msm: the evaluated channels on their way in
    DevBuf<G1A> affine;              // add_msm
    DevBuf<G1J> jacobian;            // add_msm
    uint32_t host_scalar[8] = {0};   // what `scalar` is copied from (it outlives the copy)
    size_t n_proofs = 0, n_failed = 0;
    // the leg journal
    struct Entry { uint32_t slot; Fr M; size_t n_proofs, n_failed; };
    size_t j_cap = 0;                // entries the journal holds, the base included; 0 = off
    std::vector<Entry> entries;      // [0] the base
    std::vector<uint32_t> free_slots;   // descending: the lowest free slot is taken first, so the slots in use stay at the front
    DevBuf<G1J> j_sums;              // [2 j_cap] slot s: the sum (l, r) of the entry that owns it
    DevBuf<uint8_t> j_records;       // [j_cap] drop_legs: W_e sum_e of the kept entries as whole-point records
    DevBuf<uint32_t> j_words;        // drop_legs: [8 K] W_e of the K kept entries, [K] their slots; check_legs: [9 j_cap ..] a verdict per slot
    std::vector<uint32_t> j_host;    // what j_words is copied from and to
    // merge / merge_states: the K sources of the call in flight
    DevBuf<G1J> m_pairs;             // [2 K] the sources' points, gathered (merge) or lifted from their bytes (merge_states)
    DevBuf<uint8_t> m_records;       // [K] c_k (L_k, R_k) as whole-point records
    DevBuf<uint32_t> m_words;        // [8 K] the draws, [K] the journal slots of the K new entries, [2 K] merge_states: the points' flags
    DevBuf<uint8_t> m_bytes;         // [128 K] merge_states: the states' affine bytes
    DevBuf<G1A> m_affine;            // [2 K] merge_states
    std::vector<uint32_t> m_host;    // what m_words is copied from and to
    // process_batch: the G legs of the call in flight (grow-only)
    DevBuf<G1J> l_pairs;             // [2 (G + 1)] the accumulator's pair, then the batch's G unscaled sums, gathered
    DevBuf<uint8_t> l_records;       // [G + 1] M (L, R), then W_g S_g, as whole-point records
    DevBuf<uint32_t> l_words;        // [8 (G + 1)] prod M_g and the W_g, [8 G] the M_g, [G] the journal slots of the G new entries
    MappedHostBuf l_legs;            // [32 G] the M_g as they come back (pinned: the copy is enqueued between the launches and must not hold the host)
    std::vector<uint32_t> l_host;    // [G] what the slots are copied from
    // enqueued feeds (h2v_accumulator_feed_batch): they share l_pairs, l_records and l_words, which stream order serialises — for a feed
    // l_words is [8 (G + 1)] the weights, [8 G] the M_g, [G] the groups' sizes, [G] their failed counts, [1] rc
    struct Feed {
        std::unique_ptr<MappedHostBuf> block;   // pinned, the feed's own until it is reported: [4 + 10 G] the report (k_feed_report), [G] the journal slots (the host's, read by the fold)
        uint32_t n = 0, G = 0;
        std::vector<uint32_t> slots;            // the journal slots reserved at enqueue (journal off: none)
        bool settled = false;
        int rc = 0; size_t failed = 0;          // of a settled feed
    };
    std::deque<Feed> feeds;          // the feeds not reported yet, in feed order: settled ones first
    size_t f_unsettled = 0;
    std::vector<std::unique_ptr<MappedHostBuf>> f_blocks;   // blocks of reported feeds, for the next ones
    std::vector<void*> f_retired;    // device arrays that grew under a pending feed: freed at settle (hipFree would wait for the device)
    hipEvent_t ev_batch = nullptr;   // recorded on a fed batch's stream; this stream waits for it
    // process_guards: staging buffers and an MSM workspace of its own (grow-only), so that accumulators that share a context do not meet
    GuardStage g_stage;              // the call's terms
    MsmWorkspace g_ws;               // the two pooled channels
    DevBuf<uint8_t> g_rand;          // [32 n] the draws
    DevBuf<Fr> g_mult, g_tiles;      // [n] the multipliers, and multipliers_enqueue's scratch
    DevBuf<G1J> g_sums;              // [2] the call's own sum: sum_i mult_i Guard_i, left and right
};

namespace {

void store_u32(uint8_t* p, uint32_t v) { for (int i = 0; i < 4; ++i) p[i] = (uint8_t)(v >> (8 * i)); }
int settle_feeds(h2v_accumulator* a, const char* who);
// every operation of the object ends here: its stream is idle when a call returns
int sync(h2v_accumulator* a, const char* who) {
    const hipError_t e = hipStreamSynchronize(a->stream);
    if (e != hipSuccess) { set_last_error(std::string(who) + ": " + hipGetErrorString(e)); return H2V_ERR_DEVICE; }
    return 0;
}

// the affine bytes of the two points into out_left / out_right (either may be null); with `ok`, the pairing check beside them
int read_points(h2v_accumulator* a, const char* who, int* ok, uint8_t* out_left, uint8_t* out_right) {
    H2V_HIP_CHECK(hipSetDevice(a->ctx->device));
    int rc;
    if ((rc = settle_feeds(a, who))) return rc;
    uint32_t okv = 0; uint8_t out[128];
    if (ok && (rc = pairing_check_enqueue(a->stream, a->ctx->pairing, a->acc.p, 1, a->words.p + 1))) return rc;
    if ((rc = point_to_bytes_enqueue(a->stream, a->acc.p, a->bytes.p, a->words.p + 2, 2))) return rc;
    if (ok) H2V_HIP_CHECK(hipMemcpyAsync(&okv, a->words.p + 1, 4, hipMemcpyDeviceToHost, a->stream));
    H2V_HIP_CHECK(hipMemcpyAsync(out, a->bytes.p, 128, hipMemcpyDeviceToHost, a->stream));
    if ((rc = sync(a, who))) return rc;
    if (ok) *ok = (okv && !a->n_failed) ? 1 : 0;
    if (out_left) memcpy(out_left, out, 64);
    if (out_right) memcpy(out_right, out + 64, 64);
    return 0;
}

// the slot the next entry will own, or (journal off) null; the caller has checked that the journal is not full
G1J* next_slot(h2v_accumulator* a) { return a->j_cap ? a->j_sums.p + 2 * (size_t)a->free_slots.back() : nullptr; }
bool journal_full(const h2v_accumulator* a) { return a->j_cap && a->entries.size() >= a->j_cap; }
// the entry of a call that has just succeeded becomes visible
constexpr uint32_t NEXT_FREE_SLOT = 0xffffffffu;
// (slot: one that an enqueued feed took out of free_slots when it was enqueued)
void commit_entry(h2v_accumulator* a, const Fr& M, size_t n_proofs, size_t n_failed, uint32_t slot = NEXT_FREE_SLOT) {
    if (!a->j_cap) return;
    if (slot != NEXT_FREE_SLOT) { a->entries.push_back({slot, M, n_proofs, n_failed}); return; }
    a->entries.push_back({a->free_slots.back(), M, n_proofs, n_failed});
    a->free_slots.pop_back();
}
// The host's half of every enqueued feed that has none yet, in feed order, behind one synchronise of the stream: a feed whose report
// says 0 commits its counters and one entry per group in the slots it reserved; a dropped feed (a draw >= r, found by k_feed_weights:
// the points kept their value) gives its slots back, leaves no entry and counts its n proofs as processed AND failed.  The reports stay
// queued for h2v_accumulator_settle.  What every entry point but feed_batch and pending begins with; nothing pending: no HIP call.
int settle_feeds(h2v_accumulator* a, const char* who) {
    if (!a->f_unsettled) return 0;
    hipSetDevice(a->ctx->device);
    const hipError_t e = hipStreamSynchronize(a->stream);
    if (e != hipSuccess) { set_last_error(std::string(who) + ": " + hipGetErrorString(e)); return H2V_ERR_DEVICE; }
    bool released = false;
    for (auto& f : a->feeds) {
        if (f.settled) continue;
        const volatile uint32_t* rep = reinterpret_cast<const volatile uint32_t*>(f.block->p);
        f.rc = (int)rep[0];
        if (f.rc == 0) {
            f.failed = rep[3];
            for (uint32_t g = 0; g < f.G && a->j_cap; ++g) {
                uint8_t m_bytes[32];
                for (int j = 0; j < 8; ++j) store_u32(m_bytes + 4 * j, rep[4 + 10 * (size_t)g + j]);
                Fr M;
                Fr::from_bytes(m_bytes, M);
                commit_entry(a, M, rep[4 + 10 * (size_t)g + 8], rep[4 + 10 * (size_t)g + 9], f.slots[g]);
            }
        } else {
            f.failed = f.n;
            for (uint32_t sl : f.slots) { a->free_slots.push_back(sl); released = true; }
        }
        a->n_proofs += f.n; a->n_failed += f.failed;
        f.slots.clear();
        f.settled = true;
    }
    if (released) std::sort(a->free_slots.begin(), a->free_slots.end(), std::greater<uint32_t>());
    a->f_unsettled = 0;
    for (void* p : a->f_retired) hipFree(p);
    a->f_retired.clear();
    return 0;
}
// a grow-only array of an accumulator with feeds in flight: the old allocation is kept until settle (a feed's kernels may still use it)
template <class T> int grow_under_feeds(h2v_accumulator* a, DevBuf<T>& buf, size_t count) {
    if (buf.p && count <= buf.cap) return 0;
    if (buf.p && a->f_unsettled) { a->f_retired.push_back(buf.p); buf.p = nullptr; buf.cap = 0; }
    return buf.alloc(count);
}
void journal_off(h2v_accumulator* a) { a->j_cap = 0; a->entries.clear(); a->free_slots.clear(); }

struct Drain { hipStream_t s; bool armed = true; ~Drain() { if (armed) hipStreamSynchronize(s); } };

// What h2v_accumulator_merge and h2v_accumulator_merge_states share in front of any device work: the draws (canonical, none zero; null = OS
// draws) and room in the journal for K entries.
int merge_args(h2v_accumulator* a, const char* who, size_t K, const uint8_t*& draws32, std::vector<uint8_t>& os_draws) {
    if (int rc = resolve_draws(draws32, K, os_draws, who, true)) return rc;
    if (a->j_cap && a->entries.size() + K > a->j_cap) { set_last_error(std::string(who) + ": the journal has fewer free entries than sources"); return H2V_ERR_UNSUPPORTED; }
    return 0;
}
int merge_reserve(h2v_accumulator* a, size_t K, bool states) {
    int rc;
    if ((rc = a->m_pairs.reserve(2 * K)) || (rc = a->m_records.reserve((size_t)H2V_ACC_RECORD_BYTES * K)) || (rc = a->m_words.reserve(11 * K))) return rc;
    if (states && ((rc = a->m_bytes.reserve(128 * K)) || (rc = a->m_affine.reserve(2 * K)))) return rc;
    a->m_host.resize(11 * K);
    return 0;
}
// The merge over K pairs already on the device (m_pairs, written by work enqueued on the accumulator's stream):
//     (L, R) <- (L, R) + sum_k c_k (L_k, R_k),   the counters += the sources', and with the journal on an entry per source, in call order,
//     whose sum is c_k (L_k, R_k) and whose M is 1 (so (L, R) = sum_e W_e sum_e holds as it stands).
// One k_accumulator_scale launch of K one-wave workgroups writes the K records; one k_accumulator_merge_fold launch scatters them into the
// journal slots and writes the accumulator, as the last step.  The counters and the entries follow the synchronise.
int merge_impl(h2v_accumulator* a, const char* who, size_t K, const uint8_t* draws32, const size_t* src_proofs, const size_t* src_failed, Drain& drain) {
    uint32_t* h = a->m_host.data();
    memcpy(h, draws32, 32 * K);
    for (size_t k = 0; k < K && a->j_cap; ++k) h[8 * K + k] = a->free_slots[a->free_slots.size() - 1 - k];   // the lowest free slots, in call order
    int rc;
    H2V_HIP_CHECK(hipMemcpyAsync(a->m_words.p, h, 4 * 9 * K, hipMemcpyHostToDevice, a->stream));
    if ((rc = accumulator_scale_many_enqueue(a->stream, a->m_pairs.p, nullptr, a->m_words.p, (uint32_t)K, a->m_records.p))) return rc;
    if ((rc = accumulator_merge_fold_enqueue(a->stream, a->m_records.p, (uint32_t)K, 0, a->m_words.p + 8 * K, a->j_cap ? a->j_sums.p : nullptr, a->acc.p))) return rc;
    drain.armed = false;
    if ((rc = sync(a, who))) return rc;
    for (size_t k = 0; k < K; ++k) {
        a->n_proofs += src_proofs[k]; a->n_failed += src_failed[k];
        commit_entry(a, Fr::one(), src_proofs[k], src_failed[k]);
    }
    return 0;
}
uint32_t load_u32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
uint64_t load_u64(const uint8_t* p) { return (uint64_t)load_u32(p) | ((uint64_t)load_u32(p + 4) << 32); }
void store_u64(uint8_t* p, uint64_t v) { store_u32(p, (uint32_t)v); store_u32(p + 4, (uint32_t)(v >> 32)); }

}  // namespace

extern "C" {

int h2v_accumulator_create(h2v_ctx* ctx, h2v_accumulator** out) {
    if (!ctx || !out) { set_last_error("h2v_accumulator_create: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    *out = nullptr;
    H2V_HIP_CHECK(hipSetDevice(ctx->device));
    std::unique_ptr<h2v_accumulator, void (*)(h2v_accumulator*)> a(new h2v_accumulator, h2v_accumulator_destroy);
    a->ctx = ctx;
    // A stream of the highest priority: the runtime keeps hardware queues per priority, so this stream never shares an in-order queue
    // with the batches' streams (all of normal priority), whatever other streams the process has made — the scale step then runs
    // BESIDE a call's groups, not in front of them on their queue ("Streams and hardware queues").
    int least = 0, greatest = 0;
    H2V_HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    H2V_HIP_CHECK(hipStreamCreateWithPriority(&a->stream, hipStreamNonBlocking, greatest));
    int rc;
    if ((rc = a->acc.alloc(2)) || (rc = a->records.alloc((size_t)H2V_ACC_RECORD_BYTES * (1 + H2V_MAX_SHAPES_PER_CALL))) || (rc = a->scalar.alloc(8)) ||
        (rc = a->words.alloc(7)) || (rc = a->bytes.alloc(128)) || (rc = a->affine.alloc(2)) || (rc = a->jacobian.alloc(2))) return rc;
    const G1J empty[2] = {G1J::identity(), G1J::identity()};   // AccumulatorStrategy::new: an empty DualMSM
    H2V_HIP_CHECK(hipMemcpyAsync(a->acc.p, empty, sizeof(empty), hipMemcpyHostToDevice, a->stream));
    if ((rc = sync(a.get(), "h2v_accumulator_create"))) return rc;
    *out = a.release();
    return 0;
}

void h2v_accumulator_destroy(h2v_accumulator* a) {
    if (!a) return;
    hipSetDevice(a->ctx->device);
    if (a->stream) { hipStreamSynchronize(a->stream); hipStreamDestroy(a->stream); }   // (enqueued feeds included: their batches are free of this object afterwards)
    for (void* p : a->f_retired) hipFree(p);
    if (a->ev_batch) hipEventDestroy(a->ev_batch);
    delete a;
}

// h2v_accumulator_process, with or without hint rows (h2v_accumulator_process_hinted, include/h2v_hints.h)
static int process_proofs(const char* who, h2v_accumulator* a, h2v_ctx* const* ctxs, size_t n_keys, const uint32_t* key_of_proof, size_t n, const uint8_t* const* proofs,
                          const size_t* proof_lens, const uint8_t* const* instances32, const size_t* n_instance_columns, const size_t* col_lens,
                          const uint8_t* rand32, int* per_proof_status, int* all_ok, const CallHints& hints) {
    // every argument check comes before the first HIP call
    if (!a || (n && !key_of_proof)) { set_last_error(std::string(who) + ": null argument"); return H2V_ERR_BAD_ARGUMENT; }
    std::vector<CallGroup> groups;
    int rc;
    if ((rc = settle_feeds(a, who))) return rc;
    if ((rc = grouped_call_args(who, ctxs, n_keys, key_of_proof, n, proofs, proof_lens, instances32, n_instance_columns, col_lens, groups))) return rc;
    for (size_t k = 0; k < n_keys; ++k) {
        if (ctxs[k]->device != a->ctx->device) { set_last_error(std::string(who) + ": a context on another device than the accumulator"); return H2V_ERR_BAD_ARGUMENT; }
        if (!same_srs(ctxs[k]->params, a->ctx->params)) { set_last_error(std::string(who) + ": a context over other params than the accumulator (g[0], g2 or s_g2 differ)"); return H2V_ERR_BAD_ARGUMENT; }
    }
    std::vector<uint8_t> os_rand;
    if ((rc = resolve_draws(rand32, n, os_rand, who))) return rc;
    if (all_ok) *all_ok = 1;
    if (!n) return 0;   // no verify_proof: no scale, no Guard, no entry
    if (journal_full(a)) { set_last_error(std::string(who) + ": the journal is full"); return H2V_ERR_UNSUPPORTED; }
    // M, the product of the call's draws (host: n Fr products)
    Fr M = Fr::one();
    for (size_t i = 0; i < n; ++i) { Fr r; Fr::from_bytes(rand32 + 32 * i, r); M = M * r; }
    uint8_t m_bytes[32];
    M.to_bytes(m_bytes);
    memcpy(a->host_scalar, m_bytes, 32);
    H2V_HIP_CHECK(hipSetDevice(a->ctx->device));
    // on an error past this point the stream is drained before the call returns; the accumulator is written by the last step only
    Drain drain{a->stream};
    // the scale step first, beside the groups: staging record <- M (L, R)
    H2V_HIP_CHECK(hipMemcpyAsync(a->scalar.p, a->host_scalar, 32, hipMemcpyHostToDevice, a->stream));
    if ((rc = accumulator_scale_enqueue(a->stream, a->acc.p, a->scalar.p, a->records.p))) return rc;
    // the groups, each without a pairing, finished by the host when this returns: records 1 ..
    GroupsHeldPtr held;   // the contexts' locks and scratch batches, until the call returns
    std::vector<std::vector<int>> st;
    bool groups_ok = true;
    if ((rc = run_group_batches(ctxs, n_keys, groups, n, proofs, proof_lens, instances32, rand32, a->records.p + H2V_ACC_RECORD_BYTES, false, held, st, groups_ok, hints))) return rc;
    // the journal's entry: the groups' records alone, into a slot no entry owns yet
    if (G1J* slot = next_slot(a))
        if ((rc = fold_records_enqueue(a->stream, a->records.p + H2V_ACC_RECORD_BYTES, (uint32_t)groups.size(), 1, 1, 0, slot, nullptr, nullptr, a->words.p + 6))) return rc;
    // the commit: (L, R) <- staging record + the groups' records
    if ((rc = fold_records_enqueue(a->stream, a->records.p, (uint32_t)(1 + groups.size()), 1, 1, 0, a->acc.p, nullptr, nullptr, a->words.p))) return rc;
    drain.armed = false;
    if ((rc = sync(a, who))) return rc;
    size_t failed = 0;
    for (size_t gi = 0; gi < groups.size(); ++gi)
        for (size_t j = 0; j < groups[gi].idx.size(); ++j) {
            if (st[gi][j]) ++failed;
            if (per_proof_status) per_proof_status[groups[gi].idx[j]] = st[gi][j];
        }
    a->n_proofs += n; a->n_failed += failed;
    commit_entry(a, M, n, failed);
    if (all_ok) *all_ok = failed ? 0 : 1;
    return 0;
}
int h2v_accumulator_process(h2v_accumulator* a, h2v_ctx* const* ctxs, size_t n_keys, const uint32_t* key_of_proof, size_t n, const uint8_t* const* proofs,
                            const size_t* proof_lens, const uint8_t* const* instances32, const size_t* n_instance_columns, const size_t* col_lens,
                            const uint8_t* rand32, int* per_proof_status, int* all_ok) {
    return process_proofs("h2v_accumulator_process", a, ctxs, n_keys, key_of_proof, n, proofs, proof_lens, instances32, n_instance_columns, col_lens, rand32, per_proof_status,
                          all_ok, CallHints());
}
int h2v_accumulator_process_hinted(h2v_accumulator* a, h2v_ctx* const* ctxs, size_t n_keys, const uint32_t* key_of_proof, size_t n, const uint8_t* const* proofs,
                                   const size_t* proof_lens, const uint8_t* const* hint_rows, const uint8_t* const* instances32, const size_t* n_instance_columns,
                                   const size_t* col_lens, const uint8_t* rand32, int* per_proof_status, int* all_ok, size_t hint_stats[3]) {
    size_t stats[3] = {0, 0, 0};
    const int rc = process_proofs("h2v_accumulator_process_hinted", a, ctxs, n_keys, key_of_proof, n, proofs, proof_lens, instances32, n_instance_columns, col_lens, rand32,
                                  per_proof_status, all_ok, CallHints{hint_rows, hint_stats ? stats : nullptr});
    if (!rc && hint_stats) memcpy(hint_stats, stats, sizeof stats);
    return rc;
}

// n x (scale by the draw, add the Guard), the Guards supplied by the caller: process with the groups' chains replaced by one conversion of
// the terms (k_guard_terms: bytes -> MSM inputs, each scalar times its guard's multiplier) and one pooled MSM of two problems.
//   scale step first (staging record <- M (L, R)), beside the rest; multipliers; terms; MSM -> g_sums; the validity word read behind a
//   synchronise; then g_sums as record 1, the journal's entry, and the fold that writes the accumulator, as the last step.
int h2v_accumulator_process_guards(h2v_accumulator* a, size_t n, const size_t* left_counts, const size_t* right_counts, const uint8_t* left_scalars32,
                                   const uint8_t* left_bases64, const uint8_t* right_scalars32, const uint8_t* right_bases64, const uint8_t* rand32) {
    const char* who = "h2v_accumulator_process_guards";
    // every argument check the host can make comes before the first HIP call
    if (!a) { set_last_error(std::string(who) + ": null argument"); return H2V_ERR_BAD_ARGUMENT; }
    GuardArgs g{n, {left_counts, right_counts}, {left_scalars32, right_scalars32}, {left_bases64, right_bases64}, {}};
    int rc;
    if ((rc = settle_feeds(a, who))) return rc;
    if ((rc = guard_args_check(who, g))) return rc;
    std::vector<uint8_t> os_rand;
    if ((rc = resolve_draws(rand32, n, os_rand, who))) return rc;
    if (!n) return 0;   // no verify_proof: no scale, no Guard, no entry
    if (journal_full(a)) { set_last_error(std::string(who) + ": the journal is full"); return H2V_ERR_UNSUPPORTED; }
    Fr M = Fr::one();
    for (size_t i = 0; i < n; ++i) { Fr r; Fr::from_bytes(rand32 + 32 * i, r); M = M * r; }
    uint8_t m_bytes[32];
    M.to_bytes(m_bytes);
    memcpy(a->host_scalar, m_bytes, 32);
    H2V_HIP_CHECK(hipSetDevice(a->ctx->device));
    const GroupShape whole{1, (uint32_t)n, (uint32_t)n, nullptr};   // the Guards of one call: one group, a draw each
    const uint32_t nl = (uint32_t)std::max<size_t>(g.off[0][n], 1), nr = (uint32_t)std::max<size_t>(g.off[1][n], 1);   // (an empty side is staged as one zero term)
    if ((rc = a->g_rand.reserve(32 * n)) || (rc = a->g_mult.reserve(n)) || (rc = a->g_tiles.reserve(multipliers_scratch(whole))) || (rc = a->g_sums.reserve(2)) ||
        (rc = a->g_ws.reserve(std::max(nl + nr, 1024u), 2, std::max(nl, nr)))) return rc;
    hipStream_t s = a->stream;
    Drain drain{s};
    // the scale step first: it depends on the draws and the previous accumulator only
    H2V_HIP_CHECK(hipMemcpyAsync(a->scalar.p, a->host_scalar, 32, hipMemcpyHostToDevice, s));
    if ((rc = accumulator_scale_enqueue(s, a->acc.p, a->scalar.p, a->records.p))) return rc;
    H2V_HIP_CHECK(hipMemcpyAsync(a->g_rand.p, rand32, 32 * n, hipMemcpyHostToDevice, s));
    if ((rc = multipliers_enqueue(s, whole, a->g_rand.p, nullptr, a->g_mult.p, a->g_tiles.p))) return rc;
    GuardStage& st = a->g_stage;
    if ((rc = guard_stage_enqueue(s, st, g, 0, n, false, a->g_mult.p))) return rc;
    MsmProblems pr;
    for (uint32_t q = 0; q < 2; ++q) pr.p.push_back(MsmProblem(st.scal.p + 8 * (size_t)st.seg[q], st.pts.p + st.seg[q], a->g_sums.p + q, 8, 1, st.seg[q + 1] - st.seg[q]));
    a->g_ws.tune = a->ctx->tuning;
    if ((rc = msm_enqueue_multi(s, a->g_ws, pr))) return rc;
    // the one synchronise in front of the commit: no term of the call is bad, or nothing of the accumulator changes
    drain.armed = false;
    if ((rc = sync(a, who))) return rc;
    if ((rc = guard_stage_verdict(who, st, 0))) return rc;
    drain.armed = true;
    if ((rc = export_records_enqueue(s, a->g_sums.p, nullptr, 1, 0, nullptr, 0, 1, a->records.p + H2V_ACC_RECORD_BYTES))) return rc;
    // the journal's entry: the call's own sum, into a slot no entry owns yet
    if (G1J* slot = next_slot(a))
        if ((rc = fold_records_enqueue(s, a->records.p + H2V_ACC_RECORD_BYTES, 1, 1, 1, 0, slot, nullptr, nullptr, a->words.p + 6))) return rc;
    // the commit: (L, R) <- staging record + the call's sum
    if ((rc = fold_records_enqueue(s, a->records.p, 2, 1, 1, 0, a->acc.p, nullptr, nullptr, a->words.p))) return rc;
    drain.armed = false;
    if ((rc = sync(a, who))) return rc;
    a->n_proofs += n;
    commit_entry(a, M, n, 0);
    return 0;
}

// The G groups of a finished staged batch as G legs, in group order: process once per group, with the groups' chains replaced by what the
// launch left on the device.  Group g's own sum S_g is b->acc[2g], [2g + 1]; its M_g is its first draw (b->tail) times its first proof's
// multiplier (b->mult).  Three launches on the accumulator's stream, no host synchronise between them:
//   k_leg_weights             [prod M, W_0 .. W_{G-1}] and [M_0 .. M_{G-1}], W_g = prod_{f > g} M_f
//   k_accumulator_scale       G + 1 items over the gathered pairs [(L, R), S_0 .. S_{G-1}]: the records M (L, R), W_g S_g
//   k_accumulator_legs_fold   the unscaled S_g into the journal slots of G new entries, then (L, R) <- the sum of the records: the last step
// The M_g reach the host behind the one synchronise (the batch keeps no host draws); the counters and the entries follow it.  The batch
// is only read: its stream is idle (the stage is Finished), and nothing of its state changes.
int h2v_accumulator_process_batch(h2v_accumulator* a, h2v_batch* b, size_t* n_proofs_added, size_t* n_failed_added) {
    const char* who = "h2v_accumulator_process_batch";
    // every argument check comes before the first HIP call
    if (!a || !b) { set_last_error(std::string(who) + ": null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if (int rcs = settle_feeds(a, who)) return rcs;
    if (b->stage != BatchStage::Finished) { set_last_error(std::string(who) + ": the batch has no finished launch (h2v_batch_finish / _finish_groups)"); return H2V_ERR_BAD_ARGUMENT; }
    if (b->last.folded) { set_last_error(std::string(who) + ": a fold ran since the launch: the batch holds the folded records' sums, not its own"); return H2V_ERR_BAD_ARGUMENT; }
    if (b->n_tail != b->n) { set_last_error(std::string(who) + ": the batch is a shard (a tail of draws longer than the upload)"); return H2V_ERR_BAD_ARGUMENT; }
    if (b->n && !b->mult_of_draws) { set_last_error(std::string(who) + ": the batch's multipliers are not those of its uploaded draws"); return H2V_ERR_BAD_ARGUMENT; }
    if (b->plan && b->plan->host.opts.guard_terms) { set_last_error(std::string(who) + ": a guard-variant upload (h2v_guard_msm)"); return H2V_ERR_BAD_ARGUMENT; }
    if (b->ctx->device != a->ctx->device) { set_last_error(std::string(who) + ": a batch on another device than the accumulator"); return H2V_ERR_BAD_ARGUMENT; }
    if (!same_srs(b->ctx->params, a->ctx->params)) { set_last_error(std::string(who) + ": a batch over other params than the accumulator (g[0], g2 or s_g2 differ)"); return H2V_ERR_BAD_ARGUMENT; }
    const size_t G = b->groups, n = b->n;
    if (n_proofs_added) *n_proofs_added = 0;
    if (n_failed_added) *n_failed_added = 0;
    if (!n) return 0;   // no verify_proof: no scale, no Guard, no entry
    if (a->j_cap && a->entries.size() + G > a->j_cap) { set_last_error(std::string(who) + ": the journal has fewer free entries than the batch has groups"); return H2V_ERR_UNSUPPORTED; }
    // the groups' counters, from the statuses the finished launch left in the batch's host block
    const int* st = results_at(b->results_host.p, ResultsLayout{G, n}).status;
    std::vector<size_t> count(G), failed(G, 0);
    size_t all_failed = 0;
    for (size_t g = 0, i = 0; g < G; ++g) {
        count[g] = group_shape(b).count(g);
        for (size_t k = 0; k < count[g]; ++k, ++i) if (st[i]) ++failed[g];
        all_failed += failed[g];
    }
    H2V_HIP_CHECK(hipSetDevice(a->ctx->device));
    int rc;
    if ((rc = a->l_pairs.reserve(2 * (G + 1))) || (rc = a->l_records.reserve((size_t)H2V_ACC_RECORD_BYTES * (G + 1))) || (rc = a->l_words.reserve(8 * (G + 1) + 9 * G)) ||
        (rc = a->l_legs.reserve(32 * G))) return rc;
    a->l_host.resize(G);
    uint32_t* d_weights = a->l_words.p;
    uint32_t* d_legs = d_weights + 8 * (G + 1);
    uint32_t* d_slots = d_legs + 8 * G;
    const uint8_t* h_legs = a->l_legs.p;
    uint32_t* h_slots = a->l_host.data();
    hipStream_t s = a->stream;
    Drain drain{s};
    // the pairs, gathered in the accumulator's stream order: (L, R), then the groups' sums as the launch left them
    H2V_HIP_CHECK(hipMemcpyAsync(a->l_pairs.p, a->acc.p, 2 * sizeof(G1J), hipMemcpyDeviceToDevice, s));
    H2V_HIP_CHECK(hipMemcpyAsync(a->l_pairs.p + 2, b->acc.p, 2 * G * sizeof(G1J), hipMemcpyDeviceToDevice, s));
    if (a->j_cap) {
        for (size_t g = 0; g < G; ++g) h_slots[g] = a->free_slots[a->free_slots.size() - 1 - g];   // the lowest free slots, in group order
        H2V_HIP_CHECK(hipMemcpyAsync(d_slots, h_slots, 4 * G, hipMemcpyHostToDevice, s));
    }
    if ((rc = leg_weights_enqueue(s, group_shape_device(b), b->tail.p, b->mult.p, d_weights, d_legs))) return rc;
    H2V_HIP_CHECK(hipMemcpyAsync(a->l_legs.p, d_legs, 32 * G, hipMemcpyDeviceToHost, s));   // (in front of the commit: nothing that can fail is enqueued behind it)
    if ((rc = accumulator_scale_many_enqueue(s, a->l_pairs.p, nullptr, d_weights, (uint32_t)(G + 1), a->l_records.p))) return rc;
    // the commit: the journal's slots, then (L, R) <- M (L, R) + sum_g W_g S_g
    if ((rc = accumulator_legs_fold_enqueue(s, a->l_records.p, (uint32_t)(G + 1), 0, a->l_pairs.p + 2, d_slots, a->j_cap ? a->j_sums.p : nullptr, a->acc.p))) return rc;
    drain.armed = false;
    if ((rc = sync(a, who))) return rc;
    for (size_t g = 0; g < G; ++g) {
        Fr M;
        Fr::from_bytes(h_legs + 32 * g, M);
        commit_entry(a, M, count[g], failed[g]);
    }
    a->n_proofs += n; a->n_failed += all_failed;
    if (n_proofs_added) *n_proofs_added = n;
    if (n_failed_added) *n_failed_added = all_failed;
    return 0;
}

int h2v_accumulator_add_msm(h2v_accumulator* a, const uint8_t* left_scalars32, const uint8_t* left_bases64, size_t n_left,
                            const uint8_t* right_scalars32, const uint8_t* right_bases64, size_t n_right) {
    const char* who = "h2v_accumulator_add_msm";
    if (!a || (n_left && (!left_scalars32 || !left_bases64)) || (n_right && (!right_scalars32 || !right_bases64))) { set_last_error(std::string(who) + ": null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if (n_left > (1u << 24) || n_right > (1u << 24)) { set_last_error(std::string(who) + ": too many terms"); return H2V_ERR_BAD_ARGUMENT; }
    if (int rcs = settle_feeds(a, who)) return rcs;
    const uint8_t* sc[2] = {left_scalars32, right_scalars32};
    const size_t ns[2] = {n_left, n_right};
    for (int side = 0; side < 2; ++side)
        for (size_t j = 0; j < ns[side]; ++j) {
            Fr v;
            if (!Fr::from_bytes(sc[side] + 32 * j, v)) { set_last_error(std::string(who) + ": scalar not canonical"); return H2V_ERR_BAD_ARGUMENT; }
        }
    if (journal_full(a)) { set_last_error(std::string(who) + ": the journal is full"); return H2V_ERR_UNSUPPORTED; }
    // both channels are evaluated (h2v_msm_g1 rejects bases that are not on the curve) before anything of the accumulator changes
    int rc, ident = 0;
    uint8_t xy[128];
    if ((rc = h2v_msm_g1(a->ctx, left_scalars32, left_bases64, n_left, xy, &ident))) return rc;
    if ((rc = h2v_msm_g1(a->ctx, right_scalars32, right_bases64, n_right, xy + 64, &ident))) return rc;
    H2V_HIP_CHECK(hipSetDevice(a->ctx->device));
    hipStream_t s = a->stream;
    // (L, R) <- (L, R) + the two sums, unscaled: the accumulator and the sums as two whole-point records, folded
    H2V_HIP_CHECK(hipMemcpyAsync(a->bytes.p, xy, 128, hipMemcpyHostToDevice, s));
    if ((rc = bases_from_bytes_enqueue(s, a->bytes.p, a->affine.p, a->words.p + 4, 2)) ||
        (rc = affine_to_jacobian_enqueue(s, a->affine.p, a->jacobian.p, 2)) ||
        (rc = affine_to_jacobian_enqueue(s, a->affine.p, next_slot(a), next_slot(a) ? 2 : 0)) ||   // the journal's entry: the two sums
        (rc = export_records_enqueue(s, a->acc.p, nullptr, 1, 0, nullptr, 0, 1, a->records.p)) ||
        (rc = export_records_enqueue(s, a->jacobian.p, nullptr, 1, 0, nullptr, 0, 1, a->records.p + H2V_ACC_RECORD_BYTES)) ||
        (rc = fold_records_enqueue(s, a->records.p, 2, 1, 1, 0, a->acc.p, nullptr, nullptr, a->words.p))) { hipStreamSynchronize(s); return rc; }
    if ((rc = sync(a, who))) return rc;
    commit_entry(a, Fr::one(), 0, 0);
    return 0;
}

// h2v_accumulator_add_msm with both channels resident (h2v_msm, msm_object.hip): one pooled launch of two problems on the context's
// stream evaluates them straight into `jacobian`, and the steps of add_msm behind its two h2v_msm_g1 calls follow — unscaled, the same
// counters, the same journal entry; no point crosses host memory.
int h2v_accumulator_add_msms(h2v_accumulator* a, h2v_msm* left, h2v_msm* right) {
    const char* who = "h2v_accumulator_add_msms";
    if (!a) { set_last_error(std::string(who) + ": null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if (int rcs = settle_feeds(a, who)) return rcs;
    if (journal_full(a)) { set_last_error(std::string(who) + ": the journal is full"); return H2V_ERR_UNSUPPORTED; }
    // both channels are evaluated before anything of the accumulator changes (its stream is idle: the context's stream writes `jacobian`)
    int rc;
    if ((rc = msm_object_eval_pair(a->ctx, who, left, right, a->jacobian.p))) return rc;
    H2V_HIP_CHECK(hipSetDevice(a->ctx->device));
    hipStream_t s = a->stream;
    // (L, R) <- (L, R) + the two sums, unscaled: the accumulator and the sums as two whole-point records, folded
    if (G1J* slot = next_slot(a)) {   // the journal's entry: the two sums
        const hipError_t e = hipMemcpyAsync(slot, a->jacobian.p, 2 * sizeof(G1J), hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) { hipStreamSynchronize(s); set_last_error(std::string(who) + ": " + hipGetErrorString(e)); return H2V_ERR_DEVICE; }
    }
    if ((rc = export_records_enqueue(s, a->acc.p, nullptr, 1, 0, nullptr, 0, 1, a->records.p)) ||
        (rc = export_records_enqueue(s, a->jacobian.p, nullptr, 1, 0, nullptr, 0, 1, a->records.p + H2V_ACC_RECORD_BYTES)) ||
        (rc = fold_records_enqueue(s, a->records.p, 2, 1, 1, 0, a->acc.p, nullptr, nullptr, a->words.p))) { hipStreamSynchronize(s); return rc; }
    if ((rc = sync(a, who))) return rc;
    commit_entry(a, Fr::one(), 0, 0);
    return 0;
}

int h2v_accumulator_read(h2v_accumulator* a, uint8_t out_left_xy[64], uint8_t out_right_xy[64], size_t* n_proofs, size_t* n_failed) {
    if (!a) { set_last_error("h2v_accumulator_read: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if (int rc = read_points(a, "h2v_accumulator_read", nullptr, out_left_xy, out_right_xy)) return rc;
    if (n_proofs) *n_proofs = a->n_proofs;
    if (n_failed) *n_failed = a->n_failed;
    return 0;
}

int h2v_accumulator_finalize(h2v_accumulator* a, int* ok, uint8_t out_left_xy[64], uint8_t out_right_xy[64]) {
    if (!a || !ok) { set_last_error("h2v_accumulator_finalize: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    return read_points(a, "h2v_accumulator_finalize", ok, out_left_xy, out_right_xy);
}

int h2v_accumulator_journal_begin(h2v_accumulator* a, size_t capacity) {
    const char* who = "h2v_accumulator_journal_begin";
    if (!a) { set_last_error(std::string(who) + ": null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if (capacity == 1 || capacity > H2V_ACC_JOURNAL_MAX) { set_last_error(std::string(who) + ": capacity must be 0 or in [2, H2V_ACC_JOURNAL_MAX]"); return H2V_ERR_BAD_ARGUMENT; }
    if (int rcs = settle_feeds(a, who)) return rcs;
    journal_off(a);
    if (!capacity) return 0;
    H2V_HIP_CHECK(hipSetDevice(a->ctx->device));
    int rc;
    if ((rc = a->j_sums.reserve(2 * capacity)) || (rc = a->j_records.reserve((size_t)H2V_ACC_RECORD_BYTES * capacity)) || (rc = a->j_words.reserve(10 * capacity))) return rc;
    // every slot starts as a pair of identities (check_legs reads the slots up to the highest one in use); slot 0 <- the base
    const std::vector<G1J> empty(2 * capacity, G1J::identity());
    H2V_HIP_CHECK(hipMemcpyAsync(a->j_sums.p, empty.data(), empty.size() * sizeof(G1J), hipMemcpyHostToDevice, a->stream));
    H2V_HIP_CHECK(hipMemcpyAsync(a->j_sums.p, a->acc.p, 2 * sizeof(G1J), hipMemcpyDeviceToDevice, a->stream));
    if ((rc = sync(a, who))) return rc;
    a->j_cap = capacity;
    a->j_host.assign(10 * capacity, 0);
    for (size_t sl = capacity; sl-- > 1;) a->free_slots.push_back((uint32_t)sl);
    a->entries.push_back({0, Fr::one(), a->n_proofs, a->n_failed});
    return 0;
}

int h2v_accumulator_check_legs(h2v_accumulator* a, size_t cap, size_t* n_legs, size_t* leg_proofs, size_t* leg_failed, int* leg_pairing_ok) {
    const char* who = "h2v_accumulator_check_legs";
    if (!a || !n_legs) { set_last_error(std::string(who) + ": null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if (int rcs = settle_feeds(a, who)) return rcs;
    const size_t J = a->entries.size();
    *n_legs = J;
    if ((leg_proofs || leg_failed || leg_pairing_ok) && cap < J) { set_last_error(std::string(who) + ": the arrays are shorter than the journal"); return H2V_ERR_BAD_ARGUMENT; }
    for (size_t e = 0; e < J; ++e) {
        if (leg_proofs) leg_proofs[e] = a->entries[e].n_proofs;
        if (leg_failed) leg_failed[e] = a->entries[e].n_failed;
    }
    if (!J || !leg_pairing_ok) return 0;
    // the slots in use are the lowest ones but for what drop_legs freed: every slot below the highest in use holds a pair of points
    uint32_t hi = 0;
    for (const auto& e : a->entries) hi = std::max(hi, e.slot + 1);
    H2V_HIP_CHECK(hipSetDevice(a->ctx->device));
    int rc;
    uint32_t* d_ok = a->j_words.p + 9 * a->j_cap;
    uint32_t* h_ok = a->j_host.data() + 9 * a->j_cap;
    if ((rc = pairing_check_enqueue(a->stream, a->ctx->pairing, a->j_sums.p, hi, d_ok))) { hipStreamSynchronize(a->stream); return rc; }
    H2V_HIP_CHECK(hipMemcpyAsync(h_ok, d_ok, 4 * (size_t)hi, hipMemcpyDeviceToHost, a->stream));
    if ((rc = sync(a, who))) return rc;
    for (size_t e = 0; e < J; ++e) leg_pairing_ok[e] = h_ok[a->entries[e].slot] ? 1 : 0;
    return 0;
}

int h2v_accumulator_drop_legs(h2v_accumulator* a, const size_t* legs, size_t n_drop) {
    const char* who = "h2v_accumulator_drop_legs";
    if (!a || (n_drop && !legs)) { set_last_error(std::string(who) + ": null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if (int rcs = settle_feeds(a, who)) return rcs;
    if (!a->j_cap) { set_last_error(std::string(who) + ": the journal is off"); return H2V_ERR_BAD_ARGUMENT; }
    const size_t J = a->entries.size();
    std::vector<bool> drop(J, false);
    for (size_t i = 0; i < n_drop; ++i) {
        if (legs[i] == 0 || legs[i] >= J || drop[legs[i]]) { set_last_error(std::string(who) + ": an entry index that is 0 (the base), out of range or given twice"); return H2V_ERR_BAD_ARGUMENT; }
        drop[legs[i]] = true;
    }
    // W_e of the kept entries, from the last one down, and their slots
    std::vector<size_t> kept;
    for (size_t e = 0; e < J; ++e) if (!drop[e]) kept.push_back(e);
    const size_t K = kept.size();   // >= 1: the base
    uint32_t* h = a->j_host.data();
    Fr W = Fr::one();
    for (size_t i = K; i-- > 0;) {
        uint8_t w_bytes[32];
        W.to_bytes(w_bytes);
        memcpy(h + 8 * i, w_bytes, 32);
        h[8 * K + i] = a->entries[kept[i]].slot;
        W = W * a->entries[kept[i]].M;
    }
    H2V_HIP_CHECK(hipSetDevice(a->ctx->device));
    Drain drain{a->stream};
    int rc;
    H2V_HIP_CHECK(hipMemcpyAsync(a->j_words.p, h, 4 * 9 * K, hipMemcpyHostToDevice, a->stream));
    if ((rc = accumulator_scale_many_enqueue(a->stream, a->j_sums.p, a->j_words.p + 8 * K, a->j_words.p, (uint32_t)K, a->j_records.p))) return rc;
    // the commit: (L, R) <- the sum of the K records
    if ((rc = fold_records_enqueue(a->stream, a->j_records.p, (uint32_t)K, 1, 1, 0, a->acc.p, nullptr, nullptr, a->words.p))) return rc;
    drain.armed = false;
    if ((rc = sync(a, who))) return rc;
    std::vector<h2v_accumulator::Entry> next;
    size_t n_proofs = 0, n_failed = 0;
    for (size_t e = 0; e < J; ++e) {
        if (drop[e]) { a->free_slots.push_back(a->entries[e].slot); continue; }
        next.push_back(a->entries[e]);
        n_proofs += a->entries[e].n_proofs; n_failed += a->entries[e].n_failed;
    }
    std::sort(a->free_slots.begin(), a->free_slots.end(), std::greater<uint32_t>());
    a->entries.swap(next);
    a->n_proofs = n_proofs; a->n_failed = n_failed;
    return 0;
}

int h2v_accumulator_merge(h2v_accumulator* dst, h2v_accumulator* const* srcs, size_t n_src, const uint8_t* draws32, uint8_t* out_draws32) {
    const char* who = "h2v_accumulator_merge";
    // every argument check comes before the first HIP call
    if (!dst || (n_src && !srcs)) { set_last_error(std::string(who) + ": null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if (n_src > H2V_ACC_MERGE_MAX) { set_last_error(std::string(who) + ": more than H2V_ACC_MERGE_MAX sources"); return H2V_ERR_BAD_ARGUMENT; }
    for (size_t k = 0; k < n_src; ++k) {
        if (!srcs[k]) { set_last_error(std::string(who) + ": null source"); return H2V_ERR_BAD_ARGUMENT; }
        if (srcs[k] == dst) { set_last_error(std::string(who) + ": a source is the destination"); return H2V_ERR_BAD_ARGUMENT; }
        for (size_t j = 0; j < k; ++j) if (srcs[j] == srcs[k]) { set_last_error(std::string(who) + ": a source given twice"); return H2V_ERR_BAD_ARGUMENT; }
        if (srcs[k]->ctx->device != dst->ctx->device) { set_last_error(std::string(who) + ": a source on another device than the destination"); return H2V_ERR_BAD_ARGUMENT; }
        if (!same_srs(srcs[k]->ctx->params, dst->ctx->params)) { set_last_error(std::string(who) + ": a source over other params than the destination (g[0], g2 or s_g2 differ)"); return H2V_ERR_BAD_ARGUMENT; }
    }
    std::vector<uint8_t> os_draws;
    int rc;
    if ((rc = settle_feeds(dst, who))) return rc;
    for (size_t k = 0; k < n_src; ++k) if ((rc = settle_feeds(srcs[k], who))) return rc;
    if ((rc = merge_args(dst, who, n_src, draws32, os_draws))) return rc;
    if (!n_src) return 0;
    H2V_HIP_CHECK(hipSetDevice(dst->ctx->device));
    if ((rc = merge_reserve(dst, n_src, false))) return rc;
    Drain drain{dst->stream};
    // the sources are idle (every call of the object ends in a synchronise): their pairs are gathered in the destination's stream order
    std::vector<size_t> np(n_src), nf(n_src);
    for (size_t k = 0; k < n_src; ++k) {
        H2V_HIP_CHECK(hipMemcpyAsync(dst->m_pairs.p + 2 * k, srcs[k]->acc.p, 2 * sizeof(G1J), hipMemcpyDeviceToDevice, dst->stream));
        np[k] = srcs[k]->n_proofs; nf[k] = srcs[k]->n_failed;
    }
    if ((rc = merge_impl(dst, who, n_src, draws32, np.data(), nf.data(), drain))) return rc;
    if (out_draws32) memcpy(out_draws32, draws32, 32 * n_src);
    return 0;
}

int h2v_accumulator_export_state(h2v_accumulator* a, uint8_t out[H2V_ACC_STATE_BYTES]) {
    if (!a || !out) { set_last_error("h2v_accumulator_export_state: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    uint8_t xy[128];
    if (int rc = read_points(a, "h2v_accumulator_export_state", nullptr, xy, xy + 64)) return rc;
    store_u32(out, H2V_ACC_STATE_MAGIC); store_u32(out + 4, H2V_ACC_STATE_VERSION);
    store_u64(out + 8, a->n_proofs); store_u64(out + 16, a->n_failed);
    memcpy(out + 24, xy, 128);
    return 0;
}

int h2v_accumulator_merge_states(h2v_accumulator* dst, const uint8_t* states, size_t n, const uint8_t* draws32, uint8_t* out_draws32) {
    const char* who = "h2v_accumulator_merge_states";
    if (!dst || (n && !states)) { set_last_error(std::string(who) + ": null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if (n > H2V_ACC_MERGE_MAX) { set_last_error(std::string(who) + ": more than H2V_ACC_MERGE_MAX states"); return H2V_ERR_BAD_ARGUMENT; }
    std::vector<size_t> np(n), nf(n);
    for (size_t k = 0; k < n; ++k) {
        const uint8_t* st = states + (size_t)H2V_ACC_STATE_BYTES * k;
        if (load_u32(st) != H2V_ACC_STATE_MAGIC || load_u32(st + 4) != H2V_ACC_STATE_VERSION) { set_last_error(std::string(who) + ": a state with a wrong magic or version"); return H2V_ERR_BAD_ARGUMENT; }
        const uint64_t p = load_u64(st + 8), f = load_u64(st + 16);
        if (f > p) { set_last_error(std::string(who) + ": a state with more failed proofs than proofs"); return H2V_ERR_BAD_ARGUMENT; }
        np[k] = (size_t)p; nf[k] = (size_t)f;
    }
    std::vector<uint8_t> os_draws;
    int rc;
    if ((rc = settle_feeds(dst, who))) return rc;
    if ((rc = merge_args(dst, who, n, draws32, os_draws))) return rc;
    if (!n) return 0;
    H2V_HIP_CHECK(hipSetDevice(dst->ctx->device));
    if ((rc = merge_reserve(dst, n, true))) return rc;
    Drain drain{dst->stream};
    // the lift: bytes -> affine Montgomery (with the curve check) -> Jacobian pairs, as add_msm lifts its sums
    std::vector<uint8_t> xy(128 * n);
    for (size_t k = 0; k < n; ++k) memcpy(&xy[128 * k], states + (size_t)H2V_ACC_STATE_BYTES * k + 24, 128);
    uint32_t* d_flags = dst->m_words.p + 9 * n;
    uint32_t* h_flags = dst->m_host.data() + 9 * n;
    H2V_HIP_CHECK(hipMemcpyAsync(dst->m_bytes.p, xy.data(), xy.size(), hipMemcpyHostToDevice, dst->stream));
    if ((rc = bases_from_bytes_enqueue(dst->stream, dst->m_bytes.p, dst->m_affine.p, d_flags, (uint32_t)(2 * n))) ||
        (rc = affine_to_jacobian_enqueue(dst->stream, dst->m_affine.p, dst->m_pairs.p, (uint32_t)(2 * n)))) return rc;
    H2V_HIP_CHECK(hipMemcpyAsync(h_flags, d_flags, 4 * 2 * n, hipMemcpyDeviceToHost, dst->stream));
    if ((rc = sync(dst, who))) { drain.armed = false; return rc; }
    for (size_t i = 0; i < 2 * n; ++i)
        if (h_flags[i]) { set_last_error(std::string(who) + ": a state with a point that is not canonical or not on the curve"); return H2V_ERR_BAD_ARGUMENT; }
    if ((rc = merge_impl(dst, who, n, draws32, np.data(), nf.data(), drain))) return rc;
    if (out_draws32) memcpy(out_draws32, draws32, 32 * n);
    return 0;
}

// h2v_accumulator_process_batch, enqueued (include/h2v_feed.h).  On the batch's stream join_tail / ensure_whole and an event; on the
// accumulator's stream, behind that event:
//   k_feed_gather             l_pairs <- [(L, R), S_0 .. S_{G-1}]; the groups' sizes and failed counts from the device's status words
//   k_feed_weights            k_leg_weights, failing closed on the upload's fault word: [1, 0 .. 0] and rc = H2V_ERR_BAD_ARGUMENT
//   -- the batch's read event: nothing behind it reads the batch
//   k_accumulator_scale       G + 1 items
//   k_accumulator_legs_fold   the journal slots (read from the feed's pinned block), then (L, R): the only write to the accumulator
//   k_feed_report             the report into the feed's pinned block
// No synchronise, no copy.  The host's half waits in a->feeds for settle_feeds.
int h2v_accumulator_feed_batch(h2v_accumulator* a, h2v_batch* b) {
    const char* who = "h2v_accumulator_feed_batch";
    // every check comes before the first HIP call: a refusal leaves both objects untouched
    if (!a || !b) { set_last_error(std::string(who) + ": null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if (b->stage < BatchStage::Launched) { set_last_error(std::string(who) + ": the batch has no launch (h2v_batch_launch)"); return H2V_ERR_BAD_ARGUMENT; }
    if (b->last.folded) { set_last_error(std::string(who) + ": a fold ran since the launch: the batch holds the folded records' sums, not its own"); return H2V_ERR_BAD_ARGUMENT; }
    if (b->n_tail != b->n) { set_last_error(std::string(who) + ": the batch is a shard (a tail of draws longer than the upload)"); return H2V_ERR_BAD_ARGUMENT; }
    if (b->n && !b->mult_of_draws) { set_last_error(std::string(who) + ": the batch's multipliers are not those of its uploaded draws"); return H2V_ERR_BAD_ARGUMENT; }
    if (b->plan && b->plan->host.opts.guard_terms) { set_last_error(std::string(who) + ": a guard-variant upload (h2v_guard_msm)"); return H2V_ERR_BAD_ARGUMENT; }
    if (b->ctx->device != a->ctx->device) { set_last_error(std::string(who) + ": a batch on another device than the accumulator"); return H2V_ERR_BAD_ARGUMENT; }
    if (!same_srs(b->ctx->params, a->ctx->params)) { set_last_error(std::string(who) + ": a batch over other params than the accumulator (g[0], g2 or s_g2 differ)"); return H2V_ERR_BAD_ARGUMENT; }
    const size_t G = b->groups, n = b->n;
    if (!n) return 0;   // no verify_proof: no scale, no Guard, no entry, no report
    if (G > 512) { set_last_error(std::string(who) + ": more than 512 groups"); return H2V_ERR_BAD_ARGUMENT; }
    size_t legs_pending = 0;
    for (const auto& f : a->feeds) legs_pending += f.slots.size();   // (a settled feed holds none)
    if (a->j_cap && a->entries.size() + legs_pending + G > a->j_cap) {
        set_last_error(std::string(who) + ": the journal has fewer free entries than the batch has groups (the legs of the feeds not settled yet counted)");
        return H2V_ERR_UNSUPPORTED;
    }
    if (a->feeds.size() >= H2V_FEED_MAX_PENDING) { set_last_error(std::string(who) + ": H2V_FEED_MAX_PENDING feeds wait for h2v_accumulator_settle"); return H2V_ERR_UNSUPPORTED; }
    H2V_HIP_CHECK(hipSetDevice(a->ctx->device));
    int rc;
    if (!a->ev_batch) H2V_HIP_CHECK(hipEventCreateWithFlags(&a->ev_batch, hipEventDisableTiming));
    if (!b->ev_read) H2V_HIP_CHECK(hipEventCreateWithFlags(&b->ev_read, hipEventDisableTiming));
    if ((rc = grow_under_feeds(a, a->l_pairs, 2 * (G + 1))) || (rc = grow_under_feeds(a, a->l_records, (size_t)H2V_ACC_RECORD_BYTES * (G + 1))) ||
        (rc = grow_under_feeds(a, a->l_words, 8 * (G + 1) + 10 * G + 1))) return rc;
    h2v_accumulator::Feed f;
    const size_t block_bytes = 4 * (H2V_FEED_REPORT_WORDS(G) + G);
    for (size_t i = 0; i < a->f_blocks.size() && !f.block; ++i)
        if (a->f_blocks[i]->cap >= block_bytes) { f.block = std::move(a->f_blocks[i]); a->f_blocks.erase(a->f_blocks.begin() + i); }
    if (!f.block) { f.block.reset(new MappedHostBuf); if ((rc = f.block->reserve(block_bytes))) return rc; }
    f.n = (uint32_t)n; f.G = (uint32_t)G;
    uint32_t* const h_report = reinterpret_cast<uint32_t*>(f.block->p);
    uint32_t* const d_report = static_cast<uint32_t*>(f.block->dev);
    h_report[0] = (uint32_t)H2V_ERR_DEVICE;   // (what settle finds if the report kernel never ran)
    for (size_t g = 0; g < G && a->j_cap; ++g) h_report[H2V_FEED_REPORT_WORDS(G) + g] = a->free_slots[a->free_slots.size() - 1 - g];   // the lowest free slots, in group order
    uint32_t* d_weights = a->l_words.p;
    uint32_t* d_legs = d_weights + 8 * (G + 1);
    uint32_t* d_sizes = d_legs + 8 * G;
    uint32_t* d_failed = d_sizes + G;
    uint32_t* d_rc = d_failed + G;
    hipStream_t s = a->stream;
    // the batch's stream: what h2v_batch_finish_device begins with, then the event this stream waits for
    if ((rc = join_tail(b)) || (rc = ensure_whole(b))) return rc;
    H2V_HIP_CHECK(hipEventRecord(a->ev_batch, b->stream));
    H2V_HIP_CHECK(hipStreamWaitEvent(s, a->ev_batch, 0));
    // everything that reads the batch, then the batch's read event
    const GroupShape shape = group_shape_device(b);
    if ((rc = feed_gather_enqueue(s, a->acc.p, b->acc.p, b->status, shape, a->l_pairs.p, d_sizes, d_failed)) ||
        (rc = feed_weights_enqueue(s, shape, b->tail.p, b->mult.p, b->device_draws ? b->ingest_verdict.p : nullptr, d_weights, d_legs, d_rc))) return rc;
    H2V_HIP_CHECK(hipEventRecord(b->ev_read, s));
    b->read_pending = b->read_unseen = true;
    if ((rc = accumulator_scale_many_enqueue(s, a->l_pairs.p, nullptr, d_weights, (uint32_t)(G + 1), a->l_records.p))) return rc;
    // the commit: the journal's slots, then (L, R) <- M (L, R) + sum_g W_g S_g; the report behind it
    if ((rc = accumulator_legs_fold_enqueue(s, a->l_records.p, (uint32_t)(G + 1), 0, a->l_pairs.p + 2, d_report + H2V_FEED_REPORT_WORDS(G), a->j_cap ? a->j_sums.p : nullptr, a->acc.p))) return rc;
    // (from here on the accumulator changes: the feed is recorded whatever the last launch returns)
    rc = feed_report_enqueue(s, d_rc, (uint32_t)n, (uint32_t)G, d_legs, d_sizes, d_failed, d_report);
    for (size_t g = 0; g < G && a->j_cap; ++g) { f.slots.push_back(a->free_slots.back()); a->free_slots.pop_back(); }
    a->feeds.push_back(std::move(f));
    ++a->f_unsettled;
    return rc;
}

int h2v_accumulator_pending(const h2v_accumulator* a, size_t* n_unsettled, size_t* n_unreported) {
    if (!a) { set_last_error("h2v_accumulator_pending: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if (n_unsettled) *n_unsettled = a->f_unsettled;
    if (n_unreported) *n_unreported = a->feeds.size();
    return 0;
}

int h2v_accumulator_settle(h2v_accumulator* a, size_t cap, size_t* n_feeds, int* feed_rc, size_t* feed_proofs, size_t* feed_failed) {
    const char* who = "h2v_accumulator_settle";
    if (!a || !n_feeds) { set_last_error(std::string(who) + ": null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if (int rc = settle_feeds(a, who)) return rc;
    const size_t F = a->feeds.size();
    *n_feeds = F;
    const bool wanted = feed_rc || feed_proofs || feed_failed;
    if (!wanted && !cap) return 0;   // the count alone: the reports are kept
    if (cap < F) { set_last_error(std::string(who) + ": the arrays are shorter than the feeds to report"); return H2V_ERR_BAD_ARGUMENT; }
    for (size_t i = 0; i < F; ++i) {
        h2v_accumulator::Feed& f = a->feeds[i];
        if (feed_rc) feed_rc[i] = f.rc;
        if (feed_proofs) feed_proofs[i] = f.n;
        if (feed_failed) feed_failed[i] = f.failed;
        a->f_blocks.push_back(std::move(f.block));
    }
    a->feeds.clear();
    return 0;
}

}  // extern "C"
