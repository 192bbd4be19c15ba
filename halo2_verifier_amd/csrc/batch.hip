// C-ABI staged batch (include/h2v.h, h2v_batch_*): upload / launch / finish, range re-checks, export and fold.  The one-shot entry
// points (oneshot.hip) run on it through the steps batch.h declares.
#include "../../include/h2v.h"
#include "../../include/h2v_hint_rows.h"
#include "batch.h"
#include "msm_object.h"
#include <string.h>
#include <algorithm>
#include <functional>
#include <utility>
#include <stdio.h>

using namespace h2v;

namespace h2v {

// Element counts of a batch's buffers for a plan, max_proofs N and G groups.  The batch keeps the largest it has met (ensure_buffers).
struct BatchSizes {
    uint32_t stream_words;   // the absorbed stream of one proof, in 64-bit words
    size_t proofs, inst, pts, ycanon, words, chal, mult, slots, msm_scal, shared, left_scal, insteval, guard_scal, acc, results;
    uint32_t ws_terms, ws_problems, ws_per_problem;   // MsmWorkspace::reserve
};
// `largest`: the proofs of the largest group (the bucket arrays follow the largest problem of a launch)
BatchSizes batch_sizes(const Plan& pl, size_t N, size_t G, size_t largest) {
    BatchSizes z;
    z.stream_words = stream_words_for(pl.stream.size(), pl.opts.transcript);
    z.proofs = N * pl.proof_len;
    z.inst = N * (size_t)pl.n_instance_values * 32;
    z.pts = N * pl.n_points + pl.n_shared;
    z.ycanon = N * pl.n_points * 32;
    z.words = (size_t)z.stream_words * N;
    z.chal = (size_t)pl.squeeze_at.size() * N;
    z.mult = N;
    z.slots = (size_t)std::max(std::max(pl.n_slots, pl.n_slots_k[0]), std::max(pl.n_slots_k[1], pl.n_slots_k[2])) * N;
    z.msm_scal = (N * pl.n_points + G * pl.n_shared) * 8;
    z.shared = (size_t)pl.n_shared * N;
    z.left_scal = N * pl.n_points * 8;
    z.insteval = N * pl.inst_queries.size();
    z.guard_scal = N * pl.guard_term_order.size() * 8;
    z.acc = 2 * G;
    z.results = ResultsLayout{G, N}.total();
    z.ws_terms = (uint32_t)(2 * (N * pl.n_points + G * pl.n_shared));
    z.ws_problems = (uint32_t)(2 * G);
    z.ws_per_problem = (uint32_t)(largest * pl.n_points + pl.n_shared);
    return z;
}

// grow the batch's buffers to what `pl` needs at the batch's capacity and group count, and point ok / fold_failed / out_ident /
// out_bytes / status into the results block laid out for that group count
int ensure_buffers(h2v_batch* b, const Plan& pl) {
    const size_t N = b->max_proofs, G = b->groups;
    // the shape at capacity: equal groups of ceil(N / G) proofs each; unequal groups: the sizes set
    const BatchSizes z = batch_sizes(pl, N, G, group_shape_of(b, N + G - 1, N + G - 1, b->group_off.data()).largest());
    int rc;
    if ((rc = b->proofs.reserve(z.proofs)) || (rc = b->inst.reserve(z.inst)) || (rc = b->pts.reserve(z.pts)) || (rc = b->phi.reserve(z.pts)) ||
        (rc = b->ycanon.reserve(z.ycanon)) || (rc = b->words.reserve(z.words)) || (rc = b->chal.reserve(z.chal)) || (rc = b->mult.reserve(z.mult)) ||
        (rc = b->slots.reserve(z.slots)) || (rc = b->msm_scal.reserve(z.msm_scal)) || (rc = b->shared.reserve(z.shared)) ||
        (rc = b->left_scal.reserve(z.left_scal)) || (rc = b->insteval.reserve(z.insteval)) || (rc = b->guard_scal.reserve(z.guard_scal)) ||
        (rc = b->acc.reserve(z.acc)) || (rc = b->results.reserve(z.results)) || (rc = b->results_host.reserve(z.results)))
        return rc;
    // the verdicts are the LAST thing a launch produces: the pairing kernel writes them into the host block itself (one word per group over
    // PCIe) and no copy follows it; everything else in the block is final before the pairing starts and is copied beside it (close_enqueue)
    const ResultsLayout L{G, N};
    const ResultsPtrs dev = results_at(b->results.p, L);
    b->ok = results_at(b->results_host.dev, L).ok;
    b->fold_failed = dev.fold_failed; b->out_ident = dev.out_ident; b->out_bytes = dev.out_bytes; b->status = dev.status;
    if ((rc = b->ws.reserve(z.ws_terms, z.ws_problems, z.ws_per_problem))) return rc;
    b->stream_words = z.stream_words;
    return 0;
}

bool scalar_is_canonical(const uint8_t* s) {
    uint32_t raw[8];
    for (int j = 0; j < 8; ++j) raw[j] = (uint32_t)s[4 * j] | ((uint32_t)s[4 * j + 1] << 8) | ((uint32_t)s[4 * j + 2] << 16) | ((uint32_t)s[4 * j + 3] << 24);
    return !Fr::geq_p(raw);
}
bool scalar_is_zero(const uint8_t* s) { for (int k = 0; k < 32; ++k) if (s[k]) return false; return true; }

// Fr::random(getrandom_or_panic()) of AccumulatorStrategy::process (kzg/strategy.rs:129): 64 OS-random bytes reduced mod r
int os_random_scalars(std::vector<uint8_t>& out, size_t n) {
    out.resize(32 * n);
    FILE* f = fopen("/dev/urandom", "rb");
    if (!f) { set_last_error("cannot open /dev/urandom"); return H2V_ERR_DEVICE; }
    for (size_t i = 0; i < n; ++i) {
        uint8_t buf[64];
        if (fread(buf, 1, 64, f) != 64) { fclose(f); set_last_error("short read from /dev/urandom"); return H2V_ERR_DEVICE; }
        uint32_t w[16];
        for (int j = 0; j < 16; ++j) w[j] = (uint32_t)buf[4 * j] | ((uint32_t)buf[4 * j + 1] << 8) | ((uint32_t)buf[4 * j + 2] << 16) | ((uint32_t)buf[4 * j + 3] << 24);
        Fr::from_uniform_words(w).to_bytes(&out[32 * i]);
    }
    fclose(f);
    return 0;
}

// A call made from a stage it does not accept: every call accepts the stages from `least` on
int require_stage(const h2v_batch* b, BatchStage least, const char* who) {
    if (b && b->stage >= least) return 0;
    static const char* const missing[] = {"", "nothing uploaded since the last failed call or set_groups", "nothing launched", "no finished launch"};
    set_last_error(std::string(who) + ": " + (b ? missing[(int)least] : "null argument"));
    return H2V_ERR_BAD_ARGUMENT;
}

// The stage an operation leaves: Empty on every way out but its last step, commit(its stage of success).  (b may be null.)
struct StageCommit {
    h2v_batch* b;
    ~StageCommit() { if (b) { b->stage = BatchStage::Empty; b->hinted = false; } }   // (an empty batch has no upload, so no hints)
    void commit(BatchStage st) { b->stage = st; b = nullptr; }
};

#define H2V_SPLIT_MAX_GROUPS 64u

// the left channel is one term per proof, in the same slot of every proof (SHPLONK's h2): a strided problem, its other slots never read
static bool left_strided(const Plan& pl) { return pl.left_term_order.size() == 1 && !pl.left_term_order[0].first; }
// The two MSM problems of the proofs [p0, p0 + count) of an uploaded batch: acc2[0] <- the left channel (SHPLONK: sum_p m_p * h2_p;
// GWC: the witness points), acc2[1] <- the right channel = the proofs' pooled Guard terms + the VK-wide bases with the n_shared
// folded scalars `shared_scal`.  Both index the batch's point array; unused slots have zero scalars and cost nothing.
// the term counts of those two problems: the one rule, for channel_problems and for whoever must know a launch's layout before it is built
ChannelTerms channel_terms(const Plan& pl, uint32_t count, uint32_t n_shared) {
    const bool strided = left_strided(pl);
    return ChannelTerms{strided, strided ? count : count * pl.n_points, count * pl.n_points + n_shared};
}
bool groups_cut_within_limit(const Plan& pl, const size_t* sizes, size_t n_groups) {
    std::vector<uint32_t> terms;
    for (size_t g = 0; g < n_groups; ++g) { const ChannelTerms t = channel_terms(pl, (uint32_t)sizes[g], pl.n_shared); terms.push_back(t.left); terms.push_back(t.right); }
    return msm_cuts_within_limit(terms.data(), terms.size());
}
void channel_problems(MsmProblems& pr, const h2v_batch* b, const Plan& pl, size_t p0, uint32_t count, G1J* acc2, const uint32_t* shared_scal, uint32_t n_shared) {
    const uint32_t np = pl.n_points;
    const size_t first = p0 * np;
    const ChannelTerms terms = channel_terms(pl, count, n_shared);
    if (terms.strided) {
        // SHPLONK: one left term per proof (its h2): the problem is that slot of every proof — a strided view of `count` terms, not the
        // count * np slots with `count` of them non-zero (msm_glv_prep wrote twelve zero words for each of the other slots)
        const size_t at = first + pl.left_term_order[0].second;
        pr.p.push_back(MsmProblem(b->left_scal.p + at * 8, b->pts.p + at, acc2, 8 * np, np, terms.left));
        pr.p.back().phi = b->phi.p + at;
    } else {
        pr.p.push_back(MsmProblem(b->left_scal.p + first * 8, b->pts.p + first, acc2, 8, 1, terms.left));
        pr.p.back().phi = b->phi.p + first;
        pr.p.back().nnz = count * (uint32_t)pl.left_term_order.size();   // the program writes only these slots, the rest stay zero
    }
    pr.p.push_back(MsmProblem(b->msm_scal.p + first * 8, b->pts.p + first, acc2 + 1, 8, 1, terms.right - n_shared, shared_scal, b->pts.p + (size_t)b->n * np, n_shared));
    pr.p.back().phi = b->phi.p + first; pr.p.back().phi2 = b->phi.p + (size_t)b->n * np;
}

// The streams of a batch exist from their first use on: a batch whose caller binds a stream (h2v_batch_set_stream) never creates one of
// its own, and the auxiliary stream is made by the first launch whose tail needs it.  (The runtime gives every stream of the process one
// of a few in-order hardware queues, and the kernels of all streams on a queue run one after another: with a second and a third stream
// per batch, seven of eight launches in flight shared one queue — profiles/r04_queue_gaps.txt)
int need_stream(h2v_batch* b) {
    if (b->stream || !b->owns_stream) return 0;   // (a caller's stream may be the null stream)
    H2V_HIP_CHECK(hipSetDevice(b->ctx->device));
    H2V_HIP_CHECK(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    return 0;
}
int need_aux(h2v_batch* b) {
    if (b->aux) return 0;
    H2V_HIP_CHECK(hipStreamCreateWithFlags(&b->aux, hipStreamNonBlocking));
    H2V_HIP_CHECK(hipEventCreateWithFlags(&b->ev_fork, hipEventDisableTiming));
    H2V_HIP_CHECK(hipEventCreateWithFlags(&b->ev_join, hipEventDisableTiming));
    return 0;
}

// The end of a launch: the pairing checks and the conversion of the accumulators to affine bytes only READ the accumulators, and
// both are latency chains on a few waves (0.5 ms and 0.35 ms) — they run side by side.  A launch that left its accumulators in pieces
// (every launch of at most 64 groups) does both in ONE kernel launch on its own stream: the checks' workgroups first, then the
// workgroups that put the whole points together, convert them and send the result block to the host (PairTail, pairing.hip).  The
// launch then lives on one stream from its first kernel to its last: with more streams in flight than hardware queues, every
// event that forks to or joins a second stream is a barrier packet in a queue that other launches' kernels sit in as well.
// Otherwise (whole accumulators, the one-stream pairing table) the conversion and the copy of the result block run on the batch's
// auxiliary stream, which is NOT joined back into the main one (its last event, ev_join, is what join_tail makes the main stream
// wait for if anything but h2v_batch_finish comes next).
int close_enqueue(h2v_batch* b, bool with_pairing) {
    hipStream_t s = b->stream;
    const uint32_t G = b->groups;
    int rc;
    b->last.pairing = with_pairing; b->last.pieces = false; b->last.host_block = false;
    if (!with_pairing) {
        if (b->split.parts) { b->last.pieces = true; return 0; }   // pieces only for now
        return point_to_bytes_enqueue(s, b->acc.p, b->out_bytes, b->out_ident, 2 * G);
    }
    const ResultsLayout L{G, b->n};
    const ResultsPtrs host = results_at(b->results_host.dev, L);   // (the mapped host block, as the device sees it)
    const bool one_stream = b->ctx->tuning.pairing_one_stream != 0;
    if (b->split.parts && pairing_tail_fits(b->ctx->pairing, one_stream)) {
        // (the verdicts are still the last thing the launch writes: the tail's workgroups are done long before the checks')
        PairTail t;
        t.pieces = b->split.pts; t.prs = b->ws.final_problems; t.count = b->split.count; t.parts = b->split.parts; t.shift = b->split.shift;
        t.out_bytes = b->out_bytes; t.out_ident = b->out_ident;
        t.host_bytes = host.out_bytes; t.host_ident = host.out_ident;
        t.src = b->fold_failed; t.dst = host.fold_failed;
        t.n_words = (uint32_t)((L.total() - L.fold_failed()) / 4);
        t.skip_lo = (uint32_t)((L.out_ident() - L.fold_failed()) / 4); t.skip_hi = (uint32_t)((L.status() - L.fold_failed()) / 4);   // (the converting workgroups write those)
        if (t.count != 2 * G) { set_last_error("close_enqueue: the pieces are not this launch's"); return H2V_ERR_BAD_ARGUMENT; }
        b->last.host_block = true;
        return pairing_check_split_enqueue(s, b->ctx->pairing, b->split.ready, G, b->split.parts, b->split.shift, b->line_ws.p, b->ok, false, &t);
    }
    if ((rc = need_aux(b))) return rc;
    H2V_HIP_CHECK(hipEventRecord(b->ev_fork, s));
    H2V_HIP_CHECK(hipStreamWaitEvent(b->aux, b->ev_fork, 0));
    // (beside the pairing: kept off the pairing workgroups' CUs by an LDS request, internal.h)
    if (b->split.parts && (rc = msm_combine_enqueue(b->aux, b->ws, b->split, H2V_AUX_LDS_RESERVE))) return rc;   // acc <- the whole points
    if ((rc = point_to_bytes_enqueue(b->aux, b->acc.p, b->out_bytes, b->out_ident, 2 * G, H2V_AUX_LDS_RESERVE))) return rc;
    // the result block (all but the verdicts, which the pairing kernel writes to the host itself) goes back on the auxiliary stream too, and the
    // main stream does NOT wait for it: its last operation is the pairing kernel.  h2v_batch_finish waits for both streams; anything else
    // that touches the batch first calls join_tail.
    // (by a kernel, not hipMemcpyAsync: a copy enqueued now, behind kernels that end a launch later, can hold up an SDMA queue — util.hip)
    if ((rc = copy_words_enqueue(b->aux, b->fold_failed, host.fold_failed, (L.total() - L.fold_failed()) / 4, H2V_AUX_LDS_RESERVE))) return rc;
    H2V_HIP_CHECK(hipEventRecord(b->ev_join, b->aux));
    b->last.tail_on_aux = true; b->last.host_block = true;
    if (b->split.parts) { if ((rc = pairing_check_split_enqueue(s, b->ctx->pairing, b->split.ready, G, b->split.parts, b->split.shift, b->line_ws.p, b->ok, one_stream))) return rc; }
    else if ((rc = pairing_check_enqueue(s, b->ctx->pairing, b->acc.p, G, b->ok))) return rc;
    return 0;
}
// the main stream waits for what the last launch left on the auxiliary stream (before anything new reads or overwrites it)
int join_tail(h2v_batch* b) {
    // (a feed enqueued on an accumulator's stream may still read what the next call overwrites: h2v_accumulator_feed_batch)
    if (b->read_pending) { b->read_pending = false; H2V_HIP_CHECK(hipStreamWaitEvent(b->stream, b->ev_read, 0)); }
    if (!b->last.tail_on_aux) return 0;
    b->last.tail_on_aux = false;
    H2V_HIP_CHECK(hipStreamWaitEvent(b->stream, b->ev_join, 0));
    return 0;
}
// the whole accumulators (acc) and their affine bytes, if the last launch left pieces only
int ensure_whole(h2v_batch* b) {
    if (!b->last.pieces) return 0;
    int rc;
    if ((rc = msm_combine_enqueue(b->stream, b->ws, b->split))) return rc;
    if ((rc = point_to_bytes_enqueue(b->stream, b->acc.p, b->out_bytes, b->out_ident, 2 * b->groups))) return rc;
    b->last.pieces = false;
    return 0;
}

// The draws of a call: the caller's `rand32` (n scalars, refused unless canonical) or, when it is null, n OS draws kept in `storage`.
// `nonzero`: a zero draw of the caller's is refused and an OS draw of zero is drawn again.
int resolve_draws(const uint8_t*& rand32, size_t n, std::vector<uint8_t>& storage, const char* who, bool nonzero) {
    int rc;
    std::vector<uint8_t> one;
    if (!rand32) {
        if ((rc = os_random_scalars(storage, n))) return rc;
        for (size_t i = 0; nonzero && i < n; ++i)   // (an OS draw of zero: probability 2^-254)
            while (scalar_is_zero(&storage[32 * i])) { if ((rc = os_random_scalars(one, 1))) return rc; memcpy(&storage[32 * i], one.data(), 32); }
        rand32 = storage.data();
        return 0;
    }
    for (size_t i = 0; i < n; ++i) {
        if (nonzero && scalar_is_zero(rand32 + 32 * i)) { set_last_error(std::string(who) + ": a draw in rand32 is zero"); return H2V_ERR_BAD_ARGUMENT; }
        if (!scalar_is_canonical(rand32 + 32 * i)) { set_last_error(std::string(who) + ": rand32 scalar not canonical"); return H2V_ERR_BAD_ARGUMENT; }
    }
    return 0;
}

// what the decompression and transcript stages work on: the batch's upload (its plan and n) and its buffers
static StageArgs stage_args(const h2v_batch* b) {
    StageArgs g{b->n, &b->plan->host, b->plan, b->proofs.p, b->inst.p, b->pts.p, b->phi.p, b->ycanon.p, b->status, b->words.p, b->stream_words, b->chal.p};
    // (h2v_batch_set_hints: the hints wait where the canonical y will lie; the miss list and its counter: hints_stage)
    if (b->hinted) { g.hint_misses = b->hint_misses.p; g.hints = b->ycanon.p; g.miss_list = b->miss_list.p; g.miss_list_count = b->hint_misses.p + 1; }
    return g;
}

// ---- An upload, whatever its source: host bytes (upload_impl) or device memory (h2v_batch_upload_device).  Every step the sources share
// exists once — upload_pin, upload_size_checks, upload_take, shared_bases_enqueue, upload_commit — and an entry point adds its own
// checks between the first two and after the second, and its own transfer between upload_take and upload_commit.

// What the sources share of their arguments.  proofs / instances: host or device memory; tail: the caller's draws, or null for OS draws
struct UploadArgs {
    const char* who; size_t n;  // the entry point, in the error messages; the proofs
    const void* proofs; const void* instances;
    size_t ncols; const size_t* col_lens;
    const void* tail; size_t n_tail;
};

// The checks that need no plan, then the plan of the instance shape -> pin.  columns_code: what a wrong column count returns, the
// reference's own refusal H2V_ERR_INVALID_INSTANCES (lib.rs:51-55, in pack_inputs' words) or the entry point's H2V_ERR_BAD_ARGUMENT.
static int upload_pin(const h2v_batch* b, const UploadArgs& a, int columns_code, bool guard, PlanPin& pin) {
    const std::string w(a.who);
    if (!b || (a.n && !a.proofs) || (a.ncols && !a.col_lens)) { set_last_error(w + ": null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if (a.n > b->max_proofs) { set_last_error(w + ": n exceeds the batch capacity"); return H2V_ERR_BAD_ARGUMENT; }
    h2v_ctx* ctx = b->ctx;
    H2V_HIP_CHECK(hipSetDevice(ctx->device));
    if (!ctx->vk) { set_last_error("the context was created without a VerifyingKey"); return H2V_ERR_BAD_ARGUMENT; }
    if (a.ncols != ctx_total_instance_columns(ctx)) {
        set_last_error((columns_code == H2V_ERR_INVALID_INSTANCES ? std::string() : w + ": ") + "instances do not match the VK's instance column count");
        return columns_code;
    }
    pin.ctx = ctx;   // (b may be null: the pin learns its context here)
    return pin.get(std::vector<size_t>(a.col_lens, a.col_lens + a.ncols), guard);
}

// The checks of an upload on its sizes alone, for the plan `pl` of its instance shape: instances where the plan has instance values, the
// proofs and draws against the batch's groups (GroupShape::misfit), and the launch's MSM cut.
static int upload_size_checks(const h2v_batch* b, const Plan& pl, const UploadArgs& a) {
    const std::string w(a.who);
    const bool have_tail = a.tail != nullptr;
    if (pl.n_instance_values && a.n && !a.instances) { set_last_error(w + ": instances missing"); return H2V_ERR_BAD_ARGUMENT; }
    const GroupShape shape = group_shape_of(b, a.n, have_tail ? a.n_tail : a.n, b->group_off.data());
    if (const char* why = shape.misfit(a.n, a.n_tail, have_tail)) { set_last_error(w + ": " + why); return H2V_ERR_BAD_ARGUMENT; }
    if (shape.off) {
        // the MSM cuts problems too large for its per-window sort into sub-problems, at most MSM_MAX_PROBLEMS per launch; equal groups that miss
        // the limit all run uncut, a form that unequal groups have never taken: refused before any device work
        std::vector<size_t> sizes(shape.G);
        for (uint32_t g = 0; g < shape.G; ++g) sizes[g] = shape.count(g);
        if (!b->ctx->tuning.msm_no_term_split && !groups_cut_within_limit(pl, sizes.data(), sizes.size())) {
            set_last_error(w + ": the groups' MSM problems, cut into sub-problems of at most 16384 terms, exceed the launch's problem limit");
            return H2V_ERR_UNSUPPORTED;
        }
    }
    return 0;
}
// a zero draw zeroes the multipliers of every earlier proof of its group: h2v_batch_recheck refuses ranges over those proofs.
// (k_ingest_draws runs the body of this loop, a thread per draw, for draws in device memory.)
static void zero_below_of_draws(h2v_batch* b, const uint8_t* rand_tail) {
    b->zero_below.assign(b->groups, 0);
    const GroupShape shape = group_shape(b);
    for (uint32_t i = 0; i < b->n_tail; ++i)
        if (scalar_is_zero(rand_tail + 32 * (size_t)i)) {
            const GroupShape::Draw d = shape.draw_at(i);
            b->zero_below[d.g] = std::max(b->zero_below[d.g], shape.zero_below(d.j, d.g));
        }
}

// Every argument is valid: from here on the batch takes the upload of n proofs under the pinned plan, with n_tail draws: host_draws,
// or (device_draws) the caller's draws in device memory, which the host cannot see and k_ingest_draws checks into the verdict block.
static int upload_take(h2v_batch* b, PlanPin& pin, size_t n, size_t n_tail, const uint8_t* host_draws, bool device_draws) {
    int rc;
    if ((rc = need_stream(b)) || (rc = join_tail(b))) return rc;
    if (b->read_unseen) {
        // an enqueued feed may still read acc, mult, the status words, tail and ingest_verdict on an accumulator's stream: the batch's
        // stream waits for it on the device (join_tail), but an array that this upload would free is waited for by the host
        const BatchSizes z = batch_sizes(pin.pd->host, b->max_proofs, b->groups, 1);
        auto grows = [](const auto& buf, size_t count) { return !buf.p || count > buf.cap; };
        if (grows(b->acc, z.acc) || grows(b->mult, z.mult) || grows(b->results, z.results) || grows(b->tail, 32 * n_tail) ||
            (device_draws && grows(b->ingest_verdict, (size_t)b->groups + 2))) {
            b->read_unseen = false;
            H2V_HIP_CHECK(hipEventSynchronize(b->ev_read));
        }
    }
    if ((rc = ensure_buffers(b, pin.pd->host))) return rc;
    if (b->plan) ctx_put_plan(b->ctx, b->plan);   // the batch holds its plan from upload to the next upload (or its destruction)
    b->plan = pin.take(); b->n = (uint32_t)n; b->n_tail = (uint32_t)n_tail;
    const size_t G = b->groups;
    if (device_draws) b->zero_below.assign(G, 0);   // (filled by h2v_batch_finish from the verdict block)
    else zero_below_of_draws(b, host_draws);
    if ((rc = b->tail.reserve(32 * n_tail))) return rc;
    if (device_draws && ((rc = b->ingest_verdict.reserve(G + 2)) || (rc = b->ingest_host.reserve(4 * (G + 1))))) return rc;
    if ((rc = b->mult_scratch.reserve(multipliers_scratch(group_shape(b))))) return rc;   // (d_group_off and d_group_last are on the device since h2v_batch_set_group_sizes)
    b->mult_of_draws = false; b->decompressed = false; b->device_draws = device_draws;
    b->hinted = false;   // (hints belong to one upload)
    return 0;
}
// VK-wide bases sit behind the batch's own points so that one MSM covers both (and their phi images behind the points' images)
static int shared_bases_enqueue(h2v_batch* b, hipStream_t cs) {
    const PlanDevice* pd = b->plan;
    const Plan& pl = pd->host;
    if (!b->n) return 0;
    H2V_HIP_CHECK(hipMemcpyAsync(b->pts.p + b->n * (size_t)pl.n_points, pd->shared_bases.p, sizeof(G1A) * pl.n_shared, hipMemcpyDeviceToDevice, cs));
    H2V_HIP_CHECK(hipMemcpyAsync(b->phi.p + b->n * (size_t)pl.n_points, pd->shared_phi.p, sizeof(G1A) * pl.n_shared, hipMemcpyDeviceToDevice, cs));
    return 0;
}
// The end of an upload, its draws on the device: the batch multipliers depend on the draws alone, so they are computed once per upload
// and kept by every launch of it
static int upload_commit(h2v_batch* b, StageCommit& commit) {
    if (b->n) { if (int rc = multipliers_enqueue(b->stream, group_shape_device(b), b->tail.p, b->d_group_last.p, b->mult.p, b->mult_scratch.p)) return rc; b->mult_of_draws = true; }
    commit.commit(BatchStage::Uploaded);
    return 0;
}

// `overlap`: where it pays (see `points_first` below), the point bytes are copied first on the batch's copy stream and the decompression
// runs under the copy of everything else (h2v_batch_upload_launch); otherwise everything is copied on the batch's stream (h2v_batch_upload).
// `guard`: the guard variant of the plan (h2v_guard_msm)
int upload_impl(h2v_batch* b, size_t n, const uint8_t* proofs_flat, size_t proof_len, const uint8_t* instances_flat, size_t ncols, const size_t* col_lens,
                const uint8_t* rand_tail, size_t n_tail, bool overlap, bool guard) {
    const UploadArgs a{"h2v_batch_upload", n, proofs_flat, instances_flat, ncols, col_lens, rand_tail, n_tail};
    StageCommit commit{b};
    PlanPin pin(nullptr);
    int rc;
    if ((rc = upload_pin(b, a, H2V_ERR_INVALID_INSTANCES, guard, pin))) return rc;
    const Plan& pl = pin.pd->host;
    if (proof_len < pl.proof_len) { set_last_error("h2v_batch_upload: proof_len is shorter than this VK's proof"); return H2V_ERR_BAD_ARGUMENT; }
    if ((rc = upload_size_checks(b, pl, a))) return rc;
    std::vector<uint8_t> os_rand;
    if (!rand_tail) n_tail = n;
    if ((rc = resolve_draws(rand_tail, n_tail, os_rand, a.who))) return rc;
    if ((rc = upload_take(b, pin, n, n_tail, rand_tail, false))) return rc;
    hipStream_t s = b->stream;
    auto copy_proofs = [&](hipStream_t cs, size_t p0, size_t p1) -> int {
        if (proof_len == pl.proof_len) H2V_HIP_CHECK(hipMemcpyAsync(b->proofs.p + p0 * pl.proof_len, proofs_flat + p0 * proof_len, (p1 - p0) * proof_len, hipMemcpyHostToDevice, cs));
        else H2V_HIP_CHECK(hipMemcpy2DAsync(b->proofs.p + p0 * pl.proof_len, pl.proof_len, proofs_flat + p0 * proof_len, proof_len, pl.proof_len, p1 - p0, hipMemcpyHostToDevice, cs));
        return 0;
    };
    auto copy_rest = [&](hipStream_t cs) -> int {
        if (pl.n_instance_values) H2V_HIP_CHECK(hipMemcpyAsync(b->inst.p, instances_flat, n * (size_t)pl.n_instance_values * 32, hipMemcpyHostToDevice, cs));
        H2V_HIP_CHECK(hipMemcpyAsync(b->tail.p, rand_tail, 32 * n_tail, hipMemcpyHostToDevice, cs));
        return shared_bases_enqueue(b, cs);   // (the offsets and marks of unequal groups are on the device since h2v_batch_set_group_sizes)
    };
    // Overlapped form (h2v_batch_upload_launch).  What was measured on the way (profiles/r03_h2d_microbench.txt, r03_upload_timeline.txt):
    //  * a 26 MB copy takes 0.47 ms from pageable and from pinned memory alike, and an "asynchronous" copy out of pageable memory
    //    returns only when the data is on the device — the calling thread is the one thing it blocks;
    //  * chunks on a second stream with an event per chunk for the kernels to wait on: erratic (0.64 ms best, 1.8 ms mean for eight
    //    chunks) — cross-stream event waits set the pace, slower than one blocking copy;
    //  * decompression in chunks, each enqueued when its chunk has arrived: point decompression is ONE round of ~0.5 ms of dependent
    //    work per lane whatever the launch size, so eight chunk launches are eight rounds (4.2 ms per launch instead of 3.6);
    //  * a decompression kernel reading the caller's registered buffer over the link: 0.82 ms instead of 0.60; a gather kernel for
    //    the point bytes alone: 0.23 ms — and hipHostUnregister waits for EVERY kernel in flight on the device (3.0 ms behind a 3 ms
    //    kernel, tools/unregister_probe.hip), so a registration cannot be dropped before the launch it helped has finished.
    // What is left: the decompression needs only the POINT bytes of a proof (12 x 32 of 1024 bytes for the headline VK), and those lie in
    // a few runs at fixed offsets.  The thread copies the point runs first (strided copies, a third of the bytes), enqueues the ONE
    // decompression launch — when the blocking copy has returned the bytes are in device memory, so no event is needed — and copies
    // everything (whole proofs, instances, draws) while the GPU decompresses; the later stages are enqueued after that copy returned.
    std::vector<std::pair<uint32_t, uint32_t>> runs;   // (offset, length) of the maximal runs of point bytes inside a proof
    {
        std::vector<uint32_t> offs(pl.point_offsets);
        std::sort(offs.begin(), offs.end());
        for (uint32_t o : offs) { if (!runs.empty() && runs.back().first + runs.back().second == o) runs.back().second += 32; else runs.push_back({o, 32u}); }
    }
    size_t point_bytes = 0;
    for (auto& r : runs) point_bytes += r.second;
    // (one launch + finish, best of 15, tools/h2d_probe.py: resident 2.98 ms, points-first 3.29, plain 3.47.  A third form — the proofs
    //  in two halves, each decompressed as soon as it had arrived, the second copy behind the first half's round — was measured and
    //  removed: 3.33 ms there, and in the benchmark's loop, PCIe-inclusive over resident, 0.885 against 0.905 for points-first and
    //  0.835 for plain: 5.90 against 6.05 and 5.50 M proofs/s with re-upload, profiles/r03_variants_ab.txt.)
    const bool points_first = overlap && n >= 2048 &&                                  // a copy of a megabyte or two is not worth two launches
                              runs.size() <= 4 && 2 * point_bytes <= pl.proof_len;    // points all over the proof, or most of it: nothing to gain
    if (!points_first) {
        if (n && ((rc = copy_proofs(s, 0, n)) || (rc = copy_rest(s)))) return rc;
        H2V_HIP_CHECK(hipStreamSynchronize(s));  // the host buffers are the caller's again
    } else {
        if (!b->copy) H2V_HIP_CHECK(hipStreamCreateWithFlags(&b->copy, hipStreamNonBlocking));
        H2V_HIP_CHECK(hipStreamSynchronize(s));   // an earlier launch of this batch may still read the buffers (normally long finished: h2v_batch_finish)
        const StageArgs g = stage_args(b);
        for (auto& r : runs) H2V_HIP_CHECK(hipMemcpy2DAsync(b->proofs.p + r.first, pl.proof_len, proofs_flat + r.first, proof_len, r.second, n, hipMemcpyHostToDevice, b->copy));
        H2V_HIP_CHECK(hipStreamSynchronize(b->copy));
        if ((rc = decompress_begin_enqueue(s, g))) return rc;
        if ((rc = decompress_range_enqueue(s, g, 0, (uint32_t)n))) return rc;
        // (the whole proofs again, point bytes included: identical bytes over the ones the kernel is reading)
        if ((rc = copy_proofs(b->copy, 0, n)) || (rc = copy_rest(b->copy))) return rc;
        H2V_HIP_CHECK(hipStreamSynchronize(b->copy));   // everything is on the device; the host buffers are the caller's again
        if ((rc = decompress_finish_enqueue(s, g))) return rc;
    }
    b->decompressed = points_first;
    return upload_commit(b, commit);
}

// `bytes` bytes from `p` on are device memory of `device`, inside one allocation, and p lies on a 16-byte boundary
// (who / does: the entry point and the verb of the error message)
int device_range_check(const void* p, size_t bytes, int device, const char* what, const char* who, const char* does) {
    const std::string w = std::string(who) + ": " + what;
    if ((uintptr_t)p & 15u) { set_last_error(w + " is not 16-byte aligned"); return H2V_ERR_BAD_ARGUMENT; }
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); set_last_error(w + " is not device memory"); return H2V_ERR_BAD_ARGUMENT; }   // (a plain host address)
    if (at.type != hipMemoryTypeDevice || at.device != device) { set_last_error(w + " is not device memory of the context's device"); return H2V_ERR_BAD_ARGUMENT; }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); set_last_error(w + ": no allocation holds the address"); return H2V_ERR_BAD_ARGUMENT; }
    const uintptr_t lo = (uintptr_t)base, at_p = (uintptr_t)p;
    if (at_p < lo || at_p - lo > size || bytes > size - (at_p - lo)) { set_last_error(w + ": the bytes the call " + does + " end past the pointer's allocation"); return H2V_ERR_BAD_ARGUMENT; }
    return 0;
}


// ext_mult / ext_idx: the multipliers of a non-contiguous subset of a larger accumulation (h2v_verify_batch_shapes), instead of the draws'
int launch_impl(h2v_batch* b, int with_pairing, const Fr* ext_mult, const uint32_t* ext_idx) {
    int rc;
    if ((rc = require_stage(b, BatchStage::Uploaded, "h2v_batch_launch"))) return rc;
    StageCommit commit{b};
    h2v_ctx* ctx = b->ctx;
    H2V_HIP_CHECK(hipSetDevice(ctx->device));
    PlanDevice* pd = b->plan;
    const Plan& pl = pd->host;
    hipStream_t s = b->stream;
    uint32_t n = b->n;
    const uint32_t G = b->groups;
    const GroupShape host_shape = group_shape(b), shape = group_shape_device(b);   // for this function's own loops; for the kernels
    if ((rc = join_tail(b))) return rc;
    int ev = 0;
    auto mark = [&]() { if (b->profiling >= 2) hipEventRecord(b->ev[ev], s); ++ev; };   // (an event record is a barrier packet: ~6 us of idle stream each)
    mark();
    const StageArgs g = stage_args(b);
    // stage 1: point decompression + canonicity checks (already on the stream, behind its chunked upload, after h2v_batch_upload_launch);
    // stage 2: absorbed stream, Blake2b challenges.  Everything is enqueued on the batch's one stream: the scalar canonicity check reads a
    // word per scalar, the multipliers are the upload's, the MSM's problem descriptors stay on the device from launch to launch
    const bool run_decompress = !(b->stage == BatchStage::Uploaded && b->decompressed);   // (a relaunch of the same upload runs it again)
    // cleared per launch: fold_failed (set by h2v_batch_fold_check_enqueue only) and — unless the upload already did (h2v_batch_upload_launch) —
    // the status words.  The results block is [ok][fold_failed][out_ident][out_bytes][status]: one fill from fold_failed to the last status word
    // (the output bytes in between are written later in the launch) instead of two
    const ResultsLayout L{G, n};
    if (run_decompress && n) H2V_HIP_CHECK(hipMemsetAsync(b->fold_failed, 0, L.total() - L.fold_failed(), s));
    else H2V_HIP_CHECK(hipMemsetAsync(b->fold_failed, 0, 4 * (size_t)G, s));   // (its G words)
    const bool hinted = run_decompress && n && g.hints;   // (a launch without hints enqueues nothing new)
    if (hinted) H2V_HIP_CHECK(hipMemsetAsync(b->hint_misses.p, 0, sizeof(uint32_t), s));
    if (run_decompress && n && ((rc = decompress_finish_enqueue(s, g)) || (rc = decompress_range_enqueue(s, g, 0, n)))) return rc;   // k_check_scalars, k_decompress (with hints: k_decompress_hinted)
    mark();
    if ((rc = transcript_stage_enqueue(s, g))) return rc;
    // both channels of every group in one set of launches: [2g] left, [2g+1] right (channel_problems), the group's folded VK-wide
    // scalars at the tail of msm_scal.  The descriptors are addresses and sizes: msm_enqueue_multi sends them only when they differ from the workspace's.
    MsmProblems pr;
    for (uint32_t g = 0; g < G; ++g)
        channel_problems(pr, b, pl, host_shape.first(g), host_shape.count(g), b->acc.p + 2 * g, b->msm_scal.p + ((size_t)n * pl.n_points + (size_t)g * pl.n_shared) * 8, n ? pl.n_shared : 0);
    b->ws.tune = ctx->tuning;
    if (n) {
        // gathered multipliers replace the upload's; a launch on the draws after one on gathered multipliers computes the upload's again
        if (ext_mult) { b->mult_of_draws = false; if ((rc = gather_multipliers_enqueue(s, ext_mult, ext_idx, n, b->mult.p))) return rc; }
        else if (!b->mult_of_draws) { if ((rc = multipliers_enqueue(s, shape, b->tail.p, b->d_group_last.p, b->mult.p, b->mult_scratch.p))) return rc; b->mult_of_draws = true; }
        // the program writes only the slots the left channel uses; with ONE left term per proof the MSM reads exactly those (the strided problem above)
        if (!left_strided(pl)) H2V_HIP_CHECK(hipMemsetAsync(b->left_scal.p, 0, (size_t)n * pl.n_points * 32, s));
    }
    mark();
    FrvmArgs a{pd->code.p, (uint32_t)pl.code.size(), pd->consts.p, b->slots.p, n, b->proofs.p, pl.proof_len, pd->scalar_offsets.p, b->inst.p, pl.n_instance_values,
               b->chal.p, b->mult.p, b->status, b->msm_scal.p, pl.n_points, b->shared.p, b->left_scal.p, b->insteval.p, b->guard_scal.p, (uint32_t)pl.guard_term_order.size()};
    if (n && pl.wide_instances) {
        Fr step = pl.omega;
        for (int i = 0; i < 8; ++i) step = step.sqr();   // omega^256: a thread's stride through the column
        const Fr step_inv = step.inv();
        for (size_t q = 0; q < pl.inst_queries.size(); ++q) {
            InstEvalArgs ia{b->inst.p, pl.n_instance_values, b->chal.p, pl.x_chal, n, pl.domain_k, pl.inst_queries[q].base, pl.inst_queries[q].len,
                            pl.inst_queries[q].w_start, pl.omega, step, step_inv, pl.n_inv, b->insteval.p + q * (size_t)n, b->status};
            if ((rc = instance_eval_enqueue(s, ia))) return rc;
        }
    }
    a.force_streams = ctx->tuning.frvm_streams; a.force_lds_kb = ctx->tuning.frvm_lds_kb;
    for (int k = 0; k < 3; ++k) { for (int q = 0; q < k + 2; ++q) { a.code_k[k][q] = pd->code_k[k][q].p; a.n_code_k[k][q] = (uint32_t)pl.code_k[k][q].size(); } a.n_slots_k[k] = pl.n_slots_k[k]; }
    if ((rc = frvm_enqueue(s, a, pl.n_slots))) return rc;
    mark();
    if (n && (rc = fold_shared_enqueue(s, shape, b->shared.p, n, pl.n_points, pl.n_shared, b->msm_scal.p))) return rc;
    mark();
    {
        b->ws.profile = b->profiling >= 1; b->ws.profile_recorded = false;
        // A launch leaves the accumulators in pieces (MsmSplit): its own pairing checks take the pieces and the whole points are put
        // together beside them (close_enqueue); a launch without a pairing (a shard) exports the pieces, the folded pairing takes them,
        // and the whole points are only made if somebody reads them (ensure_whole).  Worth it while the launch is a latency chain, i.e. few groups.
        b->split = MsmSplit();
        const uint32_t parts_knob = ctx->tuning.msm_parts > 0 ? (uint32_t)ctx->tuning.msm_parts : MSM_MAX_PARTS;   // h2v_tuning.msm_parts
        b->ws.tune = ctx->tuning;
        if (n && G <= H2V_SPLIT_MAX_GROUPS && parts_knob > 1) {
            const size_t line_bytes = (size_t)G * H2V_PAIRING_LINE_WS_BYTES;
            if (b->line_ws.p && line_bytes > b->line_ws.cap) H2V_HIP_CHECK(hipStreamSynchronize(s));   // (an earlier launch's pairing may still read it)
            if ((rc = b->line_ws.reserve(line_bytes))) return rc;
            b->split.want_parts = parts_knob;
        }
        if ((rc = msm_enqueue_multi(s, b->ws, pr, b->split.want_parts > 1 ? &b->split : nullptr))) return rc;
    }
    mark();
    if ((rc = close_enqueue(b, with_pairing != 0))) return rc;
    b->last.folded = false;
    b->launch_hinted = hinted; b->launch_null_rows = hinted ? b->null_rows : 0;
    if (hinted) b->null_rows = 0;   // (a relaunch of this upload finds the canonical y of ALL its points where the rows lay: every point hinted)
    mark();
    commit.commit(BatchStage::Launched);
    return 0;
}

// the batch's accumulator records as whole points.  For a record in pieces, the one-pairing fold (fold_check_locked) puts the pieces
// together with ~254 dependent doublings per record, one record after another: 1.15 ms for two records at 1024 proofs each, where
// the batch's own msm_combine_parts takes 0.34 ms on its stream, beside the other batches of the call (h2v_verify_batch_keys).
int export_whole_records(h2v_batch* b, void* device_dst) {
    int rc;
    if ((rc = join_tail(b)) || (rc = ensure_whole(b))) return rc;
    return export_records_enqueue(b->stream, b->acc.p, nullptr, 1, 0, b->status, b->n, b->groups, device_dst);
}

// group_ok / out_left / out_right hold one entry (64 bytes) per group
int finish_impl(h2v_batch* b, const char* who, int* per_proof_status, int* group_ok, uint8_t* out_left, uint8_t* out_right) {
    if (int rc = require_stage(b, BatchStage::Launched, who)) return rc;
    StageCommit commit{b};
    H2V_HIP_CHECK(hipSetDevice(b->ctx->device));
    hipStream_t s = b->stream;
    const uint32_t n = b->n, G = b->groups;
    { int rcw = ensure_whole(b); if (rcw) return rcw; }
    const ResultsLayout L{G, n};
    const ResultsPtrs host = results_at(b->results_host.p, L);
    hipError_t e;
    if (b->last.host_block) {
        // a launch that ended in its own pairing checks: the block travels by the launch's own kernels (the pairing launch's tail workgroups,
        // or the auxiliary stream), the verdicts come from the pairing kernel
        e = hipStreamSynchronize(s);
        if (e == hipSuccess && b->last.tail_on_aux) e = hipStreamSynchronize(b->aux);
        b->last.tail_on_aux = false;   // (not hipEventSynchronize on its last event: that wait goes through the runtime's event thread, and a host that re-uploads per launch lost 40 % to it)
    } else {
        H2V_HIP_CHECK(hipMemcpyAsync(host.fold_failed, b->fold_failed, L.total() - L.fold_failed(), hipMemcpyDeviceToHost, s));
        e = hipStreamSynchronize(s);
    }
    if (e != hipSuccess) { set_last_error(std::string("h2v_batch_finish: ") + hipGetErrorString(e)); return H2V_ERR_DEVICE; }
    if (b->device_draws) {
        // the upload took its draws from device memory (h2v_batch_upload_device): k_ingest_draws' verdict, [fault][zero_below x G], has been
        // in the batch's pinned block since the upload's kernels ran.  A draw >= r: nothing is written and the batch is left Empty.
        const uint32_t* verdict = reinterpret_cast<const uint32_t*>(b->ingest_host.p);
        if (verdict[0] != 0xffffffffu) {
            set_last_error(std::string(who) + ": rand_tail scalar not canonical (draw " + std::to_string(verdict[0]) + " of the tail uploaded from device memory)");
            return H2V_ERR_BAD_ARGUMENT;
        }
        b->zero_below.assign(verdict + 1, verdict + 1 + G);
    }
    const int* st = host.status;
    for (int i = 0; i < 7; ++i) b->last_ms[i] = 0;
    // events: 0 start, 1 after decompression, 2 after transcript + multipliers, 3 after Fr program, 4 after fold, 5 after MSMs, 6 after pairing
    for (int i = 0; i < 6 && b->profiling >= 2; ++i)
        if (hipEventElapsedTime(&b->last_ms[i], b->ev[i], b->ev[i + 1]) != hipSuccess) b->last_ms[i] = 0;   // (a pair that was not recorded)
    if (b->profiling >= 1) {
        float tacc = 0;
        if (b->ws.profile_recorded) hipEventElapsedTime(&tacc, b->ws.ev_acc[0], b->ws.ev_acc[1]);
        b->last_ms[6] = tacc;
    }
    std::vector<char> all_ok(G, 1);
    // (the common case — no proof of the launch was rejected — is found by a word-wide scan: decoding 20 480 statuses one by one, with a
    // division each for the group, was 30 us of host time behind the GPU's last kernel)
    uint32_t any = 0;
    for (uint32_t i = 0; i < n; ++i) any |= (uint32_t)st[i];
    if (!any) { if (per_proof_status && n) memset(per_proof_status, 0, sizeof(int) * (size_t)n); }
    else for (uint32_t g = 0, i = 0; g < G; ++g) for (uint32_t k = 0, gs = group_shape(b).count(g); k < gs; ++k, ++i) {
        const int v = status_decode(st[i]);
        if (per_proof_status) per_proof_status[i] = v;
        if (v != 0) all_ok[g] = 0;
    }
    for (uint32_t g = 0; g < G; ++g) {
        // a sharded group is accepted only if no shard reported a failed proof (their terms are zeroed out of the accumulators)
        if (group_ok) group_ok[g] = (all_ok[g] && !host.fold_failed[g] && (!b->last.pairing || host.ok[g])) ? 1 : 0;
        if (out_left) memcpy(out_left + 64 * (size_t)g, &host.out_bytes[128 * (size_t)g], 64);
        if (out_right) memcpy(out_right + 64 * (size_t)g, &host.out_bytes[128 * (size_t)g + 64], 64);
    }
    commit.commit(BatchStage::Finished);
    return 0;
}
// the verdict of group g's own pairing check in the last finished launch (finish_impl folds the statuses into group_ok; this is the pairing alone)
bool pairing_passed(const h2v_batch* b, uint32_t g) {
    return b->last.pairing && results_at(b->results_host.p, ResultsLayout{b->groups, b->n}).ok[g] != 0;
}
hipError_t wait_for_streams(h2v_batch* b) {
    hipError_t first = hipSuccess;
    auto wait = [&](hipStream_t s) { const hipError_t e = hipStreamSynchronize(s); if (first == hipSuccess) first = e; };
    if (b->stream || !b->owns_stream) wait(b->stream);   // (a caller's stream may be the null stream)
    if (b->aux) wait(b->aux);                             // (the tail of the last launch may still be running there)
    if (b->copy) wait(b->copy);                           // (the last upload's copies)
    // (an accumulator's stream may still read the batch: an enqueued feed)
    if (b->read_unseen) { b->read_unseen = false; const hipError_t e = hipEventSynchronize(b->ev_read); if (first == hipSuccess) first = e; }
    return first;
}


bool same_srs(const ParamsHost& a, const ParamsHost& b) {
    auto same_g2 = [](const G2A& p, const G2A& q) { return p.inf == q.inf && !memcmp(&p.x, &q.x, sizeof(Fq2)) && !memcmp(&p.y, &q.y, sizeof(Fq2)); };
    return !memcmp(&a.g, &b.g, sizeof(G1A)) && same_g2(a.g2, b.g2) && same_g2(a.s_g2, b.s_g2);
}

// Range re-checks (h2v_batch_recheck, h2v_batches_recheck).  A range [first, first + count) of group g of a batch is checked as the
// launch checks the whole group: e(sum_p m_p L_p, s_g2) e(sum_p m_p R_p, -g2) = 1 over its proofs' resident scalars (already multiplied
// by m_p, zeroed for failed proofs) — the range's own fold of the VK-wide scalars, two MSMs, one pairing.  Nothing before the MSM runs
// again, and nothing the launches left (ws, acc, split, the result block) is touched: the re-check has its own workspace and outputs, the
// first batch's (batches[0]->recheck), and runs on that batch's stream.  The ranges of one set of launches may belong to different batches
// over the same SRS: the fold, the MSM problems and the pairing take addresses and sizes range by range, and one batch's pairing tables
// serve them all.  At most MSM_MAX_PROBLEMS / 2 ranges, and about the largest launch's own term count, go into one set of launches.
int recheck_impl(const char* who, h2v_batch* const* batches, size_t n_batches, size_t n_ranges, const uint32_t* batch_of_range, const size_t* first,
                 const size_t* count, int* range_ok, uint8_t* out_left, uint8_t* out_right) {
    const std::string w(who);
    int rc;
    // every argument check comes before the first HIP call and the first output
    if (!batches || !n_batches) { set_last_error(w + ": null argument"); return H2V_ERR_BAD_ARGUMENT; }
    for (size_t k = 0; k < n_batches; ++k) {
        if ((rc = require_stage(batches[k], BatchStage::Finished, who))) return rc;
        if (batches[k]->ctx->device != batches[0]->ctx->device) { set_last_error(w + ": batches on different devices"); return H2V_ERR_BAD_ARGUMENT; }
        if (!same_srs(batches[k]->ctx->params, batches[0]->ctx->params)) { set_last_error(w + ": batches over different params (g[0], g2 or s_g2 differ)"); return H2V_ERR_BAD_ARGUMENT; }
    }
    if (n_ranges && (!first || !count || !range_ok)) { set_last_error(w + ": null argument"); return H2V_ERR_BAD_ARGUMENT; }
    auto batch_of = [&](size_t i) -> h2v_batch* { return batches[batch_of_range ? batch_of_range[i] : 0]; };
    for (size_t i = 0; i < n_ranges; ++i) {
        if (batch_of_range && batch_of_range[i] >= n_batches) { set_last_error(w + ": batch index out of range"); return H2V_ERR_BAD_ARGUMENT; }
        const h2v_batch* b = batch_of(i);
        const size_t n = b->n;
        const size_t f = first[i], c = count[i];
        if (!c || f >= n || c > n - f) { set_last_error(w + ": empty range, or a range past the launch's proofs"); return H2V_ERR_BAD_ARGUMENT; }
        const GroupShape shape = group_shape(b);
        const uint32_t g = shape.of((uint32_t)f);
        // multipliers are products of the later draws of the proof's OWN group: the last proof of every group has multiplier 1, and a range
        // over two groups could hold two proofs with equal multipliers whose errors cancel
        if (shape.of((uint32_t)(f + c - 1)) != g) { set_last_error(w + ": a range crosses a group boundary of the launch"); return H2V_ERR_BAD_ARGUMENT; }
        if (f - shape.first(g) < b->zero_below[g]) { set_last_error(w + ": a range covers a proof whose multiplier is zero (a zero draw)"); return H2V_ERR_BAD_ARGUMENT; }
    }
    if (!n_ranges) return 0;
    h2v_batch* host = batches[0];
    h2v_ctx* ctx = host->ctx;
    H2V_HIP_CHECK(hipSetDevice(ctx->device));
    // the re-check runs on the first batch's stream behind what its last launch left; every other batch's streams are idle before it reads
    // their buffers (a finished batch's normally are: only a fold after the finish leaves work behind)
    if ((rc = join_tail(host))) return rc;
    for (size_t k = 1; k < n_batches; ++k)
        if (batches[k] != host) H2V_HIP_CHECK(wait_for_streams(batches[k]));
    hipStream_t s = host->stream;
    Recheck& rk = host->recheck;
    const uint32_t max_ranges = MSM_MAX_PROBLEMS / 2;
    // the plan facts of every range's batch, and the term budget of a set: about the largest launch's own
    auto plan_of = [&](size_t i) -> const Plan& { return batch_of(i)->plan->host; };
    auto terms_of = [&](size_t i) -> size_t { const Plan& pl = plan_of(i); const ChannelTerms t = channel_terms(pl, (uint32_t)count[i], pl.n_shared); return (size_t)t.left + t.right; };
    size_t budget = 0;   // > terms_of(every range): every range fits in a set of its own
    for (size_t k = 0; k < n_batches; ++k) { const Plan& pl = batches[k]->plan->host; budget = std::max(budget, 2 * ((size_t)batches[k]->n * pl.n_points + (size_t)max_ranges * pl.n_shared)); }
    if ((rc = rk.ranges.reserve(max_ranges)) || (rc = rk.acc.reserve(2 * (size_t)max_ranges)) || (rc = rk.ok.reserve(max_ranges)) ||
        (rc = rk.out_bytes.reserve(128 * (size_t)max_ranges)) || (rc = rk.out_ident.reserve(2 * (size_t)max_ranges))) return rc;
    std::vector<FoldRange> desc;
    std::vector<uint32_t> okv;
    std::vector<uint8_t> outb;
    for (size_t i0 = 0; i0 < n_ranges;) {
        size_t i1 = i0, total = 0;
        uint32_t per = 0, rows = 0, max_shared = 0;
        while (i1 < n_ranges && i1 - i0 < max_ranges && (i1 == i0 || total + terms_of(i1) <= budget)) {
            const Plan& pl = plan_of(i1);
            total += terms_of(i1);
            per = std::max(per, (uint32_t)(count[i1] * pl.n_points + pl.n_shared));
            rows += pl.n_shared; max_shared = std::max(max_shared, pl.n_shared);
            ++i1;
        }
        const uint32_t R = (uint32_t)(i1 - i0);
        const bool grow = !rk.ws.covers((uint32_t)total, 2 * R, per) || rk.fold.cap < 8 * (size_t)rows;
        if (grow) H2V_HIP_CHECK(hipStreamSynchronize(s));   // (an earlier set may still use the workspace)
        if ((rc = rk.ws.reserve((uint32_t)total, 2 * R, per)) || (rc = rk.fold.reserve(8 * (size_t)std::max(rows, 1u)))) return rc;
        desc.resize(R);
        for (uint32_t r = 0, row = 0; r < R; ++r) {
            const h2v_batch* b = batch_of(i0 + r);
            const uint32_t ns = b->plan->host.n_shared;
            desc[r] = FoldRange{b->shared.p, b->n, ns, (uint32_t)first[i0 + r], (uint32_t)count[i0 + r], row, 0};
            row += ns;
        }
        H2V_HIP_CHECK(hipMemcpyAsync(rk.ranges.p, desc.data(), sizeof(FoldRange) * R, hipMemcpyHostToDevice, s));
        if ((rc = fold_shared_ranges_enqueue(s, rk.ranges.p, R, max_shared, rk.fold.p))) return rc;
        MsmProblems pr;
        for (uint32_t r = 0; r < R; ++r)
            channel_problems(pr, batch_of(i0 + r), plan_of(i0 + r), first[i0 + r], (uint32_t)count[i0 + r], rk.acc.p + 2 * r, rk.fold.p + (size_t)desc[r].out * 8, desc[r].n_shared);
        rk.ws.tune = ctx->tuning; rk.ws.profile = false;
        if ((rc = msm_enqueue_multi(s, rk.ws, pr))) return rc;
        if ((rc = pairing_check_enqueue(s, ctx->pairing, rk.acc.p, R, rk.ok.p))) return rc;
        okv.resize(R);
        H2V_HIP_CHECK(hipMemcpyAsync(okv.data(), rk.ok.p, 4 * (size_t)R, hipMemcpyDeviceToHost, s));
        if (out_left || out_right) {
            if ((rc = point_to_bytes_enqueue(s, rk.acc.p, rk.out_bytes.p, rk.out_ident.p, 2 * R))) return rc;
            outb.resize(128 * (size_t)R);
            H2V_HIP_CHECK(hipMemcpyAsync(outb.data(), rk.out_bytes.p, outb.size(), hipMemcpyDeviceToHost, s));
        }
        const hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) { set_last_error(w + ": " + hipGetErrorString(e)); return H2V_ERR_DEVICE; }
        for (uint32_t r = 0; r < R; ++r) {
            range_ok[i0 + r] = okv[r] ? 1 : 0;
            if (out_left) memcpy(out_left + 64 * (i0 + r), &outb[128 * (size_t)r], 64);
            if (out_right) memcpy(out_right + 64 * (i0 + r), &outb[128 * (size_t)r + 64], 64);
        }
        i0 = i1;
    }
    return 0;
}

}  // namespace h2v

extern "C" {

int h2v_batch_recheck(h2v_batch* b, size_t n_ranges, const size_t* first, const size_t* count, int* range_ok, uint8_t* out_left, uint8_t* out_right) {
    if (!b) return require_stage(b, BatchStage::Finished, "h2v_batch_recheck");
    return recheck_impl("h2v_batch_recheck", &b, 1, n_ranges, nullptr, first, count, range_ok, out_left, out_right);
}

int h2v_batches_recheck(h2v_batch* const* batches, size_t n_batches, size_t n_ranges, const uint32_t* batch_of_range, const size_t* first, const size_t* count,
                        int* range_ok, uint8_t* out_left_xy, uint8_t* out_right_xy) {
    if (!batches || (n_ranges && !batch_of_range)) { set_last_error("h2v_batches_recheck: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    return recheck_impl("h2v_batches_recheck", batches, n_batches, n_ranges, batch_of_range, first, count, range_ok, out_left_xy, out_right_xy);
}

int h2v_random_scalars(uint8_t* out32, size_t n) {
    if (n && !out32) { set_last_error("h2v_random_scalars: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    std::vector<uint8_t> v;
    int rc = os_random_scalars(v, n);
    if (rc) return rc;
    if (n) memcpy(out32, v.data(), 32 * n);
    return 0;
}

int h2v_ctx_proof_shape(const h2v_ctx* ctx, size_t* proof_len, size_t* n_points, size_t* n_scalars, size_t* n_right_terms, size_t* n_instance_columns) {
    if (!ctx || !ctx->vk) { set_last_error("the context was created without a VerifyingKey"); return H2V_ERR_BAD_ARGUMENT; }
    // the layout does not depend on instance lengths; compile (or fetch) the plan for empty columns of the right count
    std::vector<size_t> lens(ctx_total_instance_columns(ctx), 0);
    PlanPin pin(const_cast<h2v_ctx*>(ctx));
    int rc = pin.get(lens);
    if (rc) return rc;
    PlanDevice* pd = pin.pd;
    if (proof_len) *proof_len = pd->host.proof_len;
    if (n_points) *n_points = pd->host.n_points;
    if (n_scalars) *n_scalars = pd->host.n_scalars;
    if (n_right_terms) *n_right_terms = pd->host.right_term_order.size();
    if (n_instance_columns) *n_instance_columns = ctx_total_instance_columns(ctx);
    return 0;
}

int h2v_batch_create(h2v_ctx* ctx, size_t max_proofs, size_t max_instance_values_per_proof, h2v_batch** out) {
    if (!ctx || !out || !max_proofs) { set_last_error("h2v_batch_create: bad argument"); return H2V_ERR_BAD_ARGUMENT; }
    if (max_proofs > (1u << 22)) { set_last_error("h2v_batch_create: max_proofs too large"); return H2V_ERR_BAD_ARGUMENT; }
    H2V_HIP_CHECK(hipSetDevice(ctx->device));
    h2v_batch* b = new h2v_batch();
    b->ctx = ctx; b->max_proofs = max_proofs; b->max_inst = max_instance_values_per_proof;
    // (no stream yet: need_stream, need_aux)
    for (int i = 0; i < 8; ++i) hipEventCreate(&b->ev[i]);
    *out = b;
    return 0;
}

void h2v_batch_destroy(h2v_batch* b) {
    if (!b) return;
    hipSetDevice(b->ctx->device);
    wait_for_streams(b);
    if (b->plan) { ctx_put_plan(b->ctx, b->plan); b->plan = nullptr; }
    for (int i = 0; i < 8; ++i) if (b->ev[i]) hipEventDestroy(b->ev[i]);
    if (b->aux) hipStreamDestroy(b->aux);
    if (b->copy) hipStreamDestroy(b->copy);
    if (b->ev_fork) hipEventDestroy(b->ev_fork);
    if (b->ev_join) hipEventDestroy(b->ev_join);
    if (b->ev_read) hipEventDestroy(b->ev_read);
    if (b->stream && b->owns_stream) hipStreamDestroy(b->stream);
    delete b;   // (frees the buffers)
}

int h2v_batch_upload(h2v_batch* b, size_t n, const uint8_t* proofs_flat, size_t proof_len, const uint8_t* instances_flat, size_t n_instance_columns,
                     const size_t* col_lens, const uint8_t* rand32_tail, size_t n_tail) {
    return upload_impl(b, n, proofs_flat, proof_len, instances_flat, n_instance_columns, col_lens, rand32_tail, n_tail);
}
// h2v_batch_upload_device: upload_impl for inputs in device memory.  Every check comes before the first device work; with the caller's
// draws nothing here waits for the stream, and what the host cannot see — the draws — is checked by k_ingest_draws, whose verdict
// finish_impl reads (b->device_draws).
int h2v_batch_upload_device(h2v_batch* b, size_t n, const void* d_proofs, size_t proof_stride, const void* d_instances, size_t n_instance_columns,
                            const size_t* col_lens, const void* d_rand_tail, size_t n_tail) {
    static const char who[] = "h2v_batch_upload_device";
    const UploadArgs a{who, n, d_proofs, d_instances, n_instance_columns, col_lens, d_rand_tail, n_tail};
    StageCommit commit{b};
    PlanPin pin(nullptr);
    int rc;
    if ((rc = upload_pin(b, a, H2V_ERR_BAD_ARGUMENT, false, pin))) return rc;
    const Plan& pl = pin.pd->host;
    const int device = b->ctx->device;
    if (proof_stride < pl.proof_len || (proof_stride & 15u)) { set_last_error(std::string(who) + ": proof_stride is below this VK's proof length, or no multiple of 16"); return H2V_ERR_BAD_ARGUMENT; }
    if (pl.proof_len & 15u) { set_last_error(std::string(who) + ": this VK's proof length is no multiple of 16"); return H2V_ERR_UNSUPPORTED; }
    if ((rc = upload_size_checks(b, pl, a))) return rc;
    const size_t inst_bytes = n * (size_t)pl.n_instance_values * 32;
    if (!d_rand_tail) n_tail = n;
    if (n && (rc = device_range_check(d_proofs, (n - 1) * proof_stride + pl.proof_len, device, "d_proofs"))) return rc;
    if (inst_bytes && (rc = device_range_check(d_instances, inst_bytes, device, "d_instances"))) return rc;
    if (d_rand_tail && n_tail && (rc = device_range_check(d_rand_tail, 32 * n_tail, device, "d_rand_tail"))) return rc;
    std::vector<uint8_t> os_rand;
    const uint8_t* host_tail = nullptr;
    if (!d_rand_tail && (rc = resolve_draws(host_tail, n_tail, os_rand, who))) return rc;
    if ((rc = upload_take(b, pin, n, n_tail, host_tail, d_rand_tail != nullptr))) return rc;
    hipStream_t s = b->stream;
    const uint32_t G = b->groups;
    if ((rc = ingest_rows_enqueue(s, d_proofs, proof_stride, pl.proof_len, n, d_instances, inst_bytes, b->proofs.p, b->inst.p, d_rand_tail ? b->ingest_verdict.p : nullptr, G))) return rc;
    if (d_rand_tail) {
        if ((rc = ingest_draws_enqueue(s, d_rand_tail, b->tail.p, (uint32_t)n_tail, (uint32_t)n, group_shape_device(b), b->ingest_verdict.p,
                                       static_cast<uint32_t*>(b->ingest_host.dev)))) return rc;
    } else if (n_tail) H2V_HIP_CHECK(hipMemcpyAsync(b->tail.p, host_tail, 32 * n_tail, hipMemcpyHostToDevice, s));
    if ((rc = shared_bases_enqueue(b, s))) return rc;
    if (!d_rand_tail) H2V_HIP_CHECK(hipStreamSynchronize(s));   // (the OS draws leave with this call)
    return upload_commit(b, commit);
}
// h2v_batch_finish_device: what finish_impl hands the host, handed to the caller's device arrays by kernels on the batch's stream
// (results_enqueue, util.hip).  Nothing here waits: no synchronise, no copy.  Every check comes before the first device work and a refusal
// leaves the batch as it was; the stage does not change, so the call may be repeated and a host finish may precede or follow it.
int h2v_batch_finish_device(h2v_batch* b, void* d_status, void* d_group_ok, void* d_left_xy, void* d_right_xy, void* d_group_failed, void* d_failed_index, size_t failed_cap,
                            void* d_summary) {
    static const char who[] = "h2v_batch_finish_device";
    int rc;
    if ((rc = require_stage(b, BatchStage::Launched, who))) return rc;
    const uint32_t n = b->n, G = b->groups;
    const int device = b->ctx->device;
    H2V_HIP_CHECK(hipSetDevice(device));
    if (d_failed_index && !failed_cap) { set_last_error(std::string(who) + ": failed_cap is 0 with d_failed_index given"); return H2V_ERR_BAD_ARGUMENT; }
    const uint32_t cap = d_failed_index ? (uint32_t)std::min<size_t>(failed_cap, n) : 0;   // (no more than n indices exist)
    const struct { const void* p; size_t bytes; const char* what; } outs[] = {
        {d_status, 4 * (size_t)n, "d_status"}, {d_group_ok, 4 * (size_t)G, "d_group_ok"}, {d_left_xy, 64 * (size_t)G, "d_left_xy"}, {d_right_xy, 64 * (size_t)G, "d_right_xy"},
        {d_group_failed, 4 * (size_t)G, "d_group_failed"}, {d_failed_index, 4 * (size_t)cap, "d_failed_index"}, {d_summary, 4 * (size_t)H2V_SUMMARY_WORDS, "d_summary"}};
    for (const auto& o : outs)
        if (o.p && (rc = device_range_check(o.p, o.bytes, device, o.what, who, "writes"))) return rc;
    // every argument is valid: device work from here on, and a failure of it leaves the batch Empty like any other
    StageCommit commit{b};
    const BatchStage stage = b->stage;
    if ((rc = join_tail(b)) || (rc = ensure_whole(b))) return rc;
    // the scratch: grow-only, for the batch's capacity and group count (ensure_buffers' rule).  The group words are zero between calls
    // (results_enqueue), so new memory is zeroed once, on the stream.
    if ((rc = b->finish_tiles.reserve(results_tiles(b->max_proofs)))) return rc;
    if (!b->finish_groups.p || G > b->finish_groups.cap) {
        if ((rc = b->finish_groups.reserve(G))) return rc;
        H2V_HIP_CHECK(hipMemsetAsync(b->finish_groups.p, 0, 4 * b->finish_groups.cap, b->stream));
    }
    ResultsOut out;
    out.status = static_cast<int*>(d_status); out.group_ok = static_cast<int*>(d_group_ok);
    out.left_xy = static_cast<uint8_t*>(d_left_xy); out.right_xy = static_cast<uint8_t*>(d_right_xy);
    out.group_failed = static_cast<uint32_t*>(d_group_failed); out.failed_index = cap ? static_cast<uint32_t*>(d_failed_index) : nullptr; out.failed_cap = cap;
    out.summary = static_cast<uint32_t*>(d_summary);
    const uint32_t flags = (b->last.pairing ? 1u : 0u) | (b->last.folded ? 2u : 0u);
    if ((rc = results_enqueue(b->stream, b->status, n, group_shape_device(b), b->fold_failed, b->ok, flags, b->out_bytes,
                              b->device_draws ? b->ingest_verdict.p : nullptr, b->finish_tiles.p, b->finish_groups.p, out))) return rc;
    commit.commit(stage);
    return 0;
}

// ---- every proof's Guard out of a launch (include/h2v_guards.h; the kernels: guards_out.hip).  The three forms share their checks
// (guards_call_check) and the kernels' arguments (gather_args); like h2v_batch_finish_device they begin with join_tail / ensure_whole,
// leave the stage as it is, and only READ what the launch left: msm_scal, left_scal, shared, pts, mult and the status words stay put
// until the next upload (h2v_batch_recheck relies on the same).
namespace {
struct GuardsCall { uint32_t first, count, TL, TR; };
// Launched or Finished, no guard variant, the range inside the upload, fewer than 2^31 terms per channel: before any device work
int guards_call_check(const h2v_batch* b, const char* who, size_t first, size_t count, GuardsCall& c) {
    if (int rc = require_stage(b, BatchStage::Launched, who)) return rc;
    const std::string w(who);
    if (!b->plan) { set_last_error(w + ": the batch holds no plan"); return H2V_ERR_BAD_ARGUMENT; }
    const Plan& pl = b->plan->host;
    if (pl.opts.guard_terms) { set_last_error(w + ": a guard-variant upload (h2v_guard_msm)"); return H2V_ERR_BAD_ARGUMENT; }
    if (first > b->n || count > b->n - first) { set_last_error(w + ": a range outside the upload"); return H2V_ERR_BAD_ARGUMENT; }
    for (const auto& t : pl.left_term_order)   // (no plan has one: the left channel's terms are the proof's own points)
        if (t.first) { set_last_error(w + ": a VK-wide base in the left channel"); return H2V_ERR_UNSUPPORTED; }
    const size_t TL = pl.left_term_order.size(), TR = pl.right_term_order.size();
    if ((uint64_t)count * std::max(TL, TR) >= (1ull << 31)) { set_last_error(w + ": 2^31 terms or more in one call: take the range in pieces"); return H2V_ERR_UNSUPPORTED; }
    c = GuardsCall{(uint32_t)first, (uint32_t)count, (uint32_t)TL, (uint32_t)TR};
    return 0;
}
GuardsGather gather_args(const h2v_batch* b, bool left, const GuardsCall& c) {
    const PlanDevice* pd = b->plan;
    return GuardsGather{left ? pd->left_terms.p : pd->right_terms.p, left ? c.TL : c.TR, left ? b->left_scal.p : b->msm_scal.p, b->shared.p, b->pts.p, b->status,
                        b->n, pd->host.n_points, c.first, c.count};
}
// the byte form of the range into six arrays of device memory (each may be null), on the batch's stream
int guards_bytes_enqueue(h2v_batch* b, const GuardsCall& c, uint8_t* const d[6]) {
    int rc;
    if ((rc = guards_gather_bytes_enqueue(b->stream, gather_args(b, true, c), d[0], d[1])) ||
        (rc = guards_gather_bytes_enqueue(b->stream, gather_args(b, false, c), d[2], d[3]))) return rc;
    return guards_proofs_enqueue(b->stream, b->mult.p, b->status, c.first, c.count, d[4], reinterpret_cast<int*>(d[5]));
}
// After a synchronise of the batch's stream: an upload that took its draws from device memory (h2v_batch_upload_device) has
// k_ingest_draws' verdict in the batch's pinned block, and a draw >= r there is what finish_impl refuses the launch for.  The forms that
// wait for the stream refuse it in the same words and hand out nothing; the stage stays, so the finish still reports it.
int guards_draw_fault(const h2v_batch* b, const char* who) {
    if (!b->device_draws) return 0;
    const uint32_t* verdict = reinterpret_cast<const uint32_t*>(b->ingest_host.p);
    if (verdict[0] == 0xffffffffu) return 0;
    set_last_error(std::string(who) + ": rand_tail scalar not canonical (draw " + std::to_string(verdict[0]) + " of the tail uploaded from device memory)");
    return H2V_ERR_BAD_ARGUMENT;
}
// the bytes the byte form writes per output: scalars and bases of either channel, multipliers, statuses
void guards_bytes_sizes(const GuardsCall& c, size_t bytes[6]) {
    const size_t n = c.count;
    bytes[0] = 32 * n * c.TL; bytes[1] = 64 * n * c.TL; bytes[2] = 32 * n * c.TR; bytes[3] = 64 * n * c.TR; bytes[4] = 32 * n; bytes[5] = 4 * n;
}
}  // namespace

int h2v_batch_guard_shape(const h2v_batch* b, size_t* n_left_terms, size_t* n_right_terms) {
    static const char who[] = "h2v_batch_guard_shape";
    if (int rc = require_stage(b, BatchStage::Uploaded, who)) return rc;
    if (!b->plan) { set_last_error(std::string(who) + ": the batch holds no plan"); return H2V_ERR_BAD_ARGUMENT; }
    if (n_left_terms) *n_left_terms = b->plan->host.left_term_order.size();
    if (n_right_terms) *n_right_terms = b->plan->host.right_term_order.size();
    return 0;
}

int h2v_batch_guards_device(h2v_batch* b, size_t first, size_t count, void* d_left_scalars32, void* d_left_bases64, void* d_right_scalars32, void* d_right_bases64,
                            void* d_mult32, void* d_status) {
    static const char who[] = "h2v_batch_guards_device";
    static const char* const what[6] = {"d_left_scalars32", "d_left_bases64", "d_right_scalars32", "d_right_bases64", "d_mult32", "d_status"};
    GuardsCall c;
    int rc;
    if ((rc = guards_call_check(b, who, first, count, c))) return rc;
    if (!count) return 0;
    uint8_t* const d[6] = {static_cast<uint8_t*>(d_left_scalars32), static_cast<uint8_t*>(d_left_bases64), static_cast<uint8_t*>(d_right_scalars32),
                           static_cast<uint8_t*>(d_right_bases64), static_cast<uint8_t*>(d_mult32), static_cast<uint8_t*>(d_status)};
    size_t bytes[6];
    guards_bytes_sizes(c, bytes);
    const int device = b->ctx->device;
    H2V_HIP_CHECK(hipSetDevice(device));
    for (int k = 0; k < 6; ++k)
        if (d[k] && (rc = device_range_check(d[k], bytes[k], device, what[k], who, "writes"))) return rc;
    // every argument is valid: device work from here on, and a failure of it leaves the batch Empty like any other
    StageCommit commit{b};
    const BatchStage stage = b->stage;
    if ((rc = join_tail(b)) || (rc = ensure_whole(b)) || (rc = guards_bytes_enqueue(b, c, d))) return rc;
    commit.commit(stage);
    return 0;
}

int h2v_batch_guards(h2v_batch* b, size_t first, size_t count, uint8_t* left_scalars32, uint8_t* left_bases64, uint8_t* right_scalars32, uint8_t* right_bases64,
                     uint8_t* mult32, int* per_proof_status) {
    static const char who[] = "h2v_batch_guards";
    GuardsCall c;
    int rc;
    if ((rc = guards_call_check(b, who, first, count, c))) return rc;
    uint8_t* const h[6] = {left_scalars32, left_bases64, right_scalars32, right_bases64, mult32, reinterpret_cast<uint8_t*>(per_proof_status)};
    size_t bytes[6], at[6], total = 0;
    guards_bytes_sizes(c, bytes);
    for (int k = 0; k < 6; ++k) { at[k] = total; if (h[k]) total += bytes[k]; }   // (every size but the last is a multiple of 16)
    if (!total) return 0;
    H2V_HIP_CHECK(hipSetDevice(b->ctx->device));
    StageCommit commit{b};
    const BatchStage stage = b->stage;
    if ((rc = join_tail(b)) || (rc = ensure_whole(b))) return rc;
    // (the scratch is idle: the call that used it last has waited for the stream)
    if ((rc = b->guards_scratch.reserve(total))) return rc;
    uint8_t* d[6];
    for (int k = 0; k < 6; ++k) d[k] = h[k] ? b->guards_scratch.p + at[k] : nullptr;
    if ((rc = guards_bytes_enqueue(b, c, d))) return rc;
    std::vector<uint8_t> host(total);   // (nothing is written on an error)
    H2V_HIP_CHECK(hipMemcpyAsync(host.data(), b->guards_scratch.p, total, hipMemcpyDeviceToHost, b->stream));
    H2V_HIP_CHECK(hipStreamSynchronize(b->stream));
    commit.commit(stage);   // (the device work is done; a draw fault below refuses the call and leaves the launch to its finish)
    if ((rc = guards_draw_fault(b, who))) return rc;
    for (int k = 0; k < 6; ++k) if (h[k]) memcpy(h[k], host.data() + at[k], bytes[k]);
    return 0;
}

// The object form: k_guards_gather writes the words and the points straight behind the objects' ends, on the BATCH's stream.  The
// objects' arrays belong to their contexts' streams, which every h2v_msm_* call leaves idle and which the locks held here keep idle;
// the batch's stream is waited for before the lengths change, so the call returns as every call on an object does: nothing in flight
// over its arrays.  (h2v_accumulator_process_batch orders the two sides the same way: one side idle, one synchronise at the end.)
int h2v_batch_guards_append(h2v_batch* b, size_t first, size_t count, h2v_msm* left, h2v_msm* right, size_t* n_failed) {
    static const char who[] = "h2v_batch_guards_append";
    const std::string w(who);
    GuardsCall c;
    int rc;
    if ((rc = guards_call_check(b, who, first, count, c))) return rc;
    if (left && left == right) { set_last_error(w + ": left and right are the same object"); return H2V_ERR_BAD_ARGUMENT; }
    h2v_msm* const objs[2] = {left, right};
    const size_t add[2] = {count * (size_t)c.TL, count * (size_t)c.TR};
    for (int k = 0; k < 2; ++k) {
        const h2v_msm* m = objs[k];
        if (!m) continue;
        if (m->ctx->device != b->ctx->device) { set_last_error(w + ": an object on another device than the batch"); return H2V_ERR_BAD_ARGUMENT; }
        if (m->ctx != b->ctx && !same_srs(m->ctx->params, b->ctx->params)) { set_last_error(w + ": an object over other params than the batch (g[0], g2 or s_g2 differ)"); return H2V_ERR_BAD_ARGUMENT; }
    }
    const CtxLocksPtr locks = lock_contexts(left ? left->ctx : nullptr, right ? right->ctx : nullptr);   // the objects' contexts, in the one order, until the call returns
    for (int k = 0; k < 2; ++k)   // (the lengths are read under the lock)
        if (objs[k] && (add[k] > H2V_MSM_MAX_TERMS || objs[k]->n + add[k] > H2V_MSM_MAX_TERMS)) { set_last_error(w + ": more than 2^24 terms in one object"); return H2V_ERR_BAD_ARGUMENT; }
    if (!count) { if (n_failed) *n_failed = 0; return 0; }
    H2V_HIP_CHECK(hipSetDevice(b->ctx->device));
    for (int k = 0; k < 2; ++k)   // grow first: nothing a caller can see changes
        if (objs[k] && (rc = msm_object_reserve(objs[k], objs[k]->n + add[k], objs[k]->ctx->stream))) return rc;
    StageCommit commit{b};
    const BatchStage stage = b->stage;
    if ((rc = join_tail(b)) || (rc = ensure_whole(b)) || (rc = b->guards_scratch.reserve(4 * (size_t)count))) return rc;
    int* const d_status = reinterpret_cast<int*>(b->guards_scratch.p);
    if ((left && (rc = guards_gather_terms_enqueue(b->stream, gather_args(b, true, c), left->scal.p + 8 * left->n, left->pts.p + left->n))) ||
        (right && (rc = guards_gather_terms_enqueue(b->stream, gather_args(b, false, c), right->scal.p + 8 * right->n, right->pts.p + right->n))) ||
        (rc = guards_proofs_enqueue(b->stream, nullptr, b->status, c.first, c.count, nullptr, d_status))) { hipStreamSynchronize(b->stream); return rc; }
    std::vector<int> st(count);
    hipError_t e = hipMemcpyAsync(st.data(), d_status, 4 * count, hipMemcpyDeviceToHost, b->stream);
    const hipError_t e2 = hipStreamSynchronize(b->stream);   // (whatever the copy said: nothing stays in flight over the objects' arrays)
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) { set_last_error(w + ": " + hipGetErrorString(e)); return H2V_ERR_DEVICE; }
    commit.commit(stage);   // (the device work is done; a draw fault below refuses the call and leaves the launch to its finish)
    if ((rc = guards_draw_fault(b, who))) return rc;
    // the commit: both lengths, then what the caller reads
    for (int k = 0; k < 2; ++k) if (objs[k]) objs[k]->n += add[k];
    size_t failed = 0;
    for (int v : st) if (v) ++failed;
    if (n_failed) *n_failed = failed;
    return 0;
}

// ---- point hints (include/h2v_hints.h; the kernels: k_decompress_hinted in verify_kernels.hip, k_hint_rows_out in util.hip).  The hints of an upload wait in `ycanon`, which has their shape and
// which no call between an upload and its launch reads or writes: k_decompress_hinted reads each point's hint there and writes the
// canonical y back, so what a launch leaves is a right set of hints for the next one (zeros for the points that do not decode), and
// h2v_batch_hints hands out the same bytes.  Like every h2v_batch_* call these take no context lock.
namespace {
// the checks the two forms of set_hints share, before any device work: Uploaded and not launched since, not decompressed by its upload, the upload's n
int set_hints_check(const h2v_batch* b, const char* who, size_t n) {
    const std::string w(who);
    if (!b) { set_last_error(w + ": null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if (b->stage != BatchStage::Uploaded || !b->plan) { set_last_error(w + ": the batch holds no upload that has not been launched yet"); return H2V_ERR_BAD_ARGUMENT; }
    if (b->decompressed) { set_last_error(w + ": the upload has decompressed its points already (h2v_batch_upload_launch)"); return H2V_ERR_BAD_ARGUMENT; }
    if (n != b->n) { set_last_error(w + ": n is not the upload's"); return H2V_ERR_BAD_ARGUMENT; }
    return 0;
}
// a range of a launch's rows: Launched or Finished, inside the upload
int hints_range_check(const h2v_batch* b, const char* who, size_t first, size_t count) {
    if (int rc = require_stage(b, BatchStage::Launched, who)) return rc;
    if (!b->plan) { set_last_error(std::string(who) + ": the batch holds no plan"); return H2V_ERR_BAD_ARGUMENT; }
    if (first > b->n || count > b->n - first) { set_last_error(std::string(who) + ": a range outside the upload"); return H2V_ERR_BAD_ARGUMENT; }
    return 0;
}
// What the three set_hints forms do once their arguments are checked and there are hints to stage.  Device work from the StageCommit
// on: a failure of it leaves the batch Empty like any other.  Reserved: what every hinted launch needs beside the hints, the miss word
// and the list counter, and a list word per point `ycanon` holds (grow-only: it grows only when ycanon has grown).  `transfer` brings
// the rows into `ycanon` and waits for whatever host memory it read; null_rows of the upload's proofs came without a row.
int hints_stage(h2v_batch* b, size_t null_rows, const std::function<int()>& transfer) {
    H2V_HIP_CHECK(hipSetDevice(b->ctx->device));
    StageCommit commit{b};
    int rc;
    if ((rc = b->hint_misses.reserve(2)) || (rc = b->miss_list.reserve(b->ycanon.cap / 32)) || (rc = transfer())) return rc;
    commit.commit(BatchStage::Uploaded);
    b->hinted = true; b->null_rows = (uint32_t)null_rows;
    return 0;
}
int strided_rows_check(const char* who, const void* d, size_t rows, size_t row_len, size_t row_stride, int device, const char* does) {
    if (row_stride < row_len || (row_stride & 15u) || (row_stride >> 4) > 0xffffffffu) { set_last_error(std::string(who) + ": row_stride is below 32 x n_points, or no multiple of 16"); return H2V_ERR_BAD_ARGUMENT; }
    return device_range_check(d, (rows - 1) * row_stride + row_len, device, "d_y32", who, does);
}
}  // namespace

int h2v_hints_point_offsets(const h2v_ctx* ctx, size_t* offsets, size_t cap, size_t* n_points) {
    static const char who[] = "h2v_hints_point_offsets";
    if (!ctx || !ctx->vk) { set_last_error(std::string(who) + ": the context was created without a VerifyingKey"); return H2V_ERR_BAD_ARGUMENT; }
    // (the layout does not depend on instance lengths: the plan for empty columns, as h2v_ctx_proof_shape takes it)
    std::vector<size_t> lens(ctx_total_instance_columns(ctx), 0);
    PlanPin pin(const_cast<h2v_ctx*>(ctx));
    if (int rc = pin.get(lens)) return rc;
    const std::vector<uint32_t>& po = pin.pd->host.point_offsets;
    if (n_points) *n_points = po.size();
    if (!offsets) return 0;
    if (cap < po.size()) { set_last_error(std::string(who) + ": cap is below the number of points"); return H2V_ERR_BAD_ARGUMENT; }
    for (size_t j = 0; j < po.size(); ++j) offsets[j] = po[j];
    return 0;
}

int h2v_hints_from_points(const uint8_t* points32, size_t n, uint8_t* y32, uint8_t* decoded) {
    if (n && (!points32 || !y32)) { set_last_error("h2v_hints_from_points: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* in = points32 + 32 * i;
        G1A pt;
        // (the identity's own encoding decodes but is no point of a proof: k_decompress refuses the flag, and so does this)
        const bool ok = !(in[31] & G1_FLAG_IDENTITY) && g1_decompress(in, pt);
        if (ok) pt.y.to_bytes(y32 + 32 * i); else memset(y32 + 32 * i, 0, 32);
        if (decoded) decoded[i] = ok ? 1 : 0;
    }
    return 0;
}

int h2v_batch_set_hints(h2v_batch* b, size_t n, const uint8_t* y32) {
    static const char who[] = "h2v_batch_set_hints";
    if (int rc = set_hints_check(b, who, n)) return rc;
    if (!y32) { b->hinted = false; return 0; }
    const size_t bytes = (size_t)n * b->plan->host.n_points * 32;
    return hints_stage(b, 0, [&]() -> int {
        if (!bytes) return 0;
        H2V_HIP_CHECK(hipMemcpyAsync(b->ycanon.p, y32, bytes, hipMemcpyHostToDevice, b->stream));
        H2V_HIP_CHECK(hipStreamSynchronize(b->stream));   // the host buffer is the caller's again
        return 0;
    });
}

// A row per proof, or none: the rows given are packed beside zero rows for the others (a zero hint always misses: no point of the
// curve has y = 0), and the whole goes where h2v_batch_set_hints puts its rows.  An upload none of whose proofs has a row has no hints.
int h2v_batch_set_hint_rows(h2v_batch* b, size_t n, const uint8_t* const* rows) {
    static const char who[] = "h2v_batch_set_hint_rows";
    if (int rc = set_hints_check(b, who, n)) return rc;
    if (!rows) { b->hinted = false; return 0; }
    const size_t row_len = (size_t)b->plan->host.n_points * 32;
    std::vector<uint8_t> flat(n * row_len, 0);
    size_t null_rows = 0;
    for (size_t i = 0; i < n; ++i)
        if (rows[i]) { if (row_len) memcpy(&flat[i * row_len], rows[i], row_len); } else ++null_rows;
    if (null_rows == n) { b->hinted = false; return 0; }
    return hints_stage(b, null_rows, [&]() -> int {
        if (flat.empty()) return 0;
        H2V_HIP_CHECK(hipMemcpyAsync(b->ycanon.p, flat.data(), flat.size(), hipMemcpyHostToDevice, b->stream));
        H2V_HIP_CHECK(hipStreamSynchronize(b->stream));   // (flat goes with this call)
        return 0;
    });
}

int h2v_batch_set_hints_device(h2v_batch* b, size_t n, const void* d_y32, size_t row_stride) {
    static const char who[] = "h2v_batch_set_hints_device";
    int rc;
    if ((rc = set_hints_check(b, who, n))) return rc;
    if (!d_y32) { b->hinted = false; return 0; }
    const size_t row_len = (size_t)b->plan->host.n_points * 32;
    const int device = b->ctx->device;
    H2V_HIP_CHECK(hipSetDevice(device));   // (the pointer's check asks the runtime: an argument check still, it leaves the stage alone)
    if (n && row_len && (rc = strided_rows_check(who, d_y32, n, row_len, row_stride, device, "reads"))) return rc;
    return hints_stage(b, 0, [&] { return ingest_rows_enqueue(b->stream, d_y32, row_stride, row_len, n, nullptr, 0, b->ycanon.p, nullptr, nullptr, 0); });   // (no wait: stream-ordered)
}

int h2v_batch_hints(h2v_batch* b, size_t first, size_t count, uint8_t* y32) {
    static const char who[] = "h2v_batch_hints";
    if (int rc = hints_range_check(b, who, first, count)) return rc;
    const size_t row_len = (size_t)b->plan->host.n_points * 32;
    if (!count || !row_len) return 0;
    if (!y32) { set_last_error(std::string(who) + ": null argument"); return H2V_ERR_BAD_ARGUMENT; }
    H2V_HIP_CHECK(hipSetDevice(b->ctx->device));
    StageCommit commit{b};
    const BatchStage stage = b->stage;
    H2V_HIP_CHECK(hipMemcpyAsync(y32, b->ycanon.p + first * row_len, count * row_len, hipMemcpyDeviceToHost, b->stream));
    H2V_HIP_CHECK(hipStreamSynchronize(b->stream));
    commit.commit(stage);
    return 0;
}

int h2v_batch_hints_device(h2v_batch* b, size_t first, size_t count, void* d_y32, size_t row_stride) {
    static const char who[] = "h2v_batch_hints_device";
    int rc;
    if ((rc = hints_range_check(b, who, first, count))) return rc;
    const size_t row_len = (size_t)b->plan->host.n_points * 32;
    if (!count || !row_len) return 0;
    if (!d_y32) { set_last_error(std::string(who) + ": null argument"); return H2V_ERR_BAD_ARGUMENT; }
    const int device = b->ctx->device;
    H2V_HIP_CHECK(hipSetDevice(device));
    if ((rc = strided_rows_check(who, d_y32, count, row_len, row_stride, device, "writes"))) return rc;
    StageCommit commit{b};
    const BatchStage stage = b->stage;
    if ((rc = hint_rows_out_enqueue(b->stream, b->ycanon.p + first * row_len, row_len, count, d_y32, row_stride))) return rc;
    commit.commit(stage);
    return 0;
}

int h2v_batch_hint_stats(h2v_batch* b, size_t* n_points, size_t* n_hinted, size_t* n_missed) {
    static const char who[] = "h2v_batch_hint_stats";
    if (int rc = require_stage(b, BatchStage::Launched, who)) return rc;
    if (!b->plan) { set_last_error(std::string(who) + ": the batch holds no plan"); return H2V_ERR_BAD_ARGUMENT; }
    H2V_HIP_CHECK(hipSetDevice(b->ctx->device));
    StageCommit commit{b};
    const BatchStage stage = b->stage;
    uint32_t missed = 0;
    if (b->launch_hinted) H2V_HIP_CHECK(hipMemcpyAsync(&missed, b->hint_misses.p, sizeof missed, hipMemcpyDeviceToHost, b->stream));
    H2V_HIP_CHECK(hipStreamSynchronize(b->stream));
    commit.commit(stage);
    const size_t points = (size_t)b->n * b->plan->host.n_points;
    if (n_points) *n_points = points;
    // (the points of proofs without a row were staged as zero hints and all missed: neither hinted nor missed)
    const size_t unhinted = (size_t)b->launch_null_rows * b->plan->host.n_points;
    if (n_hinted) *n_hinted = b->launch_hinted ? points - unhinted : 0;
    if (n_missed) *n_missed = b->launch_hinted ? missed - unhinted : 0;
    return 0;
}

int h2v_batch_launch(h2v_batch* b, int with_pairing) { return launch_impl(b, with_pairing); }
int h2v_batch_upload_launch(h2v_batch* b, size_t n, const uint8_t* proofs_flat, size_t proof_len, const uint8_t* instances_flat, size_t n_instance_columns,
                            const size_t* col_lens, const uint8_t* rand32_tail, size_t n_tail, int with_pairing) {
    if (int rc = upload_impl(b, n, proofs_flat, proof_len, instances_flat, n_instance_columns, col_lens, rand32_tail, n_tail, true)) return rc;
    return launch_impl(b, with_pairing);
}
int h2v_batch_finish(h2v_batch* b, int* per_proof_status, int* batch_ok, uint8_t out_left_xy[64], uint8_t out_right_xy[64]) {
    if (b && b->groups > 1) { set_last_error("h2v_batch_finish: the batch is grouped, use h2v_batch_finish_groups"); return H2V_ERR_BAD_ARGUMENT; }
    return finish_impl(b, "h2v_batch_finish", per_proof_status, batch_ok, out_left_xy, out_right_xy);
}
int h2v_batch_set_groups(h2v_batch* b, size_t groups) {
    if (!b || !groups || groups > MSM_MAX_PROBLEMS / 2 || groups > b->max_proofs) { set_last_error("h2v_batch_set_groups: bad group count"); return H2V_ERR_BAD_ARGUMENT; }
    wait_for_streams(b);   // (the last launch and the last upload read what changes below)
    if (b->plan) { ctx_put_plan(b->ctx, b->plan); b->plan = nullptr; }
    b->groups = (uint32_t)groups; b->stage = BatchStage::Empty; b->hinted = false;  // the next upload grows the buffers if the group count needs more
    b->group_off.clear(); b->group_last.clear();   // (equal groups again after h2v_batch_set_group_sizes)
    return 0;
}
int h2v_batch_set_group_sizes(h2v_batch* b, const size_t* sizes, size_t n_groups) {
    static const char who[] = "h2v_batch_set_group_sizes";
    if (!b || !sizes || !n_groups || n_groups > MSM_MAX_PROBLEMS / 2) { set_last_error(std::string(who) + ": null argument or bad group count"); return H2V_ERR_BAD_ARGUMENT; }
    size_t total = 0;
    for (size_t g = 0; g < n_groups; ++g) {
        if (!sizes[g]) { set_last_error(std::string(who) + ": a group of no proofs"); return H2V_ERR_BAD_ARGUMENT; }
        if (sizes[g] > b->max_proofs - total) { set_last_error(std::string(who) + ": the sizes exceed the batch capacity"); return H2V_ERR_BAD_ARGUMENT; }
        total += sizes[g];
    }
    wait_for_streams(b);   // (the last launch reads the device copies replaced below)
    if (b->plan) { ctx_put_plan(b->ctx, b->plan); b->plan = nullptr; }
    b->groups = (uint32_t)n_groups; b->stage = BatchStage::Empty; b->hinted = false;
    b->group_off.assign(n_groups + 1, 0); b->group_last.assign(total, 0);
    for (size_t g = 0; g < n_groups; ++g) { b->group_off[g + 1] = b->group_off[g] + (uint32_t)sizes[g]; b->group_last[b->group_off[g + 1] - 1] = 1; }
    // The offsets and the last-of-group marks go to the device here, where they change and every stream of the batch is idle, and
    // nowhere else: no upload copies them (one from device memory enqueues behind a busy stream and must not copy from host vectors there).
    int rc;
    H2V_HIP_CHECK(hipSetDevice(b->ctx->device));
    if ((rc = b->d_group_off.reserve(b->group_off.size())) || (rc = b->d_group_last.reserve(total))) return rc;
    H2V_HIP_CHECK(hipMemcpy(b->d_group_off.p, b->group_off.data(), 4 * b->group_off.size(), hipMemcpyHostToDevice));
    H2V_HIP_CHECK(hipMemcpy(b->d_group_last.p, b->group_last.data(), total, hipMemcpyHostToDevice));
    return 0;
}
int h2v_batch_finish_groups(h2v_batch* b, int* per_proof_status, int* group_ok, uint8_t* out_left_xy, uint8_t* out_right_xy, size_t n_groups) {
    if (!b || n_groups != b->groups) { set_last_error("h2v_batch_finish_groups: n_groups does not match h2v_batch_set_groups"); return H2V_ERR_BAD_ARGUMENT; }
    return finish_impl(b, "h2v_batch_finish_groups", per_proof_status, group_ok, out_left_xy, out_right_xy);
}
int h2v_batch_accumulators(h2v_batch* b, void** device_ptr, size_t* nbytes) {
    if (!b || !b->acc.p || !device_ptr) { set_last_error("h2v_batch_accumulators: nothing uploaded"); return H2V_ERR_BAD_ARGUMENT; }
    if (b->stage >= BatchStage::Launched) { H2V_HIP_CHECK(hipSetDevice(b->ctx->device)); int rcw = join_tail(b); if (!rcw) rcw = ensure_whole(b); if (rcw) return rcw; }
    *device_ptr = b->acc.p;
    if (nbytes) *nbytes = 2 * sizeof(G1J) * b->groups;   // raw points, no failure word: see h2v_batch_export_accumulators
    return 0;
}
void* h2v_batch_stream(h2v_batch* b) { return b && !need_stream(b) ? (void*)b->stream : nullptr; }
int h2v_batch_set_stream(h2v_batch* b, void* hip_stream) {
    if (!b) return H2V_ERR_BAD_ARGUMENT;
    hipSetDevice(b->ctx->device);
    if (b->stream || !b->owns_stream) hipStreamSynchronize(b->stream);
    if (b->owns_stream && b->stream) hipStreamDestroy(b->stream);
    b->stream = (hipStream_t)hip_stream; b->owns_stream = false;
    return join_tail(b);   // (the new stream waits for what the last launch left on the auxiliary stream)
}
int h2v_batch_export_accumulators(h2v_batch* b, void* device_dst) {
    if (int rc = require_stage(b, BatchStage::Launched, "h2v_batch_export_accumulators")) return rc;
    if (!device_dst) { set_last_error("h2v_batch_export_accumulators: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if (group_shape(b).off) { set_last_error("h2v_batch_export_accumulators: the batch has groups of unequal size (a record counts the failures of n / groups proofs)"); return H2V_ERR_BAD_ARGUMENT; }
    H2V_HIP_CHECK(hipSetDevice(b->ctx->device));
    if (int rc = join_tail(b)) return rc;   // (the records: pieces if the launch left pieces)
    if (b->split.parts) return export_records_enqueue(b->stream, nullptr, b->split.pts, b->split.parts, b->split.shift, b->status, b->n, b->groups, device_dst);
    return export_records_enqueue(b->stream, b->acc.p, nullptr, 1, 0, b->status, b->n, b->groups, device_dst);
}
int h2v_batch_fold_check_enqueue(h2v_batch* b, const void* device_accumulators, size_t n_parts) {
    int rc;
    if ((rc = require_stage(b, BatchStage::Launched, "h2v_batch_fold_check_enqueue"))) return rc;
    if (group_shape(b).off) { set_last_error("h2v_batch_fold_check_enqueue: the batch has groups of unequal size"); return H2V_ERR_BAD_ARGUMENT; }
    StageCommit commit{b};
    if (!device_accumulators || !n_parts) { set_last_error("h2v_batch_fold_check_enqueue: bad argument"); return H2V_ERR_BAD_ARGUMENT; }
    H2V_HIP_CHECK(hipSetDevice(b->ctx->device));
    if ((rc = join_tail(b))) return rc;
    const uint32_t G = b->groups;
    // the fold keeps the cut of this rank's own launch: records cut the same way add up piece by piece, the pairing takes the pieces
    // (the folded pieces replace the rank's own in the workspace: they were exported before the collective that brought these records)
    if (b->split.parts) {
        G1JSlot* pieces = b->ws.pieces.p; G1JSlot* ready = b->ws.pieces.p + (size_t)MSM_MAX_PARTS * b->ws.cap_problems;
        if ((rc = fold_records_enqueue(b->stream, device_accumulators, (uint32_t)n_parts, G, b->split.parts, b->split.shift, b->acc.p, pieces, ready, b->fold_failed))) return rc;
    } else if ((rc = fold_records_enqueue(b->stream, device_accumulators, (uint32_t)n_parts, G, 1, 0, b->acc.p, nullptr, nullptr, b->fold_failed))) return rc;
    if ((rc = close_enqueue(b, true))) return rc;
    b->last.folded = true;     // (h2v_batch_identify: the batch's own accumulators are now only in the record it exported)
    commit.commit(b->stage);   // (a launch folded after its finish stays Finished)
    return 0;
}
// Which proofs of a finished staged batch fail the pairing.  Step 1: every group's OWN verdict — the launch's bit if its pairing ran
// over the group's own accumulators, else one pairing launch over all groups (the records the launch exported put together, or the
// whole points a launch without a pairing left); no MSM.  Step 2: one pooled search (identify_search) from the groups whose own check
// fails.  Only the re-check's buffers are written.
int h2v_batch_identify(h2v_batch* b, const void* own_records, int* per_proof_status, int* group_own_ok, size_t* n_range_checks) {
    static const char who[] = "h2v_batch_identify";
    int rc;
    if ((rc = require_stage(b, BatchStage::Finished, who))) return rc;
    const uint32_t n = b->n, G = b->groups;
    if (!own_records && b->last.folded) { set_last_error(std::string(who) + ": a fold has replaced the batch's own accumulators: pass the records it exported"); return H2V_ERR_BAD_ARGUMENT; }
    // a single proof's check equals SingleStrategy's only when its multiplier is non-zero (h2v_batch_recheck's rule, for every proof)
    for (uint32_t g = 0; g < G; ++g)
        if (b->zero_below[g]) { set_last_error(std::string(who) + ": a proof of the batch has a zero multiplier (a zero draw)"); return H2V_ERR_BAD_ARGUMENT; }
    h2v_ctx* ctx = b->ctx;
    H2V_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = b->stream;
    // (a fold after the finish may still be sending the result block: the same statuses again)
    H2V_HIP_CHECK(wait_for_streams(b));
    const int* raw = results_at(b->results_host.p, ResultsLayout{G, n}).status;
    std::vector<std::vector<int>> st(1, std::vector<int>(n));
    std::vector<uint32_t> failed(G, 0);
    const GroupShape shape = group_shape(b);
    for (uint32_t i = 0; i < n; ++i) { st[0][i] = status_decode(raw[i]); if (raw[i]) ++failed[shape.of(i)]; }
    if (own_records && shape.off) { set_last_error(std::string(who) + ": a batch with groups of unequal size exports no records"); return H2V_ERR_BAD_ARGUMENT; }
    if (own_records) {
        std::vector<uint32_t> hdr(4 * (size_t)G);   // [failed, parts, shift, 0] of every record
        H2V_HIP_CHECK(hipMemcpy2DAsync(hdr.data(), 16, own_records, H2V_ACC_RECORD_BYTES, 16, G, hipMemcpyDeviceToHost, s));
        H2V_HIP_CHECK(hipStreamSynchronize(s));
        for (uint32_t g = 0; g < G; ++g)
            if (hdr[4 * g + 1] < 1 || hdr[4 * g + 1] > H2V_ACC_RECORD_PIECES || hdr[4 * g] != failed[g]) {
                set_last_error(std::string(who) + ": own_records does not hold the records this launch exported (piece count, or failure count against the statuses)");
                return H2V_ERR_BAD_ARGUMENT;
            }
    }
    std::vector<uint32_t> own(G, 0);
    if (b->last.pairing && !b->last.folded) {
        for (uint32_t g = 0; g < G; ++g) own[g] = pairing_passed(b, g) ? 1u : 0u;
    } else {
        Recheck& rk = b->recheck;
        const uint32_t max_ranges = MSM_MAX_PROBLEMS / 2;   // (recheck_impl's sizes: G <= max_ranges, h2v_batch_set_groups)
        if ((rc = rk.acc.reserve(2 * (size_t)max_ranges)) || (rc = rk.ok.reserve(max_ranges)) || (rc = rk.failed.reserve(max_ranges))) return rc;
        if ((rc = join_tail(b))) return rc;
        // without records: a finished launch without a pairing has its whole points in acc (finish_impl: ensure_whole)
        const G1J* pts = b->acc.p;
        if (own_records) {
            if ((rc = fold_records_enqueue(s, own_records, 1, G, 1, 0, rk.acc.p, nullptr, nullptr, rk.failed.p))) return rc;
            pts = rk.acc.p;
        }
        if ((rc = pairing_check_enqueue(s, ctx->pairing, pts, G, rk.ok.p))) return rc;
        H2V_HIP_CHECK(hipMemcpyAsync(own.data(), rk.ok.p, 4 * (size_t)G, hipMemcpyDeviceToHost, s));
        const hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) { set_last_error(std::string(who) + ": " + hipGetErrorString(e)); return H2V_ERR_DEVICE; }
    }
    std::vector<IdentifyStart> start;
    for (uint32_t g = 0; g < G; ++g) if (!own[g] && shape.count(g)) start.push_back({0, shape.first(g), shape.count(g)});
    size_t checks = 0;
    if (!start.empty() && (rc = identify_search({b}, start, true, st, &checks))) return rc;
    if (per_proof_status) for (uint32_t i = 0; i < n; ++i) per_proof_status[i] = st[0][i];
    if (group_own_ok) for (uint32_t g = 0; g < G; ++g) group_own_ok[g] = own[g] ? 1 : 0;
    if (n_range_checks) *n_range_checks = checks;
    return 0;
}
int h2v_batch_set_profiling(h2v_batch* b, int level) { if (!b) return H2V_ERR_BAD_ARGUMENT; b->profiling = level == 0 ? 0 : (level == H2V_PROFILE_KERNEL ? 1 : 2); return 0; }
int h2v_batch_timings(h2v_batch* b, float* ms, int cap) {
    if (!b || !ms) return H2V_ERR_BAD_ARGUMENT;
    int k = cap < 7 ? cap : 7;
    for (int i = 0; i < k; ++i) ms[i] = b->last_ms[i];
    return k;
}

}  // extern "C"
