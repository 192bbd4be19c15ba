// C-ABI one-shot verification entry points (include/h2v.h): h2v_verify_batch and its _seeded / _shapes / _keys / _identify / _keys_identify forms,
// h2v_verify_each, h2v_guard_msm and h2v_fold_check.  Each call runs on its context's scratch batch through the staged batch of batch.hip.
#include "../../include/h2v.h"
#include "../../include/h2v_hint_rows.h"
#include "batch.h"
#include <string.h>
#include <algorithm>
#include <functional>
#include <map>
#include <memory>
#include <utility>

using namespace h2v;

namespace {

// A one-shot call's hold on its context: ctx->mu (the context's stream and scratch batch serve one call at a time) and, once taken, the
// scratch batch, given back at the end of the call — or destroyed if it holds more than H2V_SCRATCH_BATCH_MAX proofs.  (After an error it is Empty.)
// It also holds the proofs last packed for the batch (pack_inputs, owned copies): each caller collects them before it packs the next.
#define H2V_SCRATCH_BATCH_MAX 1024u
struct ScratchBatch {
    h2v_ctx* const ctx;
    std::lock_guard<std::mutex> lock;
    h2v_batch* b = nullptr;
    PlanPin pin;                        // the packed proofs' plan
    std::vector<size_t> cols;           // and its column lengths
    std::vector<uint8_t> flat, iflat;   // the proofs and their instances, proof after proof
    std::vector<int> forced;            // per proof: the status fixed on the host (a short proof), or 0
    // point hints (include/h2v_hints.h; a _hinted call): per packed proof its hint row where the caller holds it, or null (none given, or
    // a short proof); empty in a call without hints.  hstats: where the call sums its launches' h2v_batch_hint_stats, or null
    std::vector<const uint8_t*> hrows;
    size_t* hstats = nullptr;
    explicit ScratchBatch(h2v_ctx* c) : ctx(c), lock(c->mu), pin(c) {}
    ~ScratchBatch() { if (b && b->max_proofs <= H2V_SCRATCH_BATCH_MAX && !ctx->scratch_batch) ctx->scratch_batch = b; else h2v_batch_destroy(b); }
    int take(size_t capacity, size_t max_inst) {   // the context's batch, or a new one if it has none or a smaller one (once per holder)
        b = std::exchange(ctx->scratch_batch, nullptr);
        if (b && (b->max_proofs < capacity || b->max_inst < max_inst)) { h2v_batch_destroy(b); b = nullptr; }
        return b ? 0 : h2v_batch_create(ctx, capacity, max_inst, &b);
    }
};

// The argument checks of a one-shot call over one instance shape, its plan (in `sb.pin`), and its pointer-array proofs / instances packed
// into the flat layout (in `sb`): proof i is proofs[idx[i]] (idx null: proofs[i]).  Proofs shorter than the VK's proof are the reader
// running dry: "failed to fill whole buffer" -> Error::Transcript, or Opening inside the multi-open part (pl.opening_offset: h1, the first
// point after all scalars).  hints: the call's hint rows, indexed like the proofs, and its counters (a call without hints: neither)
int pack_inputs(ScratchBatch& sb, size_t n, const size_t* idx, const uint8_t* const* proofs, const size_t* proof_lens, const uint8_t* const* instances32,
                size_t ncols, const size_t* col_lens, const CallHints& hints = CallHints()) {
    if ((n && (!proofs || !proof_lens)) || (ncols && !col_lens)) { set_last_error("null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if (sb.ctx->vk && ncols != ctx_total_instance_columns(sb.ctx)) { set_last_error("instances do not match the VK's instance column count"); return H2V_ERR_INVALID_INSTANCES; }
    sb.cols.assign(col_lens, col_lens + ncols);
    if (int rc = sb.pin.get(sb.cols)) return rc;   // (it refuses a context without a VK)
    const Plan& pl = sb.pin.pd->host;
    const size_t per_inst = (size_t)pl.n_instance_values * 32;
    sb.flat.assign(n * pl.proof_len, 0); sb.iflat.assign(n * per_inst, 0); sb.forced.assign(n, 0);
    sb.hrows.assign(hints.rows ? n : 0, nullptr); sb.hstats = hints.stats;
    for (size_t i = 0; i < n; ++i) {
        const size_t j = idx ? idx[i] : i;
        if (!proofs[j]) { set_last_error("null proof pointer"); return H2V_ERR_BAD_ARGUMENT; }
        if (proof_lens[j] < pl.proof_len) {
            // the reader runs dry; every point of the packed copy is made undecodable (x = 2^254-1 >= p) so that the proof
            // contributes nothing, and the status is set to what the reference reports for the place where it ran dry
            sb.forced[i] = proof_lens[j] < pl.opening_offset ? H2V_ERR_TRANSCRIPT : H2V_ERR_OPENING;
            memset(&sb.flat[i * pl.proof_len], 0xff, pl.proof_len);
        } else {
            memcpy(&sb.flat[i * pl.proof_len], proofs[j], pl.proof_len);
            if (hints.rows) sb.hrows[i] = hints.rows[j];   // (a short proof keeps none: the batch stages a zero row for it)
        }
        if (per_inst) { if (!instances32 || !instances32[j]) { set_last_error("null instances pointer"); return H2V_ERR_BAD_ARGUMENT; } memcpy(&sb.iflat[i * per_inst], instances32[j], per_inst); }
    }
    return 0;
}

// n draws of 1: SingleStrategy's multipliers, or placeholders where the multipliers are gathered (run_groups)
std::vector<uint8_t> unit_draws(size_t n) {
    std::vector<uint8_t> d(32 * n, 0);
    for (size_t i = 0; i < n; ++i) d[32 * i] = 1;
    return d;
}

// Packed proofs on a batch (the scratch batch, or one the call made for itself), first half: proofs [off, off + m) of `sb` as `groups`
// groups on b, uploaded with the draws rand32 (null: OS draws) and launched with or without the pairing checks, the multipliers gathered
// from mult[idx[..]] if mult is given.  Nothing waits (but the copy of the hint rows of a call that has them).
// The hint rows of the packed proofs [off, off + m) onto b's upload of them, through the staged batch's own setter; a call without hints: nothing
int place_hints(const ScratchBatch& sb, h2v_batch* b, size_t off, size_t m) {
    return sb.hrows.empty() ? 0 : h2v_batch_set_hint_rows(b, m, sb.hrows.data() + off);
}
int enqueue_group(const ScratchBatch& sb, h2v_batch* b, size_t off, size_t m, size_t groups, const uint8_t* rand32, int with_pairing, bool guard = false,
                  const Fr* mult = nullptr, const uint32_t* idx = nullptr) {
    const Plan& pl = sb.pin.pd->host;
    int rc;
    if ((rc = h2v_batch_set_groups(b, groups)) ||
        (rc = upload_impl(b, m, sb.flat.data() + off * pl.proof_len, pl.proof_len, sb.iflat.data() + off * (size_t)pl.n_instance_values * 32, sb.cols.size(), sb.cols.data(),
                          rand32, m, false, guard)) || (rc = place_hints(sb, b, off, m))) return rc;
    return launch_impl(b, with_pairing, mult, idx);
}

// Second half: the statuses of b's launch of proofs [off, ..) of `sb` into st and its group verdicts into group_ok (either may be null),
// with the statuses pack_inputs forced in place of the device's and the groups that hold such a proof failed
int collect_group(const ScratchBatch& sb, h2v_batch* b, size_t off, int* st, int* group_ok, uint8_t* out_left = nullptr, uint8_t* out_right = nullptr) {
    if (int rc = h2v_batch_finish_groups(b, st, group_ok, out_left, out_right, b->groups)) return rc;
    for (uint32_t i = 0; i < b->n; ++i)
        if (const int v = sb.forced[off + i]) { if (st) st[i] = v; if (group_ok) group_ok[group_shape(b).of(i)] = 0; }
    if (sb.hstats) {   // a _hinted call that asked for its counters: this launch's
        size_t c[3];
        if (int rc = h2v_batch_hint_stats(b, &c[0], &c[1], &c[2])) return rc;
        for (int k = 0; k < 3; ++k) sb.hstats[k] += c[k];
    }
    return 0;
}

// One AccumulatorStrategy batch of a one-shot call, packed and run on the context's scratch batch; the batch stays in `sb` for the caller
int pack_and_run(ScratchBatch& sb, size_t n, const uint8_t* const* proofs, const size_t* proof_lens, const uint8_t* const* instances32, size_t ncols,
                 const size_t* col_lens, const uint8_t* rand32, int with_pairing, bool guard, int* per_proof_status, int* batch_ok, uint8_t* out_left,
                 uint8_t* out_right, const CallHints& hints = CallHints()) {
    int rc;
    if ((rc = pack_inputs(sb, n, nullptr, proofs, proof_lens, instances32, ncols, col_lens, hints)) || (rc = sb.take(n ? n : 1, sb.pin.pd->host.n_instance_values)) ||
        (rc = enqueue_group(sb, sb.b, 0, n, 1, rand32, with_pairing, guard))) return rc;
    return collect_group(sb, sb.b, 0, per_proof_status, batch_ok, out_left, out_right);
}

// The search of h2v_verify_batch_identify, measured at 1024 proofs (tools/identify_probe.py): every failing range is cut into
// H2V_IDENTIFY_FANOUT pieces per round — or straight into single proofs once the failing ranges hold at most H2V_IDENTIFY_DIRECT
// proofs together, one set of re-check launches (MSM_MAX_PROBLEMS / 2 checks).  A round is a latency chain up to ~128 checks (32 ranges
// of 32 proofs: 1.9 ms, 128 single proofs: 2.0 ms, 512: 4.1 ms), so rounds are what to save: one bad proof in 1024 takes two (32 + 32 checks).
// Over several batches (h2v_verify_batch_keys_identify) a round starts from one failing range per group, up to 64 of them: the fanout
// shrinks as the failing ranges grow in number, so that a round stays within H2V_IDENTIFY_ROUND checks — one set of launches, whose cost
// grows far less than its width (see above) — while a round of one or a few failing ranges keeps the full fanout.
#define H2V_IDENTIFY_FANOUT 32
#define H2V_IDENTIFY_DIRECT 512
#define H2V_IDENTIFY_ROUND (MSM_MAX_PROBLEMS / 2)

}  // namespace

namespace h2v {

// the pairing's verdict of failing ranges of finished batches, proof by proof: st[k][i] = H2V_ERR_CONSTRAINT_SYSTEM_FAILURE for every proof
// i of a start range of batch bs[k] whose own check fails (st[k][i] == 0 on entry).  A range whose check fails holds at least one failing
// proof (the check of a range is the product of its pieces' checks), so every round ends with at least one failing piece per failing range.
// Every round is ONE re-check over the pieces of all start ranges (recheck_impl).  From one start range the policy is the one measured
// above.  `known`: every start range has failed a check of its own (a batch's own pairing, a group's own verdict: h2v_batch_identify);
// else only the fold of all of them is known to fail (h2v_verify_batch_keys_identify): the first round checks every start range as it
// is, a one-proof range included, before anything is flagged.
int identify_search(const std::vector<h2v_batch*>& bs, const std::vector<IdentifyStart>& start, bool known, std::vector<std::vector<int>>& st, size_t* n_checks) {
    typedef IdentifyStart Item;
    // proofs with a non-zero status contribute nothing: a range is trimmed to its first and last live proof, and one without a live proof passes
    auto trim = [&](uint32_t k, size_t a, size_t c, std::vector<Item>& out) {
        const std::vector<int>& sk = st[k];
        size_t e = a + c;
        while (a < e && sk[a]) ++a;
        while (e > a && sk[e - 1]) --e;
        if (e > a) out.push_back({k, a, e - a});
    };
    std::vector<Item> failing, pieces;
    for (const Item& r : start) trim(r.b, r.first, r.count, failing);
    const bool pooled = start.size() > 1;
    int rc = 0;
    while (!failing.empty()) {
        pieces.clear();
        size_t total = 0;
        for (auto& r : failing) total += r.count;
        const size_t fanout = pooled ? std::min<size_t>(H2V_IDENTIFY_FANOUT, std::max<size_t>(2, H2V_IDENTIFY_ROUND / failing.size())) : H2V_IDENTIFY_FANOUT;
        for (auto& r : failing) {
            if (r.count == 1 && known) { st[r.b][r.first] = H2V_ERR_CONSTRAINT_SYSTEM_FAILURE; continue; }   // (its check already was that proof's own)
            const size_t k = total <= H2V_IDENTIFY_DIRECT ? r.count : std::min<size_t>(fanout, r.count);
            for (size_t i = 0; i < k; ++i) {
                const size_t a = r.first + r.count * i / k, e = r.first + r.count * (i + 1) / k;
                trim(r.b, a, e - a, pieces);
            }
        }
        if (pieces.empty()) break;
        std::vector<uint32_t> bor(pieces.size());
        std::vector<size_t> f(pieces.size()), c(pieces.size());
        std::vector<int> ok(pieces.size(), 0);
        for (size_t i = 0; i < pieces.size(); ++i) { bor[i] = pieces[i].b; f[i] = pieces[i].first; c[i] = pieces[i].count; }
        if ((rc = recheck_impl("identification", bs.data(), bs.size(), pieces.size(), bor.data(), f.data(), c.data(), ok.data(), nullptr, nullptr))) return rc;
        *n_checks += pieces.size();
        known = true;
        failing.clear();
        for (size_t i = 0; i < pieces.size(); ++i) {
            if (ok[i]) continue;
            if (c[i] == 1) st[bor[i]][f[i]] = H2V_ERR_CONSTRAINT_SYSTEM_FAILURE;
            else failing.push_back(pieces[i]);
        }
    }
    return 0;
}

}  // namespace h2v

namespace {

// the whole range of every batch (one group each) as the start of a search
std::vector<IdentifyStart> whole_batches(const std::vector<std::vector<int>>& st) {
    std::vector<IdentifyStart> start;
    for (uint32_t k = 0; k < st.size(); ++k) start.push_back({k, 0, st[k].size()});
    return start;
}

// (the caller holds ctx->mu)  pairing_ok (may be null): the pairing's own verdict, before the records' failure counts are folded into `ok`
int fold_check_locked(h2v_ctx* ctx, const void* device_accumulators, size_t n_parts, int* ok, uint8_t* out_left_xy, uint8_t* out_right_xy,
                      int* pairing_ok = nullptr) {
    H2V_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    DevBuf<G1J> acc; DevBuf<uint32_t> d_ok, d_ident, d_failed; DevBuf<uint8_t> d_out;   // freed on every return path
    int rc;
    if ((rc = acc.alloc(2)) || (rc = d_ok.alloc(1)) || (rc = d_out.alloc(128)) || (rc = d_ident.alloc(2)) || (rc = d_failed.alloc(1))) return rc;
    uint32_t okv = 0, failed = 0; uint8_t outb[128];
    if ((rc = fold_records_enqueue(s, device_accumulators, (uint32_t)n_parts, 1, 1, 0, acc.p, nullptr, nullptr, d_failed.p))) return rc;   // whole points: records in pieces are put together
    if ((rc = pairing_check_enqueue(s, ctx->pairing, acc.p, 1, d_ok.p))) return rc;
    if ((rc = point_to_bytes_enqueue(s, acc.p, d_out.p, d_ident.p, 2))) return rc;
    H2V_HIP_CHECK(hipMemcpyAsync(&okv, d_ok.p, 4, hipMemcpyDeviceToHost, s));
    H2V_HIP_CHECK(hipMemcpyAsync(&failed, d_failed.p, 4, hipMemcpyDeviceToHost, s));
    H2V_HIP_CHECK(hipMemcpyAsync(outb, d_out.p, 128, hipMemcpyDeviceToHost, s));
    H2V_HIP_CHECK(hipStreamSynchronize(s));
    *ok = (okv && !failed) ? 1 : 0;
    if (pairing_ok) *pairing_ok = okv ? 1 : 0;
    if (out_left_xy) memcpy(out_left_xy, outb, 64);
    if (out_right_xy) memcpy(out_right_xy, outb + 64, 64);
    return 0;
}

// N x verify_proof with per-proof instance shapes (lib.rs:33-49 takes `instances` per call) and, in h2v_verify_batch_keys, per-proof
// VerifyingKeys (lib.rs:33-49 takes `vk` per call too; kzg/strategy.rs:125-140 only ever sees MSMs): proofs are grouped by (key, shape)
// (one compiled plan each), every group runs as its own batch without a pairing on its key's scratch batch, and the groups' accumulator
// records are folded into the single pairing.  The multiplier of proof i is the product of the draws of ALL later proofs in call order
// (kzg/strategy.rs:129, msm.rs:173-176), whatever group they fall in: the suffix products are computed once over the whole
// sequence and every group gathers its own.
// The instance shapes of a call are chosen by whoever supplies the proofs, and every distinct shape costs a plan compilation
// (O(program length^2) host work, ~10 device uploads) and may grow the batch's buffers: a call takes at most
// H2V_MAX_SHAPES_PER_CALL distinct (key, shape) groups (H2V_ERR_UNSUPPORTED beyond), the groups of a key share ONE batch object, and
// the plans go through the context's bounded cache (H2V_MAX_CACHED_PLANS, least recently used out).
// (H2V_MAX_SHAPES_PER_CALL: batch.h)

// the (key, shape) groups of a call in first-appearance order; every key index and every pointer the groups will read is checked here
int group_proofs(const char* who, size_t n, size_t n_keys, const uint32_t* key_of_proof, const size_t* n_instance_columns, const size_t* col_lens,
                 const uint8_t* const* proofs, const uint8_t* const* instances32, std::vector<CallGroup>& groups) {
    std::map<std::pair<size_t, std::vector<size_t>>, size_t> group_of;
    const size_t* cl = col_lens;
    size_t last = 0;   // the previous proof's group: runs of one key and shape (the common case) skip the map
    for (size_t i = 0; i < n; ++i) {
        const size_t k = key_of_proof ? key_of_proof[i] : 0;
        if (k >= n_keys) { set_last_error(std::string(who) + ": key index out of range"); return H2V_ERR_BAD_ARGUMENT; }
        const size_t nc = n_instance_columns[k];
        if (nc && !col_lens) { set_last_error(std::string(who) + ": null argument"); return H2V_ERR_BAD_ARGUMENT; }
        const size_t* shape_at = cl;
        cl += nc;
        if (!proofs[i]) { set_last_error(std::string(who) + ": null proof pointer"); return H2V_ERR_BAD_ARGUMENT; }
        size_t values = 0;
        for (size_t c = 0; c < nc; ++c) values += shape_at[c];
        if (values && (!instances32 || !instances32[i])) { set_last_error(std::string(who) + ": null instances pointer"); return H2V_ERR_BAD_ARGUMENT; }
        if (i && groups[last].key == k && groups[last].shape.size() == nc && std::equal(shape_at, shape_at + nc, groups[last].shape.begin())) {
            groups[last].idx.push_back(i);
            continue;
        }
        std::pair<size_t, std::vector<size_t>> key(k, std::vector<size_t>(shape_at, shape_at + nc));
        auto it = group_of.find(key);
        if (it == group_of.end()) {
            if (groups.size() == H2V_MAX_SHAPES_PER_CALL) { set_last_error(std::string(who) + ": more than 64 distinct (key, instance shape) groups in one call"); return H2V_ERR_UNSUPPORTED; }
            groups.push_back({k, key.second, {}});
            it = group_of.emplace(std::move(key), groups.size() - 1).first;
        }
        last = it->second;
        groups[last].idx.push_back(i);
    }
    return 0;
}

}  // namespace

namespace h2v {

// What a grouped call holds until it returns: every context's lock and scratch batch (ctxs[k]'s: hold[k]), the batches made for the
// call (identification), and the batch every group ran on
struct GroupsHeld {
    std::vector<std::unique_ptr<ScratchBatch>> hold;
    struct Destroy { void operator()(h2v_batch* b) const { h2v_batch_destroy(b); } };
    std::vector<std::unique_ptr<h2v_batch, Destroy>> own;
    std::vector<h2v_batch*> on;
};
void GroupsHeldDelete::operator()(GroupsHeld* h) const { delete h; }

// The argument checks of a grouped call, every one before the first HIP call, and its (key, shape) groups.  `who` names the entry point
// in the error messages.
int grouped_call_args(const char* who, h2v_ctx* const* ctxs, size_t n_keys, const uint32_t* key_of_proof, size_t n, const uint8_t* const* proofs,
                      const size_t* proof_lens, const uint8_t* const* instances32, const size_t* n_instance_columns, const size_t* col_lens,
                      std::vector<CallGroup>& groups) {
    const std::string w(who);
    if (!ctxs || !n_keys || !n_instance_columns || (n && (!proofs || !proof_lens))) { set_last_error(w + ": null argument"); return H2V_ERR_BAD_ARGUMENT; }
    for (size_t k = 0; k < n_keys; ++k) {
        if (!ctxs[k]) { set_last_error(w + ": null context"); return H2V_ERR_BAD_ARGUMENT; }
        if (!ctxs[k]->vk) { set_last_error(w + ": a context was created without a VerifyingKey"); return H2V_ERR_BAD_ARGUMENT; }
        for (size_t j = 0; j < k; ++j) if (ctxs[j] == ctxs[k]) { set_last_error(w + ": the same context twice"); return H2V_ERR_BAD_ARGUMENT; }
        if (ctxs[k]->device != ctxs[0]->device) { set_last_error(w + ": contexts on different devices"); return H2V_ERR_BAD_ARGUMENT; }
        if (!same_srs(ctxs[k]->params, ctxs[0]->params)) { set_last_error(w + ": contexts over different params (g[0], g2 or s_g2 differ)"); return H2V_ERR_BAD_ARGUMENT; }
    }
    for (size_t k = 0; k < n_keys; ++k) if (n_instance_columns[k] != ctx_total_instance_columns(ctxs[k])) { set_last_error(w + ": instances do not match a VK's instance column count"); return H2V_ERR_INVALID_INSTANCES; }
    return group_proofs(who, n, n_keys, key_of_proof, n_instance_columns, col_lens, proofs, instances32, groups);
}

// The groups of a call on their keys' scratch batches (ctxs[k]'s; keys without a group are not touched), their records (whole points:
// export_whole_records) written to d_records, H2V_ACC_RECORD_BYTES per group in the groups' order.  rand32: the n draws in call order
// (resolved).  Every context's lock and scratch batch is taken for the whole call and handed to the caller in `held` (released when it
// goes); the whole-sequence multipliers are computed on the first group's context's stream.
// Keys do not wait for each other on the host: each round enqueues one group of every key (upload, launch without a pairing, record
// export on that key's batch stream), then finishes them; groups of one key run one after another on its batch.  When the call
// returns 0 every group is finished — the records are written — st[g] holds group g's statuses and all_ok says whether all are 0.
// resident (identification): every group stays resident — a key's first group on its scratch batch, its later groups on batches made
// for the call (held->own, destroyed with `held`).
int run_group_batches(h2v_ctx* const* ctxs, size_t n_keys, const std::vector<CallGroup>& groups, size_t n, const uint8_t* const* proofs, const size_t* proof_lens,
                      const uint8_t* const* instances32, const uint8_t* rand32, uint8_t* d_records, bool resident, GroupsHeldPtr& held,
                      std::vector<std::vector<int>>& st, bool& all_ok, const CallHints& hints) {
    held.reset(new GroupsHeld);
    // every context's lock and scratch batch for the whole call, taken in one global order (by address): calls over overlapping sets of
    // contexts cannot deadlock
    std::vector<size_t> order(n_keys);
    for (size_t k = 0; k < n_keys; ++k) order[k] = k;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return std::less<const h2v_ctx*>()(ctxs[a], ctxs[b]); });
    std::vector<std::unique_ptr<ScratchBatch>>& hold = held->hold;
    hold.resize(n_keys);
    for (size_t k : order) hold[k].reset(new ScratchBatch(ctxs[k]));
    h2v_ctx* fold_ctx = ctxs[groups[0].key];
    H2V_HIP_CHECK(hipSetDevice(fold_ctx->device));
    int rc;
    // the groups of every key, and each group's proof indices at its offset of one index array
    std::map<size_t, std::vector<size_t>> of_key;
    std::vector<uint32_t> idx32;
    std::vector<size_t> idx_off(groups.size());
    size_t rounds = 0;
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        std::vector<size_t>& kg = of_key[groups[gi].key];
        kg.push_back(gi);
        rounds = std::max(rounds, kg.size());
        idx_off[gi] = idx32.size();
        idx32.insert(idx32.end(), groups[gi].idx.begin(), groups[gi].idx.end());
    }
    // whole-sequence multipliers on the folding context's stream.  A call of ONE group needs none: the whole sequence is the group's own
    // (its proofs are the call's, in call order), and the group's upload makes exactly these multipliers from the draws themselves —
    // no buffers, no second multiplier pass, no wait (a resident accumulator's leg of one key and one shape; the one-pairing entry
    // points hand such a call to h2v_verify_batch and never come here with one group)
    const bool own_draws = groups.size() == 1;
    DevBuf<uint8_t> d_rand; DevBuf<Fr> d_mult, d_tiles; DevBuf<uint32_t> d_idx;
    if (!own_draws) {
        const GroupShape whole{1, (uint32_t)n, (uint32_t)n, nullptr};
        if ((rc = d_tiles.alloc(multipliers_scratch(whole))) || (rc = d_rand.alloc(32 * n)) || (rc = d_mult.alloc(n)) || (rc = d_idx.alloc(n))) return rc;
        H2V_HIP_CHECK(hipMemcpyAsync(d_rand.p, rand32, 32 * n, hipMemcpyHostToDevice, fold_ctx->stream));
        H2V_HIP_CHECK(hipMemcpyAsync(d_idx.p, idx32.data(), 4 * n, hipMemcpyHostToDevice, fold_ctx->stream));
        if ((rc = multipliers_enqueue(fold_ctx->stream, whole, d_rand.p, nullptr, d_mult.p, d_tiles.p))) return rc;
        H2V_HIP_CHECK(hipStreamSynchronize(fold_ctx->stream));
    }
    // one batch object per key serves every shape group of that key (its buffers grow to the largest group's plan: ensure_buffers)
    for (auto& kv : of_key) {
        size_t max_group = 1, max_inst = 0;
        for (size_t gi : kv.second) { max_group = std::max(max_group, groups[gi].idx.size()); size_t t = 0; for (size_t l : groups[gi].shape) t += l; max_inst = std::max(max_inst, t); }
        if ((rc = hold[kv.first]->take(max_group, max_inst))) return rc;
    }
    // the batch of every group: its key's scratch batch, or (identification, a key's later groups) a batch of its own for the call
    std::vector<h2v_batch*>& on = held->on;
    on.resize(groups.size());
    for (auto& kv : of_key)
        for (size_t r = 0; r < kv.second.size(); ++r) {
            const size_t gi = kv.second[r];
            on[gi] = hold[kv.first]->b;
            if (!resident || r == 0) continue;
            size_t inst = 0;
            for (size_t l : groups[gi].shape) inst += l;
            h2v_batch* b = nullptr;
            if ((rc = h2v_batch_create(ctxs[kv.first], groups[gi].idx.size(), inst, &b))) return rc;
            held->own.emplace_back(b);
            on[gi] = b;
        }
    // on an error with work in flight: nothing returns (and frees the buffers above) before every batch's streams are idle
    struct Drain {
        std::vector<h2v_batch*> bs;
        ~Drain() { for (h2v_batch* b : bs) wait_for_streams(b); }
    } drain;
    drain.bs = on;
    all_ok = true;
    st.assign(groups.size(), std::vector<int>());
    for (size_t r = 0; r < rounds; ++r) {
        for (auto& kv : of_key) {
            if (r >= kv.second.size()) continue;
            const size_t gi = kv.second[r];
            const CallGroup& grp = groups[gi];
            ScratchBatch& sb = *hold[kv.first];
            const size_t m = grp.idx.size();
            if ((rc = pack_inputs(sb, m, grp.idx.data(), proofs, proof_lens, instances32, grp.shape.size(), grp.shape.data(), hints)) ||
                (rc = own_draws ? enqueue_group(sb, on[gi], 0, m, 1, rand32, 0)
                                : enqueue_group(sb, on[gi], 0, m, 1, unit_draws(m).data(), 0, false, d_mult.p, d_idx.p + idx_off[gi])) ||
                (rc = export_whole_records(on[gi], d_records + gi * H2V_ACC_RECORD_BYTES))) return rc;
        }
        for (auto& kv : of_key) {
            if (r >= kv.second.size()) continue;
            const size_t gi = kv.second[r];
            st[gi].assign(groups[gi].idx.size(), 0); int gok = 0;
            if ((rc = collect_group(*hold[kv.first], on[gi], 0, st[gi].data(), &gok))) return rc;
            all_ok = all_ok && gok;
        }
    }
    drain.bs.clear();   // (every group is finished)
    return 0;
}

}  // namespace h2v

namespace {

// A grouped call closed by its own pairing: the groups' records (run_group_batches) folded into ONE pairing on the first group's context.
// n_checks (identification, h2v_verify_batch_keys_identify): every group stays resident, and when the folded pairing itself fails, the
// failing proofs are searched for over all groups at once (identify_search); the number of range checks it ran is ADDED to *n_checks.
int run_groups(h2v_ctx* const* ctxs, size_t n_keys, const std::vector<CallGroup>& groups, size_t n, const uint8_t* const* proofs, const size_t* proof_lens,
               const uint8_t* const* instances32, const uint8_t* rand32, int* per_proof_status, int* batch_ok, uint8_t* out_left_xy, uint8_t* out_right_xy,
               size_t* n_checks = nullptr, const CallHints& hints = CallHints()) {
    h2v_ctx* fold_ctx = ctxs[groups[0].key];
    int rc;
    DevBuf<uint8_t> d_records;
    H2V_HIP_CHECK(hipSetDevice(fold_ctx->device));
    if ((rc = d_records.alloc(H2V_ACC_RECORD_BYTES * groups.size()))) return rc;
    GroupsHeldPtr held;   // (declared after d_records: the batches go, and the contexts are released, before the records are freed)
    std::vector<std::vector<int>> st;
    bool all_ok = true;
    if ((rc = run_group_batches(ctxs, n_keys, groups, n, proofs, proof_lens, instances32, rand32, d_records.p, n_checks != nullptr, held, st, all_ok, hints))) return rc;
    int ok = 0, pairing_ok = 0;
    if ((rc = fold_check_locked(fold_ctx, d_records.p, groups.size(), &ok, out_left_xy, out_right_xy, &pairing_ok))) return rc;
    // identification: only a failing pairing has failing proofs to find (a proof with a non-zero status contributes nothing to it)
    if (n_checks && !pairing_ok && (rc = identify_search(held->on, whole_batches(st), false, st, n_checks))) return rc;
    if (per_proof_status)
        for (size_t gi = 0; gi < groups.size(); ++gi)
            for (size_t j = 0; j < groups[gi].idx.size(); ++j) per_proof_status[groups[gi].idx[j]] = st[gi][j];
    if (batch_ok) *batch_ok = (ok && all_ok) ? 1 : 0;
    return 0;
}

// h2v_verify_batch on a context the caller has checked, with or without hint rows
int verify_one(h2v_ctx* ctx, size_t n, const uint8_t* const* proofs, const size_t* proof_lens, const uint8_t* const* instances32, size_t n_instance_columns,
               const size_t* col_lens, const uint8_t* rand32, int* per_proof_status, int* batch_ok, uint8_t* out_left_xy, uint8_t* out_right_xy, const CallHints& hints) {
    ScratchBatch sb(ctx);
    return pack_and_run(sb, n, proofs, proof_lens, instances32, n_instance_columns, col_lens, rand32, 1, false, per_proof_status, batch_ok, out_left_xy, out_right_xy, hints);
}

// h2v_verify_batch_keys, and h2v_verify_batch_shapes as its call with one context (key_of_proof NULL: every proof is of key 0).  `who`
// names the entry point in the error messages.  n_checks (h2v_verify_batch_keys_identify): identification as well — the draws must be
// non-zero, and the number of range checks is written there; one group is h2v_verify_batch_identify's case.
int verify_grouped(const char* who, h2v_ctx* const* ctxs, size_t n_keys, const uint32_t* key_of_proof, size_t n, const uint8_t* const* proofs,
                   const size_t* proof_lens, const uint8_t* const* instances32, const size_t* n_instance_columns, const size_t* col_lens, const uint8_t* rand32,
                   int* per_proof_status, int* batch_ok, uint8_t* out_left_xy, uint8_t* out_right_xy, size_t* n_checks = nullptr,
                   const CallHints& hints = CallHints()) {
    // every argument check comes before the first HIP call
    std::vector<CallGroup> groups;
    int rc;
    if ((rc = grouped_call_args(who, ctxs, n_keys, key_of_proof, n, proofs, proof_lens, instances32, n_instance_columns, col_lens, groups))) return rc;
    if (groups.empty()) groups.push_back({0, std::vector<size_t>(n_instance_columns[0], 0), {}});   // (no proofs: ctxs[0] over empty columns)
    std::vector<uint8_t> os_rand;
    if (n_checks) {
        // a single proof's check equals SingleStrategy's only when its multiplier is non-zero: no draw may be zero (refused before any device work)
        if ((rc = resolve_draws(rand32, n, os_rand, who, true))) return rc;
        size_t checks = 0;
        if (groups.size() == 1) {
            if ((rc = h2v_verify_batch_identify(ctxs[groups[0].key], n, proofs, proof_lens, instances32, groups[0].shape.size(), groups[0].shape.data(), rand32,
                                                per_proof_status, batch_ok, out_left_xy, out_right_xy, &checks))) return rc;
        } else if ((rc = run_groups(ctxs, n_keys, groups, n, proofs, proof_lens, instances32, rand32, per_proof_status, batch_ok, out_left_xy, out_right_xy, &checks)))
            return rc;
        *n_checks = checks;
        return 0;
    }
    if (groups.size() == 1)   // one key, one shape: the proofs are that group, in call order: h2v_verify_batch
        return verify_one(ctxs[groups[0].key], n, proofs, proof_lens, instances32, groups[0].shape.size(), groups[0].shape.data(), rand32,
                          per_proof_status, batch_ok, out_left_xy, out_right_xy, hints);
    if ((rc = resolve_draws(rand32, n, os_rand, who))) return rc;
    return run_groups(ctxs, n_keys, groups, n, proofs, proof_lens, instances32, rand32, per_proof_status, batch_ok, out_left_xy, out_right_xy, nullptr, hints);
}

}  // namespace

extern "C" {

int h2v_fold_check(h2v_ctx* ctx, const void* device_accumulators, size_t n_parts, int* ok, uint8_t out_left_xy[64], uint8_t out_right_xy[64]) {
    if (!ctx || !device_accumulators || !n_parts || !ok) { set_last_error("h2v_fold_check: bad argument"); return H2V_ERR_BAD_ARGUMENT; }
    std::lock_guard<std::mutex> lock(ctx->mu);
    return fold_check_locked(ctx, device_accumulators, n_parts, ok, out_left_xy, out_right_xy);
}

int h2v_verify_batch(h2v_ctx* ctx, size_t n, const uint8_t* const* proofs, const size_t* proof_lens, const uint8_t* const* instances32, size_t n_instance_columns,
                     const size_t* col_lens, const uint8_t* rand32, int* per_proof_status, int* batch_ok, uint8_t out_left_xy[64], uint8_t out_right_xy[64]) {
    if (!ctx) { set_last_error("null argument"); return H2V_ERR_BAD_ARGUMENT; }
    return verify_one(ctx, n, proofs, proof_lens, instances32, n_instance_columns, col_lens, rand32, per_proof_status, batch_ok, out_left_xy, out_right_xy, CallHints());
}

// AccumulatorStrategy::with(msm_accumulator) (kzg/strategy.rs:75-78): the strategy starts from an existing DualMSM — the
// reference's only pause / resume hook — instead of an empty one.  Every later process() scales the WHOLE accumulator by its fresh
// draw before the proof's Guard joins (strategy.rs:129), so the seed ends up scaled by the product of ALL n draws of this call:
// the seed's two channels are evaluated (two pooled MSMs with the scalars already multiplied by that product), written as a
// record, and folded with the batch's own record into the one pairing.
// n_checks (h2v_verify_batch_seeded_identify): identification as well.  The seed's terms belong to no proof, so the failing proofs
// are those of the batch's OWN record — record 0 of the fold, still in device memory: h2v_batch_identify checks it on its own and
// searches only when it fails.  seed_ok: the pairing of the evaluated seed alone (scaled by the product of the draws, which is
// non-zero: the verdict of the seed as it was given).  Nothing is written before the call's last step.
static int verify_seeded(const char* who, h2v_ctx* ctx, size_t n, const uint8_t* const* proofs, const size_t* proof_lens, const uint8_t* const* instances32,
                         size_t n_instance_columns, const size_t* col_lens, const uint8_t* rand32,
                         const uint8_t* seed_left_scalars32, const uint8_t* seed_left_bases64, size_t n_seed_left,
                         const uint8_t* seed_right_scalars32, const uint8_t* seed_right_bases64, size_t n_seed_right,
                         int* per_proof_status, int* batch_ok, uint8_t* out_left_xy, uint8_t* out_right_xy, int* seed_ok, size_t* n_checks) {
    const std::string w(who);
    if (!ctx || (n_seed_left && (!seed_left_scalars32 || !seed_left_bases64)) || (n_seed_right && (!seed_right_scalars32 || !seed_right_bases64))) {
        set_last_error(w + ": null argument"); return H2V_ERR_BAD_ARGUMENT;
    }
    if (n_seed_left > (1u << 24) || n_seed_right > (1u << 24)) { set_last_error(w + ": seed too large"); return H2V_ERR_BAD_ARGUMENT; }
    int rc;
    std::vector<uint8_t> os_rand;
    // (identification: a single proof's check equals SingleStrategy's only when its multiplier is non-zero)
    if ((rc = resolve_draws(rand32, n, os_rand, who, n_checks != nullptr))) return rc;
    // the product of this call's draws, and the seed's scalars times it (host: a few hundred Fr products)
    Fr M = Fr::one();
    for (size_t i = 0; i < n; ++i) { Fr r; Fr::from_bytes(rand32 + 32 * i, r); M = M * r; }
    std::vector<uint8_t> sc[2];
    const uint8_t* in_s[2] = {seed_left_scalars32, seed_right_scalars32};
    const size_t ns[2] = {n_seed_left, n_seed_right};
    for (int side = 0; side < 2; ++side) {
        sc[side].resize(32 * ns[side]);
        for (size_t j = 0; j < ns[side]; ++j) {
            Fr v;
            if (!Fr::from_bytes(in_s[side] + 32 * j, v)) { set_last_error(w + ": seed scalar not canonical"); return H2V_ERR_BAD_ARGUMENT; }
            (v * M).to_bytes(&sc[side][32 * j]);
        }
    }
    uint8_t seed_xy[128]; int ident = 0;
    // (before the scratch batch is taken: h2v_msm_g1 and h2v_pairing_check hold ctx->mu themselves)
    if ((rc = h2v_msm_g1(ctx, sc[0].data(), seed_left_bases64, n_seed_left, seed_xy, &ident))) return rc;         // (rejects bases that are not on the curve)
    if ((rc = h2v_msm_g1(ctx, sc[1].data(), seed_right_bases64, n_seed_right, seed_xy + 64, &ident))) return rc;
    int seed_passes = 1;   // (an empty seed: two identities)
    if (n_checks && (n_seed_left || n_seed_right) && (rc = h2v_pairing_check(ctx, seed_xy, seed_xy + 64, &seed_passes))) return rc;
    // the proofs: one batch without its pairing, kept for the fold
    ScratchBatch sb(ctx);
    std::vector<int> st(n ? n : 1, 0);
    if ((rc = pack_and_run(sb, n, proofs, proof_lens, instances32, n_instance_columns, col_lens, rand32, 0, false, st.data(), nullptr, nullptr, nullptr))) return rc;
    h2v_batch* b = sb.b;
    if (hipSetDevice(ctx->device) != hipSuccess) return H2V_ERR_DEVICE;
    DevBuf<uint8_t> d_xy, d_records; DevBuf<G1A> d_aff; DevBuf<G1J> d_jac; DevBuf<uint32_t> d_flags;
    if ((rc = d_xy.alloc(128)) || (rc = d_records.alloc(2 * H2V_ACC_RECORD_BYTES)) || (rc = d_aff.alloc(2)) || (rc = d_jac.alloc(2)) || (rc = d_flags.alloc(2))) return rc;
    hipStream_t s = b->stream;
    if (hipMemcpyAsync(d_xy.p, seed_xy, 128, hipMemcpyHostToDevice, s) != hipSuccess) { set_last_error(w + ": copy failed"); return H2V_ERR_DEVICE; }
    if ((rc = bases_from_bytes_enqueue(s, d_xy.p, d_aff.p, d_flags.p, 2))) return rc;
    if ((rc = affine_to_jacobian_enqueue(s, d_aff.p, d_jac.p, 2))) return rc;
    if ((rc = h2v_batch_export_accumulators(b, d_records.p))) return rc;                                                                  // record 0: the proofs of this call
    if ((rc = export_records_enqueue(s, d_jac.p, nullptr, 1, 0, nullptr, 0, 1, d_records.p + H2V_ACC_RECORD_BYTES))) return rc;   // record 1: the scaled seed
    if ((rc = h2v_batch_fold_check_enqueue(b, d_records.p, 2))) return rc;
    // (synchronises: the scoped buffers outlive their use)
    int ok = 0; uint8_t left[64], right[64];
    if ((rc = collect_group(sb, sb.b, 0, nullptr, &ok, left, right))) return rc;
    size_t checks = 0;
    if (n_checks) {
        // the statuses the device set; those pack_inputs forced (a short proof: its points undecodable, so never flagged) go over them
        int own_ok = 0;
        if ((rc = h2v_batch_identify(b, d_records.p, st.data(), &own_ok, &checks))) return rc;
    }
    for (size_t i = 0; i < n; ++i) if (sb.forced[i]) st[i] = sb.forced[i];
    if (per_proof_status) for (size_t i = 0; i < n; ++i) per_proof_status[i] = st[i];
    if (batch_ok) *batch_ok = ok;
    if (out_left_xy) memcpy(out_left_xy, left, 64);
    if (out_right_xy) memcpy(out_right_xy, right, 64);
    if (seed_ok) *seed_ok = seed_passes;
    if (n_checks) *n_checks = checks;
    return 0;
}

int h2v_verify_batch_seeded(h2v_ctx* ctx, size_t n, const uint8_t* const* proofs, const size_t* proof_lens, const uint8_t* const* instances32, size_t n_instance_columns,
                            const size_t* col_lens, const uint8_t* rand32,
                            const uint8_t* seed_left_scalars32, const uint8_t* seed_left_bases64, size_t n_seed_left,
                            const uint8_t* seed_right_scalars32, const uint8_t* seed_right_bases64, size_t n_seed_right,
                            int* per_proof_status, int* batch_ok, uint8_t out_left_xy[64], uint8_t out_right_xy[64]) {
    return verify_seeded("h2v_verify_batch_seeded", ctx, n, proofs, proof_lens, instances32, n_instance_columns, col_lens, rand32, seed_left_scalars32, seed_left_bases64,
                         n_seed_left, seed_right_scalars32, seed_right_bases64, n_seed_right, per_proof_status, batch_ok, out_left_xy, out_right_xy, nullptr, nullptr);
}

int h2v_verify_batch_seeded_identify(h2v_ctx* ctx, size_t n, const uint8_t* const* proofs, const size_t* proof_lens, const uint8_t* const* instances32,
                                     size_t n_instance_columns, const size_t* col_lens, const uint8_t* rand32,
                                     const uint8_t* seed_left_scalars32, const uint8_t* seed_left_bases64, size_t n_seed_left,
                                     const uint8_t* seed_right_scalars32, const uint8_t* seed_right_bases64, size_t n_seed_right,
                                     int* per_proof_status, int* batch_ok, int* seed_ok, uint8_t out_left_xy[64], uint8_t out_right_xy[64], size_t* n_range_checks) {
    size_t checks = 0;
    const int rc = verify_seeded("h2v_verify_batch_seeded_identify", ctx, n, proofs, proof_lens, instances32, n_instance_columns, col_lens, rand32, seed_left_scalars32,
                                 seed_left_bases64, n_seed_left, seed_right_scalars32, seed_right_bases64, n_seed_right, per_proof_status, batch_ok, out_left_xy, out_right_xy,
                                 seed_ok, &checks);
    if (!rc && n_range_checks) *n_range_checks = checks;
    return rc;
}

int h2v_verify_batch_shapes(h2v_ctx* ctx, size_t n, const uint8_t* const* proofs, const size_t* proof_lens, const uint8_t* const* instances32,
                            size_t n_instance_columns, const size_t* col_lens_per_proof, const uint8_t* rand32, int* per_proof_status, int* batch_ok,
                            uint8_t out_left_xy[64], uint8_t out_right_xy[64]) {
    // absent column lengths are refused before the VK checks, and a call without proofs has none to plan for (as h2v_verify_batch)
    if (ctx && n_instance_columns && (n ? !col_lens_per_proof : n_instance_columns == ctx_total_instance_columns(ctx))) { set_last_error("h2v_verify_batch_shapes: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    return verify_grouped("h2v_verify_batch_shapes", &ctx, 1, nullptr, n, proofs, proof_lens, instances32, &n_instance_columns, col_lens_per_proof, rand32,
                          per_proof_status, batch_ok, out_left_xy, out_right_xy);
}

int h2v_verify_batch_keys(h2v_ctx* const* ctxs, size_t n_keys, const uint32_t* key_of_proof, size_t n, const uint8_t* const* proofs, const size_t* proof_lens,
                          const uint8_t* const* instances32, const size_t* n_instance_columns, const size_t* col_lens, const uint8_t* rand32,
                          int* per_proof_status, int* batch_ok, uint8_t out_left_xy[64], uint8_t out_right_xy[64]) {
    if (n && !key_of_proof) { set_last_error("h2v_verify_batch_keys: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    return verify_grouped("h2v_verify_batch_keys", ctxs, n_keys, key_of_proof, n, proofs, proof_lens, instances32, n_instance_columns, col_lens, rand32,
                          per_proof_status, batch_ok, out_left_xy, out_right_xy);
}

// (include/h2v_hints.h)  The counters are the call's own until it has succeeded
int h2v_verify_batch_keys_hinted(h2v_ctx* const* ctxs, size_t n_keys, const uint32_t* key_of_proof, size_t n, const uint8_t* const* proofs, const size_t* proof_lens,
                                 const uint8_t* const* hint_rows, const uint8_t* const* instances32, const size_t* n_instance_columns, const size_t* col_lens,
                                 const uint8_t* rand32, int* per_proof_status, int* batch_ok, uint8_t out_left_xy[64], uint8_t out_right_xy[64], size_t hint_stats[3]) {
    if (n && !key_of_proof) { set_last_error("h2v_verify_batch_keys_hinted: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    size_t stats[3] = {0, 0, 0};
    const int rc = verify_grouped("h2v_verify_batch_keys_hinted", ctxs, n_keys, key_of_proof, n, proofs, proof_lens, instances32, n_instance_columns, col_lens, rand32,
                                  per_proof_status, batch_ok, out_left_xy, out_right_xy, nullptr, CallHints{hint_rows, hint_stats ? stats : nullptr});
    if (!rc && hint_stats) memcpy(hint_stats, stats, sizeof stats);
    return rc;
}

int h2v_verify_batch_keys_identify(h2v_ctx* const* ctxs, size_t n_keys, const uint32_t* key_of_proof, size_t n, const uint8_t* const* proofs,
                                   const size_t* proof_lens, const uint8_t* const* instances32, const size_t* n_instance_columns, const size_t* col_lens,
                                   const uint8_t* rand32, int* per_proof_status, int* batch_ok, uint8_t out_left_xy[64], uint8_t out_right_xy[64],
                                   size_t* n_range_checks) {
    if (n && !key_of_proof) { set_last_error("h2v_verify_batch_keys_identify: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    size_t checks = 0;
    const int rc = verify_grouped("h2v_verify_batch_keys_identify", ctxs, n_keys, key_of_proof, n, proofs, proof_lens, instances32, n_instance_columns, col_lens,
                                  rand32, per_proof_status, batch_ok, out_left_xy, out_right_xy, &checks);
    if (!rc && n_range_checks) *n_range_checks = checks;
    return rc;
}

int h2v_verify_batch_identify(h2v_ctx* ctx, size_t n, const uint8_t* const* proofs, const size_t* proof_lens, const uint8_t* const* instances32, size_t n_instance_columns,
                              const size_t* col_lens, const uint8_t* rand32, int* per_proof_status, int* batch_ok, uint8_t out_left_xy[64], uint8_t out_right_xy[64],
                              size_t* n_range_checks) {
    if (n_range_checks) *n_range_checks = 0;
    if (!ctx) { set_last_error("null argument"); return H2V_ERR_BAD_ARGUMENT; }
    // a single proof's check equals SingleStrategy's only when its multiplier is non-zero: no draw may be zero
    std::vector<uint8_t> os_rand;
    int rc;
    if ((rc = resolve_draws(rand32, n, os_rand, "h2v_verify_batch_identify", true))) return rc;
    std::vector<std::vector<int>> st(1, std::vector<int>(n, 0));
    int ok = 0;
    ScratchBatch sb(ctx);
    if ((rc = pack_and_run(sb, n, proofs, proof_lens, instances32, n_instance_columns, col_lens, rand32, 1, false, st[0].data(), &ok, out_left_xy, out_right_xy))) return rc;
    size_t checks = 0;
    if (n && !pairing_passed(sb.b, 0) && (rc = identify_search({sb.b}, whole_batches(st), true, st, &checks))) return rc;
    if (per_proof_status) for (size_t i = 0; i < n; ++i) per_proof_status[i] = st[0][i];
    if (batch_ok) *batch_ok = ok;
    if (n_range_checks) *n_range_checks = checks;
    return 0;
}

int h2v_verify_each(h2v_ctx* ctx, size_t n, const uint8_t* const* proofs, const size_t* proof_lens, const uint8_t* const* instances32, size_t n_instance_columns,
                    const size_t* col_lens, int* per_proof_status) {
    if (!ctx) { set_last_error("null argument"); return H2V_ERR_BAD_ARGUMENT; }
    ScratchBatch sb(ctx);
    int rc;
    // SingleStrategy (kzg/strategy.rs:143-181) = an accumulator of ONE proof with multiplier 1 and its own pairing: run the
    // proofs as one-proof groups of grouped launches, at most MSM_MAX_PROBLEMS / 2 per launch
    const size_t per = MSM_MAX_PROBLEMS / 2;
    if ((rc = pack_inputs(sb, n, nullptr, proofs, proof_lens, instances32, n_instance_columns, col_lens)) ||
        (rc = sb.take(std::min(n ? n : 1, per), sb.pin.pd->host.n_instance_values))) return rc;
    for (size_t off = 0; off < n; off += per) {
        const size_t m = std::min(per, n - off);
        std::vector<int> st(m, 0), gok(m, 0);
        if ((rc = enqueue_group(sb, sb.b, off, m, m, unit_draws(m).data(), 1)) || (rc = collect_group(sb, sb.b, off, st.data(), gok.data()))) return rc;
        for (size_t i = 0; i < m; ++i) {
            if (st[i] == 0 && !gok[i]) st[i] = H2V_ERR_CONSTRAINT_SYSTEM_FAILURE;  // kzg/strategy.rs:171-175
            if (per_proof_status) per_proof_status[off + i] = st[i];
        }
    }
    return 0;
}

// Many AccumulatorStrategy batches of their own sizes: cut, in call order, into launches of unequal groups on the scratch batch
// (h2v_batch_set_group_sizes), each of at most MSM_MAX_PROBLEMS / 2 batches, H2V_BATCHES_LAUNCH_PROOFS proofs and MSM_MAX_PROBLEMS MSM sub-problems.  The budget is the size
// at which a grouped launch has long reached its rate (20 x 1024 proofs: DESIGN.md section 6) and whose buffers a context holds anyway for a
// batch of that size; a batch above it runs alone, as one equal group — exactly h2v_verify_batch's launch.
#define H2V_BATCHES_LAUNCH_PROOFS 16384u
static int verify_batches(const char* who, h2v_ctx* ctx, size_t n_batches, const size_t* batch_sizes, const uint8_t* const* proofs, const size_t* proof_lens,
                          const uint8_t* const* instances32, size_t n_instance_columns, const size_t* col_lens, const uint8_t* rand32, int* per_proof_status, int* batch_ok,
                          uint8_t* out_left_xy, uint8_t* out_right_xy, const CallHints& hints) {
    if (!ctx || (n_batches && (!batch_sizes || !batch_ok))) { set_last_error(std::string(who) + ": null argument"); return H2V_ERR_BAD_ARGUMENT; }
    size_t n = 0;
    for (size_t i = 0; i < n_batches; ++i) {
        if (!batch_sizes[i]) { set_last_error(std::string(who) + ": a batch of no proofs"); return H2V_ERR_BAD_ARGUMENT; }
        if (batch_sizes[i] > ((size_t)1 << 22) || n + batch_sizes[i] > ((size_t)1 << 30)) { set_last_error(std::string(who) + ": too many proofs"); return H2V_ERR_BAD_ARGUMENT; }
        n += batch_sizes[i];
    }
    int rc;
    std::vector<uint8_t> os_rand;
    if ((rc = resolve_draws(rand32, n, os_rand, who))) return rc;
    ScratchBatch sb(ctx);
    if ((rc = pack_inputs(sb, n, nullptr, proofs, proof_lens, instances32, n_instance_columns, col_lens, hints))) return rc;
    const Plan& pl = sb.pin.pd->host;
    // the launches: [first batch, batches, first proof, proofs].  A launch is closed by the batch count, by the proof budget, and where the
    // next batch would take the launch's MSM problems, cut into sub-problems, past what a launch holds — the rule an upload of unequal
    // groups is refused by (upload_impl): every launch cut here passes it, and a batch left alone runs as one equal group
    struct Cut { size_t i0, k, off, m; };
    std::vector<Cut> cuts;
    size_t capacity = 1;
    const bool no_split = ctx->tuning.msm_no_term_split != 0;   // (then nothing is cut and nothing refused)
    for (size_t i = 0, off = 0; i < n_batches;) {
        Cut c{i, 0, off, 0};
        while (i < n_batches && c.k < MSM_MAX_PROBLEMS / 2 && (!c.k || c.m + batch_sizes[i] <= H2V_BATCHES_LAUNCH_PROOFS) &&
               (!c.k || no_split || groups_cut_within_limit(pl, batch_sizes + c.i0, c.k + 1))) { c.m += batch_sizes[i]; ++c.k; ++i; }
        off += c.m; capacity = std::max(capacity, c.m);
        cuts.push_back(c);
    }
    if ((rc = sb.take(capacity, pl.n_instance_values))) return rc;
    for (const Cut& c : cuts) {
        // (one batch alone: the equal-groups launch, whatever its size)
        if ((rc = c.k == 1 ? h2v_batch_set_groups(sb.b, 1) : h2v_batch_set_group_sizes(sb.b, batch_sizes + c.i0, c.k)) ||
            (rc = upload_impl(sb.b, c.m, sb.flat.data() + c.off * pl.proof_len, pl.proof_len, sb.iflat.data() + c.off * (size_t)pl.n_instance_values * 32, sb.cols.size(),
                              sb.cols.data(), rand32 + 32 * c.off, c.m)) ||
            (rc = place_hints(sb, sb.b, c.off, c.m)) || (rc = launch_impl(sb.b, 1)) ||
            (rc = collect_group(sb, sb.b, c.off, per_proof_status ? per_proof_status + c.off : nullptr, batch_ok + c.i0, out_left_xy ? out_left_xy + 64 * c.i0 : nullptr,
                                out_right_xy ? out_right_xy + 64 * c.i0 : nullptr))) return rc;
    }
    return 0;
}

int h2v_verify_batches(h2v_ctx* ctx, size_t n_batches, const size_t* batch_sizes, const uint8_t* const* proofs, const size_t* proof_lens, const uint8_t* const* instances32,
                       size_t n_instance_columns, const size_t* col_lens, const uint8_t* rand32, int* per_proof_status, int* batch_ok, uint8_t* out_left_xy,
                       uint8_t* out_right_xy) {
    return verify_batches("h2v_verify_batches", ctx, n_batches, batch_sizes, proofs, proof_lens, instances32, n_instance_columns, col_lens, rand32, per_proof_status, batch_ok,
                          out_left_xy, out_right_xy, CallHints());
}
int h2v_verify_batches_hinted(h2v_ctx* ctx, size_t n_batches, const size_t* batch_sizes, const uint8_t* const* proofs, const size_t* proof_lens,
                              const uint8_t* const* hint_rows, const uint8_t* const* instances32, size_t n_instance_columns, const size_t* col_lens,
                              const uint8_t* rand32, int* per_proof_status, int* batch_ok, uint8_t* out_left_xy, uint8_t* out_right_xy, size_t hint_stats[3]) {
    size_t stats[3] = {0, 0, 0};
    const int rc = verify_batches("h2v_verify_batches_hinted", ctx, n_batches, batch_sizes, proofs, proof_lens, instances32, n_instance_columns, col_lens, rand32,
                                  per_proof_status, batch_ok, out_left_xy, out_right_xy, CallHints{hint_rows, hint_stats ? stats : nullptr});
    if (!rc && hint_stats) memcpy(hint_stats, stats, sizeof stats);
    return rc;
}

int h2v_guard_msm(h2v_ctx* ctx, const uint8_t* proof, size_t proof_len, const uint8_t* instances32, size_t n_instance_columns, const size_t* col_lens,
                  uint8_t* right_scalars32, uint8_t* right_bases64, size_t* n_right, uint8_t* left_scalars32, uint8_t* left_bases64, size_t* n_left,
                  uint8_t* challenges32, size_t* n_challenges) {
    if (!ctx || !proof || !n_right || !n_left) { set_last_error("h2v_guard_msm: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    int st = 0;
    ScratchBatch sb(ctx);
    if (int rc = pack_and_run(sb, 1, &proof, &proof_len, &instances32, n_instance_columns, col_lens, unit_draws(1).data(), 0, true, &st, nullptr, nullptr, nullptr)) return rc;
    if (st != 0) return st;
    const h2v_batch* b = sb.b;
    const Plan& pl = b->plan->host;
    size_t T = pl.right_term_order.size(), TL = pl.left_term_order.size();
    if (T > *n_right || TL > *n_left) { set_last_error("h2v_guard_msm: output capacity too small"); return H2V_ERR_BAD_ARGUMENT; }
    std::vector<uint32_t> lscal((size_t)pl.n_points * 8), scal((size_t)pl.n_points * 8);
    std::vector<Fr> shared(pl.n_shared);
    std::vector<G1A> pts(pl.n_points + pl.n_shared);
    std::vector<Fr> chal(pl.squeeze_at.size());
    if (hipMemcpy(lscal.data(), b->left_scal.p, lscal.size() * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(scal.data(), b->msm_scal.p, scal.size() * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(shared.data(), b->shared.p, sizeof(Fr) * pl.n_shared, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(pts.data(), b->pts.p, sizeof(G1A) * pts.size(), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(chal.data(), b->chal.p, sizeof(Fr) * chal.size(), hipMemcpyDeviceToHost) != hipSuccess) return H2V_ERR_DEVICE;
    auto put_pt = [](const G1A& p, uint8_t* o) { if (p.is_identity()) memset(o, 0, 64); else { p.x.to_bytes(o); p.y.to_bytes(o + 32); } };
    if (!pl.guard_term_order.empty()) {
        // GWC: term by term as the reference appends them (gwc.rs:86-132), each with its own scalar
        T = pl.guard_term_order.size();
        if (T > *n_right) { set_last_error("h2v_guard_msm: output capacity too small"); return H2V_ERR_BAD_ARGUMENT; }
        std::vector<uint32_t> gs(T * 8);
        if (hipMemcpy(gs.data(), b->guard_scal.p, gs.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return H2V_ERR_DEVICE;
        for (size_t t = 0; t < T; ++t) {
            auto w = pl.guard_term_order[t];
            memcpy(right_scalars32 + 32 * t, &gs[t * 8], 32);
            put_pt(pts[w.first ? pl.n_points + w.second : w.second], right_bases64 + 64 * t);
        }
    } else
    for (size_t t = 0; t < T; ++t) {
        auto w = pl.right_term_order[t];
        if (w.first) { shared[w.second].to_bytes(right_scalars32 + 32 * t); put_pt(pts[pl.n_points + w.second], right_bases64 + 64 * t); }
        else { memcpy(right_scalars32 + 32 * t, &scal[(size_t)w.second * 8], 32); put_pt(pts[w.second], right_bases64 + 64 * t); }
    }
    *n_right = T;
    for (size_t t = 0; t < TL; ++t) {
        uint32_t slot = pl.left_term_order[t].second;
        memcpy(left_scalars32 + 32 * t, &lscal[(size_t)slot * 8], 32);
        put_pt(pts[slot], left_bases64 + 64 * t);
    }
    *n_left = TL;
    if (challenges32 && n_challenges) {
        // reorder squeeze order -> [user challenges.., theta, beta, gamma, y, x, y', v, u]
        size_t nc = pl.n_challenges;
        if (nc > *n_challenges) { set_last_error("h2v_guard_msm: challenge capacity too small"); return H2V_ERR_BAD_ARGUMENT; }
        memset(challenges32, 0, 32 * nc);   // a user challenge that is never squeezed stays zero, as in the reference (lib.rs:89-108)
        for (size_t q = 0; q < chal.size(); ++q) chal[q].to_bytes(challenges32 + 32 * pl.squeeze_order[q]);
        *n_challenges = nc;
    }
    return 0;
}

}  // extern "C"
