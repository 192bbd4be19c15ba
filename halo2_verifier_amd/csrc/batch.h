// The batch object behind h2v_batch and the argument blocks of the per-proof kernels.
#pragma once
#include "ctx.h"
#include "vkplan.h"
#include <algorithm>
#include <memory>

namespace h2v {

// Per-proof status words on the device.  The reference stops at the FIRST failing step of verify_proof, so when several
// kernels (or several lanes of one) find different faults in one proof the earliest step of the reference's sequence must
// win, whatever order the lanes run in: instance values are typed Fr before the call (lib.rs:33-49), then the main transcript
// reads (Error::Transcript, lib.rs:91-253), then the inversions of the evaluation part (the reference panics: vanishing.rs:100,
// domain.rs:187-212), then the multi-open reads (Error::Opening, lib.rs:420-424).  Every writer uses atomicMin on these
// rank-coded values; the host translates them back to the ABI's codes (status_decode).
#define H2V_DEV_ST_INVALID_INSTANCES (-40)
#define H2V_DEV_ST_TRANSCRIPT (-30)
#define H2V_DEV_ST_PANIC (-20)
#define H2V_DEV_ST_OPENING (-10)
__device__ __forceinline__ void status_set(int* status, uint32_t p, int dev_code) { atomicMin(&status[p], dev_code); }
// a status word that another wave of the same kernel may have set (the Fr program's inversion, ordered before this read by a
// workgroup barrier): read at device scope, past the CU's vector cache, like the atomic that wrote it
__device__ __forceinline__ int status_get(const int* status, uint32_t p) { return __hip_atomic_load(&status[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__host__ __device__ inline int status_decode(int dev) {
    switch (dev) {
        case 0: return 0;
        case H2V_DEV_ST_INVALID_INSTANCES: return H2V_ERR_INVALID_INSTANCES;
        case H2V_DEV_ST_TRANSCRIPT: return H2V_ERR_TRANSCRIPT;
        case H2V_DEV_ST_PANIC: return H2V_ERR_REFERENCE_PANIC;
        case H2V_DEV_ST_OPENING: return H2V_ERR_OPENING;
        default: return dev;
    }
}

struct FrvmArgs {
    const VmInstr* code; uint32_t n_code;   // the program as ONE stream (k_frvm)
    const Fr* consts;
    Fr* slots;
    uint32_t n;
    const uint8_t* proofs; uint32_t proof_len; const uint32_t* scalar_offsets;
    const uint8_t* inst; uint32_t ninst;
    const Fr* chal; const Fr* mult;
    int* status;
    uint32_t* msm_scal; uint32_t np;
    Fr* shared;
    uint32_t* left_scal;
    const Fr* insteval;   // [query][proof], wide instance vectors only
    uint32_t* guard_scal; uint32_t n_guard;   // [proof][term][8], guard variant of a GWC plan only (h2v_guard_msm)
    // the same program as 2 / 3 / 4 instruction streams per proof (k_frvm2; index K - 2, slot numbering of its own): frvm_enqueue chooses
    const VmInstr* code_k[3][FRVM_MAX_STREAMS] = {{nullptr}}; uint32_t n_code_k[3][FRVM_MAX_STREAMS] = {{0}}; uint32_t n_slots_k[3] = {0, 0, 0};
    uint32_t streams = 0;   // set by frvm_enqueue: the K the launch uses
    int force_streams = 0, force_lds_kb = 0;   // h2v_tuning (0 = automatic)
};

// sum_j inst[base + j] * l_{j - rot}(x) for one instance query of every proof (lib.rs:173-218; l_i_range poly/domain.rs:187-212)
struct InstEvalArgs {
    const uint8_t* inst; uint32_t ninst;      // canonical instance bytes [proof][ninst][32]
    const Fr* chal; uint32_t x_chal;          // challenges [c][proof]; index of x
    uint32_t n, k;                            // proofs; domain size 2^k
    uint32_t base, len;                       // the query's column inside a proof's instance values
    Fr w_start, omega, omega_step, omega_step_inv, n_inv;   // omega^(-rot), omega, omega^256, omega^(-256), 1/2^k
    Fr* out;                                  // [proof]
    int* status;
};
int instance_eval_enqueue(hipStream_t s, const InstEvalArgs& a);

// 64-bit words a proof's absorbed stream of `stream_len` bytes takes in the `words` buffer: whole hash blocks (136-byte Keccak /
// 128-byte Blake2b), plus room for a final partial one.  The rule of batch_sizes, and of whoever fills a StageArgs by hand.
inline uint32_t stream_words_for(size_t stream_len, int transcript) {
    const uint32_t words = (uint32_t)((stream_len + 7) / 8);
    const uint32_t blockw = transcript == H2V_TRANSCRIPT_KECCAK256 ? 17 : 16;
    return (words + blockw) / blockw * blockw;
}
struct StageArgs {
    uint32_t n;
    const Plan* plan; const PlanDevice* pd;
    const uint8_t* proofs; const uint8_t* inst;
    G1A* pts; G1A* phi; uint8_t* ycanon; int* status;
    unsigned long long* words; uint32_t stream_words;
    Fr* chal;
    // point hints (include/h2v_hints.h): the claimed canonical y of every point, [proof][point][32] like ycanon (and possibly ycanon
    // itself: a workgroup reads its own 64 rows before it writes them), and the word that counts the hints not used.  Null: no hints,
    // decompress_range_enqueue launches k_decompress as ever.
    uint32_t* hint_misses = nullptr;
    const uint8_t* hints = nullptr;
    // the miss list of a stage with hints: one word per point of the stage, and the word that counts a piece's entries (cleared on the
    // stream by every decompress_range_enqueue).  A wave with a hit and a miss lists its misses, and k_decompress_misses takes their
    // roots densely right behind.  A stage with hints has both (decompress_range_enqueue refuses it otherwise); without hints, null.
    uint32_t* miss_list = nullptr;
    uint32_t* miss_list_count = nullptr;
};

// the decompression stage in pieces (h2v_batch_upload_launch runs them around its copies): reset the status words; decompress the points of proofs [p0, p1); check the
// scalars of all proofs.  A stage with hints: _range launches k_decompress_hinted with k_decompress_misses behind it (the miss word is
// cleared by _begin or by the launch) and leaves its range complete all the same.
int decompress_begin_enqueue(hipStream_t s, const StageArgs& g);
int decompress_range_enqueue(hipStream_t s, const StageArgs& g, uint32_t p0, uint32_t p1);
int decompress_finish_enqueue(hipStream_t s, const StageArgs& g);
int transcript_stage_enqueue(hipStream_t s, const StageArgs& g);
// The groups of one upload: which proofs and which draws belong to group g.  One plain struct for host code and kernels (a kernel
// takes it by value); everything that must know where a group starts, how long it is or whose a proof is asks it.
//   off null      G equal groups (h2v_batch_set_groups) of gs proofs and nt >= gs draws each (nt > gs: a shard's tail): group g owns
//                 the proofs [g gs, (g + 1) gs) and the draws [g nt, (g + 1) nt)
//   off[0 .. G]   groups of unequal size (h2v_batch_set_group_sizes), host or device memory as the reader needs: group g owns the
//                 proofs [off[g], off[g + 1]) and the same draws, one per proof; gs = nt = off[G], all the proofs, so that fits()
//                 looks into no array
struct GroupShape {
    uint32_t G, gs, nt; const uint32_t* off;
    static GroupShape equal(uint32_t G, uint32_t n, uint32_t n_tail) { return GroupShape{G, n / G, n_tail / G, nullptr}; }
    static GroupShape unequal(uint32_t G, uint32_t n, const uint32_t* off) { return GroupShape{G, n, n, off}; }
    __host__ __device__ uint32_t first(uint32_t g) const { return off ? off[g] : g * gs; }
    __host__ __device__ uint32_t count(uint32_t g) const { return off ? off[g + 1] - off[g] : gs; }
    __host__ __device__ uint32_t draw_first(uint32_t g) const { return off ? off[g] : g * nt; }
    __host__ __device__ uint32_t of(uint32_t proof) const { return owner(proof, gs); }   // proof < n
    struct Draw { uint32_t g, j; };
    __host__ __device__ Draw draw_at(uint32_t i) const { const uint32_t g = owner(i, nt); return Draw{g, i - draw_first(g)}; }   // draw i < n_tail is the j-th of group g
    // A zero draw zeroes the multipliers of every earlier proof of its group: the j-th draw of group g, when zero, leaves the group's
    // proofs [0, zero_below(j, g)) with a zero multiplier (an equal group's draws past its proofs, a shard's tail, zero them all)
    __host__ __device__ uint32_t zero_below(uint32_t j, uint32_t g) const { const uint32_t c = count(g); return j < c ? j : c; }
    uint32_t largest() const { uint32_t m = off ? 0 : gs; for (uint32_t g = 0; off && g < G; ++g) m = std::max(m, count(g)); return m; }
    // What keeps an upload of n proofs and n_tail draws (have_tail false: no draws of the caller's, n_tail is not looked at) from having
    // this shape, in the words of the upload's error messages; null: it fits
    const char* misfit(size_t n, size_t n_tail, bool have_tail) const {
        if (have_tail && n_tail < n) return "n_tail < n";
        if (off) {
            if (n != gs) return "n is not the sum of the group sizes (h2v_batch_set_group_sizes)";
            if (have_tail && n_tail != n) return "groups of unequal size take one draw per proof (n_tail == n)";
        } else if (n != (size_t)G * gs || (have_tail && n_tail != (size_t)G * nt)) return "n and n_tail must be multiples of the group count";
        return nullptr;
    }
    bool fits(size_t n, size_t n_tail, bool have_tail) const { return !misfit(n, n_tail, have_tail); }
private:
    // the group that owns index i: i / per for equal groups, else the last g with off[g] <= i (off[0] = 0, off[G] > i)
    __host__ __device__ uint32_t owner(uint32_t i, uint32_t per) const {
        if (!off) return i / per;
        uint32_t lo = 0, hi = G;
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (off[mid] <= i) lo = mid; else hi = mid; }
        return lo;
    }
};
// d_mult[p] = the product of the draws behind proof p's own inside p's group, for the draws d_tail of `shape` (off in device memory or
// not: only its presence is read): one segmented suffix scan over the whole draw array, work proportional to the draws whatever the
// sizes.  Unequal groups end where d_last[j] != 0 (one byte per draw, d_last[n - 1] != 0); equal groups end by arithmetic, d_last is
// not read and may be null.  d_scratch: multipliers_scratch(shape) elements.
size_t multipliers_scratch(const GroupShape& shape);
int multipliers_enqueue(hipStream_t s, const GroupShape& shape, const uint8_t* d_tail, const uint8_t* d_last, Fr* d_mult, Fr* d_scratch);
// The legs of a finished batch (k_leg_weights; h2v_accumulator_process_batch): with M_g = the product of group g's draws — the draw of
// its first proof, d_tail[32 shape.first(g) ..], times that proof's multiplier d_mult[shape.first(g)] (one draw per proof; off in
// device memory, read up to off[G - 1]) —
// d_weights <- [prod_g M_g, W_0 .. W_{G-1}], W_g = prod_{f > g} M_f, and d_legs <- [M_0 .. M_{G-1}], canonical 8-word scalars.
// 1 <= shape.G <= 512: one workgroup.
int leg_weights_enqueue(hipStream_t s, const GroupShape& shape, const uint8_t* d_tail, const Fr* d_mult, uint32_t* d_weights, uint32_t* d_legs);
// The kernels of an enqueued feed (h2v_accumulator_feed_batch, include/h2v_feed.h), all on the accumulator's stream.
// feed_gather (k_feed_gather, a workgroup per group): d_pairs <- [d_acc[0], d_acc[1], d_sums[0 .. 2 G)], the accumulator's pair and the
// batch's unscaled sums; d_sizes[g] <- shape.count(g), d_failed[g] <- the non-zero words among group g's d_status (off in device memory).
int feed_gather_enqueue(hipStream_t s, const G1J* d_acc, const G1J* d_sums, const int* d_status, const GroupShape& shape, G1J* d_pairs, uint32_t* d_sizes, uint32_t* d_failed);
// feed_weights (k_feed_weights): leg_weights_enqueue that fails closed on a draw the upload's kernel found >= r.  d_fault: the fault word
// of k_ingest_draws' verdict block (null: the host has checked the draws).  No fault: k_leg_weights' outputs and d_rc[0] <- 0.  A fault:
// d_weights <- [1, 0 .. 0] (the accumulator keeps its value, every leg is scaled away) and d_rc[0] <- H2V_ERR_BAD_ARGUMENT.
int feed_weights_enqueue(hipStream_t s, const GroupShape& shape, const uint8_t* d_tail, const Fr* d_mult, const uint32_t* d_fault, uint32_t* d_weights, uint32_t* d_legs,
                         uint32_t* d_rc);
// feed_report (k_feed_report), a feed's last kernel: the report [rc, n, G, failed][M_g x 8, size_g, failed_g] x G -> d_report, mapped
// pinned memory, by plain stores behind a system-scope fence.  H2V_FEED_REPORT_WORDS(G) words.
#define H2V_FEED_REPORT_WORDS(G) (4 + 10 * (size_t)(G))
int feed_report_enqueue(hipStream_t s, const uint32_t* d_rc, uint32_t n, uint32_t G, const uint32_t* d_legs, const uint32_t* d_sizes, const uint32_t* d_failed, uint32_t* d_report);
// out[i] = src[idx[i]]: the multipliers of a non-contiguous subset of a larger accumulation
int gather_multipliers_enqueue(hipStream_t s, const Fr* d_src, const uint32_t* d_idx, uint32_t n, Fr* d_out);
int frvm_enqueue(hipStream_t s, const FrvmArgs& a, uint32_t n_slots);
// d_msm_scal[(n np + g n_shared + j) 8 ..] = canonical( sum over the proofs p of group g of d_shared[j n + p] ), n the proofs of the
// upload (shape.off in device memory)
int fold_shared_enqueue(hipStream_t s, const GroupShape& shape, const Fr* d_shared, uint32_t n, uint32_t np, uint32_t n_shared, uint32_t* d_msm_scal);
// One range of a re-check (k_fold_ranges): proofs [first, first + count) of a batch whose VK-wide scalars are shared[j][p] (j <
// n_shared, p < n); its n_shared folded scalars go to rows [out, out + n_shared) of the output.  Ranges of one launch may belong to
// different batches (h2v_batches_recheck), so each carries its own batch's pointer and sizes.
struct FoldRange {
    const Fr* shared;
    uint32_t n, n_shared;
    uint32_t first, count;
    uint32_t out, pad;
};
// the same fold as fold_shared_enqueue over R ranges: d_out[(d_ranges[r].out + j) * 8] = canonical( sum over the proofs p of range r of
// its shared[j][p] ); max_shared >= every range's n_shared
int fold_shared_ranges_enqueue(hipStream_t s, const FoldRange* d_ranges, uint32_t n_ranges, uint32_t max_shared, uint32_t* d_out);

// The re-check of ranges of finished launches (h2v_batch_recheck, h2v_batches_recheck, on the first batch's): resources of its own,
// grow-only, so that the launches' accumulators, workspaces and result blocks are never touched
struct Recheck {
    MsmWorkspace ws;
    DevBuf<FoldRange> ranges;     // [range]
    DevBuf<uint32_t> fold;        // [range's rows][8]: the ranges' folded VK-wide scalars, one after another
    DevBuf<G1J> acc;              // [2 r] left, [2 r + 1] right
    DevBuf<uint32_t> ok;          // [range]
    DevBuf<uint8_t> out_bytes; DevBuf<uint32_t> out_ident;     // [range][128]; [2 range]
    DevBuf<uint32_t> failed;      // [group]: the failure counts of the records h2v_batch_identify puts together (read by nobody)
};

// The block of everything h2v_batch_finish reads back, in bytes, for G groups and n proofs: [ok G][fold_failed G][out_ident 2 G]
// [out_bytes 128 G][status n] (words, words, words, bytes, words).  One device block and one pinned host block share it: one copy
// per launch (four separate copies into pageable memory were ~0.13 ms of a 20-step launch).  The device block keeps the place of `ok`,
// unused: the verdicts are written into the host block, and the offsets of the two blocks agree.
struct ResultsLayout {
    size_t G, n;
    size_t ok() const { return 0; }
    size_t fold_failed() const { return 4 * G; }
    size_t out_ident() const { return 8 * G; }
    size_t out_bytes() const { return 16 * G; }
    size_t status() const { return 144 * G; }
    size_t total() const { return 144 * G + 4 * n; }
};
// The block at `base` as typed pointers: the device block, the pinned host block, or the host block's mapped device address.  The one
// place that says what lies at each offset.
struct ResultsPtrs { uint32_t* ok; uint32_t* fold_failed; uint32_t* out_ident; uint8_t* out_bytes; int* status; };
inline ResultsPtrs results_at(void* base, const ResultsLayout& L) {
    uint8_t* const p = static_cast<uint8_t*>(base);
    return ResultsPtrs{reinterpret_cast<uint32_t*>(p + L.ok()), reinterpret_cast<uint32_t*>(p + L.fold_failed()), reinterpret_cast<uint32_t*>(p + L.out_ident()),
                       p + L.out_bytes(), reinterpret_cast<int*>(p + L.status())};
}

// Where a batch is in its life.  An operation sets the stage as its last step, once it has succeeded; a failed upload, launch, finish or
// fold leaves the batch Empty, and the calls that need an upload or a launch refuse it until an upload succeeds.
enum class BatchStage { Empty, Uploaded, Launched, Finished };
struct LaunchRecord {           // what the last launch (or fold) left (close_enqueue)
    bool pairing = false;       // its pairing checks were enqueued: the `ok` words are its verdicts
    bool pieces = false;        // no pairing, accumulators in pieces only: acc / out_bytes are put together on demand (ensure_whole)
    bool tail_on_aux = false;   // whatever the stage: its whole accumulators, their bytes and the result copy are still on the auxiliary stream (join_tail)
    bool host_block = false;    // the launch itself sends the result block to the host (the pairing launch's tail workgroups, or the auxiliary stream)
    bool folded = false;        // a fold ran since the launch: acc / the pieces / the `ok` words are the folded records', not the launch's own
};
// The staged batch's steps (batch.hip) that the one-shot entry points (oneshot.hip) run on their scratch batches
int resolve_draws(const uint8_t*& rand32, size_t n, std::vector<uint8_t>& storage, const char* who, bool nonzero = false);
int upload_impl(h2v_batch* b, size_t n, const uint8_t* proofs_flat, size_t proof_len, const uint8_t* instances_flat, size_t ncols, const size_t* col_lens,
                const uint8_t* rand_tail, size_t n_tail, bool overlap = false, bool guard = false);
int launch_impl(h2v_batch* b, int with_pairing, const Fr* ext_mult = nullptr, const uint32_t* ext_idx = nullptr);
// `bytes` bytes from `p` on are device memory of `device`, inside one allocation, and p lies on a 16-byte boundary (who / does: the entry
// point and the verb of the error message): what every entry point that takes a caller's device pointer holds it to
int device_range_check(const void* p, size_t bytes, int device, const char* what, const char* who = "h2v_batch_upload_device", const char* does = "reads");
bool pairing_passed(const h2v_batch* b, uint32_t g);
// The gather of a batch's Guards (k_guards_gather, guards_out.hip; include/h2v_guards.h): the terms of one channel of the proofs
// [first, first + count) of an upload of n proofs with np point slots each, T terms per proof in the order d_order, one thread per
// (proof, term); output term i = (p - first) * T + t.  A slot term reads its 8 canonical words at d_slot_scal[(p np + slot) 8] and its
// base at d_pts[p np + slot]; a VK-wide term reads d_shared[j n + p] (Montgomery) and d_pts[n np + j].  A proof whose status word is
// non-zero gives zero scalars under the identity.  Either output may be null.  count * T < 2^31
// (H2V_ERR_UNSUPPORTED beyond); every index of d_order lies below np (kind 0) or the number of VK-wide bases (kind 1): the caller's.
struct GuardsGather {
    const GuardTerm* d_order; uint32_t T;
    const uint32_t* d_slot_scal; const Fr* d_shared; const G1A* d_pts; const int* d_status;
    uint32_t n, np, first, count;
};
// bytes: 32 canonical little-endian bytes per scalar, 64 bytes x | y per base (the identity all-zero); both on 16-byte boundaries
int guards_gather_bytes_enqueue(hipStream_t s, const GuardsGather& g, uint8_t* d_scalars32, uint8_t* d_bases64);
// object form: the 8 words and the G1A as they lie, for the arrays of a resident h2v_msm (d_words on a 16-byte boundary)
int guards_gather_terms_enqueue(hipStream_t s, const GuardsGather& g, uint32_t* d_words, G1A* d_bases);
// per proof of [first, first + count): d_mult32[32 j ..] = d_mult[first + j] as canonical bytes, d_status_out[j] = status_decode(d_status[first + j]);
// either output may be null; d_mult32 on a 16-byte boundary
int guards_proofs_enqueue(hipStream_t s, const Fr* d_mult, const int* d_status, uint32_t first, uint32_t count, uint8_t* d_mult32, int* d_status_out);
// the host waits for every stream the batch has (its own or the caller's, the auxiliary and the copy stream) -> the first error
hipError_t wait_for_streams(h2v_batch* b);
// What every enqueueing h2v_batch_* call begins with, and an enqueued feed of a resident accumulator as well (batch.hip): the batch's
// stream exists; it waits for what the last launch left on the auxiliary stream and for a pending read event (h2v_batch::ev_read);
// the whole accumulators are in `acc` if the last launch left pieces only
int need_stream(h2v_batch* b);
int join_tail(h2v_batch* b);
int ensure_whole(h2v_batch* b);
// The terms of a group's two MSM problems (left channel, right channel with the VK-wide bases) for `count` proofs; strided: the left
// problem is one slot of every proof.  channel_problems builds its problems from these counts.
struct ChannelTerms { bool strided; uint32_t left, right; };
ChannelTerms channel_terms(const Plan& pl, uint32_t count, uint32_t n_shared);
// whether a launch of groups of these sizes passes msm_enqueue_multi's rule (msm_cuts_within_limit over the groups' channel_terms): what an
// upload of unequal groups is held to, and what h2v_verify_batches cuts its launches by
bool groups_cut_within_limit(const Plan& pl, const size_t* sizes, size_t n_groups);
// what the accumulation and its pairing read from the params (shplonk.rs's -g term, msm.rs:185-203); k may differ
bool same_srs(const ParamsHost& a, const ParamsHost& b);
// h2v_batches_recheck (h2v_batch_recheck: one batch, batch_of_range NULL); `who` names the entry point in the error messages
int recheck_impl(const char* who, h2v_batch* const* batches, size_t n_batches, size_t n_ranges, const uint32_t* batch_of_range, const size_t* first,
                 const size_t* count, int* range_ok, uint8_t* out_left, uint8_t* out_right);
int export_whole_records(h2v_batch* b, void* device_dst);
// The search of the identifying entry points (oneshot.hip): st[k][i] = H2V_ERR_CONSTRAINT_SYSTEM_FAILURE for every proof i of bs[k] that
// lies in a start range and whose own check fails.  start: ranges of finished batches, each inside one group of its launch;
// known: every start range has failed a check of its own (else the first round checks them as they are).  The number of ranges
// handed to re-check launches is ADDED to *n_checks.
struct IdentifyStart { uint32_t b; size_t first, count; };
int identify_search(const std::vector<h2v_batch*>& bs, const std::vector<IdentifyStart>& start, bool known, std::vector<std::vector<int>>& st, size_t* n_checks);

// ---- grouped one-shot calls (oneshot.hip): h2v_verify_batch_keys and its forms, and a resident accumulator's process (accumulator.hip)
#define H2V_MAX_SHAPES_PER_CALL 64   // distinct (key, instance shape) groups one call takes (H2V_ERR_UNSUPPORTED beyond)
// the proofs of one key with one instance shape, in call order
struct CallGroup { size_t key; std::vector<size_t> shape, idx; };
// what a grouped call holds until it returns: the contexts' locks and scratch batches, and the batches made for the call
struct GroupsHeld;
struct GroupsHeldDelete { void operator()(GroupsHeld* h) const; };
typedef std::unique_ptr<GroupsHeld, GroupsHeldDelete> GroupsHeldPtr;
int grouped_call_args(const char* who, h2v_ctx* const* ctxs, size_t n_keys, const uint32_t* key_of_proof, size_t n, const uint8_t* const* proofs,
                      const size_t* proof_lens, const uint8_t* const* instances32, const size_t* n_instance_columns, const size_t* col_lens,
                      std::vector<CallGroup>& groups);
// the point hints of a _hinted call (include/h2v_hints.h): rows[i] is proof i's row or null, in call order (null: a call without hints);
// stats: three counters to which every launch of the call adds its h2v_batch_hint_stats (null: not asked for)
struct CallHints { const uint8_t* const* rows = nullptr; size_t* stats = nullptr; };
int run_group_batches(h2v_ctx* const* ctxs, size_t n_keys, const std::vector<CallGroup>& groups, size_t n, const uint8_t* const* proofs, const size_t* proof_lens,
                      const uint8_t* const* instances32, const uint8_t* rand32, uint8_t* d_records, bool resident, GroupsHeldPtr& held,
                      std::vector<std::vector<int>>& st, bool& all_ok, const CallHints& hints = CallHints());
}  // namespace h2v

struct h2v_batch {
    h2v_ctx* ctx = nullptr;
    hipStream_t stream = nullptr;     // the caller's (h2v_batch_set_stream), or the batch's own from its first use on (need_stream)
    bool owns_stream = true;
    hipStream_t aux = nullptr;        // only for a launch whose tail the pairing launch cannot carry (close_enqueue, need_aux): the affine conversion beside the pairing
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // h2v_batch_upload_launch: the host -> device copies run on `copy`, chunk by chunk, each followed (after the blocking copy has
    // returned) by the decompression of that chunk on `stream`
    hipStream_t copy = nullptr;
    h2v::BatchStage stage = h2v::BatchStage::Empty;
    bool decompressed = false;        // Uploaded: the upload has decompressed the points already (h2v_batch_upload_launch)
    // point hints (include/h2v_hints.h).  hinted: h2v_batch_set_hints has put the claimed y of the upload's points into `ycanon`, where
    // k_decompress_hinted reads them and writes the canonical y back; set there, cleared by upload_take and by every way to Empty, never
    // inferred from the buffer.  launch_hinted: the last launch ran with hints, and hint_misses[0] counts the ones it did not use.
    // hint_misses[1] counts the entries of a piece's segment of miss_list (StageArgs::miss_list: one word per point `ycanon` holds),
    // which every hinted launch is given.  null_rows: the proofs whose hint row h2v_batch_set_hint_rows staged as zeros because the
    // caller gave none (0 after h2v_batch_set_hints / _device); launch_null_rows: the same of the last launch.  h2v_batch_hint_stats
    // counts neither as hinted nor as missed the Np points of each of them.
    bool hinted = false, launch_hinted = false;
    uint32_t null_rows = 0, launch_null_rows = 0;
    h2v::DevBuf<uint32_t> hint_misses, miss_list;
    h2v::LaunchRecord last;
    // A resident accumulator's enqueued feed (h2v_accumulator_feed_batch, include/h2v_feed.h) reads acc, tail, mult, the status words,
    // the group offsets and ingest_verdict on the ACCUMULATOR's stream, and records ev_read there behind the last of those reads.
    // read_pending: the batch's stream has not waited for it yet (join_tail does, before anything new is enqueued); read_unseen: nor has
    // the host (wait_for_streams does, and an upload that would free one of those arrays).  A batch that was never fed has no event.
    hipEvent_t ev_read = nullptr;
    bool read_pending = false, read_unseen = false;
    size_t max_proofs = 0, max_inst = 0;
    h2v::PlanDevice* plan = nullptr;  // set at upload (depends on the instance shape)
    uint32_t n = 0, n_tail = 0;
    uint32_t groups = 1;              // independent accumulator batches inside this launch (h2v_batch_set_groups)
    // groups of unequal size (h2v_batch_set_group_sizes): group g owns the proofs [group_off[g], group_off[g + 1]) of an upload of
    // group_off[groups] proofs.  Empty: equal groups of n / groups proofs (h2v_batch_set_groups)
    std::vector<uint32_t> group_off;
    std::vector<uint8_t> group_last;  // per proof: it is the last of its group (the segmented scan's input, copied with the draws)
    h2v::DevBuf<uint32_t> d_group_off; h2v::DevBuf<uint8_t> d_group_last;
    std::vector<uint32_t> zero_below; // per group: proofs [0, zero_below[g]) of the group have a zero multiplier (a zero draw behind them in the uploaded tail)
    // h2v_batch_upload_device with the caller's draws: k_ingest_draws checks them, and its verdict [fault][zero_below x groups] waits in
    // pinned memory of the batch's own for h2v_batch_finish, which fills zero_below from it (device block: + the count of workgroups done)
    bool device_draws = false;
    h2v::DevBuf<uint32_t> ingest_verdict; h2v::MappedHostBuf ingest_host;
    // h2v_batch_finish_device's scratch (results_enqueue): a word per tile of 256 proofs; a word per group, zero between calls
    h2v::DevBuf<uint32_t> finish_tiles, finish_groups;
    // h2v_batch_guards' scratch (guards_out.hip): the byte form of the range's terms on their way to the host, grow-only
    h2v::DevBuf<uint8_t> guards_scratch;
    // device buffers: every one grow-only, sized for max_proofs, the group count and the largest plan uploaded so far (ensure_buffers)
    h2v::DevBuf<uint8_t> proofs, inst, tail;
    h2v::DevBuf<h2v::G1A> pts, phi;   // the batch's points + the VK-wide bases, and their images under the GLV endomorphism (same shape)
    h2v::DevBuf<uint8_t> ycanon;
    h2v::DevBuf<unsigned long long> words; h2v::DevBuf<h2v::Fr> chal, mult, slots;
    h2v::DevBuf<h2v::Fr> mult_scratch;  // multipliers_enqueue's scratch
    bool mult_of_draws = false;       // Uploaded and later: `mult` holds the multipliers of the uploaded draws (not gathered ones, h2v_verify_batch_shapes)
    h2v::DevBuf<uint32_t> msm_scal; h2v::DevBuf<h2v::Fr> shared; h2v::DevBuf<uint32_t> left_scal;
    h2v::DevBuf<h2v::Fr> insteval;    // [query][proof] (wide instance vectors)
    h2v::DevBuf<uint32_t> guard_scal; // [proof][guard term][8] (h2v_guard_msm with GWC)
    h2v::DevBuf<h2v::G1J> acc;        // per group: [2g] left, [2g+1] right
    // the results block (h2v::ResultsLayout) on the device and in pinned host memory; the pointers below point into it for the upload's group count
    h2v::DevBuf<uint8_t> results; h2v::MappedHostBuf results_host;
    uint32_t* ok = nullptr;           // [groups] — in the host block: the pairing kernels write their verdicts straight to the host
    uint8_t* out_bytes = nullptr; uint32_t* out_ident = nullptr;
    uint32_t* fold_failed = nullptr;  // [groups] failed proofs reported by the folded shards (h2v_batch_fold_check_enqueue)
    int* status = nullptr;
    h2v::MsmWorkspace ws;
    h2v::Recheck recheck;             // h2v_batch_recheck's own workspace and outputs
    h2v::MsmSplit split;              // how the last launch left its accumulators to the pairing (parts == 0: whole points in acc)
    h2v::DevBuf<uint8_t> line_ws;     // k_pair_lines' output, H2V_PAIRING_LINE_WS_BYTES per group
    uint32_t stream_words = 0;
    // profiling
    int profiling = 0;                // 0 off, 1: the dominant kernel's own events (msm_accumulate), 2: + an event between the stages
    hipEvent_t ev[8] = {nullptr};
    float last_ms[7] = {0, 0, 0, 0, 0, 0, 0};
};

namespace h2v {
// The groups of the batch's upload — what (groups, n, n_tail, group_off) fixed — for host code, and with the offsets' device copy for
// a kernel; group_shape_of: of an upload of n proofs and n_tail draws that the batch has not taken yet
inline GroupShape group_shape_of(const h2v_batch* b, size_t n, size_t n_tail, const uint32_t* off) {
    return b->group_off.empty() ? GroupShape::equal(b->groups, (uint32_t)n, (uint32_t)n_tail) : GroupShape::unequal(b->groups, b->group_off.back(), off);
}
inline GroupShape group_shape(const h2v_batch* b) { return group_shape_of(b, b->n, b->n_tail, b->group_off.data()); }
inline GroupShape group_shape_device(const h2v_batch* b) { return group_shape_of(b, b->n, b->n_tail, b->d_group_off.p); }
}  // namespace h2v
