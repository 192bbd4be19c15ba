// Internal declarations shared by the translation units of libh2v_amd.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/h2v.h"
#include "../../include/h2v_draws.h"
#include "../../include/h2v_guards.h"
#include "curve.hip.h"

namespace h2v {

void set_last_error(const std::string& s);
#define H2V_HIP_CHECK(expr)                                                                     \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            ::h2v::set_last_error(std::string(#expr) + ": " + hipGetErrorString(e_));           \
            return H2V_ERR_DEVICE;                                                              \
        }                                                                                       \
    } while (0)

// Device allocation owned by its holder (a scope, a batch, a workspace): error paths that `return` from the middle of an entry point
// free what they took, and long-lived objects free theirs when they are deleted.
template <class T> struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;   // elements p holds
    DevBuf() {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~DevBuf() { reset(); }
    int alloc(size_t count) {
        reset();
        H2V_HIP_CHECK(hipMalloc(&p, (count ? count : 1) * sizeof(T)));
        cap = count ? count : 1;
        return 0;
    }
    // grow-only: a new allocation (contents not kept) only when count exceeds what p holds
    int reserve(size_t count) { return p && count <= cap ? 0 : alloc(count); }
    void reset() { if (p) hipFree(p); p = nullptr; cap = 0; }
};

// Pinned host memory mapped into the device's address space (hipHostMallocMapped): `p` for the host, `dev` for kernels that write
// to it directly.  Grow-only like DevBuf::reserve.
struct MappedHostBuf {
    uint8_t* p = nullptr;
    void* dev = nullptr;
    size_t cap = 0;   // bytes
    MappedHostBuf() {}
    MappedHostBuf(const MappedHostBuf&) = delete;
    MappedHostBuf& operator=(const MappedHostBuf&) = delete;
    ~MappedHostBuf() { reset(); }
    int reserve(size_t bytes) {
        if (p && bytes <= cap) return 0;
        reset();
        H2V_HIP_CHECK(hipHostMalloc((void**)&p, bytes ? bytes : 1, hipHostMallocMapped));
        H2V_HIP_CHECK(hipHostGetDevicePointer(&dev, p, 0));
        cap = bytes ? bytes : 1;
        return 0;
    }
    void reset() { if (p) hipHostFree(p); p = nullptr; dev = nullptr; cap = 0; }
};

// Forced kernel variants: the validated h2v_tuning itself (include/h2v.h; every field 0 = automatic) lives in the context, and a launch
// copies it into the objects that choose (MsmWorkspace::tune, FrvmArgs, the pairing launcher's argument).  The library reads no
// environment variable.

// ------------------------------------------------------------------ MSM (msm.hip)
// Pippenger over pooled (scalar, base) terms.  Scalars: canonical little-endian 32-bit words, 8 per
// term; bases: affine Montgomery, (0,0) = identity (skipped).
struct MsmPlan {
    uint32_t n;        // terms
    uint32_t c;        // window bits
    uint32_t windows;  // ceil(130 / c) (msm_plan).  GLV halves are magnitudes below 2^127 (glv_decompose: exact floors) and the signed-digit carry adds a
                       // bit: ceil(128 / c) windows hold every digit — the top digit sits in window floor(126 / c) or, by the carry, floor(127 / c)
                       // (tests/test_gpu_msm_units.py) — and the plan keeps two bits more (one more window at c = 2, 3, 4 and 8, none at the other widths up to 15)
    uint32_t buckets;  // 2^(c-1) per window (signed digits)
};
MsmPlan msm_plan(uint32_t n, bool latency = false);

// One MSM of a multi-problem launch: term i < n1 reads scalars[i * sstride ..+8) and bases[i * bstride]; terms n1 <= i < n
// read a second segment (scalars2, bases2) at index i - n1 (a batch's VK-wide bases live apart from its own points).
struct MsmProblem {
    const uint32_t* scalars; const G1A* bases; G1J* out;
    uint32_t sstride, bstride, n;
    uint32_t n1;
    const uint32_t* scalars2; const G1A* bases2;
    const G1A* phi = nullptr; const G1A* phi2 = nullptr;   // optional: phi(P) = (beta x, y) of every base, arrays parallel to bases / bases2 (same stride).  Without them
                                                           // the launch makes its own table (msm_glv_prep); the verifier's points carry theirs from decompression
    uint32_t glv_off = 0;   // first record of this problem in the launch's GLV table (set by msm_enqueue_multi)
    uint32_t sub_first = 0, sub_count = 0;   // set by msm_enqueue_multi when it cuts a large problem into sub-problems (their window sums are merged)
    uint32_t nnz = 0;       // if non-zero: a promise that at most this many of the n scalars are non-zero (sizes msm_accumulate's grid; a broken
                            // promise costs time, not correctness)
    MsmProblem() : scalars(nullptr), bases(nullptr), out(nullptr), sstride(8), bstride(1), n(0), n1(0), scalars2(nullptr), bases2(nullptr) {}
    MsmProblem(const uint32_t* s, const G1A* b, G1J* o, uint32_t ss, uint32_t bs, uint32_t n_) : scalars(s), bases(b), out(o), sstride(ss), bstride(bs), n(n_), n1(n_), scalars2(nullptr), bases2(nullptr) {}
    MsmProblem(const uint32_t* s, const G1A* b, G1J* o, uint32_t ss, uint32_t bs, uint32_t n1_, const uint32_t* s2, const G1A* b2, uint32_t n2)
        : scalars(s), bases(b), out(o), sstride(ss), bstride(bs), n(n1_ + n2), n1(n1_), scalars2(s2), bases2(b2) {}
};
#define MSM_MAX_PROBLEMS 1024     // per launch (a grouped batch: two channels per group; SingleStrategy: one group per proof)
#define MSM_PROBLEM_CHUNK 44      // descriptors handed to the device per setter launch (kernel-argument space)
struct MsmProblemChunk { MsmProblem p[MSM_PROBLEM_CHUNK]; };
static_assert(sizeof(MsmProblemChunk) <= 4000, "a chunk of problem descriptors travels as one kernel argument (4 KB limit)");
struct MsmProblems { std::vector<MsmProblem> p; };

// A Jacobian point in its own 128-byte line: the MSM's intermediate arrays are written once per lane at scattered
// indices, and a 108-byte object that straddles lines costs partial-line writes on both (measured 2.5x the bytes)
struct alignas(128) G1JSlot {
    G1J p;
    uint32_t pad[5];   // written with the point: a store that leaves part of a 32-byte sector untouched is a read-modify-write in memory
    __host__ __device__ G1JSlot& operator=(const G1J& v) { p = v; for (int i = 0; i < 5; ++i) pad[i] = 0; return *this; }
    __host__ __device__ operator const G1J&() const { return p; }
};

#define MSM_MAX_PARTS 6
struct MsmSplit {
    uint32_t want_parts = 0;                        // in
    uint32_t parts = 0, shift = 0, count = 0;       // out
    const G1JSlot* pts = nullptr;                   // out: the workspace's piece array
    const G1JSlot* ready = nullptr;                 // out: the same pieces as (X Z, Y, Z^3), the form the Miller lines are evaluated at
};

// The record a rank contributes to a sharded batch (include/h2v.h H2V_ACC_RECORD_BYTES): the two accumulators of one group —
// in the pieces the launch left them in (MsmSplit), or whole (parts = 1) — plus the number of the shard's proofs that failed
// before the MSM.  A failed proof is zeroed out of its shard's accumulators, so without the count every OTHER rank's folded
// pairing would still pass.
struct AccRecord { uint32_t failed, parts, shift, reserved; G1J left[H2V_ACC_RECORD_PIECES], right[H2V_ACC_RECORD_PIECES]; };
static_assert(sizeof(AccRecord) == H2V_ACC_RECORD_BYTES && H2V_ACC_RECORD_BYTES == 16 + 2 * H2V_ACC_RECORD_PIECES * 108, "accumulator record layout");
static_assert(H2V_ACC_RECORD_PIECES >= MSM_MAX_PARTS, "a record holds every piece a launch can leave");

struct MsmWorkspace {
    // what the workspace was sized for (reserve): terms of a launch, the caller's problems, terms of the largest problem
    uint32_t cap_terms = 0, cap_parents = 0, cap_per_problem = 0;
    uint32_t cap_problems = 0;                 // problems of a launch once large ones are cut into sub-problems
    size_t cap_buckets = 0, cap_list = 0;
    DevBuf<uint32_t> counts;       // [problems * windows * buckets + 3]  (last three words: number of heavy buckets, list cursor, number of straddling buckets)
    DevBuf<uint32_t> offsets;      // [problems * windows * buckets]
    DevBuf<uint32_t> cursor;       // scatter cursors, then the heavy-bucket list
    DevBuf<uint32_t> list;         // term indices sorted by (problem, window, bucket)
    DevBuf<G1JSlot> bucket_pts;    // [problems * windows * buckets]
    DevBuf<G1JSlot> window_sums;   // [problems * windows]
    DevBuf<G1JSlot> pieces;        // [2][problems * MSM_MAX_PARTS] partial Horner sums (MsmSplit): Jacobian, then line-ready
    std::vector<MsmProblem> resident; // the caller's problems whose descriptors `problems` (and `parents`) hold since the last msm_enqueue_multi (empty: none)
    int resident_no_split = 0;        // ... cut under this h2v_tuning.msm_no_term_split
    DevBuf<MsmProblem> problems;   // [cap_problems] descriptors of the launch in flight (sub-problems when large problems are cut)
    DevBuf<MsmProblem> parents;    // [cap_parents] the caller's problems when they were cut
    DevBuf<G1JSlot> merged_sums;   // [cap_parents * 128] window sums of the caller's problems, merged over their sub-problems
    const MsmProblem* final_problems = nullptr;   // whichever of the two the last launch's Horner wrote through
    DevBuf<uint32_t> block_sums;   // [cap_buckets / 1024 + 2] prefix-sum scratch
    DevBuf<G1JSlot> partial;       // [2 * cap_list / chunk] head and tail pieces of the accumulation chunks
    DevBuf<uint32_t> redo;         // [cap_list / chunk] chunks msm_accumulate left to msm_accumulate_redo (complete formulas)
    DevBuf<uint32_t> glv;          // [cap_list / 2] signed window digits of the launch's terms, window-major per problem (LDS sort path)
    DevBuf<G1A> phi_pts;           // [cap_terms] phi(P) = (beta x, y) of every base of the launch (LDS sort path): made once per term instead of once per list entry
    DevBuf<uint32_t> seg_total;    // [problems * windows] entries per list segment
    DevBuf<uint32_t> seg_start;    // [problems * windows + 1] logical start of every segment
    // optional HIP events around msm_accumulate (the dominant kernel: bench.py's roofline.kernels), recorded when `profile` is set
    h2v_tuning tune = {};            // forced variants for the next launch (copied from the context by the caller)
    bool profile = false, profile_recorded = false;
    hipEvent_t ev_acc[2] = {nullptr, nullptr};
    // Grow-only: every dimension becomes the larger of what the workspace holds and what is asked for, and the buffers are allocated
    // again only if one of them grew (a workspace sized for more serves less).  max_terms_per_problem sizes the bucket arrays (the window
    // plan follows the largest problem of a launch); 0 = max_total_terms.
    int reserve(uint32_t max_total_terms, uint32_t max_problems, uint32_t max_terms_per_problem = 0);
    bool covers(uint32_t max_total_terms, uint32_t max_problems, uint32_t max_terms_per_problem = 0) const;
    MsmWorkspace() {}
    MsmWorkspace(const MsmWorkspace&) = delete;
    MsmWorkspace& operator=(const MsmWorkspace&) = delete;
    ~MsmWorkspace() { for (hipEvent_t e : ev_acc) if (e) hipEventDestroy(e); }
};
// Enqueue all problems of `pr` (each: sum_i scalars[i] * bases[i] -> *out, Jacobian, device memory).  Asynchronous on `s`.
// With `split` (want_parts > 1) the Horner over the windows stops early: problem q is left as `parts` points
//   pts[q * parts + j],   sum_i scalars[i] * bases[i] = sum_j 2^(shift * j) * pts[q * parts + j]
// and *out is NOT written until msm_combine_enqueue (any stream ordered after `s`).  split->parts == 0 on return: the launch was
// not cut (no terms, or a single window) and *out is written as without `split`.
int msm_enqueue_multi(hipStream_t s, MsmWorkspace& ws, const MsmProblems& pr, MsmSplit* split = nullptr);
int msm_combine_enqueue(hipStream_t s, MsmWorkspace& ws, const MsmSplit& sp, size_t lds_reserve = 0);
// msm_enqueue_multi's rule for a launch of problems of these term counts, for callers that must know before any device work: true if
// every problem fits the per-window LDS sort as it is, or all of them cut into sub-problems that do are at most MSM_MAX_PROBLEMS
bool msm_cuts_within_limit(const uint32_t* terms, size_t n_problems);
// `lds_reserve` (msm_combine_enqueue, point_to_bytes_enqueue): bytes of LDS the launch asks for without using them.  The two kernels run
// on a batch's auxiliary stream BESIDE the pairing, as a handful of waves with a 0.3 ms chain of their own; where one of those waves
// landed on a SIMD of a pairing workgroup (which issues at raised priority) it crawled — msm_combine_parts took 0.29 ms alone and up to
// 0.53 ms beside k_pairing2, and the launch then waited for IT.  A workgroup that asks for more LDS than a CU has left beside a
// k_pairing2 workgroup (160 KB - 58 KB) is never placed on such a CU, and its CU takes no pairing workgroup afterwards.
#define H2V_AUX_LDS_RESERVE ((size_t)110 * 1024)
int msm_enqueue(hipStream_t s, MsmWorkspace& ws, const uint32_t* d_scalars, const G1A* d_bases, uint32_t n, G1J* d_out);
// d_record (an accumulator record, whole points: parts = 1, failed = 0) <- M * (d_points[0], d_points[1]); d_scalar_words: M as 8 canonical
// little-endian words.  One wave (k_accumulator_scale): the scale step of a resident accumulator (accumulator.hip)
int accumulator_scale_enqueue(hipStream_t s, const G1J* d_points, const uint32_t* d_scalar_words, void* d_record);
// The same for n (pair, scalar) items in one launch, one one-wave workgroup each: d_records[i] <- scalar i * (d_pairs[2 slot],
// d_pairs[2 slot + 1]) with slot = d_slots[i], scalar i = d_scalar_words[8 i ..].  The rebuild of a journaled accumulator.
int accumulator_scale_many_enqueue(hipStream_t s, const G1J* d_pairs, const uint32_t* d_slots, const uint32_t* d_scalar_words, uint32_t n, void* d_records);

// ------------------------------------------------------------------ small helpers (util.hip)
// canonical x|y bytes (64 B each, all-zero = identity) -> affine Montgomery; flags[i] = 0 ok, 1 not canonical / not on curve
int bases_from_bytes_enqueue(hipStream_t s, const uint8_t* d_bytes, G1A* d_out, uint32_t* d_flags, uint32_t n);
// canonical 32-B scalars -> 8 x 32-bit words (validated < r); flags[i] = 1 when >= r
int scalars_from_bytes_enqueue(hipStream_t s, const uint8_t* d_bytes, uint32_t* d_out, uint32_t* d_flags, uint32_t n);
// Both conversions for the n terms of a call's Guards in one launch (k_guard_terms), one validity word instead of a flag per term:
// *d_first_bad = the lowest index of a term whose scalar is >= r or whose base is neither all-zero nor a canonical point on the curve
// (0xffffffff: none; the launcher presets it; such a term is written as a zero scalar and the identity).  With d_mult, scalar i is
// multiplied by d_mult[d_guard_of_term[i]] (multipliers as multipliers_enqueue leaves them); d_mult null: unscaled, d_guard_of_term
// is not read.  The byte arrays and d_out_scalars lie on 16-byte boundaries.
int guard_terms_enqueue(hipStream_t s, const uint8_t* d_scalars32, const uint8_t* d_bases64, const uint32_t* d_guard_of_term, const Fr* d_mult, uint32_t* d_out_scalars,
                        G1A* d_out_bases, uint32_t* d_first_bad, uint32_t n);
// A resident MSM object's scalars in place (k_msm_scale): words i <- words i * f mod r for n terms of 8 canonical words, `factor` = f in
// Montgomery form.  d_words lies on a 16-byte boundary.
int msm_scale_enqueue(hipStream_t s, uint32_t* d_words, const Fr& factor, uint32_t n);
// affine Montgomery -> canonical x|y bytes (64 B each, the identity all-zero): the inverse of bases_from_bytes_enqueue (k_affine_to_bytes).
// d_out lies on a 16-byte boundary.
int affine_to_bytes_enqueue(hipStream_t s, const G1A* d_in, uint8_t* d_out, uint32_t n);
// Jacobian -> canonical x|y bytes (+ identity flag word after the 64 bytes: out is 68 B aligned to 4)
int copy_words_enqueue(hipStream_t s, const void* d_src, void* d_dst, size_t n_words, size_t lds_reserve = 0);   // by a kernel (the destination may be mapped host memory)
int point_to_bytes_enqueue(hipStream_t s, const G1J* d_in, uint8_t* d_out_xy64, uint32_t* d_is_identity, uint32_t n, size_t lds_reserve = 0);
// An upload from device memory (h2v_batch_upload_device), two launches.  The verdict block d_verdict holds groups + 2 words:
// [fault][zero_below x groups][workgroups done].
// rows: n rows of row_len bytes, `stride` bytes apart -> packed at d_out_rows, and inst_bytes bytes d_inst -> d_out_inst, in one launch
// (k_ingest_rows); every pointer, the stride and both lengths are multiples of 16.  With d_verdict the launch presets the verdict block
// (fault 0xffffffff, the rest 0), also when there is nothing to copy.
int ingest_rows_enqueue(hipStream_t s, const void* d_rows, size_t stride, size_t row_len, size_t n, const void* d_inst, size_t inst_bytes, uint8_t* d_out_rows,
                        uint8_t* d_out_inst, uint32_t* d_verdict, uint32_t groups);
// k_ingest_rows the other way round (k_hint_rows_out; h2v_batch_hints_device): n packed rows of row_len bytes at d_rows into the caller's
// rows at d_out + i * stride; every pointer, the stride and the length are multiples of 16
int hint_rows_out_enqueue(hipStream_t s, const uint8_t* d_rows, size_t row_len, size_t n, void* d_out, size_t stride);
// draws: n_tail 32-byte scalars d_draws -> d_tail, the scalar 1 in place of a draw >= r (k_ingest_draws); the verdict block preset by
// ingest_rows_enqueue on the same stream takes the lowest index of such a draw and every group's zero_below (GroupShape::zero_below; the
// n proofs and n_tail draws fit `shape`, batch.h, its offsets in device memory), and its first 1 + shape.G words go to d_host_verdict
// (mapped host memory) when the last workgroup is done.
struct GroupShape;
int ingest_draws_enqueue(hipStream_t s, const void* d_draws, uint8_t* d_tail, uint32_t n_tail, uint32_t n, const GroupShape& shape, uint32_t* d_verdict, uint32_t* d_host_verdict);
// A finish into device memory (h2v_batch_finish_device): two launches, three with the failing proofs' indices (k_results_tiles,
// k_results_close, k_results_scatter).  Every output of ResultsOut may be null = not wanted.
struct ResultsOut {
    int* status = nullptr;              // [n] the ABI's codes (status_decode of the device words)
    int* group_ok = nullptr;            // [groups] 0 / 1
    uint8_t* left_xy = nullptr;         // [groups][64]
    uint8_t* right_xy = nullptr;        // [groups][64]
    uint32_t* group_failed = nullptr;   // [groups] proofs of the group with a non-zero status
    uint32_t* failed_index = nullptr;   // the first failed_cap proofs with a non-zero status, ascending
    uint32_t failed_cap = 0;
    uint32_t* summary = nullptr;        // [H2V_SUMMARY_WORDS]
};
// the words of d_tile_words: a word per tile of 256 proofs
inline size_t results_tiles(size_t n) { return (n + 255) / 256; }
// d_status: the n rank-coded status words of the proofs of `shape` (batch.h; its offsets in device memory); d_fold_failed, d_ok (read
// only with flag bit 0; may be mapped host memory), d_out_bytes: [shape.G] words, words and 128 bytes of the results block; d_fault: the
// word the summary reports as the draw fault (null: none; a value other than 0xffffffff rejects every group); flags: summary word 5.
// Scratch: d_tile_words (results_tiles(n) words, any contents) and d_group_words (shape.G words: ZERO on entry, and zero again when the
// launches have run).
int results_enqueue(hipStream_t s, const int* d_status, uint32_t n, const GroupShape& shape, const uint32_t* d_fold_failed, const uint32_t* d_ok, uint32_t flags,
                    const uint8_t* d_out_bytes, const uint32_t* d_fault, uint32_t* d_tile_words, uint32_t* d_group_words, const ResultsOut& out);
// Sharded batches exchange H2V_ACC_RECORD_BYTES records per group: [failed, parts, shift, 0][left pieces][right pieces] (h2v.h).
// export: d_out[g] <- the group's accumulators — pieces [(2g + side) * parts + j] if d_pieces, else the whole points d_acc[2g], [2g+1] —
// and the number of non-zero statuses among the group's n / groups proofs
int export_records_enqueue(hipStream_t s, const G1J* d_acc, const G1JSlot* d_pieces, uint32_t parts, uint32_t shift, const int* d_status, uint32_t n, uint32_t groups, void* d_out);
// fold: the sums over the records [i][g] of each group's accumulators, cut into `parts` pieces of weight 2^(shift j) (-> d_pieces and,
// as (X Z, Y, Z^3), d_ready) or whole (parts <= 1 -> d_acc[2g + side]); d_fold_failed[g] = sum of the records' failure counts
int fold_records_enqueue(hipStream_t s, const void* d_recs, uint32_t n_recs, uint32_t groups, uint32_t parts, uint32_t shift, G1J* d_acc, G1JSlot* d_pieces, G1JSlot* d_ready,
                         uint32_t* d_fold_failed);
// The fold of a merge (k_accumulator_merge_fold), one launch: d_acc[side] <- d_acc[side] + the sum of the n whole-point records' side,
// and with d_sums record k's two points -> d_sums[2 slot], [2 slot + 1], slot = d_slots[k] (d_slots null: k).  team: the lanes that
// share a side's sum, a power of two in 1 .. 64; 0 = accumulator_merge_team(n) = min(64, the next power of two >= n + 1).
uint32_t accumulator_merge_team(uint32_t n);
int accumulator_merge_fold_enqueue(hipStream_t s, const void* d_recs, uint32_t n, uint32_t team, const uint32_t* d_slots, G1J* d_sums, G1J* d_acc);
// The fold of a batch's legs (k_accumulator_legs_fold), one launch: d_acc[side] <- the sum of the n >= 1 whole-point records' side (the
// accumulator is replaced: record 0 is its scaled self), and with d_sums the unscaled pair of leg g < n - 1, d_pairs[2 g], [2 g + 1]
// -> d_sums[2 slot], [2 slot + 1], slot = d_slots[g] (d_slots null: g).  team: as above; 0 = accumulator_merge_team(n - 1).
int accumulator_legs_fold_enqueue(hipStream_t s, const void* d_recs, uint32_t n, uint32_t team, const G1J* d_pairs, const uint32_t* d_slots, G1J* d_sums, G1J* d_acc);

// ------------------------------------------------------------------ draws from a seed (verify_kernels.hip, draws.hip; include/h2v_draws.h)
// d_out[32 j ..] <- draw(seed32, first + j) for j < n, canonical bytes (k_expand_draws: one launch, 16 draws per wave; the seed
// travels as kernel arguments).  d_out lies on a 16-byte boundary; first + n does not wrap; n <= H2V_DRAWS_DEVICE_MAX (the launch stays
// below 2^32 threads).  n = 0 launches nothing.
int expand_draws_enqueue(hipStream_t s, const uint8_t seed32[32], uint64_t first, size_t n, void* d_out);
// the same values on the host (a BLAKE2b-512 single-block compression of its own, RFC 7693)
void expand_draws_host(const uint8_t seed32[32], uint64_t first, size_t n, uint8_t* out32);

}  // namespace h2v
