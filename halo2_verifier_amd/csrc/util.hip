// Format-conversion and small group kernels at the C-ABI boundary.
#include "../../include/h2v.h"
#include "ctx.h"
#include "batch.h"   // the status words' rank codes (k_results_tiles)

namespace h2v {

__global__ void __launch_bounds__(256) k_bases_from_bytes(const uint8_t* __restrict__ in, G1A* __restrict__ out, uint32_t* __restrict__ flags, uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* b = in + 64 * (size_t)i;
    uint8_t tmp[64]; uint32_t any = 0;
    for (int j = 0; j < 64; ++j) { tmp[j] = b[j]; any |= tmp[j]; }
    G1A p; uint32_t bad = 0;
    if (!any) p = G1A::identity();
    else {
        if (!Fq::from_bytes(tmp, p.x) || !Fq::from_bytes(tmp + 32, p.y)) { bad = 1; p = G1A::identity(); }
        else if (!p.on_curve()) { bad = 1; p = G1A::identity(); }
    }
    out[i] = p; flags[i] = bad;
}

__global__ void __launch_bounds__(256) k_scalars_from_bytes(const uint8_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t* __restrict__ flags, uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* b = in + 32 * (size_t)i;
    uint32_t raw[8];
    for (int j = 0; j < 8; ++j) raw[j] = (uint32_t)b[4 * j] | ((uint32_t)b[4 * j + 1] << 8) | ((uint32_t)b[4 * j + 2] << 16) | ((uint32_t)b[4 * j + 3] << 24);
    uint32_t bad = Fr::geq_p(raw) ? 1u : 0u;
    for (int j = 0; j < 8; ++j) out[8 * (size_t)i + j] = bad ? 0u : raw[j];
    flags[i] = bad;
}

// The terms of a call's Guards (h2v_accumulator_process_guards, h2v_guards_check_each: the term lists a CPU verify_proof hands over), one
// thread per term, both conversions above in one launch and the draw's multiplier on the way:
//   scalar: 32 canonical bytes, refused when >= r; with `mult`, s * mult[guard_of_term[i]] — ONE Montgomery product: the bytes' integer
//           times the multiplier as multipliers_enqueue leaves it (m R) is s m — as the 8 canonical words the MSM reads (sstride 8);
//   base:   64 bytes x | y, all-zero = the identity, else canonical and on the curve, as a G1A.
// A bad term writes a zero scalar and the identity, and its index joins *first_bad by atomicMin (the launcher presets the word to
// 0xffffffff): one word per launch, the lowest offending term.  The byte arrays are read as 16-byte words (every term lies at a
// multiple of 32 / 64 bytes of a hipMalloc allocation; the launcher checks the pointers): 2 + 4 loads per lane, not 96 byte loads.
// gfx950 (-Rpass-analysis=kernel-resource-usage): 74 VGPRs, 52 SGPRs, no spills, 80 bytes of scratch per lane (the call frames of the
// field product and the square, real function calls throughout the library: bn254.hip.h), no LDS; 6 waves per SIMD.
__global__ void __launch_bounds__(256) k_guard_terms(const uint4* __restrict__ scalars, const uint4* __restrict__ bases, const uint32_t* __restrict__ guard_of_term,
                                                     const Fr* __restrict__ mult, uint4* __restrict__ out_scalars, G1A* __restrict__ out_bases,
                                                     uint32_t* __restrict__ first_bad, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 s0 = scalars[2 * (size_t)i], s1 = scalars[2 * (size_t)i + 1];
    uint32_t raw[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    bool bad = Fr::geq_p(raw);
    uint32_t w[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) { const uint4 v = bases[4 * (size_t)i + j]; w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w; }
    uint32_t any = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) any |= w[j];
    G1A p = G1A::identity();
    if (any) {
        if (Fq::geq_p(w) || Fq::geq_p(w + 8)) bad = true;
        else {
            p.x = Fq::from_raw(w); p.y = Fq::from_raw(w + 8);
            if (!p.on_curve()) bad = true;
        }
    }
    if (!bad && mult) {
        Fr t;
        Fr::pack29(t.v, raw);
        const Fr prod = Fr::mul(t, mult[guard_of_term[i]]);
        uint32_t c[9];
        prod.canonical(c);
        Fr::unpack29(raw, c);
    }
    if (bad) {
        p = G1A::identity();
#pragma unroll
        for (int j = 0; j < 8; ++j) raw[j] = 0;
        atomicMin(first_bad, i);
    }
    out_scalars[2 * (size_t)i] = make_uint4(raw[0], raw[1], raw[2], raw[3]);
    out_scalars[2 * (size_t)i + 1] = make_uint4(raw[4], raw[5], raw[6], raw[7]);
    out_bases[i] = p;
}

// scalar_i <- scalar_i * f mod r over the n terms of a resident MSM object (h2v_msm_scale, msm_object.hip: MSMKZG::scale, msm.rs:67-75), one
// thread per term, in place.  The words are 8 canonical little-endian u32 per term (what the MSM reads, sstride 8); `factor` is f in
// Montgomery form (f R, made once per call on the host), and the words' integer times f R under the Montgomery product is s f — the
// identity k_guard_terms relies on for its multipliers.  Two 16-byte loads, ONE field product, canonical, two 16-byte stores; a thread
// past n touches nothing.
// gfx950 (-Rpass-analysis=kernel-resource-usage): 30 VGPRs, 39 SGPRs, no spills, 48 bytes of scratch per lane (the call frame of the
// field product), no LDS; 8 waves per SIMD.
__global__ void __launch_bounds__(256) k_msm_scale(uint4* __restrict__ scalars, const Fr factor, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 s0 = scalars[2 * (size_t)i], s1 = scalars[2 * (size_t)i + 1];
    uint32_t raw[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    Fr t;
    Fr::pack29(t.v, raw);
    const Fr prod = Fr::mul(t, factor);
    uint32_t c[9];
    prod.canonical(c);
    Fr::unpack29(raw, c);
    scalars[2 * (size_t)i] = make_uint4(raw[0], raw[1], raw[2], raw[3]);
    scalars[2 * (size_t)i + 1] = make_uint4(raw[4], raw[5], raw[6], raw[7]);
}

// Affine Montgomery points -> canonical little-endian x | y, 64 bytes each, the identity as 64 zero bytes: the inverse of
// k_bases_from_bytes, for the read-back of a resident MSM object's bases (h2v_msm_terms: MSMKZG::bases, msm.rs:88-90).  One thread per
// point: x and y leave Montgomery form by one product with 1 each (to_raw), four 16-byte stores.  `out` lies on a 16-byte boundary
// (the launcher checks); the points are read as they lie (a G1A is 72 bytes: word loads).
// gfx950 (-Rpass-analysis=kernel-resource-usage): 56 VGPRs, 39 SGPRs, no spills, 48 bytes of scratch per lane (the call frame of the
// field product), no LDS; 8 waves per SIMD.
__global__ void __launch_bounds__(256) k_affine_to_bytes(const G1A* __restrict__ in, uint4* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const G1A a = in[i];
    uint32_t w[16];
    a.to_xy_raw(w);
#pragma unroll
    for (int j = 0; j < 4; ++j) out[4 * (size_t)i + j] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
}

__global__ void k_point_to_bytes(const G1J* __restrict__ in, uint8_t* __restrict__ out, uint32_t* __restrict__ is_identity, uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    G1A a = g1_to_affine(in[i]);
    uint8_t tmp[64];
    if (a.is_identity()) { for (int j = 0; j < 64; ++j) tmp[j] = 0; is_identity[i] = 1; }
    else { a.x.to_bytes(tmp); a.y.to_bytes(tmp + 32); is_identity[i] = 0; }
    for (int j = 0; j < 64; ++j) out[64 * (size_t)i + j] = tmp[j];
}

// (AccRecord, the record a rank contributes to a sharded batch: internal.h)
// acc: whole points [2g], [2g+1] (parts == 1) — or pieces: [(2g + side) * parts + j]
__global__ void __launch_bounds__(256) k_export_records(const G1J* __restrict__ acc, const G1JSlot* __restrict__ pieces, uint32_t parts, uint32_t shift,
                                                        const int* __restrict__ status, uint32_t gs, AccRecord* __restrict__ out) {
    __shared__ uint32_t failed;
    const uint32_t g = blockIdx.x, t = threadIdx.x;
    if (t == 0) failed = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t p = t; p < gs; p += 256) mine += status[(size_t)g * gs + p] != 0 ? 1u : 0u;
    if (mine) atomicAdd(&failed, mine);
    __syncthreads();
    if (t < 2 * H2V_ACC_RECORD_PIECES) {
        const uint32_t side = t / H2V_ACC_RECORD_PIECES, j = t % H2V_ACC_RECORD_PIECES;
        G1J v = G1J::identity();
        if (j < parts) v = pieces ? pieces[(size_t)(2 * g + side) * parts + j].p : acc[2 * g + side];
        (side ? out[g].right : out[g].left)[j] = v;
    }
    if (t == 0) { out[g].failed = failed; out[g].parts = parts; out[g].shift = shift; out[g].reserved = 0; }
}
// a record's accumulator put together: sum_j 2^(shift j) piece_j, 1 <= parts <= H2V_ACC_RECORD_PIECES (only for records that do not match the
// fold's own split: rare).  shift (parts - 1) dependent doublings: the caller bounds them (ACC_RECORD_MAX_SPAN)
__device__ __noinline__ G1J acc_record_whole(const G1J* pc, uint32_t parts, uint32_t shift) {
    G1J a = pc[parts - 1];
    for (uint32_t j = parts - 1; j-- > 0;) {
        for (uint32_t i = 0; i < shift; ++i) a = g1_add(a, a);
        a = g1_add(a, pc[j]);
    }
    return a;
}
// The doublings a record may ask for, shift (parts - 1).  What a launch exports: msm_plan picks c in 2 .. 15 with ceil(130 / c) windows, and
// msm_enqueue_multi cuts them into parts of wpp windows, shift = c wpp with (parts - 1) wpp < windows: shift (parts - 1) <= c (windows - 1) <= 129, and
// over every (c, parts wanted) at most 128 (c = 2, 4 and 8; tests/record_reference.py max_exported_span).  The record's words come from the caller's memory, and the loop above must not run for as long as a garbage word says.
#define ACC_RECORD_MAX_SPAN 256u
__device__ __forceinline__ uint32_t sat_add_u32(uint32_t a, uint32_t b) { const uint32_t s = a + b; return s < a ? 0xffffffffu : s; }
// Fold: piece j of (group g, side) = sum over the ranks' records of their piece j — records that were cut the same way
// (parts, shift) add up piece by piece; a record cut differently is put together first and joins piece 0, whose weight is 1.
// parts == 1: the result is the whole point, written to acc[2g + side]; else to pieces[(2g + side) * parts + j] and, in the form
// the Miller lines are evaluated at (X Z, Y, Z^3), to ready[...].  fold_failed[g] = total failed proofs over all records, saturating.
// A malformed record — parts outside 1 .. H2V_ACC_RECORD_PIECES (a record never written is one), or a foreign cut with
// shift (parts - 1) > ACC_RECORD_MAX_SPAN — contributes the identity and counts as max(its failed word, 1) failed proofs: the fold cannot pass.
__global__ void __launch_bounds__(64) k_fold_records(const AccRecord* __restrict__ recs, uint32_t n_recs, uint32_t groups, uint32_t parts, uint32_t shift,
                                                     G1J* __restrict__ acc, G1JSlot* __restrict__ pieces, G1JSlot* __restrict__ ready, uint32_t* __restrict__ fold_failed) {
    // a team of eight lanes per output point: lane r adds the records r, r + 8, ..., then a three-level butterfly — the sum over the
    // ranks is on the critical path of every sharded launch (eight ranks: 4 dependent additions instead of 8)
    const uint32_t k = (blockIdx.x * blockDim.x + threadIdx.x) >> 3, r = threadIdx.x & 7u;
    const bool live = k < 2 * groups * parts;
    const uint32_t j = live ? k % parts : 0, gs2 = live ? k / parts : 0, g = gs2 >> 1, side = gs2 & 1u;
    G1J sum = G1J::identity();
    uint32_t failed = 0;
    if (live) for (uint32_t i = r; i < n_recs; i += 8) {
        const AccRecord& rec = recs[(size_t)i * groups + g];
        const G1J* pc = side ? rec.right : rec.left;
        const bool sized = rec.parts >= 1 && rec.parts <= H2V_ACC_RECORD_PIECES;
        const bool same = sized && rec.parts == parts && (rec.shift == shift || parts == 1);
        const bool foreign = sized && !same && (uint64_t)rec.shift * (rec.parts - 1) <= ACC_RECORD_MAX_SPAN;
        if (same) sum = g1_add(sum, pc[j]);
        else if (foreign && j == 0) sum = g1_add(sum, acc_record_whole(pc, rec.parts, rec.shift));
        failed = sat_add_u32(failed, same || foreign ? rec.failed : (rec.failed ? rec.failed : 1u));
    }
    for (uint32_t d = 4; d > 0; d >>= 1) {
        G1J other;
        uint32_t* dst = reinterpret_cast<uint32_t*>(&other);
        const uint32_t* src = reinterpret_cast<const uint32_t*>(&sum);
#pragma unroll
        for (uint32_t w = 0; w < sizeof(G1J) / 4; ++w) dst[w] = (uint32_t)__shfl_down((int)src[w], d, 8);
        sum = g1_add(sum, other);   // lanes r >= 8 - d add a value they do not own: only r = 0 is kept
        failed = sat_add_u32(failed, (uint32_t)__shfl_down((int)failed, d, 8));
    }
    if (!live || r) return;
    if (parts == 1) acc[gs2] = sum;
    else {
        pieces[k] = sum;
        G1J rd; rd.X = sum.X * sum.Z; rd.Y = sum.Y; rd.Z = sum.Z.sqr() * sum.Z;
        ready[k] = rd;
    }
    if (j == 0 && side == 0) fold_failed[g] = failed;
}
int export_records_enqueue(hipStream_t s, const G1J* d_acc, const G1JSlot* d_pieces, uint32_t parts, uint32_t shift, const int* d_status, uint32_t n, uint32_t groups, void* d_out) {
    if (!d_pieces) { parts = 1; shift = 0; }
    hipLaunchKernelGGL(k_export_records, dim3(groups), dim3(256), 0, s, d_acc, d_pieces, parts, shift, d_status, n / groups, (AccRecord*)d_out);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
int fold_records_enqueue(hipStream_t s, const void* d_recs, uint32_t n_recs, uint32_t groups, uint32_t parts, uint32_t shift, G1J* d_acc, G1JSlot* d_pieces, G1JSlot* d_ready,
                         uint32_t* d_fold_failed) {
    if (parts <= 1 || !d_pieces) { parts = 1; shift = 0; }
    hipLaunchKernelGGL(k_fold_records, dim3((8 * 2 * groups * parts + 63) / 64), dim3(64), 0, s, (const AccRecord*)d_recs, n_recs, groups, parts, shift, d_acc, d_pieces, d_ready, d_fold_failed);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}

// The fold of a merge (h2v_accumulator_merge, accumulator.hip): acc[side] <- acc[side] + sum_k recs[k][side] over n whole-point records
// (parts = 1, what k_accumulator_scale writes; a record's failed word is not read: the counters of a merge are the host's), and, with
// `sums`, record k's two points into the journal slot the host assigned: sums[2 slot + side], slot = slots[k] (slots null: slot = k).
// One one-wave workgroup per side.  The team is the first `team` lanes, a power of two in 1 .. 64 that the host fits to n (k_fold_records'
// team is eight lanes whatever the count: 67 dependent additions at 512 records, 9 + 6 here): lane r adds the items r, r + team, ..,
// item 0 the previous accumulator and item i the record i - 1, then a butterfly of log2(team) levels over the words of a G1J.  Every
// addition is the complete one (items may be identities, equal, or each other's negatives).  Lane 0 writes acc[side], the kernel's last
// store, after it has read it; the slots are written before it.
__global__ void __launch_bounds__(64) k_accumulator_merge_fold(const AccRecord* __restrict__ recs, uint32_t n, uint32_t team, const uint32_t* __restrict__ slots,
                                                               G1J* __restrict__ sums, G1J* __restrict__ acc) {
    const uint32_t side = blockIdx.x, lane = threadIdx.x;
    if (sums)
        for (uint32_t k = lane; k < n; k += 64) sums[2 * (size_t)(slots ? slots[k] : k) + side] = (side ? recs[k].right : recs[k].left)[0];
    G1J sum = G1J::identity();
    if (lane < team)
        for (uint32_t i = lane; i <= n; i += team) sum = g1_add(sum, i ? (side ? recs[i - 1].right : recs[i - 1].left)[0] : acc[side]);
    for (uint32_t d = team >> 1; d > 0; d >>= 1) {
        G1J other;
        uint32_t* dst = reinterpret_cast<uint32_t*>(&other);
        const uint32_t* src = reinterpret_cast<const uint32_t*>(&sum);
#pragma unroll
        for (uint32_t w = 0; w < sizeof(G1J) / 4; ++w) dst[w] = (uint32_t)__shfl_down((int)src[w], d, 64);
        sum = g1_add(sum, other);   // lanes r >= d add a value that is not part of the sum: only lane 0 is kept
    }
    if (lane == 0) acc[side] = sum;
}
uint32_t accumulator_merge_team(uint32_t n) {
    uint32_t t = 1;
    while (t < 64 && t < n + 1) t <<= 1;
    return t;
}
int accumulator_merge_fold_enqueue(hipStream_t s, const void* d_recs, uint32_t n, uint32_t team, const uint32_t* d_slots, G1J* d_sums, G1J* d_acc) {
    if (!team) team = accumulator_merge_team(n);
    if (team > 64 || (team & (team - 1))) { set_last_error("accumulator_merge_fold_enqueue: the team is not a power of two in 1 .. 64"); return H2V_ERR_BAD_ARGUMENT; }
    hipLaunchKernelGGL(k_accumulator_merge_fold, dim3(2), dim3(64), 0, s, (const AccRecord*)d_recs, n, team, d_slots, d_sums, d_acc);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}

// The fold of a batch's legs (h2v_accumulator_process_batch, accumulator.hip): acc[side] <- sum_i recs[i][side] over n whole-point records
// — it REPLACES the accumulator: record 0 is the scaled accumulator M (L, R), record 1 + g is W_g S_g, all written by one
// k_accumulator_scale launch.  With `sums`, the UNSCALED pair of leg g, pairs[2 g + side], goes into the journal slot the host assigned:
// sums[2 slot + side], slot = slots[g] (slots null: slot = g), for the n - 1 legs.  k_accumulator_merge_fold's shape: one one-wave
// workgroup per side, a team of the first `team` lanes (a power of two in 1 .. 64), lane r adds the records r, r + team, .., then a
// butterfly of log2(team) levels; every addition is the complete one (records may be identities, equal, or each other's negatives).
// The slots are written before acc[side], lane 0's store and the kernel's last.
__global__ void __launch_bounds__(64) k_accumulator_legs_fold(const AccRecord* __restrict__ recs, uint32_t n, uint32_t team, const G1J* __restrict__ pairs,
                                                              const uint32_t* __restrict__ slots, G1J* __restrict__ sums, G1J* __restrict__ acc) {
    const uint32_t side = blockIdx.x, lane = threadIdx.x;
    if (sums)
        for (uint32_t g = lane; g + 1 < n; g += 64) sums[2 * (size_t)(slots ? slots[g] : g) + side] = pairs[2 * (size_t)g + side];
    G1J sum = G1J::identity();
    if (lane < team)
        for (uint32_t i = lane; i < n; i += team) sum = g1_add(sum, (side ? recs[i].right : recs[i].left)[0]);
    for (uint32_t d = team >> 1; d > 0; d >>= 1) {
        G1J other;
        uint32_t* dst = reinterpret_cast<uint32_t*>(&other);
        const uint32_t* src = reinterpret_cast<const uint32_t*>(&sum);
#pragma unroll
        for (uint32_t w = 0; w < sizeof(G1J) / 4; ++w) dst[w] = (uint32_t)__shfl_down((int)src[w], d, 64);
        sum = g1_add(sum, other);   // lanes r >= d add a value that is not part of the sum: only lane 0 is kept
    }
    if (lane == 0) acc[side] = sum;
}
int accumulator_legs_fold_enqueue(hipStream_t s, const void* d_recs, uint32_t n, uint32_t team, const G1J* d_pairs, const uint32_t* d_slots, G1J* d_sums, G1J* d_acc) {
    if (!n) { set_last_error("accumulator_legs_fold_enqueue: no record"); return H2V_ERR_BAD_ARGUMENT; }
    if (!team) team = accumulator_merge_team(n - 1);   // (n items, as a merge of n - 1 records has)
    if (team > 64 || (team & (team - 1))) { set_last_error("accumulator_legs_fold_enqueue: the team is not a power of two in 1 .. 64"); return H2V_ERR_BAD_ARGUMENT; }
    if (d_sums && n > 1 && !d_pairs) { set_last_error("accumulator_legs_fold_enqueue: journal slots without the legs' pairs"); return H2V_ERR_BAD_ARGUMENT; }
    hipLaunchKernelGGL(k_accumulator_legs_fold, dim3(2), dim3(64), 0, s, (const AccRecord*)d_recs, n, team, d_pairs, d_slots, d_sums, d_acc);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- an enqueued feed of a batch's legs (h2v_accumulator_feed_batch, accumulator.hip; include/h2v_feed.h): the two kernels around
// k_feed_weights (verify_kernels.hip), k_accumulator_scale and k_accumulator_legs_fold, on the accumulator's stream.
//
// k_feed_gather: everything the feed reads of the batch but its draws, into arrays of the accumulator's own, so that the batch is free
// once this and k_feed_weights have run (no copy engine: k_copy_words' reason below).  Workgroup g: the words of the batch's sums
// sums[2 g], [2 g + 1] -> pairs[2 + 2 g], [3 + 2 g] (workgroup 0 also acc[0], [1] -> pairs[0], [1]); sizes[g] <- the group's proofs,
// failed[g] <- its non-zero status words (a strided count per thread, a butterfly per wave, the four waves' counts through LDS).
// gfx950 (-Rpass-analysis=kernel-resource-usage): DESIGN.md section 3, "An enqueued feed".
#define FEED_GATHER_THREADS 256u
__global__ void __launch_bounds__(FEED_GATHER_THREADS) k_feed_gather(const G1J* __restrict__ acc, const G1J* __restrict__ sums, const int* __restrict__ status, GroupShape shape,
                                                                     G1J* __restrict__ pairs, uint32_t* __restrict__ sizes, uint32_t* __restrict__ failed) {
    __shared__ uint32_t wave_count[FEED_GATHER_THREADS / 64];
    constexpr uint32_t PAIR_WORDS = 2 * sizeof(G1J) / 4;
    const uint32_t g = blockIdx.x, t = threadIdx.x;
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(sums + 2 * (size_t)g);
        uint32_t* dst = reinterpret_cast<uint32_t*>(pairs + 2 + 2 * (size_t)g);
        for (uint32_t w = t; w < PAIR_WORDS; w += FEED_GATHER_THREADS) dst[w] = src[w];
        if (g == 0) {
            const uint32_t* a = reinterpret_cast<const uint32_t*>(acc);
            uint32_t* d0 = reinterpret_cast<uint32_t*>(pairs);
            for (uint32_t w = t; w < PAIR_WORDS; w += FEED_GATHER_THREADS) d0[w] = a[w];
        }
    }
    const uint32_t first = shape.first(g), count = shape.count(g);
    uint32_t c = 0;
    for (uint32_t i = t; i < count; i += FEED_GATHER_THREADS) c += status[first + i] != 0 ? 1u : 0u;
    for (uint32_t d = 32; d > 0; d >>= 1) c += (uint32_t)__shfl_down((int)c, d, 64);
    if ((t & 63u) == 0) wave_count[t >> 6] = c;
    __syncthreads();
    if (t == 0) {
        uint32_t all = 0;
        for (uint32_t w = 0; w < FEED_GATHER_THREADS / 64; ++w) all += wave_count[w];
        sizes[g] = count; failed[g] = all;
    }
}
int feed_gather_enqueue(hipStream_t s, const G1J* d_acc, const G1J* d_sums, const int* d_status, const GroupShape& shape, G1J* d_pairs, uint32_t* d_sizes, uint32_t* d_failed) {
    if (!shape.G || !d_acc || !d_sums || !d_status || !d_pairs || !d_sizes || !d_failed) { set_last_error("feed_gather_enqueue: null argument or no group"); return H2V_ERR_BAD_ARGUMENT; }
    hipLaunchKernelGGL(k_feed_gather, dim3(shape.G), dim3(FEED_GATHER_THREADS), 0, s, d_acc, d_sums, d_status, shape, d_pairs, d_sizes, d_failed);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
// k_feed_report, a feed's last kernel: the report into mapped pinned memory, [rc, n, G, failed] and per group [M_g x 8, size, failed],
// from the accumulator's own scratch (legs: k_feed_weights; sizes, failed: k_feed_gather).  One workgroup, thread t the groups t,
// t + 256, ..; the total of the failed counts meets in LDS.  Plain vector stores, a system-scope fence behind them (k_ingest_draws'
// verdict block); the host reads the report behind a synchronise of the accumulator's stream (h2v_accumulator_settle).
// gfx950 (-Rpass-analysis=kernel-resource-usage): DESIGN.md section 3, "An enqueued feed".
__global__ void __launch_bounds__(256) k_feed_report(const uint32_t* __restrict__ rc, uint32_t n, uint32_t G, const uint32_t* __restrict__ legs,
                                                     const uint32_t* __restrict__ sizes, const uint32_t* __restrict__ failed, uint32_t* __restrict__ report) {
    __shared__ uint32_t total;
    const uint32_t t = threadIdx.x;
    if (t == 0) total = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t g = t; g < G; g += 256) {
        uint32_t* row = report + 4 + 10 * (size_t)g;
        for (uint32_t j = 0; j < 8; ++j) row[j] = legs[8 * (size_t)g + j];
        row[8] = sizes[g]; row[9] = failed[g];
        mine += failed[g];
    }
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    if (t == 0) { report[0] = rc[0]; report[1] = n; report[2] = G; report[3] = total; }
    __threadfence_system();
}
int feed_report_enqueue(hipStream_t s, const uint32_t* d_rc, uint32_t n, uint32_t G, const uint32_t* d_legs, const uint32_t* d_sizes, const uint32_t* d_failed, uint32_t* d_report) {
    if (!G || !d_rc || !d_legs || !d_sizes || !d_failed || !d_report) { set_last_error("feed_report_enqueue: null argument or no group"); return H2V_ERR_BAD_ARGUMENT; }
    hipLaunchKernelGGL(k_feed_report, dim3(1), dim3(256), 0, s, d_rc, n, G, d_legs, d_sizes, d_failed, d_report);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}

__global__ void k_affine_to_jacobian(const G1A* __restrict__ in, G1J* __restrict__ out, uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = G1J::from_affine(in[i]);
}
int affine_to_jacobian_enqueue(hipStream_t s, const G1A* d_in, G1J* d_out, uint32_t n) {
    if (!n) return 0;
    hipLaunchKernelGGL(k_affine_to_jacobian, dim3((n + 63) / 64), dim3(64), 0, s, d_in, d_out, n);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}

int bases_from_bytes_enqueue(hipStream_t s, const uint8_t* d_bytes, G1A* d_out, uint32_t* d_flags, uint32_t n) {
    if (!n) return 0;
    hipLaunchKernelGGL(k_bases_from_bytes, dim3((n + 255) / 256), dim3(256), 0, s, d_bytes, d_out, d_flags, n);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
int scalars_from_bytes_enqueue(hipStream_t s, const uint8_t* d_bytes, uint32_t* d_out, uint32_t* d_flags, uint32_t n) {
    if (!n) return 0;
    hipLaunchKernelGGL(k_scalars_from_bytes, dim3((n + 255) / 256), dim3(256), 0, s, d_bytes, d_out, d_flags, n);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
int guard_terms_enqueue(hipStream_t s, const uint8_t* d_scalars32, const uint8_t* d_bases64, const uint32_t* d_guard_of_term, const Fr* d_mult, uint32_t* d_out_scalars,
                        G1A* d_out_bases, uint32_t* d_first_bad, uint32_t n) {
    if (!d_first_bad || (n && (!d_scalars32 || !d_bases64 || !d_out_scalars || !d_out_bases)) || (n && d_mult && !d_guard_of_term)) {
        set_last_error("guard_terms_enqueue: null argument"); return H2V_ERR_BAD_ARGUMENT;
    }
    if (((uintptr_t)d_scalars32 | (uintptr_t)d_bases64 | (uintptr_t)d_out_scalars) & 15u) { set_last_error("guard_terms_enqueue: an array off a 16-byte boundary"); return H2V_ERR_BAD_ARGUMENT; }
    H2V_HIP_CHECK(hipMemsetAsync(d_first_bad, 0xff, 4, s));
    if (!n) return 0;
    hipLaunchKernelGGL(k_guard_terms, dim3((n + 255) / 256), dim3(256), 0, s, (const uint4*)d_scalars32, (const uint4*)d_bases64, d_guard_of_term, d_mult, (uint4*)d_out_scalars, d_out_bases,
                       d_first_bad, n);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
int msm_scale_enqueue(hipStream_t s, uint32_t* d_words, const Fr& factor, uint32_t n) {
    if (!n) return 0;
    if (!d_words) { set_last_error("msm_scale_enqueue: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if ((uintptr_t)d_words & 15u) { set_last_error("msm_scale_enqueue: the words off a 16-byte boundary"); return H2V_ERR_BAD_ARGUMENT; }
    hipLaunchKernelGGL(k_msm_scale, dim3((n + 255) / 256), dim3(256), 0, s, (uint4*)d_words, factor, n);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
int affine_to_bytes_enqueue(hipStream_t s, const G1A* d_in, uint8_t* d_out, uint32_t n) {
    if (!n) return 0;
    if (!d_in || !d_out) { set_last_error("affine_to_bytes_enqueue: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if ((uintptr_t)d_out & 15u) { set_last_error("affine_to_bytes_enqueue: the bytes off a 16-byte boundary"); return H2V_ERR_BAD_ARGUMENT; }
    hipLaunchKernelGGL(k_affine_to_bytes, dim3((n + 255) / 256), dim3(256), 0, s, d_in, (uint4*)d_out, n);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
// device words -> (mapped host) words by a kernel.  A hipMemcpyAsync enqueued at launch time, behind kernels that finish milliseconds later,
// may sit on an SDMA engine's in-order queue with its dependency unmet — and the host -> device copies of the NEXT launches queue up behind
// it (measured: with several launches in flight, h2v_batch_upload_launch blocked for a whole launch, 13.1 -> 8.1 M proofs/s PCIe-inclusive).
__global__ void __launch_bounds__(256) k_copy_words(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, uint32_t n_words) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_words) dst[i] = src[i];
}
int copy_words_enqueue(hipStream_t s, const void* d_src, void* d_dst, size_t n_words, size_t lds_reserve) {
    if (!n_words) return 0;
    if (lds_reserve > 64 * 1024) H2V_HIP_CHECK(hipFuncSetAttribute((const void*)k_copy_words, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_reserve));
    hipLaunchKernelGGL(k_copy_words, dim3((uint32_t)((n_words + 255) / 256)), dim3(256), lds_reserve, s, (const uint32_t*)d_src, (uint32_t*)d_dst, (uint32_t)n_words);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
// ---- an upload from device memory (h2v_batch_upload_device, batch.hip): two launches, both on the batch's stream.
// The verdict block is [fault][zero_below x G][blocks done] on the device and its first 1 + G words in the batch's pinned host memory.
//
// k_ingest_rows: the caller's strided proof rows -> the batch's packed proofs, and the instance bytes behind them in the same launch
// (by a kernel, not hipMemcpy2DAsync: k_copy_words' reason above).  One 16-byte load and one 16-byte store per thread: thread i owns
// 16-byte word i of the packed rows (row i / row16, word i % row16 of it: consecutive lanes read consecutive words of a row and write
// consecutive words of the output), the threads behind the rows own the instance words; a thread past both touches nothing.  The first
// workgroup also presets the verdict block for k_ingest_draws, which runs behind it on the stream: fault 0xffffffff, the rest 0.
// gfx950 (tools/kernel_resources.py): 14 VGPRs, 24 SGPRs, no spills, no scratch, no LDS; 8 waves per SIMD.
__global__ void __launch_bounds__(256) k_ingest_rows(const uint4* __restrict__ rows, uint32_t stride16, uint32_t row16, uint64_t rows16, const uint4* __restrict__ inst,
                                                     uint64_t inst16, uint4* __restrict__ out_rows, uint4* __restrict__ out_inst, uint32_t* __restrict__ verdict,
                                                     uint32_t n_verdict) {
    if (blockIdx.x == 0)
        for (uint32_t t = threadIdx.x; t < n_verdict; t += 256) verdict[t] = t ? 0u : 0xffffffffu;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < rows16) {
        const uint64_t r = i / row16;
        out_rows[i] = rows[r * stride16 + (i - r * row16)];
    } else if (i - rows16 < inst16) out_inst[i - rows16] = inst[i - rows16];
}
// k_ingest_draws: one thread per draw of the caller's tail, the checks the host makes for a tail in host memory (upload_impl): two
// 16-byte loads, Fr::geq_p and a zero test as k_guard_terms reads its scalars.  The draw goes into the batch's tail, or the scalar 1
// in place of a draw >= r, whose index joins verdict[0] by atomicMin (a stored zero would zero the multipliers of the earlier proofs
// and drop them out of the accumulators).  A zero draw, the j-th of group g's draws (GroupShape::draw_at), raises zero_below[g] =
// verdict[1 + g] by atomicMax to GroupShape::zero_below(j, g): the loop of zero_below_of_draws (batch.hip), a thread per draw.  The
// workgroup that finishes last (a count of the workgroups done, behind a device-wide fence) sends the 1 + G verdict words to
// host_verdict, so the verdict needs no third launch.
// gfx950 (tools/kernel_resources.py): 22 VGPRs, 48 SGPRs, no spills, no scratch, 4 bytes of LDS; 8 waves per SIMD.
__global__ void __launch_bounds__(256) k_ingest_draws(const uint4* __restrict__ draws, uint4* __restrict__ tail, uint32_t n_tail, GroupShape shape,
                                                      uint32_t* __restrict__ verdict, uint32_t* __restrict__ host_verdict) {
    __shared__ uint32_t last;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_tail) {
        const uint4 s0 = draws[2 * (size_t)i], s1 = draws[2 * (size_t)i + 1];
        const uint32_t raw[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
        const bool zero = !(s0.x | s0.y | s0.z | s0.w | s1.x | s1.y | s1.z | s1.w);
        if (Fr::geq_p(raw)) {
            atomicMin(&verdict[0], i);
            tail[2 * (size_t)i] = make_uint4(1, 0, 0, 0); tail[2 * (size_t)i + 1] = make_uint4(0, 0, 0, 0);
        } else { tail[2 * (size_t)i] = s0; tail[2 * (size_t)i + 1] = s1; }
        if (zero) {
            const GroupShape::Draw d = shape.draw_at(i);
            if (const uint32_t below = shape.zero_below(d.j, d.g)) atomicMax(&verdict[1 + d.g], below);
        }
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) last = atomicAdd(&verdict[1 + shape.G], 1u) == gridDim.x - 1 ? 1u : 0u;
    __syncthreads();
    if (!last) return;
    for (uint32_t t = threadIdx.x; t < 1 + shape.G; t += 256) host_verdict[t] = __hip_atomic_load(&verdict[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// k_ingest_rows (util.hip) the other way round: thread i owns 16-byte word i of the packed rows (row i / row16, word i % row16 of it)
// and stores it into the caller's row; the bytes between the caller's rows are not touched.  One 16-byte load and store per thread.
__global__ void __launch_bounds__(256) k_hint_rows_out(const uint4* __restrict__ rows, uint32_t row16, uint64_t rows16, uint4* __restrict__ out, uint32_t stride16) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows16) return;
    const uint64_t r = i / row16;
    out[r * stride16 + (i - r * row16)] = rows[i];
}

int hint_rows_out_enqueue(hipStream_t s, const uint8_t* d_rows, size_t row_len, size_t n, void* d_out, size_t stride) {
    if (!n || !row_len) return 0;
    if (!d_rows || !d_out) { set_last_error("hint_rows_out_enqueue: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if (((uintptr_t)d_rows | (uintptr_t)d_out | stride | row_len) & 15u) { set_last_error("hint_rows_out_enqueue: a pointer, the stride or the length is not a multiple of 16 bytes"); return H2V_ERR_BAD_ARGUMENT; }
    if (stride < row_len || (stride >> 4) > 0xffffffffu) { set_last_error("hint_rows_out_enqueue: the stride is below the row length, or too large"); return H2V_ERR_BAD_ARGUMENT; }
    const uint64_t rows16 = (uint64_t)n * (row_len >> 4);
    if (rows16 > 0xffffff00ull) { set_last_error("hint_rows_out_enqueue: too many bytes for one launch"); return H2V_ERR_BAD_ARGUMENT; }
    hipLaunchKernelGGL(k_hint_rows_out, dim3((uint32_t)((rows16 + 255) / 256)), dim3(256), 0, s, (const uint4*)d_rows, (uint32_t)(row_len >> 4), rows16, (uint4*)d_out, (uint32_t)(stride >> 4));
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
int ingest_rows_enqueue(hipStream_t s, const void* d_rows, size_t stride, size_t row_len, size_t n, const void* d_inst, size_t inst_bytes, uint8_t* d_out_rows,
                        uint8_t* d_out_inst, uint32_t* d_verdict, uint32_t groups) {
    if ((n && row_len && (!d_rows || !d_out_rows)) || (inst_bytes && (!d_inst || !d_out_inst))) { set_last_error("ingest_rows_enqueue: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if (((uintptr_t)d_rows | (uintptr_t)d_inst | (uintptr_t)d_out_rows | (uintptr_t)d_out_inst | stride | row_len | inst_bytes) & 15u) {
        set_last_error("ingest_rows_enqueue: a pointer, the stride or a length is not a multiple of 16 bytes"); return H2V_ERR_BAD_ARGUMENT;
    }
    if (stride < row_len || (stride >> 4) > 0xffffffffu) { set_last_error("ingest_rows_enqueue: the stride is below the row length, or too large"); return H2V_ERR_BAD_ARGUMENT; }
    const uint64_t rows16 = (uint64_t)n * (row_len >> 4), inst16 = inst_bytes >> 4;
    if (rows16 + inst16 > 0xffffff00ull) { set_last_error("ingest_rows_enqueue: too many bytes for one launch"); return H2V_ERR_BAD_ARGUMENT; }
    const uint64_t blocks = (rows16 + inst16 + 255) / 256;
    if (!blocks && !d_verdict) return 0;
    hipLaunchKernelGGL(k_ingest_rows, dim3((uint32_t)(blocks ? blocks : 1)), dim3(256), 0, s, (const uint4*)d_rows, (uint32_t)(stride >> 4), (uint32_t)(row_len >> 4), rows16,
                       (const uint4*)d_inst, inst16, (uint4*)d_out_rows, (uint4*)d_out_inst, d_verdict, d_verdict ? groups + 2 : 0u);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
int ingest_draws_enqueue(hipStream_t s, const void* d_draws, uint8_t* d_tail, uint32_t n_tail, uint32_t n, const GroupShape& shape, uint32_t* d_verdict, uint32_t* d_host_verdict) {
    if (!shape.G || !d_verdict || !d_host_verdict || (n_tail && (!d_draws || !d_tail))) { set_last_error("ingest_draws_enqueue: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if (((uintptr_t)d_draws | (uintptr_t)d_tail) & 15u) { set_last_error("ingest_draws_enqueue: an array off a 16-byte boundary"); return H2V_ERR_BAD_ARGUMENT; }
    if (!shape.fits(n, n_tail, true)) { set_last_error("ingest_draws_enqueue: the draws do not match the groups"); return H2V_ERR_BAD_ARGUMENT; }
    // (no draw: one workgroup still sends the preset verdict)
    hipLaunchKernelGGL(k_ingest_draws, dim3(n_tail ? (n_tail + 255) / 256 : 1), dim3(256), 0, s, (const uint4*)d_draws, (uint4*)d_tail, n_tail, shape, d_verdict, d_host_verdict);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
// ---- a finish into device memory (h2v_batch_finish_device, batch.hip): what finish_impl hands the host, written by kernels on the
// batch's stream into the caller's device arrays — two launches, and a third when the failing proofs' indices are wanted.  No copy
// engine (k_copy_words' reason above).  The scratch is a word per tile of 256 proofs and a word per group; the group words are ZERO
// on entry and are left zero: k_results_close clears each after reading it, so no launch is spent on zeroing.
//
// k_results_tiles: one thread per proof, a workgroup per tile of RESULTS_TILE.  The status word is decoded (status_decode, batch.h) and
// stored, 4 bytes per lane, consecutive lanes to consecutive words.  A wave's failing lanes (status != 0) are one 64-bit ballot: its
// popcount goes into the tile's count through LDS, and into the groups' words by one atomicAdd per group present among them — the lanes of
// the lowest failing lane's group are peeled off the ballot until it is empty, so a wave without a failing proof (every wave of a clean
// launch) does no lookup and no atomic.  Only failing lanes find their group (GroupShape::of).  The sums do not depend on the order of
// the additions.
// gfx950 (tools/kernel_resources.py): 10 VGPRs, 26 SGPRs, no spills, no scratch, 16 bytes of LDS; 8 waves per SIMD.
#define RESULTS_TILE 256u
__global__ void __launch_bounds__(RESULTS_TILE) k_results_tiles(const int* __restrict__ status, uint32_t n, GroupShape shape, int* __restrict__ out_status,
                                                                uint32_t* __restrict__ tile_count, uint32_t* __restrict__ group_failed) {
    __shared__ uint32_t wave_count[RESULTS_TILE / 64];
    const uint32_t t = threadIdx.x, lane = t & 63u, i = blockIdx.x * RESULTS_TILE + t;
    const int w = i < n ? status[i] : 0;
    if (i < n && out_status) out_status[i] = status_decode(w);
    unsigned long long failing = __ballot(w != 0);
    if (lane == 0) wave_count[t >> 6] = (uint32_t)__popcll(failing);
    const uint32_t g = w != 0 ? shape.of(i) : 0;
    while (failing) {   // (the same value in every lane of the wave)
        const uint32_t leader = (uint32_t)__ffsll((long long)failing) - 1;
        const uint32_t gl = (uint32_t)__shfl((int)g, (int)leader);
        const unsigned long long same = __ballot(w != 0 && g == gl);
        if (lane == leader) atomicAdd(&group_failed[gl], (uint32_t)__popcll(same));
        failing &= ~same;
    }
    __syncthreads();
    if (t == 0) tile_count[blockIdx.x] = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
}
// k_results_close: ONE workgroup, behind k_results_tiles on the stream (its own launch: see DESIGN.md, "A finish into device memory").
//  - the tile counts become their exclusive prefix sums in place, 256 tiles per pass with the running total carried from pass to pass
//    (as k_seg_mult_scan_tiles carries its value); the total is the number of failing proofs;
//  - a thread per group: group_ok = no failing proof && !fold_failed && (no pairing of the launch's own || ok) && no draw fault, the
//    group's word of the scratch read and cleared, the 128 bytes of its accumulators split into the caller's two arrays (16 bytes a thread);
//  - the summary words (h2v.h).
// `ok` is host memory behind a mapped pointer, written by the pairing kernel earlier on the same stream: it is read by an atomic load
// of SYSTEM scope, which goes past the vector cache and the device's L2 to the memory itself; a plain (cached) vector load could be
// served a line that was fetched before the pairing kernel's store arrived.
// gfx950 (tools/kernel_resources.py): 18 VGPRs, 49 SGPRs, no spills, no scratch, 1028 bytes of LDS.
__global__ void __launch_bounds__(256) k_results_close(uint32_t* __restrict__ tile_count, uint32_t tiles, uint32_t* __restrict__ group_failed, uint32_t G, uint32_t n,
                                                       const uint32_t* __restrict__ fold_failed, const uint32_t* ok, uint32_t flags, const uint4* __restrict__ out_bytes,
                                                       const uint32_t* __restrict__ fault, int* __restrict__ out_group_ok, uint4* __restrict__ out_left,
                                                       uint4* __restrict__ out_right, uint32_t* __restrict__ out_group_failed, uint32_t* __restrict__ summary) {
    __shared__ uint32_t part[256];
    __shared__ uint32_t n_ok;
    const uint32_t t = threadIdx.x;
    if (t == 0) n_ok = 0;
    uint32_t total = 0;
    for (uint32_t base = 0; base < tiles; base += 256) {
        const uint32_t v = base + t < tiles ? tile_count[base + t] : 0;
        part[t] = v;
        __syncthreads();
        for (uint32_t d = 1; d < 256; d <<= 1) {
            const uint32_t below = t >= d ? part[t - d] : 0;
            __syncthreads();
            part[t] += below;
            __syncthreads();
        }
        if (base + t < tiles) tile_count[base + t] = total + part[t] - v;
        total += part[255];
        __syncthreads();
    }
    __syncthreads();   // (n_ok = 0 before the first addition, also without a tile)
    const uint32_t fault_word = fault ? fault[0] : 0xffffffffu;
    for (uint32_t g = t; g < G; g += 256) {
        const uint32_t failed = group_failed[g];
        group_failed[g] = 0;
        const uint32_t paired = (flags & 1u) ? __hip_atomic_load(&ok[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 1u;
        const bool good = !failed && !fold_failed[g] && paired && fault_word == 0xffffffffu;
        if (out_group_ok) out_group_ok[g] = good ? 1 : 0;
        if (out_group_failed) out_group_failed[g] = failed;
        if (good) atomicAdd(&n_ok, 1u);
    }
    if (out_left || out_right)
        for (uint32_t q = t; q < 8 * G; q += 256) {   // 16-byte word q & 7 of group q >> 3: 0 .. 3 left, 4 .. 7 right
            const uint32_t g = q >> 3, k = q & 7u;
            uint4* const dst = k < 4 ? out_left : out_right;
            if (dst) dst[4 * (size_t)g + (k & 3u)] = out_bytes[q];
        }
    __syncthreads();
    if (t < 8 && summary) summary[t] = t == 0 ? fault_word : t == 1 ? total : t == 2 ? n_ok : t == 3 ? n : t == 4 ? G : t == 5 ? flags : 0u;
}
// k_results_scatter: the failing proofs' indices, ascending.  A tile's failing lanes go to [the tile's offset (k_results_close's prefix
// sum) + the lane's rank inside the tile), the rank being the failing lanes below it in its wave's ballot plus the earlier waves' counts
// from LDS; tiles follow each other in the offsets and lanes in the ranks, so the output is sorted without a sort.  A position from
// `cap` on is not written.
// gfx950 (tools/kernel_resources.py): 14 VGPRs, 20 SGPRs, no spills, no scratch, 16 bytes of LDS; 8 waves per SIMD.
__global__ void __launch_bounds__(RESULTS_TILE) k_results_scatter(const int* __restrict__ status, uint32_t n, const uint32_t* __restrict__ tile_offset,
                                                                  uint32_t* __restrict__ failed_index, uint32_t cap) {
    __shared__ uint32_t wave_count[RESULTS_TILE / 64];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6, i = blockIdx.x * RESULTS_TILE + t;
    const int w = i < n ? status[i] : 0;
    const unsigned long long failing = __ballot(w != 0);
    if (lane == 0) wave_count[wave] = (uint32_t)__popcll(failing);
    __syncthreads();
    if (w == 0) return;
    uint32_t pos = tile_offset[blockIdx.x] + (uint32_t)__popcll(failing & ((1ull << lane) - 1ull));
    for (uint32_t k = 0; k < wave; ++k) pos += wave_count[k];
    if (pos < cap) failed_index[pos] = i;
}
int results_enqueue(hipStream_t s, const int* d_status, uint32_t n, const GroupShape& shape, const uint32_t* d_fold_failed, const uint32_t* d_ok, uint32_t flags,
                    const uint8_t* d_out_bytes, const uint32_t* d_fault, uint32_t* d_tile_words, uint32_t* d_group_words, const ResultsOut& out) {
    const uint32_t groups = shape.G;
    if (!groups || !d_fold_failed || !d_out_bytes || !d_group_words || (n && (!d_status || !d_tile_words)) || ((flags & 1u) && !d_ok)) { set_last_error("results_enqueue: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if (((uintptr_t)d_out_bytes | (uintptr_t)out.left_xy | (uintptr_t)out.right_xy) & 15u) { set_last_error("results_enqueue: accumulator bytes off a 16-byte boundary"); return H2V_ERR_BAD_ARGUMENT; }
    if (((uintptr_t)d_status | (uintptr_t)out.status | (uintptr_t)out.group_ok | (uintptr_t)out.group_failed | (uintptr_t)out.failed_index | (uintptr_t)out.summary) & 3u) {
        set_last_error("results_enqueue: a word array off a 4-byte boundary"); return H2V_ERR_BAD_ARGUMENT;
    }
    if (!shape.fits(n, n, false)) { set_last_error("results_enqueue: equal groups do not divide n"); return H2V_ERR_BAD_ARGUMENT; }
    if (groups > (1u << 24) || (flags & ~3u)) { set_last_error("results_enqueue: too many groups, or an unknown flag"); return H2V_ERR_BAD_ARGUMENT; }
    if (out.failed_index && !out.failed_cap) { set_last_error("results_enqueue: failed_cap is 0"); return H2V_ERR_BAD_ARGUMENT; }
    const uint32_t tiles = (uint32_t)(((uint64_t)n + RESULTS_TILE - 1) / RESULTS_TILE);
    uint32_t* const tile_words = d_tile_words;
    uint32_t* const group_words = d_group_words;
    if (tiles) {
        hipLaunchKernelGGL(k_results_tiles, dim3(tiles), dim3(RESULTS_TILE), 0, s, d_status, n, shape, out.status, tile_words, group_words);
        H2V_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_results_close, dim3(1), dim3(256), 0, s, tile_words, tiles, group_words, groups, n, d_fold_failed, d_ok, flags, (const uint4*)d_out_bytes, d_fault,
                       out.group_ok, (uint4*)out.left_xy, (uint4*)out.right_xy, out.group_failed, out.summary);
    H2V_HIP_CHECK(hipGetLastError());
    if (tiles && out.failed_index) {
        hipLaunchKernelGGL(k_results_scatter, dim3(tiles), dim3(RESULTS_TILE), 0, s, d_status, n, tile_words, out.failed_index, out.failed_cap);
        H2V_HIP_CHECK(hipGetLastError());
    }
    return 0;
}
int point_to_bytes_enqueue(hipStream_t s, const G1J* d_in, uint8_t* d_out_xy64, uint32_t* d_is_identity, uint32_t n, size_t lds_reserve) {
    if (!n) return 0;
    if (lds_reserve > 64 * 1024) H2V_HIP_CHECK(hipFuncSetAttribute((const void*)k_point_to_bytes, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_reserve));
    hipLaunchKernelGGL(k_point_to_bytes, dim3((n + 63) / 64), dim3(64), lds_reserve, s, d_in, d_out_xy64, d_is_identity, n);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace h2v
