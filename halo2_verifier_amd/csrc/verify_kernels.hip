// Per-proof kernels of the batch verifier: everything verify_proof (lib.rs:33-425) and
// VerifierSHPLONK::verify_proof (shplonk.rs:175-267) do before the MSMs are evaluated.
//
//   k_decompress      one lane per (proof, point)   G1Affine::from_bytes               transcript/mod.rs:158-166
//   k_decompress_hinted  the same with the claimed y beside every point (include/h2v_hints.h): a curve check, the root only on a miss
//   k_decompress_misses  one lane per point that a wave of k_decompress_hinted with hits and misses listed: its root
//   k_check_scalars   one lane per (proof, scalar)  Fr::from_repr canonicity           transcript/mod.rs:168-176
//   k_stream_build    one lane per (proof, 8-byte word of the absorbed stream)         transcript/mod.rs:216-231
//   k_transcript      four lanes per proof          Blake2b-512 + challenges           transcript/mod.rs:124-133,209-214,500-514
//   k_instance_eval   one workgroup per proof       Lagrange sum over a wide instance column   lib.rs:173-218, poly/domain.rs:187-212
//   k_frvm            one lane per proof            the compiled Fr program            lib.rs:173-346, shplonk.rs:202-264
//   k_seg_mult_tiles ...  a segmented two-level scan  suffix products of the batch draws, group by group   kzg/strategy.rs:129, msm.rs:173-176
//   k_fold_shared     one workgroup per (shared base, group)   sum over the group's proofs of the scalars of VK-wide bases
//   k_fold_ranges     one wave per (shared base, range)   the same over arbitrary ranges of proofs, of one batch or several (h2v_batches_recheck)
//
// Layouts are chosen so that lanes (= proofs) are contiguous in the fastest dimension for
// everything the per-proof kernels re-read: stream words [word][proof], challenges [c][proof],
// program slots [slot][proof], shared scalars [j][proof].
#include "../../include/h2v.h"
#include "batch.h"
#include <atomic>

namespace h2v {

// ------------------------------------------------------------------ point decompression
// k_decompress, k_decompress_hinted and k_decompress_misses, and in front of them the steps they share, each force-inlined into its
// kernels: what is said at a step holds for every kernel that takes it.

// A point's 32 bytes as they lie in its proof, two 16-byte loads (a point sits at a multiple of 32 bytes inside a proof whose length is
// a multiple of 32; round 1 moved every byte on its own: 13x the algorithmic traffic, profiles/r01_pmc_fetch_write.csv), taken apart
// as G1Affine::from_bytes (compressed) takes them: flags in the top byte, x below.
struct PointIn { uint32_t w[8]; bool is_inf, sign; };
__device__ __forceinline__ PointIn point_load(const uint8_t* __restrict__ proofs, uint32_t proof_len, const uint32_t* __restrict__ point_offsets, uint32_t p, uint32_t slot) {
    const uint4* src = reinterpret_cast<const uint4*>(proofs + (size_t)p * proof_len + point_offsets[slot]);
    const uint4 lo = src[0], hi = src[1];
    PointIn in = {{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}, (bool)((hi.w >> 24) & G1_FLAG_IDENTITY), (bool)((hi.w >> 24) & G1_FLAG_SIGN)};
    in.w[7] &= 0x3fffffffu;
    return in;
}
// the curve's right-hand side, x^3 + 3
__device__ __forceinline__ Fq curve_rhs(const Fq& x) {
    const Fq one = {{FqParams::ONE(0), FqParams::ONE(1), FqParams::ONE(2), FqParams::ONE(3), FqParams::ONE(4), FqParams::ONE(5), FqParams::ONE(6), FqParams::ONE(7), FqParams::ONE(8)}};
    return x.sqr() * x + (one + one + one);
}
// a = (x, y) and yraw = the canonical y, from the root of rhs = x^3 + 3 on; false, with a and yraw untouched (the caller
// refuses the point), where rhs has no root.  The canonical y is needed raw: its parity decides the sign, its bytes are absorbed.
__device__ __forceinline__ bool point_from_root(const Fq& x, const Fq& rhs, bool sign, G1A& a, uint32_t yraw[8]) {
    Fq y = fq_sqrt_candidate_loop_w3(rhs);
    if (y.sqr() != rhs) return false;
    y.to_raw(yraw);
    uint32_t nz = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) nz |= yraw[i];
    if ((bool)(yraw[0] & 1u) != sign && nz) {   // the other root: p - y (y = 0 is its own negative)
        y = y.neg();
        uint64_t borrow = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) { const uint64_t d = (uint64_t)FqParams::P(i) - yraw[i] - borrow; yraw[i] = (uint32_t)d; borrow = (d >> 32) & 1u; }
    }
    a.x = x; a.y = y;
    return true;
}
// G1Affine::from_bytes from the bytes on: x < p, not the identity, a root of the right sign
__device__ __forceinline__ bool point_decode(const PointIn& in, G1A& a, uint32_t yraw[8]) {
    if (Fq::geq_p(in.w)) return false;
    const Fq x = Fq::from_raw(in.w);
    if (in.is_inf) return false;   // the identity decodes (x = 0, no sign) but cannot be absorbed ("cannot write points at infinity to the transcript"): an error either way
    return point_from_root(x, curve_rhs(x), in.sign, a, yraw);
}
// what a point that does not decode leaves in its rows: the identity and a zero y
__device__ __forceinline__ void point_none(G1A& a, uint32_t yraw[8]) {
    a = G1A::identity();
    for (int i = 0; i < 8; ++i) yraw[i] = 0;
}
// ... and in its proof's status word, by the slot's kind (status_set: the rank-coded atomic minimum, so the order of refusals does not matter)
__device__ __forceinline__ void point_refuse(int* __restrict__ status, uint32_t p, uint32_t slot, uint32_t n_main_points, G1A& a, uint32_t yraw[8]) {
    status_set(status, p, slot < n_main_points ? H2V_DEV_ST_TRANSCRIPT : H2V_DEV_ST_OPENING);
    point_none(a, yraw);
}
// A workgroup's 64 rows of pts, phi and ycanon (the pointers: the launch's first row; `total` rows in the launch), through LDS.
// Consecutive lanes own consecutive points (t = proof * np + slot), so a wave's 64 points are 4608 contiguous bytes and its 64 canonical
// y are 2048.  Written lane by lane (72-byte stride) every store instruction touched 36 lines partially, and the L2 fetched each of
// them to merge the bytes: 0.2 GB of reads and 0.14 GB of writes for 26 MB of output (profiles/r02_pmc_fetch_write_steps20.csv, first
// collection).  Transposed in LDS, every store instruction writes 256 contiguous bytes.  EVERY lane of the workgroup must come here (five
// barriers); a lane past the end brings the shadow of the last point, which is not stored.  a.x leaves as beta x.
// The array asks for 10 KiB (4.5 are used): k_decompress's occupancy cap, see there.
#define K_DECOMPRESS_LDS_WORDS 2560
__device__ __forceinline__ void wave_rows_store(G1A& a, const uint32_t yraw[8], uint32_t total, G1A* __restrict__ pts, G1A* __restrict__ phi, uint8_t* ycanon) {
    __shared__ uint32_t out_lds[K_DECOMPRESS_LDS_WORDS];
    const uint32_t lane = threadIdx.x, t0 = blockIdx.x * blockDim.x, live = min(64u, total - t0);
    const uint32_t* av = reinterpret_cast<const uint32_t*>(&a);
#pragma unroll
    for (int i = 0; i < 18; ++i) out_lds[lane * 18 + i] = av[i];
    __syncthreads();
    uint32_t* dp = reinterpret_cast<uint32_t*>(pts + t0);
#pragma unroll
    for (int i = 0; i < 18; ++i) { const uint32_t k = i * 64 + lane; if (k < live * 18) dp[k] = out_lds[k]; }
    __syncthreads();
    // phi(P) = (beta x, y) beside every point: the MSM's second GLV half gathers it instead of multiplying per list entry (msm.hip: msm_entry_load)
    a.x = g1_beta_times(a.x);
#pragma unroll
    for (int i = 0; i < 9; ++i) out_lds[lane * 18 + i] = av[i];     // (y is still there)
    __syncthreads();
    dp = reinterpret_cast<uint32_t*>(phi + t0);
#pragma unroll
    for (int i = 0; i < 18; ++i) { const uint32_t k = i * 64 + lane; if (k < live * 18) dp[k] = out_lds[k]; }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) out_lds[lane * 8 + i] = yraw[i];
    __syncthreads();
    uint32_t* dy = reinterpret_cast<uint32_t*>(ycanon + (size_t)t0 * 32);
#pragma unroll
    for (int i = 0; i < 8; ++i) { const uint32_t k = i * 64 + lane; if (k < live * 8) dy[k] = out_lds[k]; }
}

// One lane per (proof, point): 32 B in, 72 + 72 + 32 B out.
// The kernel asks for 10 KiB of LDS (it uses 4.5): sixteen workgroups, four waves per SIMD, fill a CU's 160 KiB.  With the chained field
// products the kernel needs 76 registers instead of 120 and would fit six waves per SIMD; the dispatcher fills a CU before it moves on
// to the next, so a launch that does not fill the chip (the 20-step launch: 1920 waves for 1024 SIMDs) sat on fewer SIMDs and took
// 542 us instead of 487.  Held to four waves it takes 452 (profiles/field_chain_kernel_stats.txt); caps of three and two measured the same.
// gfx950 (-Rpass-analysis=kernel-resource-usage): 76 VGPRs, 62 SGPRs, no spills, 48 bytes of scratch, 10240 bytes of LDS; 4 waves per SIMD.
__global__ void __launch_bounds__(64, 4) k_decompress(const uint8_t* __restrict__ proofs, uint32_t proof_len, const uint32_t* __restrict__ point_offsets,
                                                   uint32_t np, uint32_t n_main_points, uint32_t n, G1A* __restrict__ pts, G1A* __restrict__ phi, uint8_t* __restrict__ ycanon,
                                                   int* __restrict__ status) {
    const uint32_t total = n * np;
    const uint32_t t = min(blockIdx.x * blockDim.x + threadIdx.x, total - 1);   // lanes past the end shadow the last point (wave_rows_store)
    const uint32_t p = t / np, slot = t % np;
    G1A a;
    uint32_t yraw[8];
    if (!point_decode(point_load(proofs, proof_len, point_offsets, p, slot), a, yraw)) point_refuse(status, p, slot, n_main_points, a, yraw);
    wave_rows_store(a, yraw, total, pts, phi, ycanon);
}

// k_decompress with a hint per point (include/h2v_hints.h).  The encoding fixes y completely — y^2 = x^3 + 3 and the parity of the
// canonical y is the sign flag — so the hint h is CHECKED, never trusted: it is used exactly when x < p, the identity flag is clear,
// h < p, (h & 1) == sign and h^2 == x^3 + 3, and then h IS the canonical y that point_from_root would have found (the two roots y and
// p - y differ in parity, p being odd).  That is two squarings, one product and a comparison instead of the ~320 products of the root.
// BN254's G1 has prime order, so no point of the curve has y = 0 (it would have order 2): the `nz` test of point_from_root is dead for
// every decodable point and the hinted path needs no special case for it — a zero hint fails h^2 == x^3 + 3 like any other wrong value.
//
// hints and ycanon may be the same memory (the batch keeps its hints where the canonical y will lie): a workgroup reads the 64 rows of
// its own lanes before it writes the same 64 rows, and no other workgroup touches them.  Hence no __restrict__ on the two.
//
// Misses are counted per wave: a ballot over the live lanes, and one atomic add by lane 0 only when the count is not zero.
//
// Then the WAVE decides, from the same ballot, so that one miss does not cost its wave a root.  If all its live lanes miss, each takes
// its root in place: what k_decompress computes for its point, statuses included; no lane waits for another, and a sender of nothing
// but bad hints keeps k_decompress's speed.  If it has a hit and a miss, the missing lanes store the placeholder a failed decode
// stores (point_none) WITHOUT a status, and append their point indices to the list: one returning atomic add per wave by lane 0, the
// lanes' places from their ranks in the ballot.  k_decompress_misses, enqueued right behind on the same stream, takes those roots
// densely, 64 listed points per wave whatever waves they came from.  The entries are indices into the whole stage (t_base = p0 x Np of
// the piece added), written to the piece's own segment of the list, which starts at t_base: a piece lists at most its own points, so
// the segments of pieces never overlap.  Every lane reaches wave_rows_store (the divergent part has no barrier).
//
// gfx950 (-Rpass-analysis=kernel-resource-usage): 102 VGPRs, 62 SGPRs, no spills, 48 bytes of scratch, 10240 bytes of LDS; 4 waves per SIMD.
// Launch bounds and LDS: k_decompress's, 64 threads held to four waves per SIMD by the 10 KiB of wave_rows_store — four waves is also
// all that 102 registers allow.  The root in place IS k_decompress's loop, which was measured fastest under that cap when the launch
// does not fill the chip (see its comment), and a sender of bad hints is promised that speed.  The hit path is too short for the cap to
// bind at the sizes measured: the 1920 waves of the headline launch are all resident at once under four waves per SIMD (4096 places).
// Whether the dispatcher's packing matters to an all-hit launch was not measured apart from that.
__global__ void __launch_bounds__(64, 4) k_decompress_hinted(const uint8_t* __restrict__ proofs, uint32_t proof_len, const uint32_t* __restrict__ point_offsets,
                                                          uint32_t np, uint32_t n_main_points, uint32_t n, G1A* __restrict__ pts, G1A* __restrict__ phi, const uint8_t* hints,
                                                          uint8_t* ycanon, int* __restrict__ status, uint32_t* __restrict__ misses,
                                                          uint32_t* __restrict__ list, uint32_t* __restrict__ list_count, uint32_t t_base) {
    const uint32_t total = n * np;
    const uint32_t t_raw = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t t = min(t_raw, total - 1);   // lanes past the end shadow the last point (wave_rows_store)
    const uint32_t p = t / np, slot = t % np;
    const PointIn in = point_load(proofs, proof_len, point_offsets, p, slot);
    const uint4* hsrc = reinterpret_cast<const uint4*>(hints + (size_t)t * 32);
    const uint4 hlo = hsrc[0], hhi = hsrc[1];
    uint32_t yraw[8] = {hlo.x, hlo.y, hlo.z, hlo.w, hhi.x, hhi.y, hhi.z, hhi.w};   // the hint; on a hit, the canonical y as it is
    G1A a;
    const bool ok = !Fq::geq_p(in.w) && !in.is_inf;   // (point_decode's first two refusals)
    bool hit = false;
    Fq x = Fq::zero(), rhs = Fq::zero();
    if (ok) {
        x = Fq::from_raw(in.w);
        rhs = curve_rhs(x);
        if (!Fq::geq_p(yraw) && (bool)(yraw[0] & 1u) == in.sign) {
            const Fq h = Fq::from_raw(yraw);
            if (h.sqr() == rhs) { hit = true; a.x = x; a.y = h; }
        }
    }
    const unsigned long long missed = __ballot(!hit && t_raw < total);
    if (missed && threadIdx.x == 0) atomicAdd(misses, (uint32_t)__popcll(missed));
    const bool in_place = missed == __ballot(t_raw < total);   // (uniform over the wave)
    if (missed && !in_place) {
        uint32_t at = 0;
        if (threadIdx.x == 0) at = atomicAdd(list_count, (uint32_t)__popcll(missed));   // (lane 0 is live in every workgroup)
        at = __shfl(at, 0);
        if (!hit && t_raw < total) list[at + (uint32_t)__popcll(missed & ((1ull << threadIdx.x) - 1))] = t_base + t;
    }
    if (!hit && !in_place) point_none(a, yraw);   // the placeholder; k_decompress_misses writes the point and its status
    if (!hit && in_place && !(ok && point_from_root(x, rhs, in.sign, a, yraw))) point_refuse(status, p, slot, n_main_points, a, yraw);
    wave_rows_store(a, yraw, total, pts, phi, ycanon);
}

// The roots that the mixed waves of k_decompress_hinted left out, densely: lane i below *list_count takes point t = list[i] of the
// stage (an index over all its proofs: the pointers are the stage's own, not a piece's) from the proof bytes on, and writes that
// point's pts, phi and ycanon rows and, where it does not decode, its proof's status.  The grid is fixed from the piece's size on the
// host, which never reads the count: a workgroup past the count leaves at once.  The listed points are scattered, so the rows are
// stored lane by lane (72 and 32 bytes each, as 8- and 16-byte stores) and not through LDS; rows that are not listed are not touched,
// so hints and ycanon may still be the same memory.  Launched with k_decompress's 10 KiB of LDS (dynamic: none is used), which holds it
// to the four waves per SIMD that k_decompress's root loop was measured fastest at.
// gfx950 (-Rpass-analysis=kernel-resource-usage): 76 VGPRs, 39 SGPRs, no spills, 48 bytes of scratch, no static LDS; 6 waves per SIMD by its
// registers, 4 under the launch's LDS request.
__global__ void __launch_bounds__(64, 4) k_decompress_misses(const uint8_t* __restrict__ proofs, uint32_t proof_len, const uint32_t* __restrict__ point_offsets,
                                                          uint32_t np, uint32_t n_main_points, G1A* __restrict__ pts, G1A* __restrict__ phi, uint8_t* __restrict__ ycanon,
                                                          int* __restrict__ status, const uint32_t* __restrict__ list, const uint32_t* __restrict__ list_count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *list_count) return;
    const uint32_t t = list[i];
    const uint32_t p = t / np, slot = t % np;
    G1A a;
    uint32_t yraw[8];
    if (!point_decode(point_load(proofs, proof_len, point_offsets, p, slot), a, yraw)) point_refuse(status, p, slot, n_main_points, a, yraw);
    const uint2* av = reinterpret_cast<const uint2*>(&a);   // (a G1A: 18 words, 8-byte aligned)
    uint2* dp = reinterpret_cast<uint2*>(pts + t);
#pragma unroll
    for (int k = 0; k < 9; ++k) dp[k] = av[k];
    a.x = g1_beta_times(a.x);   // phi(P) = (beta x, y)
    dp = reinterpret_cast<uint2*>(phi + t);
#pragma unroll
    for (int k = 0; k < 9; ++k) dp[k] = av[k];
    uint4* dy = reinterpret_cast<uint4*>(ycanon + (size_t)t * 32);
    dy[0] = make_uint4(yraw[0], yraw[1], yraw[2], yraw[3]);
    dy[1] = make_uint4(yraw[4], yraw[5], yraw[6], yraw[7]);
}

__global__ void __launch_bounds__(256) k_check_scalars(const uint8_t* __restrict__ proofs, uint32_t proof_len, const uint32_t* __restrict__ scalar_offsets,
                                                       uint32_t ns, const uint8_t* __restrict__ inst, uint32_t ninst, uint32_t n, int* __restrict__ status) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t per = ns + ninst;
    if (t >= n * per) return;
    uint32_t p = t / per, i = t % per;
    const uint8_t* b = i < ns ? proofs + (size_t)p * proof_len + scalar_offsets[i] : inst + ((size_t)p * ninst + (i - ns)) * 32;
    // The top word decides for all but 2^-32 of the values: below r's top word the scalar is canonical whatever the rest holds.  One
    // aligned word per lane instead of 32 byte loads: the kernel was 283 us of byte loads per 20-step launch, and it now sits on the
    // launch's own stream in front of the decompression instead of on a second stream beside it.
    const uint32_t top = ((uintptr_t)b & 3u) == 0 ? *reinterpret_cast<const uint32_t*>(b + 28)
                                                  : (uint32_t)b[28] | ((uint32_t)b[29] << 8) | ((uint32_t)b[30] << 16) | ((uint32_t)b[31] << 24);
    if (top < FrParams::P(7)) return;
    uint32_t raw[8];
    for (int j = 0; j < 8; ++j) raw[j] = (uint32_t)b[4 * j] | ((uint32_t)b[4 * j + 1] << 8) | ((uint32_t)b[4 * j + 2] << 16) | ((uint32_t)b[4 * j + 3] << 24);
    // a non-canonical public input cannot be represented as an Fr on the reference side at all: bad argument for that proof
    if (Fr::geq_p(raw)) status_set(status, p, i < ns ? H2V_DEV_ST_TRANSCRIPT : H2V_DEV_ST_INVALID_INSTANCES);
}

// One 8-byte word of the absorbed stream per thread, PROOF-MAJOR: words[proof][word].  Consecutive lanes build consecutive words
// of one proof, so their source bytes are (mostly) consecutive bytes of that proof and the stores are contiguous; the hash kernels
// then read a proof's 128-byte block as one line.  Round 1 had lanes = proofs: every byte load of a wave touched 64 different
// lines (0.13 ms per 20-step launch for 37 MB of stream).
#define STREAM_PROOFS_PER_BLOCK 8u   // a workgroup per proof was launch-rate bound: 20 480 workgroups of ~1 us of work each took 0.15 ms
__global__ void __launch_bounds__(256) k_stream_build(const TranscriptSrc* __restrict__ stream, uint32_t stream_len, const uint8_t* __restrict__ proofs,
                                                      uint32_t proof_len, const uint8_t* __restrict__ ycanon, uint32_t np, const uint8_t* __restrict__ inst,
                                                      uint32_t ninst, uint32_t n, uint32_t stream_words, unsigned long long* __restrict__ words) {
    const uint32_t p0 = blockIdx.x * STREAM_PROOFS_PER_BLOCK, p1 = min(n, p0 + STREAM_PROOFS_PER_BLOCK);
    for (uint32_t w = threadIdx.x; w < stream_words; w += blockDim.x) {
        // the word's eight table entries are the same for every proof: read once, used for the block's proofs
        uint32_t kind[8], value[8], off[8];
#pragma unroll
        for (uint32_t b = 0; b < 8; ++b) {
            const uint32_t pos = w * 8 + b, q = pos < stream_len ? pos : stream_len - 1;
            const TranscriptSrc sd = stream[q];
            kind[b] = pos < stream_len ? sd.kind : (uint32_t)TranscriptSrc::CONST;
            value[b] = pos < stream_len ? sd.value : 0u;
            off[b] = kind[b] == TranscriptSrc::CONST ? 0u : sd.offset;
        }
        // A word is [tail of item A][constant bytes (prefixes, markers)][head of item B] with either part possibly empty; items are 32
        // bytes (a point's x or y, a scalar, a public input) at odd addresses (every item is preceded by a one-byte prefix).  Each part
        // is ONE unaligned 8-byte load per proof — the eight bytes that END with A's last byte, shifted down; the eight that START with
        // B's first byte, shifted up: both stay inside their 32-byte items — instead of eight byte loads per word (58 -> 38 us per
        // 20-step launch).  A flag byte inside the word is masked afterwards.  A word of any other shape takes the byte path below.
        auto is_data = [](uint32_t k) { return k != TranscriptSrc::CONST; };
        auto src_of = [](uint32_t k) { return k == TranscriptSrc::PROOF_MASKED ? (uint32_t)TranscriptSrc::PROOF : k; };
        uint32_t la = 0;                                    // bytes of run A: positions [0, la)
        while (la < 8 && is_data(kind[la]) && src_of(kind[la]) == src_of(kind[0]) && off[la] == off[0] + la) ++la;
        uint32_t sb = la;                                   // run B: positions [sb, 8)
        unsigned long long cbytes = 0;
        while (sb < 8 && !is_data(kind[sb])) { cbytes |= (unsigned long long)value[sb] << (8 * sb); ++sb; }
        bool fits = true;
        for (uint32_t b2 = sb; b2 < 8; ++b2) fits = fits && is_data(kind[b2]) && src_of(kind[b2]) == src_of(kind[sb]) && off[b2] == off[sb] + (b2 - sb);
        // (A shorter than the word is the TAIL of its item — what follows it is a constant or another source — so the bytes in front of
        // it, which the shifted load also reads, belong to the same item; B is the HEAD of its item for the same reason.  Items are 32 bytes.)
        if (la > 0 && la < 8 && off[0] < 8 - la) fits = false;
        uint32_t mask_byte = 8;
#pragma unroll
        for (uint32_t b2 = 0; b2 < 8; ++b2) if (kind[b2] == TranscriptSrc::PROOF_MASKED) mask_byte = b2;
        if (fits) {
            typedef unsigned long long u64_unaligned __attribute__((aligned(1)));
            const unsigned long long keep = mask_byte < 8 ? ~(0xc0ULL << (8 * mask_byte)) : ~0ULL;
            auto base_of = [&](uint32_t k) -> const uint8_t* { return k == TranscriptSrc::YCOORD ? ycanon : (k == TranscriptSrc::INSTANCE ? inst : proofs); };
            auto per_of = [&](uint32_t k) -> size_t { return k == TranscriptSrc::YCOORD ? (size_t)np * 32 : (k == TranscriptSrc::INSTANCE ? (size_t)ninst * 32 : (size_t)proof_len); };
            const uint8_t* const baseA = la ? base_of(kind[0]) : proofs;
            const size_t perA = la ? per_of(kind[0]) : 0, offA = la ? (size_t)off[0] + la - 8 : 0;       // the load ends with A's last byte
            const uint8_t* const baseB = sb < 8 ? base_of(kind[sb]) : proofs;
            const size_t perB = sb < 8 ? per_of(kind[sb]) : 0, offB = sb < 8 ? off[sb] : 0;                 // the load starts with B's first byte
            for (uint32_t p = p0; p < p1; ++p) {
                unsigned long long v = cbytes;
                if (la) v |= *reinterpret_cast<const u64_unaligned*>(baseA + (size_t)p * perA + offA) >> (8 * (8 - la));
                if (sb < 8) v |= *reinterpret_cast<const u64_unaligned*>(baseB + (size_t)p * perB + offB) << (8 * sb);
                words[(size_t)p * stream_words + w] = v & keep;
            }
            continue;
        }
        for (uint32_t p = p0; p < p1; ++p) {
            const uint8_t* const pb = proofs + (size_t)p * proof_len;
            const uint8_t* const yb = ycanon + (size_t)p * np * 32;
            const uint8_t* const ib = inst + (size_t)p * ninst * 32;
            // eight source addresses (selects, no branches: the kinds differ from lane to lane), eight byte loads back to back,
            // constants and the flag mask merged afterwards
            uint32_t raw[8];
#pragma unroll
            for (uint32_t b = 0; b < 8; ++b) {
                const uint8_t* base = kind[b] == TranscriptSrc::YCOORD ? yb : (kind[b] == TranscriptSrc::INSTANCE ? ib : pb);
                raw[b] = base[off[b]];
            }
            unsigned long long v = 0;
#pragma unroll
            for (uint32_t b = 0; b < 8; ++b) {
                uint32_t byte = raw[b];
                if (kind[b] == TranscriptSrc::CONST) byte = value[b];
                else if (kind[b] == TranscriptSrc::PROOF_MASKED) byte &= 0x3f;
                v |= (unsigned long long)byte << (8 * b);
            }
            words[(size_t)p * stream_words + w] = v;
        }
    }
}

// ------------------------------------------------------------------ BLAKE2b (RFC 7693)
// a 64-bit rotation by a constant is two v_alignbit_b32 (the shift / shift / or form the compiler makes of the C expression is four instructions)
__device__ __forceinline__ unsigned long long rotr64(unsigned long long x, int c) {
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    if (c == 32) return ((unsigned long long)lo << 32) | hi;
    const uint32_t a = c < 32 ? hi : lo, b = c < 32 ? lo : hi;      // rotating by c >= 32 = swapping the halves, then by c - 32
    const uint32_t k = (uint32_t)(c & 31);
    const uint32_t nl = __builtin_amdgcn_alignbit(a, b, k), nh = __builtin_amdgcn_alignbit(b, a, k);
    return ((unsigned long long)nh << 32) | nl;
}
__constant__ unsigned long long BLAKE_IV[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                                               0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
__constant__ uint8_t BLAKE_SIGMA[12][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};

// ---- BLAKE2b across a quad of lanes.  The compression function works on a 4 x 4 matrix of 64-bit words: a column step (four
// independent G functions) and a diagonal step (four more).  Lane r of a quad holds column r (v[r], v[4+r], v[8+r], v[12+r]);
// the diagonal step is the column step after rotating rows 1..3 by 1..3 lanes (DPP quad permutes, no LDS).  One proof per quad:
// the ~21 dependent compressions of a proof's transcript take a quarter of the instructions per lane — the transcript is a
// latency chain (16 waves per 1024 proofs), so that is a quarter of its time.
__device__ __forceinline__ unsigned long long quad_rot64(unsigned long long x, const int ctrl_sel) {
    uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    // ctrl_sel: 1 -> lane r reads lane (r + 1) & 3, 2 -> (r + 2) & 3, 3 -> (r + 3) & 3
    if (ctrl_sel == 1) { lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)lo, 0x39, 0xf, 0xf, true); hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)hi, 0x39, 0xf, 0xf, true); }
    else if (ctrl_sel == 2) { lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)lo, 0x4e, 0xf, 0xf, true); hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)hi, 0x4e, 0xf, 0xf, true); }
    else { lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)lo, 0x93, 0xf, 0xf, true); hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)hi, 0x93, 0xf, 0xf, true); }
    return ((unsigned long long)hi << 32) | lo;
}
#define H2V_G4(a, b, c, d, x, y)                     \
    a = a + b + (x); d = rotr64(d ^ a, 32);          \
    c = c + d;       b = rotr64(b ^ c, 24);          \
    a = a + b + (y); d = rotr64(d ^ a, 16);          \
    c = c + d;       b = rotr64(b ^ c, 63);
// h0 = h[r], h1 = h[4 + r]; msg = this proof's 16 message words in LDS; sig[rd] packs the lane's four message indices of round rd
__device__ __forceinline__ void blake2b_compress_quad(unsigned long long& h0, unsigned long long& h1, const unsigned long long* msg, const uint32_t* sig,
                                                       unsigned long long t, bool last, uint32_t r) {
    unsigned long long a = h0, b = h1, c = BLAKE_IV[r], d = BLAKE_IV[4 + r];
    if (r == 0) d ^= t;           // v12 ^= t0 (t1 = 0: streams are far below 2^64 bytes)
    if (last && r == 2) d = ~d;   // v14
#pragma unroll
    for (int rd = 0; rd < 12; ++rd) {
        const uint32_t s4 = sig[rd];
        H2V_G4(a, b, c, d, msg[s4 & 15u], msg[(s4 >> 4) & 15u]);
        b = quad_rot64(b, 1); c = quad_rot64(c, 2); d = quad_rot64(d, 3);
        H2V_G4(a, b, c, d, msg[(s4 >> 8) & 15u], msg[(s4 >> 12) & 15u]);
        b = quad_rot64(b, 3); c = quad_rot64(c, 2); d = quad_rot64(d, 1);
    }
    h0 ^= a ^ c; h1 ^= b ^ d;
}
#undef H2V_G4

#define TR4_MSG_STRIDE 17   // 16 message words + 1: the sixteen proofs of a wave hit sixteen different LDS banks
// squeeze_at[q] = absorbed length at which challenge q is produced: digest(stream[0..L)) with the state
// cloned (transcript/mod.rs:209-214), 64 bytes -> Fr::from_uniform_bytes (:500-514).  16 proofs per wave.
__global__ void __launch_bounds__(64) k_transcript(const unsigned long long* __restrict__ words_all, uint32_t stream_words, const uint32_t* __restrict__ squeeze_at, uint32_t n_squeeze,
                                                   uint32_t n, Fr* __restrict__ chal) {
    extern __shared__ unsigned long long tr_lds[];   // [16][TR4_MSG_STRIDE] message block, then [16][n_squeeze][8] digests
    const uint32_t tid = threadIdx.x, r = tid & 3u, pq = tid >> 2;
    const uint32_t p_raw = blockIdx.x * 16 + pq, p = p_raw < n ? p_raw : n - 1;   // lanes beyond n shadow the last proof (uniform control flow)
    const unsigned long long* words = words_all + (size_t)p * stream_words;   // this proof's stream
    unsigned long long* msg = tr_lds + pq * TR4_MSG_STRIDE;
    unsigned long long* dig = tr_lds + 16 * TR4_MSG_STRIDE + (size_t)pq * n_squeeze * 8;
    uint32_t sig[12];
#pragma unroll
    for (int rd = 0; rd < 12; ++rd)
        sig[rd] = (uint32_t)BLAKE_SIGMA[rd][2 * r] | ((uint32_t)BLAKE_SIGMA[rd][2 * r + 1] << 4) | ((uint32_t)BLAKE_SIGMA[rd][8 + 2 * r] << 8) | ((uint32_t)BLAKE_SIGMA[rd][9 + 2 * r] << 12);
    // parameter block: digest 64, no key, fanout = depth = 1, personal "Halo2-Transcript" (transcript/mod.rs:126-129)
    const unsigned long long pers0 = 0x72542d326f6c6148ULL, pers1 = 0x7470697263736e61ULL;  // "Halo2-Tr" "anscript" little endian
    unsigned long long h0 = BLAKE_IV[r] ^ (r == 0 ? 0x01010040ULL : 0ULL), h1 = BLAKE_IV[4 + r] ^ (r == 2 ? pers0 : (r == 3 ? pers1 : 0ULL));
    uint32_t blk = 0;
    // the lane's four words of the block that is needed next, fetched while the block before it is compressed (a load per block on the
    // critical path was ~1 us of every one of the ~18 compressions of a proof)
    const uint32_t n_blocks = stream_words / 16;
    unsigned long long pf[4];
    uint32_t pf_blk = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) pf[j] = words[4 * r + j];
    for (uint32_t q = 0; q < n_squeeze; ++q) {
        const uint32_t len = squeeze_at[q];  // >= 1
        const uint32_t last_blk = (len - 1) / 128;
        for (; blk < last_blk; ++blk) {
            __syncthreads();
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) msg[4 * r + j] = pf_blk == blk ? pf[j] : words[(size_t)blk * 16 + 4 * r + j];
            pf_blk = blk + 1 < n_blocks ? blk + 1 : blk;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) pf[j] = words[(size_t)pf_blk * 16 + 4 * r + j];
            __syncthreads();
            blake2b_compress_quad(h0, h1, msg, sig, (unsigned long long)(blk + 1) * 128, false, r);
        }
        const uint32_t rem = len - last_blk * 128;  // 1..128 bytes of the final block
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            unsigned long long w = pf_blk == last_blk ? pf[j] : words[(size_t)last_blk * 16 + 4 * r + j];   // (stays prefetched: the stream goes on inside this block)
            const uint32_t lo = 8 * (4 * r + j);
            if (lo >= rem) w = 0;
            else if (lo + 8 > rem) w &= (1ULL << (8 * (rem - lo))) - 1;
            msg[4 * r + j] = w;
        }
        __syncthreads();
        unsigned long long c0 = h0, c1 = h1;   // the clone
        blake2b_compress_quad(c0, c1, msg, sig, len, true, r);
        dig[q * 8 + r] = c0; dig[q * 8 + 4 + r] = c1;
    }
    __syncthreads();
    // 64 digest bytes -> Fr; the quad's lanes share the challenges
    for (uint32_t q = r; q < n_squeeze; q += 4) {
        uint32_t w32[16];
#pragma unroll
        for (int i = 0; i < 8; ++i) { const unsigned long long v = dig[q * 8 + i]; w32[2 * i] = (uint32_t)v; w32[2 * i + 1] = (uint32_t)(v >> 32); }
        const Fr c = Fr::from_uniform_words(w32);
        if (p_raw < n) chal[(size_t)q * n + p] = c;
    }
}

// The draws of a seed (include/h2v_draws.h):  draw(seed, i) = LE512(BLAKE2b-512(seed[32] | LE64(i), personal "h2v-draws-v1")) mod r,
// as 32 canonical little-endian bytes at out[2 i], out[2 i + 1].  One draw per quad of lanes, 16 per wave, one compression each: the
// 40-byte message is a single final block.  The seed arrives as four kernel arguments (no buffer, no copy); i = first + the draw's
// number, a 64-bit sum (first + n does not wrap: the entry points refuse it).
__global__ void __launch_bounds__(64) k_expand_draws(unsigned long long seed0, unsigned long long seed1, unsigned long long seed2, unsigned long long seed3,
                                                     unsigned long long first, unsigned long long n, uint4* __restrict__ out) {
    __shared__ unsigned long long ex_lds[16 * TR4_MSG_STRIDE];   // [16][TR4_MSG_STRIDE] message block; its first 8 words take the digest afterwards
    const uint32_t tid = threadIdx.x, r = tid & 3u, pq = tid >> 2;
    const unsigned long long d_raw = (unsigned long long)blockIdx.x * 16 + pq, d = d_raw < n ? d_raw : n - 1;   // lanes beyond n shadow the last draw (uniform control flow)
    unsigned long long* msg = ex_lds + pq * TR4_MSG_STRIDE;
    uint32_t sig[12];
#pragma unroll
    for (int rd = 0; rd < 12; ++rd)
        sig[rd] = (uint32_t)BLAKE_SIGMA[rd][2 * r] | ((uint32_t)BLAKE_SIGMA[rd][2 * r + 1] << 4) | ((uint32_t)BLAKE_SIGMA[rd][8 + 2 * r] << 8) | ((uint32_t)BLAKE_SIGMA[rd][9 + 2 * r] << 12);
    // parameter block: digest 64, no key, fanout = depth = 1, personal "h2v-draws-v1" and four zero bytes
    const unsigned long long pers0 = 0x776172642d763268ULL, pers1 = 0x0000000031762d73ULL;  // "h2v-draw" "s-v1\0\0\0\0" little endian
    unsigned long long h0 = BLAKE_IV[r] ^ (r == 0 ? 0x01010040ULL : 0ULL), h1 = BLAKE_IV[4 + r] ^ (r == 2 ? pers0 : (r == 3 ? pers1 : 0ULL));
    // lane r writes message words 4 r .. 4 r + 3: the seed, the index, zeros
    msg[4 * r + 0] = r == 0 ? seed0 : (r == 1 ? first + d : 0ULL);
    msg[4 * r + 1] = r == 0 ? seed1 : 0ULL;
    msg[4 * r + 2] = r == 0 ? seed2 : 0ULL;
    msg[4 * r + 3] = r == 0 ? seed3 : 0ULL;
    __syncthreads();
    blake2b_compress_quad(h0, h1, msg, sig, 40, true, r);
    __syncthreads();   // (every lane of the quad has read its message words)
    msg[r] = h0; msg[4 + r] = h1;
    __syncthreads();
    // 64 digest bytes -> Fr -> canonical words: the quad's lanes all hold the draw, lanes 0 and 1 store its two halves
    uint32_t w32[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) { const unsigned long long v = msg[i]; w32[2 * i] = (uint32_t)v; w32[2 * i + 1] = (uint32_t)(v >> 32); }
    uint32_t raw[8];
    Fr::from_uniform_words(w32).to_raw(raw);
    if (d_raw < n && r < 2) out[2 * d + r] = r == 0 ? make_uint4(raw[0], raw[1], raw[2], raw[3]) : make_uint4(raw[4], raw[5], raw[6], raw[7]);
}

// ------------------------------------------------------------------ legacy Keccak-256 transcript (transcript/mod.rs:234-272)
__device__ __forceinline__ unsigned long long rotl64(unsigned long long x, int c) { return c ? (x << c) | (x >> (64 - c)) : x; }
__constant__ unsigned long long KECCAK_RC[24] = {
    0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL, 0x000000000000808bULL, 0x0000000080000001ULL,
    0x8000000080008081ULL, 0x8000000000008009ULL, 0x000000000000008aULL, 0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000aULL,
    0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL, 0x8000000000008003ULL, 0x8000000000008002ULL, 0x8000000000000080ULL,
    0x000000000000800aULL, 0x800000008000000aULL, 0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
__device__ __noinline__ void keccak_f1600(unsigned long long a[25]) {
    const int ROT[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
    for (int r = 0; r < 24; ++r) {
        unsigned long long c[5], b[25];
#pragma unroll
        for (int x = 0; x < 5; ++x) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
        for (int x = 0; x < 5; ++x) {
            unsigned long long d = c[(x + 4) % 5] ^ rotl64(c[(x + 1) % 5], 1);
#pragma unroll
            for (int y = 0; y < 5; ++y) a[x + 5 * y] ^= d;
        }
#pragma unroll
        for (int x = 0; x < 5; ++x)
#pragma unroll
            for (int y = 0; y < 5; ++y) b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl64(a[x + 5 * y], ROT[x + 5 * y]);
#pragma unroll
        for (int x = 0; x < 5; ++x)
#pragma unroll
            for (int y = 0; y < 5; ++y) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
        a[0] ^= KECCAK_RC[r];
    }
}
// digest of  stream[0..len) | suffix  given the running state `st` that has absorbed the first `blk` full 136-byte blocks
__device__ __forceinline__ void keccak_tail(const unsigned long long st[25], const unsigned long long* __restrict__ words, uint32_t stream_words, uint32_t p, uint32_t blk,
                                            uint32_t len, uint32_t suffix, unsigned long long out[4]) {
    unsigned long long a[25];
    for (int i = 0; i < 25; ++i) a[i] = st[i];
    uint32_t rem = len - blk * 136;  // 0..135 bytes of the stream remain, then the suffix byte, then the padding
    for (int j = 0; j < 17; ++j) {
        unsigned long long w = 0;
        uint32_t lo = 8 * j;
        if (lo < rem) {
            w = words[(size_t)p * stream_words + (size_t)blk * 17 + j];
            if (lo + 8 > rem) w &= (1ULL << (8 * (rem - lo))) - 1;
        }
        if (rem >= lo && rem < lo + 8) w |= (unsigned long long)suffix << (8 * (rem - lo));
        a[j] ^= w;
    }
    uint32_t pad_at = rem + 1;  // first padding byte
    if (pad_at == 136) {        // the suffix filled the block: the padding gets a block of its own
        keccak_f1600(a);
        a[0] ^= 0x01ULL; a[16] ^= 0x8000000000000000ULL;
    } else {
        a[pad_at / 8] ^= 0x01ULL << (8 * (pad_at % 8));
        a[16] ^= 0x8000000000000000ULL;
    }
    keccak_f1600(a);
    for (int i = 0; i < 4; ++i) out[i] = a[i];
}
// stream words are laid out in 136-byte blocks here: word (blk * 17 + j)
__global__ void __launch_bounds__(64) k_transcript_keccak(const unsigned long long* __restrict__ words, uint32_t stream_words, const uint32_t* __restrict__ squeeze_at, uint32_t n_squeeze,
                                                          uint32_t n, Fr* __restrict__ chal) {
    uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    unsigned long long st[25];
    for (int i = 0; i < 25; ++i) st[i] = 0;
    uint32_t blk = 0;
    for (uint32_t q = 0; q < n_squeeze; ++q) {
        uint32_t len = squeeze_at[q];
        uint32_t full = len / 136;
        for (; blk < full; ++blk) {
            for (int j = 0; j < 17; ++j) st[j] ^= words[(size_t)p * stream_words + (size_t)blk * 17 + j];
            keccak_f1600(st);
        }
        unsigned long long lo[4], hi[4];
        keccak_tail(st, words, stream_words, p, blk, len, 10, lo);   // KECCAK256_PREFIX_CHALLENGE_LO
        keccak_tail(st, words, stream_words, p, blk, len, 11, hi);   // KECCAK256_PREFIX_CHALLENGE_HI
        uint32_t w32[16];
        for (int i = 0; i < 4; ++i) { w32[2 * i] = (uint32_t)lo[i]; w32[2 * i + 1] = (uint32_t)(lo[i] >> 32); w32[8 + 2 * i] = (uint32_t)hi[i]; w32[8 + 2 * i + 1] = (uint32_t)(hi[i] >> 32); }
        chal[(size_t)q * n + p] = Fr::from_uniform_words(w32);
    }
}

// The batch multipliers: mult[p] = the product of the draws BEHIND proof p's own inside p's group (kzg/strategy.rs:129, msm.rs:173-176),
// for the groups of a GroupShape, equal or not, as ONE segmented suffix scan over the whole draw array in tiles of MULT_TILE draws —
// work proportional to the draws whatever the groups' sizes.  A group is the segment of its draws: it ends at the draw whose byte in
// last[] is not zero (unequal groups: one draw per proof) or, by arithmetic, at the nt-th draw of an equal group, whose draws past its
// gs proofs (a shard's tail) count in the products and have no multiplier of their own.  The scan carries a pair (v, closed) per span
// [i, k] of draws: v = the product of the draws from i to the end of i's group or k, whichever comes first; closed = i's group ends
// inside the span.  (a, b) of two adjacent spans combine to a if a is closed, else (a.v b.v, b.closed).
//   k_seg_mult_tiles       a workgroup per tile: mult[j] <- the later draws of j's group inside the tile; the tile's pair;
//                          open_from[tile] <- the first thread whose group goes on behind the tile (the closed spans are a prefix of the tile)
//   k_seg_mult_scan_tiles  one workgroup: tile_prod[tile] <- what the later tiles give a group that is still open at the tile's end
//   k_seg_mult_apply       mult[j] <- mult[j] * tile_prod[j's tile] for the threads from open_from[tile] on
// (One 1024-thread workgroup per group walked its draws in 1024 serial chunks: 210 us for a 20-step launch.  The multipliers depend on
// the uploaded draws alone, so they are computed once per upload, not per launch: upload_impl.)
#define MULT_TILE 256u
// part[t] <- prod_{t' >= t} part[t'] over the workgroup's T values (T a power of two); every thread calls it (k_leg_weights)
template <uint32_t T> __device__ __forceinline__ void fr_suffix_scan(Fr* part, uint32_t t) {
    __syncthreads();
    for (uint32_t d = 1; d < T; d <<= 1) {
        const Fr v = t + d < T ? part[t + d] : Fr::one();
        __syncthreads();
        part[t] = part[t] * v;
        __syncthreads();
    }
}
// part[t] <- the pair of the span [t, T); every thread calls it (fr_suffix_scan's barriers)
template <uint32_t T> __device__ __forceinline__ void fr_seg_suffix_scan(Fr* part, uint32_t* closed, uint32_t t) {
    __syncthreads();
    for (uint32_t d = 1; d < T; d <<= 1) {
        const bool has = t + d < T;
        const Fr v = has ? part[t + d] : Fr::one();
        const uint32_t c = has ? closed[t + d] : 0u;
        __syncthreads();
        if (!closed[t]) { part[t] = part[t] * v; closed[t] = c; }   // (closed[t] is read and written by thread t alone in this phase)
        __syncthreads();
    }
}
// draw j of the array: where its proof keeps its multiplier (NO_MULT: a draw without a proof), and whether it is the last of its group
#define NO_MULT 0xffffffffu
struct SegDraw { uint32_t slot; bool end; };
__device__ __forceinline__ SegDraw seg_draw(const GroupShape& shape, const uint8_t* __restrict__ last, uint32_t j) {
    if (shape.off) return SegDraw{j, last[j] != 0};
    const GroupShape::Draw d = shape.draw_at(j);
    return SegDraw{d.j < shape.gs ? shape.first(d.g) + d.j : NO_MULT, d.j + 1 == shape.nt};
}
__global__ void __launch_bounds__(MULT_TILE) k_seg_mult_tiles(const uint8_t* __restrict__ tail, const uint8_t* __restrict__ last, GroupShape shape, uint32_t n_draws,
                                                              Fr* __restrict__ mult, Fr* __restrict__ tile_prod, uint32_t* __restrict__ tile_closed, uint32_t* __restrict__ open_from) {
    __shared__ Fr part[MULT_TILE];
    __shared__ uint32_t closed[MULT_TILE];
    const uint32_t t = threadIdx.x, j = blockIdx.x * MULT_TILE + t;
    Fr r = Fr::one();
    SegDraw d{NO_MULT, true};   // (past the draws: one-element groups of their own, behind the last group's end)
    if (j < n_draws) { Fr::from_bytes(tail + 32 * (size_t)j, r); d = seg_draw(shape, last, j); }
    part[t] = r; closed[t] = d.end ? 1u : 0u;
    fr_seg_suffix_scan<MULT_TILE>(part, closed, t);
    if (d.slot != NO_MULT) mult[d.slot] = (d.end || t + 1 == MULT_TILE) ? Fr::one() : part[t + 1];
    if (!closed[t] && (t == 0 || closed[t - 1])) open_from[blockIdx.x] = t;
    if (t + 1 == MULT_TILE && closed[t]) open_from[blockIdx.x] = MULT_TILE;
    if (t == 0) { tile_prod[blockIdx.x] = part[0]; tile_closed[blockIdx.x] = closed[0]; }
}
__global__ void __launch_bounds__(1024) k_seg_mult_scan_tiles(Fr* __restrict__ tile_prod, const uint32_t* __restrict__ tile_closed, uint32_t tiles) {
    __shared__ Fr part[1024];
    __shared__ uint32_t closed[1024];
    const uint32_t t = threadIdx.x;
    Fr carry = Fr::one();   // the value of all tiles behind the chunk (behind the last tile: nothing, no group goes on there; its closed bit is never needed: the last draw closes the last group)
    for (uint32_t hi = tiles; hi > 0; hi = hi > 1024 ? hi - 1024 : 0) {
        const uint32_t lo = hi > 1024 ? hi - 1024 : 0, i = lo + t;
        part[t] = i < hi ? tile_prod[i] : Fr::one();
        closed[t] = i < hi ? tile_closed[i] : 0u;   // (the combination's identity)
        fr_seg_suffix_scan<1024>(part, closed, t);
        // the later tiles of the chunk, then the carry
        Fr later = carry;
        if (t + 1 < 1024) later = closed[t + 1] ? part[t + 1] : part[t + 1] * carry;
        const Fr all = closed[0] ? part[0] : part[0] * carry;
        __syncthreads();   // (part is written again in the next round)
        if (i < hi) tile_prod[i] = later;
        carry = all;
    }
}
__global__ void __launch_bounds__(MULT_TILE) k_seg_mult_apply(Fr* __restrict__ mult, const uint8_t* __restrict__ last, GroupShape shape, uint32_t n_draws,
                                                              const Fr* __restrict__ tile_prod, const uint32_t* __restrict__ open_from) {
    const uint32_t j = blockIdx.x * MULT_TILE + threadIdx.x;
    if (j >= n_draws || threadIdx.x < open_from[blockIdx.x]) return;
    const uint32_t slot = seg_draw(shape, last, j).slot;
    if (slot != NO_MULT) mult[slot] = mult[slot] * tile_prod[blockIdx.x];
}

// The weights of a finished batch's groups fed to a resident accumulator as G legs (h2v_accumulator_process_batch, accumulator.hip).
// Group g's M_g, the product of its draws, is its first draw times the multiplier of its first proof (the product of the later draws
// of the group, what the upload left in mult); first_g = GroupShape::first(g).  One workgroup of LEG_WEIGHTS_MAX
// threads, thread g its group (the threads past G hold 1), one suffix scan in LDS (18 KB), then as canonical 8-word scalars
//   weights[0] = prod_g M_g,  weights[1 + g] = W_g = prod_{f > g} M_f   (the items of the k_accumulator_scale launch that follows)
//   legs[g] = M_g                                                       (for the host's journal)
#define LEG_WEIGHTS_MAX 512u
__device__ __forceinline__ void fr_store_canonical(uint32_t* out, const Fr& v) {
    uint32_t raw[8];
    v.to_raw(raw);
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = raw[j];
}
__global__ void __launch_bounds__(LEG_WEIGHTS_MAX) k_leg_weights(const uint8_t* __restrict__ tail, const Fr* __restrict__ mult, GroupShape shape,
                                                                 uint32_t* __restrict__ weights, uint32_t* __restrict__ legs) {
    __shared__ Fr part[LEG_WEIGHTS_MAX];
    const uint32_t t = threadIdx.x, G = shape.G;
    Fr m = Fr::one();
    if (t < G) {
        const size_t first = shape.first(t);
        Fr r;
        Fr::from_bytes(tail + 32 * first, r);
        m = r * mult[first];
    }
    part[t] = m;
    fr_suffix_scan<LEG_WEIGHTS_MAX>(part, t);
    if (t < G) {
        fr_store_canonical(weights + 8 * (size_t)(t + 1), t + 1 < LEG_WEIGHTS_MAX ? part[t + 1] : Fr::one());
        fr_store_canonical(legs + 8 * (size_t)t, m);
    }
    if (t == 0) fr_store_canonical(weights, part[0]);
}
// k_leg_weights for an enqueued feed (h2v_accumulator_feed_batch, include/h2v_feed.h), where no host has seen the upload's verdict: the
// kernel reads the fault word of k_ingest_draws' verdict block itself (fault null: draws the host checked) and fails closed.  A draw
// >= r (fault[0] != 0xffffffff): weights <- [1, 0 .. 0], so that the k_accumulator_scale launch behind it leaves (L, R) its value and
// scales every leg away, and rc[0] <- H2V_ERR_BAD_ARGUMENT for the report; legs is written as ever (nobody commits it).  Otherwise
// k_leg_weights' outputs, word for word, and rc[0] <- 0.  Same shape: one workgroup, one suffix scan in LDS (18 KB).
// gfx950 (-Rpass-analysis=kernel-resource-usage): DESIGN.md section 3, "An enqueued feed".
__global__ void __launch_bounds__(LEG_WEIGHTS_MAX) k_feed_weights(const uint8_t* __restrict__ tail, const Fr* __restrict__ mult, GroupShape shape,
                                                                  const uint32_t* __restrict__ fault, uint32_t* __restrict__ weights, uint32_t* __restrict__ legs,
                                                                  uint32_t* __restrict__ rc) {
    __shared__ Fr part[LEG_WEIGHTS_MAX];
    const uint32_t t = threadIdx.x, G = shape.G;
    const bool bad = fault && fault[0] != 0xffffffffu;
    Fr m = Fr::one();
    if (t < G) {
        const size_t first = shape.first(t);
        Fr r;
        Fr::from_bytes(tail + 32 * first, r);
        m = r * mult[first];
    }
    part[t] = m;
    fr_suffix_scan<LEG_WEIGHTS_MAX>(part, t);
    if (t < G) {
        const Fr w = t + 1 < LEG_WEIGHTS_MAX ? part[t + 1] : Fr::one();
        fr_store_canonical(weights + 8 * (size_t)(t + 1), bad ? Fr::zero() : w);
        fr_store_canonical(legs + 8 * (size_t)t, m);
    }
    if (t == 0) {
        fr_store_canonical(weights, bad ? Fr::one() : part[0]);
        rc[0] = bad ? (uint32_t)H2V_ERR_BAD_ARGUMENT : 0u;
    }
}

// Instance evaluation for wide instance vectors (lib.rs:173-218; l_i_range, poly/domain.rs:187-212):
//   E = sum_j a_j * l_{j-rot}(x),   l_i(x) = omega^i (x^n - 1) / (n (x - omega^i))
// One workgroup per proof.  Thread t owns j = t, t + 256, ...: omega^(j-rot) advances by omega^256 per step.  The
// denominators are inverted in chunks of INSTEVAL_CHUNK per thread with Montgomery's trick (prefix products in LDS, one
// Fermat inversion per chunk, the denominators recomputed on the way back instead of stored); partial sums meet in an LDS
// tree.  A zero denominator (x on the domain) is reported like the program's zero inversions (H2V_ERR_REFERENCE_PANIC).
#define INSTEVAL_THREADS 256
#define INSTEVAL_CHUNK 16
__global__ void __launch_bounds__(INSTEVAL_THREADS) k_instance_eval(InstEvalArgs a) {
    extern __shared__ Fr insteval_lds[];                         // [INSTEVAL_CHUNK][256] prefix products, then [256] partial sums
    Fr* pre = insteval_lds;
    Fr* red = insteval_lds + (size_t)INSTEVAL_CHUNK * INSTEVAL_THREADS;
    const uint32_t p = blockIdx.x, t = threadIdx.x;
    const Fr x = a.chal[(size_t)a.x_chal * a.n + p];
    Fr w = a.w_start * a.omega.pow_u32(t);                       // omega^(t - rot)
    Fr acc = Fr::zero();
    bool zero_den = false;
    const uint8_t* vals = a.inst + ((size_t)p * a.ninst + a.base) * 32;
    for (uint32_t j0 = t; j0 < a.len; j0 += INSTEVAL_THREADS * INSTEVAL_CHUNK) {
        // forward: prefix products of the chunk's denominators
        Fr run = Fr::one(), wc = w;
        uint32_t cnt = 0;
        for (uint32_t c = 0; c < INSTEVAL_CHUNK && j0 + c * INSTEVAL_THREADS < a.len; ++c, ++cnt) {
            pre[(size_t)c * INSTEVAL_THREADS + t] = run;
            run = run * (x - wc);
            wc = wc * a.omega_step;
        }
        w = wc;                                                  // start of the thread's next chunk
        if (run.is_zero()) { zero_den = true; continue; }
        Fr inv = run.inv();
        // backward: 1/d_c = inv * prefix_c, then inv *= d_c; omega^(j-rot) steps back by omega^-256
        for (uint32_t c = cnt; c-- > 0;) {
            wc = wc * a.omega_step_inv;
            const Fr inv_d = inv * pre[(size_t)c * INSTEVAL_THREADS + t];
            inv = inv * (x - wc);
            uint8_t tmp[32];
            const uint8_t* src = vals + (size_t)(j0 + c * INSTEVAL_THREADS) * 32;
            for (int i = 0; i < 32; ++i) tmp[i] = src[i];
            Fr v;
            if (!Fr::from_bytes(tmp, v)) v = Fr::zero();        // non-canonical values were already reported by k_check_scalars
            acc = acc + v * wc * inv_d;
        }
    }
    red[t] = acc;
    __syncthreads();
    for (uint32_t d = INSTEVAL_THREADS / 2; d > 0; d >>= 1) {
        if (t < d) red[t] = red[t] + red[t + d];
        __syncthreads();
    }
    if (zero_den) status_set(a.status, p, H2V_DEV_ST_PANIC);
    if (t == 0) {
        Fr xn = x;
        for (uint32_t i = 0; i < a.k; ++i) xn = xn.sqr();
        a.out[p] = red[0] * (xn - Fr::one()) * a.n_inv;
    }
}

// Program slots.  The hottest ones (the lowest numbers: the allocator hands out freed slots last-in first-out) live in LDS,
// [slot][limb][lane]; the rest are limb-planar in global memory: limb l of slot s of proof p is word (s * 9 + l) * n + p, so that
// a wave's 64 proofs read 64 consecutive words per limb.  Round 1 kept every slot in global memory: each of the ~600
// instructions of a program waited for two L2 round trips before its ~0.5 us of arithmetic.
// a 32-byte little-endian scalar -> Fr (zero when not canonical).  Proof scalars and instance values sit at multiples of 32
// bytes inside records whose length is a multiple of 32, in hipMalloc'ed buffers: two 16-byte loads instead of 32 byte loads.
__device__ __forceinline__ Fr fr_from_le32(const uint8_t* b) {
    const uint4 lo = reinterpret_cast<const uint4*>(b)[0], hi = reinterpret_cast<const uint4*>(b)[1];
    const uint32_t raw[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    if (Fr::geq_p(raw)) return Fr::zero();
    return Fr::from_raw(raw);
}

struct SlotFile {
    uint32_t* lds; uint32_t lds_slots;
    Fr* glob; uint32_t n, p, lane;
    __device__ __forceinline__ Fr load(uint32_t s) const {
        Fr r;
        if (s < lds_slots) {
            const uint32_t* q = lds + (size_t)s * H2V_LIMBS * 64 + lane;
#pragma unroll
            for (int l = 0; l < H2V_LIMBS; ++l) r.v[l] = q[l * 64];
        } else {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(glob) + (size_t)s * H2V_LIMBS * n + p;
#pragma unroll
            for (int l = 0; l < H2V_LIMBS; ++l) r.v[l] = q[(size_t)l * n];
        }
        return r;
    }
    __device__ __forceinline__ void store(uint32_t s, const Fr& v) const {
        if (s < lds_slots) {
            uint32_t* q = lds + (size_t)s * H2V_LIMBS * 64 + lane;
#pragma unroll
            for (int l = 0; l < H2V_LIMBS; ++l) q[l * 64] = v.v[l];
        } else {
            uint32_t* q = reinterpret_cast<uint32_t*>(glob) + (size_t)s * H2V_LIMBS * n + p;
#pragma unroll
            for (int l = 0; l < H2V_LIMBS; ++l) q[(size_t)l * n] = v.v[l];
        }
    }
};

// one instruction stream over the slot file `sf` of proof p; `live` = p is a real proof (lanes past the end of a two-stream
// workgroup keep running for the barriers but touch no memory of their own)
template <bool TWO> __device__ __forceinline__ void frvm_run(const FrvmArgs& a, const VmInstr* __restrict__ code, uint32_t n_code, const SlotFile& sf, uint32_t p, bool live) {
    const uint32_t n = a.n;
    // an operand of MUL / ADD / SUB is a slot or (VM_CONST_OPERAND) a program constant, read with uniform loads
    // (an operand that is the previous instruction's result is taken from registers, not read back from the slot file: chains —
    // Horner folds, prefix products — skip a dependent LDS round trip per instruction.  The test is on wave-uniform instruction words.)
    Fr last = Fr::zero(); uint32_t last_d = 0xffffffffu;
    auto slot = [&](uint32_t x) -> Fr { return x == last_d ? last : sf.load(x); };
    auto opnd = [&](uint32_t x) -> Fr { return (x & VM_CONST_OPERAND) ? a.consts[x & ~VM_CONST_OPERAND] : slot(x); };
    auto put = [&](uint32_t d, const Fr& v) { sf.store(d, v); last = v; last_d = d; };
    VmInstr nx = code[0];
    for (uint32_t pc = 0; pc < n_code; ++pc) {
        const VmInstr in = nx;  // wave-uniform; the next instruction is fetched while this one executes
        nx = code[pc + 1 < n_code ? pc + 1 : pc];
        switch (in.op) {
            case OP_BARRIER: if (TWO) __syncthreads(); last_d = 0xffffffffu; break;   // (behind a barrier another stream may own the slot `last` mirrored)
            case OP_CONST: put(in.d, a.consts[in.a]); break;
            case OP_MUL: put(in.d, Fr::mul_chain(opnd(in.a), opnd(in.b))); break;
            case OP_ADD: put(in.d, opnd(in.a) + opnd(in.b)); break;
            case OP_SUB: put(in.d, opnd(in.a) - opnd(in.b)); break;
            case OP_NEG: put(in.d, slot(in.a).neg()); break;
            case OP_INV: {
                Fr v = slot(in.a);
                if (live && v.is_zero()) status_set(a.status, p, H2V_DEV_ST_PANIC);
                // all lanes invert at once: the divsteps of Fp::inv are branch-free, so the wave stays uniform
                put(in.d, v.inv());
                break;
            }
            case OP_POW: put(in.d, slot(in.a).pow_u32(in.b)); break;
            case OP_SQRN: {
                Fr v = slot(in.a);
                for (uint32_t i = 0; i < in.b; ++i) v = v.sqr();
                put(in.d, v);
                break;
            }
            case OP_LOAD_SCALAR: put(in.d, fr_from_le32(a.proofs + (size_t)p * a.proof_len + a.scalar_offsets[in.a])); break;  // status already set by k_check_scalars
            case OP_LOAD_INST: put(in.d, fr_from_le32(a.inst + ((size_t)p * a.ninst + in.a) * 32)); break;
            case OP_LOAD_CHAL: put(in.d, a.chal[(size_t)in.a * n + p]); break;
            case OP_LOAD_INSTEVAL: put(in.d, a.insteval[(size_t)in.a * n + p]); break;
            case OP_LOAD_MULT: put(in.d, a.mult[p]); break;
            case OP_STORE_MSM: {
                uint32_t raw[8];
                slot(in.a).to_raw(raw);
                bool bad = status_get(a.status, p) != 0;
                uint32_t* dst = a.msm_scal + ((size_t)p * a.np + in.b) * 8;
                if (live) for (int i = 0; i < 8; ++i) dst[i] = bad ? 0u : raw[i];
                break;
            }
            case OP_STORE_GUARD: {
                uint32_t raw[8];
                slot(in.a).to_raw(raw);
                uint32_t* dst = a.guard_scal + ((size_t)p * a.n_guard + in.b) * 8;
                if (live) for (int i = 0; i < 8; ++i) dst[i] = raw[i];
                break;
            }
            case OP_STORE_SHARED: {
                Fr v = slot(in.a);
                if (status_get(a.status, p) != 0) v = Fr::zero();
                if (live) a.shared[(size_t)in.b * n + p] = v;
                break;
            }
            case OP_STORE_LEFT: {
                uint32_t raw[8];
                slot(in.a).to_raw(raw);
                bool bad = status_get(a.status, p) != 0;
                uint32_t* dst = a.left_scal + ((size_t)p * a.np + in.b) * 8;
                if (live) for (int i = 0; i < 8; ++i) dst[i] = bad ? 0u : raw[i];
                break;
            }
            default: break;
        }
    }
}
__global__ void __launch_bounds__(64) k_frvm(FrvmArgs a, uint32_t lds_slots) {
    __builtin_amdgcn_s_setprio(3);   // a latency chain: its waves win the issue arbitration over the throughput kernels of other launches in flight
    extern __shared__ uint32_t frvm_lds[];
    uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    const SlotFile sf{frvm_lds, lds_slots, a.slots, a.n, p, threadIdx.x};
    frvm_run<false>(a, a.code, a.n_code, sf, p, true);
}
// Several instruction streams per proof (vkplan.hip: Builder::emit_streams): the K waves of a workgroup work on the SAME 64 proofs —
// wave w runs stream w — and share the slot file; values cross between them over OP_BARRIER only.  While one wave sits in the batched
// inversion's single inverse (a sixth of the program's work, indivisible), the others evaluate the expressions that do not need it.
__global__ void __launch_bounds__(64 * FRVM_MAX_STREAMS) k_frvm2(FrvmArgs a, uint32_t lds_slots) {
    __builtin_amdgcn_s_setprio(3);
    extern __shared__ uint32_t frvm_lds[];
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u, k = a.streams - 2;
    const uint32_t p_raw = blockIdx.x * 64 + lane;
    const bool live = p_raw < a.n;
    const uint32_t p = live ? p_raw : a.n - 1;   // lanes past the end shadow the last proof: they read its inputs, write nothing, and keep the barriers whole
    // (a shadow lane has its own LDS lane but shares the last proof's global slots: it writes there exactly what that proof's lane writes)
    const SlotFile sf{frvm_lds, lds_slots, a.slots, a.n, p, lane};
    frvm_run<true>(a, a.code_k[k][w], a.n_code_k[k][w], sf, p, live);
}

// dst[0 .. 8) = canonical( sum over the proofs p of [p0, p1) of col[p] ) by the workgroup's T threads (T a power of two; every thread
// calls it): a strided sum per thread, a tree in LDS
template <uint32_t T> __device__ __forceinline__ void fold_column(const Fr* __restrict__ col, uint32_t p0, uint32_t p1, uint32_t* __restrict__ dst) {
    __shared__ Fr red[T];
    const uint32_t t = threadIdx.x;
    Fr acc = Fr::zero();
    for (uint32_t p = p0 + t; p < p1; p += T) acc = acc + col[p];
    red[t] = acc;
    __syncthreads();
    for (uint32_t d = T / 2; d > 0; d >>= 1) {
        if (t < d) red[t] = red[t] + red[t + d];
        __syncthreads();
    }
    if (t == 0) {
        uint32_t raw[8]; red[0].to_raw(raw);
        for (int i = 0; i < 8; ++i) dst[i] = raw[i];
    }
}
// msm_scal[n*np + g*n_shared + j] = canonical( sum over the proofs p of group g of shared[j][p] ): a workgroup per (shared base, group)
// (the offsets of unequal groups are validated on the host: first(g) + count(g) <= n)
// gfx950 (tools/kernel_resources.py), with equal and with unequal groups as the two kernels it replaces: 32 VGPRs, 39 SGPRs, no spills,
// 48 bytes of scratch, 9216 bytes of LDS; 8 waves per SIMD.
__global__ void __launch_bounds__(256) k_fold_shared(const Fr* __restrict__ shared, uint32_t n, uint32_t np, GroupShape shape, uint32_t* __restrict__ msm_scal) {
    const uint32_t j = blockIdx.x, g = blockIdx.y, p0 = shape.first(g);
    fold_column<256>(shared + (size_t)j * n, p0, p0 + shape.count(g), msm_scal + ((size_t)n * np + (size_t)g * gridDim.x + j) * 8);
}

// out[(ranges[r].out + j) * 8] = canonical( sum over the proofs p of range r of ranges[r].shared[j][p] ).  The ranges of a re-check
// are mostly short (a search ends on single proofs): one wave per (base, range), a wave-wide tree in LDS.  The ranges of one launch
// may belong to batches of different keys (h2v_batches_recheck): the grid is as wide as the most VK-wide bases of any of them, and the
// blocks past a range's own n_shared leave at once (the whole block: the exit is uniform, before the first barrier)
// gfx950 (tools/kernel_resources.py): 32 VGPRs, 39 SGPRs, no spills, 48 bytes of scratch, 2304 bytes of LDS; 8 waves per SIMD.
__global__ void __launch_bounds__(64) k_fold_ranges(const FoldRange* __restrict__ ranges, uint32_t* __restrict__ out) {
    const uint32_t j = blockIdx.x;
    const FoldRange rg = ranges[blockIdx.y];
    if (j >= rg.n_shared) return;
    fold_column<64>(rg.shared + (size_t)j * rg.n, rg.first, rg.first + rg.count, out + ((size_t)rg.out + j) * 8);   // (validated on the host: first + count <= n)
}

// ------------------------------------------------------------------ launchers
int decompress_begin_enqueue(hipStream_t s, const StageArgs& g) {
    if (g.n) H2V_HIP_CHECK(hipMemsetAsync(g.status, 0, sizeof(int) * g.n, s));
    if (g.n && g.hints && g.hint_misses) H2V_HIP_CHECK(hipMemsetAsync(g.hint_misses, 0, sizeof(uint32_t), s));   // (a stage with hints: the misses of its pieces add up)
    return 0;
}
int decompress_range_enqueue(hipStream_t s, const StageArgs& g, uint32_t p0, uint32_t p1) {
    if (p1 <= p0) return 0;
    const Plan& pl = *g.plan;
    const uint32_t m = p1 - p0, tp = m * pl.n_points;
    if (!tp) return 0;
    const size_t off = (size_t)p0 * pl.n_points;   // the piece's first row of pts, phi, ycanon and (their rows are the points') the hints
    const uint8_t* proofs = g.proofs + (size_t)p0 * pl.proof_len;
    uint8_t* ycanon = g.ycanon + off * 32;
    const dim3 grid((tp + 63) / 64), block(64);
    if (!g.hints) {
        hipLaunchKernelGGL(k_decompress, grid, block, 0, s, proofs, pl.proof_len, g.pd->point_offsets.p, pl.n_points, pl.n_main_points, m, g.pts + off, g.phi + off, ycanon, g.status + p0);
        H2V_HIP_CHECK(hipGetLastError());
        return 0;
    }
    // With hints: k_decompress_hinted, the same outputs with a square root only where a hint fails, and k_decompress_misses behind it.
    // The piece's segment of the list starts at its first point, and its counter is cleared here, on the stream, in front of its two
    // kernels — so a piece neither sees nor redoes an earlier piece's entries, and every call leaves its own range complete.
    if (!g.hint_misses) { set_last_error("decompress_range_enqueue: hints without a miss word"); return H2V_ERR_BAD_ARGUMENT; }
    if (!g.miss_list || !g.miss_list_count) { set_last_error("decompress_range_enqueue: hints without a miss list and its counter"); return H2V_ERR_BAD_ARGUMENT; }
    H2V_HIP_CHECK(hipMemsetAsync(g.miss_list_count, 0, sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_decompress_hinted, grid, block, 0, s, proofs, pl.proof_len, g.pd->point_offsets.p, pl.n_points, pl.n_main_points, m, g.pts + off, g.phi + off, g.hints + off * 32,
                       ycanon, g.status + p0, g.hint_misses, g.miss_list + off, g.miss_list_count, (uint32_t)off);
    hipLaunchKernelGGL(k_decompress_misses, grid, block, K_DECOMPRESS_LDS_WORDS * sizeof(uint32_t), s, g.proofs, pl.proof_len, g.pd->point_offsets.p, pl.n_points, pl.n_main_points,
                       g.pts, g.phi, g.ycanon, g.status, g.miss_list + off, g.miss_list_count);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
int decompress_finish_enqueue(hipStream_t s, const StageArgs& g) {
    const Plan& pl = *g.plan;
    const uint32_t ts = g.n * (pl.n_scalars + pl.n_instance_values);
    if (ts) hipLaunchKernelGGL(k_check_scalars, dim3((ts + 255) / 256), dim3(256), 0, s, g.proofs, pl.proof_len, g.pd->scalar_offsets.p, pl.n_scalars, g.inst, pl.n_instance_values, g.n, g.status);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
int transcript_stage_enqueue(hipStream_t s, const StageArgs& g) {
    const uint32_t n = g.n;
    if (!n) return 0;
    const Plan& pl = *g.plan;
    uint32_t stream_len = (uint32_t)pl.stream.size();
    uint32_t n_words = g.stream_words;
    const bool keccak = pl.opts.transcript == H2V_TRANSCRIPT_KECCAK256;
    const uint32_t nsq = (uint32_t)pl.squeeze_at.size();
    const size_t lds = ((size_t)16 * TR4_MSG_STRIDE + (size_t)16 * nsq * 8) * 8;   // k_transcript's message blocks and digests
    // (refused before anything is launched: a stage that returns an error has not touched the words either)
    if (!keccak && lds > 60 * 1024) { set_last_error("transcript: too many challenges for one workgroup's LDS"); return H2V_ERR_UNSUPPORTED; }
    hipLaunchKernelGGL(k_stream_build, dim3((n + STREAM_PROOFS_PER_BLOCK - 1) / STREAM_PROOFS_PER_BLOCK), dim3(256), 0, s, g.pd->stream.p, stream_len, g.proofs, pl.proof_len, g.ycanon, pl.n_points, g.inst,
                       pl.n_instance_values, n, n_words, g.words);
    if (keccak)
        hipLaunchKernelGGL(k_transcript_keccak, dim3((n + 63) / 64), dim3(64), 0, s, g.words, n_words, g.pd->squeeze_at.p, nsq, n, g.chal);
    else
        hipLaunchKernelGGL(k_transcript, dim3((n + 15) / 16), dim3(64), lds, s, g.words, n_words, g.pd->squeeze_at.p, nsq, n, g.chal);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
int expand_draws_enqueue(hipStream_t s, const uint8_t seed32[32], uint64_t first, size_t n, void* d_out) {
    if (!n) return 0;
    if (n > (size_t)H2V_DRAWS_DEVICE_MAX) { set_last_error("expand_draws: more than H2V_DRAWS_DEVICE_MAX draws for one launch"); return H2V_ERR_BAD_ARGUMENT; }
    const size_t blocks = (n - 1) / 16 + 1;   // (< 2^26: the launch's 64 x blocks threads stay below 2^32, which HIP refuses)
    unsigned long long w[4];
    for (int j = 0; j < 4; ++j) { w[j] = 0; for (int k = 7; k >= 0; --k) w[j] = (w[j] << 8) | seed32[8 * j + k]; }
    hipLaunchKernelGGL(k_expand_draws, dim3((uint32_t)blocks), dim3(64), 0, s, w[0], w[1], w[2], w[3], (unsigned long long)first, (unsigned long long)n, (uint4*)d_out);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
// The scratch of the multipliers, in elements: a product per tile of the draw array and, behind the products, two words per tile
// (closed, open_from)
static uint32_t mult_tiles_of(const GroupShape& shape) { return (uint32_t)(((uint64_t)(shape.off ? 1u : shape.G) * shape.nt + MULT_TILE - 1) / MULT_TILE); }
size_t multipliers_scratch(const GroupShape& shape) {
    const size_t tiles = mult_tiles_of(shape);
    return tiles + (2 * tiles * sizeof(uint32_t) + sizeof(Fr) - 1) / sizeof(Fr);
}
int multipliers_enqueue(hipStream_t s, const GroupShape& shape, const uint8_t* d_tail, const uint8_t* d_last, Fr* d_mult, Fr* d_scratch) {
    const uint32_t tiles = mult_tiles_of(shape), n_draws = (shape.off ? 1u : shape.G) * shape.nt;
    if (!tiles || !shape.gs) return 0;
    if (shape.off && !d_last) { set_last_error("multipliers: groups of unequal size without their last-of-group marks"); return H2V_ERR_BAD_ARGUMENT; }
    uint32_t* tile_closed = reinterpret_cast<uint32_t*>(d_scratch + tiles); uint32_t* open_from = tile_closed + tiles;
    hipLaunchKernelGGL(k_seg_mult_tiles, dim3(tiles), dim3(MULT_TILE), 0, s, d_tail, d_last, shape, n_draws, d_mult, d_scratch, tile_closed, open_from);
    if (tiles > 1) {
        hipLaunchKernelGGL(k_seg_mult_scan_tiles, dim3(1), dim3(1024), 0, s, d_scratch, (const uint32_t*)tile_closed, tiles);
        hipLaunchKernelGGL(k_seg_mult_apply, dim3(tiles), dim3(MULT_TILE), 0, s, d_mult, d_last, shape, n_draws, (const Fr*)d_scratch, (const uint32_t*)open_from);
    }
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
int leg_weights_enqueue(hipStream_t s, const GroupShape& shape, const uint8_t* d_tail, const Fr* d_mult, uint32_t* d_weights, uint32_t* d_legs) {
    if (!shape.G || shape.G > LEG_WEIGHTS_MAX) { set_last_error("leg_weights_enqueue: the group count is not in 1 .. 512"); return H2V_ERR_BAD_ARGUMENT; }
    if (!d_tail || !d_mult || !d_weights || !d_legs) { set_last_error("leg_weights_enqueue: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    hipLaunchKernelGGL(k_leg_weights, dim3(1), dim3(LEG_WEIGHTS_MAX), 0, s, d_tail, d_mult, shape, d_weights, d_legs);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
int feed_weights_enqueue(hipStream_t s, const GroupShape& shape, const uint8_t* d_tail, const Fr* d_mult, const uint32_t* d_fault, uint32_t* d_weights, uint32_t* d_legs,
                         uint32_t* d_rc) {
    if (!shape.G || shape.G > LEG_WEIGHTS_MAX) { set_last_error("feed_weights_enqueue: the group count is not in 1 .. 512"); return H2V_ERR_BAD_ARGUMENT; }
    if (!d_tail || !d_mult || !d_weights || !d_legs || !d_rc) { set_last_error("feed_weights_enqueue: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    hipLaunchKernelGGL(k_feed_weights, dim3(1), dim3(LEG_WEIGHTS_MAX), 0, s, d_tail, d_mult, shape, d_fault, d_weights, d_legs, d_rc);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
__global__ void __launch_bounds__(256) k_gather_multipliers(const Fr* __restrict__ src, const uint32_t* __restrict__ idx, uint32_t n, Fr* __restrict__ out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = src[idx[i]];
}
int gather_multipliers_enqueue(hipStream_t s, const Fr* d_src, const uint32_t* d_idx, uint32_t n, Fr* d_out) {
    if (!n) return 0;
    hipLaunchKernelGGL(k_gather_multipliers, dim3((n + 255) / 256), dim3(256), 0, s, d_src, d_idx, n, d_out);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
int instance_eval_enqueue(hipStream_t s, const InstEvalArgs& a) {
    if (!a.n) return 0;
    const size_t lds = ((size_t)INSTEVAL_CHUNK + 1) * INSTEVAL_THREADS * sizeof(Fr);   // 153 KB: one workgroup per CU
    H2V_HIP_CHECK(hipFuncSetAttribute((const void*)k_instance_eval, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));   // per device; cheap
    hipLaunchKernelGGL(k_instance_eval, dim3(a.n), dim3(INSTEVAL_THREADS), lds, s, a);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
int frvm_enqueue(hipStream_t s, const FrvmArgs& a, uint32_t n_slots) {
    if (!a.n) return 0;
    // LDS for the hottest slots: 2304 bytes per slot and 64 proofs.  Every wave should still get a SIMD of its own (a program is a
    // latency chain), so the budget follows the number of workgroups: the whole 160 KB of a CU while there are at most 256,
    // half of it up to 384.
    const uint32_t waves = (a.n + 63) / 64;
    // streams per proof: as many as leave every wave of the launch a SIMD of its own (1024 SIMDs)
    uint32_t K = waves <= 341 ? 4u : 2u;   // measured at 320 workgroups: 260 / 255 / 242 us with 2 / 3 / 4 streams (four still win with 1280 waves)
    if (a.force_streams > 0) K = (uint32_t)a.force_streams;   // h2v_tuning.frvm_streams (1 = the single-stream interpreter k_frvm)
    const bool two = K >= 2 && K <= FRVM_MAX_STREAMS && a.code_k[K - 2][0] && a.n_code_k[K - 2][0];
    FrvmArgs ak = a;
    if (two) { n_slots = a.n_slots_k[K - 2]; ak.streams = K; }
    // (a launch with more workgroups than that is a throughput launch — several of them are in flight — and an LDS-hungry kernel keeps
    // the other kernels' workgroups off its CUs: a small slice then)
    uint32_t budget = waves <= 256 ? 156 * 1024 : (waves <= 384 ? 78 * 1024 : 36 * 1024);
    if (a.force_lds_kb > 0) budget = (uint32_t)std::min(a.force_lds_kb, 156) * 1024;   // h2v_tuning.frvm_lds_kb
    const uint32_t lds_slots = std::min<uint32_t>(n_slots, budget / (H2V_LIMBS * 64 * 4));
    const size_t lds = (size_t)lds_slots * H2V_LIMBS * 64 * 4;
    static std::atomic<size_t> granted{0};   // raising the limit is per function and sticky; do it once per size class
    if (lds > 64 * 1024 && granted.load() < lds) {
        H2V_HIP_CHECK(hipFuncSetAttribute((const void*)k_frvm, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        H2V_HIP_CHECK(hipFuncSetAttribute((const void*)k_frvm2, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        granted.store(160 * 1024);
    }
    if (two) hipLaunchKernelGGL(k_frvm2, dim3(waves), dim3(64 * K), lds, s, ak, lds_slots);
    else hipLaunchKernelGGL(k_frvm, dim3(waves), dim3(64), lds, s, a, lds_slots);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
int fold_shared_enqueue(hipStream_t s, const GroupShape& shape, const Fr* d_shared, uint32_t n, uint32_t np, uint32_t n_shared, uint32_t* d_msm_scal) {
    if (!n_shared || !shape.G) return 0;
    hipLaunchKernelGGL(k_fold_shared, dim3(n_shared, shape.G), dim3(256), 0, s, d_shared, n, np, shape, d_msm_scal);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
int fold_shared_ranges_enqueue(hipStream_t s, const FoldRange* d_ranges, uint32_t n_ranges, uint32_t max_shared, uint32_t* d_out) {
    if (!max_shared || !n_ranges) return 0;
    hipLaunchKernelGGL(k_fold_ranges, dim3(max_shared, n_ranges), dim3(64), 0, s, d_ranges, d_out);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace h2v
