// The two kernels behind h2v_accumulator_process_batch that are its own, one by one, each through the library's own launcher, on inputs
// chosen by tests/test_gpu_legs_units.py.  Built with the library's flags by halo2_verifier_amd/csrc/Makefile (build/legs_units); the
// prelude is tests/cpp/units.h.
//
//   legs_units weights   IN OUT   k_leg_weights (verify_kernels.hip) through leg_weights_enqueue
//   legs_units legs_fold IN OUT   k_accumulator_legs_fold (util.hip) through accumulator_legs_fold_enqueue
// Files are little-endian uint32 words; the layouts are in the readers below.  Points and records are raw 29-bit limbs as they lie in
// memory (the Python side picks every representative); scalars are 8 canonical words.  Every output buffer is preset to 0xff and lies
// between two guard bands that are checked after the kernel: a write past an output ends the program with status 5.  Every count,
// offset and slot that reaches a kernel is checked on the host first.
#include "../../halo2_verifier_amd/csrc/verify_kernels.hip"
#include "../../halo2_verifier_amd/csrc/util.hip"
#include "units.h"

// ---- weights
// IN: n_jobs; per job: G, n (draws = proofs), with_off, gs (equal groups: proofs per group; with_off: ignored), (with_off) G offsets,
//     n draws (8 words each, canonical), n multipliers (8 words each, canonical: the harness puts them into the library's form)
// OUT per job: 8 (G + 1) words [prod M, W_0 .. W_{G-1}], 8 G words [M_0 .. M_{G-1}]
static void job_weights(In& in, Out& out) {
    const uint32_t G = in.word(), n = in.word(), with_off = in.word(), gs = in.word();
    REQUIRE(G >= 1 && G <= 512 && n >= 1 && n <= (1u << 16) && with_off <= 1, "bad weights job");
    const std::vector<uint32_t> off = in.words(with_off ? G : 0);
    for (uint32_t g = 0; g < G; ++g) REQUIRE(with_off ? off[g] < n : (uint64_t)g * gs < n, "a group's first proof past the draws");
    uint8_t* d_tail = to_device(in.bytes((size_t)32 * n), (size_t)32 * n);
    const std::vector<Fr> mult = in.fields<Fr>(n);
    Fr* d_mult = to_device(mult.data(), n);
    uint32_t* d_off = with_off ? to_device(off.data(), G) : nullptr;
    Guarded<uint32_t> weights((size_t)8 * (G + 1)), legs((size_t)8 * G);
    RC(leg_weights_enqueue(0, GroupShape{G, gs, gs, d_off}, d_tail, d_mult, weights.p, legs.p));   // (the kernel reads first(g) alone: off[0 .. G - 1], or g * gs)
    CK(hipDeviceSynchronize());
    weights.collect(out, "weights"); legs.collect(out, "legs");
    CK(hipFree(d_tail)); CK(hipFree(d_mult));
    if (d_off) CK(hipFree(d_off));
}

// ---- legs_fold
// IN: n_jobs; per job: n (records, >= 1), team (0: the host rule), with_sums, with_map, n_slots (pairs the journal array holds), (with_map)
//     n - 1 slot words, the accumulator as it stands (2 points of 27 words: the fold must replace it), n records (328 words each),
//     (with_sums) the n - 1 unscaled pairs (2 points each)
// OUT per job: the team the launch ran with, the accumulator (2 points), (with_sums) the journal array (2 n_slots points): a slot that no
//     leg owns comes back as its preset
static void job_legs_fold(In& in, Out& out) {
    const uint32_t n = in.word(), team = in.word(), with_sums = in.word(), with_map = in.word(), n_slots = in.word();
    REQUIRE(n >= 1 && n <= 513 && with_sums <= 1 && with_map <= 1 && n_slots <= 1024, "bad legs_fold job");
    REQUIRE(team <= 64 && (team & (team - 1)) == 0, "the team is 0 or a power of two in 1 .. 64");
    REQUIRE(!with_map || with_sums, "a slot map without a journal array");
    REQUIRE(!with_sums || n_slots >= n - 1, "fewer slots than legs");
    const std::vector<uint32_t> slots = in.words(with_map ? n - 1 : 0);
    std::vector<bool> seen(n_slots, false);
    for (uint32_t s : slots) { REQUIRE(s < n_slots && !seen[s], "a slot out of range or given twice"); seen[s] = true; }
    static_assert(sizeof(G1J) == 108 && sizeof(AccRecord) == 1312, "word layouts");
    Guarded<G1J> acc(2), sums(with_sums ? (size_t)2 * n_slots : 0);
    CK(hipMemcpy((void*)acc.p, in.span(2 * sizeof(G1J) / 4), 2 * sizeof(G1J), hipMemcpyHostToDevice));
    std::vector<AccRecord> recs(n);
    in.take(recs.data(), n);
    std::vector<G1J> pairs(with_sums ? (size_t)2 * (n - 1) : 0);
    in.take(pairs.data(), pairs.size());
    AccRecord* d_recs = to_device(recs.data(), n);
    G1J* d_pairs = with_sums ? to_device(pairs.data(), pairs.size()) : nullptr;
    uint32_t* d_slots = with_map ? to_device(slots.data(), slots.size()) : nullptr;
    RC(accumulator_legs_fold_enqueue(0, d_recs, n, team, d_pairs, d_slots, with_sums ? sums.p : nullptr, acc.p));
    CK(hipDeviceSynchronize());
    out.word(team ? team : accumulator_merge_team(n - 1));
    acc.collect(out, "acc"); sums.collect(out, "sums");
    CK(hipFree(d_recs));
    if (d_pairs) CK(hipFree(d_pairs));
    if (d_slots) CK(hipFree(d_slots));
}

static const Mode MODES[] = {{"weights", each_job<job_weights, 256>, true, false}, {"legs_fold", each_job<job_legs_fold, 256>, true, false}};
int main(int argc, char** argv) { return units_main("legs_units", MODES, argc, argv); }
