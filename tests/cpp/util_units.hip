// The record, byte-conversion and small group kernels and the fold of a merge (halo2_verifier_amd/csrc/util.hip) one by one, each
// through the library's own *_enqueue launcher, on inputs chosen by tests/test_gpu_record_units.py and tests/test_gpu_merge_units.py.
// Built with the library's flags by halo2_verifier_amd/csrc/Makefile (build/util_units); the prelude is tests/cpp/units.h.
//
//   util_units fold        IN OUT   k_fold_records: per job one fold over records given word for word
//   util_units export      IN OUT   k_export_records: from whole points or from pieces, with or without a status array
//   util_units to_bytes    IN OUT   k_point_to_bytes, with or without the LDS request of the auxiliary stream
//   util_units bases       IN OUT   k_bases_from_bytes
//   util_units scalars     IN OUT   k_scalars_from_bytes
//   util_units to_jacobian IN OUT   k_affine_to_jacobian
//   util_units copy        IN OUT   k_copy_words, with or without the LDS request
//   util_units merge_fold  IN OUT   k_accumulator_merge_fold through accumulator_merge_fold_enqueue
// Files are little-endian uint32 words; the layouts are in the readers below.  Points and records are raw 29-bit limbs as they lie
// in memory (the Python side picks every representative).  Every output buffer is preset to 0xff and lies between two guard bands
// that are checked after the kernel: a write past an output ends the program with status 5.  Every count, offset, index and slot
// that reaches a kernel is checked on the host first, and a record whose shift exceeds 1024 is refused: k_fold_records doubles a
// foreign record shift times per piece, and no input may turn that into a long-running kernel.
#include "../../halo2_verifier_amd/csrc/util.hip"
#include "units.h"

#define MAX_SHIFT 1024u

// ---- fold
// IN: n_jobs; per job: n_recs, groups, parts, shift, with_pieces (0: d_pieces = d_ready = nullptr), n_recs * groups records ([i][g], 328 words each)
// OUT per job: the parts the launcher folded into; acc (2 groups points of 27 words); (parts > 1) pieces, then ready (2 groups parts slots of 32
//     words each); fold_failed (groups words)
static void run_fold(In& in, Out& out) {
    for (uint32_t job = 0, jobs = job_count(in, 256); job < jobs; ++job) {
        const uint32_t n_recs = in.word(), groups = in.word(), parts = in.word(), shift = in.word(), with_pieces = in.word();
        REQUIRE(n_recs >= 1 && n_recs <= 256 && groups >= 1 && groups <= 64, "bad fold job");
        REQUIRE(parts >= 1 && parts <= H2V_ACC_RECORD_PIECES && shift <= MAX_SHIFT && with_pieces <= 1, "bad fold split");
        std::vector<AccRecord> recs((size_t)n_recs * groups);
        in.take(recs.data(), recs.size());
        for (const AccRecord& r : recs) REQUIRE(r.shift <= MAX_SHIFT, "record shift above 1024: refused");   // (parts is the kernel's to judge)
        const uint32_t eff = parts > 1 && with_pieces ? parts : 1;
        AccRecord* d_recs = to_device(recs.data(), recs.size());
        Guarded<G1J> acc((size_t)2 * groups);
        Guarded<G1JSlot> pieces(eff > 1 ? (size_t)2 * groups * eff : 0), ready(eff > 1 ? (size_t)2 * groups * eff : 0);
        Guarded<uint32_t> failed(groups);
        RC(fold_records_enqueue(0, d_recs, n_recs, groups, parts, shift, acc.p, eff > 1 ? pieces.p : nullptr, eff > 1 ? ready.p : nullptr, failed.p));
        CK(hipDeviceSynchronize());
        out.word(eff);
        acc.collect(out, "acc"); pieces.collect(out, "pieces"); ready.collect(out, "ready"); failed.collect(out, "fold_failed");
        CK(hipFree(d_recs));
    }
}

// ---- export
// IN: n_jobs; per job: groups, gs (proofs per group), parts, shift, from_pieces, with_status; the points (27 words each): 2 groups whole points, or
//     2 groups parts pieces ([(2g + side) parts + j]); (with_status) groups * gs status words
// OUT per job: groups records (328 words each)
static void run_export(In& in, Out& out) {
    for (uint32_t job = 0, jobs = job_count(in, 256); job < jobs; ++job) {
        const uint32_t groups = in.word(), gs = in.word(), parts = in.word(), shift = in.word(), from_pieces = in.word(), with_status = in.word();
        REQUIRE(groups >= 1 && groups <= 64 && gs <= 4096 && from_pieces <= 1 && with_status <= 1, "bad export job");
        REQUIRE(parts >= 1 && parts <= H2V_ACC_RECORD_PIECES && shift <= MAX_SHIFT, "bad export split");
        REQUIRE(with_status ? gs >= 1 : gs == 0, "a status array holds gs >= 1 words per group; without one gs = 0");
        const size_t n_pts = (size_t)2 * groups * (from_pieces ? parts : 1);
        std::vector<G1J> pts(n_pts);
        in.take(pts.data(), n_pts);
        std::vector<G1JSlot> slots(n_pts);
        for (size_t i = 0; i < n_pts; ++i) slots[i] = pts[i];
        G1J* d_acc = from_pieces ? nullptr : to_device(pts.data(), n_pts);
        G1JSlot* d_pieces = from_pieces ? to_device(slots.data(), n_pts) : nullptr;
        int* d_status = with_status ? to_device(reinterpret_cast<const int*>(in.span((size_t)groups * gs)), (size_t)groups * gs) : nullptr;
        Guarded<AccRecord> recs(groups);
        RC(export_records_enqueue(0, d_acc, d_pieces, parts, shift, d_status, groups * gs, groups, recs.p));
        CK(hipDeviceSynchronize());
        recs.collect(out, "records");
        if (d_acc) CK(hipFree(d_acc));
        if (d_pieces) CK(hipFree(d_pieces));
        if (d_status) CK(hipFree(d_status));
    }
}

// ---- to_bytes
// IN: n_jobs; per job: n, reserve (1: lds_reserve = H2V_AUX_LDS_RESERVE), n points (27 words)
// OUT per job: n * 16 words of x | y bytes, n identity flags
static void run_to_bytes(In& in, Out& out) {
    for (uint32_t job = 0, jobs = job_count(in, 256); job < jobs; ++job) {
        const uint32_t n = in.word(), reserve = in.word();
        REQUIRE(n <= 4096 && reserve <= 1, "bad to_bytes job");
        std::vector<G1J> pts(n);
        in.take(pts.data(), n);
        G1J* d_in = to_device(pts.data(), n);
        Guarded<uint32_t> bytes((size_t)16 * n), flags(n);
        RC(point_to_bytes_enqueue(0, d_in, reinterpret_cast<uint8_t*>(bytes.p), flags.p, n, reserve ? H2V_AUX_LDS_RESERVE : 0));
        CK(hipDeviceSynchronize());
        bytes.collect(out, "bytes"); flags.collect(out, "identity flags");
        CK(hipFree(d_in));
    }
}

// ---- bases
// IN: n_jobs; per job: n, n * 16 words of x | y bytes
// OUT per job: n affine points (18 words: x, y), n flags
static void run_bases(In& in, Out& out) {
    for (uint32_t job = 0, jobs = job_count(in, 256); job < jobs; ++job) {
        const uint32_t n = in.word();
        REQUIRE(n <= 4096, "bad bases job");
        uint32_t* d_in = to_device(in.span((size_t)16 * n), (size_t)16 * n);
        Guarded<G1A> pts(n);
        Guarded<uint32_t> flags(n);
        RC(bases_from_bytes_enqueue(0, reinterpret_cast<const uint8_t*>(d_in), pts.p, flags.p, n));
        CK(hipDeviceSynchronize());
        pts.collect(out, "bases"); flags.collect(out, "flags");
        CK(hipFree(d_in));
    }
}

// ---- scalars
// IN: n_jobs; per job: n, n * 8 words of scalar bytes
// OUT per job: n * 8 words, n flags
static void run_scalars(In& in, Out& out) {
    for (uint32_t job = 0, jobs = job_count(in, 256); job < jobs; ++job) {
        const uint32_t n = in.word();
        REQUIRE(n <= 4096, "bad scalars job");
        uint32_t* d_in = to_device(in.span((size_t)8 * n), (size_t)8 * n);
        Guarded<uint32_t> words((size_t)8 * n), flags(n);
        RC(scalars_from_bytes_enqueue(0, reinterpret_cast<const uint8_t*>(d_in), words.p, flags.p, n));
        CK(hipDeviceSynchronize());
        words.collect(out, "scalar words"); flags.collect(out, "flags");
        CK(hipFree(d_in));
    }
}

// ---- to_jacobian
// IN: n_jobs; per job: n, n affine points (18 words);  OUT per job: n Jacobian points (27 words)
static void run_to_jacobian(In& in, Out& out) {
    for (uint32_t job = 0, jobs = job_count(in, 256); job < jobs; ++job) {
        const uint32_t n = in.word();
        REQUIRE(n <= 4096, "bad to_jacobian job");
        std::vector<G1A> pts(n);
        in.take(pts.data(), n);
        G1A* d_in = to_device(pts.data(), n);
        Guarded<G1J> res(n);
        RC(affine_to_jacobian_enqueue(0, d_in, res.p, n));
        CK(hipDeviceSynchronize());
        res.collect(out, "points");
        CK(hipFree(d_in));
    }
}

// ---- copy
// IN: n_jobs; per job: n_words, reserve, n_words words;  OUT per job: n_words words
static void run_copy(In& in, Out& out) {
    for (uint32_t job = 0, jobs = job_count(in, 256); job < jobs; ++job) {
        const uint32_t n = in.word(), reserve = in.word();
        REQUIRE(n <= (1u << 20) && reserve <= 1, "bad copy job");
        uint32_t* d_in = to_device(in.span(n), n);
        Guarded<uint32_t> dst(n);
        RC(copy_words_enqueue(0, d_in, dst.p, n, reserve ? H2V_AUX_LDS_RESERVE : 0));
        CK(hipDeviceSynchronize());
        dst.collect(out, "words");
        CK(hipFree(d_in));
    }
}

// ---- merge_fold
// IN: n_jobs; per job: n (records), team (0: the host rule), with_sums, with_map, n_slots (pairs the journal array holds), (with_map) n slot
//     words, the accumulator (2 points of 27 words), n records (328 words each)
// OUT per job: the team the launch ran with, the accumulator (2 points), (with_sums) the journal array (2 n_slots points): a slot that no
//     record owns comes back as its preset
static void run_merge_fold(In& in, Out& out) {
    for (uint32_t job = 0, jobs = job_count(in, 256); job < jobs; ++job) {
        const uint32_t n = in.word(), team = in.word(), with_sums = in.word(), with_map = in.word(), n_slots = in.word();
        REQUIRE(n <= 512 && with_sums <= 1 && with_map <= 1 && n_slots <= 1024, "bad fold job");
        REQUIRE(team <= 64 && (team & (team - 1)) == 0, "the team is 0 or a power of two in 1 .. 64");
        REQUIRE(!with_map || with_sums, "a slot map without a journal array");
        REQUIRE(!with_sums || n_slots >= n, "fewer slots than records");
        const std::vector<uint32_t> slots = in.words(with_map ? n : 0);
        std::vector<bool> seen(n_slots, false);
        for (uint32_t s : slots) { REQUIRE(s < n_slots && !seen[s], "a slot out of range or given twice"); seen[s] = true; }
        static_assert(sizeof(G1J) == 108 && sizeof(AccRecord) == 1312, "word layouts");
        Guarded<G1J> acc(2), sums(with_sums ? (size_t)2 * n_slots : 0);
        CK(hipMemcpy((void*)acc.p, in.span(2 * sizeof(G1J) / 4), 2 * sizeof(G1J), hipMemcpyHostToDevice));
        std::vector<AccRecord> recs(n);
        in.take(recs.data(), n);
        AccRecord* d_recs = to_device(recs.data(), n);
        uint32_t* d_slots = with_map ? to_device(slots.data(), n) : nullptr;
        RC(accumulator_merge_fold_enqueue(0, d_recs, n, team, d_slots, with_sums ? sums.p : nullptr, acc.p));
        CK(hipDeviceSynchronize());
        out.word(team ? team : accumulator_merge_team(n));
        acc.collect(out, "acc"); sums.collect(out, "sums");
        CK(hipFree(d_recs));
        if (d_slots) CK(hipFree(d_slots));
    }
}

static const Mode MODES[] = {{"fold", run_fold, true, false}, {"export", run_export, true, false}, {"to_bytes", run_to_bytes, true, false},
                             {"bases", run_bases, true, false}, {"scalars", run_scalars, true, false}, {"to_jacobian", run_to_jacobian, true, false},
                             {"copy", run_copy, true, false}, {"merge_fold", run_merge_fold, true, false}};
int main(int argc, char** argv) { return units_main("util_units", MODES, argc, argv); }
