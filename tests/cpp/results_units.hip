// k_results_tiles, k_results_close and k_results_scatter (halo2_verifier_amd/csrc/util.hip), the launches of a finish into device memory
// (h2v_batch_finish_device), alone through their launcher results_enqueue, on inputs chosen by tests/test_gpu_results_units.py.  Built
// with the library's flags by halo2_verifier_amd/csrc/Makefile (build/results_units); the prelude is tests/cpp/units.h.
//
//   results_units finish IN OUT
// Files are little-endian uint32 words.  Every output buffer is preset to 0xff and lies between two guard bands that are checked after
// the kernels: a write past an output ends the program with status 5.  Every size and every group offset is checked on the host
// before the launch.
#include "../../halo2_verifier_amd/csrc/util.hip"
#include "units.h"

// IN: n_jobs; per job: n, groups, ragged, flags, fault (0xffffffff: no fault block is passed), cap, want (bit k: output k is given, in
//     the order status, group_ok, left, right, group_failed, failed_index, summary), repeat (1 or 2: the launcher runs that often on
//     the same scratch); (ragged) groups + 1 offsets; n status words; groups fold_failed words; groups ok words; 32 * groups words of
//     accumulator bytes
// OUT per job: every output in that order, given or not (one not given: a buffer of its own that must come back untouched, 0xff) —
//     n words, groups words, 16 * groups words, 16 * groups words, groups words, cap words, 8 words — and the groups words of the
//     scratch, which must be zero again
static void finish_job(In& in, Out& out) {
    const uint32_t n = in.word(), groups = in.word(), is_ragged = in.word(), flags = in.word(), fault = in.word(), cap = in.word(), want = in.word(), repeat = in.word();
    REQUIRE(n <= (1u << 17) && groups >= 1 && groups <= 512 && is_ragged <= 1 && flags <= 3 && cap <= (1u << 17) && want < 128 && repeat >= 1 && repeat <= 2, "bad finish job");
    REQUIRE(!(want & 32u) || cap >= 1, "indices wanted with no room");
    uint32_t* d_off = nullptr;
    if (is_ragged) {
        const std::vector<uint32_t> off = in.words(groups + 1);
        REQUIRE(off[0] == 0 && off[groups] == n, "offsets from 0 to n");
        for (uint32_t g = 0; g < groups; ++g) REQUIRE(off[g] < off[g + 1], "a group of no proofs");
        d_off = to_device(off.data(), off.size());
    } else REQUIRE(n % groups == 0, "equal groups divide n");
    uint32_t* d_status = to_device(in.span(n), n);
    uint32_t* d_fold = to_device(in.span(groups), groups);
    uint32_t* d_ok = to_device(in.span(groups), groups);
    uint32_t* d_bytes = to_device(in.span((size_t)32 * groups), (size_t)32 * groups);
    uint32_t* d_fault = fault != 0xffffffffu ? to_device(&fault, 1) : nullptr;
    Guarded<uint32_t> status(n), group_ok(groups), left((size_t)16 * groups), right((size_t)16 * groups), group_failed(groups), index(cap), summary(8);
    Guarded<uint32_t> tile_words(results_tiles(n)), group_words(groups, 0);
    ResultsOut o;
    if (want & 1u) o.status = reinterpret_cast<int*>(status.p);
    if (want & 2u) o.group_ok = reinterpret_cast<int*>(group_ok.p);
    if (want & 4u) o.left_xy = reinterpret_cast<uint8_t*>(left.p);
    if (want & 8u) o.right_xy = reinterpret_cast<uint8_t*>(right.p);
    if (want & 16u) o.group_failed = group_failed.p;
    if (want & 32u) { o.failed_index = index.p; o.failed_cap = cap; }
    if (want & 64u) o.summary = summary.p;
    const GroupShape shape = d_off ? GroupShape::unequal(groups, n, d_off) : GroupShape::equal(groups, n, n);
    for (uint32_t r = 0; r < repeat; ++r)
        RC(results_enqueue(0, reinterpret_cast<const int*>(d_status), n, shape, d_fold, d_ok, flags, reinterpret_cast<const uint8_t*>(d_bytes), d_fault, tile_words.p, group_words.p, o));
    CK(hipDeviceSynchronize());
    status.collect(out, "status"); group_ok.collect(out, "group_ok"); left.collect(out, "left_xy"); right.collect(out, "right_xy");
    group_failed.collect(out, "group_failed"); index.collect(out, "failed_index"); summary.collect(out, "summary");
    (void)tile_words.host("tile words");
    group_words.collect(out, "group words");
    CK(hipFree(d_status)); CK(hipFree(d_fold)); CK(hipFree(d_ok)); CK(hipFree(d_bytes));
    if (d_off) CK(hipFree(d_off));
    if (d_fault) CK(hipFree(d_fault));
}

static const Mode MODES[] = {{"finish", each_job<finish_job, 1024>, true, false}};
int main(int argc, char** argv) { return units_main("results_units", MODES, argc, argv); }
