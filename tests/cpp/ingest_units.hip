// k_ingest_rows and k_ingest_draws (halo2_verifier_amd/csrc/util.hip), the two launches of an upload from device memory
// (h2v_batch_upload_device), alone through their launchers ingest_rows_enqueue and ingest_draws_enqueue, on inputs chosen by
// tests/test_gpu_ingest_units.py.  Built with the library's flags by halo2_verifier_amd/csrc/Makefile (build/ingest_units); the prelude
// is tests/cpp/units.h.
//
//   ingest_units rows|draws IN OUT
// Files are little-endian uint32 words.  Every output buffer is preset to 0xff and lies between two guard bands that are checked after
// the kernels: a write past an output ends the program with status 5.  Every size and every group offset is checked on the host
// before the launch.
#include "../../halo2_verifier_amd/csrc/util.hip"
#include "units.h"

// IN: n_jobs; per job: n (rows), row_len, stride, inst_bytes (bytes, multiples of 16), groups; n * stride bytes of rows (padding
//     included); inst_bytes bytes of instance values
// OUT per job: the n * row_len packed bytes, the inst_bytes instance bytes, the groups + 2 words of the preset verdict block
static void rows_job(In& in, Out& out) {
    const uint32_t n = in.word(), row_len = in.word(), stride = in.word(), inst_bytes = in.word(), groups = in.word();
    REQUIRE(n <= 4096 && row_len <= 4096 && stride <= 8192 && inst_bytes <= (1u << 20) && groups >= 1 && groups <= 512, "bad rows job");
    REQUIRE(stride >= row_len && !((row_len | stride | inst_bytes) & 15u), "lengths: multiples of 16, the stride at least a row");
    const size_t src_words = (size_t)n * stride / 4;
    uint32_t* d_rows = to_device(in.span(src_words), src_words);
    uint32_t* d_inst = to_device(in.span(inst_bytes / 4), inst_bytes / 4);
    Guarded<uint8_t> rows((size_t)n * row_len), inst(inst_bytes);
    Guarded<uint32_t> verdict(groups + 2);
    RC(ingest_rows_enqueue(0, d_rows, stride, row_len, n, d_inst, inst_bytes, rows.p, inst.p, verdict.p, groups));
    CK(hipDeviceSynchronize());
    rows.collect(out, "packed rows"); inst.collect(out, "instance bytes"); verdict.collect(out, "verdict block");
    CK(hipFree(d_rows)); CK(hipFree(d_inst));
}

// IN: n_jobs; per job: n_tail, n, groups, ragged; (ragged) groups + 1 offsets; n_tail * 8 words of draw bytes
// OUT per job: the n_tail * 8 words of the stored tail, the 1 + groups words sent to the host block, the groups + 2 words of the device block
static void draws_job(In& in, Out& out) {
    const uint32_t n_tail = in.word(), n = in.word(), groups = in.word(), is_ragged = in.word();
    REQUIRE(n_tail <= (1u << 16) && n <= n_tail && groups >= 1 && groups <= 512 && is_ragged <= 1, "bad draws job");
    uint32_t* d_off = nullptr;
    if (is_ragged) {
        const std::vector<uint32_t> off = in.words(groups + 1);
        REQUIRE(off[0] == 0 && off[groups] == n_tail && n == n_tail, "offsets from 0 to n_tail == n");
        for (uint32_t g = 0; g < groups; ++g) REQUIRE(off[g] < off[g + 1], "a group of no proofs");
        d_off = to_device(off.data(), off.size());
    } else REQUIRE(n % groups == 0 && n_tail % groups == 0, "equal groups divide n and n_tail");
    uint32_t* d_draws = to_device(in.span((size_t)8 * n_tail), (size_t)8 * n_tail);
    Guarded<uint32_t> tail((size_t)8 * n_tail), host(1 + groups), verdict(groups + 2);
    RC(ingest_rows_enqueue(0, nullptr, 0, 0, 0, nullptr, 0, nullptr, nullptr, verdict.p, groups));   // (the preset, as the upload makes it)
    const GroupShape shape = d_off ? GroupShape::unequal(groups, n, d_off) : GroupShape::equal(groups, n, n_tail);
    RC(ingest_draws_enqueue(0, d_draws, reinterpret_cast<uint8_t*>(tail.p), n_tail, n, shape, verdict.p, host.p));
    CK(hipDeviceSynchronize());
    tail.collect(out, "tail"); host.collect(out, "host verdict"); verdict.collect(out, "verdict block");
    CK(hipFree(d_draws));
    if (d_off) CK(hipFree(d_off));
}

static const Mode MODES[] = {{"rows", each_job<rows_job, 256>, true, false}, {"draws", each_job<draws_job, 256>, true, false}};
int main(int argc, char** argv) { return units_main("ingest_units", MODES, argc, argv); }
