// C++ caller of point hints (include/h2v_hints.hpp over include/h2v_hints.h), end to end.
//
//   hints_harness <dir> <n> <groups> <proof_len> <values per proof>
// reads <dir>/params.bin, vk.bin and the flat inputs of a staged batch (tests/cpp/caller.h), and runs the same grouped batch four
// times: without hints; with the hints h2v::hints::for_proofs makes on the host; with the rows the first launch left
// (h2v::hints::of_launch) from device memory, the rows 16 bytes apart with the gaps filled with 0xAB (set_device), reading the rows
// back through of_launch_device; and with all-zero hints.  It prints
//   offsets <the point offsets>
//   plain|host|device|zero <group verdicts> <status...> <left hex per group> <right hex per group> | <n_points> <n_hinted> <n_missed>
//   rows <same|differ> <same|differ>      the rows of_launch handed out against for_proofs; of_launch_device's against those
//   refused <code>                        twice: what the mirror refuses itself (a stride, a pointer off a 16-byte boundary)
// tests/test_gpu_cpp_hints.py builds it and compares the lines with each other and with Batch in Python.
#include "caller_hip.h"
#include "../../include/h2v_hints.hpp"

using namespace caller;

static void finish_and_print(const char* tag, h2v_batch* b, size_t n, size_t groups) {
    std::vector<int> st(n), ok(groups);
    Bytes left(64 * groups), right(64 * groups);
    check(h2v_batch_launch(b, 1));
    check(h2v_batch_finish_groups(b, st.data(), ok.data(), left.data(), right.data(), groups));
    group_results(tag, ok, st, left, right);
    const hints::Stats s = hints::stats(b);
    printf(" | %zu %zu %zu\n", s.points, s.hinted, s.missed);
}

int main(int argc, char** argv) {
    if (argc != 6) { fprintf(stderr, "usage: hints_harness <dir> <n> <groups> <proof_len> <values per proof>\n"); return 2; }
    const std::string d = argv[1];
    const size_t n = std::stoul(argv[2]), groups = std::stoul(argv[3]), plen = std::stoul(argv[4]), values = std::stoul(argv[5]);
    void *d_rows = nullptr, *d_back = nullptr;
    int rc = 0;
    try {
        ParamsKZG params{slurp(d + "/params.bin"), SerdeFormat::RawBytes};
        VerifyingKey vk{slurp(d + "/vk.bin"), SerdeFormat::RawBytes};
        const Staged in = read_staged(d, n, plen, values);
        Context ctx(params, vk);
        const std::vector<size_t> off = hints::point_offsets(ctx.handle());
        printf("offsets");
        for (size_t o : off) printf(" %zu", o);
        printf("\n");
        const size_t row = 32 * off.size(), stride = row + 16;
        BatchHolder batch;   // (gone before its context; waits for the batch's stream before the device rows go)
        stage(batch, ctx, n, groups, plen, values, in);
        h2v_batch* const b = batch.b;
        finish_and_print("plain", b, n, groups);
        const Bytes left_behind = hints::of_launch(b, 0, n, off.size());
        const Bytes made = hints::for_proofs(off, in.proofs, plen);

        check(h2v_batch_upload(b, n, in.proofs.data(), plen, in.inst.data(), 1, &values, in.rand.data(), n));
        hints::set(b, n, made);
        finish_and_print("host", b, n, groups);

        Bytes rows(n * stride, 0xAB);
        for (size_t i = 0; i < n; ++i) std::copy(left_behind.begin() + i * row, left_behind.begin() + (i + 1) * row, rows.begin() + i * stride);
        HIP(hipMalloc(&d_rows, rows.size())); HIP(hipMalloc(&d_back, rows.size()));
        HIP(hipMemcpy(d_rows, rows.data(), rows.size(), hipMemcpyHostToDevice));
        HIP(hipMemset(d_back, 0xCD, rows.size()));
        check(h2v_batch_upload(b, n, in.proofs.data(), plen, in.inst.data(), 1, &values, in.rand.data(), n));
        try { hints::set_device(b, n, d_rows, stride + 8); printf("unrefused stride\n"); } catch (const Failure& f) { printf("refused %d\n", f.code); }
        try { hints::set_device(b, n, static_cast<uint8_t*>(d_rows) + 4, stride); printf("unrefused pointer\n"); } catch (const Failure& f) { printf("refused %d\n", f.code); }
        hints::set_device(b, n, d_rows, stride);
        finish_and_print("device", b, n, groups);
        hints::of_launch_device(b, 0, n, d_back, stride);
        (void)hints::stats(b);   // (of_launch_device waits for nothing; stats waits for the batch's stream, and the copy below reads behind it)
        Bytes back(rows.size());
        HIP(hipMemcpy(back.data(), d_back, back.size(), hipMemcpyDeviceToHost));
        bool same_back = true;
        for (size_t i = 0; i < n; ++i) {
            same_back = same_back && std::equal(back.begin() + i * stride, back.begin() + i * stride + row, left_behind.begin() + i * row);
            for (size_t k = row; k < stride && i + 1 < n; ++k) same_back = same_back && back[i * stride + k] == 0xCD;
        }
        printf("rows %s %s\n", left_behind == made ? "same" : "differ", same_back ? "same" : "differ");

        check(h2v_batch_upload(b, n, in.proofs.data(), plen, in.inst.data(), 1, &values, in.rand.data(), n));
        hints::set(b, n, Bytes(n * row, 0));
        finish_and_print("zero", b, n, groups);
    } catch (const Failure& f) {
        fprintf(stderr, "failure %d: %s\n", f.code, f.what());
        rc = 1;
    }
    (void)hipFree(d_rows); (void)hipFree(d_back);
    return rc;
}
