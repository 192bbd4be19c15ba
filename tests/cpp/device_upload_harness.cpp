// C++ caller of a staged batch's upload from device memory (include/h2v.hpp upload_device -> h2v_batch_upload_device).
//
//   device_upload_harness <dir> <n> <groups> <proof_len> <values per proof>
// reads <dir>/params.bin, vk.bin and the flat inputs of a staged batch (tests/cpp/caller.h), runs the same grouped batch twice —
// h2v_batch_upload from the host bytes, then h2v::upload_device from copies of them in device memory, the proof rows 48 bytes apart
// with the gaps filled with 0xAB — and prints, once per run,
//   host|device <group verdicts> <status...> <left hex per group> <right hex per group>
// tests/test_gpu_cpp_device_upload.py builds it and compares the two lines with each other and with Batch.upload in Python.
#include "caller_hip.h"

using namespace caller;

static void finish_and_print(const char* tag, h2v_batch* b, size_t n, size_t groups) {
    std::vector<int> st(n), ok(groups);
    Bytes left(64 * groups), right(64 * groups);
    check(h2v_batch_launch(b, 1));
    check(h2v_batch_finish_groups(b, st.data(), ok.data(), left.data(), right.data(), groups));
    group_results(tag, ok, st, left, right);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 6) { fprintf(stderr, "usage: device_upload_harness <dir> <n> <groups> <proof_len> <values per proof>\n"); return 2; }
    const std::string d = argv[1];
    const size_t n = std::stoul(argv[2]), groups = std::stoul(argv[3]), plen = std::stoul(argv[4]), values = std::stoul(argv[5]);
    const size_t stride = plen + 48;
    void *d_proofs = nullptr, *d_inst = nullptr, *d_rand = nullptr;
    int rc = 0;
    try {
        ParamsKZG params{slurp(d + "/params.bin"), SerdeFormat::RawBytes};
        VerifyingKey vk{slurp(d + "/vk.bin"), SerdeFormat::RawBytes};
        const Staged in = read_staged(d, n, plen, values);
        Context ctx(params, vk);
        const std::vector<size_t> col_lens{values};
        BatchHolder batch;   // (gone before its context; waits for the batch's stream before the inputs go)
        stage(batch, ctx, n, groups, plen, values, in);
        h2v_batch* const b = batch.b;
        finish_and_print("host", b, n, groups);
        Bytes rows(n * stride, 0xAB);
        for (size_t i = 0; i < n; ++i) std::copy(in.proofs.begin() + i * plen, in.proofs.begin() + (i + 1) * plen, rows.begin() + i * stride);
        HIP(hipMalloc(&d_proofs, rows.size())); HIP(hipMalloc(&d_inst, in.inst.size() + 16)); HIP(hipMalloc(&d_rand, in.rand.size()));
        HIP(hipMemcpy(d_proofs, rows.data(), rows.size(), hipMemcpyHostToDevice));
        HIP(hipMemcpy(d_inst, in.inst.data(), in.inst.size(), hipMemcpyHostToDevice));
        HIP(hipMemcpy(d_rand, in.rand.data(), in.rand.size(), hipMemcpyHostToDevice));
        // what the mirror refuses itself, before the library
        try { upload_device(b, n, d_proofs, stride + 8, d_inst, col_lens, d_rand, n); printf("unrefused stride\n"); } catch (const Failure& f) { printf("refused %d\n", f.code); }
        try { upload_device(b, n, static_cast<uint8_t*>(d_proofs) + 4, stride, d_inst, col_lens, d_rand, n); printf("unrefused pointer\n"); } catch (const Failure& f) { printf("refused %d\n", f.code); }
        upload_device(b, n, d_proofs, stride, d_inst, col_lens, d_rand, n);
        finish_and_print("device", b, n, groups);
    } catch (const Failure& f) {
        fprintf(stderr, "failure %d: %s\n", f.code, f.what());
        rc = 1;
    }
    (void)hipFree(d_proofs); (void)hipFree(d_inst); (void)hipFree(d_rand);
    return rc;
}
