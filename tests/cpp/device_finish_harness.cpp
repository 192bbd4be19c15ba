// C++ caller of a staged batch's finish into device memory (include/h2v.hpp finish_device -> h2v_batch_finish_device).
//
//   device_finish_harness <dir> <n> <groups> <proof_len> <values per proof>
// reads <dir>/params.bin, vk.bin and the flat inputs of a staged batch (tests/cpp/caller.h), uploads and launches one grouped batch,
// and prints
//   refused <code>          three times: what the mirror refuses itself (a pointer off a 16-byte boundary, failed_cap 0), and what the
//                           library refuses (a status array in an allocation ONE byte short)
//   device <group verdicts> <status...> <left hex per group> <right hex per group> | <failed per group...> | <indices...> | <summary...>
//                           h2v::finish_device before the host finish, read after one synchronise of the batch's stream
//   host <group verdicts> <status...> <left hex> <right hex>          h2v_batch_finish_groups of the same launch
//   device ...              h2v::finish_device again, after the host finish
// tests/test_gpu_cpp_device_finish.py builds it and compares the lines with each other and with Batch.finish_groups in Python.
#include "caller_hip.h"

using namespace caller;

// the seven outputs in device memory, every byte preset to 0xEE
struct DeviceArrays {
    size_t n, groups;
    DeviceResults r;
    int alloc() {
        HIP(hipMalloc(&r.status, 4 * n + 16)); HIP(hipMalloc(&r.group_ok, 4 * groups)); HIP(hipMalloc(&r.left_xy, 64 * groups)); HIP(hipMalloc(&r.right_xy, 64 * groups));
        HIP(hipMalloc(&r.group_failed, 4 * groups)); HIP(hipMalloc(&r.failed_index, 4 * n)); HIP(hipMalloc(&r.summary, 4 * H2V_SUMMARY_WORDS));
        r.failed_cap = n;
        return 0;
    }
    int preset() {
        HIP(hipMemset(r.status, 0xEE, 4 * n)); HIP(hipMemset(r.group_ok, 0xEE, 4 * groups)); HIP(hipMemset(r.left_xy, 0xEE, 64 * groups)); HIP(hipMemset(r.right_xy, 0xEE, 64 * groups));
        HIP(hipMemset(r.group_failed, 0xEE, 4 * groups)); HIP(hipMemset(r.failed_index, 0xEE, 4 * n)); HIP(hipMemset(r.summary, 0xEE, 4 * H2V_SUMMARY_WORDS));
        return hipDeviceSynchronize() == hipSuccess ? 0 : 3;
    }
    // (after the batch's stream has been synchronised)
    int print() const {
        std::vector<int> st(n), ok(groups);
        std::vector<uint32_t> failed(groups), index(n), summary(H2V_SUMMARY_WORDS);
        Bytes left(64 * groups), right(64 * groups);
        HIP(hipMemcpy(st.data(), r.status, 4 * n, hipMemcpyDeviceToHost)); HIP(hipMemcpy(ok.data(), r.group_ok, 4 * groups, hipMemcpyDeviceToHost));
        HIP(hipMemcpy(left.data(), r.left_xy, 64 * groups, hipMemcpyDeviceToHost)); HIP(hipMemcpy(right.data(), r.right_xy, 64 * groups, hipMemcpyDeviceToHost));
        HIP(hipMemcpy(failed.data(), r.group_failed, 4 * groups, hipMemcpyDeviceToHost)); HIP(hipMemcpy(index.data(), r.failed_index, 4 * n, hipMemcpyDeviceToHost));
        HIP(hipMemcpy(summary.data(), r.summary, 4 * H2V_SUMMARY_WORDS, hipMemcpyDeviceToHost));
        group_results("device", ok, st, left, right);
        printf(" |"); for (uint32_t v : failed) printf(" %u", v);
        printf(" |"); for (uint32_t v : index) printf(" %u", v);
        printf(" |"); for (uint32_t v : summary) printf(" %u", v);
        printf("\n");
        return 0;
    }
    ~DeviceArrays() {
        for (void* p : {r.status, r.group_ok, r.left_xy, r.right_xy, r.group_failed, r.failed_index, r.summary}) (void)hipFree(p);
    }
};

int main(int argc, char** argv) {
    if (argc != 6) { fprintf(stderr, "usage: device_finish_harness <dir> <n> <groups> <proof_len> <values per proof>\n"); return 2; }
    const std::string d = argv[1];
    const size_t n = std::stoul(argv[2]), groups = std::stoul(argv[3]), plen = std::stoul(argv[4]), values = std::stoul(argv[5]);
    DeviceArrays out{n, groups, {}};
    void* short_status = nullptr;
    int rc = 0;
    try {
        ParamsKZG params{slurp(d + "/params.bin"), SerdeFormat::RawBytes};
        VerifyingKey vk{slurp(d + "/vk.bin"), SerdeFormat::RawBytes};
        const Staged in = read_staged(d, n, plen, values);
        Context ctx(params, vk);
        BatchHolder batch;   // (gone before its context; waits for the batch's stream before the outputs go)
        stage(batch, ctx, n, groups, plen, values, in);
        h2v_batch* const b = batch.b;
        check(h2v_batch_launch(b, 1));
        if ((rc = out.alloc()) || (rc = out.preset())) return rc;
        HIP(hipMalloc(&short_status, 4 * n - 1));
        // what the mirror refuses itself, before the library; and the library's own bounds check
        DeviceResults bad = out.r;
        bad.status = static_cast<uint8_t*>(out.r.status) + 4;
        try { finish_device(b, bad); printf("unrefused pointer\n"); } catch (const Failure& f) { printf("refused %d\n", f.code); }
        bad = out.r; bad.failed_cap = 0;
        try { finish_device(b, bad); printf("unrefused cap\n"); } catch (const Failure& f) { printf("refused %d\n", f.code); }
        bad = out.r; bad.status = short_status;
        try { finish_device(b, bad); printf("unrefused allocation\n"); } catch (const Failure& f) { printf("refused %d\n", f.code); }
        hipStream_t s = static_cast<hipStream_t>(h2v_batch_stream(b));
        finish_device(b, out.r);
        HIP(hipStreamSynchronize(s));
        if ((rc = out.print())) return rc;
        std::vector<int> st(n), ok(groups);
        Bytes left(64 * groups), right(64 * groups);
        check(h2v_batch_finish_groups(b, st.data(), ok.data(), left.data(), right.data(), groups));
        group_results("host", ok, st, left, right);
        printf("\n");
        if ((rc = out.preset())) return rc;
        finish_device(b, out.r);
        HIP(hipStreamSynchronize(s));
        if ((rc = out.print())) return rc;
    } catch (const Failure& f) {
        fprintf(stderr, "failure %d: %s\n", f.code, f.what());
        rc = 1;
    }
    (void)hipFree(short_status);
    return rc;
}
