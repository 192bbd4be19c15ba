// C++ caller of every proof's Guard out of a launch (include/h2v_guards.hpp -> include/h2v_guards.h).
//
//   guards_out_harness <dir> <n> <groups> <proof_len> <values per proof> <first> <count>
// reads <dir>/params.bin, vk.bin and the flat inputs of a staged batch (tests/cpp/caller.h), uploads and launches one grouped batch,
// and prints for the range [first, first + count)
//   shape <T_L> <T_R>
//   refused <code>          twice: what the mirror refuses itself (a pointer off a 16-byte boundary) and what the library refuses (a
//                           range past the upload)
//   host <status...> | <left scalars hex> <left bases hex> <right scalars hex> <right bases hex> <mult hex>      h2v::guards::to_host
//   device ...              h2v::guards::to_device into hipMalloc'ed arrays, read after one synchronise of the batch's stream
//   append <failed> | <left scalars hex> <left bases hex> <right scalars hex> <right bases hex>                  h2v::guards::append
//                           into two empty h2v::Msm objects, read back through Msm::scalars / bases
//   guard <j> <right scalars hex>                                   h2v::guards::guard_of for the range's last proof
//   finish <group verdicts> <status...>                             h2v_batch_finish_groups afterwards
// tests/test_gpu_cpp_guards_out.py builds it and compares the lines with each other and with Batch.guards in Python.
#include "caller_hip.h"
#include "../../include/h2v_guards.hpp"

using namespace caller;

static void print_guards(const char* tag, const std::vector<int>& st, const Guard& g, const Bytes& mult) {
    printf("%s", tag);
    for (int v : st) printf(" %d", v);
    printf(" | "); hex_or_dash(g.left_scalars); printf(" "); hex_or_dash(g.left_bases); printf(" "); hex_or_dash(g.right_scalars); printf(" "); hex_or_dash(g.right_bases);
    printf(" "); hex_or_dash(mult);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 8) { fprintf(stderr, "usage: guards_out_harness <dir> <n> <groups> <proof_len> <values per proof> <first> <count>\n"); return 2; }
    const std::string d = argv[1];
    const size_t n = std::stoul(argv[2]), groups = std::stoul(argv[3]), plen = std::stoul(argv[4]), values = std::stoul(argv[5]), first = std::stoul(argv[6]),
                 count = std::stoul(argv[7]);
    void* dev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int rc = 0;
    try {
        ParamsKZG params{slurp(d + "/params.bin"), SerdeFormat::RawBytes};
        VerifyingKey vk{slurp(d + "/vk.bin"), SerdeFormat::RawBytes};
        const Staged in = read_staged(d, n, plen, values);
        if (!count || first + count > n) bad_input("the range lies outside the n proofs");
        Context ctx(params, vk);
        Msm left(ctx), right(ctx);   // (gone before the context, after the batch)
        BatchHolder batch;           // (waits for the batch's stream before the outputs go)
        stage(batch, ctx, n, groups, plen, values, in);
        h2v_batch* const b = batch.b;
        check(h2v_batch_launch(b, 1));
        const guards::Shape sh = guards::shape(b);
        printf("shape %zu %zu\n", sh.left_terms, sh.right_terms);
        const size_t bytes[6] = {32 * count * sh.left_terms, 64 * count * sh.left_terms, 32 * count * sh.right_terms, 64 * count * sh.right_terms, 32 * count, 4 * count};
        for (int k = 0; k < 6; ++k) { HIP(hipMalloc(&dev[k], bytes[k])); HIP(hipMemset(dev[k], 0xEE, bytes[k])); }
        HIP(hipDeviceSynchronize());
        guards::DeviceGuards out{dev[0], dev[1], dev[2], dev[3], dev[4], dev[5]};
        guards::DeviceGuards bad = out;
        bad.mult = static_cast<uint8_t*>(dev[4]) + 4;
        try { guards::to_device(b, first, count, bad); printf("unrefused pointer\n"); } catch (const Failure& f) { printf("refused %d\n", f.code); }
        try { guards::to_device(b, first, n - first + 1, out); printf("unrefused range\n"); } catch (const Failure& f) { printf("refused %d\n", f.code); }
        const guards::HostGuards host = guards::to_host(b, first, count);
        print_guards("host", host.status, host.terms, host.mult);
        guards::to_device(b, first, count, out);
        HIP(hipStreamSynchronize(static_cast<hipStream_t>(h2v_batch_stream(b))));
        Guard g;
        Bytes mult(bytes[4]);
        std::vector<int> st(count);
        g.left_scalars.resize(bytes[0]); g.left_bases.resize(bytes[1]); g.right_scalars.resize(bytes[2]); g.right_bases.resize(bytes[3]);
        HIP(hipMemcpy(g.left_scalars.data(), dev[0], bytes[0], hipMemcpyDeviceToHost)); HIP(hipMemcpy(g.left_bases.data(), dev[1], bytes[1], hipMemcpyDeviceToHost));
        HIP(hipMemcpy(g.right_scalars.data(), dev[2], bytes[2], hipMemcpyDeviceToHost)); HIP(hipMemcpy(g.right_bases.data(), dev[3], bytes[3], hipMemcpyDeviceToHost));
        HIP(hipMemcpy(mult.data(), dev[4], bytes[4], hipMemcpyDeviceToHost)); HIP(hipMemcpy(st.data(), dev[5], bytes[5], hipMemcpyDeviceToHost));
        print_guards("device", st, g, mult);
        const size_t failed = guards::append(b, first, count, &left, &right);
        printf("append %zu | ", failed); hex_or_dash(left.scalars()); printf(" "); hex_or_dash(left.bases()); printf(" "); hex_or_dash(right.scalars()); printf(" "); hex_or_dash(right.bases());
        printf("\n");
        const Guard last = guards::guard_of(host, count - 1);
        printf("guard %zu ", count - 1); hex_or_dash(last.right_scalars); printf("\n");
        std::vector<int> fst(n), ok(groups);
        check(h2v_batch_finish_groups(b, fst.data(), ok.data(), nullptr, nullptr, groups));
        printf("finish ");
        for (int v : ok) printf("%d", v);
        for (int v : fst) printf(" %d", v);
        printf("\n");
    } catch (const Failure& f) {
        fprintf(stderr, "failure %d: %s\n", f.code, f.what());
        rc = 1;
    }
    for (void* p : dev) (void)hipFree(p);
    return rc;
}
