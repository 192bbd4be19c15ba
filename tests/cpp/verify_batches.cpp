// C++ caller of many AccumulatorStrategy batches of their own sizes in one call (include/h2v.hpp verify_batches -> h2v_verify_batches).
//
//   verify_batches <dir>
// reads <dir>/params.bin, vk.bin, rand.bin (n x 32) and an items.txt with a header of its own: "n_batches", the batch sizes, then one
// unkeyed line per proof in call order (tests/cpp/caller.h read_item), and prints per batch
//   batch <ok 0/1> <left hex> <right hex> <status...>
// then "empty_refused <code>" for a call with a batch of no proofs.  tests/test_gpu_verify_batches.py builds it with g++.
#include "caller.h"

using namespace caller;

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: verify_batches <dir>\n"); return 2; }
    const std::string d = argv[1];
    std::ifstream in(d + "/items.txt");
    size_t k = 0;
    if (!(in >> k)) bad_input("items.txt: no header");
    std::vector<size_t> sizes;
    for (size_t g = 0, sz = 0; g < k; ++g) {
        if (!(in >> sz)) bad_input("items.txt: fewer batch sizes than batches");
        sizes.push_back(sz);
    }
    std::vector<std::vector<BatchItem>> batches;
    for (size_t sz : sizes) {
        batches.emplace_back();
        for (size_t i = 0; i < sz; ++i) {
            Item it = read_item(in, false);
            batches.back().push_back({it.inst, it.proof});
        }
    }
    try {
        ParamsKZG params{slurp(d + "/params.bin"), SerdeFormat::RawBytes};
        VerifyingKey vk{slurp(d + "/vk.bin"), SerdeFormat::RawBytes};
        Context ctx(params, vk);
        for (const BatchResult& r : verify_batches(ctx, batches, slurp(d + "/rand.bin"))) {
            printf("batch %d ", r.ok ? 1 : 0); hex(r.left); printf(" "); hex(r.right);
            for (int s : r.statuses) printf(" %d", s);
            printf("\n");
        }
        batches.push_back({});
        try { verify_batches(ctx, batches); printf("empty_refused 0\n"); } catch (const Failure& f) { printf("empty_refused %d\n", f.code); }
    } catch (const Failure& f) {
        fprintf(stderr, "failure %d: %s\n", f.code, f.what());
        return 1;
    }
    return 0;
}
