// C++ caller of one AccumulatorStrategy over proofs of several VerifyingKeys (include/h2v.hpp -> h2v_verify_batch_keys).
//
//   multi_key <dir>
// reads <dir>/params.bin, vk<k>.bin (k < n_keys), rand.bin (n x 32) and the keyed items.txt (tests/cpp/caller.h), and prints
//   multi <ok 0/1> <left hex> <right hex> <status...>
//   identify_refused <code>      (finalize_identify over several VKs)
//   seeded_refused <code>        (AccumulatorStrategy::with over several VKs)
// tests/test_gpu_cpp_multi_key.py builds it with g++ and compares the lines with the CPU oracle.
#include "caller.h"

using namespace caller;

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: multi_key <dir>\n"); return 2; }
    const std::string d = argv[1];
    const Items in = read_items(d, true);
    try {
        ParamsKZG params{slurp(d + "/params.bin"), SerdeFormat::RawBytes};
        const std::vector<VerifyingKey> vks = read_vks(d, in.n_keys);
        const Bytes rand = slurp(d + "/rand.bin");
        // let mut s = AccumulatorStrategy::new(&params); for each proof { s = verify_proof(&params, &vk_i, s, ..)? } s.finalize()
        AccumulatorStrategy acc(params);
        acc.set_randomness(rand);
        for (const Item& it : in.items) verify_proof(params, vks[it.key], acc, it.inst, it.proof);
        const bool ok = acc.finalize();
        verdict("multi", ok, acc.left(), acc.right());
        for (int s : acc.statuses()) printf(" %d", s);
        printf("\n");
        try { acc.finalize_identify(); printf("identify_refused 0\n"); } catch (const Failure& f) { printf("identify_refused %d\n", f.code); }
        Bytes one(32, 0); one[0] = 1;
        Bytes left(acc.left(), acc.left() + 64), right(acc.right(), acc.right() + 64);
        AccumulatorStrategy seeded = AccumulatorStrategy::with(params, one, left, one, right);
        seeded.set_randomness(rand);
        for (const Item& it : in.items) verify_proof(params, vks[it.key], seeded, it.inst, it.proof);
        try { seeded.finalize(); printf("seeded_refused 0\n"); } catch (const Failure& f) { printf("seeded_refused %d\n", f.code); }
    } catch (const Failure& f) {
        fprintf(stderr, "failure %d: %s\n", f.code, f.what());
        return 1;
    }
    return 0;
}
