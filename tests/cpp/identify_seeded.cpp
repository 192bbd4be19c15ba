// C++ caller of a SEEDED AccumulatorStrategy's finalize_identify() (include/h2v.hpp -> h2v_verify_batch_seeded_identify).
//
//   identify_seeded <dir>
// reads <dir>/params.bin, vk.bin, rand.bin (n x 32), seed.bin (left x|y, right x|y: 128 bytes, the evaluated channels of the
// accumulation to resume) and the unkeyed items.txt (tests/cpp/caller.h), resumes the accumulation (AccumulatorStrategy::with, scalar 1
// on either channel), queues the proofs and prints
//   identify <ok 0/1> <left hex> <right hex> <status...>
//   seed_ok <0/1>
//   range_checks <count>
//   plain <ok 0/1> <left hex> <right hex>        (finalize() on the same accumulation)
// tests/test_gpu_cpp_identify_seeded.py builds it with g++ and compares the lines with the CPU oracle.
#include "caller.h"

using namespace caller;

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: identify_seeded <dir>\n"); return 2; }
    const std::string d = argv[1];
    const Items in = read_items(d, false);
    try {
        ParamsKZG params{slurp(d + "/params.bin"), SerdeFormat::RawBytes};
        VerifyingKey vk{slurp(d + "/vk.bin"), SerdeFormat::RawBytes};
        const Bytes rand = slurp(d + "/rand.bin"), seed = slurp(d + "/seed.bin");
        if (seed.size() != 128) { fprintf(stderr, "seed.bin is two 64-byte points\n"); return 2; }
        Bytes one(32, 0);
        one[0] = 1;
        // let mut s = AccumulatorStrategy::with(&params, msm_accumulator); for each proof { s = verify_proof(&params, &vk, s, ..)? }
        AccumulatorStrategy acc = AccumulatorStrategy::with(params, one, Bytes(seed.begin(), seed.begin() + 64), one, Bytes(seed.begin() + 64, seed.end()));
        acc.set_randomness(rand);
        for (const Item& it : in.items) verify_proof(params, vk, acc, it.inst, it.proof);
        const bool ok = acc.finalize_identify();
        verdict("identify", ok, acc.left(), acc.right());
        for (int s : acc.statuses()) printf(" %d", s);
        printf("\n");
        printf("seed_ok %d\n", acc.seed_ok() ? 1 : 0);
        printf("range_checks %zu\n", acc.range_checks());
        const bool plain = acc.finalize();
        verdict("plain", plain, acc.left(), acc.right());
        printf("\n");
    } catch (const Failure& f) {
        fprintf(stderr, "failure %d: %s\n", f.code, f.what());
        return 1;
    }
    return 0;
}
