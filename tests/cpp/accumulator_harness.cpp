// C++ caller of the resident accumulator (include/h2v.hpp Accumulator -> h2v_accumulator_*) over proofs of several VerifyingKeys.
//
//   accumulator_harness <dir> <cut>
// reads <dir>/params.bin, vk<k>.bin (k < n_keys), rand.bin (n x 32) and the keyed items.txt (tests/cpp/caller.h).  The proofs are fed in
// two legs, [0, cut) and [cut, n), every leg given every context, and it prints
//   first <left hex> <right hex> <n_proofs> <n_failed>        (read() after the first leg)
//   acc <ok 0/1> <left hex> <right hex> <status...>           (finalize() after the second)
//   again <ok 0/1>                                            (finalize() once more: the accumulator is not consumed)
// tests/test_gpu_cpp_accumulator.py builds it with g++ and compares the lines with the Python class and the CPU oracle.
#include "caller.h"

using namespace caller;

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: accumulator_harness <dir> <cut>\n"); return 2; }
    const std::string d = argv[1];
    const size_t cut = std::stoul(argv[2]);
    const Items in = read_items(d, true);
    if (cut > in.items.size()) return 2;
    const std::vector<Accumulator::Item> items = accumulator_items(in.items);
    try {
        ParamsKZG params{slurp(d + "/params.bin"), SerdeFormat::RawBytes};
        const Contexts ctxs(params, read_vks(d, in.n_keys));
        const Bytes rand = slurp(d + "/rand.bin");
        // let mut s = AccumulatorStrategy::new(&params); for each proof as it arrives { s = verify_proof(&params, &vk_i, s, ..)? } s.finalize()
        Accumulator acc(*ctxs.owned[0]);
        std::vector<int> st = acc.process(ctxs.handles, std::vector<Accumulator::Item>(items.begin(), items.begin() + cut), Bytes(rand.begin(), rand.begin() + 32 * cut));
        acc.read();
        printf("first "); hex(acc.left(), 64); printf(" "); hex(acc.right(), 64); printf(" %zu %zu\n", acc.n_proofs(), acc.n_failed());
        const std::vector<int> st2 = acc.process(ctxs.handles, std::vector<Accumulator::Item>(items.begin() + cut, items.end()), Bytes(rand.begin() + 32 * cut, rand.end()));
        st.insert(st.end(), st2.begin(), st2.end());
        const bool ok = acc.finalize();
        verdict("acc", ok, acc.left(), acc.right());
        for (int s : st) printf(" %d", s);
        printf("\n");
        printf("again %d\n", acc.finalize() ? 1 : 0);
    } catch (const Failure& f) {
        fprintf(stderr, "failure %d: %s\n", f.code, f.what());
        return 1;
    }
    return 0;
}
