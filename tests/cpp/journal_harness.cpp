// C++ caller of the resident accumulator's leg journal (include/h2v.hpp Accumulator::journal_begin / check_legs / drop_legs) over proofs
// of several VerifyingKeys.
//
//   journal_harness <dir> <cut1> <cut2>
// reads <dir>/params.bin, vk<k>.bin (k < n_keys), rand.bin (n x 32) and the keyed items.txt (tests/cpp/caller.h).  The proofs are fed to
// a journaled accumulator in three legs, [0, cut1), [cut1, cut2) and [cut2, n), every leg given every context; the legs whose own
// pairing fails are dropped, and it prints
//   leg <entry> <n_proofs> <n_failed> <pairing ok 0/1>        (check_legs() after the third leg, the base first)
//   before <ok 0/1> <left hex> <right hex>                    (finalize() with every leg in)
//   dropped <entry>...                                        (the entries handed to drop_legs())
//   after <ok 0/1> <left hex> <right hex> <n_proofs> <n_failed> <entries>    (finalize(), read() and check_legs().size() afterwards)
// tests/test_gpu_cpp_journal.py builds it with g++ and compares the lines with the Python class and the CPU oracle.
#include "caller.h"

using namespace caller;

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: journal_harness <dir> <cut1> <cut2>\n"); return 2; }
    const std::string d = argv[1];
    const Items in = read_items(d, true);
    const size_t n = in.items.size();
    const size_t bounds[4] = {0, std::stoul(argv[2]), std::stoul(argv[3]), n};
    if (bounds[1] > bounds[2] || bounds[2] > n) return 2;
    const std::vector<Accumulator::Item> items = accumulator_items(in.items);
    try {
        ParamsKZG params{slurp(d + "/params.bin"), SerdeFormat::RawBytes};
        const Contexts ctxs(params, read_vks(d, in.n_keys));
        const Bytes rand = slurp(d + "/rand.bin");
        Accumulator acc(*ctxs.owned[0]);
        acc.journal_begin(4);
        for (int leg = 0; leg < 3; ++leg)
            acc.process(ctxs.handles, std::vector<Accumulator::Item>(items.begin() + bounds[leg], items.begin() + bounds[leg + 1]),
                        Bytes(rand.begin() + 32 * bounds[leg], rand.begin() + 32 * bounds[leg + 1]));
        const std::vector<Accumulator::Leg> legs = acc.check_legs();
        std::vector<size_t> failing;
        for (size_t e = 0; e < legs.size(); ++e) {
            printf("leg %zu %zu %zu %d\n", e, legs[e].n_proofs, legs[e].n_failed, legs[e].pairing_ok ? 1 : 0);
            if (e && !legs[e].pairing_ok) failing.push_back(e);
        }
        bool ok = acc.finalize();
        verdict("before", ok, acc.left(), acc.right());
        printf("\n");
        acc.drop_legs(failing);
        printf("dropped");
        for (size_t e : failing) printf(" %zu", e);
        printf("\n");
        ok = acc.finalize();
        acc.read();
        verdict("after", ok, acc.left(), acc.right());
        printf(" %zu %zu %zu\n", acc.n_proofs(), acc.n_failed(), acc.check_legs().size());
    } catch (const Failure& f) {
        fprintf(stderr, "failure %d: %s\n", f.code, f.what());
        return 1;
    }
    return 0;
}
