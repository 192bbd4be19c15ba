// C++ caller of the Guard entry points (include/h2v.hpp Accumulator::process_guards, check_guards -> h2v_accumulator_process_guards,
// h2v_guards_check_each): the trait seam, where a CPU verify_proof made the Guards.
//
//   guards_harness <dir> <cut>
// reads <dir>/params.bin, vk0.bin, rand.bin (n x 32), the keyed items.txt of one key and guards.txt with one Guard per proof
// (tests/cpp/caller.h).  It prints
//   mixed <ok 0/1> <left hex> <right hex> <n_proofs> <n_failed>   (proofs [0, cut) through process, Guards [cut, n) through process_guards)
//   guards <ok 0/1> <left hex> <right hex> <n_proofs> <n_failed>  (every Guard through process_guards, in the same two legs)
//   each <0/1>...                                                 (check_guards over all of them)
//   refused                                                       (a Guard with 33 scalar bytes, or one draw too few: no C call)
// tests/test_gpu_cpp_guards.py builds it over the library; tests/test_guards_host.py over the stand-in library, with sanitizers.
#include "caller.h"

using namespace caller;

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: guards_harness <dir> <cut>\n"); return 2; }
    const std::string d = argv[1];
    const size_t cut = std::stoul(argv[2]);
    const Items in = read_items(d, true);
    const size_t n = in.items.size();
    if (in.n_keys != 1 || cut > n) return 2;
    const std::vector<Accumulator::Item> items = accumulator_items(in.items);
    const std::vector<Guard> guards = read_guards(d);
    if (guards.size() != n) bad_input("guards.txt: not one Guard per proof");
    try {
        ParamsKZG params{slurp(d + "/params.bin"), SerdeFormat::RawBytes};
        Context ctx(params, VerifyingKey{slurp(d + "/vk0.bin"), SerdeFormat::RawBytes});
        const Bytes rand = slurp(d + "/rand.bin");
        const Bytes r0(rand.begin(), rand.begin() + 32 * cut), r1(rand.begin() + 32 * cut, rand.end());
        const std::vector<Guard> g0(guards.begin(), guards.begin() + cut), g1(guards.begin() + cut, guards.end());
        {
            // let mut s = AccumulatorStrategy::new(&params); s = verify_proof(.., s, ..)? on the GPU for the first proofs, on the CPU for the rest
            Accumulator acc(ctx);
            acc.process({&ctx}, std::vector<Accumulator::Item>(items.begin(), items.begin() + cut), r0);
            acc.process_guards(g1, r1);
            report("mixed", acc);
        }
        {
            Accumulator acc(ctx);
            acc.process_guards(g0, r0);
            acc.process_guards(g1, r1);
            report("guards", acc);
            // what the mirror refuses before any C call
            int refused = 0;
            std::vector<Guard> bad = g1;
            if (!bad.empty()) {
                bad[0].right_scalars.push_back(0);
                try { acc.process_guards(bad, r1); } catch (const Failure& f) { refused += f.code == H2V_ERR_BAD_ARGUMENT; }
                try { check_guards(ctx, bad); } catch (const Failure& f) { refused += f.code == H2V_ERR_BAD_ARGUMENT; }
                try { acc.process_guards(g1, Bytes(r1.begin(), r1.end() - 32)); } catch (const Failure& f) { refused += f.code == H2V_ERR_BAD_ARGUMENT; }
                if (refused == 3) printf("refused\n");
            }
        }
        const std::vector<bool> each = check_guards(ctx, guards);
        printf("each");
        for (bool ok : each) printf(" %d", ok ? 1 : 0);
        printf("\n");
    } catch (const Failure& f) {
        fprintf(stderr, "failure %d: %s\n", f.code, f.what());
        return 1;
    }
    return 0;
}
