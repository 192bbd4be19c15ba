// C++ caller of the merge of resident accumulators (include/h2v.hpp Accumulator::merge / export_state / merge_states).
//
//   merge_harness <dir> <n_sources>
// reads <dir>/params.bin, vk0.bin, rand.bin (n x 32), draws.bin (n_sources x 32) and the keyed items.txt of one key (tests/cpp/caller.h:
// "1 n", then a line per proof).  Proof i is fed to source i % n_sources, each source in one process call with the draws of its
// proofs; a journaled destination merges the sources with the draws of draws.bin, a second one
// merges their exported states with the same draws, a third with draws of the library's own.  It prints
//   state <k> <hex of the 152 bytes>                         (export_state() of every source)
//   merge <ok 0/1> <left hex> <right hex> <n_proofs> <n_failed> <entries> <draws used hex>
//   states <the same for merge_states>
//   drawn <ok 0/1> <n_proofs> <draws used hex>                (merge with OS draws)
//   refused <what>                                           (what the mirror refuses before any C call: too many sources, draws of a
//                                                             wrong length, states of a wrong length, the destination as a source)
// tests/test_gpu_cpp_merge.py builds it with g++ over the library and compares the lines with the Python class and the CPU oracle;
// tests/test_accumulator_merge_host.py builds it with the address and undefined-behaviour sanitizers over the stand-in library.
#include "caller.h"

using namespace caller;

static void report(const char* what, Accumulator& acc, const Bytes& used) {
    const bool ok = acc.finalize();
    acc.read();
    const size_t entries = acc.check_legs().size();
    verdict(what, ok, acc.left(), acc.right());
    printf(" %zu %zu %zu ", acc.n_proofs(), acc.n_failed(), entries); hex(used); printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: merge_harness <dir> <n_sources>\n"); return 2; }
    const std::string d = argv[1];
    const size_t K = std::stoul(argv[2]);
    const Items in = read_items(d, true);
    const size_t n = in.items.size();
    if (in.n_keys != 1 || K < 1 || K > 16) return 2;
    const std::vector<Accumulator::Item> items = accumulator_items(in.items);
    try {
        ParamsKZG params{slurp(d + "/params.bin"), SerdeFormat::RawBytes};
        Context ctx(params, VerifyingKey{slurp(d + "/vk0.bin"), SerdeFormat::RawBytes});
        const Bytes rand = slurp(d + "/rand.bin"), draws = slurp(d + "/draws.bin");
        if (rand.size() != 32 * n || draws.size() != 32 * K) return 2;
        std::vector<std::unique_ptr<Accumulator>> srcs;
        std::vector<Accumulator*> handles;
        Bytes states;
        for (size_t k = 0; k < K; ++k) {
            srcs.emplace_back(new Accumulator(ctx));
            std::vector<Accumulator::Item> mine;
            Bytes r;
            for (size_t i = k; i < n; i += K) { mine.push_back(items[i]); r.insert(r.end(), rand.begin() + 32 * i, rand.begin() + 32 * i + 32); }
            srcs.back()->process({&ctx}, mine, r);
            handles.push_back(srcs.back().get());
            const Bytes st = srcs.back()->export_state();
            printf("state %zu ", k); hex(st); printf("\n");
            states.insert(states.end(), st.begin(), st.end());
        }
        Accumulator a(ctx), b(ctx), c(ctx);
        a.journal_begin(K + 1);
        b.journal_begin(K + 1);
        report("merge", a, a.merge(handles, draws));
        report("states", b, b.merge_states(states, draws));
        const Bytes used = c.merge(handles);
        const bool ok = c.finalize();
        c.read();
        printf("drawn %d %zu ", ok ? 1 : 0, c.n_proofs()); hex(used); printf("\n");
        refused("too many sources", [&] { c.merge(std::vector<Accumulator*>(H2V_ACC_MERGE_MAX + 1, handles[0]), Bytes()); });
        refused("draws of a wrong length", [&] { c.merge(handles, Bytes(32 * K + 1)); });
        refused("states of a wrong length", [&] { c.merge_states(Bytes(states.begin(), states.end() - 1)); });
        refused("too many states", [&] { c.merge_states(Bytes((size_t)H2V_ACC_STATE_BYTES * (H2V_ACC_MERGE_MAX + 1))); });
        refused("the destination as a source", [&] { c.merge({&c}); });
        refused("a null source", [&] { c.merge({nullptr}); });
    } catch (const Failure& f) {
        fprintf(stderr, "failure %d: %s\n", f.code, f.what());
        return 1;
    }
    return 0;
}
