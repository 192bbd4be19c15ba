// C++ caller of the feed of a finished staged batch to a resident accumulator (include/h2v.hpp Accumulator::process_batch).
//
//   batch_legs_harness <dir> <sizes>
// reads <dir>/params.bin, vk0.bin, rand.bin (n x 32) and the keyed items.txt of one key (tests/cpp/caller.h: "1 n", then a line per
// proof), all of one instance shape; <sizes> are the group sizes, comma-separated, summing to n.  The proofs go through
// one staged launch of those groups without a pairing (the C ABI's h2v_batch_*), and the finished batch is fed to a journaled
// accumulator; a second accumulator is given the same proofs by one process call per group.  It prints
//   added <n_proofs> <n_failed> <all_ok 0/1>
//   batch <ok 0/1> <left hex> <right hex> <n_proofs> <n_failed>      (finalize + read of the batch-fed accumulator)
//   leg <e> <n_proofs> <n_failed> <pairing_ok 0/1>                    (its check_legs, the base first)
//   process <ok 0/1> <left hex> <right hex> <n_proofs> <n_failed>    (the accumulator fed by process, group by group)
//   again <n_proofs> <n_failed>                                       (the same batch fed a second time: the counters afterwards)
//   refused <what>                                                    (what the mirror refuses before any C call: a null batch)
// tests/test_gpu_cpp_batch_legs.py builds it with g++ over the library and compares the lines with the Python class and the CPU oracle;
// tests/test_accumulator_batch_host.py builds it with the address and undefined-behaviour sanitizers over the stand-in library.
#include <sstream>
#include "caller.h"

using namespace caller;

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: batch_legs_harness <dir> <sizes>\n"); return 2; }
    const std::string d = argv[1];
    std::vector<size_t> sizes;
    {
        std::stringstream ss(argv[2]);
        for (std::string tok; std::getline(ss, tok, ',');) sizes.push_back(std::stoul(tok));
    }
    const Items in = read_items(d, true);
    const size_t n = in.items.size();
    size_t total = 0;
    for (size_t v : sizes) total += v;
    if (in.n_keys != 1 || sizes.empty() || total != n || !n) return 2;
    const std::vector<Accumulator::Item> items = accumulator_items(in.items);
    // a staged launch holds one shape: proofs of one length, instance columns of the same lengths
    std::vector<size_t> col_lens;
    for (const Column& c : items[0].instances) col_lens.push_back(c.size());
    const size_t proof_len = items[0].proof.size();
    Bytes proofs_flat, inst_flat;
    for (const Accumulator::Item& it : items) {
        if (it.instances.size() != col_lens.size() || it.proof.size() != proof_len) return 2;
        for (size_t c = 0; c < col_lens.size(); ++c) {
            if (it.instances[c].size() != col_lens[c]) return 2;
            for (const Bytes& v : it.instances[c]) inst_flat.insert(inst_flat.end(), v.begin(), v.end());
        }
        proofs_flat.insert(proofs_flat.end(), it.proof.begin(), it.proof.end());
    }
    try {
        ParamsKZG params{slurp(d + "/params.bin"), SerdeFormat::RawBytes};
        Context ctx(params, VerifyingKey{slurp(d + "/vk0.bin"), SerdeFormat::RawBytes});
        const Bytes rand = slurp(d + "/rand.bin");
        if (rand.size() != 32 * n) return 2;
        size_t n_inst = 0;
        for (size_t l : col_lens) n_inst += l;
        // the staged launch: groups of the given sizes, no pairing of its own
        BatchHolder bh;
        check(h2v_batch_create(ctx.handle(), n, n_inst, &bh.b));
        set_group_sizes(bh.b, sizes);
        check(h2v_batch_upload(bh.b, n, proofs_flat.data(), proof_len, inst_flat.data(), col_lens.size(), col_lens.data(), rand.data(), n));
        check(h2v_batch_launch(bh.b, 0));
        const size_t G = sizes.size();
        std::vector<int> st(n), group_ok(G);
        Bytes lefts(64 * G), rights(64 * G);
        check(h2v_batch_finish_groups(bh.b, st.data(), group_ok.data(), lefts.data(), rights.data(), G));
        // the feed
        Accumulator fed(ctx), ref(ctx);
        fed.journal_begin(2 * G + 1);
        const Accumulator::Added added = fed.process_batch(bh.b);
        printf("added %zu %zu %d\n", added.n_proofs, added.n_failed, fed.all_ok() ? 1 : 0);
        report("batch", fed);
        const std::vector<Accumulator::Leg> legs = fed.check_legs();
        for (size_t e = 0; e < legs.size(); ++e) printf("leg %zu %zu %zu %d\n", e, legs[e].n_proofs, legs[e].n_failed, legs[e].pairing_ok ? 1 : 0);
        // process, group by group
        for (size_t g = 0, at = 0; g < G; at += sizes[g], ++g) {
            const std::vector<Accumulator::Item> mine(items.begin() + at, items.begin() + at + sizes[g]);
            ref.process({&ctx}, mine, Bytes(rand.begin() + 32 * at, rand.begin() + 32 * (at + sizes[g])));
        }
        report("process", ref);
        // the batch is only read: it feeds a second time
        fed.process_batch(bh.b);
        fed.read();
        printf("again %zu %zu\n", fed.n_proofs(), fed.n_failed());
        refused("a null batch", [&] { fed.process_batch(nullptr); });
    } catch (const Failure& f) {
        fprintf(stderr, "failure %d: %s\n", f.code, f.what());
        return 1;
    }
    return 0;
}
