// C++ caller of the calls that take a hint row per proof, or none (include/h2v_hints.hpp -> include/h2v_hint_rows.h), beside the same
// calls without hints (include/h2v.hpp).
//
//   hinted_calls <dir>
// reads <dir>/params.bin, vk<k>.bin (k < n_keys), rand.bin (n x 32) and the keyed items.txt (tests/cpp/caller.h).  The rows are made
// here, on the host (hints::for_proofs over the key's point_offsets), for every proof but each third one, which goes without.  Prints
//   keys <ok 0/1> <left hex> <right hex> <status...>            AccumulatorStrategy::finalize over all items (h2v_verify_batch_keys)
//   keys_hinted <the same words>                                 hints::verify_batch_keys
//   process <ok> <left> <right> <n_proofs> <n_failed>            Accumulator::process in two calls, finalize, read
//   process_hinted <the same words>                              hints::process in the same two calls
//   batches <ok...> <status...> <left...> <right...>             verify_batches over key 0's items as batches of 1 and the rest
//   batches_hinted <the same words>                              hints::verify_batches
//   stats <call> <points> <hinted> <missed>                      the counters of each hinted call
//   staged_stats <points> <hinted> <missed>                      a staged batch of key 0's items under hints::set_rows
//   refused <what>                                               what the mirror refuses before any C call
// tests/test_gpu_cpp_hinted_calls.py builds it with g++ and compares each hinted line with the line without hints.
#include "caller.h"
#include "../../include/h2v_hints.hpp"

using namespace caller;

static void keys_line(const char* tag, bool ok, const uint8_t* left, const uint8_t* right, const std::vector<int>& st) {
    verdict(tag, ok, left, right);
    for (int s : st) printf(" %d", s);
    printf("\n");
}
static void batches_line(const char* tag, const std::vector<int>& ok, const std::vector<int>& st, const Bytes& left, const Bytes& right) {
    group_results(tag, ok, st, left, right);
    printf("\n");
}
static void stats_line(const char* call, const hints::Stats& s) { printf("stats %s %zu %zu %zu\n", call, s.points, s.hinted, s.missed); }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: hinted_calls <dir>\n"); return 2; }
    const std::string d = argv[1];
    const Items in = read_items(d, true);
    try {
        ParamsKZG params{slurp(d + "/params.bin"), SerdeFormat::RawBytes};
        const std::vector<VerifyingKey> vks = read_vks(d, in.n_keys);
        const Bytes rand = slurp(d + "/rand.bin");
        const size_t n = in.items.size();
        if (rand.size() != 32 * n || n < 4) bad_input("rand.bin does not hold a draw per proof, or fewer than four proofs");
        Contexts ctxs(params, vks);
        std::vector<std::vector<size_t>> offsets;
        for (const Context* c : ctxs.handles) offsets.push_back(hints::point_offsets(c->handle()));
        std::vector<hints::Item> hinted;
        for (size_t i = 0; i < n; ++i) {
            const Item& it = in.items[i];
            hinted.push_back({(uint32_t)it.key, it.inst, it.proof, i % 3 == 2 ? Bytes() : hints::for_proofs(offsets[it.key], it.proof, it.proof.size())});
        }
        // 1. one AccumulatorStrategy over every item
        AccumulatorStrategy acc(params);
        acc.set_randomness(rand);
        for (const Item& it : in.items) verify_proof(params, vks[it.key], acc, it.inst, it.proof);
        const bool ok = acc.finalize();
        keys_line("keys", ok, acc.left(), acc.right(), acc.statuses());
        const hints::Result r = hints::verify_batch_keys(ctxs.handles, hinted, rand);
        keys_line("keys_hinted", r.ok, r.left.data(), r.right.data(), r.statuses);
        stats_line("keys", r.stats);
        // 2. the resident accumulator, in two calls
        const size_t half = n / 2;
        const Bytes rand_a(rand.begin(), rand.begin() + 32 * half), rand_b(rand.begin() + 32 * half, rand.end());
        {
            const std::vector<Accumulator::Item> all = accumulator_items(in.items);
            Accumulator plain(*ctxs.handles[0]);
            plain.process(ctxs.handles, std::vector<Accumulator::Item>(all.begin(), all.begin() + half), rand_a);
            plain.process(ctxs.handles, std::vector<Accumulator::Item>(all.begin() + half, all.end()), rand_b);
            report("process", plain);
            Accumulator with(*ctxs.handles[0]);
            hints::Stats sa, sb;
            hints::process(with, ctxs.handles, std::vector<hints::Item>(hinted.begin(), hinted.begin() + half), rand_a, &sa);
            hints::process(with, ctxs.handles, std::vector<hints::Item>(hinted.begin() + half, hinted.end()), rand_b, &sb);
            report("process_hinted", with);
            sa.points += sb.points; sa.hinted += sb.hinted; sa.missed += sb.missed;
            stats_line("process", sa);
        }
        // 3. key 0's items as batches of 1 and the rest
        std::vector<BatchItem> mine;
        std::vector<hints::Item> mine_hinted;
        Bytes mine_rand;
        for (size_t i = 0; i < n; ++i)
            if (in.items[i].key == 0) {
                mine.push_back({in.items[i].inst, in.items[i].proof});
                mine_hinted.push_back(hinted[i]);
                mine_rand.insert(mine_rand.end(), rand.begin() + 32 * i, rand.begin() + 32 * i + 32);
            }
        if (mine.size() < 2) bad_input("fewer than two proofs of key 0");
        auto flat = [](const auto& results, std::vector<int>& oks, std::vector<int>& st, Bytes& left, Bytes& right) {
            for (const auto& res : results) {
                oks.push_back(res.ok ? 1 : 0);
                st.insert(st.end(), res.statuses.begin(), res.statuses.end());
                left.insert(left.end(), res.left.begin(), res.left.end());
                right.insert(right.end(), res.right.begin(), res.right.end());
            }
        };
        {
            std::vector<int> oks, st; Bytes left, right;
            flat(verify_batches(*ctxs.handles[0], {{mine[0]}, std::vector<BatchItem>(mine.begin() + 1, mine.end())}, mine_rand), oks, st, left, right);
            batches_line("batches", oks, st, left, right);
        }
        {
            std::vector<int> oks, st; Bytes left, right;
            hints::Stats s;
            flat(hints::verify_batches(*ctxs.handles[0], {{mine_hinted[0]}, std::vector<hints::Item>(mine_hinted.begin() + 1, mine_hinted.end())}, mine_rand, &s), oks, st,
                 left, right);
            batches_line("batches_hinted", oks, st, left, right);
            stats_line("batches", s);
        }
        // 4. a staged batch of key 0's items (one instance column) under a row per proof
        {
            Bytes proofs, inst;
            std::vector<Bytes> rows;
            size_t values = 0;
            for (const hints::Item& it : mine_hinted) {
                proofs.insert(proofs.end(), it.proof.begin(), it.proof.end());
                if (it.instances.size() != 1) bad_input("key 0 has more than one instance column");
                values = it.instances[0].size();
                for (const Bytes& v : it.instances[0]) inst.insert(inst.end(), v.begin(), v.end());
                rows.push_back(it.row);
            }
            BatchHolder batch;
            stage(batch, *ctxs.handles[0], mine.size(), 1, mine[0].proof.size(), values, Staged{proofs, inst, mine_rand});
            hints::set_rows(batch.b, rows, offsets[0].size());
            check(h2v_batch_launch(batch.b, 1));
            std::vector<int> st(mine.size(), 0); int batch_ok = 0; uint8_t left[64], right[64];
            check(h2v_batch_finish(batch.b, st.data(), &batch_ok, left, right));
            const hints::Stats s = hints::stats(batch.b);
            printf("staged_stats %zu %zu %zu\n", s.points, s.hinted, s.missed);
        }
        // 5. the mirror's own refusals: a row of another length
        std::vector<hints::Item> wrong = hinted;
        wrong[0].row.push_back(0);
        refused("a row one byte too long", [&] { hints::verify_batch_keys(ctxs.handles, wrong, rand); });
        refused("a draw too few", [&] { hints::verify_batch_keys(ctxs.handles, hinted, Bytes(rand.begin(), rand.end() - 32)); });
    } catch (const Failure& f) {
        fprintf(stderr, "failure %d: %s\n", f.code, f.what());
        return 1;
    }
    return 0;
}
