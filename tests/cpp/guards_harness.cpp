// C++ caller of the Guard entry points (include/h2v.hpp Accumulator::process_guards, check_guards -> h2v_accumulator_process_guards,
// h2v_guards_check_each): the trait seam, where a CPU verify_proof made the Guards.
//
//   guards_harness <dir> <cut>
// reads <dir>/params.bin, vk0.bin, rand.bin (n x 32), items.txt in the format of tests/cpp/multi_key.cpp ("1 n", then one line per
// proof, "0 <n_cols> <col_len>... <proof hex> <instance values hex, or ->") and guards.txt: one line per proof's Guard,
// "<left scalars hex> <left bases hex> <right scalars hex> <right bases hex>", "-" for an empty list.  It prints
//   mixed <ok 0/1> <left hex> <right hex> <n_proofs> <n_failed>   (proofs [0, cut) through process, Guards [cut, n) through process_guards)
//   guards <ok 0/1> <left hex> <right hex> <n_proofs> <n_failed>  (every Guard through process_guards, in the same two legs)
//   each <0/1>...                                                 (check_guards over all of them)
//   refused                                                       (a Guard with 33 scalar bytes, or one draw too few: no C call)
// tests/test_gpu_cpp_guards.py builds it over the library; tests/test_guards_host.py over the stand-in library, with sanitizers.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include "../../include/h2v.hpp"

using namespace halo2_verifier;

static Bytes slurp(const std::string& p) {
    std::ifstream f(p, std::ios::binary);
    if (!f) { fprintf(stderr, "cannot read %s\n", p.c_str()); exit(2); }
    return Bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static Bytes unhex(const std::string& h) {
    Bytes out;
    if (h == "-") return out;
    for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)std::stoul(h.substr(i, 2), nullptr, 16));
    return out;
}
static void hex(const uint8_t* b, size_t n) { for (size_t i = 0; i < n; ++i) printf("%02x", b[i]); }
static void report(const char* name, Accumulator& acc) {
    const bool ok = acc.finalize();
    acc.read();
    printf("%s %d ", name, ok ? 1 : 0); hex(acc.left(), 64); printf(" "); hex(acc.right(), 64); printf(" %zu %zu\n", acc.n_proofs(), acc.n_failed());
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: guards_harness <dir> <cut>\n"); return 2; }
    const std::string d = argv[1];
    const size_t cut = std::stoul(argv[2]);
    std::ifstream in(d + "/items.txt");
    size_t n_keys = 0, n = 0;
    if (!(in >> n_keys >> n) || n_keys != 1 || cut > n) return 2;
    std::vector<Accumulator::Item> items(n);
    for (Accumulator::Item& it : items) {
        size_t ncols = 0;
        in >> it.key >> ncols;
        std::vector<size_t> lens(ncols);
        for (size_t& l : lens) in >> l;
        std::string ph, ih;
        in >> ph >> ih;
        it.proof = unhex(ph);
        const Bytes flat = unhex(ih);
        size_t at = 0;
        for (size_t l : lens) {
            Column c;
            for (size_t j = 0; j < l; ++j, at += 32) c.emplace_back(flat.begin() + at, flat.begin() + at + 32);
            it.instances.push_back(c);
        }
    }
    std::ifstream gin(d + "/guards.txt");
    std::vector<Guard> guards(n);
    for (Guard& g : guards) {
        std::string a, b, c, e;
        if (!(gin >> a >> b >> c >> e)) return 2;
        g.left_scalars = unhex(a); g.left_bases = unhex(b); g.right_scalars = unhex(c); g.right_bases = unhex(e);
    }
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
