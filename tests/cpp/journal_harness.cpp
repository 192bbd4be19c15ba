// C++ caller of the resident accumulator's leg journal (include/h2v.hpp Accumulator::journal_begin / check_legs / drop_legs) over proofs
// of several VerifyingKeys.
//
//   journal_harness <dir> <cut1> <cut2>
// reads <dir>/params.bin, vk<k>.bin (k < n_keys), rand.bin (n x 32) and items.txt in the format of tests/cpp/multi_key.cpp: "n_keys n",
// then one line per proof in call order, "<key> <n_cols> <col_len>... <proof hex> <instance values hex, or ->".  The proofs are fed to
// a journaled accumulator in three legs, [0, cut1), [cut1, cut2) and [cut2, n), every leg given every context; the legs whose own
// pairing fails are dropped, and it prints
//   leg <entry> <n_proofs> <n_failed> <pairing ok 0/1>        (check_legs() after the third leg, the base first)
//   before <ok 0/1> <left hex> <right hex>                    (finalize() with every leg in)
//   dropped <entry>...                                        (the entries handed to drop_legs())
//   after <ok 0/1> <left hex> <right hex> <n_proofs> <n_failed> <entries>    (finalize(), read() and check_legs().size() afterwards)
// tests/test_gpu_cpp_journal.py builds it with g++ and compares the lines with the Python class and the CPU oracle.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>
#include <memory>
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

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: journal_harness <dir> <cut1> <cut2>\n"); return 2; }
    const std::string d = argv[1];
    std::ifstream in(d + "/items.txt");
    size_t n_keys = 0, n = 0;
    if (!(in >> n_keys >> n)) return 2;
    const size_t bounds[4] = {0, std::stoul(argv[2]), std::stoul(argv[3]), n};
    if (bounds[1] > bounds[2] || bounds[2] > n) return 2;
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
    try {
        ParamsKZG params{slurp(d + "/params.bin"), SerdeFormat::RawBytes};
        std::vector<std::unique_ptr<Context>> ctxs;
        std::vector<const Context*> handles;
        for (size_t k = 0; k < n_keys; ++k) {
            ctxs.emplace_back(new Context(params, VerifyingKey{slurp(d + "/vk" + std::to_string(k) + ".bin"), SerdeFormat::RawBytes}));
            handles.push_back(ctxs.back().get());
        }
        const Bytes rand = slurp(d + "/rand.bin");
        Accumulator acc(*ctxs[0]);
        acc.journal_begin(4);
        for (int leg = 0; leg < 3; ++leg)
            acc.process(handles, std::vector<Accumulator::Item>(items.begin() + bounds[leg], items.begin() + bounds[leg + 1]),
                        Bytes(rand.begin() + 32 * bounds[leg], rand.begin() + 32 * bounds[leg + 1]));
        const std::vector<Accumulator::Leg> legs = acc.check_legs();
        std::vector<size_t> failing;
        for (size_t e = 0; e < legs.size(); ++e) {
            printf("leg %zu %zu %zu %d\n", e, legs[e].n_proofs, legs[e].n_failed, legs[e].pairing_ok ? 1 : 0);
            if (e && !legs[e].pairing_ok) failing.push_back(e);
        }
        bool ok = acc.finalize();
        printf("before %d ", ok ? 1 : 0); hex(acc.left(), 64); printf(" "); hex(acc.right(), 64); printf("\n");
        acc.drop_legs(failing);
        printf("dropped");
        for (size_t e : failing) printf(" %zu", e);
        printf("\n");
        ok = acc.finalize();
        acc.read();
        printf("after %d ", ok ? 1 : 0); hex(acc.left(), 64); printf(" "); hex(acc.right(), 64);
        printf(" %zu %zu %zu\n", acc.n_proofs(), acc.n_failed(), acc.check_legs().size());
    } catch (const Failure& f) {
        fprintf(stderr, "failure %d: %s\n", f.code, f.what());
        return 1;
    }
    return 0;
}
