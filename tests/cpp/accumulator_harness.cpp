// C++ caller of the resident accumulator (include/h2v.hpp Accumulator -> h2v_accumulator_*) over proofs of several VerifyingKeys.
//
//   accumulator_harness <dir> <cut>
// reads <dir>/params.bin, vk<k>.bin (k < n_keys), rand.bin (n x 32) and items.txt in the format of tests/cpp/multi_key.cpp: "n_keys n",
// then one line per proof in call order, "<key> <n_cols> <col_len>... <proof hex> <instance values hex, or ->".  The proofs are fed in
// two legs, [0, cut) and [cut, n), every leg given every context, and it prints
//   first <left hex> <right hex> <n_proofs> <n_failed>        (read() after the first leg)
//   acc <ok 0/1> <left hex> <right hex> <status...>           (finalize() after the second)
//   again <ok 0/1>                                            (finalize() once more: the accumulator is not consumed)
// tests/test_gpu_cpp_accumulator.py builds it with g++ and compares the lines with the Python class and the CPU oracle.
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
    if (argc != 3) { fprintf(stderr, "usage: accumulator_harness <dir> <cut>\n"); return 2; }
    const std::string d = argv[1];
    const size_t cut = std::stoul(argv[2]);
    std::ifstream in(d + "/items.txt");
    size_t n_keys = 0, n = 0;
    if (!(in >> n_keys >> n) || cut > n) return 2;
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
        // let mut s = AccumulatorStrategy::new(&params); for each proof as it arrives { s = verify_proof(&params, &vk_i, s, ..)? } s.finalize()
        Accumulator acc(*ctxs[0]);
        std::vector<int> st = acc.process(handles, std::vector<Accumulator::Item>(items.begin(), items.begin() + cut), Bytes(rand.begin(), rand.begin() + 32 * cut));
        acc.read();
        printf("first "); hex(acc.left(), 64); printf(" "); hex(acc.right(), 64); printf(" %zu %zu\n", acc.n_proofs(), acc.n_failed());
        const std::vector<int> st2 = acc.process(handles, std::vector<Accumulator::Item>(items.begin() + cut, items.end()), Bytes(rand.begin() + 32 * cut, rand.end()));
        st.insert(st.end(), st2.begin(), st2.end());
        const bool ok = acc.finalize();
        printf("acc %d ", ok ? 1 : 0); hex(acc.left(), 64); printf(" "); hex(acc.right(), 64);
        for (int s : st) printf(" %d", s);
        printf("\n");
        printf("again %d\n", acc.finalize() ? 1 : 0);
    } catch (const Failure& f) {
        fprintf(stderr, "failure %d: %s\n", f.code, f.what());
        return 1;
    }
    return 0;
}
