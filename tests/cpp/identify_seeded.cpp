// C++ caller of a SEEDED AccumulatorStrategy's finalize_identify() (include/h2v.hpp -> h2v_verify_batch_seeded_identify).
//
//   identify_seeded <dir>
// reads <dir>/params.bin, vk.bin, rand.bin (n x 32), seed.bin (left x|y, right x|y: 128 bytes, the evaluated channels of the
// accumulation to resume) and items.txt: "n", then one line per proof, "<n_cols> <col_len>... <proof hex> <instance values hex, or ->",
// resumes the accumulation (AccumulatorStrategy::with, scalar 1 on either channel), queues the proofs and prints
//   identify <ok 0/1> <left hex> <right hex> <status...>
//   seed_ok <0/1>
//   range_checks <count>
//   plain <ok 0/1> <left hex> <right hex>        (finalize() on the same accumulation)
// tests/test_gpu_cpp_identify_seeded.py builds it with g++ and compares the lines with the CPU oracle.
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

struct Item { Instances inst; Bytes proof; };

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: identify_seeded <dir>\n"); return 2; }
    const std::string d = argv[1];
    std::ifstream in(d + "/items.txt");
    size_t n = 0;
    if (!(in >> n)) return 2;
    std::vector<Item> items(n);
    for (Item& it : items) {
        size_t ncols = 0;
        in >> ncols;
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
            it.inst.push_back(c);
        }
    }
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
        for (const Item& it : items) verify_proof(params, vk, acc, it.inst, it.proof);
        const bool ok = acc.finalize_identify();
        printf("identify %d ", ok ? 1 : 0); hex(acc.left(), 64); printf(" "); hex(acc.right(), 64);
        for (int s : acc.statuses()) printf(" %d", s);
        printf("\n");
        printf("seed_ok %d\n", acc.seed_ok() ? 1 : 0);
        printf("range_checks %zu\n", acc.range_checks());
        const bool plain = acc.finalize();
        printf("plain %d ", plain ? 1 : 0); hex(acc.left(), 64); printf(" "); hex(acc.right(), 64); printf("\n");
    } catch (const Failure& f) {
        fprintf(stderr, "failure %d: %s\n", f.code, f.what());
        return 1;
    }
    return 0;
}
