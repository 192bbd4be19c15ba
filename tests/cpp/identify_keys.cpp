// C++ caller of AccumulatorStrategy::finalize_identify_keys() over proofs of several VerifyingKeys (include/h2v.hpp ->
// h2v_verify_batch_keys_identify).
//
//   identify_keys <dir>
// reads <dir>/params.bin, vk<k>.bin (k < n_keys), rand.bin (n x 32) and items.txt: "n_keys n", then one line per proof in call order,
// "<key> <n_cols> <col_len>... <proof hex> <instance values hex, or ->", and prints
//   identify <ok 0/1> <left hex> <right hex> <status...>
//   range_checks <count>
//   identify_refused <code>      (finalize_identify, the one-VK form, over several VKs)
// tests/test_gpu_cpp_identify_keys.py builds it with g++ and compares the lines with the CPU oracle.
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

struct Item { size_t key; Instances inst; Bytes proof; };

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: identify_keys <dir>\n"); return 2; }
    const std::string d = argv[1];
    std::ifstream in(d + "/items.txt");
    size_t n_keys = 0, n = 0;
    if (!(in >> n_keys >> n)) return 2;
    std::vector<Item> items(n);
    for (Item& it : items) {
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
            it.inst.push_back(c);
        }
    }
    try {
        ParamsKZG params{slurp(d + "/params.bin"), SerdeFormat::RawBytes};
        std::vector<VerifyingKey> vks;
        for (size_t k = 0; k < n_keys; ++k) vks.push_back(VerifyingKey{slurp(d + "/vk" + std::to_string(k) + ".bin"), SerdeFormat::RawBytes});
        const Bytes rand = slurp(d + "/rand.bin");
        // let mut s = AccumulatorStrategy::new(&params); for each proof { s = verify_proof(&params, &vk_i, s, ..)? } then the verdict of
        // the accumulation and of every proof
        AccumulatorStrategy acc(params);
        acc.set_randomness(rand);
        for (const Item& it : items) verify_proof(params, vks[it.key], acc, it.inst, it.proof);
        const bool ok = acc.finalize_identify_keys();
        printf("identify %d ", ok ? 1 : 0); hex(acc.left(), 64); printf(" "); hex(acc.right(), 64);
        for (int s : acc.statuses()) printf(" %d", s);
        printf("\n");
        printf("range_checks %zu\n", acc.range_checks());
        try { acc.finalize_identify(); printf("identify_refused 0\n"); } catch (const Failure& f) { printf("identify_refused %d\n", f.code); }
    } catch (const Failure& f) {
        fprintf(stderr, "failure %d: %s\n", f.code, f.what());
        return 1;
    }
    return 0;
}
