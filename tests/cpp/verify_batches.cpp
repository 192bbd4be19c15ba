// C++ caller of many AccumulatorStrategy batches of their own sizes in one call (include/h2v.hpp verify_batches -> h2v_verify_batches).
//
//   verify_batches <dir>
// reads <dir>/params.bin, vk.bin, rand.bin (n x 32) and items.txt: "n_batches", the batch sizes, then one line per proof in call order,
// "<n_cols> <col_len>... <proof hex> <instance values hex, or ->", and prints per batch
//   batch <ok 0/1> <left hex> <right hex> <status...>
// then "empty_refused <code>" for a call with a batch of no proofs.  tests/test_gpu_verify_batches.py builds it with g++.
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
static void hex(const Bytes& b) { for (uint8_t v : b) printf("%02x", v); }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: verify_batches <dir>\n"); return 2; }
    const std::string d = argv[1];
    std::ifstream in(d + "/items.txt");
    size_t k = 0;
    if (!(in >> k)) return 2;
    std::vector<std::vector<BatchItem>> batches(k);
    for (auto& b : batches) { size_t sz = 0; in >> sz; b.resize(sz); }
    for (auto& b : batches)
        for (BatchItem& it : b) {
            size_t ncols = 0;
            in >> ncols;
            std::vector<size_t> lens(ncols);
            for (size_t& l : lens) in >> l;
            std::string ph, ih;
            if (!(in >> ph >> ih)) return 2;
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
        VerifyingKey vk{slurp(d + "/vk.bin"), SerdeFormat::RawBytes};
        Context ctx(params, vk);
        for (const BatchResult& r : verify_batches(ctx, batches, slurp(d + "/rand.bin"))) {
            printf("batch %d ", r.ok ? 1 : 0); hex(r.left); printf(" "); hex(r.right);
            for (int s : r.statuses) printf(" %d", s);
            printf("\n");
        }
        batches.push_back({});
        try { verify_batches(ctx, batches); printf("empty_refused 0\n"); } catch (const Failure& f) { printf("empty_refused %d\n", f.code); }
    } catch (const Failure& f) {
        fprintf(stderr, "failure %d: %s\n", f.code, f.what());
        return 1;
    }
    return 0;
}
