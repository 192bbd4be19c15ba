// The shared prelude of the C++ caller programs (tests/cpp/*.cpp): stand-alone programs that drive the library as a user would, through
// include/h2v.hpp, include/h2v_guards.hpp and the C ABI.  tests/caller_harness.py builds and runs them.  Plain C++17, no HIP headers
// (tests/cpp/caller_hip.h adds the HIP runtime's check for the programs built with hipcc).
//
// A program is given a directory.  The files it may hold:
//   params.bin                the KZG parameters, raw bytes
//   vk.bin | vk<k>.bin        one verifying key, or one per key k < n_keys, raw bytes
//   rand.bin                  n x 32 bytes: one draw per proof, little-endian canonical Fr
//   proofs.bin                n x proof_len bytes   } the flat inputs of a staged batch (read_staged): proofs of one length and
//   instances.bin             n x values x 32 bytes } one instance column of `values` values
//   items.txt                 proofs with instances of their own shapes, as text (read_items).  A header, then one line per proof in
//                             call order:
//                                 [<key>] <n_cols> <col_len>... <proof hex> <instance values hex, or ->
//                             <key> is there when the header is "<n_keys> <n>" (keyed) and absent when it is "<n>"; the instance values
//                             are the columns' 32-byte values one after the other, 32 x (the sum of the col_len) bytes, "-" for none.
//                             tests/cpp/verify_batches.cpp has a header of its own ("<n_batches>", then the sizes) over the same lines.
//   guards.txt                one line per Guard (read_guards):
//                                 <left scalars hex> <left bases hex> <right scalars hex> <right bases hex>
//                             "-" for an empty array.
// A word of hex is an even number of hex digits, or "-" for no bytes.  A file that cannot be read or is malformed (an odd-length or
// non-hex word, fewer lines than the header promises, instance bytes that are not 32 x the sum of the col_len) ends the program with
// status 2 and a message on stderr.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include "../../include/h2v.hpp"

namespace caller {
using namespace halo2_verifier;

[[noreturn]] inline void bad_input(const std::string& what) {
    fprintf(stderr, "%s\n", what.c_str());
    exit(2);
}

inline Bytes slurp(const std::string& p) {
    std::ifstream f(p, std::ios::binary);
    if (!f) bad_input("cannot read " + p);
    return Bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

inline Bytes unhex(const std::string& h) {
    Bytes out;
    if (h == "-") return out;
    auto digit = [&](char c) -> int {
        if (c >= '0' && c <= '9') return c - '0';
        if (c >= 'a' && c <= 'f') return c - 'a' + 10;
        if (c >= 'A' && c <= 'F') return c - 'A' + 10;
        bad_input("not a hex word: " + h.substr(0, 40));
    };
    if (h.size() % 2) bad_input("a hex word of odd length: " + h.substr(0, 40));
    out.reserve(h.size() / 2);
    for (size_t i = 0; i < h.size(); i += 2) out.push_back((uint8_t)(digit(h[i]) * 16 + digit(h[i + 1])));
    return out;
}

inline void hex(const uint8_t* b, size_t n) { for (size_t i = 0; i < n; ++i) printf("%02x", b[i]); }
inline void hex(const Bytes& b) { hex(b.data(), b.size()); }
inline void hex_or_dash(const Bytes& b) { if (b.empty()) printf("-"); else hex(b); }

// "<tag> <ok 0/1> <left hex> <right hex>", no newline: the verdict and the two evaluated channels (64 bytes each)
inline void verdict(const char* tag, bool ok, const uint8_t* left, const uint8_t* right) {
    printf("%s %d ", tag, ok ? 1 : 0); hex(left, 64); printf(" "); hex(right, 64);
}
// "<tag> <group verdicts> <status...> <left hex per group> <right hex per group>", no newline: the results of a grouped batch
inline void group_results(const char* tag, const std::vector<int>& ok, const std::vector<int>& st, const Bytes& left, const Bytes& right) {
    printf("%s ", tag);
    for (int v : ok) printf("%d", v);
    for (int v : st) printf(" %d", v);
    printf(" "); hex(left); printf(" "); hex(right);
}
// "<what> <ok 0/1> <left hex> <right hex> <n_proofs> <n_failed>": finalize() and read() of a resident accumulator
inline void report(const char* what, Accumulator& acc) {
    const bool ok = acc.finalize();
    acc.read();
    verdict(what, ok, acc.left(), acc.right());
    printf(" %zu %zu\n", acc.n_proofs(), acc.n_failed());
}
// what the mirror must refuse with H2V_ERR_BAD_ARGUMENT before any C call
template <class F> void refused(const char* what, F call) {
    try { call(); printf("accepted %s\n", what); } catch (const Failure& f) { if (f.code == H2V_ERR_BAD_ARGUMENT) printf("refused %s\n", what); else throw; }
}

// ---------------------------------------------------------------------------------------------------------------- items.txt, guards.txt
struct Item { size_t key; Instances inst; Bytes proof; };
struct Items { size_t n_keys = 1; std::vector<Item> items; };

// one line of items.txt
inline Item read_item(std::istream& in, bool keyed) {
    Item it{0, {}, {}};
    size_t ncols = 0, values = 0;
    if ((keyed && !(in >> it.key)) || !(in >> ncols)) bad_input("items.txt: fewer proofs than its header promises, or a line that does not start with numbers");
    std::vector<size_t> lens;
    for (size_t c = 0; c < ncols; ++c) {
        size_t l = 0;
        if (!(in >> l)) bad_input("items.txt: a line with fewer column lengths than columns");
        lens.push_back(l);
        values += l;
    }
    std::string ph, ih;
    if (!(in >> ph >> ih)) bad_input("items.txt: a line without its proof and instance words");
    it.proof = unhex(ph);
    const Bytes flat = unhex(ih);
    if (flat.size() % 32 || flat.size() / 32 != values) bad_input("items.txt: instance values that are not 32 bytes for each of the columns' lengths");
    size_t at = 0;
    for (size_t l : lens) {
        Column c;
        for (size_t j = 0; j < l; ++j, at += 32) c.emplace_back(flat.begin() + at, flat.begin() + at + 32);
        it.inst.push_back(c);
    }
    return it;
}

// <dir>/items.txt under the header "<n_keys> <n>" (keyed) or "<n>"
inline Items read_items(const std::string& dir, bool keyed) {
    std::ifstream in(dir + "/items.txt");
    if (!in) bad_input("cannot read " + dir + "/items.txt");
    Items out;
    size_t n = 0;
    if ((keyed && !(in >> out.n_keys)) || !(in >> n)) bad_input("items.txt: no header");
    for (size_t i = 0; i < n; ++i) {
        out.items.push_back(read_item(in, keyed));
        if (out.items.back().key >= out.n_keys) bad_input("items.txt: a key that its header does not count");
    }
    return out;
}

inline std::vector<Accumulator::Item> accumulator_items(const std::vector<Item>& items) {
    std::vector<Accumulator::Item> out;
    for (const Item& it : items) out.push_back({(uint32_t)it.key, it.inst, it.proof});
    return out;
}

// <dir>/guards.txt, every line of it
inline std::vector<Guard> read_guards(const std::string& dir) {
    std::ifstream in(dir + "/guards.txt");
    if (!in) bad_input("cannot read " + dir + "/guards.txt");
    std::vector<Guard> guards;
    for (std::string a, b, c, e; in >> a;) {
        if (!(in >> b >> c >> e)) bad_input("guards.txt: a line of fewer than four words");
        guards.push_back(Guard{unhex(a), unhex(b), unhex(c), unhex(e)});
    }
    return guards;
}

// ---------------------------------------------------------------------------------------------------------------- keys and contexts
// <dir>/vk<k>.bin for k < n_keys
inline std::vector<VerifyingKey> read_vks(const std::string& dir, size_t n_keys) {
    std::vector<VerifyingKey> vks;
    for (size_t k = 0; k < n_keys; ++k) vks.push_back(VerifyingKey{slurp(dir + "/vk" + std::to_string(k) + ".bin"), SerdeFormat::RawBytes});
    return vks;
}

// one Context per key, and their addresses as Accumulator::process takes them
struct Contexts {
    std::vector<std::unique_ptr<Context>> owned;
    std::vector<const Context*> handles;
    Contexts(const ParamsKZG& params, const std::vector<VerifyingKey>& vks) {
        for (const VerifyingKey& vk : vks) {
            owned.emplace_back(new Context(params, vk));
            handles.push_back(owned.back().get());
        }
    }
};

// ---------------------------------------------------------------------------------------------------------------- a staged batch
// owns an h2v_batch; h2v_batch_destroy waits for the batch's stream, so declare it after the arrays its launch reads or writes and
// after its context
struct BatchHolder {
    h2v_batch* b = nullptr;
    BatchHolder() = default;
    BatchHolder(const BatchHolder&) = delete;
    BatchHolder& operator=(const BatchHolder&) = delete;
    ~BatchHolder() { if (b) h2v_batch_destroy(b); }
};

// the flat inputs of n proofs of proof_len bytes with one instance column of `values` values
struct Staged { Bytes proofs, inst, rand; };
inline Staged read_staged(const std::string& dir, size_t n, size_t proof_len, size_t values) {
    Staged s{slurp(dir + "/proofs.bin"), slurp(dir + "/instances.bin"), slurp(dir + "/rand.bin")};
    if (!n || s.proofs.size() != n * proof_len || s.inst.size() != n * values * 32 || s.rand.size() != n * 32) bad_input("the files do not hold n proofs");
    return s;
}
// h2v_batch_create, h2v_batch_set_groups and h2v_batch_upload of them from the host, every proof with a draw
inline void stage(BatchHolder& batch, const Context& ctx, size_t n, size_t groups, size_t proof_len, size_t values, const Staged& s) {
    check(h2v_batch_create(ctx.handle(), n, values, &batch.b));
    check(h2v_batch_set_groups(batch.b, groups));
    check(h2v_batch_upload(batch.b, n, s.proofs.data(), proof_len, s.inst.data(), 1, &values, s.rand.data(), n));
}
}  // namespace caller
