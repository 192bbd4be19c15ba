// What the C++ host mirror (include/h2v.hpp) hands to the C ABI, call by call: walks the public classes over tiny fake proofs with
// tests/cpp/h2v_stub.cpp linked in place of the library, which prints every call; this file prints what the mirror returned.
// tests/test_mirror_trace.py builds both with -fsanitize=address,undefined and compares stdout with tests/golden/mirror_calls_cpp.txt.
#include <cstdio>
#include <functional>
#include "../../include/h2v.hpp"
#include "h2v_stub.h"

using namespace halo2_verifier;

static Bytes fe(uint8_t v) { Bytes b(32, 0); b[0] = v; return b; }
static Bytes run(size_t n, uint8_t from) { Bytes b(n); for (size_t i = 0; i < n; ++i) b[i] = (uint8_t)(from + i); return b; }
static Bytes proof(uint8_t i) { Bytes p = run(20 + i, i); p[3] = 0; return p; }
static Instances uniform(uint8_t i) { return {{fe(10 * i + 1), fe(0)}, {fe(10 * i + 3)}}; }             // columns of 2 and 1
static Instances mixed(uint8_t i) {                                                                        // shapes a, b, a, c
    switch (i) {
        case 0: return {{fe(1)}, {fe(2), fe(3)}};
        case 1: return {{fe(4), fe(5)}, {fe(6)}};
        case 2: return {{fe(7)}, {fe(8), fe(9)}};
        default: return {{}, {fe(0)}};
    }
}
using h2v_stub::fnv;   // (the hash the stand-in prints of what it is handed)
static void scenario(const char* name, const std::function<void()>& body) {
    printf("## %s\n", name);
    try { body(); } catch (const Failure& f) { printf("  Failure %d: %s\n", f.code, f.what()); }
}
static void report(const char* what, bool ok, const AccumulatorStrategy& s) {
    printf("  %s -> %d statuses=[", what, ok ? 1 : 0);
    for (size_t i = 0; i < s.statuses().size(); ++i) printf(i ? ",%d" : "%d", s.statuses()[i]);
    printf("] left=%016llx right=%016llx range_checks=%zu seed_ok=%d\n", (unsigned long long)fnv(s.left(), 64), (unsigned long long)fnv(s.right(), 64),
           s.range_checks(), s.seed_ok() ? 1 : 0);
}
static void report(const RangeChecks& r) {
    printf("  -> ok=[");
    for (size_t i = 0; i < r.ok.size(); ++i) printf(i ? ",%d" : "%d", r.ok[i] ? 1 : 0);
    printf("] lefts=%zu:%016llx rights=%zu:%016llx\n", r.lefts.size(), (unsigned long long)fnv(r.lefts.data(), r.lefts.size()), r.rights.size(),
           (unsigned long long)fnv(r.rights.data(), r.rights.size()));
}

int main() {
    const ParamsKZG params{run(164, 8), SerdeFormat::RawBytes};
    const VerifyingKey vk_a{run(9, 'A'), SerdeFormat::RawBytes}, vk_b{run(9, 'B'), SerdeFormat::Processed};
    const Bytes one = fe(1), base_l = run(64, 7), base_r = run(128, 9);
    Bytes two = fe(2), three = fe(3);
    two.insert(two.end(), three.begin(), three.end());
    typedef std::function<void(AccumulatorStrategy&)> Fill;
    const Fill nothing = [](AccumulatorStrategy&) {};
    const Fill one_key = [&](AccumulatorStrategy& s) { for (uint8_t i = 0; i < 3; ++i) verify_proof(params, vk_a, s, uniform(i), proof(i)); };
    const Fill one_key_mixed = [&](AccumulatorStrategy& s) { for (uint8_t i = 0; i < 4; ++i) verify_proof(params, vk_a, s, mixed(i), proof(i)); };
    const Fill two_keys = [&](AccumulatorStrategy& s) { for (uint8_t i = 0; i < 4; ++i) verify_proof(params, i % 2 ? vk_a : vk_b, s, mixed(i), proof(i)); };
    const Fill wrong_columns = [&](AccumulatorStrategy& s) { verify_proof(params, vk_a, s, uniform(0), proof(0)); verify_proof(params, vk_a, s, {{fe(1)}}, proof(1)); };
    // every proof with one column where the key has two: the one-key calls hand proof 0's column count over and the library judges it
    const Fill one_column = [&](AccumulatorStrategy& s) { for (uint8_t i = 0; i < 2; ++i) verify_proof(params, vk_a, s, {{fe(i), fe(9)}}, proof(i)); };
    struct { const char* name; Fill fill; size_t draws; } fills[] = {{"empty", nothing, 0}, {"one_key", one_key, 3}, {"one_key_mixed_shapes", one_key_mixed, 4},
                                                                    {"two_keys", two_keys, 4}, {"wrong_column_count", wrong_columns, 2}, {"one_column_throughout", one_column, 2}};
    struct { const char* name; std::function<bool(AccumulatorStrategy&)> call; } finalizers[] = {
        {"finalize", [](AccumulatorStrategy& s) { return s.finalize(); }},
        {"finalize_identify", [](AccumulatorStrategy& s) { return s.finalize_identify(); }},
        {"finalize_identify_keys", [](AccumulatorStrategy& s) { return s.finalize_identify_keys(); }}};
    for (const auto& fin : finalizers)
        for (const auto& f : fills)
            for (int variant = 0; variant < 4; ++variant) {   // OS draws; given draws; draws of the wrong length; seeded (AccumulatorStrategy::with) with draws
                const char* tags[] = {"os_draws", "draws", "short_draws", "seeded"};
                const std::string name = std::string(fin.name) + "/" + f.name + "/" + tags[variant];
                scenario(name.c_str(), [&] {
                    AccumulatorStrategy s = variant == 3 ? AccumulatorStrategy::with(params, one, base_l, two, base_r, 1, MultiOpen::GWC, TranscriptKind::Keccak256, 2)
                                                         : AccumulatorStrategy(params);
                    f.fill(s);
                    if (variant) s.set_randomness(run(32 * f.draws + (variant == 2 ? 32 : 0), 100));
                    report(fin.name, fin.call(s), s);
                    if (variant == 1) report("again", fin.call(s), s);   // a strategy may be finalized twice
                });
            }
    scenario("with/bad_channel", [&] { AccumulatorStrategy::with(params, one, run(63, 0), Bytes(), Bytes()); });
    scenario("with/empty_channels", [&] {
        AccumulatorStrategy s = AccumulatorStrategy::with(params, Bytes(), Bytes(), Bytes(), Bytes());
        one_key(s);
        report("finalize", s.finalize(), s);
    });
    // the refusals the GPU harnesses pin: finalize_identify over several VKs, a seeded accumulation over several VKs
    scenario("identify_refused", [&] { AccumulatorStrategy s(params); two_keys(s); s.finalize_identify(); });
    scenario("seeded_refused", [&] { AccumulatorStrategy s = AccumulatorStrategy::with(params, one, base_l, one, base_l); two_keys(s); s.finalize(); });

    scenario("single_strategy", [&] {
        SingleStrategy s(params, 2, MultiOpen::GWC, TranscriptKind::Keccak256, 1);
        printf("  -> %d\n", (int)verify_proof(params, vk_b, s, uniform(1), proof(1)));
        printf("  -> %d\n", (int)verify_proof(params, vk_b, s, {{fe(1)}}, proof(2)));   // a wrong column count never reaches verify_each
        printf("  -> %d\n", (int)verify_proof(params, vk_b, s, {{}, {}}, Bytes()));
    });

    scenario("accumulator", [&] {
        Context base(params, VerifyingKey{}), ca(params, vk_a), cb(params, vk_b, 0, MultiOpen::SHPLONK, TranscriptKind::Blake2b, 1);
        Accumulator acc(base);
        auto show = [&](const std::vector<int>& st) {
            printf("  -> all_ok=%d statuses=[", acc.all_ok() ? 1 : 0);
            for (size_t i = 0; i < st.size(); ++i) printf(i ? ",%d" : "%d", st[i]);
            printf("]\n");
        };
        std::vector<Accumulator::Item> items;
        for (uint8_t i = 0; i < 4; ++i) items.push_back({(uint32_t)(i % 2), mixed(i), proof(i)});
        show(acc.process({&ca, &cb}, items, run(128, 50)));
        show(acc.process({&ca}, {{0, uniform(0), proof(0)}}));
        show(acc.process({&cb, &ca}, {}));
        for (int bad = 0; bad < 4; ++bad)
            try {
                if (bad == 0) acc.process({}, items);
                if (bad == 1) acc.process({&ca, &cb}, items, run(96, 0));
                if (bad == 2) acc.process({&ca}, items);
                if (bad == 3) acc.process({&ca}, {{0, {{fe(1)}}, proof(0)}});
            } catch (const Failure& f) { printf("  Failure %d: %s\n", f.code, f.what()); }
        acc.add_msm(one, base_l, two, base_r);
        acc.add_msm(Bytes(), Bytes(), Bytes(), Bytes());
        try { acc.add_msm(one, base_r, Bytes(), Bytes()); } catch (const Failure& f) { printf("  Failure %d: %s\n", f.code, f.what()); }
        acc.read();
        printf("  -> n_proofs=%zu n_failed=%zu left=%016llx right=%016llx\n", acc.n_proofs(), acc.n_failed(), (unsigned long long)fnv(acc.left(), 64),
               (unsigned long long)fnv(acc.right(), 64));
        printf("  -> finalize %d left=%016llx right=%016llx\n", acc.finalize() ? 1 : 0, (unsigned long long)fnv(acc.left(), 64), (unsigned long long)fnv(acc.right(), 64));
        acc.journal_begin(8);
        for (const Accumulator::Leg& l : acc.check_legs()) printf("  -> leg n_proofs=%zu n_failed=%zu pairing_ok=%d\n", l.n_proofs, l.n_failed, l.pairing_ok ? 1 : 0);
        acc.drop_legs({2, 1});
        acc.drop_legs({});
        for (size_t cap : {(size_t)1, (size_t)H2V_ACC_JOURNAL_MAX + 1})
            try { acc.journal_begin(cap); } catch (const Failure& f) { printf("  Failure %d: %s\n", f.code, f.what()); }
        try { acc.drop_legs({1, 0}); } catch (const Failure& f) { printf("  Failure %d: %s\n", f.code, f.what()); }
        try { acc.drop_legs({2, 3, 2}); } catch (const Failure& f) { printf("  Failure %d: %s\n", f.code, f.what()); }
        acc.journal_begin(0);
    });

    scenario("recheck", [&] {
        h2v_batch* b0 = (h2v_batch*)0x9000;
        h2v_batch* b1 = (h2v_batch*)0xA000;
        report(recheck(b0, {{0, 2}, {2, 1}, {1, 1}}));
        report(recheck(b0, {}));
        report(recheck(std::vector<h2v_batch*>{b0, b1}, std::vector<BatchRange>{{0, 0, 3}, {1, 0, 1}, {1, 1, 1}}));
        report(recheck(std::vector<h2v_batch*>{b1}, std::vector<BatchRange>{}));
        report(recheck(std::vector<h2v_batch*>{b0}, std::vector<BatchRange>{{1, 0, 1}}));   // a batch index out of range
    });
    return 0;
}
