// The fold of a merge, k_accumulator_merge_fold (halo2_verifier_amd/csrc/util.hip), alone, through the library's own
// accumulator_merge_fold_enqueue, on inputs chosen by tests/test_gpu_merge_units.py.  Built with the library's flags by
// halo2_verifier_amd/csrc/Makefile (build/merge_units).
//
//   merge_units fold IN OUT
// IN (little-endian uint32 words): n_jobs; per job: n (records), team (0: the host rule), with_sums, with_map, n_slots (pairs the
//     journal array holds), (with_map) n slot words, the accumulator (2 points of 27 words), n records (328 words each)
// OUT per job: the team the launch ran with, the accumulator (2 points), (with_sums) the journal array (2 n_slots points)
// Points and records are raw 29-bit limbs as they lie in memory.  Every output buffer lies between two bands of 0xA5 that are
// checked after the kernel (a write past an output ends the program with status 5); the journal array is preset to 0xff, so a slot
// that no record owns must come back untouched.  Every HIP call is checked.  Every count and every slot that reaches the kernel is
// checked on the host first: n <= 512, the team a power of two in 1 .. 64, every slot below n_slots and none given twice.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>
#include "../../halo2_verifier_amd/csrc/util.hip"

namespace h2v {
static std::string g_err;
void set_last_error(const std::string& s) { g_err = s; }
}
using namespace h2v;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); exit(3); } } while (0)
#define REQUIRE(c, msg) do { if (!(c)) { fprintf(stderr, "bad input: %s\n", msg); exit(2); } } while (0)
#define RC(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "%s: %d %s\n", #x, rc_, g_err.c_str()); exit(4); } } while (0)

static std::vector<uint32_t> slurp_words(const char* path) {
    std::ifstream f(path, std::ios::binary);
    REQUIRE(f.good(), "cannot open input");
    std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    REQUIRE(b.size() % 4 == 0, "input is not whole words");
    std::vector<uint32_t> w(b.size() / 4);
    memcpy(w.data(), b.data(), b.size());
    return w;
}
static void spill(const char* path, const std::vector<uint32_t>& out) {
    FILE* f = fopen(path, "wb");
    REQUIRE(f && fwrite(out.data(), 4, out.size(), f) == out.size() && fclose(f) == 0, "cannot write output");
}
struct Words {
    const std::vector<uint32_t>& w;
    size_t at = 0;
    uint32_t next() { REQUIRE(at < w.size(), "input too short"); return w[at++]; }
    const uint32_t* span(size_t words) { REQUIRE(words <= w.size() - at, "input too short"); const uint32_t* p = w.data() + at; at += words; return p; }
};
// `bytes` of device memory between two bands of 0xA5, 128 bytes each
struct Guarded {
    static constexpr size_t BAND = 128;
    uint8_t* base = nullptr;
    size_t bytes = 0;
    Guarded(size_t n_bytes, int preset) : bytes(n_bytes) {
        CK(hipMalloc(&base, 2 * BAND + bytes));
        CK(hipMemset(base, 0xA5, 2 * BAND + bytes));
        if (bytes) CK(hipMemset(base + BAND, preset, bytes));
    }
    Guarded(const Guarded&) = delete;
    Guarded& operator=(const Guarded&) = delete;
    void* p() const { return base + BAND; }
    void collect(std::vector<uint32_t>& out, const char* what) {
        std::vector<uint8_t> h(2 * BAND + bytes);
        CK(hipMemcpy(h.data(), base, h.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < BAND; ++i)
            if (h[i] != 0xA5 || h[BAND + bytes + i] != 0xA5) { fprintf(stderr, "guard band of %s overwritten at byte %zu\n", what, i); exit(5); }
        const size_t o = out.size();
        out.resize(o + bytes / 4);
        if (bytes) memcpy(out.data() + o, h.data() + BAND, bytes);
    }
    ~Guarded() { if (base) (void)hipFree(base); }
};

static void run_fold(Words& in, std::vector<uint32_t>& out) {
    const uint32_t jobs = in.next();
    REQUIRE(jobs <= 256, "too many jobs");
    for (uint32_t job = 0; job < jobs; ++job) {
        const uint32_t n = in.next(), team = in.next(), with_sums = in.next(), with_map = in.next(), n_slots = in.next();
        REQUIRE(n <= 512 && with_sums <= 1 && with_map <= 1 && n_slots <= 1024, "bad fold job");
        REQUIRE(team <= 64 && (team & (team - 1)) == 0, "the team is 0 or a power of two in 1 .. 64");
        REQUIRE(!with_map || with_sums, "a slot map without a journal array");
        REQUIRE(!with_sums || n_slots >= n, "fewer slots than records");
        std::vector<uint32_t> slots;
        if (with_map) {
            const uint32_t* sp = in.span(n);
            slots.assign(sp, sp + n);
            std::vector<bool> seen(n_slots, false);
            for (uint32_t s : slots) { REQUIRE(s < n_slots && !seen[s], "a slot out of range or given twice"); seen[s] = true; }
        }
        static_assert(sizeof(G1J) == 108 && sizeof(AccRecord) == 1312, "word layouts");
        Guarded acc(2 * sizeof(G1J), 0xff), sums(with_sums ? (size_t)2 * n_slots * sizeof(G1J) : 0, 0xff);
        CK(hipMemcpy(acc.p(), in.span(2 * 27), 2 * sizeof(G1J), hipMemcpyHostToDevice));
        void* d_recs = nullptr;
        uint32_t* d_slots = nullptr;
        CK(hipMalloc(&d_recs, (n ? n : 1) * sizeof(AccRecord)));
        if (n) CK(hipMemcpy(d_recs, in.span((size_t)n * 328), (size_t)n * sizeof(AccRecord), hipMemcpyHostToDevice));
        if (with_map) {
            CK(hipMalloc(&d_slots, (n ? n : 1) * 4));
            if (n) CK(hipMemcpy(d_slots, slots.data(), 4 * (size_t)n, hipMemcpyHostToDevice));
        }
        RC(accumulator_merge_fold_enqueue(0, d_recs, n, team, d_slots, with_sums ? (G1J*)sums.p() : nullptr, (G1J*)acc.p()));
        CK(hipDeviceSynchronize());
        out.push_back(team ? team : accumulator_merge_team(n));
        acc.collect(out, "acc");
        sums.collect(out, "sums");
        CK(hipFree(d_recs));
        if (d_slots) CK(hipFree(d_slots));
    }
}

int main(int argc, char** argv) {
    REQUIRE(argc == 4 && std::string(argv[1]) == "fold", "usage: merge_units fold IN OUT");
    const std::vector<uint32_t> words = slurp_words(argv[2]);
    Words in{words};
    std::vector<uint32_t> out;
    run_fold(in, out);
    REQUIRE(in.at == words.size(), "input longer than its jobs");
    spill(argv[3], out);
    return 0;
}
