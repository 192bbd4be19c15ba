// The batch multipliers' kernels (halo2_verifier_amd/csrc/verify_kernels.hip: k_mult_tiles, k_mult_scan_tiles, k_mult_apply behind
// multipliers_enqueue) run on raw draws chosen by the test (tests/test_gpu_multipliers.py):
//   multipliers_units IN OUT
//   IN:  words: n_jobs, then per job: groups, n_tail per group, n per group, then groups * n_tail draws of 32 little-endian bytes
//   OUT: per job, groups * n multipliers of 32 little-endian canonical bytes: mult[g][p] = prod_{j > p} draw[g][j] mod r
// and k_gather_multipliers behind gather_multipliers_enqueue:
//   multipliers_units gather IN OUT
//   IN:  words: n_jobs, then per job: n_src, n, n_src source elements (9 raw limbs each, as they lie in memory), n indices
//   OUT: per job, n elements (9 limbs each): out[i] = src[idx[i]].  The output is preset to 0xff between two 32-byte bands of 0xA5, which
//        are checked; every index is checked against n_src on the host before the launch
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>
#include "../../halo2_verifier_amd/csrc/verify_kernels.hip"

namespace h2v {
static std::string g_err;
void set_last_error(const std::string& s) { g_err = s; }
}
using namespace h2v;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); exit(3); } } while (0)
#define REQUIRE(c, msg) do { if (!(c)) { fprintf(stderr, "bad input: %s\n", msg); exit(2); } } while (0)

static int run_gather(const char* in_path, const char* out_path) {
    std::ifstream f(in_path, std::ios::binary);
    REQUIRE(f.good(), "cannot open input");
    std::vector<char> in((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    REQUIRE(in.size() % 4 == 0, "input is not whole words");
    const uint32_t* w = reinterpret_cast<const uint32_t*>(in.data());
    const size_t total = in.size() / 4;
    size_t at = 0;
    auto span = [&](size_t words) { REQUIRE(words <= total - at, "input too short"); const uint32_t* p = w + at; at += words; return p; };
    static_assert(sizeof(Fr) == 36, "nine limbs");
    constexpr size_t BAND = 32;
    std::vector<uint32_t> out;
    const uint32_t jobs = *span(1);
    REQUIRE(jobs <= 64, "too many jobs");
    for (uint32_t job = 0; job < jobs; ++job) {
        const uint32_t n_src = *span(1), n = *span(1);
        REQUIRE(n_src >= 1 && n_src <= (1u << 16) && n <= (1u << 16), "bad gather job");
        const uint32_t* src = span((size_t)9 * n_src);
        const uint32_t* idx = span(n);
        for (uint32_t i = 0; i < n; ++i) REQUIRE(idx[i] < n_src, "index outside the source");
        Fr* d_src = nullptr; uint32_t* d_idx = nullptr; uint8_t* d_out = nullptr;
        const size_t bytes = (size_t)n * sizeof(Fr);
        CK(hipMalloc(&d_src, (size_t)n_src * sizeof(Fr))); CK(hipMalloc(&d_idx, (n ? n : 1) * 4)); CK(hipMalloc(&d_out, bytes + 2 * BAND));
        CK(hipMemcpy((void*)d_src, src, (size_t)n_src * sizeof(Fr), hipMemcpyHostToDevice));
        if (n) CK(hipMemcpy(d_idx, idx, (size_t)n * 4, hipMemcpyHostToDevice));
        CK(hipMemset(d_out, 0xA5, bytes + 2 * BAND));
        if (n) CK(hipMemset(d_out + BAND, 0xff, bytes));
        const int rc = gather_multipliers_enqueue(0, d_src, d_idx, n, reinterpret_cast<Fr*>(d_out + BAND));
        if (rc) { fprintf(stderr, "gather_multipliers_enqueue: %d %s\n", rc, g_err.c_str()); return 4; }
        CK(hipDeviceSynchronize());
        std::vector<uint8_t> h(bytes + 2 * BAND);
        CK(hipMemcpy(h.data(), d_out, h.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < BAND; ++i)
            if (h[i] != 0xA5 || h[BAND + bytes + i] != 0xA5) { fprintf(stderr, "guard band overwritten at byte %zu\n", i); return 5; }
        const size_t o = out.size();
        out.resize(o + bytes / 4);
        if (bytes) memcpy(out.data() + o, h.data() + BAND, bytes);
        CK(hipFree(d_src)); CK(hipFree(d_idx)); CK(hipFree(d_out));
    }
    REQUIRE(at == total, "input longer than its jobs");
    FILE* g = fopen(out_path, "wb");
    REQUIRE(g && fwrite(out.data(), 4, out.size(), g) == out.size() && fclose(g) == 0, "cannot write output");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && std::string(argv[1]) == "gather") return run_gather(argv[2], argv[3]);
    REQUIRE(argc == 3, "usage: multipliers_units IN OUT | multipliers_units gather IN OUT");
    std::ifstream f(argv[1], std::ios::binary);
    REQUIRE(f.good(), "cannot open input");
    std::vector<char> in((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    size_t at = 0;
    auto word = [&]() { REQUIRE(at + 4 <= in.size(), "input too short"); uint32_t w; memcpy(&w, in.data() + at, 4); at += 4; return w; };
    std::vector<uint8_t> out;
    const uint32_t jobs = word();
    for (uint32_t job = 0; job < jobs; ++job) {
        const uint32_t G = word(), nt = word(), n = word();
        REQUIRE(G && nt && n && n <= nt && G <= 1024 && nt <= (1u << 22), "bad job");
        const size_t draws = (size_t)G * nt, mults = (size_t)G * n;
        REQUIRE(at + 32 * draws <= in.size(), "input too short");
        uint8_t* d_tail = nullptr; Fr* d_mult = nullptr; Fr* d_scratch = nullptr;
        CK(hipMalloc(&d_tail, 32 * draws)); CK(hipMalloc(&d_mult, mults * sizeof(Fr))); CK(hipMalloc(&d_scratch, multipliers_scratch(G * nt, G) * sizeof(Fr)));
        CK(hipMemcpy(d_tail, in.data() + at, 32 * draws, hipMemcpyHostToDevice));
        CK(hipMemset(d_mult, 0xff, mults * sizeof(Fr)));
        at += 32 * draws;
        const int rc = multipliers_enqueue(0, d_tail, G * nt, G * n, G, d_mult, d_scratch);
        if (rc) { fprintf(stderr, "multipliers_enqueue: %d %s\n", rc, g_err.c_str()); return 4; }
        CK(hipDeviceSynchronize());
        std::vector<Fr> m(mults);
        CK(hipMemcpy((void*)m.data(), d_mult, mults * sizeof(Fr), hipMemcpyDeviceToHost));
        const size_t o = out.size();
        out.resize(o + 32 * mults);
        for (size_t i = 0; i < mults; ++i) m[i].to_bytes(&out[o + 32 * i]);
        CK(hipFree(d_tail)); CK(hipFree(d_mult)); CK(hipFree(d_scratch));
    }
    FILE* g = fopen(argv[2], "wb");
    REQUIRE(g && fwrite(out.data(), 1, out.size(), g) == out.size() && fclose(g) == 0, "cannot write output");
    return 0;
}
