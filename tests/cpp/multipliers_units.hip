// The batch multipliers' kernels (halo2_verifier_amd/csrc/verify_kernels.hip: k_mult_tiles, k_mult_scan_tiles, k_mult_apply behind
// multipliers_enqueue) run on raw draws chosen by the test (tests/test_gpu_multipliers.py):
//   multipliers_units IN OUT
//   IN:  words: n_jobs, then per job: groups, n_tail per group, n per group, then groups * n_tail draws of 32 little-endian bytes
//   OUT: per job, groups * n multipliers of 32 little-endian canonical bytes: mult[g][p] = prod_{j > p} draw[g][j] mod r
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

int main(int argc, char** argv) {
    REQUIRE(argc == 3, "usage: multipliers_units IN OUT");
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
