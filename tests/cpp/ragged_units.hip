// The multipliers of groups of unequal size (halo2_verifier_amd/csrc/verify_kernels.hip: the segmented suffix scan k_seg_mult_tiles,
// k_seg_mult_scan_tiles, k_seg_mult_apply behind ragged_multipliers_enqueue) run on raw draws chosen by the test
// (tests/test_gpu_ragged_multipliers.py):
//   ragged_units IN OUT
//   IN:  words: n_jobs, then per job: n_groups, the n_groups sizes, then sum(sizes) draws of 32 little-endian bytes
//   OUT: per job, sum(sizes) multipliers of 32 little-endian canonical bytes: mult[p] = the product of the draws behind p in p's group
// The "last proof of its group" bytes are built here as the library's host side builds them.  The multipliers and the per-tile scratch
// arrays are preset to 0xff between two 64-byte bands of 0xA5, which are checked after the launch.
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

constexpr size_t BAND = 64;
// a device array of `bytes` bytes of 0xff between two bands of 0xA5
struct Banded {
    uint8_t* p = nullptr; size_t bytes;
    explicit Banded(size_t b) : bytes(b) { CK(hipMalloc(&p, bytes + 2 * BAND)); CK(hipMemset(p, 0xA5, bytes + 2 * BAND)); if (bytes) CK(hipMemset(p + BAND, 0xff, bytes)); }
    ~Banded() { hipFree(p); }
    template <class T> T* at() const { return reinterpret_cast<T*>(p + BAND); }
    bool intact(std::vector<uint8_t>& body) const {
        std::vector<uint8_t> h(bytes + 2 * BAND);
        CK(hipMemcpy(h.data(), p, h.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < BAND; ++i) if (h[i] != 0xA5 || h[BAND + bytes + i] != 0xA5) return false;
        body.assign(h.begin() + BAND, h.begin() + BAND + bytes);
        return true;
    }
};

int main(int argc, char** argv) {
    REQUIRE(argc == 3, "usage: ragged_units IN OUT");
    std::ifstream f(argv[1], std::ios::binary);
    REQUIRE(f.good(), "cannot open input");
    std::vector<char> in((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    size_t at = 0;
    auto word = [&]() { REQUIRE(at + 4 <= in.size(), "input too short"); uint32_t w; memcpy(&w, in.data() + at, 4); at += 4; return w; };
    static_assert(sizeof(Fr) == 36 && BAND % 4 == 0, "nine limbs");
    std::vector<uint8_t> out;
    const uint32_t jobs = word();
    REQUIRE(jobs <= 64, "too many jobs");
    for (uint32_t job = 0; job < jobs; ++job) {
        const uint32_t G = word();
        REQUIRE(G >= 1 && G <= (1u << 20), "bad group count");
        std::vector<uint8_t> last;
        for (uint32_t g = 0; g < G; ++g) {
            const uint32_t sz = word();
            REQUIRE(sz >= 1 && sz <= (1u << 22) && last.size() + sz <= (1u << 22), "bad group size");
            last.resize(last.size() + sz, 0); last.back() = 1;
        }
        const size_t n = last.size(), tiles = ragged_multipliers_tiles((uint32_t)n);
        REQUIRE(at + 32 * n <= in.size(), "input too short");
        uint8_t* d_tail = nullptr; uint8_t* d_last = nullptr;
        CK(hipMalloc(&d_tail, 32 * n)); CK(hipMalloc(&d_last, n));
        CK(hipMemcpy(d_tail, in.data() + at, 32 * n, hipMemcpyHostToDevice));
        CK(hipMemcpy(d_last, last.data(), n, hipMemcpyHostToDevice));
        at += 32 * n;
        Banded mult(n * sizeof(Fr)), tile_prod(tiles * sizeof(Fr)), tile_words(2 * tiles * 4);
        const int rc = ragged_multipliers_enqueue(0, d_tail, d_last, (uint32_t)n, mult.at<Fr>(), tile_prod.at<Fr>(), tile_words.at<uint32_t>());
        if (rc) { fprintf(stderr, "ragged_multipliers_enqueue: %d %s\n", rc, g_err.c_str()); return 4; }
        CK(hipDeviceSynchronize());
        std::vector<uint8_t> body, scratch;
        if (!mult.intact(body) || !tile_prod.intact(scratch) || !tile_words.intact(scratch)) { fprintf(stderr, "job %u: guard band overwritten\n", job); return 5; }
        const size_t o = out.size();
        out.resize(o + 32 * n);
        for (size_t i = 0; i < n; ++i) { Fr m; memcpy((void*)&m, body.data() + i * sizeof(Fr), sizeof(Fr)); m.to_bytes(&out[o + 32 * i]); }
        CK(hipFree(d_tail)); CK(hipFree(d_last));
    }
    REQUIRE(at == in.size(), "input longer than its jobs");
    FILE* g = fopen(argv[2], "wb");
    REQUIRE(g && fwrite(out.data(), 1, out.size(), g) == out.size() && fclose(g) == 0, "cannot write output");
    return 0;
}
