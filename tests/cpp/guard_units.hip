// k_guard_terms (halo2_verifier_amd/csrc/util.hip), the conversion of a call's Guard terms, alone through its launcher
// guard_terms_enqueue, on inputs chosen by tests/test_gpu_guard_units.py.  Built with the library's flags by
// halo2_verifier_amd/csrc/Makefile (build/guard_units); the prelude is tests/cpp/units.h.
//
//   guard_units terms IN OUT
// Files are little-endian uint32 words.  Every output buffer is preset to 0xff and lies between two guard bands that are checked after
// the kernel: a write past an output ends the program with status 5.  Every guard index is checked against the multiplier count on
// the host before the launch.
#include "../../halo2_verifier_amd/csrc/util.hip"
#include "units.h"

// IN: n_jobs; per job: n (terms), with_mult, n_guards; n * 8 words of scalar bytes; n * 16 words of x | y bytes; (with_mult) n guard
//     indices, then n_guards multipliers as 8 words of canonical bytes each
// OUT per job: n * 8 scalar words, n affine points (18 words: x, y, raw limbs), the validity word
static void run_terms(In& in, Out& out) {
    for (uint32_t job = 0, jobs = job_count(in, 256); job < jobs; ++job) {
        const uint32_t n = in.word(), with_mult = in.word(), n_guards = in.word();
        REQUIRE(n <= 4096 && with_mult <= 1 && n_guards <= 4096, "bad terms job");
        REQUIRE(with_mult ? n_guards >= 1 : n_guards == 0, "multipliers: at least one guard; none without them");
        uint32_t* d_sc = to_device(in.span((size_t)8 * n), (size_t)8 * n);
        uint32_t* d_bs = to_device(in.span((size_t)16 * n), (size_t)16 * n);
        uint32_t* d_gidx = nullptr;
        Fr* d_mult = nullptr;
        if (with_mult) {
            const std::vector<uint32_t> gidx = in.words(n);
            for (uint32_t g : gidx) REQUIRE(g < n_guards, "a guard index past the multipliers");
            const std::vector<Fr> mult = in.fields<Fr>(n_guards);
            d_gidx = to_device(gidx.data(), n);
            d_mult = to_device(mult.data(), n_guards);
        }
        static_assert(sizeof(G1A) == 72, "word layouts");
        Guarded<uint32_t> words((size_t)8 * n), word(1, 0);   // (the validity word preset to 0: the launcher makes it 0xffffffff itself)
        Guarded<G1A> pts(n);
        RC(guard_terms_enqueue(0, reinterpret_cast<const uint8_t*>(d_sc), reinterpret_cast<const uint8_t*>(d_bs), d_gidx, d_mult, words.p, pts.p, word.p, n));
        CK(hipDeviceSynchronize());
        words.collect(out, "scalar words"); pts.collect(out, "bases"); word.collect(out, "validity word");
        CK(hipFree(d_sc)); CK(hipFree(d_bs));
        if (d_gidx) CK(hipFree(d_gidx));
        if (d_mult) CK(hipFree(d_mult));
    }
}

static const Mode MODES[] = {{"terms", run_terms, true, false}};
int main(int argc, char** argv) { return units_main("guard_units", MODES, argc, argv); }
