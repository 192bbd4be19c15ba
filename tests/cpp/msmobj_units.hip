// The two kernels of the resident MSM object (halo2_verifier_amd/csrc/util.hip), alone through their launchers, on inputs chosen by
// tests/test_gpu_msmobj_units.py: k_msm_scale (msm_scale_enqueue) and k_affine_to_bytes (affine_to_bytes_enqueue).  Built with the
// library's flags by halo2_verifier_amd/csrc/Makefile (build/msmobj_units); the prelude is tests/cpp/units.h.
//
//   msmobj_units scale|to_bytes IN OUT
// Files are little-endian uint32 words.  Every buffer a kernel writes lies between two guard bands that are checked after the kernel: a
// write past it ends the program with status 5.  Each buffer is `slack` elements longer than the n the launcher is given: what lies past
// n must come back unchanged.
#include "../../halo2_verifier_amd/csrc/util.hip"
#include "units.h"

// IN per job: n (terms), slack; the factor as 8 words of canonical bytes; (n + slack) * 8 scalar words
// OUT per job: the (n + slack) * 8 words after the launch
static void job_scale(In& in, Out& out) {
    const uint32_t n = in.word(), slack = in.word();
    REQUIRE(n <= 65536 && slack <= 4096, "bad scale job");
    const Fr factor = in.field<Fr>();   // Montgomery form: f R
    const size_t total = (size_t)8 * (n + slack);
    const uint32_t* h = in.span(total);
    Guarded<uint32_t> words(total);
    if (total) CK(hipMemcpy(words.p, h, 4 * total, hipMemcpyHostToDevice));
    RC(msm_scale_enqueue(0, words.p, factor, n));
    CK(hipDeviceSynchronize());
    words.collect(out, "scalar words");
}

// IN per job: n (points), slack; n points as 16 words of canonical x | y bytes (all-zero: the identity; not checked against the curve)
// OUT per job: (n + slack) * 16 words: the bytes the kernel wrote, then the preset (0xff) past n
static void job_to_bytes(In& in, Out& out) {
    const uint32_t n = in.word(), slack = in.word();
    REQUIRE(n <= 65536 && slack <= 4096, "bad to_bytes job");
    std::vector<G1A> pts(n);
    for (G1A& p : pts) { p.x = in.field<Fq>(); p.y = in.field<Fq>(); }   // (0, 0) is the identity as the library holds it
    G1A* d_in = to_device(pts.data(), n);
    Guarded<uint8_t> bytes((size_t)64 * (n + slack));
    RC(affine_to_bytes_enqueue(0, d_in, bytes.p, n));
    CK(hipDeviceSynchronize());
    bytes.collect(out, "point bytes");
    CK(hipFree(d_in));
}

static const Mode MODES[] = {{"scale", each_job<job_scale, 256>, true, false}, {"to_bytes", each_job<job_to_bytes, 256>, true, false}};
int main(int argc, char** argv) { return units_main("msmobj_units", MODES, argc, argv); }
