// The decompression stage with point hints and their miss list (k_decompress_hinted and k_decompress_misses,
// halo2_verifier_amd/csrc/verify_kernels.hip; include/h2v_hints.h), on points and hints programmed by
// tests/test_gpu_hints_list_units.py and compared there with tests/hints_reference.py and with the same stage without hints.  Built
// with the library's flags by halo2_verifier_amd/csrc/Makefile (build/hints_list_units); the prelude is tests/cpp/units.h.
//
//   hints_list_units decompress IN OUT   decompress_begin / _range (in the pieces the input gives) / _finish; a job with hints runs with the list
//
// IN is little-endian: a word n_jobs, then per job
//   n, np, n_main, proof_len, hinted (0 none | 1 a buffer of their own | 3 in the ycanon buffer), n_pieces, n_pieces + 1 piece bounds (0 = b[0] < .. < b[n_pieces] = n), point_offsets[np],
//   proofs [n][proof_len], and with hinted != 0 the hints [n][np][32]
// OUT per job: per (proof, point) x, y of pts, x, y of phi (32 canonical bytes each), a word (1 = pts holds the identity), the 32 ycanon
// bytes; then n raw status words, the miss word (0xffffffff in a job without hints: nobody wrote it), the list's counter word as the
// last piece left it, and the n x np words of the list as they lie (0xffffffff: never written — no point has that index).
// Every count and offset that reaches a kernel is checked on the host against the buffer sizes first ("bad input", status 2); every
// output buffer, the list and its counter included, lies between guard bands that are checked after the launch.
#include "../../halo2_verifier_amd/csrc/verify_kernels.hip"
#include "units.h"

#define FILL 0x11
#define MAX_PROOFS 4096u
#define MAX_ITEMS 64u
#define MAX_LEN (1u << 16)

static void run_decompress(In& in, Out& out) {
    const uint32_t n = in.word(), np = in.word(), n_main = in.word(), proof_len = in.word(), hinted = in.word(), n_pieces = in.word();
    REQUIRE(n >= 1 && n <= MAX_PROOFS && np >= 1 && np <= MAX_ITEMS && n_main <= np, "counts");
    REQUIRE(proof_len >= 32 && proof_len <= MAX_LEN && proof_len % 32 == 0 && hinted <= 3 && hinted != 2, "proof length, hinted");
    REQUIRE(n_pieces >= 1 && n_pieces <= n, "pieces");
    const std::vector<uint32_t> cut = in.words(n_pieces + 1);
    REQUIRE(cut[0] == 0 && cut[n_pieces] == n, "pieces must cover [0, n)");
    for (uint32_t i = 0; i < n_pieces; ++i) REQUIRE(cut[i] < cut[i + 1], "pieces must ascend");
    PlanDevice pd;
    Plan& pl = pd.host;
    pl.n_points = np; pl.n_main_points = n_main; pl.n_scalars = 0; pl.n_instance_values = 0; pl.proof_len = proof_len;
    pl.point_offsets = in.words(np);
    for (uint32_t o : pl.point_offsets) REQUIRE(o % 32 == 0 && o <= proof_len - 32, "point offset");      // (two 16-byte loads per point)
    RC(pd.point_offsets.alloc(np));
    CK(hipMemcpy(pd.point_offsets.p, pl.point_offsets.data(), 4 * (size_t)np, hipMemcpyHostToDevice));
    const size_t tp = (size_t)n * np;
    uint8_t* proofs = to_device(in.bytes((size_t)n * proof_len), (size_t)n * proof_len);
    Guarded<G1A> pts(tp, FILL), phi(tp, FILL); Guarded<uint8_t> ycanon(tp * 32, FILL); Guarded<int> status(n, FILL);
    Guarded<uint32_t> misses(1, 0xff), list(tp, 0xff), count(1, 0xff);   // the list: one word per point of the stage
    uint8_t* own = nullptr;
    StageArgs g{n, &pl, &pd, proofs, nullptr, pts.p, phi.p, ycanon.p, status.p, nullptr, 0, nullptr};
    if (hinted) {
        const uint8_t* h = in.bytes(tp * 32);
        if (hinted & 2) { CK(hipMemcpy(ycanon.p, h, tp * 32, hipMemcpyHostToDevice)); g.hints = ycanon.p; }   // in place, as the batch keeps them
        else g.hints = own = to_device(h, tp * 32);
        g.hint_misses = misses.p;
        g.miss_list = list.p; g.miss_list_count = count.p;
    }
    RC(decompress_begin_enqueue(0, g));
    for (uint32_t i = 0; i < n_pieces; ++i) RC(decompress_range_enqueue(0, g, cut[i], cut[i + 1]));
    RC(decompress_finish_enqueue(0, g));
    CK(hipDeviceSynchronize());
    const std::vector<G1A> hp = pts.host("pts"), hf = phi.host("phi");
    const std::vector<uint8_t> hy = ycanon.host("ycanon");
    for (size_t i = 0; i < tp; ++i) {
        out.field(hp[i].x); out.field(hp[i].y); out.field(hf[i].x); out.field(hf[i].y);
        out.word(hp[i].is_identity() ? 1u : 0u);
        out.raw(&hy[32 * i], 32);
    }
    status.collect(out, "status");
    misses.collect(out, "miss word");
    count.collect(out, "list counter");
    list.collect(out, "miss list");
    CK(hipFree(proofs));
    if (own) CK(hipFree(own));
}

int main(int argc, char** argv) {
    static const Mode modes[] = {{"decompress", each_job<run_decompress, 4096>, false, false}};
    return units_main("hints_list_units", modes, argc, argv);
}
