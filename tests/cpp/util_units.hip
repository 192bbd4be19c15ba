// The record, byte-conversion and small group kernels (halo2_verifier_amd/csrc/util.hip) one by one, each through the library's own
// *_enqueue launcher, on inputs chosen by tests/test_gpu_record_units.py.  Built with the library's flags by
// halo2_verifier_amd/csrc/Makefile (build/util_units).
//
//   util_units fold        IN OUT   k_fold_records: per job one fold over records given word for word
//   util_units export      IN OUT   k_export_records: from whole points or from pieces, with or without a status array
//   util_units to_bytes    IN OUT   k_point_to_bytes, with or without the LDS request of the auxiliary stream
//   util_units bases       IN OUT   k_bases_from_bytes
//   util_units scalars     IN OUT   k_scalars_from_bytes
//   util_units to_jacobian IN OUT   k_affine_to_jacobian
//   util_units copy        IN OUT   k_copy_words, with or without the LDS request
// Files are little-endian uint32 words; the layouts are in the readers below.  Points and records are raw 29-bit limbs as they lie
// in memory (the Python side picks every representative).  Every output buffer is preset to 0xff and lies between two bands of
// 0xA5 (at least 32 bytes each) that are checked after the kernel: a write past an output ends the program with status 5.  Every HIP
// call is checked: the first error ends the program with a non-zero status.  Every count, offset and index that reaches a kernel is
// checked on the host first, and a record whose shift exceeds 1024 is refused: k_fold_records doubles a foreign record shift times
// per piece, and no input may turn that into a long-running kernel.
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
#define MAX_SHIFT 1024u

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
template <class T> static T* to_device(const T* h, size_t n) {
    T* d = nullptr;
    CK(hipMalloc(&d, (n ? n : 1) * sizeof(T)));
    if (n) CK(hipMemcpy((void*)d, (const void*)h, n * sizeof(T), hipMemcpyHostToDevice));
    return d;
}
// a cursor over the input words
struct Words {
    const std::vector<uint32_t>& w;
    size_t at = 0;
    uint32_t next() { REQUIRE(at < w.size(), "input too short"); return w[at++]; }
    const uint32_t* span(size_t words) { REQUIRE(words <= w.size() - at, "input too short"); const uint32_t* p = w.data() + at; at += words; return p; }
    template <class T> void take(T* out, size_t n) { static_assert(sizeof(T) % 4 == 0, "word records"); memcpy((void*)out, span(n * sizeof(T) / 4), n * sizeof(T)); }
};
// n elements of device memory preset to 0xff between two bands of 0xA5: 128 bytes each, so that p keeps the alignment of a G1JSlot
template <class T> struct Guarded {
    static constexpr size_t BAND = 128;
    static_assert(sizeof(T) % 4 == 0 && BAND >= 32 && BAND % alignof(T) == 0, "word records behind an aligned band");
    uint8_t* base = nullptr;
    T* p = nullptr;
    size_t n = 0;
    explicit Guarded(size_t count) : n(count) {
        CK(hipMalloc(&base, 2 * BAND + n * sizeof(T)));
        CK(hipMemset(base, 0xA5, 2 * BAND + n * sizeof(T)));
        if (n) CK(hipMemset(base + BAND, 0xff, n * sizeof(T)));
        p = reinterpret_cast<T*>(base + BAND);
    }
    Guarded(const Guarded&) = delete;
    Guarded& operator=(const Guarded&) = delete;
    // the bands checked, the elements appended to the output words
    void collect(std::vector<uint32_t>& out, const char* what) {
        std::vector<uint8_t> h(2 * BAND + n * sizeof(T));
        CK(hipMemcpy(h.data(), base, h.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < BAND; ++i)
            if (h[i] != 0xA5 || h[BAND + n * sizeof(T) + i] != 0xA5) { fprintf(stderr, "guard band of %s overwritten at byte %zu (%s)\n", what, i, h[i] != 0xA5 ? "before" : "after"); exit(5); }
        const size_t o = out.size(), words = n * sizeof(T) / 4;
        out.resize(o + words);
        if (words) memcpy(out.data() + o, h.data() + BAND, words * 4);
    }
    ~Guarded() { if (base) (void)hipFree(base); }
};
static uint32_t job_count(Words& in) { const uint32_t jobs = in.next(); REQUIRE(jobs <= 256, "too many jobs"); return jobs; }

// ---- fold
// IN: n_jobs; per job: n_recs, groups, parts, shift, with_pieces (0: d_pieces = d_ready = nullptr), n_recs * groups records ([i][g], 328 words each)
// OUT per job: the parts the launcher folded into; acc (2 groups points of 27 words); (parts > 1) pieces, then ready (2 groups parts slots of 32
//     words each); fold_failed (groups words)
static void run_fold(Words& in, std::vector<uint32_t>& out) {
    for (uint32_t job = 0, jobs = job_count(in); job < jobs; ++job) {
        const uint32_t n_recs = in.next(), groups = in.next(), parts = in.next(), shift = in.next(), with_pieces = in.next();
        REQUIRE(n_recs >= 1 && n_recs <= 256 && groups >= 1 && groups <= 64, "bad fold job");
        REQUIRE(parts >= 1 && parts <= H2V_ACC_RECORD_PIECES && shift <= MAX_SHIFT && with_pieces <= 1, "bad fold split");
        std::vector<AccRecord> recs((size_t)n_recs * groups);
        in.take(recs.data(), recs.size());
        for (const AccRecord& r : recs) REQUIRE(r.shift <= MAX_SHIFT, "record shift above 1024: refused");   // (parts is the kernel's to judge)
        const uint32_t eff = parts > 1 && with_pieces ? parts : 1;
        AccRecord* d_recs = to_device(recs.data(), recs.size());
        Guarded<G1J> acc((size_t)2 * groups);
        Guarded<G1JSlot> pieces(eff > 1 ? (size_t)2 * groups * eff : 0), ready(eff > 1 ? (size_t)2 * groups * eff : 0);
        Guarded<uint32_t> failed(groups);
        RC(fold_records_enqueue(0, d_recs, n_recs, groups, parts, shift, acc.p, eff > 1 ? pieces.p : nullptr, eff > 1 ? ready.p : nullptr, failed.p));
        CK(hipDeviceSynchronize());
        out.push_back(eff);
        acc.collect(out, "acc"); pieces.collect(out, "pieces"); ready.collect(out, "ready"); failed.collect(out, "fold_failed");
        CK(hipFree(d_recs));
    }
}

// ---- export
// IN: n_jobs; per job: groups, gs (proofs per group), parts, shift, from_pieces, with_status; the points (27 words each): 2 groups whole points, or
//     2 groups parts pieces ([(2g + side) parts + j]); (with_status) groups * gs status words
// OUT per job: groups records (328 words each)
static void run_export(Words& in, std::vector<uint32_t>& out) {
    for (uint32_t job = 0, jobs = job_count(in); job < jobs; ++job) {
        const uint32_t groups = in.next(), gs = in.next(), parts = in.next(), shift = in.next(), from_pieces = in.next(), with_status = in.next();
        REQUIRE(groups >= 1 && groups <= 64 && gs <= 4096 && from_pieces <= 1 && with_status <= 1, "bad export job");
        REQUIRE(parts >= 1 && parts <= H2V_ACC_RECORD_PIECES && shift <= MAX_SHIFT, "bad export split");
        REQUIRE(with_status ? gs >= 1 : gs == 0, "a status array holds gs >= 1 words per group; without one gs = 0");
        const size_t n_pts = (size_t)2 * groups * (from_pieces ? parts : 1);
        std::vector<G1J> pts(n_pts);
        in.take(pts.data(), n_pts);
        std::vector<G1JSlot> slots(n_pts);
        for (size_t i = 0; i < n_pts; ++i) slots[i] = pts[i];
        G1J* d_acc = from_pieces ? nullptr : to_device(pts.data(), n_pts);
        G1JSlot* d_pieces = from_pieces ? to_device(slots.data(), n_pts) : nullptr;
        int* d_status = with_status ? to_device(reinterpret_cast<const int*>(in.span((size_t)groups * gs)), (size_t)groups * gs) : nullptr;
        Guarded<AccRecord> recs(groups);
        RC(export_records_enqueue(0, d_acc, d_pieces, parts, shift, d_status, groups * gs, groups, recs.p));
        CK(hipDeviceSynchronize());
        recs.collect(out, "records");
        if (d_acc) CK(hipFree(d_acc));
        if (d_pieces) CK(hipFree(d_pieces));
        if (d_status) CK(hipFree(d_status));
    }
}

// ---- to_bytes
// IN: n_jobs; per job: n, reserve (1: lds_reserve = H2V_AUX_LDS_RESERVE), n points (27 words)
// OUT per job: n * 16 words of x | y bytes, n identity flags
static void run_to_bytes(Words& in, std::vector<uint32_t>& out) {
    for (uint32_t job = 0, jobs = job_count(in); job < jobs; ++job) {
        const uint32_t n = in.next(), reserve = in.next();
        REQUIRE(n <= 4096 && reserve <= 1, "bad to_bytes job");
        std::vector<G1J> pts(n);
        in.take(pts.data(), n);
        G1J* d_in = to_device(pts.data(), n);
        Guarded<uint32_t> bytes((size_t)16 * n), flags(n);
        RC(point_to_bytes_enqueue(0, d_in, reinterpret_cast<uint8_t*>(bytes.p), flags.p, n, reserve ? H2V_AUX_LDS_RESERVE : 0));
        CK(hipDeviceSynchronize());
        bytes.collect(out, "bytes"); flags.collect(out, "identity flags");
        CK(hipFree(d_in));
    }
}

// ---- bases
// IN: n_jobs; per job: n, n * 16 words of x | y bytes
// OUT per job: n affine points (18 words: x, y), n flags
static void run_bases(Words& in, std::vector<uint32_t>& out) {
    for (uint32_t job = 0, jobs = job_count(in); job < jobs; ++job) {
        const uint32_t n = in.next();
        REQUIRE(n <= 4096, "bad bases job");
        uint32_t* d_in = to_device(in.span((size_t)16 * n), (size_t)16 * n);
        Guarded<G1A> pts(n);
        Guarded<uint32_t> flags(n);
        RC(bases_from_bytes_enqueue(0, reinterpret_cast<const uint8_t*>(d_in), pts.p, flags.p, n));
        CK(hipDeviceSynchronize());
        pts.collect(out, "bases"); flags.collect(out, "flags");
        CK(hipFree(d_in));
    }
}

// ---- scalars
// IN: n_jobs; per job: n, n * 8 words of scalar bytes
// OUT per job: n * 8 words, n flags
static void run_scalars(Words& in, std::vector<uint32_t>& out) {
    for (uint32_t job = 0, jobs = job_count(in); job < jobs; ++job) {
        const uint32_t n = in.next();
        REQUIRE(n <= 4096, "bad scalars job");
        uint32_t* d_in = to_device(in.span((size_t)8 * n), (size_t)8 * n);
        Guarded<uint32_t> words((size_t)8 * n), flags(n);
        RC(scalars_from_bytes_enqueue(0, reinterpret_cast<const uint8_t*>(d_in), words.p, flags.p, n));
        CK(hipDeviceSynchronize());
        words.collect(out, "scalar words"); flags.collect(out, "flags");
        CK(hipFree(d_in));
    }
}

// ---- to_jacobian
// IN: n_jobs; per job: n, n affine points (18 words);  OUT per job: n Jacobian points (27 words)
static void run_to_jacobian(Words& in, std::vector<uint32_t>& out) {
    for (uint32_t job = 0, jobs = job_count(in); job < jobs; ++job) {
        const uint32_t n = in.next();
        REQUIRE(n <= 4096, "bad to_jacobian job");
        std::vector<G1A> pts(n);
        in.take(pts.data(), n);
        G1A* d_in = to_device(pts.data(), n);
        Guarded<G1J> res(n);
        RC(affine_to_jacobian_enqueue(0, d_in, res.p, n));
        CK(hipDeviceSynchronize());
        res.collect(out, "points");
        CK(hipFree(d_in));
    }
}

// ---- copy
// IN: n_jobs; per job: n_words, reserve, n_words words;  OUT per job: n_words words
static void run_copy(Words& in, std::vector<uint32_t>& out) {
    for (uint32_t job = 0, jobs = job_count(in); job < jobs; ++job) {
        const uint32_t n = in.next(), reserve = in.next();
        REQUIRE(n <= (1u << 20) && reserve <= 1, "bad copy job");
        uint32_t* d_in = to_device(in.span(n), n);
        Guarded<uint32_t> dst(n);
        RC(copy_words_enqueue(0, d_in, dst.p, n, reserve ? H2V_AUX_LDS_RESERVE : 0));
        CK(hipDeviceSynchronize());
        dst.collect(out, "words");
        CK(hipFree(d_in));
    }
}

int main(int argc, char** argv) {
    REQUIRE(argc == 4, "usage: util_units fold|export|to_bytes|bases|scalars|to_jacobian|copy IN OUT");
    const std::string mode = argv[1];
    const std::vector<uint32_t> words = slurp_words(argv[2]);
    Words in{words};
    std::vector<uint32_t> out;
    if (mode == "fold") run_fold(in, out);
    else if (mode == "export") run_export(in, out);
    else if (mode == "to_bytes") run_to_bytes(in, out);
    else if (mode == "bases") run_bases(in, out);
    else if (mode == "scalars") run_scalars(in, out);
    else if (mode == "to_jacobian") run_to_jacobian(in, out);
    else if (mode == "copy") run_copy(in, out);
    else REQUIRE(false, "unknown mode");
    REQUIRE(in.at == words.size(), "input longer than its jobs");
    spill(argv[3], out);
    return 0;
}
