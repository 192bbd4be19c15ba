// The one prelude of the kernel unit harnesses (tests/cpp/*_units.hip).  A harness includes it after the library source it tests,
// in its only translation unit.  Here are: the stub behind the library's set_last_error, the checking macros with the programs'
// exit statuses, the cursor over an input file, the output buffer, the file and device helpers, device buffers between guard
// bands, and the main() that every file-reading harness shares.
//
// Exit statuses: 0 done; 2 bad input or usage (before any HIP call where the input is short); 3 a HIP error; 4 a launcher's
// non-zero return code; 5 a guard band overwritten.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <hip/hip_runtime.h>

namespace h2v {
static std::string g_err;
void set_last_error(const std::string& s) { g_err = s; }
}
using namespace h2v;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); exit(3); } } while (0)
#define REQUIRE(c, msg) do { if (!(c)) { fprintf(stderr, "bad input: %s (%s)\n", msg, #c); exit(2); } } while (0)
#define RC(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "%s: %d %s\n", #x, rc_, g_err.c_str()); exit(4); } } while (0)

// ---- files
static std::vector<uint8_t> read_file(const char* path) {
    FILE* f = fopen(path, "rb");
    REQUIRE(f, "cannot open input");
    std::vector<uint8_t> b;
    uint8_t buf[1 << 16];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) b.insert(b.end(), buf, buf + got);
    REQUIRE(!ferror(f) && fclose(f) == 0, "cannot read input");
    return b;
}
static void write_file(const char* path, const void* p, size_t bytes) {
    FILE* f = fopen(path, "wb");
    REQUIRE(f && fwrite(p, 1, bytes, f) == bytes && fclose(f) == 0, "cannot write output");
}

// a cursor over the input file's bytes; every read is checked against what is left
struct In {
    std::vector<uint8_t> b;
    size_t at = 0;
    const char* params = nullptr;   // the PARAMS operand of a mode that takes one
    size_t left() const { return b.size() - at; }
    bool at_end() const { return at == b.size(); }
    const uint8_t* bytes(size_t n) { REQUIRE(n <= left(), "input too short"); const uint8_t* p = b.data() + at; at += n; return p; }
    uint32_t word() { uint32_t w; memcpy(&w, bytes(4), 4); return w; }
    std::vector<uint32_t> words(size_t n) { span_bytes(n, 4); std::vector<uint32_t> v(n); if (n) memcpy(v.data(), bytes(4 * n), 4 * n); return v; }
    // n words where they lie (a file of whole words keeps every read on a word boundary)
    const uint32_t* span(size_t n) { REQUIRE(at % 4 == 0, "words off a word boundary"); return reinterpret_cast<const uint32_t*>(bytes(span_bytes(n, 4))); }
    template <class T> void take(T* out, size_t n) { const size_t sz = span_bytes(n, sizeof(T)); const uint8_t* p = bytes(sz); if (n) memcpy((void*)out, p, sz); }
    // field elements of 32 canonical little-endian bytes
    template <class F> F field() { F v; REQUIRE(F::from_bytes(bytes(32), v), "field element not canonical"); return v; }
    template <class F> std::vector<F> fields(size_t n) { span_bytes(n, 32); std::vector<F> v(n); for (F& x : v) x = field<F>(); return v; }
private:
    size_t span_bytes(size_t n, size_t each) { REQUIRE(n <= left() / each, "input too short"); return n * each; }
};
// the output file's bytes
struct Out {
    std::vector<uint8_t> b;
    std::string path;
    void raw(const void* p, size_t n) { const size_t o = b.size(); b.resize(o + n); if (n) memcpy(&b[o], p, n); }
    void word(uint32_t w) { raw(&w, 4); }
    void words(const std::vector<uint32_t>& v) { raw(v.data(), 4 * v.size()); }
    template <class F> void field(const F& v) { const size_t o = b.size(); b.resize(o + 32); v.to_bytes(&b[o]); }   // 32 canonical bytes
};
static uint32_t job_count(In& in, uint32_t max) { const uint32_t jobs = in.word(); REQUIRE(jobs <= max, "too many jobs"); return jobs; }

// ---- device memory
template <class T> static T* to_device(const T* h, size_t n) {
    T* d = nullptr;
    CK(hipMalloc(&d, (n ? n : 1) * sizeof(T)));
    if (n) CK(hipMemcpy((void*)d, (const void*)h, n * sizeof(T), hipMemcpyHostToDevice));
    return d;
}
template <class T> static std::vector<T> download(const T* d, size_t n) {
    std::vector<T> h(n);
    if (n) CK(hipMemcpy((void*)h.data(), (const void*)d, n * sizeof(T), hipMemcpyDeviceToHost));
    return h;
}
template <class T> static void append(Out& out, const T* d, size_t n) {   // device records -> output bytes
    const std::vector<T> h = download(d, n);
    out.raw(h.data(), n * sizeof(T));
}
// n elements of device memory preset to one byte value between two bands of 0xA5: 128 bytes each, so that p keeps the alignment of
// a G1JSlot.  Whatever reads the elements back checks both bands first: a kernel that wrote past either end ends the program.
template <class T> struct Guarded {
    static constexpr size_t BAND = 128;
    static_assert(BAND % alignof(T) == 0, "elements behind an aligned band");
    uint8_t* base = nullptr;
    T* p = nullptr;
    size_t n = 0;
    explicit Guarded(size_t count, int preset = 0xff) : n(count) {
        CK(hipMalloc(&base, 2 * BAND + n * sizeof(T)));
        CK(hipMemset(base, 0xA5, 2 * BAND + n * sizeof(T)));
        if (n) CK(hipMemset(base + BAND, preset, n * sizeof(T)));
        p = reinterpret_cast<T*>(base + BAND);
    }
    Guarded(const Guarded&) = delete;
    Guarded& operator=(const Guarded&) = delete;
    ~Guarded() { if (base) (void)hipFree(base); }
    // the bands checked, the elements on the host
    std::vector<T> host(const char* what) const {
        const std::vector<uint8_t> h = download(base, 2 * BAND + n * sizeof(T));
        for (size_t i = 0; i < BAND; ++i)
            if (h[i] != 0xA5 || h[BAND + n * sizeof(T) + i] != 0xA5) { fprintf(stderr, "guard band of %s overwritten at byte %zu (%s)\n", what, i, h[i] != 0xA5 ? "before" : "after"); exit(5); }
        std::vector<T> v(n);
        if (n) memcpy((void*)v.data(), h.data() + BAND, n * sizeof(T));
        return v;
    }
    // the bands checked, the first `count` elements (all by default) appended to the output as they lie in memory
    void collect(Out& out, const char* what, size_t count = SIZE_MAX) const { const std::vector<T> v = host(what); out.raw(v.data(), (count < n ? count : n) * sizeof(T)); }
};

// ---- main
// whole_words: the file is uint32 words throughout; params: the mode's operands are PARAMS IN OUT
struct Mode { const char* name; void (*run)(In&, Out&); bool whole_words; bool params; };
// a mode whose file is a job count and then JOB's input that many times
template <void (*JOB)(In&, Out&), uint32_t MAX> static void each_job(In& in, Out& out) { for (uint32_t job = 0, jobs = job_count(in, MAX); job < jobs; ++job) JOB(in, out); }
// PROG MODE [PARAMS] IN OUT: no HIP call before the mode's own first one
template <size_t N> static int units_main(const char* prog, const Mode (&modes)[N], int argc, char** argv) {
    const Mode* m = nullptr;
    for (const Mode& k : modes) if (argc > 1 && std::string(argv[1]) == k.name) m = &k;
    if (!m || argc != (m->params ? 5 : 4)) {
        std::string u = std::string("usage: ") + prog + " ";
        for (size_t i = 0; i < N; ++i) {
            u += modes[i].name;
            if (i + 1 < N && modes[i + 1].params == modes[i].params) u += "|";
            else u += std::string(modes[i].params ? " PARAMS IN OUT" : " IN OUT") + (i + 1 < N ? " | " + std::string(prog) + " " : "");
        }
        fprintf(stderr, "%s\n", u.c_str());
        return 2;
    }
    In in;
    Out out;
    in.params = m->params ? argv[2] : nullptr;
    in.b = read_file(argv[argc - 2]);
    out.path = argv[argc - 1];
    REQUIRE(!m->whole_words || in.b.size() % 4 == 0, "input is not whole words");
    m->run(in, out);
    REQUIRE(in.at_end(), "input longer than its jobs");
    write_file(out.path.c_str(), out.b.data(), out.b.size());
    return 0;
}
