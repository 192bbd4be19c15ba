// The ten entry points of the resident MSM object (h2v_msm_*, h2v_dual_msm_check_many, h2v_accumulator_add_msms) for the stand-in
// library of tests/cpp/h2v_stub.cpp, linked beside it by tests/test_msm_object_host.py: into a stand-alone sanitizer build of
// tests/cpp/msm_object_harness.cpp, and into a shared library the Python mirror is pointed at through ctypes.  Each call appends a line
// to a log (its name, its scalar arguments, an FNV-1a hash of every input array read with the lengths the call itself passes — so a
// sanitizer build catches a caller that hands over too short a buffer) and prints it, then writes canned outputs of the lengths the call
// promises.  An object is a counter of its terms.  No GPU, no arithmetic.
//   h2v_stub_set_fail(name, rc): from now on the entry point `name` returns rc and does nothing else (null / rc 0: none); the environment
//   variable H2V_STUB_FAIL=name does the same with rc -16 for a program that cannot call it.
//   h2v_stub_take_log(): the log since the last call, as one string.
#include <cstdlib>
#include <cstring>
#include <string>
#include "../../include/h2v.h"
#include "h2v_stub.h"

struct h2v_msm { size_t n; h2v_ctx* ctx; };

namespace {
using h2v_stub::fnv;
std::string g_log, g_taken, g_fail;
int g_fail_rc = 0;
bool g_env_read = false;
std::string arr(const char* name, const void* p, size_t n) {
    char buf[96];
    if (!p) snprintf(buf, sizeof buf, " %s=null", name); else snprintf(buf, sizeof buf, " %s=%zu:%016" PRIx64, name, n, fnv(p, n));
    return buf;
}
std::string num(const char* name, size_t v) { return std::string(" ") + name + "=" + std::to_string(v); }
// an object is named by its number of creation, so that logs do not depend on addresses
size_t g_made = 0;
struct Named { h2v_msm m; size_t id; };
std::string obj(const char* name, const h2v_msm* m) { return std::string(" ") + name + "=" + (m ? "m" + std::to_string(((const Named*)m)->id) + ":" + std::to_string(m->n) : std::string("null")); }
// the line is logged; -> the code the call is told to fail with (0: go on)
int line(const char* name, const std::string& rest) {
    if (!g_env_read) { g_env_read = true; if (const char* e = getenv("H2V_STUB_FAIL")) { g_fail = e; g_fail_rc = -16; } }
    const int rc = g_fail == name ? g_fail_rc : 0;
    const std::string l = std::string(name) + rest + (rc ? " -> " + std::to_string(rc) : std::string());
    g_log += l + "\n";
#ifndef H2V_STUB_QUIET   // (the shared library a test reads the log of)
    printf("%s\n", l.c_str());
#endif
    return rc;
}
}

extern "C" {
void h2v_stub_set_fail(const char* name, int rc) { g_env_read = true; g_fail = name && rc ? name : ""; g_fail_rc = rc; }
const char* h2v_stub_take_log(void) { g_taken.swap(g_log); g_log.clear(); return g_taken.c_str(); }

int h2v_msm_create(h2v_ctx* ctx, h2v_msm** out) {
    if (int rc = line("h2v_msm_create", "")) return rc;
    Named* m = new Named{{0, ctx}, ++g_made};
    *out = &m->m;
    return 0;
}
void h2v_msm_destroy(h2v_msm* m) {
    line("h2v_msm_destroy", obj("m", m));
    delete (Named*)m;
}
int h2v_msm_append_terms(h2v_msm* m, const uint8_t* scalars32, const uint8_t* bases64, size_t n) {
    if (int rc = line("h2v_msm_append_terms", obj("m", m) + num("n", n) + arr("scalars", scalars32, 32 * n) + arr("bases", bases64, 64 * n))) return rc;
    m->n += n;
    return 0;
}
int h2v_msm_add_msm(h2v_msm* dst, const h2v_msm* src) {
    if (int rc = line("h2v_msm_add_msm", obj("dst", dst) + obj("src", src))) return rc;
    if (dst == src) return -16;
    dst->n += src->n;
    return 0;
}
int h2v_msm_scale(h2v_msm* m, const uint8_t factor32[32]) {
    return line("h2v_msm_scale", obj("m", m) + arr("factor", factor32, 32));
}
int h2v_msm_len(const h2v_msm* m, size_t* n) {
    if (int rc = line("h2v_msm_len", obj("m", m))) return rc;
    *n = m->n;
    return 0;
}
int h2v_msm_terms(h2v_msm* m, size_t first, size_t count, uint8_t* scalars32, uint8_t* bases64) {
    if (int rc = line("h2v_msm_terms", obj("m", m) + num("first", first) + num("count", count) + (scalars32 ? " scalars" : "") + (bases64 ? " bases" : ""))) return rc;
    if (first > m->n || count > m->n - first) return -16;
    for (size_t i = 0; scalars32 && i < count; ++i) { memset(scalars32 + 32 * i, 0, 32); scalars32[32 * i] = (uint8_t)(first + i); }   // term i's scalar: its index
    for (size_t i = 0; bases64 && i < count; ++i) memset(bases64 + 64 * i, (int)(0x40 + first + i), 64);
    return 0;
}
int h2v_msm_eval_many(h2v_msm* const* msms, size_t k, uint8_t* out_xy, int* out_is_identity) {
    std::string rest = num("k", k);
    for (size_t i = 0; i < k; ++i) rest += obj("", msms[i]);
    if (int rc = line("h2v_msm_eval_many", rest)) return rc;
    for (size_t i = 0; i < k; ++i) {
        if (out_xy) memset(out_xy + 64 * i, msms[i]->n ? (int)(0x80 + i) : 0, 64);
        if (out_is_identity) out_is_identity[i] = msms[i]->n ? 0 : 1;
    }
    return 0;
}
int h2v_dual_msm_check_many(h2v_msm* const* lefts, h2v_msm* const* rights, size_t k, int* ok, uint8_t* out_left_xy, uint8_t* out_right_xy) {
    std::string rest = num("k", k);
    for (size_t i = 0; i < k; ++i) rest += obj("l", lefts[i]) + obj("r", rights[i]);
    if (int rc = line("h2v_dual_msm_check_many", rest + (out_left_xy ? " lefts" : "") + (out_right_xy ? " rights" : ""))) return rc;
    for (size_t i = 0; i < k; ++i) {
        ok[i] = lefts[i]->n == rights[i]->n ? 1 : 0;   // (a rule a test can steer)
        if (out_left_xy) memset(out_left_xy + 64 * i, (int)(0x10 + i), 64);
        if (out_right_xy) memset(out_right_xy + 64 * i, (int)(0x20 + i), 64);
    }
    return 0;
}
int h2v_accumulator_add_msms(h2v_accumulator* a, h2v_msm* left, h2v_msm* right) {
    return line("h2v_accumulator_add_msms", std::string(a ? " acc" : " acc=null") + obj("left", left) + obj("right", right));
}
}
