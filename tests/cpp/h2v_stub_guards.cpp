// The Guard entry points of include/h2v.h for the stand-in library of tests/cpp/h2v_stub.cpp (linked beside it by
// tests/test_guards_host.py): each prints its name, its scalar arguments and an FNV-1a hash of every input array, read with the
// lengths the call's own counts give — so a sanitizer build catches a mirror that hands over too short a buffer — and writes canned
// verdicts.  No GPU, no arithmetic.
#include "../../include/h2v.h"
#include "h2v_stub.h"

namespace {
using h2v_stub::bytes;
void guards(size_t n, const size_t* lc, const size_t* rc, const uint8_t* ls, const uint8_t* lb, const uint8_t* rs, const uint8_t* rb) {
    size_t nl = 0, nr = 0;
    for (size_t i = 0; i < n; ++i) { nl += lc[i]; nr += rc[i]; }
    printf(" n=%zu", n);
    bytes("left_counts", lc, sizeof(size_t) * n); bytes("right_counts", rc, sizeof(size_t) * n);
    bytes("ls", ls, 32 * nl); bytes("lb", lb, 64 * nl); bytes("rs", rs, 32 * nr); bytes("rb", rb, 64 * nr);
}
}

extern "C" {
int h2v_accumulator_process_guards(h2v_accumulator* a, size_t n, const size_t* lc, const size_t* rc, const uint8_t* ls, const uint8_t* lb, const uint8_t* rs,
                                   const uint8_t* rb, const uint8_t* rand32) {
    printf("h2v_accumulator_process_guards acc=%p", (void*)a); guards(n, lc, rc, ls, lb, rs, rb); bytes("rand", rand32, 32 * n); printf("\n");
    return 0;
}
int h2v_guards_check_each(h2v_ctx* ctx, size_t n, const size_t* lc, const size_t* rc, const uint8_t* ls, const uint8_t* lb, const uint8_t* rs, const uint8_t* rb,
                          int* guard_ok) {
    printf("h2v_guards_check_each ctx=%p", (void*)ctx); guards(n, lc, rc, ls, lb, rs, rb); printf("\n");
    for (size_t i = 0; i < n; ++i) guard_ok[i] = (int)(i % 3 != 1);
    return 0;
}
}
