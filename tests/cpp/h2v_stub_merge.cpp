// The merge entry points of include/h2v.h for the stand-in library of tests/cpp/h2v_stub.cpp (linked beside it by
// tests/test_accumulator_merge_host.py): each prints its name, its scalar arguments and an FNV-1a hash of every input array, read
// with the lengths the call itself passes — so a sanitizer build catches a mirror that hands over too short a buffer — and writes
// canned outputs.  No GPU, no arithmetic.
#include <cstring>
#include "../../include/h2v.h"
#include "h2v_stub.h"

namespace {
using h2v_stub::bytes;
void draws_out(uint8_t* out, size_t n) { if (out) for (size_t i = 0; i < 32 * n; ++i) out[i] = (uint8_t)(0xd0 + i % 16); }
}

extern "C" {
int h2v_accumulator_merge(h2v_accumulator* dst, h2v_accumulator* const* srcs, size_t n_src, const uint8_t* draws32, uint8_t* out_draws32) {
    printf("h2v_accumulator_merge acc=%p srcs=[", (void*)dst);
    for (size_t k = 0; k < n_src; ++k) printf(k ? ",%p" : "%p", (void*)srcs[k]);
    printf("]"); bytes("draws", draws32, 32 * n_src); printf(" out=%s\n", out_draws32 ? "asked" : "null");
    draws_out(out_draws32, n_src);
    return 0;
}
int h2v_accumulator_export_state(h2v_accumulator* a, uint8_t* out) {
    printf("h2v_accumulator_export_state acc=%p\n", (void*)a);
    for (int i = 0; i < H2V_ACC_STATE_BYTES; ++i) out[i] = (uint8_t)(i + (int)((uintptr_t)a >> 12));
    return 0;
}
int h2v_accumulator_merge_states(h2v_accumulator* dst, const uint8_t* states, size_t n, const uint8_t* draws32, uint8_t* out_draws32) {
    printf("h2v_accumulator_merge_states acc=%p n=%zu", (void*)dst, n);
    bytes("states", states, (size_t)H2V_ACC_STATE_BYTES * n); bytes("draws", draws32, 32 * n); printf(" out=%s\n", out_draws32 ? "asked" : "null");
    draws_out(out_draws32, n);
    return 0;
}
}
