// The staged-batch entry points that tests/cpp/batch_legs_harness.cpp calls, and h2v_accumulator_process_batch, for the stand-in library
// of tests/cpp/h2v_stub.cpp (linked beside it by tests/test_accumulator_batch_host.py): each prints its name, its scalar arguments and
// an FNV-1a hash of every input array, read with the lengths the call itself passes — so a sanitizer build catches a caller that hands
// over too short a buffer — and writes canned outputs of the lengths the call promises.  No GPU, no arithmetic.
#include <cstring>
#include "../../include/h2v.h"
#include "h2v_stub.h"

namespace {
using h2v_stub::bytes;
size_t batch_n = 0, batch_groups = 1;
}

extern "C" {
int h2v_batch_create(h2v_ctx* ctx, size_t max_proofs, size_t max_inst, h2v_batch** out) {
    *out = (h2v_batch*)(uintptr_t)0xb000;
    printf("h2v_batch_create ctx=%p max_proofs=%zu max_inst=%zu -> %p\n", (void*)ctx, max_proofs, max_inst, (void*)*out);
    return 0;
}
void h2v_batch_destroy(h2v_batch* b) { printf("h2v_batch_destroy batch=%p\n", (void*)b); }
int h2v_batch_set_group_sizes(h2v_batch* b, const size_t* sizes, size_t n_groups) {
    printf("h2v_batch_set_group_sizes batch=%p sizes=[", (void*)b);
    for (size_t g = 0; g < n_groups; ++g) printf(g ? ",%zu" : "%zu", sizes[g]);
    printf("]\n");
    batch_groups = n_groups;
    return 0;
}
int h2v_batch_upload(h2v_batch* b, size_t n, const uint8_t* proofs_flat, size_t proof_len, const uint8_t* instances_flat, size_t ncols, const size_t* col_lens,
                     const uint8_t* rand_tail, size_t n_tail) {
    size_t ninst = 0;
    for (size_t c = 0; c < ncols; ++c) ninst += col_lens[c];
    printf("h2v_batch_upload batch=%p n=%zu proof_len=%zu ncols=%zu n_tail=%zu", (void*)b, n, proof_len, ncols, n_tail);
    bytes("proofs", proofs_flat, n * proof_len); bytes("inst", instances_flat, 32 * n * ninst); bytes("tail", rand_tail, 32 * n_tail);
    printf("\n");
    batch_n = n;
    return 0;
}
int h2v_batch_launch(h2v_batch* b, int with_pairing) { printf("h2v_batch_launch batch=%p with_pairing=%d\n", (void*)b, with_pairing); return 0; }
int h2v_batch_finish_groups(h2v_batch* b, int* st, int* group_ok, uint8_t* left, uint8_t* right, size_t n_groups) {
    printf("h2v_batch_finish_groups batch=%p n_groups=%zu\n", (void*)b, n_groups);
    for (size_t i = 0; st && i < batch_n; ++i) st[i] = 0;
    for (size_t g = 0; g < n_groups; ++g) group_ok[g] = 1;
    if (left) memset(left, 0x11, 64 * n_groups);
    if (right) memset(right, 0x22, 64 * n_groups);
    return 0;
}
int h2v_accumulator_process_batch(h2v_accumulator* a, h2v_batch* b, size_t* n_proofs_added, size_t* n_failed_added) {
    printf("h2v_accumulator_process_batch acc=%p batch=%p added=%s,%s\n", (void*)a, (void*)b, n_proofs_added ? "asked" : "null", n_failed_added ? "asked" : "null");
    if (n_proofs_added) *n_proofs_added = batch_n;
    if (n_failed_added) *n_failed_added = batch_groups > 2 ? 1 : 0;
    return 0;
}
}
