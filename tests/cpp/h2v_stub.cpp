// A stand-in for the library behind include/h2v.h, for tests/cpp/mirror_trace.cpp: exactly the h2v_* symbols include/h2v.hpp calls.
// Every one prints its name, its scalar arguments and an FNV-1a hash of every input array (read with the lengths the call itself
// passes, so a sanitizer build catches a mirror that hands over too short a buffer), then writes canned outputs.  No GPU, no arithmetic.
#include <cstring>
#include "../../include/h2v.h"
#include "h2v_stub.h"

namespace {
using h2v_stub::bytes;
void sizes(const char* name, const size_t* p, size_t n) {
    printf(" %s=[", name);
    for (size_t i = 0; p && i < n; ++i) printf(i ? ",%zu" : "%zu", p[i]);
    printf("]");
}
size_t sum(const size_t* p, size_t n) { size_t s = 0; for (size_t i = 0; i < n; ++i) s += p[i]; return s; }
uintptr_t handles = 0;
void* next_handle() { return (void*)(uintptr_t)(0x1000 * ++handles); }
void point(uint8_t* out, uint8_t from) { if (out) for (int j = 0; j < 64; ++j) out[j] = (uint8_t)(from + j); }
void statuses(int* st, size_t n) { for (size_t i = 0; i < n; ++i) st[i] = i % 2 ? -2 : 0; }

// the proofs of a call whose proofs share one shape (per_proof = false) or bring ncols column lengths each
void one_key(const char* name, h2v_ctx* ctx, size_t n, const uint8_t* const* proofs, const size_t* lens, const uint8_t* const* insts, size_t ncols,
             const size_t* col_lens, bool per_proof, const uint8_t* rand32) {
    printf("%s ctx=%p n=%zu ncols=%zu", name, (void*)ctx, n, ncols);
    sizes("col_lens", col_lens, per_proof ? n * ncols : ncols);
    bytes("rand", rand32, 32 * n);
    for (size_t i = 0; i < n; ++i) {
        bytes("proof", proofs[i], lens[i]);
        bytes("inst", insts[i], 32 * sum(col_lens + (per_proof ? i * ncols : 0), ncols));
    }
}
void keyed(const char* name, void* acc, h2v_ctx* const* ctxs, size_t n_keys, const uint32_t* key_of, size_t n, const uint8_t* const* proofs, const size_t* lens,
           const uint8_t* const* insts, const size_t* ncols, const size_t* col_lens, const uint8_t* rand32) {
    printf("%s acc=%p n_keys=%zu ctxs=[", name, acc, n_keys);
    for (size_t k = 0; k < n_keys; ++k) printf(k ? ",%p" : "%p", (void*)ctxs[k]);
    printf("] n=%zu", n);
    sizes("ncols", ncols, n_keys);
    bytes("rand", rand32, 32 * n);
    for (size_t i = 0, at = 0; i < n; at += ncols[key_of[i]], ++i) {
        printf(" key=%u", key_of[i]);
        sizes("col_lens", col_lens + at, ncols[key_of[i]]);
        bytes("proof", proofs[i], lens[i]);
        bytes("inst", insts[i], 32 * sum(col_lens + at, ncols[key_of[i]]));
    }
}
void seed(const uint8_t* ls, const uint8_t* lb, size_t nl, const uint8_t* rs, const uint8_t* rb, size_t nr) {
    printf(" n_left=%zu n_right=%zu", nl, nr);
    bytes("left_scalars", ls, 32 * nl); bytes("left_bases", lb, 64 * nl); bytes("right_scalars", rs, 32 * nr); bytes("right_bases", rb, 64 * nr);
}
void ranges(size_t k, const uint32_t* bor, const size_t* first, const size_t* count, int* ok, uint8_t* left, uint8_t* right) {
    printf(" n_ranges=%zu", k);
    if (bor) { printf(" batch_of=["); for (size_t i = 0; i < k; ++i) printf(i ? ",%u" : "%u", bor[i]); printf("]"); }
    sizes("first", first, k); sizes("count", count, k);
    printf(" lefts=%s rights=%s\n", left ? "given" : "null", right ? "given" : "null");
    for (size_t i = 0; i < k; ++i) { ok[i] = i % 2 ? 0 : 1; point(left ? left + 64 * i : nullptr, (uint8_t)(3 * i)); point(right ? right + 64 * i : nullptr, (uint8_t)(5 * i + 1)); }
}
}  // namespace

extern "C" {
const char* h2v_last_error(void) { return "stub"; }
int h2v_ctx_create_ex(const uint8_t* params, size_t params_len, int params_format, const uint8_t* vk, size_t vk_len, int vk_format, int device,
                      const h2v_options* o, h2v_ctx** out) {
    *out = (h2v_ctx*)next_handle();
    printf("h2v_ctx_create_ex params_format=%d vk_format=%d device=%d options=%zu,%d,%d,%d,%d", params_format, vk_format, device, o->struct_size, o->multiopen,
           o->transcript, o->circuit_instances, o->instance_kernel_threshold);
    bytes("params", params, params_len); bytes("vk", vk, vk_len);
    printf(" -> %p\n", (void*)*out);
    return 0;
}
void h2v_ctx_destroy(h2v_ctx* ctx) { printf("h2v_ctx_destroy ctx=%p\n", (void*)ctx); }
int h2v_ctx_proof_shape(const h2v_ctx* ctx, size_t* proof_len, size_t* n_points, size_t* n_scalars, size_t* n_right_terms, size_t* n_instance_columns) {
    printf("h2v_ctx_proof_shape ctx=%p asked=%d%d%d%d%d\n", (const void*)ctx, !!proof_len, !!n_points, !!n_scalars, !!n_right_terms, !!n_instance_columns);
    if (proof_len) *proof_len = 96;
    if (n_points) *n_points = 3;
    if (n_scalars) *n_scalars = 4;
    if (n_right_terms) *n_right_terms = 5;
    if (n_instance_columns) *n_instance_columns = 2;
    return 0;
}
int h2v_verify_batch(h2v_ctx* ctx, size_t n, const uint8_t* const* proofs, const size_t* lens, const uint8_t* const* insts, size_t ncols, const size_t* col_lens,
                     const uint8_t* rand32, int* st, int* ok, uint8_t* left, uint8_t* right) {
    one_key("h2v_verify_batch", ctx, n, proofs, lens, insts, ncols, col_lens, false, rand32); printf("\n");
    statuses(st, n); *ok = 1; point(left, 0); point(right, 64);
    return 0;
}
int h2v_verify_batch_shapes(h2v_ctx* ctx, size_t n, const uint8_t* const* proofs, const size_t* lens, const uint8_t* const* insts, size_t ncols,
                            const size_t* col_lens, const uint8_t* rand32, int* st, int* ok, uint8_t* left, uint8_t* right) {
    one_key("h2v_verify_batch_shapes", ctx, n, proofs, lens, insts, ncols, col_lens, true, rand32); printf("\n");
    statuses(st, n); *ok = 0; point(left, 1); point(right, 65);
    return 0;
}
int h2v_verify_batch_keys(h2v_ctx* const* ctxs, size_t n_keys, const uint32_t* key_of, size_t n, const uint8_t* const* proofs, const size_t* lens,
                          const uint8_t* const* insts, const size_t* ncols, const size_t* col_lens, const uint8_t* rand32, int* st, int* ok, uint8_t* left,
                          uint8_t* right) {
    keyed("h2v_verify_batch_keys", nullptr, ctxs, n_keys, key_of, n, proofs, lens, insts, ncols, col_lens, rand32); printf("\n");
    statuses(st, n); *ok = 1; point(left, 2); point(right, 66);
    return 0;
}
int h2v_verify_batch_seeded(h2v_ctx* ctx, size_t n, const uint8_t* const* proofs, const size_t* lens, const uint8_t* const* insts, size_t ncols,
                            const size_t* col_lens, const uint8_t* rand32, const uint8_t* ls, const uint8_t* lb, size_t nl, const uint8_t* rs, const uint8_t* rb,
                            size_t nr, int* st, int* ok, uint8_t* left, uint8_t* right) {
    one_key("h2v_verify_batch_seeded", ctx, n, proofs, lens, insts, ncols, col_lens, false, rand32); seed(ls, lb, nl, rs, rb, nr); printf("\n");
    statuses(st, n); *ok = 1; point(left, 3); point(right, 67);
    return 0;
}
int h2v_verify_each(h2v_ctx* ctx, size_t n, const uint8_t* const* proofs, const size_t* lens, const uint8_t* const* insts, size_t ncols, const size_t* col_lens,
                    int* st) {
    one_key("h2v_verify_each", ctx, n, proofs, lens, insts, ncols, col_lens, false, nullptr); printf("\n");
    for (size_t i = 0; i < n; ++i) st[i] = -4;
    return 0;
}
int h2v_verify_batch_identify(h2v_ctx* ctx, size_t n, const uint8_t* const* proofs, const size_t* lens, const uint8_t* const* insts, size_t ncols,
                              const size_t* col_lens, const uint8_t* rand32, int* st, int* ok, uint8_t* left, uint8_t* right, size_t* checks) {
    one_key("h2v_verify_batch_identify", ctx, n, proofs, lens, insts, ncols, col_lens, false, rand32); printf(" checks=%s\n", checks ? "asked" : "null");
    statuses(st, n); *ok = 0; point(left, 4); point(right, 68);
    if (checks) *checks = 7;
    return 0;
}
int h2v_verify_batch_keys_identify(h2v_ctx* const* ctxs, size_t n_keys, const uint32_t* key_of, size_t n, const uint8_t* const* proofs, const size_t* lens,
                                   const uint8_t* const* insts, const size_t* ncols, const size_t* col_lens, const uint8_t* rand32, int* st, int* ok,
                                   uint8_t* left, uint8_t* right, size_t* checks) {
    keyed("h2v_verify_batch_keys_identify", nullptr, ctxs, n_keys, key_of, n, proofs, lens, insts, ncols, col_lens, rand32);
    printf(" checks=%s\n", checks ? "asked" : "null");
    statuses(st, n); *ok = 0; point(left, 5); point(right, 69);
    if (checks) *checks = 9;
    return 0;
}
int h2v_verify_batch_seeded_identify(h2v_ctx* ctx, size_t n, const uint8_t* const* proofs, const size_t* lens, const uint8_t* const* insts, size_t ncols,
                                     const size_t* col_lens, const uint8_t* rand32, const uint8_t* ls, const uint8_t* lb, size_t nl, const uint8_t* rs,
                                     const uint8_t* rb, size_t nr, int* st, int* ok, int* seed_ok, uint8_t* left, uint8_t* right, size_t* checks) {
    one_key("h2v_verify_batch_seeded_identify", ctx, n, proofs, lens, insts, ncols, col_lens, false, rand32); seed(ls, lb, nl, rs, rb, nr);
    printf(" seed_ok=%s checks=%s\n", seed_ok ? "asked" : "null", checks ? "asked" : "null");
    statuses(st, n); *ok = 0; point(left, 6); point(right, 70);
    if (seed_ok) *seed_ok = 0;
    if (checks) *checks = 11;
    return 0;
}
int h2v_accumulator_create(h2v_ctx* ctx, h2v_accumulator** out) {
    *out = (h2v_accumulator*)next_handle();
    printf("h2v_accumulator_create ctx=%p -> %p\n", (void*)ctx, (void*)*out);
    return 0;
}
void h2v_accumulator_destroy(h2v_accumulator* a) { printf("h2v_accumulator_destroy acc=%p\n", (void*)a); }
int h2v_accumulator_process(h2v_accumulator* a, h2v_ctx* const* ctxs, size_t n_keys, const uint32_t* key_of, size_t n, const uint8_t* const* proofs,
                            const size_t* lens, const uint8_t* const* insts, const size_t* ncols, const size_t* col_lens, const uint8_t* rand32, int* st,
                            int* all_ok) {
    keyed("h2v_accumulator_process", a, ctxs, n_keys, key_of, n, proofs, lens, insts, ncols, col_lens, rand32); printf("\n");
    statuses(st, n); *all_ok = n < 2;
    return 0;
}
int h2v_accumulator_add_msm(h2v_accumulator* a, const uint8_t* ls, const uint8_t* lb, size_t nl, const uint8_t* rs, const uint8_t* rb, size_t nr) {
    printf("h2v_accumulator_add_msm acc=%p", (void*)a); seed(ls, lb, nl, rs, rb, nr); printf("\n");
    return 0;
}
int h2v_accumulator_read(h2v_accumulator* a, uint8_t* left, uint8_t* right, size_t* n_proofs, size_t* n_failed) {
    printf("h2v_accumulator_read acc=%p\n", (void*)a);
    point(left, 7); point(right, 71); *n_proofs = 6; *n_failed = 1;
    return 0;
}
int h2v_accumulator_finalize(h2v_accumulator* a, int* ok, uint8_t* left, uint8_t* right) {
    printf("h2v_accumulator_finalize acc=%p\n", (void*)a);
    *ok = 1; point(left, 8); point(right, 72);
    return 0;
}
int h2v_accumulator_journal_begin(h2v_accumulator* a, size_t capacity) { printf("h2v_accumulator_journal_begin acc=%p capacity=%zu\n", (void*)a, capacity); return 0; }
int h2v_accumulator_check_legs(h2v_accumulator* a, size_t cap, size_t* n_legs, size_t* leg_proofs, size_t* leg_failed, int* leg_ok) {
    printf("h2v_accumulator_check_legs acc=%p cap=%zu arrays=%d%d%d\n", (void*)a, cap, !!leg_proofs, !!leg_failed, !!leg_ok);
    static const size_t proofs[3] = {0, 2, 0}, failed[3] = {0, 1, 0};
    static const int ok[3] = {1, 0, 0};
    *n_legs = 3;
    for (size_t e = 0; e < 3 && e < cap; ++e) {
        if (leg_proofs) leg_proofs[e] = proofs[e];
        if (leg_failed) leg_failed[e] = failed[e];
        if (leg_ok) leg_ok[e] = ok[e];
    }
    return 0;
}
int h2v_accumulator_drop_legs(h2v_accumulator* a, const size_t* legs, size_t n_drop) {
    printf("h2v_accumulator_drop_legs acc=%p", (void*)a); sizes("legs", legs, n_drop); printf("\n");
    return 0;
}
int h2v_batch_recheck(h2v_batch* b, size_t k, const size_t* first, const size_t* count, int* ok, uint8_t* left, uint8_t* right) {
    printf("h2v_batch_recheck batch=%p", (void*)b); ranges(k, nullptr, first, count, ok, left, right);
    return 0;
}
int h2v_batches_recheck(h2v_batch* const* batches, size_t n_batches, size_t k, const uint32_t* bor, const size_t* first, const size_t* count, int* ok,
                        uint8_t* left, uint8_t* right) {
    printf("h2v_batches_recheck batches=[");
    for (size_t i = 0; i < n_batches; ++i) printf(i ? ",%p" : "%p", (void*)batches[i]);
    printf("]"); ranges(k, bor, first, count, ok, left, right);
    return 0;
}
}
