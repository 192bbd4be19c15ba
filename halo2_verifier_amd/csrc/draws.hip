// Draws from a seed (include/h2v_draws.h): the host twin of k_expand_draws (verify_kernels.hip) and the two entry points.
//
//   draw(seed, i) = LE512(BLAKE2b-512(seed[32] | LE64(i), no key, personal "h2v-draws-v1" | 0 x 4)) mod r, 32 canonical bytes
//
// The host side has a BLAKE2b of its own, written from RFC 7693 for the one shape it needs: a 40-byte message, so a single final
// block.  Nothing here takes a context, a lock or any state shared between calls.
#include "../../include/h2v_draws.h"
#include "batch.h"
#include <string.h>

namespace h2v {

namespace {
// RFC 7693, 2.6 (IV) and 2.7 (message schedule; rounds 10 and 11 repeat rows 0 and 1)
const uint64_t B2B_IV[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                            0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
const uint8_t B2B_SIGMA[10][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
inline uint64_t b2b_rotr(uint64_t x, int c) { return (x >> c) | (x << (64 - c)); }
// RFC 7693, 3.1: the mixing function G
inline void b2b_g(uint64_t v[16], int a, int b, int c, int d, uint64_t x, uint64_t y) {
    v[a] = v[a] + v[b] + x; v[d] = b2b_rotr(v[d] ^ v[a], 32);
    v[c] = v[c] + v[d];     v[b] = b2b_rotr(v[b] ^ v[c], 24);
    v[a] = v[a] + v[b] + y; v[d] = b2b_rotr(v[d] ^ v[a], 16);
    v[c] = v[c] + v[d];     v[b] = b2b_rotr(v[b] ^ v[c], 63);
}
// RFC 7693, 3.2: the compression function F over the one and final block m of a message of t < 2^64 bytes
void b2b_compress_final(uint64_t h[8], const uint64_t m[16], uint64_t t) {
    uint64_t v[16];
    for (int i = 0; i < 8; ++i) { v[i] = h[i]; v[8 + i] = B2B_IV[i]; }
    v[12] ^= t;          // (the high word of the counter is zero)
    v[14] = ~v[14];      // the final block
    for (int rd = 0; rd < 12; ++rd) {
        const uint8_t* s = B2B_SIGMA[rd % 10];
        b2b_g(v, 0, 4, 8, 12, m[s[0]], m[s[1]]);
        b2b_g(v, 1, 5, 9, 13, m[s[2]], m[s[3]]);
        b2b_g(v, 2, 6, 10, 14, m[s[4]], m[s[5]]);
        b2b_g(v, 3, 7, 11, 15, m[s[6]], m[s[7]]);
        b2b_g(v, 0, 5, 10, 15, m[s[8]], m[s[9]]);
        b2b_g(v, 1, 6, 11, 12, m[s[10]], m[s[11]]);
        b2b_g(v, 2, 7, 8, 13, m[s[12]], m[s[13]]);
        b2b_g(v, 3, 4, 9, 14, m[s[14]], m[s[15]]);
    }
    for (int i = 0; i < 8; ++i) h[i] ^= v[i] ^ v[8 + i];
}
inline uint64_t le64(const uint8_t* p) { uint64_t w = 0; for (int k = 7; k >= 0; --k) w = (w << 8) | p[k]; return w; }
}  // namespace

void expand_draws_host(const uint8_t seed32[32], uint64_t first, size_t n, uint8_t* out32) {
    // RFC 7693, 2.5: the parameter block — digest 64, no key, fanout = depth = 1 in word 0; the personal string in words 6 and 7
    uint64_t h_init[8];
    for (int i = 0; i < 8; ++i) h_init[i] = B2B_IV[i];
    h_init[0] ^= 0x01010040ULL;
    static const uint8_t personal[16] = {'h', '2', 'v', '-', 'd', 'r', 'a', 'w', 's', '-', 'v', '1', 0, 0, 0, 0};
    h_init[6] ^= le64(personal);
    h_init[7] ^= le64(personal + 8);
    uint64_t m[16];
    memset(m, 0, sizeof m);
    for (int j = 0; j < 4; ++j) m[j] = le64(seed32 + 8 * j);
    for (size_t i = 0; i < n; ++i) {
        uint64_t h[8];
        for (int j = 0; j < 8; ++j) h[j] = h_init[j];
        m[4] = first + i;
        b2b_compress_final(h, m, 40);
        uint32_t w[16];
        for (int j = 0; j < 8; ++j) { w[2 * j] = (uint32_t)h[j]; w[2 * j + 1] = (uint32_t)(h[j] >> 32); }
        Fr::from_uniform_words(w).to_bytes(out32 + 32 * i);
    }
}

// the refusals the two entry points share
static int draws_arguments(const char* who, const uint8_t* seed32, uint64_t first, size_t n, const void* out) {
    if (!seed32 || (n && !out)) { set_last_error(std::string(who) + ": null argument"); return H2V_ERR_BAD_ARGUMENT; }
    // indices first .. first + n - 1 are 64-bit: first + n may reach 2^64, not pass it
    if (n && (uint64_t)(n - 1) > UINT64_MAX - first) { set_last_error(std::string(who) + ": first_index + n wraps past 2^64"); return H2V_ERR_BAD_ARGUMENT; }
    if (n > SIZE_MAX / 32) { set_last_error(std::string(who) + ": n too large"); return H2V_ERR_BAD_ARGUMENT; }
    return 0;
}

}  // namespace h2v

using namespace h2v;

extern "C" {

int h2v_draws_expand(const uint8_t seed32[32], uint64_t first_index, size_t n, uint8_t* out32) {
    int rc = draws_arguments("h2v_draws_expand", seed32, first_index, n, out32);
    if (rc) return rc;
    expand_draws_host(seed32, first_index, n, out32);
    return 0;
}

int h2v_draws_expand_device(int device, void* stream, const uint8_t seed32[32], uint64_t first_index, size_t n, void* d_out32) {
    static const char who[] = "h2v_draws_expand_device";
    int rc = draws_arguments(who, seed32, first_index, n, d_out32);
    if (rc) return rc;
    if (!n) return 0;
    // (before the pointer is looked at: the launcher's limit, so that no range the launch would refuse gets as far as a HIP error)
    if (n > (size_t)H2V_DRAWS_DEVICE_MAX) { set_last_error(std::string(who) + ": n is above H2V_DRAWS_DEVICE_MAX draws for one call"); return H2V_ERR_BAD_ARGUMENT; }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) { (void)hipGetLastError(); count = 0; }
    if (device < 0 || device >= count) { set_last_error(std::string(who) + ": no such device"); return H2V_ERR_BAD_ARGUMENT; }
    H2V_HIP_CHECK(hipSetDevice(device));
    if ((rc = device_range_check(d_out32, 32 * n, device, "d_out32", who, "writes"))) return rc;
    return expand_draws_enqueue((hipStream_t)stream, seed32, first_index, n, d_out32);
}

}  // extern "C"
