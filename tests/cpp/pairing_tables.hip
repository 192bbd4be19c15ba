// Host dump of the pairing's tables (no GPU needed), for tests/test_pairing_tables.py: the three physical operation tables after
// pair_rename_registers, the Frobenius constants, the Miller-loop line coefficients of s_g2 and -g2 and the split tables of
// PairingDevice::split_lines.  Every Fq is printed as the integer its nine 29-bit limbs spell (a Montgomery representative,
// R = 2^261), so the Python side sees the stored representative, not only its residue.
// Usage: pairing_tables <params file (RawBytes)> [shift:parts ...]
// Build (tests/test_pairing_tables.py): hipcc -O1 -std=c++17 --offload-arch=gfx950 pairing_tables.hip
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>
#include "../../halo2_verifier_amd/csrc/pairing.hip"
#include "../../halo2_verifier_amd/csrc/params.hip"

namespace h2v {
void set_last_error(const std::string&) {}
}
using namespace h2v;

static void put_fq(const Fq& x) {
    // the limbs as one hexadecimal integer: sum v[l] 2^(29 l)
    uint32_t w[9] = {0};
    for (int l = 0; l < 9; ++l) {
        const int bit = 29 * l;
        const uint64_t v = (uint64_t)x.v[l] << (bit % 32);
        w[bit / 32] |= (uint32_t)v;
        if (bit / 32 + 1 < 9) w[bit / 32 + 1] |= (uint32_t)(v >> 32);
    }
    printf(" ");
    int top = 8;
    while (top > 0 && !w[top]) --top;
    printf("%x", w[top]);
    for (int i = top - 1; i >= 0; --i) printf("%08x", w[i]);
}
static void put_fq2(const Fq2& x) { put_fq(x.c0); put_fq(x.c1); }
static void put_lines(const char* tag, const LineCoeff* l, size_t n) {
    for (size_t i = 0; i < n; ++i) { printf("%s %zu", tag, i); put_fq2(l[i].a); put_fq2(l[i].b); put_fq2(l[i].c); printf("\n"); }
}
static void put_prog(const char* tag, const std::vector<uint32_t>& p) {
    printf("%s %zu", tag, p.size());
    for (uint32_t w : p) printf(" %x", w);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: pairing_tables params [shift:parts ...]\n"); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    const std::vector<uint8_t> pb((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    ParamsHost params;
    std::string err;
    if (!params_from_bytes(pb.data(), pb.size(), H2V_SERDE_RAW_BYTES, params, err)) { fprintf(stderr, "params: %s\n", err.c_str()); return 1; }
    printf("const N_LINES %d PAIR_ITERS %d PAIR_REGS %d PAIR1_REGS %d PAIR_MAX_OPS %d PAIR2_LOGICAL_REGS %d PAIR2_REGS %d PAIR2_MAX_STEPS %d MSM_MAX_PARTS %d\n",
           N_LINES, PAIR_ITERS, PAIR_REGS, PAIR1_REGS, PAIR_MAX_OPS, PAIR2_LOGICAL_REGS, PAIR2_REGS, PAIR2_MAX_STEPS, MSM_MAX_PARTS);
    put_prog("prog1", pairing_program(false));
    put_prog("prog1m", pairing_program(true));
    put_prog("prog2", pairing_program2());
    const PairingConsts k = pairing_consts_host();
    const Fq2* g[4] = {k.gamma1, k.gamma2, k.gamma3, k.gamma4};
    for (int n = 0; n < 4; ++n) for (int i = 0; i < 6; ++i) { printf("gamma %d %d", n + 1, i); put_fq2(g[n][i]); printf("\n"); }
    // the tables PairingDevice::upload makes
    G2A ng2 = params.g2;
    ng2.y = ng2.y.neg();
    std::vector<LineCoeff> a(MAX_LINE_COEFFS), b(MAX_LINE_COEFFS);
    if (g2_prepare(params.s_g2, k, a.data()) != N_LINES || g2_prepare(ng2, k, b.data()) != N_LINES) { fprintf(stderr, "g2_prepare: unexpected length\n"); return 1; }
    put_lines("sg2", a.data(), N_LINES);
    put_lines("ng2", b.data(), N_LINES);
    for (int i = 2; i < argc; ++i) {
        unsigned shift = 0, parts = 0;
        if (sscanf(argv[i], "%u:%u", &shift, &parts) != 2 || !parts || parts > MSM_MAX_PARTS) { fprintf(stderr, "bad split %s\n", argv[i]); return 2; }
        std::vector<LineCoeff> rows;
        if (split_line_rows(params.s_g2, ng2, shift, parts, rows)) { fprintf(stderr, "split_line_rows failed\n"); return 1; }
        for (unsigned r = 0; r < 2 * parts; ++r) {
            char tag[64];
            snprintf(tag, sizeof tag, "split %u %u %u", shift, parts, r);
            put_lines(tag, rows.data() + (size_t)r * N_LINES, N_LINES);
        }
    }
    return 0;
}
