// The pairing kernels' device arithmetic on inputs chosen by tests/test_gpu_pairing_units.py: the real pair_step6,
// pair_coefficients6 (coef_form inside both), pair_in_fq_star6, k_pair_lines and the two check entry points of pairing.hip, fed raw
// 29-bit limbs so that the Python side picks every representative (Montgomery v 2^261 mod p, or that plus p).  Built with the
// library's flags by halo2_verifier_amd/csrc/Makefile (build/pairing_units).
//
//   pairing_units step    IN OUT          one operation step per workgroup, in k_pairing's layout (128 threads) or as column B of
//                                         k_pairing2's (256 threads); OUT: the six stored forms of the destination register
//   pairing_units check   IN OUT          pair_in_fq_star6 of crafted registers
//   pairing_units lines   PARAMS IN OUT   k_pair_lines over crafted pieces with the split tables of a PairingDevice
//   pairing_units verdict PARAMS IN OUT   pairing_check_split_enqueue (k_pairing2 or one stream) and pairing_check_enqueue
//   pairing_units tail    PARAMS IN OUT   pairing_check_split_enqueue with a PairTail: the tail workgroups of k_pairing2 (pair_tail_role)
// Files are little-endian uint32 words; the layouts are in the readers below.  Every index that reaches a kernel is checked on the
// host first.  The outputs a mode allocates itself are preset to 0xff and lie between guard bands that are checked after the kernels
// (the line workspace and the mapped host blocks are the library's own types and stay as they are).  The prelude is tests/cpp/units.h.
#include "../../halo2_verifier_amd/csrc/pairing.hip"
#include "../../halo2_verifier_amd/csrc/params.hip"
#include "units.h"

// ---- step: registers 0, 1 come from the pool, register 2 starts as limbs no kernel stores (0xffffffff), the line from the line pool
#define UNIT_REGS 3
struct StepCase { uint32_t word, ra, rb, line; };   // operation word (pair_op), pool index of register 0, of register 1, line pool index
__global__ void __launch_bounds__(2 * PAIR_THREADS) k_units_step(const StepCase* __restrict__ cases, const Coef6 (*__restrict__ pool)[6],
                                                                  const Fq2 (*__restrict__ lines)[6], const PairingConsts* __restrict__ consts,
                                                                  uint32_t col, Coef6 (*__restrict__ out)[6]) {
    __shared__ Coef6 reg[UNIT_REGS][6];
    __shared__ Fq2 line[1][6];
    const StepCase c = cases[blockIdx.x];
    const uint32_t t = threadIdx.x;
    constexpr uint32_t RW = sizeof(Coef6) * 6 / 4, LW = sizeof(Fq2) * 6 / 4;
    for (uint32_t k = t; k < RW; k += blockDim.x) {
        reinterpret_cast<uint32_t*>(reg[0])[k] = reinterpret_cast<const uint32_t*>(pool[c.ra])[k];
        reinterpret_cast<uint32_t*>(reg[1])[k] = reinterpret_cast<const uint32_t*>(pool[c.rb])[k];
        reinterpret_cast<uint32_t*>(reg[2])[k] = 0xffffffffu;
    }
    for (uint32_t k = t; k < LW; k += blockDim.x) reinterpret_cast<uint32_t*>(line[0])[k] = reinterpret_cast<const uint32_t*>(lines[c.line])[k];
    __syncthreads();
    const uint32_t op = c.word & 255u, rd = (c.word >> 8) & 255u, ra = (c.word >> 16) & 255u, rb = c.word >> 24;
    if (t / PAIR_THREADS == col) {   // the group that runs the step: all of k_pairing's block, or the second half of k_pairing2's
        const uint32_t tl = t % PAIR_THREADS;
        if (op <= P_MULL) pair_step6(op, rd, ra, rb, line, reg, tl);
        else pair_coefficients6(op, rd, ra, reg, consts, tl);
    }
    __syncthreads();
    for (uint32_t k = t; k < RW; k += blockDim.x) reinterpret_cast<uint32_t*>(out[blockIdx.x])[k] = reinterpret_cast<const uint32_t*>(reg[rd])[k];
}

// IN: n_pool, n_lines, n_a (k_pairing layout), n_b (column B), pool[n_pool] (Coef6[6]), lines[n_lines] (Fq2[6]), cases[n_a + n_b]
// OUT: the destination register (Coef6[6]) of every case, in input order
static void mode_step(In& r, Out& out) {
    const uint32_t n_pool = r.word(), n_lines = r.word(), n_a = r.word(), n_b = r.word();
    REQUIRE(n_pool && n_lines && n_pool < (1u << 24) && n_lines < (1u << 24) && (size_t)n_a + n_b < (1u << 24), "sizes");
    std::vector<Coef6> pool((size_t)n_pool * 6);
    std::vector<Fq2> lines((size_t)n_lines * 6);
    std::vector<StepCase> cases((size_t)n_a + n_b);
    r.take(pool.data(), pool.size()); r.take(lines.data(), lines.size()); r.take(cases.data(), cases.size());
    REQUIRE(r.at_end(), "trailing input");
    for (const StepCase& c : cases) {
        const uint32_t op = c.word & 255u, rd = (c.word >> 8) & 255u, ra = (c.word >> 16) & 255u, rb = c.word >> 24;
        const bool known = op == P_SQR || op == P_MUL || op == P_MULL || op == P_CONJ || op == P_CONJ0 || op == P_COPY || op == P_FROB ||
                           op == P_FROB2 || op == P_FROB3 || op == P_FROB4;
        REQUIRE(known && rd < UNIT_REGS && ra < UNIT_REGS, "operation word");
        REQUIRE(op == P_MULL ? rb == 0 : (op == P_MUL ? rb < UNIT_REGS : rb == 0), "operand b");
        REQUIRE(c.ra < n_pool && c.rb < n_pool && c.line < n_lines, "pool index");
    }
    const PairingConsts k = pairing_consts_host();
    PairingConsts* d_k = to_device(&k, 1);
    auto* d_pool = reinterpret_cast<const Coef6(*)[6]>(to_device(pool.data(), pool.size()));
    auto* d_lines = reinterpret_cast<const Fq2(*)[6]>(to_device(lines.data(), lines.size()));
    StepCase* d_cases = to_device(cases.data(), cases.size());
    Guarded<Coef6> regs(cases.size() * 6);
    auto* out6 = reinterpret_cast<Coef6(*)[6]>(regs.p);
    if (n_a) hipLaunchKernelGGL(k_units_step, dim3(n_a), dim3(PAIR_THREADS), 0, 0, d_cases, d_pool, d_lines, d_k, 0u, out6);
    CK(hipGetLastError());
    if (n_b) hipLaunchKernelGGL(k_units_step, dim3(n_b), dim3(2 * PAIR_THREADS), 0, 0, d_cases + n_a, d_pool, d_lines, d_k, 1u, out6 + n_a);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    regs.collect(out, "registers");
    printf("step: %u + %u cases\n", n_a, n_b);
}

// ---- check: IN: n, registers[n] (Coef6[6]); OUT: n words, pair_in_fq_star6
__global__ void k_units_check(const Coef6 (*__restrict__ x)[6], uint32_t n, uint32_t* __restrict__ ok) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ok[i] = pair_in_fq_star6(x[i]) ? 1u : 0u;
}
static void mode_check(In& r, Out& out) {
    const uint32_t n = r.word();
    REQUIRE(n && n < (1u << 20), "sizes");
    std::vector<Coef6> regs((size_t)n * 6);
    r.take(regs.data(), regs.size());
    REQUIRE(r.at_end(), "trailing input");
    auto* d_regs = reinterpret_cast<const Coef6(*)[6]>(to_device(regs.data(), regs.size()));
    Guarded<uint32_t> ok(n);
    hipLaunchKernelGGL(k_units_check, dim3((n + 63) / 64), dim3(64), 0, 0, d_regs, n, ok.p);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    ok.collect(out, "verdicts");
    printf("check: %u registers\n", n);
}

static void upload_params(const char* path, PairingDevice& pd) {
    const std::vector<uint8_t> b = read_file(path);
    REQUIRE(b.size() % 4 == 0, "params are not whole words");
    ParamsHost params;
    std::string err;
    if (!params_from_bytes(b.data(), b.size(), H2V_SERDE_RAW_BYTES, params, err)) { fprintf(stderr, "params: %s\n", err.c_str()); exit(2); }
    RC(pd.upload(params));
}
// pieces of n checks over `parts` split accumulators, G1J each (X Z, Y, Z^3 for the split entry points), into G1JSlot
static G1JSlot* read_slots(In& r, size_t count) {
    std::vector<G1J> pts(count);
    r.take(pts.data(), count);
    std::vector<G1JSlot> slots(count);
    for (size_t i = 0; i < count; ++i) slots[i] = pts[i];
    return to_device(slots.data(), count);
}

// ---- lines: IN: n_jobs, then per job: shift, parts, n, pieces[n * 2 * parts] (check c: L_j at (2c) parts + j, R_j at (2c + 1) parts + j)
// OUT: per job, k_pair_lines' output: n x PAIR_ITERS x 6 Fq2;  OUT.tables: per job, the host rows of its table (split_line_rows)
static void mode_lines(In& r, Out& out) {
    const uint32_t jobs = r.word();
    PairingDevice pd;
    upload_params(r.params, pd);
    std::vector<LineCoeff> all_rows;
    for (uint32_t jb = 0; jb < jobs; ++jb) {
        const uint32_t shift = r.word(), parts = r.word(), n = r.word();
        REQUIRE(parts >= 1 && parts <= PL_MAX_PARTS && n >= 1 && n <= 64 && shift < 256, "lines job");
        G1JSlot* d_ready = read_slots(r, (size_t)2 * parts * n);
        const LineCoeff* tab = nullptr;
        RC(pd.split_lines(shift, parts, &tab));
        std::vector<LineCoeff> rows;
        RC(split_line_rows(pd.h_sg2, pd.h_ng2, shift, parts, rows));
        all_rows.insert(all_rows.end(), rows.begin(), rows.end());
        Guarded<Fq2> lines((size_t)n * PAIR_ITERS * 6);
        hipLaunchKernelGGL(k_pair_lines, dim3(PAIR_ITERS, n), dim3(PL_THREADS), 0, 0, d_ready, parts, tab, pair_iterations(), lines.p);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        lines.collect(out, "lines");
        CK(hipFree(d_ready));
    }
    write_file((out.path + ".tables").c_str(), all_rows.data(), all_rows.size() * sizeof(LineCoeff));
    printf("lines: %u jobs\n", jobs);
}

// ---- verdict: IN: n_jobs, then per job: kind (0: split, k_pairing2; 1: split, one stream; 2: whole points), shift, parts, n,
// pieces (split: n * 2 * parts line-ready pieces as in `lines`; whole: n pairs of Jacobian points); OUT: the n verdicts of every job
static void mode_verdict(In& r, Out& out) {
    const uint32_t jobs = r.word();
    PairingDevice pd;
    upload_params(r.params, pd);
    for (uint32_t jb = 0; jb < jobs; ++jb) {
        const uint32_t kind = r.word(), shift = r.word(), parts = r.word(), n = r.word();
        REQUIRE(kind <= 2 && n >= 1 && n <= 64 && shift < 256, "verdict job");
        Guarded<uint32_t> ok(n);
        uint32_t* d_ok = ok.p;
        if (kind == 2) {
            std::vector<G1J> pairs((size_t)2 * n);
            r.take(pairs.data(), pairs.size());
            G1J* d_pairs = to_device(pairs.data(), pairs.size());
            RC(pairing_check_enqueue(0, pd, d_pairs, n, d_ok));
            CK(hipDeviceSynchronize());
            CK(hipFree(d_pairs));
        } else {
            REQUIRE(parts >= 1 && parts <= PL_MAX_PARTS, "verdict parts");
            G1JSlot* d_ready = read_slots(r, (size_t)2 * parts * n);
            void* d_ws = nullptr;
            CK(hipMalloc(&d_ws, (size_t)n * H2V_PAIRING_LINE_WS_BYTES));
            RC(pairing_check_split_enqueue(0, pd, d_ready, n, parts, shift, d_ws, d_ok, kind == 1));
            CK(hipDeviceSynchronize());
            CK(hipFree(d_ws));
            CK(hipFree(d_ready));
        }
        ok.collect(out, "verdicts");
    }
    printf("verdict: %u jobs\n", jobs);
}

// ---- tail: IN: n_jobs, then per job: shift, parts, n, count, n_words, skip_lo, skip_hi; the checks' line-ready pieces (n * 2 * parts, as in
// `verdict`); the tail's Jacobian pieces (count * parts: point q = sum_j 2^(shift j) piece[q parts + j]); n_words source words.
// Every output the tail writes per point has count + 1 elements, preset to 0xff: the spare one belongs to no point, must keep its preset and
// is written out with the rest (its pieces are identities and its problem's `out` is the spare whole point: a lane that took it for a point
// would write there, inside the buffers).  dst has TAIL_DST_SPARE spare words behind n_words.  host_bytes, host_ident and dst are mapped
// host memory.
// OUT per job: n verdicts; count + 1 whole points (27 words); the device block: (count + 1) * 16 words of bytes, count + 1 identity words;
// the host block likewise; n_words + TAIL_DST_SPARE words of dst
#define TAIL_DST_SPARE 16u
static void mode_tail(In& r, Out& out) {
    const uint32_t jobs = job_count(r, 256);
    PairingDevice pd;
    upload_params(r.params, pd);
    if (!pairing_tail_fits(pd, false)) { fprintf(stderr, "tail: this device's pairing launch cannot carry a tail (pairing_tail_fits)\n"); exit(6); }
    for (uint32_t jb = 0; jb < jobs; ++jb) {
        const uint32_t shift = r.word(), parts = r.word(), n = r.word(), count = r.word(), n_words = r.word(), skip_lo = r.word(), skip_hi = r.word();
        REQUIRE(n >= 1 && n <= 64 && parts >= 1 && parts <= PL_MAX_PARTS && shift < 256, "tail job");
        REQUIRE(count >= 1 && count <= 128 && n_words >= 1 && n_words <= (1u << 16) && skip_lo <= skip_hi && skip_hi <= n_words, "tail shape");
        G1JSlot* d_ready = read_slots(r, (size_t)2 * parts * n);
        const size_t slots = (size_t)count + 1;
        std::vector<G1J> pts(slots * parts, G1J::identity());
        r.take(pts.data(), (size_t)count * parts);
        std::vector<G1JSlot> pieces(pts.size());
        for (size_t i = 0; i < pts.size(); ++i) pieces[i] = pts[i];
        G1JSlot* d_pieces = to_device(pieces.data(), pieces.size());
        std::vector<uint32_t> src(n_words);
        r.take(src.data(), n_words);
        uint32_t* d_src = to_device(src.data(), n_words);
        Guarded<G1J> whole(slots); Guarded<uint8_t> bytes(slots * 64); Guarded<uint32_t> ident(slots), ok(n);
        void* d_ws = nullptr;
        CK(hipMalloc(&d_ws, (size_t)n * H2V_PAIRING_LINE_WS_BYTES));
        std::vector<MsmProblem> prs(slots);
        for (size_t q = 0; q < slots; ++q) prs[q].out = whole.p + q;
        MsmProblem* d_prs = to_device(prs.data(), slots);
        MappedHostBuf h_bytes, h_ident, h_dst;
        const size_t dst_words = (size_t)n_words + TAIL_DST_SPARE;
        RC(h_bytes.reserve(slots * 64)); RC(h_ident.reserve(slots * 4)); RC(h_dst.reserve(dst_words * 4));
        memset(h_bytes.p, 0xff, slots * 64); memset(h_ident.p, 0xff, slots * 4); memset(h_dst.p, 0xff, dst_words * 4);
        PairTail t;
        t.pieces = d_pieces; t.prs = d_prs; t.count = count; t.parts = parts; t.shift = shift;
        t.out_bytes = bytes.p; t.out_ident = ident.p;
        t.host_bytes = reinterpret_cast<uint8_t*>(h_bytes.dev); t.host_ident = reinterpret_cast<uint32_t*>(h_ident.dev);
        t.src = d_src; t.dst = reinterpret_cast<uint32_t*>(h_dst.dev);
        t.n_words = n_words; t.skip_lo = skip_lo; t.skip_hi = skip_hi;
        RC(pairing_check_split_enqueue(0, pd, d_ready, n, parts, shift, d_ws, ok.p, false, &t));
        CK(hipDeviceSynchronize());
        ok.collect(out, "verdicts"); whole.collect(out, "whole points");
        bytes.collect(out, "device bytes"); ident.collect(out, "device identity words");
        out.raw(h_bytes.p, slots * 64); out.raw(h_ident.p, slots * 4);
        out.raw(h_dst.p, dst_words * 4);
        CK(hipFree(d_ready)); CK(hipFree(d_pieces)); CK(hipFree(d_src)); CK(hipFree(d_ws)); CK(hipFree(d_prs));
    }
    printf("tail: %u jobs\n", jobs);
}

static const Mode MODES[] = {{"step", mode_step, true, false}, {"check", mode_check, true, false},
                             {"lines", mode_lines, true, true}, {"verdict", mode_verdict, true, true}, {"tail", mode_tail, true, true}};
int main(int argc, char** argv) { return units_main("pairing_units", MODES, argc, argv); }
