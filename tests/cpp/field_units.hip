// The field header halo2_verifier_amd/csrc/bn254.hip.h routine by routine, and the square roots of curve.hip.h, on operands programmed by
// the tests and compared there with Python big integers (tests/field_units_reference.py).  Built with the library's flags by
// halo2_verifier_amd/csrc/Makefile (build/field_units) for tests/test_gpu_field_units.py; tests/test_field_units_host.py compiles the same
// file and runs its host mode.
//
//   field_units fq|fr gpu [GROUP]    one workgroup of 64 lanes per launch, each lane one case, the device code
//   field_units fq|fr host [GROUP]   the same cases through the host code
// GROUP is products (the default), linear, wide, convert, inverse or root (fq only).  Every limb operand must be below 2^29 ("bad
// input", status 2, before any HIP call); gpu mode wants a multiple of 64 cases.  Every HIP call is checked (status 3).  Operands are RAW
// limbs (no conversion: the Python side picks every representative), results come back exactly as the routine leaves them, truth
// values as one word.  stdout: per case one line per routine, "<routine> w0 w1 .." in hex.
//
// products   Fp::mul_inl, sqr_inl, dot2_inl and sqdot_inl, and on the device their chained forms mul_chain, sqr_chain, dot2_chain and
//            sqdot_chain (field_chain.hip.h; on the host the chained names are the same functions).  stdin: tuples of four operands
//            (a0, b0, a1, b1), each nine little-endian 32-bit words.  mul = a0 b0 / R, sqr = a0^2 / R, dot2 = (a0 b0 + a1 b1) / R,
//            sqdot = (a0^2 + a1 b1) / R.
// linear     four operands (a, b, c, d): add = a + b, sub = a - b, neg = -a, dbl = 2a, canonical of a, is_zero of a, eq = (a == b), and
//            every lazy_lin the library instantiates on (c, d): lazy_sub, lazy_neg(d), lazy_neg2(d), lazy_dbl(c), lazy_add2 and
//            lazy_lin<8, 1, 2> (curve.hip.h: g1_madd_fast, g1_add_fast).
// wide       nine signed 64-bit accumulators (18 words, low word first): from_wide.
// convert    one operand a and sixteen words w: from_raw(w[0..8)), to_raw(a), from_bytes of the 32 bytes of w[0..8) (flag, then the
//            value, zero where refused), to_bytes(a) (the bytes as eight little-endian words), from_mont256(w[0..8)),
//            from_uniform_words(w), from_u32(w[0]), is_odd(a).
// inverse    one operand a, a word e and eight words x: inv_safegcd(a), inv_fermat(a), a.pow_u32(e), a.pow_limbs(x).
// root       one operand a: fq_sqrt_candidate_w<4>(a), and on the device fq_sqrt_candidate_loop_w3<true>(a) and <false>(a).
#include "../../halo2_verifier_amd/csrc/curve.hip.h"
#include "units.h"   // (CK alone: this program speaks text over stdin and stdout)

#define TUPLE_WORDS 36u
#define LANES 64u
#define DEVICE_ROUTINES 8u

static const char* const kDeviceNames[DEVICE_ROUTINES] = {"mul_inl", "mul_chain", "sqr_inl", "sqr_chain", "dot2_inl", "dot2_chain", "sqdot_inl", "sqdot_chain"};

// in: LANES tuples; out: LANES x DEVICE_ROUTINES results of nine limbs
template <class F> __global__ void __launch_bounds__(LANES) k_field_units(const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x;
    F op[4];
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int l = 0; l < 9; ++l) op[o].v[l] = in[lane * TUPLE_WORDS + o * 9 + l];
    const F r[DEVICE_ROUTINES] = {F::mul_inl(op[0], op[1]), F::mul_chain(op[0], op[1]), op[0].sqr_inl(), op[0].sqr_chain(),
                                  F::dot2_inl(op[0], op[1], op[2], op[3]), F::dot2_chain(op[0], op[1], op[2], op[3]),
                                  F::sqdot_inl(op[0], op[2], op[3]), F::sqdot_chain(op[0], op[2], op[3])};
#pragma unroll
    for (uint32_t j = 0; j < DEVICE_ROUTINES; ++j)
#pragma unroll
        for (int l = 0; l < 9; ++l) out[(lane * DEVICE_ROUTINES + j) * 9 + l] = r[j].v[l];
}

// ---- the further groups: one case is `limb_words` words of limb operands and then `raw_words` words of anything; a group's body reads
// one case and writes its routines' words one after the other, on the host and on the device alike
struct Routine { const char* name; uint32_t words; bool device_only; };
enum GroupId { G_LINEAR, G_WIDE, G_CONVERT, G_INVERSE, G_ROOT, G_COUNT };
struct Group { const char* name; uint32_t limb_words, raw_words, routines; Routine r[13]; };
static const Group kGroups[G_COUNT] = {
    {"linear", 36, 0, 13, {{"add", 9, false}, {"sub", 9, false}, {"neg", 9, false}, {"dbl", 9, false}, {"canonical", 9, false}, {"is_zero", 1, false}, {"eq", 1, false},
                           {"lazy_sub", 9, false}, {"lazy_neg", 9, false}, {"lazy_neg2", 9, false}, {"lazy_dbl", 9, false}, {"lazy_add2", 9, false}, {"lazy_lin_8_1_2", 9, false}}},
    {"wide", 0, 18, 1, {{"from_wide", 9, false}}},
    {"convert", 9, 16, 9, {{"from_raw", 9, false}, {"to_raw", 8, false}, {"from_bytes_ok", 1, false}, {"from_bytes", 9, false}, {"to_bytes", 8, false}, {"from_mont256", 9, false},
                           {"from_uniform_words", 9, false}, {"from_u32", 9, false}, {"is_odd", 1, false}}},
    {"inverse", 9, 9, 4, {{"inv_safegcd", 9, false}, {"inv_fermat", 9, false}, {"pow_u32", 9, false}, {"pow_limbs", 9, false}}},
    {"root", 9, 0, 3, {{"sqrt_w4", 9, false}, {"sqrt_loop_chain", 9, true}, {"sqrt_loop_inl", 9, true}}},
};
static uint32_t out_words(const Group& g) { uint32_t n = 0; for (uint32_t j = 0; j < g.routines; ++j) n += g.r[j].words; return n; }

template <class F> H2V_HD F load(const uint32_t* in) { F r; for (int l = 0; l < 9; ++l) r.v[l] = in[l]; return r; }
template <class F> H2V_HD uint32_t* store(uint32_t* out, const F& x) { for (int l = 0; l < 9; ++l) out[l] = x.v[l]; return out + 9; }

template <class F> H2V_HD void linear_case(const uint32_t* in, uint32_t* out) {
    const F a = load<F>(in), b = load<F>(in + 9), c = load<F>(in + 18), d = load<F>(in + 27);
    out = store(out, a + b);
    out = store(out, a - b);
    out = store(out, a.neg());
    out = store(out, a.dbl());
    a.canonical(out); out += 9;
    *out++ = a.is_zero() ? 1u : 0u;
    *out++ = a == b ? 1u : 0u;
    out = store(out, F::lazy_sub(c, d));
    out = store(out, F::lazy_neg(d));
    out = store(out, F::lazy_neg2(d));
    out = store(out, F::lazy_dbl(c));
    out = store(out, F::lazy_add2(c, d));
    store(out, F::template lazy_lin<8, 1, 2>(c, d));
}
template <class F> H2V_HD void wide_case(const uint32_t* in, uint32_t* out) {
    int64_t acc[9];
    for (int l = 0; l < 9; ++l) acc[l] = (int64_t)((uint64_t)in[2 * l] | ((uint64_t)in[2 * l + 1] << 32));
    store(out, F::from_wide(acc));
}
template <class F> H2V_HD void convert_case(const uint32_t* in, uint32_t* out) {
    const F a = load<F>(in);
    uint32_t w[16];
    for (int i = 0; i < 16; ++i) w[i] = in[9 + i];
    uint8_t bytes[32];
    for (int i = 0; i < 32; ++i) bytes[i] = (uint8_t)(w[i / 4] >> (8 * (i % 4)));
    out = store(out, F::from_raw(w));
    a.to_raw(out); out += 8;
    F v = F::zero();
    *out++ = F::from_bytes(bytes, v) ? 1u : 0u;
    out = store(out, v);
    a.to_bytes(bytes);
    for (int i = 0; i < 8; ++i) *out++ = (uint32_t)bytes[4 * i] | ((uint32_t)bytes[4 * i + 1] << 8) | ((uint32_t)bytes[4 * i + 2] << 16) | ((uint32_t)bytes[4 * i + 3] << 24);
    out = store(out, F::from_mont256(w));
    out = store(out, F::from_uniform_words(w));
    out = store(out, F::from_u32(w[0]));
    *out = a.is_odd() ? 1u : 0u;
}
template <class F> H2V_HD void inverse_case(const uint32_t* in, uint32_t* out) {
    const F a = load<F>(in);
    uint32_t x[8];
    for (int i = 0; i < 8; ++i) x[i] = in[10 + i];
    out = store(out, a.inv_safegcd());
    out = store(out, a.inv_fermat());
    out = store(out, a.pow_u32(in[9]));
    store(out, a.pow_limbs(x));
}
// (the loop forms are device code only: the host leaves their words alone and does not print them)
H2V_HD void root_case(const uint32_t* in, uint32_t* out) {
    const Fq a = load<Fq>(in);
    out = store(out, fq_sqrt_candidate_w<4>(a));
#if defined(__HIP_DEVICE_COMPILE__)
    out = store(out, fq_sqrt_candidate_loop_w3<true>(a));
    store(out, fq_sqrt_candidate_loop_w3<false>(a));
#endif
}
template <class F, int G> H2V_HD void group_case(const uint32_t* in, uint32_t* out) {
    if constexpr (G == G_LINEAR) linear_case<F>(in, out);
    else if constexpr (G == G_WIDE) wide_case<F>(in, out);
    else if constexpr (G == G_CONVERT) convert_case<F>(in, out);
    else if constexpr (G == G_INVERSE) inverse_case<F>(in, out);
    else root_case(in, out);
}
// in: LANES cases of `rec` words; out: LANES x `outw` words
template <class F, int G> __global__ void __launch_bounds__(LANES) k_field_group(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t rec, uint32_t outw) {
    const uint32_t lane = threadIdx.x;
    group_case<F, G>(in + lane * rec, out + lane * outw);
}

static void print_limbs(const char* name, const uint32_t* v, uint32_t words = 9) {
    printf("%s", name);
    for (uint32_t l = 0; l < words; ++l) printf(" %x", v[l]);
    printf("\n");
}
// stdin as words; `rec` words a case, of which the first `limb_words` are limbs
static bool read_cases(std::vector<uint32_t>& in, uint32_t rec, uint32_t limb_words) {
    uint32_t buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, stdin)) > 0) {
        if (got % 4) { fprintf(stderr, "bad input: not whole words\n"); return false; }
        in.insert(in.end(), buf, buf + got / 4);
    }
    if (in.empty() || in.size() % rec) { fprintf(stderr, "bad input: not whole tuples\n"); return false; }
    for (size_t i = 0; i < in.size(); ++i) if (i % rec < limb_words && in[i] > H2V_LIMB_MASK) { fprintf(stderr, "bad input: a limb of 2^29 or more\n"); return false; }
    return true;
}
template <class F> static int run(bool gpu) {
    std::vector<uint32_t> in;
    if (!read_cases(in, TUPLE_WORDS, TUPLE_WORDS)) return 2;
    const size_t tuples = in.size() / TUPLE_WORDS;
    if (!gpu) {
        for (size_t t = 0; t < tuples; ++t) {
            F op[4];
            for (int o = 0; o < 4; ++o) memcpy(op[o].v, &in[t * TUPLE_WORDS + o * 9], 36);
            print_limbs("mul_inl", F::mul_inl(op[0], op[1]).v);
            print_limbs("sqr_inl", op[0].sqr_inl().v);
            print_limbs("dot2_inl", F::dot2_inl(op[0], op[1], op[2], op[3]).v);
            print_limbs("sqdot_inl", F::sqdot_inl(op[0], op[2], op[3]).v);
        }
        return 0;
    }
    if (tuples % LANES) { fprintf(stderr, "bad input: gpu mode takes a multiple of 64 tuples\n"); return 2; }
    const size_t out_words = (size_t)LANES * DEVICE_ROUTINES * 9;
    uint32_t *d_in, *d_out;
    CK(hipMalloc((void**)&d_in, LANES * TUPLE_WORDS * 4));
    CK(hipMalloc((void**)&d_out, out_words * 4));
    std::vector<uint32_t> out(out_words);
    for (size_t t = 0; t < tuples; t += LANES) {
        CK(hipMemcpy(d_in, &in[t * TUPLE_WORDS], LANES * TUPLE_WORDS * 4, hipMemcpyHostToDevice));
        CK(hipMemset(d_out, 0xff, out_words * 4));
        hipLaunchKernelGGL(k_field_units<F>, dim3(1), dim3(LANES), 0, 0, d_in, d_out);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(out.data(), d_out, out_words * 4, hipMemcpyDeviceToHost));
        for (uint32_t lane = 0; lane < LANES; ++lane)
            for (uint32_t j = 0; j < DEVICE_ROUTINES; ++j) print_limbs(kDeviceNames[j], &out[((size_t)lane * DEVICE_ROUTINES + j) * 9]);
    }
    CK(hipFree(d_in));
    CK(hipFree(d_out));
    return 0;
}
template <class F, int G> static int run_group(bool gpu) {
    const Group& g = kGroups[G];
    const uint32_t rec = g.limb_words + g.raw_words, outw = out_words(g);
    std::vector<uint32_t> in;
    if (!read_cases(in, rec, g.limb_words)) return 2;
    const size_t cases = in.size() / rec;
    if (gpu && cases % LANES) { fprintf(stderr, "bad input: gpu mode takes a multiple of 64 tuples\n"); return 2; }
    auto print_case = [&](const uint32_t* w) {
        for (uint32_t j = 0; j < g.routines; w += g.r[j].words, ++j)
            if (gpu || !g.r[j].device_only) print_limbs(g.r[j].name, w, g.r[j].words);
    };
    if (!gpu) {
        std::vector<uint32_t> out(outw);
        for (size_t t = 0; t < cases; ++t) {
            out.assign(outw, 0xffffffffu);
            group_case<F, G>(&in[t * rec], out.data());
            print_case(out.data());
        }
        return 0;
    }
    uint32_t *d_in, *d_out;
    CK(hipMalloc((void**)&d_in, (size_t)LANES * rec * 4));
    CK(hipMalloc((void**)&d_out, (size_t)LANES * outw * 4));
    std::vector<uint32_t> out((size_t)LANES * outw);
    for (size_t t = 0; t < cases; t += LANES) {
        CK(hipMemcpy(d_in, &in[t * rec], (size_t)LANES * rec * 4, hipMemcpyHostToDevice));
        CK(hipMemset(d_out, 0xff, (size_t)LANES * outw * 4));
        hipLaunchKernelGGL((k_field_group<F, G>), dim3(1), dim3(LANES), 0, 0, d_in, d_out, rec, outw);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(out.data(), d_out, (size_t)LANES * outw * 4, hipMemcpyDeviceToHost));
        for (uint32_t lane = 0; lane < LANES; ++lane) print_case(&out[(size_t)lane * outw]);
    }
    CK(hipFree(d_in));
    CK(hipFree(d_out));
    return 0;
}
template <class F> static int run_any(const std::string& group, bool gpu) {
    if (group == "products") return run<F>(gpu);
    if (group == "linear") return run_group<F, G_LINEAR>(gpu);
    if (group == "wide") return run_group<F, G_WIDE>(gpu);
    if (group == "convert") return run_group<F, G_CONVERT>(gpu);
    if (group == "inverse") return run_group<F, G_INVERSE>(gpu);
    return -1;
}
int main(int argc, char** argv) {
    const bool args = argc == 3 || argc == 4;
    const std::string field = args ? argv[1] : "", mode = args ? argv[2] : "", group = argc == 4 ? argv[3] : "products";
    int rc = -1;
    if ((field == "fq" || field == "fr") && (mode == "gpu" || mode == "host")) {
        if (group == "root") rc = field == "fq" ? run_group<Fq, G_ROOT>(mode == "gpu") : -1;
        else rc = field == "fq" ? run_any<Fq>(group, mode == "gpu") : run_any<Fr>(group, mode == "gpu");
    }
    if (rc < 0) { fprintf(stderr, "usage: field_units fq|fr gpu|host [ products|linear|wide|convert|inverse|root ]   (root: fq only)\n"); return 2; }
    return rc;
}
