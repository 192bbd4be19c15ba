// The field products of halo2_verifier_amd/csrc/bn254.hip.h limb by limb: Fp::mul_inl, sqr_inl, dot2_inl and sqdot_inl, and on the device
// their chained forms mul_chain, sqr_chain, dot2_chain and sqdot_chain (field_chain.hip.h), on operand tuples programmed by the tests and compared there
// with Python big integers (tests/field_units_reference.py).  Built with the library's flags by halo2_verifier_amd/csrc/Makefile
// (build/field_units) for tests/test_gpu_field_units.py; tests/test_field_units_host.py compiles the same file and runs its host mode.
//
//   field_units fq|fr gpu    one workgroup of 64 lanes per launch, each lane one tuple, the device code of both forms
//   field_units fq|fr host   the same tuples through the host code (the C++ form; the chained names are the same functions there)
// stdin: tuples of four operands (a0, b0, a1, b1), each nine little-endian 32-bit words holding the RAW limbs (no conversion: the
// products take any limb-normalised operands, canonical or not).  gpu mode wants a multiple of 64 tuples.  Every limb must be below
// 2^29 ("bad input", status 2).  stdout: per tuple one line per routine, "<routine> l0 .. l8" in hex: mul = a0 b0 / R, sqr = a0^2 / R,
// dot2 = (a0 b0 + a1 b1) / R, sqdot = (a0^2 + a1 b1) / R, the result limbs exactly as the routine leaves them.  Every HIP call is checked (status 3).
#include "../../halo2_verifier_amd/csrc/bn254.hip.h"
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

static void print_limbs(const char* name, const uint32_t* v) {
    printf("%s", name);
    for (int l = 0; l < 9; ++l) printf(" %x", v[l]);
    printf("\n");
}
template <class F> static int run(bool gpu) {
    std::vector<uint32_t> in;
    uint32_t buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, stdin)) > 0) {
        if (got % 4) { fprintf(stderr, "bad input: not whole words\n"); return 2; }
        in.insert(in.end(), buf, buf + got / 4);
    }
    if (in.empty() || in.size() % TUPLE_WORDS) { fprintf(stderr, "bad input: not whole tuples\n"); return 2; }
    for (uint32_t w : in) if (w > H2V_LIMB_MASK) { fprintf(stderr, "bad input: a limb of 2^29 or more\n"); return 2; }
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
int main(int argc, char** argv) {
    const std::string field = argc == 3 ? argv[1] : "", mode = argc == 3 ? argv[2] : "";
    if ((field != "fq" && field != "fr") || (mode != "gpu" && mode != "host")) { fprintf(stderr, "usage: field_units fq|fr gpu|host\n"); return 2; }
    return field == "fq" ? run<Fq>(mode == "gpu") : run<Fr>(mode == "gpu");
}
