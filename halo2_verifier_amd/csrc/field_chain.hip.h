// Device-only building block of the "chained" field products (bn254.hip.h: mul_chain, sqr_chain, dot2_chain): one column of a
// product-scanning Montgomery product as ONE asm statement, a run of v_mad_u64_u32 that all accumulate into the same register pair.
//
// Why asm at all: written in C++, the compiler reassociates a column's sum so that it starts from zero and adds the carry of the
// previous column last, a 64-bit addition (v_lshl_add_u64) per column that costs as much as a multiply-add.  A run that STARTS from
// the carry needs no such addition: the carry is the addend of the column's first multiply-add.  One statement per column (not per
// multiply-add) keeps the number of asm boundaries, and with it the wait states the hazard recogniser pads them with, at 17 per
// product.  The statements hold v_mad_u64_u32 only; quotient digits, masks and shifts stay C++ between them.
//
// MadRun<NV, NS>::run(c, x, y, m, q):  c += sum_{i < NV} x[i] * y[i] + sum_{i < NS} m[i] * q[i], with x, y, m in VGPRs and q (modulus
// limbs, compile-time constants) in SGPRs; a VOP3 instruction of gfx9 reads at most one SGPR and takes no 32-bit literal.  vcc takes the
// (always zero) carry-out.  An asm string must be a literal, so each (NV, NS) shape a product needs is instantiated by name below; a
// shape that is missing is a compile error, never a fallback.
#pragma once
#include <stdint.h>
#if defined(__HIP_DEVICE_COMPILE__)
namespace h2v {
#define H2V_MAD(x, y) "v_mad_u64_u32 %[c], vcc, %[" #x "], %[" #y "], %[c]\n\t"
#define H2V_VV1 H2V_MAD(x0, y0)
#define H2V_VV2 H2V_VV1 H2V_MAD(x1, y1)
#define H2V_VV3 H2V_VV2 H2V_MAD(x2, y2)
#define H2V_VV4 H2V_VV3 H2V_MAD(x3, y3)
#define H2V_VV5 H2V_VV4 H2V_MAD(x4, y4)
#define H2V_VV6 H2V_VV5 H2V_MAD(x5, y5)
#define H2V_VV7 H2V_VV6 H2V_MAD(x6, y6)
#define H2V_VV8 H2V_VV7 H2V_MAD(x7, y7)
#define H2V_VV9 H2V_VV8 H2V_MAD(x8, y8)
#define H2V_VV10 H2V_VV9 H2V_MAD(x9, y9)
#define H2V_VV11 H2V_VV10 H2V_MAD(x10, y10)
#define H2V_VV12 H2V_VV11 H2V_MAD(x11, y11)
#define H2V_VV13 H2V_VV12 H2V_MAD(x12, y12)
#define H2V_VV14 H2V_VV13 H2V_MAD(x13, y13)
#define H2V_VV15 H2V_VV14 H2V_MAD(x14, y14)
#define H2V_VV16 H2V_VV15 H2V_MAD(x15, y15)
#define H2V_VV17 H2V_VV16 H2V_MAD(x16, y16)
#define H2V_VV18 H2V_VV17 H2V_MAD(x17, y17)
#define H2V_OV1 [x0] "v"(x[0]), [y0] "v"(y[0])
#define H2V_OV2 H2V_OV1, [x1] "v"(x[1]), [y1] "v"(y[1])
#define H2V_OV3 H2V_OV2, [x2] "v"(x[2]), [y2] "v"(y[2])
#define H2V_OV4 H2V_OV3, [x3] "v"(x[3]), [y3] "v"(y[3])
#define H2V_OV5 H2V_OV4, [x4] "v"(x[4]), [y4] "v"(y[4])
#define H2V_OV6 H2V_OV5, [x5] "v"(x[5]), [y5] "v"(y[5])
#define H2V_OV7 H2V_OV6, [x6] "v"(x[6]), [y6] "v"(y[6])
#define H2V_OV8 H2V_OV7, [x7] "v"(x[7]), [y7] "v"(y[7])
#define H2V_OV9 H2V_OV8, [x8] "v"(x[8]), [y8] "v"(y[8])
#define H2V_OV10 H2V_OV9, [x9] "v"(x[9]), [y9] "v"(y[9])
#define H2V_OV11 H2V_OV10, [x10] "v"(x[10]), [y10] "v"(y[10])
#define H2V_OV12 H2V_OV11, [x11] "v"(x[11]), [y11] "v"(y[11])
#define H2V_OV13 H2V_OV12, [x12] "v"(x[12]), [y12] "v"(y[12])
#define H2V_OV14 H2V_OV13, [x13] "v"(x[13]), [y13] "v"(y[13])
#define H2V_OV15 H2V_OV14, [x14] "v"(x[14]), [y14] "v"(y[14])
#define H2V_OV16 H2V_OV15, [x15] "v"(x[15]), [y15] "v"(y[15])
#define H2V_OV17 H2V_OV16, [x16] "v"(x[16]), [y16] "v"(y[16])
#define H2V_OV18 H2V_OV17, [x17] "v"(x[17]), [y17] "v"(y[17])
#define H2V_VS1 H2V_MAD(m0, q0)
#define H2V_VS2 H2V_VS1 H2V_MAD(m1, q1)
#define H2V_VS3 H2V_VS2 H2V_MAD(m2, q2)
#define H2V_VS4 H2V_VS3 H2V_MAD(m3, q3)
#define H2V_VS5 H2V_VS4 H2V_MAD(m4, q4)
#define H2V_VS6 H2V_VS5 H2V_MAD(m5, q5)
#define H2V_VS7 H2V_VS6 H2V_MAD(m6, q6)
#define H2V_VS8 H2V_VS7 H2V_MAD(m7, q7)
#define H2V_OS1 , [m0] "v"(m[0]), [q0] "s"(q[0])
#define H2V_OS2 H2V_OS1, [m1] "v"(m[1]), [q1] "s"(q[1])
#define H2V_OS3 H2V_OS2, [m2] "v"(m[2]), [q2] "s"(q[2])
#define H2V_OS4 H2V_OS3, [m3] "v"(m[3]), [q3] "s"(q[3])
#define H2V_OS5 H2V_OS4, [m4] "v"(m[4]), [q4] "s"(q[4])
#define H2V_OS6 H2V_OS5, [m5] "v"(m[5]), [q5] "s"(q[5])
#define H2V_OS7 H2V_OS6, [m6] "v"(m[6]), [q6] "s"(q[6])
#define H2V_OS8 H2V_OS7, [m7] "v"(m[7]), [q7] "s"(q[7])
template <int NV, int NS> struct MadRun;
#define H2V_RUN(NV, NS)                                                                                                              \
    template <> struct MadRun<NV, NS> {                                                                                              \
        __device__ __forceinline__ static void run(uint64_t& c, const uint32_t* x, const uint32_t* y, const uint32_t* m, const uint32_t* q) { \
            asm(H2V_VV##NV H2V_VS##NS : [c] "+v"(c) : H2V_OV##NV H2V_OS##NS : "vcc");                                                \
        }                                                                                                                            \
    };
// mul: (k + 1, k) for columns 1..8, (n, n) for n = 8..1; dot2: twice as many products per column; sqr: the halved off-diagonal runs
H2V_RUN(1, 1) H2V_RUN(1, 2) H2V_RUN(2, 1) H2V_RUN(2, 2) H2V_RUN(2, 3) H2V_RUN(2, 4) H2V_RUN(3, 2)
H2V_RUN(3, 3) H2V_RUN(3, 4) H2V_RUN(3, 5) H2V_RUN(3, 6) H2V_RUN(4, 1) H2V_RUN(4, 2) H2V_RUN(4, 3)
H2V_RUN(4, 4) H2V_RUN(4, 6) H2V_RUN(4, 7) H2V_RUN(4, 8) H2V_RUN(5, 4) H2V_RUN(5, 5) H2V_RUN(5, 8)
H2V_RUN(6, 2) H2V_RUN(6, 3) H2V_RUN(6, 5) H2V_RUN(6, 6) H2V_RUN(7, 6) H2V_RUN(7, 7) H2V_RUN(8, 3)
H2V_RUN(8, 4) H2V_RUN(8, 7) H2V_RUN(8, 8) H2V_RUN(9, 8) H2V_RUN(10, 4) H2V_RUN(10, 5) H2V_RUN(12, 5)
H2V_RUN(12, 6) H2V_RUN(14, 6) H2V_RUN(14, 7) H2V_RUN(16, 7) H2V_RUN(16, 8) H2V_RUN(18, 8)
// sqdot (a squaring and a product in one pass): the halved runs of the squaring beside the product's
H2V_RUN(3, 1) H2V_RUN(5, 2) H2V_RUN(5, 3) H2V_RUN(6, 4) H2V_RUN(8, 5) H2V_RUN(9, 5) H2V_RUN(9, 6) H2V_RUN(11, 6) H2V_RUN(11, 7) H2V_RUN(12, 7) H2V_RUN(12, 8) H2V_RUN(14, 8)
}  // namespace h2v
#endif
