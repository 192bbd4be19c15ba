// The gather of a batch's Guards (include/h2v_guards.h; the entry points are batch.hip's): after any staged launch every proof's
// scalars and points lie resident in fixed layouts, and the two kernels here put them into term lists in the plan's order.
#include "../../include/h2v.h"
#include "ctx.h"
#include "batch.h"

namespace h2v {

// One thread per (proof, term) of the range, consecutive threads writing consecutive output terms.  Per thread: the term's (kind,
// index) from the order table (T entries, read by every proof: cache-resident); the scalar — a slot term's 8 canonical words by two
// 16-byte loads, a VK-wide term's Montgomery value by ONE product with 1 (Fr::to_raw); the G1A as it lies (72 bytes: word loads); the
// proof's status word through status_decode.  A proof with a status gives zero scalars (the Fr program has stored zeros for it
// already; forced here too, so that the rows do not depend on what an earlier launch left) under the identity.
//   BYTES:  scalars as 32 canonical little-endian bytes (the words as they are), bases as 64 bytes x | y, the identity all-zero
//           (G1A::to_xy_raw, the conversion k_affine_to_bytes uses): 2 + 4 16-byte stores;
//   !BYTES: the 8 words and the G1A unchanged, the form of a resident h2v_msm's arrays: no product but a VK-wide term's.
// A thread past the last term touches nothing.
// gfx950 (-Rpass-analysis=kernel-resource-usage): bytes form 56 VGPRs, object form 33 VGPRs; both 39 SGPRs, no spills, 48 bytes of
// scratch per lane (the call frame of the field product), no LDS; 8 waves per SIMD.  k_guards_proofs: 36 VGPRs, otherwise the same.
template <bool BYTES>
__global__ void __launch_bounds__(256) k_guards_gather(const GuardsGather g, const uint32_t total, uint4* __restrict__ out_scal, void* __restrict__ out_bases) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const uint32_t j = i / g.T, t = i - j * g.T, p = g.first + j;
    const GuardTerm w = g.d_order[t];
    const bool dead = status_decode(g.d_status[p]) != 0;
    uint32_t raw[8];
    G1A base;
    if (w.kind) {
        g.d_shared[(size_t)w.index * g.n + p].to_raw(raw);
        base = g.d_pts[(size_t)g.n * g.np + w.index];
    } else {
        const size_t at = (size_t)p * g.np + w.index;
        const uint4* s = reinterpret_cast<const uint4*>(g.d_slot_scal + at * 8);
        const uint4 s0 = s[0], s1 = s[1];
        raw[0] = s0.x; raw[1] = s0.y; raw[2] = s0.z; raw[3] = s0.w; raw[4] = s1.x; raw[5] = s1.y; raw[6] = s1.z; raw[7] = s1.w;
        base = g.d_pts[at];
    }
    if (dead) {
#pragma unroll
        for (int k = 0; k < 8; ++k) raw[k] = 0;
        base = G1A::identity();
    }
    if (out_scal) {
        out_scal[2 * (size_t)i] = make_uint4(raw[0], raw[1], raw[2], raw[3]);
        out_scal[2 * (size_t)i + 1] = make_uint4(raw[4], raw[5], raw[6], raw[7]);
    }
    if (!out_bases) return;
    if (BYTES) {
        uint32_t xy[16];
        base.to_xy_raw(xy);
        uint4* o = static_cast<uint4*>(out_bases) + 4 * (size_t)i;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = make_uint4(xy[4 * k], xy[4 * k + 1], xy[4 * k + 2], xy[4 * k + 3]);
    } else static_cast<G1A*>(out_bases)[i] = base;
}

// Per proof of the range: its multiplier as 32 canonical bytes (one to_raw, two 16-byte stores) and its decoded status.
__global__ void __launch_bounds__(256) k_guards_proofs(const Fr* __restrict__ mult, const int* __restrict__ status, uint32_t first, uint32_t count,
                                                       uint4* __restrict__ out_mult, int* __restrict__ out_status) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const uint32_t p = first + j;
    if (out_mult) {
        uint32_t raw[8];
        mult[p].to_raw(raw);
        out_mult[2 * (size_t)j] = make_uint4(raw[0], raw[1], raw[2], raw[3]);
        out_mult[2 * (size_t)j + 1] = make_uint4(raw[4], raw[5], raw[6], raw[7]);
    }
    if (out_status) out_status[j] = status_decode(status[p]);
}

// what both forms hold their arguments to; *total = count * T, 0 = nothing to launch
static int guards_gather_check(const GuardsGather& g, const void* out_a, const void* out_b, uint32_t* total) {
    *total = 0;
    if (!g.count || !g.T || (!out_a && !out_b)) return 0;
    if (!g.d_order || !g.d_slot_scal || !g.d_pts || !g.d_status) { set_last_error("guards_gather_enqueue: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if (g.first > g.n || g.count > g.n - g.first) { set_last_error("guards_gather_enqueue: a range outside the upload"); return H2V_ERR_BAD_ARGUMENT; }
    if ((uint64_t)g.count * g.T >= (1ull << 31)) { set_last_error("guards_gather_enqueue: 2^31 terms or more in one launch"); return H2V_ERR_UNSUPPORTED; }
    if (((uintptr_t)g.d_slot_scal | (uintptr_t)out_a) & 15u) { set_last_error("guards_gather_enqueue: scalars off a 16-byte boundary"); return H2V_ERR_BAD_ARGUMENT; }
    *total = g.count * g.T;
    return 0;
}
int guards_gather_bytes_enqueue(hipStream_t s, const GuardsGather& g, uint8_t* d_scalars32, uint8_t* d_bases64) {
    uint32_t total;
    if (int rc = guards_gather_check(g, d_scalars32, d_bases64, &total)) return rc;
    if (!total) return 0;
    if ((uintptr_t)d_bases64 & 15u) { set_last_error("guards_gather_enqueue: bases off a 16-byte boundary"); return H2V_ERR_BAD_ARGUMENT; }
    hipLaunchKernelGGL(k_guards_gather<true>, dim3((total + 255) / 256), dim3(256), 0, s, g, total, reinterpret_cast<uint4*>(d_scalars32), static_cast<void*>(d_bases64));
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
int guards_gather_terms_enqueue(hipStream_t s, const GuardsGather& g, uint32_t* d_words, G1A* d_bases) {
    uint32_t total;
    if (int rc = guards_gather_check(g, d_words, d_bases, &total)) return rc;
    if (!total) return 0;
    hipLaunchKernelGGL(k_guards_gather<false>, dim3((total + 255) / 256), dim3(256), 0, s, g, total, reinterpret_cast<uint4*>(d_words), static_cast<void*>(d_bases));
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}
int guards_proofs_enqueue(hipStream_t s, const Fr* d_mult, const int* d_status, uint32_t first, uint32_t count, uint8_t* d_mult32, int* d_status_out) {
    if (!count || (!d_mult32 && !d_status_out)) return 0;
    if ((d_mult32 && !d_mult) || (d_status_out && !d_status)) { set_last_error("guards_proofs_enqueue: null argument"); return H2V_ERR_BAD_ARGUMENT; }
    if ((uintptr_t)d_mult32 & 15u) { set_last_error("guards_proofs_enqueue: the multipliers off a 16-byte boundary"); return H2V_ERR_BAD_ARGUMENT; }
    hipLaunchKernelGGL(k_guards_proofs, dim3((count + 255) / 256), dim3(256), 0, s, d_mult, d_status, first, count, reinterpret_cast<uint4*>(d_mult32), d_status_out);
    H2V_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace h2v
