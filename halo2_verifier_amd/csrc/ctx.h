// The context object behind h2v_ctx (include/h2v.h).
#pragma once
#include "internal.h"
#include "pairing_api.h"
#include <mutex>

namespace h2v { struct VkDevice; }
struct h2v_batch;

namespace h2v {
// staging buffers of h2v_msm_g1, kept between calls (grow-only)
struct OneShotMsm {
    DevBuf<uint8_t> sb, bb, out; DevBuf<uint32_t> s, flags; DevBuf<G1A> b; DevBuf<G1J> res;
};
// Guards at the trait seam (h2v_accumulator_process_guards, h2v_guards_check_each; api.hip): guard i is counts[side][i] terms of each
// side, the terms of all guards of a call back to back in four flat arrays.
struct GuardArgs {
    size_t n;
    const size_t* counts[2];                      // [side][guard]
    const uint8_t* scalars[2]; const uint8_t* bases[2];   // [side]: 32 / 64 bytes per term
    std::vector<size_t> off[2];                   // guard_args_check: [side][guard] first term, n + 1 entries
};
// The terms of one launch on their way to the MSM: staged on the host as segments (one per MSM problem; a segment without a term holds
// one zero scalar under the identity, so that no problem of a launch is empty), copied, and converted by one k_guard_terms launch.
// Grow-only buffers, owned by whoever runs the launches (an accumulator, or the context under its lock).
struct GuardStage {
    DevBuf<uint8_t> sb, bb; DevBuf<uint32_t> gidx, scal, word; DevBuf<G1A> pts;
    std::vector<uint8_t> h_sb, h_bb, h_side;      // what sb / bb are copied from; per staged term its side
    std::vector<uint32_t> h_gidx, seg;            // per staged term its guard, counted from the launch's first; seg[q] = first staged term of segment q (+ the total)
    uint32_t h_word = 0xffffffffu;                // what `word` (k_guard_terms' validity word) is copied to
};
// null arrays that the counts say are read, n > 2^20, a side's total above 2^24 (H2V_ERR_BAD_ARGUMENT); fills g.off
int guard_args_check(const char* who, GuardArgs& g);
// Guards [g0, g1): the segments (per_guard: guard by guard its left and its right side; else every left term, then every right term), the
// copies, the conversion (d_mult: per guard of the launch, or null) and the copy of the validity word, all on s.  MSM problem q reads
// st.scal.p + 8 st.seg[q] and st.pts.p + st.seg[q], st.seg[q + 1] - st.seg[q] terms.
int guard_stage_enqueue(hipStream_t s, GuardStage& st, const GuardArgs& g, size_t g0, size_t g1, bool per_guard, const Fr* d_mult);
// after the synchronise: 0, or H2V_ERR_BAD_ARGUMENT with the guard and the side of the first bad term in the message
int guard_stage_verdict(const char* who, const GuardStage& st, size_t g0);
// What the resident MSM objects of a context (h2v_msm, msm_object.hip) share, under the context's lock (grow-only): the bytes of an
// append on their way in, the bytes of a read-back or an evaluation on their way out, and the one zero term on the identity that an
// empty object is evaluated as (8 zero words, then an all-zero G1A).  An object owns its two term arrays and nothing else.
struct MsmObjectStage {
    DevBuf<uint8_t> sb, bb, out; DevBuf<uint32_t> word, flags, zero;
    bool zero_ready = false;
};
}  // namespace h2v

struct h2v_ctx {
    int device = 0;
    h2v::ParamsHost params;
    h2v::PairingDevice pairing;
    h2v::MsmWorkspace msm_ws;      // used by h2v_msm_g1 only; batches and accumulators own their workspaces
    h2v::OneShotMsm one_shot;
    h2v::GuardStage guards;        // h2v_guards_check_each: the launch in flight, its workspace (sized for many small problems, where msm_ws
    h2v::MsmWorkspace guard_ws;    // is sized for one large one), its evaluated pairs and its verdicts
    h2v::DevBuf<h2v::G1J> guard_pairs; h2v::DevBuf<uint32_t> guard_ok;
    hipStream_t stream = nullptr;  // used by the synchronous single-shot entry points
    std::mutex mu;                 // serialises the single-shot entry points
    h2v::VkDevice* vk = nullptr;   // per-VK compiled program and constants (vkplan.hip)
    int multiopen = 0, transcript = 0, circuit_instances = 1;  // h2v_options
    int instance_kernel_threshold = 0;                         // h2v_options (debug): 0 = default
    h2v_tuning tuning = {};                                    // h2v_ctx_set_tuning (debug / test): forced kernel variants
    struct h2v_batch* scratch_batch = nullptr;  // kept between one-shot calls (h2v_verify_batch / _each): ~20 device allocations saved per call
    h2v::MsmObjectStage msm_objects;   // h2v_msm_*: staging shared by the context's resident MSM objects (they evaluate through guard_ws / guard_pairs / guard_ok)
};

namespace h2v {
// instance columns a proof of this context brings: circuit instances x the VK's instance columns (lib.rs:51-55)
size_t ctx_total_instance_columns(const h2v_ctx* ctx);
int ctx_load_vk(h2v_ctx* ctx, const uint8_t* vk, size_t vk_len, int vk_format);
void ctx_release_vk(h2v_ctx* ctx);
int affine_to_jacobian_enqueue(hipStream_t s, const G1A* d_in, G1J* d_out, uint32_t n);
}  // namespace h2v
