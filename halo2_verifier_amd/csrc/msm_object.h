// The resident MSM object behind h2v_msm (include/h2v.h), and what accumulator.hip needs of it.
#pragma once
#include "ctx.h"
#include <memory>

#define H2V_MSM_MAX_TERMS ((size_t)1 << 24)   // per object: the limit guard_args_check applies per side
#define H2V_MSM_FIRST_CAPACITY ((size_t)256)  // terms of an object's first allocation; every later one at least doubles

// MSMKZG (poly/kzg/msm.rs:17-21): parallel lists of scalars and bases, here in the form the pooled MSM reads in place.
struct h2v_msm {
    h2v_ctx* ctx = nullptr;        // the device, the params (same_srs for every object of a call), the stream and the workspaces, under its lock
    h2v::DevBuf<uint32_t> scal;    // [8 cap] canonical little-endian words, 8 per term (MsmProblem: sstride 8); 32-byte aligned per term
    h2v::DevBuf<h2v::G1A> pts;     // [cap] affine Montgomery, (0, 0) = the identity (bstride 1)
    size_t n = 0, cap = 0;         // terms held; terms the two arrays hold.  What lies past n is not part of the object
};

namespace h2v {
// The locks of the distinct contexts of a call (nulls are skipped), taken in one global order and held until the holder goes: CtxLocks of
// msm_object.hip, the one place that says the order, for a caller outside it (h2v_batch_guards_append, batch.hip)
struct CtxLocks;
struct CtxLocksDelete { void operator()(CtxLocks* l) const; };
typedef std::unique_ptr<CtxLocks, CtxLocksDelete> CtxLocksPtr;
CtxLocksPtr lock_contexts(h2v_ctx* a, h2v_ctx* b);
// The two channels of a DualMSM (either may be null: empty) evaluated by one pooled launch into d_pair[0], d_pair[1] (device memory of
// ctx's device), under the locks of ctx and the objects' contexts, on ctx's stream, which is idle on return.  H2V_ERR_BAD_ARGUMENT
// before any device work when an object lies on another device or over other params than ctx.
// room for `need` terms in m: the capacity at least doubles, the contents are copied device to device on s, which is idle on return.
// On an error the object keeps its arrays.  The object's context lock is held.
int msm_object_reserve(h2v_msm* m, size_t need, hipStream_t s);
int msm_object_eval_pair(h2v_ctx* ctx, const char* who, h2v_msm* left, h2v_msm* right, G1J* d_pair);
}  // namespace h2v
