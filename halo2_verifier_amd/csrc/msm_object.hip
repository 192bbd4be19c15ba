// The resident MSM object behind h2v_msm (include/h2v.h): the reference's MSM trait (poly/commitment.rs:56-79) as MSMKZG implements it
// (poly/kzg/msm.rs:17-95), and DualMSM's check (msm.rs:185-203) over two such objects.
//
// An object is two grow-only device arrays in the form the pooled MSM reads in place — 8 canonical words per scalar, an affine
// Montgomery point per base — and a length.  Nothing else is per object: staging bytes, the MSM workspace, the evaluated points and the
// verdict words are the context's (ctx->msm_objects, guard_ws, guard_pairs, guard_ok), used under the context's lock on the context's
// stream, so there may be an object per Guard.
//   append_terms   bytes -> staging -> k_guard_terms writes words and points directly behind the object's end; the validity word comes
//                  back with the call's one synchronise, and the length grows only if it is clean
//   add_msm        device-to-device copies behind the destination's end
//   scale          k_msm_scale over the words, in place (eager: a read-back shows the scaled values, as the reference's scalars() does)
//   terms          the words as they lie; the points through k_affine_to_bytes
//   eval_many      K objects = K problems of one msm_enqueue_multi whose descriptors point INTO the objects' arrays; an empty object is
//                  the context's one zero term on the identity.  Launches are cut the way h2v_guards_check_each cuts its own
//   dual_msm_check_many   2 K problems -> guard_pairs, one pairing_check_enqueue over the K pairs, one copy of K verdict words
// A launch per tiny object would be a bad trade, hence evaluation per many: the pooled kernels were built for many small problems.
//
// The commit rule (the library's, extended): a call that returns non-zero leaves every object it was given as it was — length,
// contents, read-back.  The length is the only thing a failing call could expose, and it is written after the call's synchronise.
// Growing an object (capacity at least doubles, contents copied device to device) changes nothing a caller can see.  Every call
// returns with the stream it used idle.
#include "../../include/h2v.h"
#include "batch.h"
#include "msm_object.h"
#include <string.h>
#include <algorithm>
#include <mutex>

using namespace h2v;

namespace h2v {
// the locks of the distinct contexts of a call, taken in one global order (by address) and held until the call returns
struct CtxLocks {
    std::vector<h2v_ctx*> c;
    bool held = false;
    void add(h2v_ctx* x) { if (x) c.push_back(x); }
    void lock() {
        std::sort(c.begin(), c.end());
        c.erase(std::unique(c.begin(), c.end()), c.end());
        for (h2v_ctx* x : c) x->mu.lock();
        held = true;
    }
    ~CtxLocks() { if (held) for (size_t i = c.size(); i-- > 0;) c[i]->mu.unlock(); }
};
void CtxLocksDelete::operator()(CtxLocks* l) const { delete l; }
CtxLocksPtr lock_contexts(h2v_ctx* a, h2v_ctx* b) {
    CtxLocksPtr l(new CtxLocks);
    l->add(a); l->add(b);
    l->lock();
    return l;
}
}  // namespace h2v

namespace {

struct Drain { hipStream_t s; ~Drain() { hipStreamSynchronize(s); } };

int bad(const char* who, const char* what) { set_last_error(std::string(who) + ": " + what); return H2V_ERR_BAD_ARGUMENT; }

// every object of a call lies on ctx's device, over ctx's params
int same_home(const char* who, const h2v_ctx* ctx, const h2v_msm* m) {
    if (m->ctx->device != ctx->device) return bad(who, "objects on different devices");
    if (m->ctx != ctx && !same_srs(m->ctx->params, ctx->params)) return bad(who, "objects over different params (g[0], g2 or s_g2 differ)");
    return 0;
}

// room for `need` terms: the capacity at least doubles, the contents are copied device to device on s (drained here, before the old
// arrays are freed).  On an error the object keeps its arrays.
int grow(h2v_msm* m, size_t need, hipStream_t s) {
    if (need <= m->cap) return 0;
    const size_t cap = std::min(std::max(std::max(need, 2 * m->cap), H2V_MSM_FIRST_CAPACITY), H2V_MSM_MAX_TERMS);
    DevBuf<uint32_t> scal; DevBuf<G1A> pts;
    int rc;
    if ((rc = scal.alloc(8 * cap)) || (rc = pts.alloc(cap))) return rc;
    if (m->n) {
        H2V_HIP_CHECK(hipMemcpyAsync(scal.p, m->scal.p, 32 * m->n, hipMemcpyDeviceToDevice, s));
        H2V_HIP_CHECK(hipMemcpyAsync(pts.p, m->pts.p, sizeof(G1A) * m->n, hipMemcpyDeviceToDevice, s));
        H2V_HIP_CHECK(hipStreamSynchronize(s));
    }
    m->scal = std::move(scal); m->pts = std::move(pts); m->cap = cap;
    return 0;
}

// The launches over P = units * K problems, problem q being objs[q] (null or without a term: the zero term).  units = 1: K objects;
// units = 2: K pairs (left, right), and a launch holds whole pairs, followed by the pairing over them.  Results per problem on the host:
// xy (64 P bytes) and ident (P flags) when asked for, ok (K verdicts) for pairs.  The last launch's points stay in ctx->guard_pairs.
// ctx's lock is held and its device is current.
int eval_launches(h2v_ctx* ctx, const char* who, h2v_msm* const* objs, size_t P, uint32_t units, std::vector<uint8_t>* xy, std::vector<uint32_t>* ident, std::vector<uint32_t>* ok) {
    hipStream_t s = ctx->stream;
    Drain drain{s};   // no return path leaves work behind on the context's stream
    MsmObjectStage& st = ctx->msm_objects;
    int rc;
    if ((rc = st.zero.reserve(8 + sizeof(G1A) / 4)) || (rc = st.out.reserve((size_t)64 * MSM_MAX_PROBLEMS)) || (rc = st.flags.reserve(MSM_MAX_PROBLEMS)) ||
        (rc = ctx->guard_pairs.reserve(MSM_MAX_PROBLEMS)) || (rc = ctx->guard_ok.reserve(MSM_MAX_PROBLEMS / 2))) return rc;
    if (!st.zero_ready) {
        H2V_HIP_CHECK(hipMemsetAsync(st.zero.p, 0, 32 + sizeof(G1A), s));   // a zero scalar, and (0, 0): the identity
        st.zero_ready = true;
    }
    if (xy) xy->assign(64 * P, 0);
    if (ident) ident->assign(P, 0);
    if (ok) ok->assign(P / units, 0);
    std::vector<uint32_t> terms;
    for (size_t q0 = 0; q0 < P;) {
        // the launch: problems [q0, q1), at most MSM_MAX_PROBLEMS, fewer where the MSM would cut them into more than it takes
        size_t q1 = q0;
        uint32_t total = 0, per = 1;
        terms.clear();
        while (q1 < P && q1 - q0 + units <= MSM_MAX_PROBLEMS) {
            uint32_t add = 0, big = 1;
            for (uint32_t u = 0; u < units; ++u) {
                const h2v_msm* m = objs[q1 + u];
                const uint32_t t = (uint32_t)std::max<size_t>(m ? m->n : 0, 1);
                terms.push_back(t); add += t; big = std::max(big, t);
            }
            if (q1 > q0 && (!msm_cuts_within_limit(terms.data(), terms.size()) || (uint64_t)total + add > (1u << 26))) { terms.resize(terms.size() - units); break; }
            total += add; per = std::max(per, big);
            q1 += units;
        }
        const uint32_t Q = (uint32_t)(q1 - q0);
        if ((rc = ctx->guard_ws.reserve(std::max(total, 1024u), Q, per))) return rc;
        MsmProblems pr;
        for (uint32_t q = 0; q < Q; ++q) {
            const h2v_msm* m = objs[q0 + q];
            if (m && m->n) pr.p.push_back(MsmProblem(m->scal.p, m->pts.p, ctx->guard_pairs.p + q, 8, 1, (uint32_t)m->n));
            else pr.p.push_back(MsmProblem(st.zero.p, reinterpret_cast<const G1A*>(st.zero.p + 8), ctx->guard_pairs.p + q, 8, 1, 1));
        }
        ctx->guard_ws.tune = ctx->tuning;
        if ((rc = msm_enqueue_multi(s, ctx->guard_ws, pr))) return rc;
        if (ok) {
            if ((rc = pairing_check_enqueue(s, ctx->pairing, ctx->guard_pairs.p, Q / 2, ctx->guard_ok.p))) return rc;
            H2V_HIP_CHECK(hipMemcpyAsync(ok->data() + q0 / 2, ctx->guard_ok.p, 4 * (size_t)(Q / 2), hipMemcpyDeviceToHost, s));
        }
        if (xy || ident) {
            if ((rc = point_to_bytes_enqueue(s, ctx->guard_pairs.p, st.out.p, st.flags.p, Q))) return rc;
            if (xy) H2V_HIP_CHECK(hipMemcpyAsync(xy->data() + 64 * q0, st.out.p, 64 * (size_t)Q, hipMemcpyDeviceToHost, s));
            if (ident) H2V_HIP_CHECK(hipMemcpyAsync(ident->data() + q0, st.flags.p, 4 * (size_t)Q, hipMemcpyDeviceToHost, s));
        }
        H2V_HIP_CHECK(hipStreamSynchronize(s));
        q0 = q1;
    }
    return 0;
}

}  // namespace

namespace h2v {
int msm_object_reserve(h2v_msm* m, size_t need, hipStream_t s) { return grow(m, need, s); }
int msm_object_eval_pair(h2v_ctx* ctx, const char* who, h2v_msm* left, h2v_msm* right, G1J* d_pair) {
    h2v_msm* objs[2] = {left, right};
    int rc;
    CtxLocks locks;
    locks.add(ctx);
    for (h2v_msm* m : objs) if (m) { if ((rc = same_home(who, ctx, m))) return rc; locks.add(m->ctx); }
    locks.lock();
    H2V_HIP_CHECK(hipSetDevice(ctx->device));
    if ((rc = eval_launches(ctx, who, objs, 2, 2, nullptr, nullptr, nullptr))) return rc;
    // (two problems are one launch: both points lie in guard_pairs, and the context's lock is still held)
    H2V_HIP_CHECK(hipMemcpyAsync(d_pair, ctx->guard_pairs.p, 2 * sizeof(G1J), hipMemcpyDeviceToDevice, ctx->stream));
    H2V_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}
}  // namespace h2v

extern "C" {

int h2v_msm_create(h2v_ctx* ctx, h2v_msm** out) {
    if (!ctx || !out) return bad("h2v_msm_create", "null argument");
    h2v_msm* m = new h2v_msm;
    m->ctx = ctx;
    *out = m;   // MSMKZG::new: no term, and no device memory until the first one
    return 0;
}

void h2v_msm_destroy(h2v_msm* m) {
    if (!m) return;
    {
        std::lock_guard<std::mutex> lock(m->ctx->mu);   // (no call of another thread has a launch over these arrays in flight)
        hipSetDevice(m->ctx->device);
        m->scal.reset(); m->pts.reset();
    }
    delete m;
}

int h2v_msm_append_terms(h2v_msm* m, const uint8_t* scalars32, const uint8_t* bases64, size_t n) {
    const char* who = "h2v_msm_append_terms";
    if (!m || (n && (!scalars32 || !bases64))) return bad(who, "null argument");
    if (n > H2V_MSM_MAX_TERMS || m->n + n > H2V_MSM_MAX_TERMS) return bad(who, "more than 2^24 terms in one object");
    if (!n) return 0;
    h2v_ctx* ctx = m->ctx;
    std::lock_guard<std::mutex> lock(ctx->mu);
    H2V_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    Drain drain{s};
    MsmObjectStage& st = ctx->msm_objects;
    const size_t cap = n < 1024 ? 1024 : n;
    int rc;
    if ((rc = st.sb.reserve(32 * cap)) || (rc = st.bb.reserve(64 * cap)) || (rc = st.word.reserve(1)) || (rc = grow(m, m->n + n, s))) return rc;
    uint32_t word = 0;
    H2V_HIP_CHECK(hipMemcpyAsync(st.sb.p, scalars32, 32 * n, hipMemcpyHostToDevice, s));
    H2V_HIP_CHECK(hipMemcpyAsync(st.bb.p, bases64, 64 * n, hipMemcpyHostToDevice, s));
    // directly behind the object's end: what is written there is not part of the object until the length says so
    if ((rc = guard_terms_enqueue(s, st.sb.p, st.bb.p, nullptr, nullptr, m->scal.p + 8 * m->n, m->pts.p + m->n, st.word.p, (uint32_t)n))) return rc;
    H2V_HIP_CHECK(hipMemcpyAsync(&word, st.word.p, 4, hipMemcpyDeviceToHost, s));
    H2V_HIP_CHECK(hipStreamSynchronize(s));
    if (word != 0xffffffffu) {
        if (word >= n) { set_last_error(std::string(who) + ": the validity word names a term the call does not have"); return H2V_ERR_DEVICE; }
        set_last_error(std::string(who) + ": term " + std::to_string(word) + ": a scalar that is not canonical, or a base that is neither all-zero nor a canonical point on the curve");
        return H2V_ERR_BAD_ARGUMENT;
    }
    m->n += n;
    return 0;
}

int h2v_msm_add_msm(h2v_msm* dst, const h2v_msm* src) {
    const char* who = "h2v_msm_add_msm";
    if (!dst || !src) return bad(who, "null argument");
    if (dst == src) return bad(who, "the source is the destination");
    if (int rc = same_home(who, dst->ctx, src)) return rc;
    if (dst->n + src->n > H2V_MSM_MAX_TERMS) return bad(who, "more than 2^24 terms in one object");
    if (!src->n) return 0;
    CtxLocks locks;
    locks.add(dst->ctx); locks.add(src->ctx);
    locks.lock();
    H2V_HIP_CHECK(hipSetDevice(dst->ctx->device));
    hipStream_t s = dst->ctx->stream;
    Drain drain{s};
    if (int rc = grow(dst, dst->n + src->n, s)) return rc;
    H2V_HIP_CHECK(hipMemcpyAsync(dst->scal.p + 8 * dst->n, src->scal.p, 32 * src->n, hipMemcpyDeviceToDevice, s));
    H2V_HIP_CHECK(hipMemcpyAsync(dst->pts.p + dst->n, src->pts.p, sizeof(G1A) * src->n, hipMemcpyDeviceToDevice, s));
    H2V_HIP_CHECK(hipStreamSynchronize(s));
    dst->n += src->n;
    return 0;
}

int h2v_msm_scale(h2v_msm* m, const uint8_t factor32[32]) {
    const char* who = "h2v_msm_scale";
    if (!m || !factor32) return bad(who, "null argument");
    Fr f;   // f R: the Montgomery form the kernel multiplies the words' integers by
    if (!Fr::from_bytes(factor32, f)) return bad(who, "factor not canonical");
    if (!m->n) return 0;
    std::lock_guard<std::mutex> lock(m->ctx->mu);
    H2V_HIP_CHECK(hipSetDevice(m->ctx->device));
    hipStream_t s = m->ctx->stream;
    Drain drain{s};
    // (the kernel is the call's only device work: it runs over all the terms or is not launched)
    if (int rc = msm_scale_enqueue(s, m->scal.p, f, (uint32_t)m->n)) return rc;
    H2V_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

int h2v_msm_len(const h2v_msm* m, size_t* n) {
    if (!m || !n) return bad("h2v_msm_len", "null argument");
    *n = m->n;
    return 0;
}

int h2v_msm_terms(h2v_msm* m, size_t first, size_t count, uint8_t* scalars32, uint8_t* bases64) {
    const char* who = "h2v_msm_terms";
    if (!m) return bad(who, "null argument");
    if (first > m->n || count > m->n - first) return bad(who, "a range outside the object");
    if (!count || (!scalars32 && !bases64)) return 0;
    h2v_ctx* ctx = m->ctx;
    std::lock_guard<std::mutex> lock(ctx->mu);
    H2V_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    Drain drain{s};
    int rc;
    std::vector<uint8_t> h_sc(scalars32 ? 32 * count : 0), h_bs(bases64 ? 64 * count : 0);   // (nothing is written on an error)
    if (scalars32) H2V_HIP_CHECK(hipMemcpyAsync(h_sc.data(), m->scal.p + 8 * first, 32 * count, hipMemcpyDeviceToHost, s));
    if (bases64) {
        MsmObjectStage& st = ctx->msm_objects;
        if ((rc = st.out.reserve(std::max<size_t>(64 * count, (size_t)64 * MSM_MAX_PROBLEMS)))) return rc;
        if ((rc = affine_to_bytes_enqueue(s, m->pts.p + first, st.out.p, (uint32_t)count))) return rc;
        H2V_HIP_CHECK(hipMemcpyAsync(h_bs.data(), st.out.p, 64 * count, hipMemcpyDeviceToHost, s));
    }
    H2V_HIP_CHECK(hipStreamSynchronize(s));
    if (scalars32) memcpy(scalars32, h_sc.data(), h_sc.size());
    if (bases64) memcpy(bases64, h_bs.data(), h_bs.size());
    return 0;
}

int h2v_msm_eval_many(h2v_msm* const* msms, size_t k, uint8_t* out_xy, int* out_is_identity) {
    const char* who = "h2v_msm_eval_many";
    if (k && !msms) return bad(who, "null argument");
    if (k > ((size_t)1 << 20)) return bad(who, "more than 2^20 objects");
    for (size_t i = 0; i < k; ++i) if (!msms[i]) return bad(who, "null object");
    if (!k) return 0;
    h2v_ctx* ctx = msms[0]->ctx;
    int rc;
    CtxLocks locks;
    for (size_t i = 0; i < k; ++i) { if ((rc = same_home(who, ctx, msms[i]))) return rc; locks.add(msms[i]->ctx); }
    locks.lock();
    H2V_HIP_CHECK(hipSetDevice(ctx->device));
    std::vector<uint8_t> xy; std::vector<uint32_t> ident;
    if ((rc = eval_launches(ctx, who, msms, k, 1, &xy, &ident, nullptr))) return rc;
    if (out_xy) memcpy(out_xy, xy.data(), 64 * k);   // nothing is written on an error
    if (out_is_identity) for (size_t i = 0; i < k; ++i) out_is_identity[i] = ident[i] ? 1 : 0;
    return 0;
}

int h2v_dual_msm_check_many(h2v_msm* const* lefts, h2v_msm* const* rights, size_t k, int* ok, uint8_t* out_left_xy, uint8_t* out_right_xy) {
    const char* who = "h2v_dual_msm_check_many";
    if (k && (!lefts || !rights || !ok)) return bad(who, "null argument");
    if (k > ((size_t)1 << 20)) return bad(who, "more than 2^20 pairs");
    for (size_t i = 0; i < k; ++i) if (!lefts[i] || !rights[i]) return bad(who, "null object");
    if (!k) return 0;
    h2v_ctx* ctx = lefts[0]->ctx;
    int rc;
    CtxLocks locks;
    std::vector<h2v_msm*> objs(2 * k);
    for (size_t i = 0; i < k; ++i) {
        objs[2 * i] = lefts[i]; objs[2 * i + 1] = rights[i];
        if ((rc = same_home(who, ctx, lefts[i])) || (rc = same_home(who, ctx, rights[i]))) return rc;
        locks.add(lefts[i]->ctx); locks.add(rights[i]->ctx);
    }
    locks.lock();
    H2V_HIP_CHECK(hipSetDevice(ctx->device));
    const bool want_xy = out_left_xy || out_right_xy;
    std::vector<uint8_t> xy; std::vector<uint32_t> verdicts;
    if ((rc = eval_launches(ctx, who, objs.data(), 2 * k, 2, want_xy ? &xy : nullptr, nullptr, &verdicts))) return rc;
    for (size_t i = 0; i < k; ++i) {   // nothing is written on an error
        ok[i] = verdicts[i] ? 1 : 0;
        if (out_left_xy) memcpy(out_left_xy + 64 * i, &xy[128 * i], 64);
        if (out_right_xy) memcpy(out_right_xy + 64 * i, &xy[128 * i + 64], 64);
    }
    return 0;
}

}  // extern "C"
