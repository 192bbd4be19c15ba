// C++ host-side mirror of the reference's surface for the accelerated path, over the C ABI in h2v.h.
//
// The reference is a Rust crate; a Rust toolchain is not available where this library is built, so the host side
// above the C ABI is offered in C++ (this header; header-only, C++17) and in Python (halo2_verifier_amd/verifier.py),
// and as uncompiled Rust source in integration/rust/.  Names, argument meaning and error behaviour follow the reference:
//
//   reference (halo2_verifier)                                   here (namespace halo2_verifier)
//   ---------------------------------------------------------    ---------------------------------------------
//   helpers::SerdeFormat                  helpers.rs:7-19         SerdeFormat
//   plonk::Error                          plonk/mod.rs:19-32      Error (same order: InvalidInstances = -1 ...)
//   ParamsKZG::read_custom                kzg/commitment.rs:155   ParamsKZG(bytes, format)
//   VerifyingKey::read                    plonk/vk.rs:76-115      VerifyingKey(bytes, format)
//   verify_proof(params, vk, strategy, instances, transcript)     verify_proof(params, vk, strategy, instances, proof)
//                                         lib.rs:33-49
//   AccumulatorStrategy::{new, process, finalize}                 AccumulatorStrategy(params): verify_proof() queues,
//                                         kzg/strategy.rs:99-141    finalize() runs the batch on the GPU
//   SingleStrategy                        kzg/strategy.rs:143-181 SingleStrategy(params): verify_proof() runs at once
//   AccumulatorStrategy used incrementally (process per proof,    Accumulator(context): process() runs a run of proofs at once into
//     finalize when the caller decides, with)  kzg/strategy.rs:69-140   two points resident on the GPU; add_msm(), read(), finalize()
//   the same two strategies handed the Guards of a verify_proof   Accumulator::process_guards(guards, rand32), check_guards(context, guards):
//     that ran on the CPU       kzg/strategy.rs:125-136, 164-176     a Guard is the two term lists of its DualMSM
//   MSM trait: MSMKZG, DualMSM    poly/commitment.rs:56-79,       Msm(context), DualMsm(context): the terms resident on the GPU; append_terms, add_msm,
//                                 kzg/msm.rs:17-95, 146-204         scale, scalars, bases; Msm::eval_many, DualMsm::check_many, Accumulator::add_msms
//   VerifierSHPLONK / VerifierGWC, Blake2bRead / Keccak256Read    MultiOpen, TranscriptKind (generic parameters of lib.rs:33-40)
//
// There is no CPU fallback: constructing a Context without a HIP device throws Failure{H2V_ERR_DEVICE}.
#pragma once
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "h2v.h"

namespace halo2_verifier {

enum class SerdeFormat : int { Processed = H2V_SERDE_PROCESSED, RawBytes = H2V_SERDE_RAW_BYTES, RawBytesUnchecked = H2V_SERDE_RAW_BYTES_UNCHECKED };
enum class MultiOpen : int { SHPLONK = H2V_MULTIOPEN_SHPLONK, GWC = H2V_MULTIOPEN_GWC };
enum class TranscriptKind : int { Blake2b = H2V_TRANSCRIPT_BLAKE2B, Keccak256 = H2V_TRANSCRIPT_KECCAK256 };

// plonk::Error (plonk/mod.rs:19-32), in declaration order
enum class Error : int {
    Ok = 0,
    InvalidInstances = H2V_ERR_INVALID_INSTANCES,
    ConstraintSystemFailure = H2V_ERR_CONSTRAINT_SYSTEM_FAILURE,
    BoundsFailure = H2V_ERR_BOUNDS_FAILURE,
    Opening = H2V_ERR_OPENING,
    Transcript = H2V_ERR_TRANSCRIPT,
    InstanceTooLarge = H2V_ERR_INSTANCE_TOO_LARGE,
};

// a failure of the library itself (bad argument, malformed VK / params, no device), as opposed to a proof that does not verify
struct Failure : std::runtime_error {
    int code;
    Failure(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};
inline void check(int rc) { if (rc != 0) throw Failure(rc, h2v_last_error()); }

typedef std::vector<uint8_t> Bytes;
typedef std::vector<Bytes> Column;            // one instance column: 32-byte little-endian canonical Fr values
typedef std::vector<Column> Instances;        // one circuit instance: its columns (the reference's &[&[Fr]]); with circuit_instances = M
                                              // (lib.rs:43: instances.len()) the M x columns of the transcript's instances, instance by instance

struct ParamsKZG { Bytes bytes; SerdeFormat format = SerdeFormat::RawBytes; };
struct VerifyingKey { Bytes bytes; SerdeFormat format = SerdeFormat::RawBytes; };

// ParamsKZG + VerifyingKey resident on one GPU (h2v_ctx)
class Context {
public:
    Context(const ParamsKZG& p, const VerifyingKey& vk, int device = 0, MultiOpen mo = MultiOpen::SHPLONK, TranscriptKind tr = TranscriptKind::Blake2b,
            int circuit_instances = 1) {
        h2v_options o = H2V_OPTIONS_INIT;
        o.multiopen = (int)mo; o.transcript = (int)tr; o.circuit_instances = circuit_instances;
        check(h2v_ctx_create_ex(p.bytes.data(), p.bytes.size(), (int)p.format, vk.bytes.data(), vk.bytes.size(), (int)vk.format, device, &o, &h_));
    }
    ~Context() { if (h_) h2v_ctx_destroy(h_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    h2v_ctx* handle() const { return h_; }

private:
    h2v_ctx* h_ = nullptr;
};

// The Guard a CPU verify_proof returns (kzg/strategy.rs:164-176: its DualMSM), as two term lists: scalars 32 bytes each, bases 64 bytes
// (x | y, all-zero = the identity) each; either side may be empty
struct Guard { Bytes left_scalars, left_bases, right_scalars, right_bases; };

// A device-resident MSMKZG (h2v_msm): the reference's MSM trait (poly/commitment.rs:56-79, poly/kzg/msm.rs:17-95) over terms kept on the
// context's GPU.  Move-only; the context must outlive the object.  Scalars 32 bytes each, bases 64 bytes (x | y, all-zero = the identity)
// each.  A Failure leaves the object as it was.  Evaluation is offered for many objects per launch: eval_many.
class Msm {
public:
    struct Evaluated { Bytes xy; std::vector<bool> is_identity; };   // k x 64 bytes, and MSMKZG::check per object
    explicit Msm(const Context& ctx) : ctx_(ctx.handle()) { halo2_verifier::check(h2v_msm_create(ctx_, &h_)); }
    ~Msm() { h2v_msm_destroy(h_); }
    Msm(const Msm&) = delete;
    Msm& operator=(const Msm&) = delete;
    Msm(Msm&& o) noexcept : ctx_(o.ctx_), h_(o.h_) { o.h_ = nullptr; }
    Msm& operator=(Msm&& o) noexcept { if (this != &o) { h2v_msm_destroy(h_); ctx_ = o.ctx_; h_ = o.h_; o.h_ = nullptr; } return *this; }
    h2v_msm* handle() const { return h_; }
    size_t size() const { size_t n = 0; halo2_verifier::check(h2v_msm_len(live(), &n)); return n; }
    void append_term(const Bytes& scalar32, const Bytes& base64) { append_terms(scalar32, base64); }                      // msm.rs:57-60
    void append_terms(const Bytes& scalars, const Bytes& bases) {
        if (scalars.size() % 32 || bases.size() != 2 * scalars.size()) throw Failure(H2V_ERR_BAD_ARGUMENT, "terms are n 32-byte scalars and n 64-byte bases");
        halo2_verifier::check(h2v_msm_append_terms(live(), scalars.data(), bases.data(), scalars.size() / 32));
    }
    void add_msm(const Msm& other) { halo2_verifier::check(h2v_msm_add_msm(live(), other.live())); }                                      // msm.rs:62-65
    void scale(const Bytes& factor32) {                                                                                   // msm.rs:67-75
        if (factor32.size() != 32) throw Failure(H2V_ERR_BAD_ARGUMENT, "a factor is 32 bytes");
        halo2_verifier::check(h2v_msm_scale(live(), factor32.data()));
    }
    Bytes scalars() const { const size_t n = size(); Bytes s(32 * n); halo2_verifier::check(h2v_msm_terms(h_, 0, n, s.data(), nullptr)); return s; }   // msm.rs:92-94
    Bytes bases() const { const size_t n = size(); Bytes b(64 * n); halo2_verifier::check(h2v_msm_terms(h_, 0, n, nullptr, b.data())); return b; }     // msm.rs:88-90
    Bytes eval() const { return eval_many({this}).xy; }                                                                   // msm.rs:81-86
    bool check() const      { return eval_many({this}).is_identity[0]; }                                                  // MSM::check, msm.rs:77-79
    Msm clone() const { Msm c(ctx_, nullptr); c.add_msm(*this); return c; }   // create + add_msm: independent of its source
    // MSM::eval for k objects, one pooled launch per 1024 of them; the same object may occur more than once
    static Evaluated eval_many(const std::vector<const Msm*>& msms) {
        Evaluated e;
        if (msms.empty()) return e;
        std::vector<h2v_msm*> hs;
        for (const Msm* m : msms) { if (!m) throw Failure(H2V_ERR_BAD_ARGUMENT, "null object"); hs.push_back(m->live()); }
        e.xy.resize(64 * hs.size());
        std::vector<int> ident(hs.size(), 0);
        halo2_verifier::check(h2v_msm_eval_many(hs.data(), hs.size(), e.xy.data(), ident.data()));
        for (int v : ident) e.is_identity.push_back(v != 0);
        return e;
    }

private:
    Msm(h2v_ctx* ctx, std::nullptr_t) : ctx_(ctx) { halo2_verifier::check(h2v_msm_create(ctx_, &h_)); }
    h2v_msm* live() const { if (!h_) throw Failure(H2V_ERR_BAD_ARGUMENT, "a moved-from Msm"); return h_; }
    h2v_ctx* ctx_ = nullptr;
    h2v_msm* h_ = nullptr;
};

// DualMSM (poly/kzg/msm.rs:146-204): two resident channels and the pairing e(left, s_g2) e(right, -g2) == 1.  Move-only.
class DualMsm {
public:
    struct Checked { std::vector<bool> ok; Bytes lefts, rights; };   // per object the raw pairing bit and the evaluated channels (k x 64 bytes each)
    explicit DualMsm(const Context& ctx) : left(ctx), right(ctx) {}
    DualMsm(Msm&& l, Msm&& r) : left(std::move(l)), right(std::move(r)) {}
    DualMsm(DualMsm&&) = default;
    DualMsm& operator=(DualMsm&&) = default;
    Msm left, right;
    void scale(const Bytes& factor32) {                                                                                   // msm.rs:173-177
        if (factor32.size() != 32) throw Failure(H2V_ERR_BAD_ARGUMENT, "a factor is 32 bytes");
        left.scale(factor32); right.scale(factor32);
    }
    void add_msm(const DualMsm& other) { left.add_msm(other.left); right.add_msm(other.right); }                          // msm.rs:179-183
    void add_guard(const Guard& g) { left.append_terms(g.left_scalars, g.left_bases); right.append_terms(g.right_scalars, g.right_bases); }
    bool check() const { return check_many({this}).ok[0]; }                                                               // msm.rs:185-203
    // DualMSM::check for k objects: per 512 of them one pooled MSM over the 2 k channels and one pairing launch
    static Checked check_many(const std::vector<const DualMsm*>& duals) {
        Checked c;
        if (duals.empty()) return c;
        std::vector<h2v_msm*> ls, rs;
        for (const DualMsm* d : duals) {
            if (!d || !d->left.handle() || !d->right.handle()) throw Failure(H2V_ERR_BAD_ARGUMENT, "a null or moved-from DualMsm");
            ls.push_back(d->left.handle()); rs.push_back(d->right.handle());
        }
        std::vector<int> ok(duals.size(), 0);
        c.lefts.resize(64 * duals.size()); c.rights.resize(64 * duals.size());
        halo2_verifier::check(h2v_dual_msm_check_many(ls.data(), rs.data(), duals.size(), ok.data(), c.lefts.data(), c.rights.data()));
        for (int v : ok) c.ok.push_back(v != 0);
        return c;
    }
};

namespace detail {
// The arguments of a call in the layout the C ABI takes: a context per key, then every proof in call order with its key and its column
// lengths.  The entry points over one context and one instance shape take key 0's column count and proof 0's shape (shape0()).
struct Marshalled {
    std::vector<h2v_ctx*> ctxs;
    std::vector<size_t> ncols;                 // the instance column count of every key
    std::vector<uint32_t> keys;                // the key of every proof
    std::vector<const uint8_t*> proofs, insts;
    std::vector<size_t> lens, col_lens;        // col_lens: proof by proof, ncols[key] entries each
    bool uniform = true;                       // every proof has proof 0's key and instance shape
    std::vector<Bytes> flat;
    // one_key: the calls over a single context hand proof 0's column count over and leave its judgement to the library
    // (H2V_ERR_INVALID_INSTANCES, lib.rs:51-55); the later proofs must agree with it, as the proofs of every key must with the key's count
    explicit Marshalled(bool one_key = false) : one_key_(one_key) {}
    void add_key(h2v_ctx* ctx) {
        ctxs.push_back(ctx);
        ncols.push_back(0);
        check(h2v_ctx_proof_shape(ctx, nullptr, nullptr, nullptr, nullptr, &ncols.back()));
    }
    void add(uint32_t key, const Instances& inst, const Bytes& proof) {
        if (key >= ctxs.size()) throw Failure(H2V_ERR_BAD_ARGUMENT, "key index out of range");
        if (one_key_ && keys.empty()) ncols[0] = inst.size();
        if (inst.size() != ncols[key]) throw Failure(H2V_ERR_INVALID_INSTANCES, "instances do not match the VK's instance column count");
        Bytes f;
        for (size_t c = 0; c < inst.size(); ++c) {
            if (!keys.empty() && (key != keys[0] || inst[c].size() != col_lens[c])) uniform = false;   // verify_proof takes `instances` per call: shapes may differ
            col_lens.push_back(inst[c].size());
            for (const Bytes& v : inst[c]) f.insert(f.end(), v.begin(), v.end());
        }
        flat.push_back(std::move(f));
        keys.push_back(key); proofs.push_back(proof.data()); lens.push_back(proof.size()); insts.push_back(flat.back().data());
    }
    size_t n() const { return keys.size(); }
    const size_t* shape0() { if (keys.empty()) col_lens.assign(ncols[0], 0); return col_lens.data(); }   // (no proofs: empty columns)

private:
    bool one_key_;
};
// Guards in the layout h2v_accumulator_process_guards / h2v_guards_check_each take: a count per guard and side, the terms of all guards
// back to back in guard order; every length the C side indexes is checked here
struct FlatGuards {
    std::vector<size_t> left_counts, right_counts;
    Bytes ls, lb, rs, rb;
    explicit FlatGuards(const std::vector<Guard>& guards) {
        for (const Guard& g : guards) {
            if (g.left_scalars.size() % 32 || g.left_bases.size() != 2 * g.left_scalars.size() || g.right_scalars.size() % 32 || g.right_bases.size() != 2 * g.right_scalars.size())
                throw Failure(H2V_ERR_BAD_ARGUMENT, "a guard's channel is n 32-byte scalars and n 64-byte bases");
            left_counts.push_back(g.left_scalars.size() / 32); right_counts.push_back(g.right_scalars.size() / 32);
            ls.insert(ls.end(), g.left_scalars.begin(), g.left_scalars.end()); lb.insert(lb.end(), g.left_bases.begin(), g.left_bases.end());
            rs.insert(rs.end(), g.right_scalars.begin(), g.right_scalars.end()); rb.insert(rb.end(), g.right_bases.begin(), g.right_bases.end());
        }
    }
};
inline void check_channels(const Bytes& ls, const Bytes& lb, const Bytes& rs, const Bytes& rb, const char* what) {
    if (ls.size() % 32 || lb.size() != 2 * ls.size() || rs.size() % 32 || rb.size() != 2 * rs.size()) throw Failure(H2V_ERR_BAD_ARGUMENT, what);
}
}  // namespace detail

// kzg/strategy.rs:99-141: verify_proof() adds a proof to the accumulator, finalize() runs ONE pairing for all of them.
// Here the proofs are queued on the host and the whole batch runs on the GPU at finalize().
class AccumulatorStrategy {
public:
    explicit AccumulatorStrategy(const ParamsKZG& p, int device = 0, MultiOpen mo = MultiOpen::SHPLONK, TranscriptKind tr = TranscriptKind::Blake2b,
                                 int circuit_instances = 1)
        : params_(p), device_(device), mo_(mo), tr_(tr), ci_(circuit_instances) {}
    // AccumulatorStrategy::with(msm_accumulator) (kzg/strategy.rs:75-78): start from an existing DualMSM; the channels are term lists
    // as MSMKZG holds them — scalars 32 bytes each, bases 64 bytes (x | y) each.  A finished accumulation resumes with scalar 1 and
    // its evaluated channels (left(), right()) as the single base of either side.
    static AccumulatorStrategy with(const ParamsKZG& p, Bytes left_scalars, Bytes left_bases, Bytes right_scalars, Bytes right_bases, int device = 0,
                                    MultiOpen mo = MultiOpen::SHPLONK, TranscriptKind tr = TranscriptKind::Blake2b, int circuit_instances = 1) {
        detail::check_channels(left_scalars, left_bases, right_scalars, right_bases, "a seed channel is n 32-byte scalars and n 64-byte bases");
        AccumulatorStrategy s(p, device, mo, tr, circuit_instances);
        s.seeded_ = true;
        s.seed_ls_ = std::move(left_scalars); s.seed_lb_ = std::move(left_bases); s.seed_rs_ = std::move(right_scalars); s.seed_rb_ = std::move(right_bases);
        return s;
    }
    // rand32: the Fr::random draws of process() (kzg/strategy.rs:129), one 32-byte canonical scalar per proof; empty = OS RNG
    void set_randomness(Bytes rand32) { rand_ = std::move(rand32); }
    // verify_proof takes a VK per call (lib.rs:33-49): proofs of several VerifyingKeys over the same params may share one strategy
    void push(const VerifyingKey& vk, Instances inst, Bytes proof) {
        size_t k = 0;
        while (k < vks_.size() && !(vks_[k].bytes == vk.bytes && vks_[k].format == vk.format)) ++k;
        if (k == vks_.size()) vks_.push_back(vk);
        key_of_.push_back((uint32_t)k);
        items_.emplace_back(std::move(inst), std::move(proof));
    }
    // -> true iff every verify_proof succeeded and the pairing check passed; statuses() then holds the per-proof plonk::Error.
    // Proofs of several VerifyingKeys: a context per key, every proof in call order (h2v_verify_batch_keys)
    bool finalize() { return run(false, vks_.size() > 1); }
    // finalize() plus the proofs that made the batch fail (h2v_verify_batch_identify): returns what finalize() returns, and statuses()
    // then holds, for every proof, the plonk::Error SingleStrategy reports for it — ConstraintSystemFailure for the proofs whose own
    // pairing fails.  The draws must be non-zero.  One instance shape.  A seeded accumulation (with) runs
    // h2v_verify_batch_seeded_identify: the seed enters no proof's check, and seed_ok() says whether the seed alone passes the pairing.
    bool finalize_identify() {
        if (vks_.size() > 1) throw Failure(H2V_ERR_UNSUPPORTED, "identification takes proofs of one VerifyingKey");
        return run(true, false);
    }
    // finalize_identify() over one or several VerifyingKeys and any instance shapes (h2v_verify_batch_keys_identify): returns what
    // finalize() returns, statuses() then holds every proof's SingleStrategy verdict and range_checks() the re-checks the search ran.
    // The draws must be non-zero; no seed.
    bool finalize_identify_keys() {
        if (seeded_) throw Failure(H2V_ERR_UNSUPPORTED, "identification takes an accumulation without a seed");
        range_checks_ = 0;
        if (items_.empty()) { statuses_.clear(); return true; }   // an empty DualMSM: both channels are the identity
        return run(true, true);
    }
    bool seed_ok() const { return seed_ok_; }               // the last finalize_identify(): the seed alone passes the pairing (true without a seed)
    size_t range_checks() const { return range_checks_; }   // re-checks the last finalize_identify() or finalize_identify_keys() ran (0: the batch passed)
    const std::vector<int>& statuses() const { return statuses_; }
    const uint8_t* left() const { return left_; }     // evaluated channels of the final DualMSM, canonical x|y
    const uint8_t* right() const { return right_; }

private:
    // Every finalizer.  keyed: the call over a context per VerifyingKey and per-proof shapes (h2v_verify_batch_keys*), else the call over
    // one context (h2v_verify_batch*, which a strategy without proofs reaches with an empty key).  The keyed calls have always refused
    // the draws before a context is made, the others after the proofs were looked at: kept.
    bool run(bool identify, bool keyed) {
        if (keyed && seeded_) throw Failure(H2V_ERR_UNSUPPORTED, "a seeded accumulation takes proofs of one VerifyingKey");
        const size_t n = items_.size();
        const auto check_draws = [&] { if (!rand_.empty() && rand_.size() != 32 * n) throw Failure(H2V_ERR_BAD_ARGUMENT, "one 32-byte draw per proof"); };
        if (keyed) check_draws();
        std::vector<std::unique_ptr<Context>> ctxs;
        detail::Marshalled m(!keyed);
        for (const VerifyingKey& vk : vks_.empty() ? std::vector<VerifyingKey>(1) : vks_) {
            ctxs.emplace_back(new Context(params_, vk, device_, mo_, tr_, ci_));
            m.add_key(ctxs.back()->handle());
        }
        for (size_t i = 0; i < n; ++i) m.add(key_of_[i], items_[i].first, items_[i].second);
        if (!keyed) {
            if (identify && !m.uniform) throw Failure(H2V_ERR_UNSUPPORTED, "identification takes one instance shape");
            check_draws();
            if (seeded_ && !m.uniform) throw Failure(H2V_ERR_UNSUPPORTED, "a seeded accumulation takes one instance shape");
        }
        statuses_.assign(n ? n : 1, 0);
        const uint8_t* rand = rand_.empty() ? nullptr : rand_.data();
        const size_t n_ls = seed_ls_.size() / 32, n_rs = seed_rs_.size() / 32;
        int ok = 0, seed_ok = 1;
        if (keyed && identify)
            check(h2v_verify_batch_keys_identify(m.ctxs.data(), m.ctxs.size(), m.keys.data(), n, m.proofs.data(), m.lens.data(), m.insts.data(), m.ncols.data(),
                                                 m.col_lens.data(), rand, statuses_.data(), &ok, left_, right_, &range_checks_));
        else if (keyed)
            check(h2v_verify_batch_keys(m.ctxs.data(), m.ctxs.size(), m.keys.data(), n, m.proofs.data(), m.lens.data(), m.insts.data(), m.ncols.data(),
                                        m.col_lens.data(), rand, statuses_.data(), &ok, left_, right_));
        else if (identify && seeded_)
            check(h2v_verify_batch_seeded_identify(m.ctxs[0], n, m.proofs.data(), m.lens.data(), m.insts.data(), m.ncols[0], m.shape0(), rand, seed_ls_.data(),
                                                   seed_lb_.data(), n_ls, seed_rs_.data(), seed_rb_.data(), n_rs, statuses_.data(), &ok, &seed_ok, left_, right_,
                                                   &range_checks_));
        else if (identify)
            check(h2v_verify_batch_identify(m.ctxs[0], n, m.proofs.data(), m.lens.data(), m.insts.data(), m.ncols[0], m.shape0(), rand, statuses_.data(), &ok,
                                            left_, right_, &range_checks_));
        else if (seeded_)
            check(h2v_verify_batch_seeded(m.ctxs[0], n, m.proofs.data(), m.lens.data(), m.insts.data(), m.ncols[0], m.shape0(), rand, seed_ls_.data(),
                                          seed_lb_.data(), n_ls, seed_rs_.data(), seed_rb_.data(), n_rs, statuses_.data(), &ok, left_, right_));
        else if (m.uniform)
            check(h2v_verify_batch(m.ctxs[0], n, m.proofs.data(), m.lens.data(), m.insts.data(), m.ncols[0], m.shape0(), rand, statuses_.data(), &ok, left_, right_));
        else
            check(h2v_verify_batch_shapes(m.ctxs[0], n, m.proofs.data(), m.lens.data(), m.insts.data(), m.ncols[0], m.col_lens.data(), rand, statuses_.data(), &ok,
                                          left_, right_));
        if (identify && !keyed) seed_ok_ = seed_ok != 0;
        statuses_.resize(n);
        return ok != 0;
    }

    ParamsKZG params_; std::vector<VerifyingKey> vks_; int device_; MultiOpen mo_; TranscriptKind tr_; int ci_;
    std::vector<uint32_t> key_of_;   // the key (index into vks_) of every queued proof
    std::vector<std::pair<Instances, Bytes>> items_;
    Bytes rand_;
    bool seeded_ = false;
    Bytes seed_ls_, seed_lb_, seed_rs_, seed_rb_;
    std::vector<int> statuses_;
    size_t range_checks_ = 0;
    bool seed_ok_ = true;
    uint8_t left_[64] = {0}, right_[64] = {0};
};

// A resident AccumulatorStrategy (h2v_accumulator): the strategy's two accumulator points stay on the GPU across calls.  process()
// feeds proofs as they arrive — any mix of keys (a Context each) and instance shapes over the context's params — and finalize() runs the
// one pairing whenever the caller decides (kzg/strategy.rs:125-140): process(A); process(B); finalize() equals one AccumulatorStrategy
// over A then B with the draws concatenated.  The context supplies the device, the params and the pairing tables, and must outlive the object.
class Accumulator {
public:
    struct Item { uint32_t key; Instances instances; Bytes proof; };   // proof of contexts[key]
    explicit Accumulator(const Context& ctx) { check(h2v_accumulator_create(ctx.handle(), &h_)); }
    ~Accumulator() { h2v_accumulator_destroy(h_); }
    Accumulator(const Accumulator&) = delete;
    Accumulator& operator=(const Accumulator&) = delete;
    // n x verify_proof on this accumulator; rand32: one 32-byte draw per item, or empty = OS RNG.  -> the statuses of this call's proofs
    // (all_ok(): whether all are 0).  A Failure leaves the accumulator as it was.
    std::vector<int> process(const std::vector<const Context*>& contexts, const std::vector<Item>& items, const Bytes& rand32 = Bytes()) {
        if (contexts.empty()) throw Failure(H2V_ERR_BAD_ARGUMENT, "at least one context");
        if (!rand32.empty() && rand32.size() != 32 * items.size()) throw Failure(H2V_ERR_BAD_ARGUMENT, "one 32-byte draw per proof");
        detail::Marshalled m;
        for (const Context* c : contexts) m.add_key(c->handle());
        for (const Item& it : items) m.add(it.key, it.instances, it.proof);
        std::vector<int> st(items.size() ? items.size() : 1, 0);
        int ok = 0;
        check(h2v_accumulator_process(h_, m.ctxs.data(), m.ctxs.size(), m.keys.data(), items.size(), m.proofs.data(), m.lens.data(), m.insts.data(), m.ncols.data(),
                                      m.col_lens.data(), rand32.empty() ? nullptr : rand32.data(), st.data(), &ok));
        all_ok_ = ok != 0;
        st.resize(items.size());
        return st;
    }
    bool all_ok() const { return all_ok_; }
    h2v_accumulator* handle() const { return h_; }   // for the extensions of the C ABI (h2v_hints.hpp: hints::process)
    // AccumulatorStrategy::with / DualMSM::add_msm: (L, R) += the two term lists evaluated, unscaled — scalars 32 bytes each, bases 64 bytes (x | y) each
    void add_msm(const Bytes& left_scalars, const Bytes& left_bases, const Bytes& right_scalars, const Bytes& right_bases) {
        detail::check_channels(left_scalars, left_bases, right_scalars, right_bases, "a channel is n 32-byte scalars and n 64-byte bases");
        check(h2v_accumulator_add_msm(h_, left_scalars.data(), left_bases.data(), left_scalars.size() / 32, right_scalars.data(), right_bases.data(),
                                      right_scalars.size() / 32));
    }
    // add_msm with both channels resident (h2v_accumulator_add_msms): evaluated in one pooled launch, added unscaled
    void add_msms(const DualMsm& msm) { add_msms(&msm.left, &msm.right); }
    void add_msms(const Msm* left, const Msm* right) {   // either may be null: empty
        if ((left && !left->handle()) || (right && !right->handle())) throw Failure(H2V_ERR_BAD_ARGUMENT, "a moved-from Msm");
        check(h2v_accumulator_add_msms(h_, left ? left->handle() : nullptr, right ? right->handle() : nullptr));
    }
    // n x (scale by the draw, add the Guard): AccumulatorStrategy::process at the trait seam (kzg/strategy.rs:125-136), the Guards made by a CPU
    // verify_proof.  rand32: one 32-byte canonical draw per guard; empty = OS RNG.  Equals process() over the proofs the Guards came from.
    void process_guards(const std::vector<Guard>& guards, const Bytes& rand32 = Bytes()) {
        if (!rand32.empty() && rand32.size() != 32 * guards.size()) throw Failure(H2V_ERR_BAD_ARGUMENT, "one 32-byte draw per guard");
        const detail::FlatGuards f(guards);
        check(h2v_accumulator_process_guards(h_, guards.size(), f.left_counts.data(), f.right_counts.data(), f.ls.data(), f.lb.data(), f.rs.data(), f.rb.data(),
                                             rand32.empty() ? nullptr : rand32.data()));
    }
    // The groups of a finished staged batch as legs, in group order (h2v_accumulator_process_batch): per group scale by its draws, add its
    // Guards' sum (kzg/strategy.rs:125-136, msm.rs:173-183) as the launch left it on the device.  Equals process() once per group.  The batch
    // is only read.  -> what the call added; all_ok(): whether no proof of the batch failed.  A Failure leaves the accumulator as it was.
    struct Added { size_t n_proofs, n_failed; };
    Added process_batch(h2v_batch* batch) {
        if (!batch) throw Failure(H2V_ERR_BAD_ARGUMENT, "process_batch takes a finished batch");
        Added added{0, 0};
        check(h2v_accumulator_process_batch(h_, batch, &added.n_proofs, &added.n_failed));
        all_ok_ = added.n_failed == 0;
        return added;
    }
    // the two points as canonical x | y (left(), right(); all-zero = identity) and the counters
    void read() { check(h2v_accumulator_read(h_, left_, right_, &n_proofs_, &n_failed_)); }
    // -> true iff the pairing of (L, R) passes and no processed proof failed; left() / right() hold the points.  The accumulator is not consumed.
    bool finalize() {
        int ok = 0;
        check(h2v_accumulator_finalize(h_, &ok, left_, right_));
        return ok != 0;
    }
    // The leg journal (h2v_accumulator_journal_begin): `capacity` entries, the base included, in [2, H2V_ACC_JOURNAL_MAX]; 0 = off.  The base is
    // the accumulator as it stands (AccumulatorStrategy::with, kzg/strategy.rs:76-78); on a journaled accumulator a checkpoint.
    void journal_begin(size_t capacity) {
        if (capacity == 1 || capacity > H2V_ACC_JOURNAL_MAX) throw Failure(H2V_ERR_BAD_ARGUMENT, "journal capacity must be 0 or in [2, H2V_ACC_JOURNAL_MAX]");
        check(h2v_accumulator_journal_begin(h_, capacity));
    }
    // DualMSM::check (kzg/msm.rs:185-203) of every entry's own sum, side by side in one launch; entry 0 is the base.  Empty with the journal off.
    struct Leg { size_t n_proofs, n_failed; bool pairing_ok; };
    std::vector<Leg> check_legs() {
        size_t n = 0;
        check(h2v_accumulator_check_legs(h_, 0, &n, nullptr, nullptr, nullptr));
        std::vector<size_t> proofs(n ? n : 1), failed(n ? n : 1);
        std::vector<int> ok(n ? n : 1, 0);
        check(h2v_accumulator_check_legs(h_, n, &n, proofs.data(), failed.data(), ok.data()));
        std::vector<Leg> legs;
        for (size_t e = 0; e < n; ++e) legs.push_back({proofs[e], failed[e], ok[e] != 0});
        return legs;
    }
    // Take entries out again (distinct, none 0, each below the entry count): the accumulator, the counters and the journal become those of
    // an accumulator that was never given the dropped calls (DualMSM::scale / add_msm over the kept entries, kzg/msm.rs:173-183)
    void drop_legs(const std::vector<size_t>& legs) {
        for (size_t i = 0; i < legs.size(); ++i) {
            if (legs[i] == 0) throw Failure(H2V_ERR_BAD_ARGUMENT, "the base entry cannot be dropped");
            for (size_t j = 0; j < i; ++j) if (legs[j] == legs[i]) throw Failure(H2V_ERR_BAD_ARGUMENT, "an entry index given twice");
        }
        check(h2v_accumulator_drop_legs(h_, legs.data(), legs.size()));
    }
    // One pairing for several accumulators (h2v_accumulator_merge): (L, R) += sum_k c_k (L_k, R_k), the counters += theirs — DualMSM::scale
    // and add_msm (kzg/msm.rs:173-183) per source, which is not changed.  draws32: one non-zero 32-byte draw per source, or empty = fresh
    // OS draws.  -> the draws used.  With the journal on every source leaves an entry.  A Failure leaves the accumulator as it was.
    Bytes merge(const std::vector<Accumulator*>& sources, const Bytes& draws32 = Bytes()) {
        check_merge(sources.size(), draws32);
        std::vector<h2v_accumulator*> hs;
        for (Accumulator* a : sources) {
            if (!a || a == this) throw Failure(H2V_ERR_BAD_ARGUMENT, "a source is null or the destination");
            hs.push_back(a->h_);
        }
        Bytes used(32 * sources.size() + 1);
        check(h2v_accumulator_merge(h_, hs.data(), hs.size(), draws32.empty() ? nullptr : draws32.data(), used.data()));
        used.resize(32 * sources.size());
        return used;
    }
    // The accumulator as H2V_ACC_STATE_BYTES bytes (h2v_accumulator_export_state: the counters and the two affine points), for a
    // merge_states on another device or in another process.  A state carries no SRS: the importer cannot check it.
    Bytes export_state() {
        Bytes out(H2V_ACC_STATE_BYTES);
        check(h2v_accumulator_export_state(h_, out.data()));
        return out;
    }
    // merge over exported states, concatenated (h2v_accumulator_merge_states).  -> the draws used.
    Bytes merge_states(const Bytes& states, const Bytes& draws32 = Bytes()) {
        if (states.size() % H2V_ACC_STATE_BYTES) throw Failure(H2V_ERR_BAD_ARGUMENT, "states are H2V_ACC_STATE_BYTES bytes each");
        const size_t n = states.size() / H2V_ACC_STATE_BYTES;
        check_merge(n, draws32);
        Bytes used(32 * n + 1);
        check(h2v_accumulator_merge_states(h_, states.data(), n, draws32.empty() ? nullptr : draws32.data(), used.data()));
        used.resize(32 * n);
        return used;
    }
    const uint8_t* left() const { return left_; }
    const uint8_t* right() const { return right_; }
    size_t n_proofs() const { return n_proofs_; }   // as of the last read()
    size_t n_failed() const { return n_failed_; }

private:
    static void check_merge(size_t n, const Bytes& draws32) {
        if (n > H2V_ACC_MERGE_MAX) throw Failure(H2V_ERR_BAD_ARGUMENT, "at most H2V_ACC_MERGE_MAX sources");
        if (!draws32.empty() && draws32.size() != 32 * n) throw Failure(H2V_ERR_BAD_ARGUMENT, "one 32-byte draw per source");
    }
    h2v_accumulator* h_ = nullptr;
    bool all_ok_ = true;
    size_t n_proofs_ = 0, n_failed_ = 0;
    uint8_t left_[64] = {0}, right_[64] = {0};
};

// n x DualMSM::check, one verdict per Guard: SingleStrategy::process at the trait seam (kzg/strategy.rs:164-176), h2v_guards_check_each
inline std::vector<bool> check_guards(const Context& ctx, const std::vector<Guard>& guards) {
    const detail::FlatGuards f(guards);
    std::vector<int> ok(guards.size() ? guards.size() : 1, 0);
    check(h2v_guards_check_each(ctx.handle(), guards.size(), f.left_counts.data(), f.right_counts.data(), f.ls.data(), f.lb.data(), f.rs.data(), f.rb.data(), ok.data()));
    std::vector<bool> out;
    for (size_t i = 0; i < guards.size(); ++i) out.push_back(ok[i] != 0);
    return out;
}

// The pairing checks of ranges (first, count) of a batch's last finished launch on its resident scalars (h2v_batch_recheck): one verdict
// per range; lefts / rights (optional) receive the evaluated channels, 64 bytes per range.
struct RangeChecks { std::vector<bool> ok; Bytes lefts, rights; };
struct BatchRange { size_t batch, first, count; };
namespace detail {
// one batch (h2v_batch_recheck, every range's batch index 0) or several (h2v_batches_recheck)
inline RangeChecks recheck(h2v_batch* const* batches, size_t n_batches, bool several, const std::vector<BatchRange>& ranges) {
    std::vector<uint32_t> bor;
    std::vector<size_t> first, count;
    for (const auto& r : ranges) {
        if (r.batch >= n_batches) throw Failure(H2V_ERR_BAD_ARGUMENT, "batch index out of range");
        bor.push_back((uint32_t)r.batch); first.push_back(r.first); count.push_back(r.count);
    }
    const size_t k = ranges.size();
    std::vector<int> ok(k ? k : 1, 0);
    RangeChecks out;
    out.lefts.assign(64 * k, 0); out.rights.assign(64 * k, 0);
    if (several) check(h2v_batches_recheck(batches, n_batches, k, bor.data(), first.data(), count.data(), ok.data(), out.lefts.data(), out.rights.data()));
    else check(h2v_batch_recheck(batches[0], k, first.data(), count.data(), ok.data(), out.lefts.data(), out.rights.data()));
    for (size_t i = 0; i < k; ++i) out.ok.push_back(ok[i] != 0);
    return out;
}
}  // namespace detail
inline RangeChecks recheck(h2v_batch* b, const std::vector<std::pair<size_t, size_t>>& ranges) {
    std::vector<BatchRange> of_one;
    for (const auto& r : ranges) of_one.push_back({0, r.first, r.second});
    return detail::recheck(&b, 1, false, of_one);
}
// The same over ranges of several finished batches in one set of launches (h2v_batches_recheck): a range is (batch index, first, count);
// the batches must be on one device and over the same params
inline RangeChecks recheck(const std::vector<h2v_batch*>& batches, const std::vector<BatchRange>& ranges) {
    return detail::recheck(batches.data(), batches.size(), true, ranges);
}

// Groups of unequal size on a staged batch (h2v_batch_set_group_sizes): group g owns the next sizes[g] proofs of later uploads and the
// same slice of the draws.  1 to 512 sizes, each at least 1.
inline void set_group_sizes(h2v_batch* b, const std::vector<size_t>& sizes) {
    for (size_t v : sizes) if (!v) throw Failure(H2V_ERR_BAD_ARGUMENT, "a group of no proofs");
    if (sizes.empty() || sizes.size() > 512) throw Failure(H2V_ERR_BAD_ARGUMENT, "a launch holds 1 to 512 groups");
    check(h2v_batch_set_group_sizes(b, sizes.data(), sizes.size()));
}

// A staged batch's upload from device memory (h2v_batch_upload_device): n proof rows `proof_stride` bytes apart at d_proofs, the flat
// instance values at d_instances, n_tail draws at d_rand_tail (null: OS draws, the one form that waits for the stream).  Device work
// only, on the batch's stream; the verdict on the draws comes with h2v_batch_finish(_groups).  What the host can check is checked here
// first: 16-byte alignment, a stride that is a multiple of 16.
inline void upload_device(h2v_batch* b, size_t n, const void* d_proofs, size_t proof_stride, const void* d_instances, const std::vector<size_t>& col_lens,
                          const void* d_rand_tail = nullptr, size_t n_tail = 0) {
    if (n && !d_proofs) throw Failure(H2V_ERR_BAD_ARGUMENT, "upload_device: no proofs");
    if (proof_stride % 16) throw Failure(H2V_ERR_BAD_ARGUMENT, "upload_device: proof_stride must be a multiple of 16");
    for (const void* p : {d_proofs, d_instances, d_rand_tail})
        if (reinterpret_cast<uintptr_t>(p) % 16) throw Failure(H2V_ERR_BAD_ARGUMENT, "upload_device: a device pointer off a 16-byte boundary");
    if (d_rand_tail && n_tail < n) throw Failure(H2V_ERR_BAD_ARGUMENT, "upload_device: n_tail < n");
    check(h2v_batch_upload_device(b, n, d_proofs, proof_stride, d_instances, col_lens.size(), col_lens.data(), d_rand_tail, d_rand_tail ? n_tail : 0));
}

// A staged batch's finish into device memory (h2v_batch_finish_device): the results of the last launch written by kernels on the batch's
// stream into the caller's device arrays, nothing waited for.  Null = not wanted.  What the host can check is checked here first.
struct DeviceResults {
    void* status = nullptr;         // n int32
    void* group_ok = nullptr;       // groups int32
    void* left_xy = nullptr;        // groups x 64 bytes
    void* right_xy = nullptr;       // groups x 64 bytes
    void* group_failed = nullptr;   // groups uint32
    void* failed_index = nullptr;   // failed_cap uint32, ascending
    size_t failed_cap = 0;
    void* summary = nullptr;        // H2V_SUMMARY_WORDS uint32
};
inline void finish_device(h2v_batch* b, const DeviceResults& out) {
    for (const void* p : {out.status, out.group_ok, out.left_xy, out.right_xy, out.group_failed, out.failed_index, out.summary})
        if (reinterpret_cast<uintptr_t>(p) % 16) throw Failure(H2V_ERR_BAD_ARGUMENT, "finish_device: a device pointer off a 16-byte boundary");
    if (out.failed_index && !out.failed_cap) throw Failure(H2V_ERR_BAD_ARGUMENT, "finish_device: failed_cap is 0");
    check(h2v_batch_finish_device(b, out.status, out.group_ok, out.left_xy, out.right_xy, out.group_failed, out.failed_index, out.failed_index ? out.failed_cap : 0, out.summary));
}

// Many AccumulatorStrategy batches of their own sizes in few launches (h2v_verify_batches): every batch is a list of (instances, proof)
// in verify_proof order and none is empty; one instance shape for the whole call; rand32: one 32-byte draw per proof of the call, batch
// after batch, or empty = OS RNG.  -> per batch what its own AccumulatorStrategy::finalize() gives: verdict, statuses, the two channels.
struct BatchItem { Instances instances; Bytes proof; };
struct BatchResult { bool ok = false; std::vector<int> statuses; Bytes left, right; };
inline std::vector<BatchResult> verify_batches(const Context& ctx, const std::vector<std::vector<BatchItem>>& batches, const Bytes& rand32 = Bytes()) {
    detail::Marshalled m(true);
    m.add_key(ctx.handle());
    std::vector<size_t> sizes;
    for (const auto& batch : batches) {
        if (batch.empty()) throw Failure(H2V_ERR_BAD_ARGUMENT, "a batch of no proofs");
        sizes.push_back(batch.size());
        for (const BatchItem& it : batch) m.add(0, it.instances, it.proof);
    }
    const size_t n = m.n(), k = sizes.size();
    if (!m.uniform) throw Failure(H2V_ERR_BAD_ARGUMENT, "verify_batches takes one instance shape per call");
    if (!rand32.empty() && rand32.size() != 32 * n) throw Failure(H2V_ERR_BAD_ARGUMENT, "one 32-byte draw per proof");
    std::vector<int> st(n ? n : 1, 0), ok(k ? k : 1, 0);
    Bytes left(64 * (k ? k : 1), 0), right(64 * (k ? k : 1), 0);
    sizes.resize(k ? k : 1, 0);
    check(h2v_verify_batches(ctx.handle(), k, sizes.data(), m.proofs.data(), m.lens.data(), m.insts.data(), m.ncols[0], m.shape0(), rand32.empty() ? nullptr : rand32.data(),
                             st.data(), ok.data(), left.data(), right.data()));
    std::vector<BatchResult> out(k);
    for (size_t g = 0, at = 0; g < k; at += sizes[g], ++g) {
        out[g].ok = ok[g] != 0;
        out[g].statuses.assign(st.begin() + at, st.begin() + at + sizes[g]);
        out[g].left.assign(left.begin() + 64 * g, left.begin() + 64 * g + 64);
        out[g].right.assign(right.begin() + 64 * g, right.begin() + 64 * g + 64);
    }
    return out;
}

// kzg/strategy.rs:143-181: one pairing per proof, checked inside verify_proof
class SingleStrategy {
public:
    explicit SingleStrategy(const ParamsKZG& p, int device = 0, MultiOpen mo = MultiOpen::SHPLONK, TranscriptKind tr = TranscriptKind::Blake2b,
                            int circuit_instances = 1)
        : params_(p), device_(device), mo_(mo), tr_(tr), ci_(circuit_instances) {}
    Error verify(const VerifyingKey& vk, const Instances& inst, const Bytes& proof) const {
        Context ctx(params_, vk, device_, mo_, tr_, ci_);
        detail::Marshalled m;
        m.add_key(ctx.handle());
        if (inst.size() != m.ncols[0]) return Error::InvalidInstances;   // lib.rs:51-55
        m.add(0, inst, proof);
        int st = 0;
        check(h2v_verify_each(ctx.handle(), 1, m.proofs.data(), m.lens.data(), m.insts.data(), m.ncols[0], m.shape0(), &st));
        return (Error)st;
    }

private:
    ParamsKZG params_; int device_; MultiOpen mo_; TranscriptKind tr_; int ci_;
};

// lib.rs:33-49.  SingleStrategy: returns the proof's plonk::Error (Ok = accepted).
inline Error verify_proof(const ParamsKZG&, const VerifyingKey& vk, const SingleStrategy& s, const Instances& inst, const Bytes& proof) { return s.verify(vk, inst, proof); }
// AccumulatorStrategy: Output = the strategy (the proof is queued; errors surface in statuses() after finalize())
inline AccumulatorStrategy& verify_proof(const ParamsKZG&, const VerifyingKey& vk, AccumulatorStrategy& s, Instances inst, Bytes proof) {
    s.push(vk, std::move(inst), std::move(proof));
    return s;
}

}  // namespace halo2_verifier
namespace h2v = halo2_verifier;   // the short name: h2v::Msm, h2v::DualMsm, ...
