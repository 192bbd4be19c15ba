// The per-proof kernels (halo2_verifier_amd/csrc/verify_kernels.hip) stage by stage, on inputs programmed by
// tests/test_gpu_verify_units.py and compared there with tests/verify_reference.py, and the batch multipliers' kernels on raw draws
// chosen by tests/test_gpu_multipliers.py and tests/test_gpu_ragged_multipliers.py.  Built with the library's flags by
// halo2_verifier_amd/csrc/Makefile (build/verify_units); the prelude is tests/cpp/units.h.
//
//   verify_units decompress  IN OUT   decompress_begin / _range (in the pieces the input gives) / _finish: k_decompress, k_check_scalars
//   verify_units stream      IN OUT   transcript_stage_enqueue: k_stream_build, then k_transcript or k_transcript_keccak
//   verify_units insteval    IN OUT   instance_eval_enqueue: k_instance_eval
//   verify_units frvm        IN OUT   frvm_enqueue: k_frvm / k_frvm2 on a programmed VmInstr program
//   verify_units fold        IN OUT   fold_shared_enqueue (k_fold_shared, equal or unequal groups) and fold_shared_ranges_enqueue (k_fold_ranges)
//   verify_units multipliers IN OUT   multipliers_enqueue over groups of equal size (a shard's longer tail included)
//   verify_units gather      IN OUT   gather_multipliers_enqueue: k_gather_multipliers (a file of whole words)
//   verify_units ragged      IN OUT   multipliers_enqueue: the segmented suffix scan k_seg_mult_tiles, k_seg_mult_scan_tiles,
//                                     k_seg_mult_apply over groups of unequal size
// IN is little-endian: a word n_jobs, then per job the words and byte blocks its reader below takes, in that order.  OUT is the jobs'
// results one after another (the layouts are at the writers).  Field elements cross the file boundary as 32 canonical little-endian
// bytes.  The Plan and PlanDevice a launcher wants are filled by hand from the input: no compile_plan, no PlanDevice::upload.
// Every count, offset and index that reaches a kernel is checked on the host against the buffer sizes first ("bad input", status 2):
// no input can make a kernel leave its buffers.  Every output buffer lies between guard bands that are checked after the launch.
#include "../../halo2_verifier_amd/csrc/verify_kernels.hip"
#include "units.h"

#define FILL 0x11   // what the per-proof stages' output buffers hold before a launch: limbs 0x11111111 are normalised, so an unwritten Fr still converts

template <class T> static void upload(DevBuf<T>& d, const T* h, size_t n) {
    RC(d.alloc(n));
    if (n) CK(hipMemcpy((void*)d.p, (const void*)h, n * sizeof(T), hipMemcpyHostToDevice));
}
// a source buffer of the stream builder: 32 bytes of slack on both sides, filled with 0xA5 (the unaligned 8-byte loads of the fast
// path stay inside the allocation for any table; a byte wrongly taken from the slack shows in the result)
struct Slack {
    DevBuf<uint8_t> buf;
    const uint8_t* p = nullptr;
    void set(const uint8_t* h, size_t n) {
        RC(buf.alloc(n + 64));
        CK(hipMemset(buf.p, 0xA5, n + 64));
        if (n) CK(hipMemcpy(buf.p + 32, h, n, hipMemcpyHostToDevice));
        p = buf.p + 32;
    }
};
static void out_fields(Out& out, const Guarded<Fr>& d, const char* what) { for (const Fr& v : d.host(what)) out.field(v); }

#define MAX_PROOFS 4096u
#define MAX_ITEMS 1024u
#define MAX_LEN (1u << 20)

// ---- decompress
// job: n, np, n_main, ns, ninst, proof_len, n_pieces, n_pieces + 1 piece bounds (0 = b[0] < .. < b[n_pieces] = n), point_offsets[np], scalar_offsets[ns],
//      proofs [n][proof_len], inst [n][ninst][32]
// out: per (proof, point): x, y of pts, x, y of phi (32 bytes each), a word (1 = pts holds the identity), the 32 ycanon bytes; then n raw status words
static void run_decompress(In& in, Out& out) {
    const uint32_t n = in.word(), np = in.word(), n_main = in.word(), ns = in.word(), ninst = in.word(), proof_len = in.word(), n_pieces = in.word();
    REQUIRE(n >= 1 && n <= MAX_PROOFS && np >= 1 && np <= MAX_ITEMS && ns <= MAX_ITEMS && ninst <= MAX_ITEMS, "counts");
    REQUIRE(n_main <= np && proof_len >= 32 && proof_len <= MAX_LEN && proof_len % 32 == 0, "proof length");
    REQUIRE(n_pieces >= 1 && n_pieces <= n, "pieces");
    const std::vector<uint32_t> cut = in.words(n_pieces + 1);
    REQUIRE(cut[0] == 0 && cut[n_pieces] == n, "pieces must cover [0, n)");
    for (uint32_t i = 0; i < n_pieces; ++i) REQUIRE(cut[i] < cut[i + 1], "pieces must ascend");
    PlanDevice pd;
    Plan& pl = pd.host;
    pl.n_points = np; pl.n_main_points = n_main; pl.n_scalars = ns; pl.n_instance_values = ninst; pl.proof_len = proof_len;
    pl.point_offsets = in.words(np); pl.scalar_offsets = in.words(ns);
    for (uint32_t o : pl.point_offsets) REQUIRE(o % 32 == 0 && o <= proof_len - 32, "point offset");      // (two 16-byte loads per point)
    for (uint32_t o : pl.scalar_offsets) REQUIRE(o % 32 == 0 && o <= proof_len - 32, "scalar offset");
    upload(pd.point_offsets, pl.point_offsets.data(), np);
    upload(pd.scalar_offsets, pl.scalar_offsets.data(), ns);
    DevBuf<uint8_t> proofs, inst;
    upload(proofs, in.bytes((size_t)n * proof_len), (size_t)n * proof_len);
    upload(inst, in.bytes((size_t)n * ninst * 32), (size_t)n * ninst * 32);
    const size_t tp = (size_t)n * np;
    Guarded<G1A> pts(tp, FILL), phi(tp, FILL); Guarded<uint8_t> ycanon(tp * 32, FILL); Guarded<int> status(n, FILL);   // (the status words too: the begin step resets them)
    StageArgs g{n, &pl, &pd, proofs.p, inst.p, pts.p, phi.p, ycanon.p, status.p, nullptr, 0, nullptr};
    RC(decompress_begin_enqueue(0, g));
    for (uint32_t i = 0; i < n_pieces; ++i) RC(decompress_range_enqueue(0, g, cut[i], cut[i + 1]));
    RC(decompress_finish_enqueue(0, g));
    CK(hipDeviceSynchronize());
    const std::vector<G1A> hp = pts.host("pts"), hf = phi.host("phi");
    const std::vector<uint8_t> hy = ycanon.host("ycanon");
    for (size_t i = 0; i < tp; ++i) {
        out.field(hp[i].x); out.field(hp[i].y); out.field(hf[i].x); out.field(hf[i].y);
        out.word(hp[i].is_identity() ? 1u : 0u);
        out.raw(&hy[32 * i], 32);
    }
    status.collect(out, "status");
}

// ---- stream
// job: n, transcript (0 Blake2b, 1 Keccak-256), proof_len, np, ninst, stream_len, n_squeeze, stream_len x (kind | value << 8, offset), squeeze_at[n_squeeze],
//      proofs [n][proof_len], ycanon [n][np][32], inst [n][ninst][32]
// out: the launcher's return code, stream_words, the words buffer [n][stream_words] (8 bytes each), the challenges [n_squeeze][n]
//      (both as the launcher left them: FILL where nothing was written)
static void run_stream(In& in, Out& out) {
    const uint32_t n = in.word(), kind = in.word(), proof_len = in.word(), np = in.word(), ninst = in.word(), stream_len = in.word(), nsq = in.word();
    REQUIRE(n >= 1 && n <= MAX_PROOFS && kind <= 1 && proof_len <= MAX_LEN && np <= MAX_ITEMS && ninst <= MAX_ITEMS, "counts");
    REQUIRE(stream_len >= 1 && stream_len <= (1u << 16) && nsq >= 1 && nsq <= 4096, "stream length");
    PlanDevice pd;
    Plan& pl = pd.host;
    pl.n_points = np; pl.n_instance_values = ninst; pl.proof_len = proof_len;
    pl.opts.transcript = kind ? H2V_TRANSCRIPT_KECCAK256 : 0;
    pl.stream.resize(stream_len);
    for (uint32_t i = 0; i < stream_len; ++i) {
        const uint32_t kv = in.word(), off = in.word(), k = kv & 0xffu;
        REQUIRE(kv <= 0xffffu && k <= TranscriptSrc::INSTANCE, "stream entry kind");
        const size_t per = k == TranscriptSrc::CONST ? 1 : (k == TranscriptSrc::YCOORD ? (size_t)np * 32 : (k == TranscriptSrc::INSTANCE ? (size_t)ninst * 32 : (size_t)proof_len));
        REQUIRE(off < per, "stream entry offset");   // a byte of the proof's own record
        pl.stream[i].kind = (uint8_t)k; pl.stream[i].value = (uint8_t)(kv >> 8); pl.stream[i].offset = off;
    }
    pl.squeeze_at = in.words(nsq);
    for (uint32_t q = 0; q < nsq; ++q) REQUIRE(pl.squeeze_at[q] >= 1 && pl.squeeze_at[q] <= stream_len && (q == 0 || pl.squeeze_at[q] >= pl.squeeze_at[q - 1]), "squeeze position");
    upload(pd.stream, pl.stream.data(), stream_len);
    upload(pd.squeeze_at, pl.squeeze_at.data(), nsq);
    Slack proofs, ycanon, inst;
    proofs.set(in.bytes((size_t)n * proof_len), (size_t)n * proof_len);
    ycanon.set(in.bytes((size_t)n * np * 32), (size_t)n * np * 32);
    inst.set(in.bytes((size_t)n * ninst * 32), (size_t)n * ninst * 32);
    const uint32_t sw = stream_words_for(stream_len, pl.opts.transcript);
    REQUIRE((size_t)sw * 8 > stream_len, "stream words");   // every squeeze's last block, and a prefetched block behind it, lie inside
    Guarded<unsigned long long> words((size_t)n * sw, FILL); Guarded<Fr> chal((size_t)nsq * n, FILL);
    StageArgs g{n, &pl, &pd, proofs.p, inst.p, nullptr, nullptr, const_cast<uint8_t*>(ycanon.p), nullptr, words.p, sw, chal.p};
    const int rc = transcript_stage_enqueue(0, g);
    CK(hipDeviceSynchronize());
    out.word((uint32_t)rc); out.word(sw);
    words.collect(out, "stream words");
    out_fields(out, chal, "challenges");
}

// ---- insteval
// job: n, k, ninst, base, len, rot (two's complement), x_chal, n_chal, omega (the 2^k-th root of unity), inst [n][ninst][32], chal [n_chal][n]
// out: out[p] (n field elements), n raw status words
static void run_insteval(In& in, Out& out) {
    const uint32_t n = in.word(), k = in.word(), ninst = in.word(), base = in.word(), len = in.word();
    const int32_t rot = (int32_t)in.word();
    const uint32_t x_chal = in.word(), n_chal = in.word();
    REQUIRE(n >= 1 && n <= 64 && k >= 1 && k <= 28 && ninst <= (1u << 16) && n_chal <= 64, "counts");
    REQUIRE(base <= ninst && len <= ninst - base && x_chal < n_chal && rot >= -1024 && rot <= 1024, "column");
    const Fr omega = in.field<Fr>();
    DevBuf<uint8_t> inst; DevBuf<Fr> chal; DevBuf<int> status;
    upload(inst, in.bytes((size_t)n * ninst * 32), (size_t)n * ninst * 32);
    const std::vector<Fr> hc = in.fields<Fr>((size_t)n_chal * n);
    upload(chal, hc.data(), hc.size());
    Guarded<Fr> res(n, FILL);
    RC(status.alloc(n));
    CK(hipMemset(status.p, 0, sizeof(int) * n));
    Fr step = omega;
    for (int i = 0; i < 8; ++i) step = step.sqr();   // omega^256: a thread's stride through the column
    const Fr w_start = rot >= 0 ? omega.inv().pow_u32((uint32_t)rot) : omega.pow_u32((uint32_t)-rot);   // omega^(-rot)
    InstEvalArgs a{inst.p, ninst, chal.p, x_chal, n, k, base, len, w_start, omega, step, step.inv(), Fr::from_u32(1u << k).inv(), res.p, status.p};
    RC(instance_eval_enqueue(0, a));
    CK(hipDeviceSynchronize());
    out_fields(out, res, "out");
    append(out, status.p, n);
}

// ---- frvm
struct VmBounds { uint32_t n_slots, n_consts, ns, ninst, n_chal, n_insteval, np, n_guard, n_shared; };
// every index of a stream lies inside its buffer; returns the stream's number of barriers
static uint32_t check_code(const std::vector<VmInstr>& code, const VmBounds& z) {
    uint32_t barriers = 0;
    auto slot = [&](uint32_t s) { REQUIRE(s < z.n_slots, "slot"); };
    auto opnd = [&](uint32_t x) { if (x & VM_CONST_OPERAND) REQUIRE((x & ~VM_CONST_OPERAND) < z.n_consts, "constant operand"); else slot(x); };
    for (const VmInstr& in : code) {
        switch (in.op) {
            case OP_BARRIER: ++barriers; break;
            case OP_CONST: slot(in.d); REQUIRE(in.a < z.n_consts, "constant"); break;
            case OP_MUL: case OP_ADD: case OP_SUB: slot(in.d); opnd(in.a); opnd(in.b); break;
            case OP_NEG: case OP_INV: case OP_POW: slot(in.d); slot(in.a); break;
            case OP_SQRN: slot(in.d); slot(in.a); REQUIRE(in.b <= 64, "squarings"); break;
            case OP_LOAD_SCALAR: slot(in.d); REQUIRE(in.a < z.ns, "scalar"); break;
            case OP_LOAD_INST: slot(in.d); REQUIRE(in.a < z.ninst, "instance value"); break;
            case OP_LOAD_CHAL: slot(in.d); REQUIRE(in.a < z.n_chal, "challenge"); break;
            case OP_LOAD_INSTEVAL: slot(in.d); REQUIRE(in.a < z.n_insteval, "insteval"); break;
            case OP_LOAD_MULT: slot(in.d); break;
            case OP_STORE_MSM: case OP_STORE_LEFT: slot(in.a); REQUIRE(in.b < z.np, "point slot"); break;
            case OP_STORE_GUARD: slot(in.a); REQUIRE(in.b < z.n_guard, "guard term"); break;
            case OP_STORE_SHARED: slot(in.a); REQUIRE(in.b < z.n_shared, "shared row"); break;
            default: REQUIRE(false, "opcode");
        }
    }
    return barriers;
}
static std::vector<VmInstr> read_code(In& in, uint32_t n_code) {
    REQUIRE(n_code <= 4096, "program length");
    std::vector<VmInstr> c(n_code);
    for (VmInstr& i : c) { i.op = in.word(); i.d = in.word(); i.a = in.word(); i.b = in.word(); }
    return c;
}
// job: n, n_code, n_slots, n_consts, ns, ninst, n_chal, n_insteval, np, n_guard, n_shared, proof_len, force_streams, force_lds_kb,
//      then for K = 2, 3, 4: n_slots_k, n_code_k[0..4) (all zero: no K-stream form);
//      code, the K forms' streams in that order, consts, scalar_offsets[ns], proofs [n][proof_len], inst [n][ninst][32], chal [n_chal][n],
//      insteval [n_insteval][n], mult [n], n status words to start from
// out: msm_scal [n][np][8], left_scal [n][np][8], guard_scal [n][n_guard][8] (raw words), shared [n_shared][n] (canonical), n raw status words
static void run_frvm(In& in, Out& out) {
    const uint32_t n = in.word(), n_code = in.word(), n_slots = in.word(), n_consts = in.word(), ns = in.word(), ninst = in.word(), n_chal = in.word(), n_insteval = in.word(),
                   np = in.word(), n_guard = in.word(), n_shared = in.word(), proof_len = in.word();
    const int force_streams = (int)in.word(), force_lds_kb = (int)in.word();
    REQUIRE(n >= 1 && n <= MAX_PROOFS && n_code >= 1 && n_slots >= 1 && n_slots <= 1024 && n_consts <= MAX_ITEMS && ns <= MAX_ITEMS && ninst <= MAX_ITEMS, "counts");
    REQUIRE(n_chal <= MAX_ITEMS && n_insteval <= MAX_ITEMS && np <= MAX_ITEMS && n_guard <= MAX_ITEMS && n_shared <= MAX_ITEMS, "counts");
    REQUIRE(proof_len <= MAX_LEN && proof_len % 32 == 0 && force_streams >= 0 && force_streams <= FRVM_MAX_STREAMS && force_lds_kb >= 0 && force_lds_kb <= 156, "sizes");
    uint32_t n_slots_k[3], n_code_k[3][FRVM_MAX_STREAMS], max_slots = n_slots;
    for (int k = 0; k < 3; ++k) {
        n_slots_k[k] = in.word();
        for (int w = 0; w < FRVM_MAX_STREAMS; ++w) n_code_k[k][w] = in.word();
        REQUIRE(n_slots_k[k] <= 1024, "slots of a K-stream form");
        if (n_slots_k[k] > max_slots) max_slots = n_slots_k[k];
    }
    VmBounds z{n_slots, n_consts, ns, ninst, n_chal, n_insteval, np, n_guard, n_shared};
    const std::vector<VmInstr> code = read_code(in, n_code);
    check_code(code, z);
    std::vector<VmInstr> code_k[3][FRVM_MAX_STREAMS];
    for (int k = 0; k < 3; ++k) {
        const bool have = n_code_k[k][0] != 0;
        uint32_t barriers = 0;
        for (int w = 0; w < FRVM_MAX_STREAMS; ++w) {
            // a K-stream form has K non-empty streams that meet at the same number of barriers (a workgroup barrier one wave skips hangs the others)
            REQUIRE(have && w < k + 2 ? n_code_k[k][w] >= 1 : n_code_k[k][w] == 0, "streams of a K-stream form");
            code_k[k][w] = read_code(in, n_code_k[k][w]);
            VmBounds zk = z; zk.n_slots = n_slots_k[k];
            const uint32_t b = check_code(code_k[k][w], zk);
            if (w == 0) barriers = b;
            else if (n_code_k[k][w]) REQUIRE(b == barriers, "barriers of a K-stream form");
        }
    }
    const std::vector<Fr> consts = in.fields<Fr>(n_consts);
    const std::vector<uint32_t> soff = in.words(ns);
    for (uint32_t o : soff) REQUIRE(proof_len >= 32 && o % 32 == 0 && o <= proof_len - 32, "scalar offset");   // (two 16-byte loads per scalar)
    DevBuf<VmInstr> d_code, d_code_k[3][FRVM_MAX_STREAMS]; DevBuf<Fr> d_consts, chal, insteval, mult; DevBuf<uint32_t> d_soff;
    DevBuf<uint8_t> proofs, inst; DevBuf<int> status;
    upload(d_code, code.data(), code.size());
    upload(d_consts, consts.data(), consts.size());
    upload(d_soff, soff.data(), soff.size());
    upload(proofs, in.bytes((size_t)n * proof_len), (size_t)n * proof_len);
    upload(inst, in.bytes((size_t)n * ninst * 32), (size_t)n * ninst * 32);
    { const std::vector<Fr> h = in.fields<Fr>((size_t)n_chal * n); upload(chal, h.data(), h.size()); }
    { const std::vector<Fr> h = in.fields<Fr>((size_t)n_insteval * n); upload(insteval, h.data(), h.size()); }
    { const std::vector<Fr> h = in.fields<Fr>(n); upload(mult, h.data(), h.size()); }
    { const std::vector<uint32_t> h = in.words(n); upload(status, (const int*)h.data(), h.size()); }
    Guarded<Fr> slots((size_t)max_slots * n, FILL), shared((size_t)n_shared * n, FILL);
    Guarded<uint32_t> msm((size_t)n * np * 8, FILL), left((size_t)n * np * 8, FILL), guard((size_t)n * n_guard * 8, FILL);
    FrvmArgs a;
    a.code = d_code.p; a.n_code = n_code; a.consts = d_consts.p; a.slots = slots.p; a.n = n;
    a.proofs = proofs.p; a.proof_len = proof_len; a.scalar_offsets = d_soff.p; a.inst = inst.p; a.ninst = ninst;
    a.chal = chal.p; a.mult = mult.p; a.status = status.p; a.msm_scal = msm.p; a.np = np; a.shared = shared.p; a.left_scal = left.p;
    a.insteval = insteval.p; a.guard_scal = guard.p; a.n_guard = n_guard;
    for (int k = 0; k < 3; ++k) {
        a.n_slots_k[k] = n_slots_k[k];
        for (int w = 0; w < FRVM_MAX_STREAMS; ++w) {
            if (!n_code_k[k][w]) continue;
            upload(d_code_k[k][w], code_k[k][w].data(), code_k[k][w].size());
            a.code_k[k][w] = d_code_k[k][w].p; a.n_code_k[k][w] = n_code_k[k][w];
        }
    }
    a.force_streams = force_streams; a.force_lds_kb = force_lds_kb;
    RC(frvm_enqueue(0, a, n_slots));
    CK(hipDeviceSynchronize());
    slots.host("slots");
    msm.collect(out, "msm_scal"); left.collect(out, "left_scal"); guard.collect(out, "guard_scal");
    out_fields(out, shared, "shared");
    append(out, status.p, n);
}

// ---- fold
// job, form 0 (fold_shared_enqueue): 0, n, np, n_shared, groups, with_off, (with_off) groups + 1 offsets from 0 to n, shared [n_shared][n];
//      without offsets the groups are equal
//      out: msm_scal, all (n np + groups n_shared) rows of 8 raw words (FILL where nothing was written)
// job, form 1 (fold_shared_ranges_enqueue): 1, n_batches, per batch (n, n_shared, shared [n_shared][n]), n_ranges, per range (batch, first, count, out),
//      max_shared, out_rows
//      out: all out_rows rows of 8 raw words (FILL where nothing was written)
static void run_fold(In& in, Out& out) {
    const uint32_t form = in.word();
    REQUIRE(form <= 1, "form");
    if (form == 0) {
        const uint32_t n = in.word(), np = in.word(), n_shared = in.word(), groups = in.word(), with_off = in.word();
        REQUIRE(n >= 1 && n <= (1u << 16) && np <= 16 && n_shared >= 1 && n_shared <= MAX_ITEMS && groups >= 1 && groups <= n && with_off <= 1, "counts");
        DevBuf<uint32_t> d_off;
        if (with_off) {
            const std::vector<uint32_t> off = in.words(groups + 1);
            REQUIRE(off[0] == 0 && off[groups] == n, "offsets from 0 to n");
            for (uint32_t g = 0; g < groups; ++g) REQUIRE(off[g] < off[g + 1], "a group of no proofs");
            upload(d_off, off.data(), off.size());
        } else REQUIRE(n % groups == 0, "equal groups divide n");
        const GroupShape shape = with_off ? GroupShape::unequal(groups, n, d_off.p) : GroupShape::equal(groups, n, n);
        DevBuf<Fr> shared;
        { const std::vector<Fr> h = in.fields<Fr>((size_t)n_shared * n); upload(shared, h.data(), h.size()); }
        const size_t rows = (size_t)n * np + (size_t)groups * n_shared;
        Guarded<uint32_t> msm(rows * 8, FILL);
        RC(fold_shared_enqueue(0, shape, shared.p, n, np, n_shared, msm.p));
        CK(hipDeviceSynchronize());
        msm.collect(out, "msm_scal");
        return;
    }
    const uint32_t n_batches = in.word();
    REQUIRE(n_batches >= 1 && n_batches <= 16, "batches");
    std::vector<DevBuf<Fr>> shared(n_batches);
    std::vector<uint32_t> bn(n_batches), bs(n_batches);
    for (uint32_t b = 0; b < n_batches; ++b) {
        bn[b] = in.word(); bs[b] = in.word();
        REQUIRE(bn[b] >= 1 && bn[b] <= (1u << 16) && bs[b] >= 1 && bs[b] <= MAX_ITEMS, "batch");
        const std::vector<Fr> h = in.fields<Fr>((size_t)bs[b] * bn[b]);
        upload(shared[b], h.data(), h.size());
    }
    const uint32_t n_ranges = in.word();
    REQUIRE(n_ranges >= 1 && n_ranges <= 4096, "ranges");
    std::vector<FoldRange> rg(n_ranges);
    std::vector<uint32_t> rb(n_ranges);
    for (uint32_t r = 0; r < n_ranges; ++r) {
        rb[r] = in.word();
        REQUIRE(rb[r] < n_batches, "range's batch");
        rg[r].shared = shared[rb[r]].p; rg[r].n = bn[rb[r]]; rg[r].n_shared = bs[rb[r]];
        rg[r].first = in.word(); rg[r].count = in.word(); rg[r].out = in.word(); rg[r].pad = 0;
        REQUIRE(rg[r].first <= rg[r].n && rg[r].count <= rg[r].n - rg[r].first, "range");
    }
    const uint32_t max_shared = in.word(), out_rows = in.word();
    REQUIRE(max_shared >= 1 && max_shared <= MAX_ITEMS && out_rows <= (1u << 20), "rows");
    for (uint32_t r = 0; r < n_ranges; ++r) REQUIRE(rg[r].n_shared <= max_shared && rg[r].out <= out_rows && rg[r].n_shared <= out_rows - rg[r].out, "range's rows");
    DevBuf<FoldRange> d_rg;
    upload(d_rg, rg.data(), rg.size());
    Guarded<uint32_t> rows((size_t)out_rows * 8, FILL);
    RC(fold_shared_ranges_enqueue(0, d_rg.p, n_ranges, max_shared, rows.p));
    CK(hipDeviceSynchronize());
    rows.collect(out, "rows");
}

// ---- multipliers
// job: groups, n_tail per group, n per group, then groups * n_tail draws of 32 little-endian bytes
// out: groups * n multipliers of 32 canonical bytes: mult[g][p] = prod_{j > p} draw[g][j] mod r
static void run_multipliers(In& in, Out& out) {
    const uint32_t G = in.word(), nt = in.word(), n = in.word();
    REQUIRE(G && nt && n && n <= nt && G <= 1024 && nt <= (1u << 22) && (size_t)G * nt <= (1u << 22), "bad job");
    const size_t draws = (size_t)G * nt, mults = (size_t)G * n;
    REQUIRE(draws <= in.left() / 32, "input too short");
    uint8_t* d_tail = to_device(in.bytes(32 * draws), 32 * draws);
    const GroupShape shape{G, n, nt, nullptr};
    Guarded<Fr> mult(mults), scratch(multipliers_scratch(shape));
    RC(multipliers_enqueue(0, shape, d_tail, nullptr, mult.p, scratch.p));
    CK(hipDeviceSynchronize());
    scratch.host("scratch");
    out_fields(out, mult, "multipliers");
    CK(hipFree(d_tail));
}

// ---- gather
// job: n_src, n, n_src source elements (9 raw limbs each, as they lie in memory), n indices
// out: n elements (9 limbs each): out[i] = src[idx[i]]
static void run_gather(In& in, Out& out) {
    static_assert(sizeof(Fr) == 36, "nine limbs");
    const uint32_t n_src = in.word(), n = in.word();
    REQUIRE(n_src >= 1 && n_src <= (1u << 16) && n <= (1u << 16), "bad gather job");
    std::vector<Fr> src(n_src);
    in.take(src.data(), n_src);
    const std::vector<uint32_t> idx = in.words(n);
    for (uint32_t i : idx) REQUIRE(i < n_src, "index outside the source");
    Fr* d_src = to_device(src.data(), n_src);
    uint32_t* d_idx = to_device(idx.data(), n);
    Guarded<Fr> res(n);
    RC(gather_multipliers_enqueue(0, d_src, d_idx, n, res.p));
    CK(hipDeviceSynchronize());
    res.collect(out, "gathered elements");
    CK(hipFree(d_src)); CK(hipFree(d_idx));
}

// ---- ragged
// job: n_groups, the n_groups sizes, then sum(sizes) draws of 32 little-endian bytes
// out: sum(sizes) multipliers of 32 canonical bytes: mult[p] = the product of the draws behind p in p's group
// The offsets and the "last proof of its group" bytes are built here as the library's host side builds them; the scratch lies between bands too.
static void run_ragged(In& in, Out& out) {
    const uint32_t G = in.word();
    REQUIRE(G >= 1 && G <= (1u << 20), "bad group count");
    std::vector<uint8_t> last;
    std::vector<uint32_t> off(1, 0);
    for (uint32_t g = 0; g < G; ++g) {
        const uint32_t sz = in.word();
        REQUIRE(sz >= 1 && sz <= (1u << 22) && last.size() + sz <= (1u << 22), "bad group size");
        last.resize(last.size() + sz, 0); last.back() = 1;
        off.push_back((uint32_t)last.size());
    }
    const size_t n = last.size();
    REQUIRE(n <= in.left() / 32, "input too short");
    uint8_t* d_tail = to_device(in.bytes(32 * n), 32 * n);
    uint8_t* d_last = to_device(last.data(), n);
    uint32_t* d_off = to_device(off.data(), off.size());
    const GroupShape shape = GroupShape::unequal(G, (uint32_t)n, d_off);
    Guarded<Fr> mult(n), scratch(multipliers_scratch(shape));
    RC(multipliers_enqueue(0, shape, d_tail, d_last, mult.p, scratch.p));
    CK(hipDeviceSynchronize());
    scratch.host("scratch");
    out_fields(out, mult, "multipliers");
    CK(hipFree(d_tail)); CK(hipFree(d_last)); CK(hipFree(d_off));
}

static const Mode MODES[] = {{"decompress", each_job<run_decompress, 4096>, false, false}, {"stream", each_job<run_stream, 4096>, false, false},
                             {"insteval", each_job<run_insteval, 4096>, false, false}, {"frvm", each_job<run_frvm, 4096>, false, false},
                             {"fold", each_job<run_fold, 4096>, false, false}, {"multipliers", each_job<run_multipliers, 64>, false, false},
                             {"gather", each_job<run_gather, 64>, true, false}, {"ragged", each_job<run_ragged, 64>, false, false}};
int main(int argc, char** argv) { return units_main("verify_units", MODES, argc, argv); }
