// The MSM kernels (halo2_verifier_amd/csrc/msm.hip) and the group law they run (curve.hip.h) stage by stage, on inputs chosen by
// tests/test_gpu_msm_units.py.  Built with the library's flags by halo2_verifier_amd/csrc/Makefile (build/msm_units).
//
//   msm_units law    IN OUT   one quad of lanes per case: g1_dbl_inl, g1_dbl_quad, g1_madd_fast, g1_add_fast, g1_add_inl,
//                             g1_add_affine_inl, g1_phi, msm_entry_apply, msm_horner_quad on raw 29-bit limbs (the Python side picks
//                             every representative); then one chain of operations, each fed from the previous result
//   msm_units digits IN OUT   per job one problem under a given plan (c, windows): msm_glv_prep's digit table, then the count, scan
//                             and scatter passes of the global sort: counts (with the control words), offsets, list
//   msm_units msm    IN OUT   per job one launch of msm_enqueue_multi on a workspace of its own, under a given h2v_tuning: every
//                             problem's result, the plan, the control words, the chunk length
//   msm_units scale  IN OUT   k_accumulator_scale through accumulator_scale_many_enqueue: the records as they are in memory
// Files are little-endian uint32 words; the layouts are in the readers below.  Scalars are 8 raw words, affine bases 64 canonical
// bytes (x | y, all zero = the identity) that the host converts with Fq::from_bytes; Jacobian points and every result are raw limbs.
// Every count and index that reaches a kernel is checked on the host first.  The results a mode allocates itself (not those of an
// MsmWorkspace) are preset to 0xff and lie between guard bands that are checked after the kernels.  The prelude is tests/cpp/units.h.
#include "../../halo2_verifier_amd/csrc/msm.hip"
#include "units.h"

// n affine bases of 64 canonical bytes each
static std::vector<G1A> bases_from_bytes(In& in, size_t n) {
    std::vector<G1A> v(n);
    REQUIRE(n <= in.left() / 64, "input too short");
    const uint8_t* b = in.bytes(64 * n);
    for (size_t i = 0; i < n; ++i) REQUIRE(Fq::from_bytes(b + 64 * i, v[i].x) && Fq::from_bytes(b + 64 * i + 32, v[i].y), "base coordinate not canonical");
    return v;
}

// ---- law
enum { LAW_DBL = 0, LAW_DBL_QUAD, LAW_MADD_FAST, LAW_ADD_FAST, LAW_ADD, LAW_ADD_AFFINE, LAW_PHI, LAW_ENTRY_APPLY, LAW_HORNER, LAW_COUNT };
struct LawCase { uint32_t op, a0, a1, a2; G1J A, B; };      // B as an affine point: (B.X, B.Y)
struct LawOut { uint32_t flag, pad[3]; G1J lane[4]; };      // flag: what a fast form returned; lane r: the value lane r of the quad ended with
static_assert(sizeof(LawCase) == 4 * 58 && sizeof(LawOut) == 4 * 112, "word records");
__global__ void __launch_bounds__(64) k_units_law(const LawCase* __restrict__ cases, uint32_t n, const G1JSlot* __restrict__ pool, LawOut* __restrict__ out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, i = t >> 2, r = t & 3u;
    if (i >= n) return;   // whole quads
    const LawCase c = cases[i];
    G1J res = c.A;
    G1A b; b.x = c.B.X; b.y = c.B.Y;
    uint32_t flag = 0;
    switch (c.op) {   // uniform inside a quad
    case LAW_DBL: res = g1_dbl_inl(c.A); break;
    case LAW_DBL_QUAD: g1_dbl_quad(res, r); break;
    case LAW_MADD_FAST: flag = g1_madd_fast(res, b) ? 1u : 0u; break;
    case LAW_ADD_FAST: flag = g1_add_fast(res, c.B) ? 1u : 0u; break;
    case LAW_ADD: res = g1_add_inl(c.A, c.B); break;
    case LAW_ADD_AFFINE: res = g1_add_affine_inl(c.A, b); break;
    case LAW_PHI: b = g1_phi(b); res.X = b.x; res.Y = b.y; res.Z = Fq::zero(); break;
    case LAW_ENTRY_APPLY: b = msm_entry_apply(b, c.a0, c.a1 != 0); res.X = b.x; res.Y = b.y; res.Z = Fq::zero(); break;
    default: res = msm_horner_quad(pool + c.a0, c.a1, c.a2, r); break;   // LAW_HORNER: pool[a0 .. a0 + a1), a2 doublings per item
    }
    out[i].lane[r] = res;
    if (r == 0) { out[i].flag = flag; out[i].pad[0] = out[i].pad[1] = out[i].pad[2] = 0; }
}
// one quad, a chain: acc <- op(acc, pool[idx]).  A fast form that returns false leaves acc as it is (counted in flag).
struct ChainOp { uint32_t op, idx; };
__global__ void __launch_bounds__(64) k_units_chain(const ChainOp* __restrict__ ops, uint32_t n_ops, const G1JSlot* __restrict__ pool, G1J start, LawOut* __restrict__ out) {
    const uint32_t r = threadIdx.x & 3u;
    G1J acc = start;
    uint32_t refused = 0;
#pragma unroll 1
    for (uint32_t k = 0; k < n_ops; ++k) {
        const ChainOp o = ops[k];
        const G1J q = pool[o.idx].p;
        G1A b; b.x = q.X; b.y = q.Y;
        switch (o.op) {
        case LAW_DBL: acc = g1_dbl_inl(acc); break;
        case LAW_DBL_QUAD: g1_dbl_quad(acc, r); break;
        case LAW_MADD_FAST: if (!g1_madd_fast(acc, b)) ++refused; break;
        case LAW_ADD_FAST: if (!g1_add_fast(acc, q)) ++refused; break;
        case LAW_ADD: acc = g1_add_inl(acc, q); break;
        default: acc = g1_add_affine_inl(acc, b); break;   // LAW_ADD_AFFINE
        }
    }
    if (threadIdx.x < 4) out->lane[r] = acc;
    if (threadIdx.x == 0) { out->flag = refused; out->pad[0] = out->pad[1] = out->pad[2] = 0; }
}
// IN: n_pool, pool points (27 words each); n_cases, cases (LawCase); n_ops, the chain's start (27 words), ops (ChainOp)
// OUT: n_cases LawOut, then (n_ops > 0) one LawOut of the chain
static void run_law(In& in, Out& out) {
    const uint32_t n_pool = in.word();
    REQUIRE(n_pool >= 1 && n_pool <= (1u << 16), "bad pool");
    std::vector<G1J> pool_pts(n_pool);
    in.take(pool_pts.data(), n_pool);
    std::vector<G1JSlot> pool(n_pool);
    for (uint32_t i = 0; i < n_pool; ++i) pool[i] = pool_pts[i];
    const uint32_t n = in.word();
    REQUIRE(n <= (1u << 16), "too many cases");
    std::vector<LawCase> cases(n);
    in.take(cases.data(), n);
    for (const LawCase& c : cases) {
        REQUIRE(c.op < LAW_COUNT, "bad operation");
        if (c.op == LAW_HORNER) REQUIRE(c.a1 >= 1 && c.a0 <= n_pool && c.a1 <= n_pool - c.a0 && c.a2 <= 64, "bad Horner case");
    }
    const uint32_t n_ops = in.word();
    REQUIRE(n_ops <= (1u << 16), "chain too long");
    G1J start = G1J::identity();
    std::vector<ChainOp> ops(n_ops);
    if (n_ops) { in.take(&start, 1); in.take(ops.data(), n_ops); }
    for (const ChainOp& o : ops) REQUIRE(o.op <= LAW_ADD_AFFINE && o.idx < n_pool, "bad chain operation");
    G1JSlot* d_pool = to_device(pool.data(), n_pool);
    LawCase* d_cases = to_device(cases.data(), n);
    ChainOp* d_ops = to_device(ops.data(), n_ops);
    Guarded<LawOut> res((size_t)n + (n_ops ? 1 : 0));
    if (n) hipLaunchKernelGGL(k_units_law, dim3((4 * n + 63) / 64), dim3(64), 0, 0, d_cases, n, d_pool, res.p);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    if (n_ops) hipLaunchKernelGGL(k_units_chain, dim3(1), dim3(64), 0, 0, d_ops, n_ops, d_pool, start, res.p + n);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    res.collect(out, "law results");
    CK(hipFree(d_pool)); CK(hipFree(d_cases)); CK(hipFree(d_ops));
}

// ---- digits
// IN: n_jobs; per job: c, windows, n, n scalars (8 words), n bases (64 bytes)
// OUT per job: windows, buckets, nb, E; the digit table (windows * n words, window-major); counts (nb + MSM_CONTROL_WORDS); offsets (nb); list (E)
static void run_digits(In& in, Out& out) {
    for (uint32_t job = 0, jobs = job_count(in, 64); job < jobs; ++job) {
        const uint32_t c = in.word(), windows = in.word(), n = in.word();
        REQUIRE(c >= 2 && c <= 15 && windows >= 1 && windows <= 128 && n >= 1 && n <= (1u << 16), "bad job");
        const MsmPlan p{n, c, windows, 1u << (c - 1)};
        const uint32_t nb = p.windows * p.buckets;
        const size_t list_cap = (size_t)2 * windows * n;
        uint32_t* d_scalars = to_device(in.span((size_t)8 * n), (size_t)8 * n);
        const std::vector<G1A> bases = bases_from_bytes(in, n);
        G1A* d_bases = to_device(bases.data(), n);
        MsmProblem q(d_scalars, d_bases, nullptr, 8, 1, n);
        MsmProblem* d_q = to_device(&q, 1);
        uint32_t *d_cursor, *d_block;
        G1A* d_phi;
        const uint32_t nblk = (nb + 1023) / 1024;
        Guarded<uint32_t> dig((size_t)windows * n), counts((size_t)nb + MSM_CONTROL_WORDS), offsets(nb), list(list_cap);
        uint32_t *d_dig = dig.p, *d_counts = counts.p, *d_offsets = offsets.p, *d_list = list.p;
        CK(hipMalloc(&d_cursor, (size_t)nb * 4)); CK(hipMalloc(&d_block, ((size_t)nblk + 2) * 4)); CK(hipMalloc(&d_phi, (size_t)n * sizeof(G1A)));
        CK(hipMemset(d_cursor, 0xff, (size_t)nb * 4));
        hipLaunchKernelGGL(msm_glv_prep, dim3((n + 255) / 256, 1), dim3(256), 0, 0, d_q, 1u, p, d_dig, d_phi);
        CK(hipGetLastError());
        // the global counting sort as msm_enqueue_multi runs it
        CK(hipMemsetAsync(d_counts, 0, ((size_t)nb + MSM_CONTROL_WORDS) * 4, 0));
        const uint32_t tiles = (n + MSM_TILE - 1) / MSM_TILE;
        const dim3 gt(8 * tiles);
        const uint32_t wpp = std::max<uint32_t>(1u, std::min<uint32_t>(p.windows, MSM_LDS_WORDS / p.buckets));
        const size_t lds = (size_t)wpp * p.buckets * 4;
        hipLaunchKernelGGL(msm_count_or_scatter<false>, gt, dim3(MSM_TILE_THREADS), lds, 0, d_q, 1u, tiles, p, wpp, d_counts, d_offsets, d_cursor, d_list);
        hipLaunchKernelGGL(msm_block_sums, dim3(nblk), dim3(1024), 0, 0, d_counts, d_block, nb);
        hipLaunchKernelGGL(msm_scan_sums, dim3(1), dim3(1024), 0, 0, d_block, nblk, d_counts + nb + 1);
        hipLaunchKernelGGL(msm_offsets, dim3(nblk), dim3(1024), 0, 0, d_counts, d_block, d_offsets, d_cursor, nb);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        uint32_t E = 0;
        CK(hipMemcpy(&E, d_counts + nb + 1, 4, hipMemcpyDeviceToHost));
        REQUIRE(E <= list_cap, "the count pass found more entries than two per term and window");   // (the scatter pass would write past the list)
        hipLaunchKernelGGL(msm_count_or_scatter<true>, gt, dim3(MSM_TILE_THREADS), lds, 0, d_q, 1u, tiles, p, wpp, d_counts, d_offsets, d_cursor, d_list);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        out.word(windows); out.word(p.buckets); out.word(nb); out.word(E);
        dig.collect(out, "digits"); counts.collect(out, "counts"); offsets.collect(out, "offsets"); list.collect(out, "list", E);
        CK(hipFree(d_scalars)); CK(hipFree(d_bases)); CK(hipFree(d_q)); CK(hipFree(d_cursor)); CK(hipFree(d_block)); CK(hipFree(d_phi));
    }
}

// ---- msm
// IN: n_jobs; per job: msm_global_sort, msm_no_term_split, msm_window_threads, msm_window_wpw, msm_window_slots, n_problems; per problem:
//     n, n1 (terms of the first segment, <= n), phi (1: the caller brings phi(P) with its bases), n scalars (8 words), n bases (64 bytes)
// OUT per job: c, windows, buckets, problems of the launch (sub-problems when cut), cut, chunk length, the control words
//     (MSM_CONTROL_WORDS of them: heavy, E, straddling, team, redo, ...), then every problem's result (27 words)
static void run_msm(In& in, Out& out) {
    for (uint32_t job = 0, jobs = job_count(in, 64); job < jobs; ++job) {
        MsmWorkspace ws;
        ws.tune.struct_size = sizeof(h2v_tuning);
        ws.tune.msm_global_sort = (int)in.word(); ws.tune.msm_no_term_split = (int)in.word(); ws.tune.msm_window_threads = (int)in.word();
        ws.tune.msm_window_wpw = (int)in.word(); ws.tune.msm_window_slots = (int)in.word();
        const uint32_t count = in.word();
        REQUIRE(count >= 1 && count <= MSM_MAX_PROBLEMS, "bad problem count");
        std::vector<void*> owned;
        MsmProblems pr;
        Guarded<G1J> res(count);
        G1J* d_out = res.p;
        size_t total = 0; uint32_t nmax = 0;
        for (uint32_t qi = 0; qi < count; ++qi) {
            const uint32_t n = in.word(), n1 = in.word(), phi = in.word();
            REQUIRE(n <= (1u << 20) && n1 <= n && phi <= 1, "bad problem");
            const uint32_t* sc = in.span((size_t)8 * n);
            const std::vector<G1A> bases = bases_from_bytes(in, n);
            std::vector<G1A> ph(phi ? n : 0);
            for (size_t i = 0; i < ph.size(); ++i) ph[i] = g1_phi(bases[i]);
            // the two segments live in allocations of their own
            uint32_t* s1 = to_device(sc, (size_t)8 * n1); uint32_t* s2 = to_device(sc + (size_t)8 * n1, (size_t)8 * (n - n1));
            G1A* b1 = to_device(bases.data(), n1); G1A* b2 = to_device(bases.data() + n1, n - n1);
            owned.push_back(s1); owned.push_back(s2); owned.push_back(b1); owned.push_back(b2);
            MsmProblem q = n1 == n ? MsmProblem(s1, b1, d_out + qi, 8, 1, n) : MsmProblem(s1, b1, d_out + qi, 8, 1, n1, s2, b2, n - n1);
            if (phi) {
                G1A* p1 = to_device(ph.data(), n1); G1A* p2 = to_device(ph.data() + n1, n - n1);
                owned.push_back(p1); owned.push_back(p2);
                q.phi = p1; if (n1 != n) q.phi2 = p2;
            }
            pr.p.push_back(q);
            total += n; nmax = std::max(nmax, n);
        }
        REQUIRE(total >= 1 && total <= (1u << 20), "bad term total");
        RC(ws.reserve((uint32_t)total, count, nmax));
        RC(msm_enqueue_multi(0, ws, pr));
        CK(hipDeviceSynchronize());
        // the plan of the launch, as msm_enqueue_multi chose it
        MsmLaunchShape L;
        RC(msm_shape(ws, pr, L));
        const MsmPlan p = msm_plan(L.nmax, msm_latency_bound(L.total));
        const uint32_t launched = (uint32_t)L.launch_p.size(), nb = p.windows * p.buckets * launched;
        REQUIRE((size_t)nb + MSM_CONTROL_WORDS <= ws.counts.cap, "plan outside the workspace");
        uint32_t control[MSM_CONTROL_WORDS];
        CK(hipMemcpy(control, ws.counts.p + nb, sizeof(control), hipMemcpyDeviceToHost));
        out.word(p.c); out.word(p.windows); out.word(p.buckets); out.word(launched); out.word(L.cut ? 1u : 0u);
        out.word(msm_chunk_len(control[1], MSM_ACC_LANES_PER_ROUND));
        out.raw(control, sizeof(control));
        res.collect(out, "results");
        for (void* d : owned) CK(hipFree(d));
    }
}

// ---- scale
// IN: n_jobs; per job: J items, n_pairs, 2 * n_pairs Jacobian points (27 words each), J slots, J scalars (8 words)
// OUT per job: words per record, then J records as k_accumulator_scale left them (memory preset to 0xff)
static void run_scale(In& in, Out& out) {
    for (uint32_t job = 0, jobs = job_count(in, 64); job < jobs; ++job) {
        const uint32_t J = in.word(), n_pairs = in.word();
        REQUIRE(J >= 1 && J <= 1024 && n_pairs >= 1 && n_pairs <= 1024, "bad job");
        std::vector<G1J> pairs((size_t)2 * n_pairs);
        in.take(pairs.data(), pairs.size());
        const uint32_t* slots = in.span(J);
        for (uint32_t i = 0; i < J; ++i) REQUIRE(slots[i] < n_pairs, "slot outside the pairs");
        uint32_t* d_slots = to_device(slots, J);
        uint32_t* d_scalars = to_device(in.span((size_t)8 * J), (size_t)8 * J);
        G1J* d_pairs = to_device(pairs.data(), pairs.size());
        Guarded<AccRecord> rec(J);
        RC(accumulator_scale_many_enqueue(0, d_pairs, d_slots, d_scalars, J, rec.p));
        CK(hipDeviceSynchronize());
        out.word((uint32_t)(sizeof(AccRecord) / 4));
        rec.collect(out, "records");
        CK(hipFree(d_slots)); CK(hipFree(d_scalars)); CK(hipFree(d_pairs));
    }
}

static const Mode MODES[] = {{"law", run_law, true, false}, {"digits", run_digits, true, false}, {"msm", run_msm, true, false}, {"scale", run_scale, true, false}};
int main(int argc, char** argv) { return units_main("msm_units", MODES, argc, argv); }
