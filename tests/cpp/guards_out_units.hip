// k_guards_gather and k_guards_proofs (halo2_verifier_amd/csrc/guards_out.hip), the gather of a batch's Guards (include/h2v_guards.h),
// alone through their launchers on programmed arrays chosen by tests/test_gpu_guards_out_units.py.  Built with the library's flags by
// halo2_verifier_amd/csrc/Makefile (build/guards_out_units); the prelude is tests/cpp/units.h.
//
//   guards_out_units gather IN OUT
// Files are little-endian uint32 words.  Every output buffer is preset to 0xff, lies between two guard bands that are checked after the
// kernels (a write past an output ends the program with status 5) and is `slack` elements longer than what the launch writes: what
// lies past the last term must come back untouched.  Every index of the order table is checked on the host before the launch.
#include "../../halo2_verifier_amd/csrc/guards_out.hip"
#include "units.h"

// IN: n_jobs; per job: n (proofs of the upload), np (point slots per proof), n_shared, T (terms per proof), first, count, slack (terms),
//     form (0: bytes, 1: object form), want (bit 0: scalars, bit 1: bases, bit 2: multipliers, bit 3: statuses); T pairs (kind, index);
//     n * np * 8 words of slot scalars; n_shared * n VK-wide scalars [j][p] of 8 words of canonical bytes (stored in Montgomery form);
//     n * np + n_shared points of 16 words of canonical x | y bytes (all-zero: the identity; not checked against the curve); n
//     multipliers of 8 words of canonical bytes; n status words
// OUT per job: (count * T + slack) * 8 words of scalars; the bases — bytes form: (count * T + slack) * 16 words; object form: count * T
//     + slack points as 16 words of canonical x | y read back from the G1As (a point past the last term: its preset, all 0xff) —; (count +
//     slack) * 8 words of multipliers; count + slack status words.  An output not wanted comes back as its preset.
static void gather_job(In& in, Out& out) {
    const uint32_t n = in.word(), np = in.word(), n_shared = in.word(), T = in.word(), first = in.word(), count = in.word(), slack = in.word(), form = in.word(),
                   want = in.word();
    REQUIRE(n >= 1 && n <= 4096 && np >= 1 && np <= 64 && n_shared <= 64 && T <= 128 && slack <= 64 && form <= 1 && want < 16, "bad gather job");
    REQUIRE(first <= n && count <= n - first, "a range outside the upload");
    std::vector<GuardTerm> order(T);
    for (GuardTerm& t : order) { t.kind = in.word(); t.index = in.word(); REQUIRE(t.kind <= 1 && t.index < (t.kind ? n_shared : np), "a term outside the arrays"); }
    GuardTerm* d_order = to_device(order.data(), T);
    uint32_t* d_slot = to_device(in.span((size_t)n * np * 8), (size_t)n * np * 8);
    const std::vector<Fr> shared = in.fields<Fr>((size_t)n_shared * n);
    Fr* d_shared = to_device(shared.data(), shared.size());
    std::vector<G1A> pts((size_t)n * np + n_shared);
    for (G1A& p : pts) { p.x = in.field<Fq>(); p.y = in.field<Fq>(); }
    G1A* d_pts = to_device(pts.data(), pts.size());
    const std::vector<Fr> mult = in.fields<Fr>(n);
    Fr* d_mult = to_device(mult.data(), n);
    uint32_t* d_status = to_device(in.span(n), n);
    const size_t terms = (size_t)count * T + slack, proofs = (size_t)count + slack;
    Guarded<uint32_t> scal(8 * terms), bytes(form ? 0 : 16 * terms), mult_out(8 * proofs), status_out(proofs);
    Guarded<G1A> objs(form ? terms : 0);
    const GuardsGather g{d_order, T, d_slot, d_shared, d_pts, reinterpret_cast<const int*>(d_status), n, np, first, count};
    if (form) RC(guards_gather_terms_enqueue(0, g, (want & 1u) ? scal.p : nullptr, (want & 2u) ? objs.p : nullptr));
    else RC(guards_gather_bytes_enqueue(0, g, (want & 1u) ? reinterpret_cast<uint8_t*>(scal.p) : nullptr, (want & 2u) ? reinterpret_cast<uint8_t*>(bytes.p) : nullptr));
    RC(guards_proofs_enqueue(0, d_mult, reinterpret_cast<const int*>(d_status), first, count, (want & 4u) ? reinterpret_cast<uint8_t*>(mult_out.p) : nullptr,
                             (want & 8u) ? reinterpret_cast<int*>(status_out.p) : nullptr));
    CK(hipDeviceSynchronize());
    scal.collect(out, "scalars");
    if (form) {
        const std::vector<G1A> got = objs.host("bases");
        const size_t written = (want & 2u) ? (size_t)count * T : 0;
        for (size_t i = 0; i < terms; ++i) {
            if (i < written) { out.field(got[i].x); out.field(got[i].y); }   // (as the library reads them: Montgomery -> canonical on the host)
            else {
                const uint8_t* raw = reinterpret_cast<const uint8_t*>(&got[i]);
                bool preset = true;
                for (size_t k = 0; k < sizeof(G1A); ++k) preset = preset && raw[k] == 0xff;
                std::vector<uint8_t> v(64, preset ? 0xff : 0x00);
                out.raw(v.data(), 64);
            }
        }
    } else bytes.collect(out, "bases");
    mult_out.collect(out, "multipliers"); status_out.collect(out, "statuses");
    CK(hipFree(d_order)); CK(hipFree(d_slot)); CK(hipFree(d_shared)); CK(hipFree(d_pts)); CK(hipFree(d_mult)); CK(hipFree(d_status));
}

static const Mode MODES[] = {{"gather", each_job<gather_job, 256>, true, false}};
int main(int argc, char** argv) { return units_main("guards_out_units", MODES, argc, argv); }
