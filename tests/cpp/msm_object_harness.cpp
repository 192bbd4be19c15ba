// C++ caller of the resident MSM object (include/h2v.hpp Msm, DualMsm, Accumulator::add_msms -> h2v_msm_*, h2v_dual_msm_check_many,
// h2v_accumulator_add_msms): AccumulatorStrategy::process by hand over the Guards of a CPU verify_proof.
//
//   msm_object_harness <dir>
// reads <dir>/params.bin, rand.bin (n x 32), factor.bin (32) and guards.txt with one line per Guard (tests/cpp/caller.h).  It prints
//   hand <ok 0/1> <left hex> <right hex> <n left terms> <n right terms>   D = DualMsm(); per Guard i: D.scale(rand_i); D.add_guard(g_i); check_many({D})
//   each <0/1>...                                                         check_many over one DualMsm per Guard
//   scaled <ok> <left hex> <right hex>                                    E = DualMsm(); E.add_msm(D); E.scale(factor)
//   eval <xy hex> <xy hex> <xy hex> <is_identity 0/1> x 3                 Msm::eval_many({D.left, D.right, D.left})
//   terms <D.left's first scalar hex> <D.right's last base hex>
//   clone <n> <n>                                                         D.left.clone() with a term appended: its length, and D.left's
//   acc <ok> <left hex> <right hex>                                       Accumulator: add_msms(D), add_msms(&D.left, null), finalize
//   empty <size of check_many({}).ok> <size of eval_many({}).xy>          no C call
//   moved <n> <n> <n>                                                     lengths after move construction and move assignment
//   refused <count>                                                       what the mirror refuses before any C call
// A Failure ends the program with status 1 after "failure <code>", every object destroyed on the way out.
// tests/test_gpu_cpp_msm_object.py builds it over the library; tests/test_msm_object_host.py over the stand-in library, with sanitizers.
#include "caller.h"

using namespace caller;

static void checked(const char* name, const DualMsm::Checked& c) { verdict(name, c.ok[0], c.lefts.data(), c.rights.data()); }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: msm_object_harness <dir>\n"); return 2; }
    const std::string d = argv[1];
    const std::vector<Guard> guards = read_guards(d);
    const Bytes rand = slurp(d + "/rand.bin"), factor = slurp(d + "/factor.bin");
    if (guards.empty() || rand.size() != 32 * guards.size() || factor.size() != 32) return 2;
    try {
        ParamsKZG params{slurp(d + "/params.bin"), SerdeFormat::RawBytes};
        Context ctx(params, VerifyingKey{});
        // let mut acc = DualMSM::new(&params); per proof: acc.scale(Fr::random(..)); acc.add_msm(guard)   (kzg/strategy.rs:125-136)
        DualMsm D(ctx);
        for (size_t i = 0; i < guards.size(); ++i) {
            D.scale(Bytes(rand.begin() + 32 * i, rand.begin() + 32 * i + 32));
            D.add_guard(guards[i]);
        }
        const size_t nl = D.left.size(), nr = D.right.size();
        checked("hand", DualMsm::check_many({&D}));
        printf(" %zu %zu\n", nl, nr);
        {
            std::vector<DualMsm> each;
            std::vector<const DualMsm*> ptrs;
            for (const Guard& g : guards) { each.emplace_back(ctx); each.back().add_guard(g); }
            for (const DualMsm& e : each) ptrs.push_back(&e);
            const DualMsm::Checked c = DualMsm::check_many(ptrs);
            printf("each");
            for (bool ok : c.ok) printf(" %d", ok ? 1 : 0);
            printf("\n");
        }
        {
            DualMsm E(ctx);
            E.add_msm(D);
            E.scale(factor);
            checked("scaled", DualMsm::check_many({&E}));
            printf("\n");
        }
        {
            const Msm::Evaluated e = Msm::eval_many({&D.left, &D.right, &D.left});
            printf("eval");
            for (int i = 0; i < 3; ++i) { printf(" "); hex(e.xy.data() + 64 * i, 64); }
            for (int i = 0; i < 3; ++i) printf(" %d", e.is_identity[i] ? 1 : 0);
            printf("\n");
            const Bytes s = D.left.scalars(), b = D.right.bases();
            printf("terms "); hex(s.data(), 32); printf(" "); hex(b.data() + b.size() - 64, 64); printf("\n");
            Msm c = D.left.clone();
            c.append_term(Bytes(guards[0].right_scalars.begin(), guards[0].right_scalars.begin() + 32), Bytes(guards[0].right_bases.begin(), guards[0].right_bases.begin() + 64));
            const size_t nc = c.size(), nd = D.left.size();
            printf("clone %zu %zu\n", nc, nd);
        }
        {
            Accumulator acc(ctx);
            acc.add_msms(D);
            acc.add_msms(&D.left, nullptr);
            const bool ok = acc.finalize();
            acc.read();
            verdict("acc", ok, acc.left(), acc.right());
            printf("\n");
        }
        const size_t e0 = DualMsm::check_many({}).ok.size(), e1 = Msm::eval_many({}).xy.size();
        printf("empty %zu %zu\n", e0, e1);
        // move-only RAII: a handle has one owner, and a moved-from object refuses to be used
        int refused = 0;
        {
            Msm a(ctx);
            a.append_terms(guards[0].left_scalars, guards[0].left_bases);
            Msm b(std::move(a));
            Msm c(ctx);
            c = std::move(b);
            Msm& alias = c;
            c = std::move(alias);   // self-assignment keeps the handle
            DualMsm X(ctx);
            DualMsm Y(std::move(X));
            Y.add_guard(guards[0]);
            DualMsm Z(ctx);
            Z = std::move(Y);
            const size_t n0 = c.size(), n1 = Z.left.size(), n2 = Z.right.size();
            printf("moved %zu %zu %zu\n", n0, n1, n2);
            try { a.size(); } catch (const Failure& f) { refused += f.code == H2V_ERR_BAD_ARGUMENT; }
            try { c.add_msm(b); } catch (const Failure& f) { refused += f.code == H2V_ERR_BAD_ARGUMENT; }
            try { DualMsm::check_many({&X}); } catch (const Failure& f) { refused += f.code == H2V_ERR_BAD_ARGUMENT; }
            try { Msm::eval_many({&c, nullptr}); } catch (const Failure& f) { refused += f.code == H2V_ERR_BAD_ARGUMENT; }
            Accumulator acc(ctx);
            try { acc.add_msms(&a, nullptr); } catch (const Failure& f) { refused += f.code == H2V_ERR_BAD_ARGUMENT; }
            Bytes s33 = guards[0].left_scalars;
            s33.push_back(0);
            try { c.append_terms(s33, guards[0].left_bases); } catch (const Failure& f) { refused += f.code == H2V_ERR_BAD_ARGUMENT; }
            try { c.scale(Bytes(31)); } catch (const Failure& f) { refused += f.code == H2V_ERR_BAD_ARGUMENT; }
            try { Z.scale(Bytes(33)); } catch (const Failure& f) { refused += f.code == H2V_ERR_BAD_ARGUMENT; }
        }
        printf("refused %d\n", refused);
    } catch (const Failure& f) {
        printf("failure %d\n", f.code);
        fprintf(stderr, "failure %d: %s\n", f.code, f.what());
        return 1;
    }
    return 0;
}
