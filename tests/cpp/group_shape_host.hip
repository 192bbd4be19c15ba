// Host-side exerciser of GroupShape (halo2_verifier_amd/csrc/batch.h), the one description of a batch's groups that host code and
// kernels share: every member against a brute-force table of who owns which proof and which draw, for equal groups (G in 1, 3;
// gs in 1, 5; nt in gs, gs + 3) and unequal ones ([1], [1, 1, 1], [4, 1, 7]), and the refusals of fits().  No argument, no input:
// prints one line per shape and "ok", or the first mismatch and exits 1.  tests/test_group_shape_host.py builds it with the host
// side under the address and undefined-behaviour sanitizers and runs it; no GPU is touched.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../halo2_verifier_amd/csrc/batch.h"
using namespace h2v;

#define CHECK(c) do { if (!(c)) { printf("%s: mismatch at line %d: %s\n", what, __LINE__, #c); exit(1); } } while (0)

// sizes[g] proofs and draws[g] >= sizes[g] draws per group, laid out one group after another
static void check(const char* what, const GroupShape& s, const std::vector<uint32_t>& sizes, const std::vector<uint32_t>& draws) {
    const uint32_t G = (uint32_t)sizes.size();
    std::vector<uint32_t> proof_owner, draw_owner, proof_first(G), draw_first(G);
    uint32_t largest = 0;
    for (uint32_t g = 0; g < G; ++g) {
        proof_first[g] = (uint32_t)proof_owner.size(); draw_first[g] = (uint32_t)draw_owner.size();
        proof_owner.insert(proof_owner.end(), sizes[g], g); draw_owner.insert(draw_owner.end(), draws[g], g);
        if (sizes[g] > largest) largest = sizes[g];
    }
    const size_t n = proof_owner.size(), n_tail = draw_owner.size();
    CHECK(s.G == G && s.largest() == largest);
    for (uint32_t g = 0; g < G; ++g) CHECK(s.first(g) == proof_first[g] && s.count(g) == sizes[g] && s.draw_first(g) == draw_first[g]);
    for (uint32_t p = 0; p < n; ++p) CHECK(s.of(p) == proof_owner[p]);
    for (uint32_t i = 0; i < n_tail; ++i) {
        const GroupShape::Draw d = s.draw_at(i);
        CHECK(d.g == draw_owner[i] && d.j == i - draw_first[d.g]);
        // a zero draw i zeroes the multipliers of the proofs of its group whose own draw comes before it: count them
        uint32_t before = 0;
        for (uint32_t k = 0; k < sizes[d.g]; ++k) if (draw_first[d.g] + k < i) ++before;
        CHECK(s.zero_below(d.j, d.g) == before);
    }
    // the one upload that fits, with the caller's draws or without; every other pair of sizes nearby does not
    for (size_t a = 0; a <= 2 * n + 2; ++a)
        for (size_t t = 0; t <= 2 * n_tail + 2; ++t) {
            CHECK(s.fits(a, t, true) == (a == n && t == n_tail));
            CHECK(s.fits(a, t, false) == (a == n));
            CHECK(!s.misfit(a, t, true) == s.fits(a, t, true));
        }
    printf("%s: %u groups, %zu proofs, %zu draws\n", what, G, n, n_tail);
}

int main() {
    const char* what = "equal";
    for (uint32_t G : {1u, 3u})
        for (uint32_t gs : {1u, 5u})
            for (uint32_t nt : {gs, gs + 3})
                check(what, GroupShape::equal(G, G * gs, G * nt), std::vector<uint32_t>(G, gs), std::vector<uint32_t>(G, nt));
    what = "unequal";
    for (const std::vector<uint32_t>& sizes : {std::vector<uint32_t>{1}, std::vector<uint32_t>{1, 1, 1}, std::vector<uint32_t>{4, 1, 7}}) {
        std::vector<uint32_t> off(1, 0);
        for (uint32_t z : sizes) off.push_back(off.back() + z);
        check(what, GroupShape::unequal((uint32_t)sizes.size(), off.back(), off.data()), sizes, sizes);
    }
    what = "refusals";
    CHECK(!GroupShape::equal(3, 7, 9).fits(7, 9, true));     // n no multiple of G
    CHECK(!GroupShape::equal(3, 7, 7).fits(7, 7, false));    // the same without draws of the caller's
    CHECK(!GroupShape::equal(3, 6, 3).fits(6, 3, true));     // n_tail < n
    CHECK(!GroupShape::equal(3, 6, 8).fits(6, 8, true));     // n_tail no multiple of G
    CHECK(GroupShape::equal(3, 6, 9).fits(6, 9, true) && GroupShape::equal(3, 6, 8).fits(6, 8, false));
    const uint32_t off[] = {0, 4, 5, 12};
    const GroupShape u = GroupShape::unequal(3, 12, off);
    CHECK(!u.fits(11, 11, true) && !u.fits(13, 13, true) && !u.fits(11, 11, false));   // n is not the sum of the sizes
    CHECK(!u.fits(12, 13, true) && !u.fits(12, 11, true));                             // n_tail != n
    CHECK(u.fits(12, 12, true) && u.fits(12, 99, false));
    printf("ok\n");
    return 0;
}
