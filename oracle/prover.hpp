// ORACLE — TEST INFRASTRUCTURE ONLY (see bn254_fp.hpp header).
//
// Test-only key generator and honest PLONKish/KZG/SHPLONK prover.  The reference ships no
// prover and no proof bytes: its tests borrow halo2_proofs::plonk::{keygen_vk, create_proof}
// (halo2_verifier/tests/helpers.rs:31-61), which is not vendored.  This file produces the
// inputs (VK bytes, params bytes, proof bytes) that the verifier under test consumes, in the
// transcript order that lib.rs:33-425 and shplonk.rs:175-267 read them.
// It is deliberately written independently of verifier.cpp (own constraint evaluation over
// the extended coset, own rotation-set construction) so that prover and verifier do not share
// a bug by construction.
#pragma once
#include "vk.hpp"
#include <functional>

namespace h2o {

struct Rng {  // splitmix64 -> uniform Fr (deterministic test randomness)
    u64 s;
    explicit Rng(u64 seed) : s(seed) {}
    u64 next() { u64 z = (s += 0x9e3779b97f4a7c15ULL); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL; z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL; return z ^ (z >> 31); }
    Fr fr() { uint8_t b[64]; for (int i = 0; i < 8; ++i) { u64 w = next(); for (int j = 0; j < 8; ++j) b[8 * i + j] = (uint8_t)(w >> (8 * j)); } return Fr::from_uniform_bytes(b); }
};

// KZG commitment key.  Two modes:
//  * known-s test SRS: commitments are single fixed-base multiplications [p(s)]G;
//  * the reference's own SRS file (halo2_proofs RawBytes layout: k | g[n] | g_lagrange[n] | g2 | s_g2,
//    SURVEY.md §2 row 21): commitments are real MSMs over g / g_lagrange.
struct CommitKey {
    uint32_t k = 0; uint64_t n = 0;
    bool known_s = false;
    Fr s;
    std::vector<Fr> lagrange_at_s;           // L_i(s), known-s mode
    std::vector<G1Affine> g, g_lagrange;     // file mode
    ParamsKZG params;                        // verifier-side params (g, g2, s_g2)
    static CommitKey from_secret(uint32_t k, const Fr& s);
    static CommitKey from_srs_file(const uint8_t* data, size_t len);
    G1Affine commit_lagrange(const std::vector<Fr>& values) const;
    G1Affine commit_coeff(const std::vector<Fr>& coeffs) const;
};

struct CopyConstraint { uint32_t col_a, row_a, col_b, row_b; };  // indices into cs.permutation_columns

// What circuit_generated decided for one seed and witness_generated needs to satisfy it (empty for the hand-written families)
struct GenGate { uint32_t result_col; uint8_t phase; ExprPoly expr; };          // S_g * (expr - result_col@0)
struct GenCell { uint32_t col, row; };
struct GenInfo {
    uint64_t features = 0;                        // GenFeature bits
    size_t act_lo = 0, act_hi = 0;                // the selector is 1 on rows [act_lo, act_hi)
    std::vector<size_t> inst_lens;
    std::vector<uint32_t> random_cols;            // advice columns the witness fills with random values, in their own phase
    std::vector<GenGate> gates;                   // in gate order
    std::vector<std::vector<std::pair<uint32_t, int32_t>>> lookup_inputs;   // per lookup: (advice column, rotation) of each input
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> shuffle_cols;   // per shuffle: (input column, shuffled column) of each position
    std::vector<std::pair<GenCell, GenCell>> advice_copies;                 // (from, to): two cells of phase-0 random columns
    std::vector<std::pair<GenCell, GenCell>> instance_copies;               // (instance cell, advice cell)
    GenCell tamper = {0, 0};                      // a result cell of an active row whose gate a wrong value breaks
};
enum GenFeature : uint64_t {   // one bit per branch of the plan compiler that only the generated family reaches (h2o_setup_features)
    GF_PERM_FIXED = 1ull << 0,           // a fixed column in the permutation
    GF_PERM_INSTANCE_NOT_FIRST = 1ull << 1,   // an instance column in the permutation behind position 0
    GF_INSTANCE_ROTATED = 1ull << 2,     // an instance query at a non-zero rotation, of a column with values, that a gate reads
    GF_FIXED_ROTATED = 1ull << 3,        // a fixed query at a non-zero rotation
    GF_ADVICE_ROT_FAR = 1ull << 4,       // an advice rotation beyond +-1
    GF_ADVICE_ROT_LAST = 1ull << 5,      // an advice rotation equal to -(blinding_factors + 1)
    GF_PHASE_2 = 1ull << 6,              // an advice column of phase 2
    GF_CHALLENGE_LATE = 1ull << 7,       // a user challenge of phase 1 or 2 that is squeezed
    GF_CHALLENGE_UNSQUEEZED = 1ull << 8, // a user challenge of a phase above every advice column's
    GF_CONSTANT_TERM = 1ull << 9,        // a term without factors
    GF_COEFFICIENTS = 1ull << 10,        // a coefficient other than 0, 1, -1
    GF_HIGH_EXPONENT = 1ull << 11,       // an exponent above 2 on a challenge and on a fixed query
    GF_SHARED_POWER = 1ull << 12,        // one (variable, exponent >= 2) pair in two gates
    GF_LOOKUP_ARITY_1 = 1ull << 13,
    GF_LOOKUP_ARITY_3 = 1ull << 14,
    GF_LOOKUP_COMPOSITE = 1ull << 15,    // a table expression of several terms or factors
    GF_MANY_ARGUMENTS_M2 = 1ull << 16,   // two or more lookups and a shuffle under two circuit instances
    GF_CHUNK_ABOVE = 1ull << 17,         // cs_degree - 2 > number of permutation columns (> 0)
    GF_CHUNK_EQUAL = 1ull << 18,
    GF_CHUNK_NOT_DIVIDING = 1ull << 19,  // several permutation sets, the last one short
    GF_DEGREE_9 = 1ull << 20,
    GF_ADVICE_UNQUERIED = 1ull << 21,
    GF_FIXED_TWICE = 1ull << 22,         // a fixed column queried twice, another never
    GF_INSTANCE_COLUMNS_0 = 1ull << 23,
    GF_INSTANCE_COLUMNS_2 = 1ull << 24,
    GF_INSTANCE_COLUMNS_3 = 1ull << 25,
    GF_INSTANCE_EMPTY_COLUMN = 1ull << 26,   // an instance column of length 0 beside a longer one
    GF_SMALL_K = 1ull << 27,             // k other than 8, 14, 18
    GF_NO_PERMUTATION = 1ull << 28,
    GF_NO_LOOKUPS = 1ull << 29,
    GF_GWC_MANY_POINTS = 1ull << 30,     // more than three distinct opening points
    GF_ROTATION_SET_3 = 1ull << 31,      // a commitment opened at three or more points
    GF_IDENTITY_GATE = 1ull << 32,       // a gate that holds identically: c * v - c * v
    GF_PERM_FIXED_QUERY_NOT_FIRST = 1ull << 33,   // a fixed column of the permutation whose rotated query precedes its query at rotation 0
    GF_TWO_INSTANCES = 1ull << 34,       // the seed asks for two circuit instances per transcript
    GF_ALL = (1ull << 34) - 1,           // every bit that names a branch (all but GF_TWO_INSTANCES)
};

struct Circuit {
    uint32_t k = 0;
    uint32_t cs_degree = 3;
    ConstraintSystem cs;
    std::vector<std::vector<Fr>> fixed;   // [num_fixed_columns][n]
    std::vector<CopyConstraint> copies;
    GenInfo gen;
    uint64_t n() const { return 1ULL << k; }
    size_t usable_rows() const { return n() - (cs.blinding_factors() + 1); }
};

// advice[col][row] for the usable rows; called once per phase with the challenges squeezed so far.
typedef std::function<void(unsigned phase, const std::vector<Fr>& challenges, std::vector<std::vector<Fr>>& advice)> WitnessFn;

struct ProvingKey {
    Circuit circuit;
    VerifyingKey vk;
    std::vector<std::vector<Fr>> sigma;          // permutation polynomials, Lagrange values
    std::vector<std::vector<Fr>> fixed_coeff, sigma_coeff;  // coefficient form
    std::vector<std::vector<Fr>> fixed_ext, sigma_ext;      // extended-coset evaluations
    std::vector<Fr> l0_ext, llast_ext, lactive_ext;         // l_0, l_last, 1-(l_last+l_blind) on the coset
    uint32_t ext_k = 0;
};

ProvingKey keygen(const Circuit& c, const CommitKey& ck);

// Produces proof bytes for one circuit instance (instances[col][row]).
// multiopen: 0 SHPLONK, 1 GWC; transcript: 0 Blake2b, 1 Keccak256 (the generic parameters of the reference's prover/verifier pair)
std::vector<uint8_t> create_proof(const ProvingKey& pk, const CommitKey& ck, const std::vector<std::vector<Fr>>& instances,
                                  const WitnessFn& witness, Rng& rng, int multiopen = 0, int transcript = 0);
// several circuit instances in one transcript (the reference's `instances: &[&[&[Fr]]]`, lib.rs:33-49): instances[m], witnesses[m]
std::vector<uint8_t> create_proof_multi(const ProvingKey& pk, const CommitKey& ck, const std::vector<std::vector<std::vector<Fr>>>& instances,
                                        const std::vector<WitnessFn>& witnesses, Rng& rng, int multiopen = 0, int transcript = 0);

// ---- synthetic circuits used by the tests and the bench
// config 1/2/3: the tests/vector_mul.rs shape — 3 advice, 1 instance, 1 fixed (selector), gate s*(a*b-c),
// equality over [instance, a0, a1, a2]; `n_mul` multiplications, products exposed as public inputs.
Circuit circuit_vector_mul(uint32_t k, size_t n_mul);
WitnessFn witness_vector_mul(const std::vector<Fr>& a, const std::vector<Fr>& b);
// tests/shuffle.rs shape: W original + W shuffled first-phase advice, z in the second phase, two user challenges,
// three selectors, no permutation argument.  `shuffled` may be an invalid shuffle (reject case).
Circuit circuit_two_phase_shuffle(uint32_t k, size_t W, size_t H);
WitnessFn witness_two_phase_shuffle(const std::vector<std::vector<Fr>>& original, const std::vector<std::vector<Fr>>& shuffled);
// config 4 style: A advice columns (every 4th also queried at -1 and +1), F fixed, L lookups with 2-column
// input/table expressions, Sh shuffle arguments, a degree-`deg` gate, permutation over all advice columns.
Circuit circuit_wide(uint32_t k, size_t A, size_t F, size_t L, size_t Sh, uint32_t gate_degree, u64 seed);
WitnessFn witness_wide(const Circuit& c, u64 seed);
// A circuit whose whole shape is drawn from `seed` (columns, phases, queries and their rotations, gates S_g * (E_g - r_g) with a
// result column r_g per gate, lookups, shuffles, permutation, cs_degree), satisfiable by construction: c.gen holds what the witness
// needs and the GenFeature bits of what the seed contains.  instances_generated draws the public inputs of one circuit instance,
// witness_generated fills the advice from the same seed; `tamper` changes one result cell of an active row afterwards.
Circuit circuit_generated(uint32_t k, u64 seed);
std::vector<std::vector<Fr>> instances_generated(const Circuit& c, u64 seed);
WitnessFn witness_generated(const Circuit& c, u64 seed, bool tamper);

}  // namespace h2o
