"""The pinned generated circuits (oracle/prover.hpp: circuit_generated) shared by tests/test_generated_circuits.py (CPU) and
tests/test_gpu_generated_circuits.py: 24 (k, seed) pairs, case i under INSTANTIATIONS[i % 4], with the circuit_instances count the
seed itself asks for.  The first six were picked so that every GenFeature bit occurs under SHPLONK and under GWC; the CPU test
asserts that they still do.  TEST INFRASTRUCTURE ONLY."""
import circuits

INSTANTIATIONS = [(circuits.SHPLONK, circuits.BLAKE2B), (circuits.GWC, circuits.KECCAK256), (circuits.SHPLONK, circuits.KECCAK256), (circuits.GWC, circuits.BLAKE2B)]
CASES = [(5, 127), (6, 286), (7, 176), (5, 399), (6, 44), (7, 76), (5, 3), (6, 7), (7, 1), (5, 2), (6, 4), (7, 5),
         (5, 6), (6, 8), (7, 9), (5, 10), (6, 11), (7, 12), (5, 13), (6, 14), (7, 15), (5, 16), (6, 17), (7, 18)]
S_SEED = 45            # one known-s SRS for all of them: setups of equal k share their params
CONSTRAINT_FAILURE = -2   # plonk Error::ConstraintSystemFailure in the oracle's and the library's numbering
IDS = [f"{i}-k{k}-seed{seed}" for i, (k, seed) in enumerate(CASES)]


def make_setup(i):
    """case i's setup with its multi-open scheme, transcript and circuit_instances selected"""
    k, seed = CASES[i]
    s = circuits.setup_generated(k, seed, s_seed=S_SEED)
    s.set_options(*INSTANTIATIONS[i % 4])
    s.set_circuit_instances(s.want_instances)
    return s


def prove(s, i, witness, tamper=False):
    """one proof of case i: honest, or with one result cell of the last circuit instance changed"""
    m = s.circuit_instances
    return circuits.prove_generated(s, m, witness_seed=1000 * (i + 1) + witness, tamper_at=m - 1 if tamper else -1, rng_seed=31 * i + witness)
