"""CPU: tools/gnark_plonk_verify_model.py - gnark's plonk.Verify with real pairings, the two openings checked separately -
against gnark_bsb22_model: the model prover's bytes are accepted, and every named tamper of tests/bn254_plonk_verify_cases.py
is refused by both this model and the trapdoor verifier, with the reason and index the verifier's issue names."""
import pytest

from bn254_plonk_verify_cases import ACCEPT, ALGEBRAIC, MALFORMED, PAIRING, R, case, parser_refuses


@pytest.mark.parametrize("n_pi", [0, 2])
@pytest.mark.parametrize("log_n", [3, 4])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_model_accepts_the_model_provers_bytes(k, log_n, n_pi):
    c = case(log_n, k, n_pi)
    assert c.trapdoor_accepts(c.proof)
    assert c.model_verdict(c.proof) == (1, ACCEPT, 0)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_named_tampers_agree_with_the_trapdoor_verifier(k):
    c = case(3, k)
    seen = set()
    for label, data, public, reason, index in c.tampers():
        got = c.model_verdict(data, public)
        print(label, got)
        assert got[0] == 0 and not c.trapdoor_accepts(data, public), label
        if reason is not None:
            assert got == (0, reason, index), label
        if got[1] != MALFORMED:
            assert not parser_refuses(data), label
        seen.add(got[1])
    assert {MALFORMED, ALGEBRAIC, PAIRING} <= seen


def test_a_changed_public_input_breaks_the_relation():
    c = case(4, 1)
    changed = list(c.public)
    changed[0] = (changed[0] + 1) % R
    assert c.model_verdict(c.proof, changed)[:2] == (0, ALGEBRAIC) and not c.trapdoor_accepts(c.proof, changed)


def test_single_bit_flips_agree_with_the_trapdoor_verifier():
    c = case(3, 1)
    for bit, data in c.bit_flips(12, 77):
        got = c.model_verdict(data)
        assert bool(got[0]) == c.trapdoor_accepts(data), bit
        if parser_refuses(data):
            assert got[1] == MALFORMED, bit
