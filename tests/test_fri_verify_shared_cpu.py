"""The two device verifiers share one core (csrc/fri_proof_layout.hpp, csrc/fri_verify.hpp, csrc/fri_verify.hip): every check of
a FRI proof is written once.  These tests read the sources - a second copy of one of these pieces is how a fix comes to be made in
one verifier and not in the other.  That both proof formats are parsed by the one parser is what the sanitizer tests of
tests/test_stark_verify_cpu.py and tests/test_plonk_verify_cpu.py run: one program, tests/tools/layout_check.cpp, for both."""
import os
import re

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "near-light-client_amd", "csrc")


def _sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".cpp"))}


@pytest.mark.parametrize("pattern, where", [
    (r"void quad_absorb\(", "fri_verify.hip"),
    (r"gl::Ext wave_sum\(", "fri_verify.hip"),
    (r"gl::Ext base_minus\(", "fri_verify.hip"),
    (r"const char\* reason_name\(", "fri_verify.hip"),
    (r"uint32_t num_layers\(", "fri_proof_layout.hpp"),
    (r"uint32_t parse\(", "fri_proof_layout.hpp"),
    (r"FRI_FAIL_FOLD << 8", "fri_verify.hip"),
    (r"!= plen && f->what == SOUND", "fri_proof_layout.hpp"),          # the path-length-byte comparison
    (r"the path kernel left a tree unwritten", "fri_verify.hip"),
    (r"the FRI kernel left a query unwritten", "fri_verify.hip"),
    (r"proof %llu does not verify", "fri_verify.hip"),
    (r"is not canonical\", \(unsigned long long\)\(i % n_pis\)", "fri_verify.hip"),   # the batch entry points' argument check
])
def test_written_once(pattern, where):
    hits = [(f, len(re.findall(pattern, text))) for f, text in _sources().items() if re.search(pattern, text)]
    assert hits == [(where, 1)], (pattern, hits)


def test_one_parser_for_both_formats():
    """the two format headers define no parser of their own, and the stand-alone program hands both formats' layouts to fpl::parse"""
    src = _sources()
    for f in ("stark_proof_layout.hpp", "plonk_proof_layout.hpp"):
        assert '#include "fri_proof_layout.hpp"' in src[f] and "struct Layout : fpl::Layout" in src[f]
        assert "parse(" not in src[f] and "struct Finding" not in src[f] and "hip/" not in src[f]
    assert "hip/" not in src["fri_proof_layout.hpp"]
    tool = open(os.path.join(ROOT, "tests", "tools", "layout_check.cpp")).read()
    assert tool.count("fpl::parse(") == 1 and "spl::make_layout(" in tool and "ppl::make_layout(" in tool
