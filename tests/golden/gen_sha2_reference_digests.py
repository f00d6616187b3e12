"""Writes tests/golden/sha2_reference_digests.json: SHA-256 digests of what the plain-Python references of sha256_air.py and
sha512_air.py compute - the bytes of reference_trace, of its final chaining value, and of binding_columns with its total - on the
inputs of tests/sha2_inputs.py.  Run it on the commit whose values are to be pinned:
    python tests/golden/gen_sha2_reference_digests.py
tests/test_sha2_reference.py recomputes the same digests with the tree under test."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import sha2_inputs as inputs  # noqa: E402


if __name__ == "__main__":
    import nlxpkg
    nlx = nlxpkg.load()
    commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    out = {"produced_by": "python tests/golden/gen_sha2_reference_digests.py", "at_commit": commit,
           "sha256": inputs.reference_cases(nlx.sha256_air, "sha256"), "sha512": inputs.reference_cases(nlx.sha512_air, "sha512")}
    with open(os.path.join(HERE, "sha2_reference_digests.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))
