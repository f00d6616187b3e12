#!/usr/bin/env python3
"""Writes tests/golden/bn254_plonk_check_cells.json: forty seeded single-cell mutations of satisfying PLONK witnesses over BN254
at 2^5 and 2^8 gates and the report the big-integer yardstick (tests/bn254_plonk_check_model.py) gives for each.
tests/test_bn254_plonk_check_model_cpu.py pins the file against the yardstick; tests/test_gpu_bn254_plonk_check.py compares
nlx_bn254_plonk_check_witness with it field by field."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bn254_plonk_check_model as model  # noqa: E402

if __name__ == "__main__":
    records = model.golden_records()
    with open(model.GOLDEN, "w") as f:
        json.dump(records, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d records -> %s" % (len(records), model.GOLDEN))
