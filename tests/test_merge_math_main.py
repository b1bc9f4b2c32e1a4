"""The main-tree merge with one exp (csrc/dev_math.hpp merge_math_main, the sampling build's top-level merge) against
merge_math_impl(.., is_main = 1, ..): `total` and `flags` bit for bit on the host, over +-0, +-inf, NaN, equal operands, sub-normal
differences, |diff| around 709 and 745, and 1e6 random pairs (Bernoulli words at the threshold included)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "merge_math_main_check.hip")
EXE = os.path.join(ROOT, "tests", "cpp", "merge_math_main_check")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc compiles the host harness (it includes dev_math.hpp)")
def test_main_tree_merge_with_one_exp_equals_merge_math_bit_for_bit():
    deps = [SRC, os.path.join(ROOT, "nuts_rs_amd", "csrc", "dev_math.hpp"), os.path.join(ROOT, "nuts_rs_amd", "csrc", "detmath_tables.hpp")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unused-value", SRC, "-o", EXE])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "0 mismatches" in r.stdout
