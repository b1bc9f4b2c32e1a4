"""The sampling build's merge filter (csrc/dev_math.hpp merge_filter_impl, round 10) on the host, against the exact procedure merge_math_impl:
soundness of every "decided" answer under perturbations of the operands up to the proven error bound (1.2e7 random cases and a grid of special
operands and words), the approximations' measured errors on every f32 of their domain against the bounds the derivation uses, 1e5 whole
trees (approximate track + filter + leaf log + replay against the all-exact procedure: flags, words consumed, every node's error, every
replayed operand's bits), and the undecided share on uniform words (at most 4 kappa).  tests/cpp/merge_filter_check.hip says what each part does."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "merge_filter_check.hip")
EXE = os.path.join(ROOT, "tests", "cpp", "merge_filter_check")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc compiles the host harness (it includes dev_math.hpp)")
def test_merge_filter_is_sound_and_its_error_bounds_hold():
    deps = [SRC, os.path.join(ROOT, "nuts_rs_amd", "csrc", "dev_math.hpp"), os.path.join(ROOT, "nuts_rs_amd", "csrc", "detmath_tables.hpp")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unused-value", "-pthread", SRC, "-o", EXE])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "\n0 mismatches" in r.stdout
