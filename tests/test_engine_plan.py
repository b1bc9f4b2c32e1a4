"""The engine's kernel selection (csrc/engine_plan.hpp: plan_engine, plan_transform, plan_draw) on the host, with a constant device —
256 compute units, 8 resident blocks per unit of the wave and group kernels, 2 of the lane kernels — against expectations written by
hand from DESIGN.md's table of kernel families and include/nuts_amd.h's description of lane_groups / lane_chains / chain_tiles: every
chain-count and dim boundary at both sides, the precedence lane > group > tile-diag > wave, the steps of a draw call (they sum to the
call, never exceed two, never name the sampling build for a warm-up draw or the first draw after a set_position), the occupancy queries
asked and their order, and the status of every refusal.  tests/cpp/engine_plan_check.hip says what each part does.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "engine_plan_check.hip")
EXE = os.path.join(ROOT, "tests", "cpp", "engine_plan_check")
CSRC = os.path.join(ROOT, "nuts_rs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc compiles the host harness (engine_plan.hpp includes dev_math.hpp for its host / device logarithm)")
def test_engine_plan_matches_the_documented_selection():
    deps = [SRC, os.path.join(ROOT, "include", "nuts_amd.h")] + [os.path.join(CSRC, h) for h in os.listdir(CSRC) if h.endswith(".hpp")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off", "-Wno-pass-failed", SRC, "-o", EXE])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "\n0 mismatches" in r.stdout
