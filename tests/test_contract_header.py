"""csrc/nuts_contract.hpp states once what host code and kernels must agree on.  Two properties, no GPU:

the header stands alone — tests/cpp/contract_check.cpp includes nothing else of the project, a plain host compiler (g++, no hipcc) builds
it, and every fact it prints (struct sizes, member offsets, enumerator values, constants, the size rules and slot functions over their
ranges, the predicates over the eight tilings and every NM_LOGP_*) equals tests/golden/host_kernel_contract_parent.json, which the same
program text recorded against the kernel headers of the commit before the facts moved (sizeof(KParams) is what a density module is checked
against at load);

the host units stay host code — engine_plan.hpp and nuts_engine.hip include no project header outside their lists."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nuts_rs_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "contract_check.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_kernel_contract_parent.json")
ROCM_INCLUDE = "/opt/rocm/include"

# the project headers each host unit may include; an exception (real kernel code the engine needs) would be listed here by name: none
ALLOWED = {
    "engine_plan.hpp": {"nuts_contract.hpp", "dev_math.hpp"},
    "nuts_engine.hip": {"nuts_contract.hpp", "dev_math.hpp", "engine_plan.hpp", "engine_host.hpp", "zig_tables.hpp"},
}


@pytest.mark.skipif(not os.path.isdir(ROCM_INCLUDE), reason="the HIP runtime's API header (hipError_t, hipStream_t) is not installed")
def test_contract_header_stands_alone_and_keeps_the_parents_values(tmp_path):
    exe = str(tmp_path / "contract_check")
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE, SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout
    got = {}
    for line in out.splitlines():
        name, value = line.rsplit(None, 1)
        assert name not in got, f"{name} printed twice"
        got[name] = int(value)
    want = json.load(open(GOLDEN))["facts"]
    assert sorted(got) == sorted(want), (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"(now, at the parent): {wrong}"


def test_contract_check_includes_the_contract_alone():
    quoted = re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(SRC).read(), flags=re.M)
    assert quoted == ["../../nuts_rs_amd/csrc/nuts_contract.hpp"]
    quoted = re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(os.path.join(CSRC, "nuts_contract.hpp")).read(), flags=re.M)
    assert quoted == ["../../include/nuts_amd.h"]
    angled = re.findall(r"^\s*#\s*include\s+<([^>]+)>", open(os.path.join(CSRC, "nuts_contract.hpp")).read(), flags=re.M)
    assert sorted(angled) == ["cstdint", "hip/hip_runtime_api.h", "type_traits"]


@pytest.mark.parametrize("unit", sorted(ALLOWED))
def test_host_units_include_no_kernel_header(unit):
    quoted = re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(os.path.join(CSRC, unit)).read(), flags=re.M)
    assert quoted, "the unit includes project headers"
    assert set(quoted) <= ALLOWED[unit], sorted(set(quoted) - ALLOWED[unit])
    assert "nuts_contract.hpp" in quoted
