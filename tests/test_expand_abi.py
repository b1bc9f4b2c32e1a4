"""`expand_vector` (reference CpuLogpFunc::expand_vector, src/math/cpu_math.rs:892-899) at the ABI: the expanded dimension of every
density kind is a host-side answer (no GPU), nm_draw_outputs carries d_expanded inside its 128 bytes, and a user module takes part by
defining expanded_dim / expand_element — detected at compile time, so that a module without them exports nothing new."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nuts_rs_amd as N
from nuts_rs_amd import _lib
from nuts_rs_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "nuts_amd.h")
MODDIR = os.path.join(HERE, "_modules")
EXPANDING_HEADER = os.path.join(HERE, "user_density", "my_expanding_normal.hpp")
PLAIN_HEADER = os.path.join(HERE, "user_density", "my_diag_normal.hpp")


def ensure_module(header, struct, dim):
    """The module of `struct` for the tiling of `dim` (a cross-compile), rebuilt when one of its sources is newer."""
    dpl, w = B.pick_tiling(dim)
    out = os.path.join(MODDIR, f"expand_{struct}_dpl{dpl}_w{w}.so")
    srcs = [header, PLAIN_HEADER, os.path.join(HERE, "..", "include", "nuts_amd.h")]
    srcs += [os.path.join(B.CSRC, f) for f in ("density_module.hip", "nuts_expand.hpp", "nuts_contract.hpp", "nuts_kernels.hpp", "nuts_launch.hpp", "dev_math.hpp",
                                               "nuts_group.hpp", "nuts_group_impl.hpp", "nuts_adapt.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs):
        os.makedirs(MODDIR, exist_ok=True)
        B.build_density_module(header, struct, dim, out)
    return out


def expanding_module(dim):
    return ensure_module(EXPANDING_HEADER, "MyExpandingNormal", dim)


def expanded_dim(spec):
    c = spec.to_c()
    out = C.c_uint64(12345)
    _lib.check(N.load_library().nm_logp_expanded_dim(C.byref(c), C.byref(out)))
    return out.value


def test_builtin_densities_expand_to_themselves_except_eight_schools():
    for dim in (0, 1, 1000):
        assert expanded_dim(N.LogpSpec.iid_normal(dim)) == dim
    assert expanded_dim(N.LogpSpec.diag_normal(np.ones(7))) == 7
    assert expanded_dim(N.LogpSpec.funnel(11)) == 11
    assert expanded_dim(N.LogpSpec.mvn_precision(np.eye(6))) == 6
    assert expanded_dim(N.LogpSpec.host_callback(13, lambda chain, x: (0.0, np.zeros_like(x)))) == 13
    assert expanded_dim(N.LogpSpec.eight_schools()) == 10
    # the Python front end asks the same function
    assert N.LogpSpec.eight_schools().expanded_dim() == 10 and N.LogpSpec.iid_normal(1000).expanded_dim() == 1000


def test_expanded_dim_rejects_bad_arguments():
    L = N.load_library()
    out = C.c_uint64()
    assert L.nm_logp_expanded_dim(None, C.byref(out)) == 1
    c = N.LogpSpec.iid_normal(3).to_c()
    assert L.nm_logp_expanded_dim(C.byref(c), None) == 1
    bad = N.LogpSpec.eight_schools()
    bad.dim = 9                                                   # the spec is checked like nm_engine_create checks it
    c = bad.to_c()
    assert L.nm_logp_expanded_dim(C.byref(c), C.byref(out)) == 1


def test_draw_outputs_layout_and_abi_version():
    assert _lib.NmDrawOutputs.d_expanded.offset == 88
    assert C.sizeof(_lib.NmDrawOutputs) == 128
    assert _lib.NmDrawOutputs.reserved.offset == 96 and _lib.NmDrawOutputs.reserved.size == 32
    header = open(HEADER).read()
    want = int(header.split("#define NM_ABI_VERSION")[1].split()[0])
    assert N.load_library().nm_abi_version() == want >= 17
    # the header's struct, field by field, is the ctypes mirror's
    body = header.split("typedef struct nm_draw_outputs {")[1].split("} nm_draw_outputs;")[0]
    names = re.findall(r"^\s*(?:double\*|nm_draw_stats\*|uint64_t)\s+(\w+(?:\[\d+\])?);", body, flags=re.M)
    assert names == [f[0] for f in _lib.NmDrawOutputs._fields_[:-1]] + ["reserved[4]"]
    for sym in ("nm_logp_expanded_dim", "nm_engine_expanded_dim", "nm_engine_expand"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(N.load_library(), sym) and sym in header


@pytest.mark.parametrize("dim", [1, 33])
def test_expanding_module_exports_its_expansion(dim):
    path = expanding_module(dim)
    m = C.CDLL(path)
    assert hasattr(m, "nm_module_expand") and hasattr(m, "nm_module_expanded_dim")
    m.nm_module_expanded_dim.restype = C.c_uint64
    m.nm_module_expanded_dim.argtypes = [C.c_uint64, C.c_void_p, C.c_uint64]
    assert m.nm_module_expanded_dim(dim, None, 0) == dim + 1
    info = (C.c_uint64 * 8)()
    m.nm_module_info(info)                                        # the eight words are what they were
    assert info[1] == N.load_library().nm_abi_version() and (info[2], info[3]) == B.pick_tiling(dim) and list(info[4:]) == [0, 0, 0, 0]
    assert expanded_dim(N.LogpSpec.module(dim, path, np.ones(dim))) == dim + 1


def test_module_without_the_members_exports_nothing_new():
    path = ensure_module(PLAIN_HEADER, "MyDiagNormal", 40)
    m = C.CDLL(path)
    assert hasattr(m, "nm_module_launch")
    assert not hasattr(m, "nm_module_expand") and not hasattr(m, "nm_module_expanded_dim")
    assert expanded_dim(N.LogpSpec.module(40, path, np.ones(40))) == 40


def test_expanded_dim_of_a_missing_module_is_an_error():
    with pytest.raises(N.NutsAmdError) as e:
        expanded_dim(N.LogpSpec.module(5, os.path.join(HERE, "no_such_module.so"), np.ones(5)))
    assert e.value.status == 1 and "cannot load" in str(e.value)
