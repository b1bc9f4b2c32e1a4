"""nuts_rs_amd.selftest: the known answers are data computed by the oracle (CPU test: regenerating them gives the
committed file), the built library reproduces them on every kernel family (GPU test), and a library that does not is reported — by the
per-instantiation guard every time an engine of the failed instantiation is created, not only the first time (CPU tests on a stub engine)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_golden_file_is_what_the_oracle_computes(oracle, tmp_path):
    import nuts_rs_amd as N
    from nuts_rs_amd import selftest
    from helpers import oracle_settings
    gold = json.load(open(selftest.GOLDEN))["cases"]
    assert set(gold) == set(selftest.CASES)
    for name, (mk, chains, seed, draws, threads) in selftest.CASES.items():
        logp = mk()
        s = N.DiagNutsSettings(num_chains=chains, seed=seed, num_tune=20, num_draws=draws)
        x0 = oracle.init_positions_uniform(s.seed, 0, chains, logp.dim)
        pos, st, steps, failed = oracle.run(oracle_settings(oracle, s), logp.kind, logp.dim, logp.params, oracle.gpu_cfg(threads), chains, x0, draws, n_threads=2)
        g = gold[name]
        assert failed == 0 and steps == g["total_leapfrogs"] and st["n_steps"].astype(int).tolist() == g["n_steps"]
        assert [format(int(v), "016x") for v in pos[-1].reshape(-1).view(np.uint64)] == g["last_position_bits"]


# ---- the per-instantiation guard must not fail open (no GPU: a stub engine, `check_case` replaced) ---------------------------------------------
class _StubBatch:
    """What `selftest.first_use` reads of an engine: here the (iid, nuts, 4 doubles per lane, 1 wavefront) instantiation."""

    def __init__(self):
        import nuts_rs_amd as N
        self.logp = N.LogpSpec.iid_normal(200, 0.5)
        self.settings = N.DiagNutsSettings(num_chains=2, seed=5)

    def blocks_per_chain(self):
        return 1

    def dims_per_lane(self):
        return 4

    def threads_per_chain(self):
        return 64


_STUB_KEY = ("iid", "nuts", 4, 1)


def _guard(monkeypatch, failing=()):
    """`selftest` with nothing verified yet and `check_case` replaced: the cases whose id is in `failing` fail -> the ids checked, in order."""
    from nuts_rs_amd import selftest, selftest_cases as SC
    seen = []

    def check_case(c, device=-1):
        seen.append(SC.case_id(c))
        return f"{SC.case_id(c)}: the draws differ from the known answer" if SC.case_id(c) in failing else None
    monkeypatch.delenv("NUTS_AMD_SELFTEST", raising=False)
    monkeypatch.setattr(selftest, "_checked", set())
    monkeypatch.setattr(selftest, "_busy", False)
    monkeypatch.setattr(selftest, "check_case", check_case)
    return selftest, seen


def _ids(key):
    from nuts_rs_amd import selftest_cases as SC
    return [SC.case_id(c) for c in SC.cases() if (c["dens"], c["fam"], c["dpl"], c["w"]) == key]


def test_first_use_refuses_a_failing_instantiation_every_time(monkeypatch):
    """After a SelfTestError a second engine of the same instantiation in the same process is checked, and refused, again: the guard used to
    mark the instantiation as verified BEFORE running its cases and let the second engine sample with the kernel that had just failed."""
    ids = _ids(_STUB_KEY)
    assert len(ids) == 2
    for victim in ids:                                   # whichever of the instantiation's cases fails
        selftest, seen = _guard(monkeypatch, failing={victim})
        for attempt in range(2):
            with pytest.raises(selftest.SelfTestError) as e:
                selftest.first_use(_StubBatch())
            assert victim in str(e.value)
            assert _STUB_KEY not in selftest._checked
        assert seen.count(victim) == 2


def test_first_use_checks_a_passing_instantiation_once(monkeypatch):
    selftest, seen = _guard(monkeypatch)
    assert selftest.first_use(_StubBatch()) == 2 and seen == _ids(_STUB_KEY)
    assert _STUB_KEY in selftest._checked
    assert selftest.first_use(_StubBatch()) == 0 and len(seen) == 2          # the second engine: nothing is run


def test_a_failing_run_all_leaves_the_failed_instantiation_unverified(monkeypatch):
    """`run_all` used to mark every instantiation it had run, the failed ones included."""
    ids = _ids(_STUB_KEY)
    selftest, seen = _guard(monkeypatch, failing={ids[1]})
    with pytest.raises(selftest.SelfTestError) as e:
        selftest.run_all(only="iid-nuts-")
    assert ids[1] in str(e.value) and "1 of 16" in str(e.value)
    assert _STUB_KEY not in selftest._checked
    assert ("iid", "nuts", 2, 1) in selftest._checked and len(selftest._checked) == 7      # its seven siblings passed
    del seen[:]
    with pytest.raises(selftest.SelfTestError):          # ... so the first engine of the failed one is still checked
        selftest.first_use(_StubBatch())
    assert seen == ids
    # a run that covered only one of an instantiation's two cases has not verified it either
    selftest, seen = _guard(monkeypatch)
    assert selftest.run_all(only=ids[0]) == 1
    assert _STUB_KEY not in selftest._checked
    assert selftest.run_all(only="iid-nuts-4x1-") == 2 and _STUB_KEY in selftest._checked


@pytest.mark.gpu
def test_selftest_passes_on_the_built_library_and_reports_a_wrong_answer(tmp_path, monkeypatch):
    from nuts_rs_amd import selftest
    assert selftest.run() == len(selftest.CASES) * len(selftest.FAMILIES)
    # a corrupted known answer stands in for a library that computes something else
    bad = json.load(open(selftest.GOLDEN))
    bad["cases"]["eight_schools"]["n_steps"][7][3] += 1
    f = tmp_path / "bad.json"
    f.write_text(json.dumps(bad))
    monkeypatch.setattr(selftest, "GOLDEN", str(f))
    with pytest.raises(selftest.SelfTestError) as e:
        selftest.run()
    assert "eight_schools" in str(e.value) and "[7, 3]" in str(e.value)
