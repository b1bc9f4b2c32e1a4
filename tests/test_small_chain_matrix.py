"""The case list of tests/test_gpu_small_chain_instantiations.py is the full product it claims to be (no GPU needed): a case that is
deleted later, or a dim that drifts off the edge where the kernel size switches, is noticed here."""
import test_gpu_small_chain_instantiations as M

DENS_GROUP = {"iid": (8, 16, 32), "diag": (8, 16, 32), "funnel": (8, 16, 32), "mvn": (8, 16, 32), "schools": (8,)}
DENS_LANE = {"iid": (2, 4, 5), "diag": (2, 4, 5), "funnel": (2, 4, 5), "schools": (5,)}
GROUP_ENDS = {8: (1, 16), 16: (17, 32), 32: (33, 64)}       # csrc/nuts_contract.hpp group_size: dim <= 16 / 32 / 64
LANE_ENDS = {2: (1, 4), 4: (5, 8), 5: (9, 10)}              # csrc/nuts_contract.hpp lane_pairs: dim <= 4 / 8 / 10


def _bottom(dens, fam, lo):
    return max(lo, 2) if dens == "funnel" or fam in ("micro", "mclmc") else lo


def test_size_functions_match_the_sources():
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nuts_rs_amd", "csrc")
    g = l = open(os.path.join(csrc, "nuts_contract.hpp")).read()      # (the size rules of both families: what the host shares with the kernels)
    assert re.search(r"group_size\(uint64_t dim\) \{ return dim <= 16 \? 8 : dim <= 32 \? 16 : dim <= 64 \? 32 : 0; \}", g)
    assert re.search(r"lane_pairs\(uint64_t dim\) \{ return dim <= 4 \? 2 : dim <= 8 \? 4 : dim <= 10 \? 5 : 0; \}", l)
    assert [M.group_size(d) for d in (1, 16, 17, 32, 33, 64, 65)] == [8, 8, 16, 16, 32, 32, 0]
    assert [M.lane_pairs(d) for d in (1, 4, 5, 8, 9, 10, 11)] == [2, 2, 4, 4, 5, 5, 0]


def test_group_matrix_is_the_full_product():
    cases = M.group_cases()
    ids = [M.case_id(c) for c in cases]
    assert len(set(ids)) == len(ids)
    plain = [c for c in cases if not c["strided"]]
    want = set()
    for dens, sizes in DENS_GROUP.items():
        for gs in sizes:
            for fam in ("euclid", "exact", "micro", "mclmc"):
                lo, hi = (10, 10) if dens == "schools" else (_bottom(dens, fam, GROUP_ENDS[gs][0]), GROUP_ENDS[gs][1])
                want |= {(dens, gs, fam, "nonroomy", lo), (dens, gs, fam, "nonroomy", hi), (dens, gs, fam, "roomy", hi)}
    assert {(c["dens"], c["size"], c["fam"], c["build"], c["dim"]) for c in plain} == want
    assert len(plain) == len(want) == 12 * 4 * 3 + 4 * 2
    # 13 (density, size) pairs x 4 families x 2 builds, each present
    assert len({(c["dens"], c["size"], c["fam"], c["build"]) for c in plain}) == 13 * 4 * 2
    # the stride loop of the non-roomy build: every group size, every family, one dim below the full end (a half-empty last lane pair)
    strided = [c for c in cases if c["strided"]]
    assert {(c["size"], c["fam"]) for c in strided} == {(gs, fam) for gs in (8, 16, 32) for fam in ("euclid", "exact", "micro", "mclmc")}
    assert all(c["build"] == "nonroomy" and c["dim"] == GROUP_ENDS[c["size"]][1] - 1 for c in strided)
    for c in cases:
        assert c["kernel"] == "group" and M.group_size(c["dim"]) == c["size"], c


def test_lane_matrix_is_the_full_product():
    cases = M.lane_cases()
    want = set()
    for dens, sizes in DENS_LANE.items():
        for npairs in sizes:
            for fam in ("euclid", "exact", "micro"):
                lo, hi = (10, 10) if dens == "schools" else (_bottom(dens, fam, LANE_ENDS[npairs][0]), LANE_ENDS[npairs][1])
                want |= {(dens, npairs, fam, lo), (dens, npairs, fam, hi)}
    assert {(c["dens"], c["size"], c["fam"], c["dim"]) for c in cases} == want
    assert len(cases) == len(want) == 9 * 3 * 2 + 3
    assert len({(c["dens"], c["size"], c["fam"]) for c in cases}) == 10 * 3
    for c in cases:
        assert c["kernel"] == "lane" and not c["strided"] and M.lane_pairs(c["dim"]) == c["size"], c


def test_chain_plans_reach_the_build_they_claim():
    """On any device: a non-roomy case needs more than 4 x CUs blocks (nuts_engine.hip's rule for the roomy build), ragged; a strided one
    more chains than its grid holds; at least 64 sampled chains in at least four windows, inside the run, one across a block boundary."""
    for cus in (256, 304, 64):
        for c in M.group_cases():
            n, grid, offs = M.chain_plan(c, cus)
            gpw = 64 // c["size"]
            need = -(-n // gpw)
            if c["build"] == "roomy":
                assert need <= 4 * cus and grid == 0 and n >= 24
                assert sorted(set(i for o in offs for i in range(o, min(o + M.WINDOW, n)))) == list(range(n))
                continue
            assert n % gpw != 0, "the last wavefront is partly empty"
            blocks = grid or need
            assert blocks > 4 * cus
            assert (need > blocks) == c["strided"]
            sampled = set(i for o in offs for i in range(o, o + M.WINDOW))
            assert len(offs) >= 4 and len(sampled) >= 64 and min(sampled) == 0 and max(sampled) == n - 1
            assert any(o // gpw != (o + M.WINDOW - 1) // gpw and blocks // 4 <= o // gpw <= 3 * blocks // 4 for o in offs), "a window across a block boundary mid-grid"
            if c["strided"]:
                assert sum(1 for o in offs if o // gpw >= grid) >= 2, "windows from the second pass"
        for c in M.lane_cases():
            n, grid, offs = M.chain_plan(c, cus)
            assert n == 70 and grid == 0 and sorted(set(i for o in offs for i in range(o, min(o + M.WINDOW, n)))) == list(range(n))
