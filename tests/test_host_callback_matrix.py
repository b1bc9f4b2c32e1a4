"""The case lists of tests/test_gpu_host_callback_instantiations.py are the full product they claim to be (no GPU needed): a tiling or a
family that is deleted later, or a dim that drifts out of its tiling's range, is noticed here."""
import os
import re

from nuts_rs_amd import selftest_cases as SC

import test_gpu_host_callback_instantiations as H

# the first dim each tiling serves when the engine chooses by itself (one past the largest smaller cap), and its cap
RANGES = {(2, 1): (2, 128), (4, 1): (129, 256), (8, 1): (257, 512), (16, 1): (513, 1024), (8, 2): (513, 1024), (16, 2): (1025, 2048),
          (4, 4): (513, 1024), (16, 4): (2049, 4096)}
ADAPTING = ("lr_adapt", "lr_mclmc")          # the estimator's range in these lists: caps of at most 256


def test_tilings_match_the_sources():
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nuts_rs_amd", "csrc")
    plan = open(os.path.join(csrc, "engine_plan.hpp")).read()
    m = re.search(r"combos\[8\]\[2\] = \{(.*?)\};", plan)
    assert [tuple(int(v) for v in p) for p in re.findall(r"\{(\d+), (\d+)\}", m.group(1))] == SC.TILINGS == list(RANGES)
    for (d, w), (lo, hi) in RANGES.items():
        assert hi == d * 64 * w and lo == max(max([0] + [dd * 64 * ww for (dd, ww) in SC.TILINGS if dd * 64 * ww < hi]) + 1, 2)
    # the three host-callback units: one launcher each, over every tiling (nuts_launch.hpp NM_DEFINE_LAUNCH)
    for unit, dens in (("kern_host_cb.hip", "HostCb"), ("kern_lr_host_cb.hip", "LrWrap<HostCb>"), ("kern_kin_host_cb.hip", "KinWrap<HostCb>")):
        assert re.search(r"NM_DEFINE_LAUNCH\(\w+, " + re.escape(dens) + r"\)", open(os.path.join(csrc, unit)).read()), unit


def test_host_callback_matrix_is_the_full_product():
    cases = H.hostcb_cases()
    ids = [SC.case_id(c) for c in cases]
    assert len(set(ids)) == len(ids) == 88
    assert all(c["dens"] == "hostcb" and i.startswith("hostcb-") for c, i in zip(cases, ids))
    want = set()
    for k, (d, w) in enumerate(SC.TILINGS):
        lo, cap = RANGES[(d, w)]
        top = cap if k % 2 == 1 else cap - 3             # a full last tile on every second tiling, a ragged one on the others
        for fam in SC.FAMILIES:
            if fam in ADAPTING and cap > 256:
                continue
            want |= {(fam, d, w, top, "top"), (fam, d, w, lo, "bottom")}
    assert {(c["fam"], c["dpl"], c["w"], c["dim"], c["end"]) for c in cases} == want
    assert len(want) == 8 * 5 * 2 + 2 * 2 * 2
    # every tiling with every family allowed at its cap, each at both ends, every dim inside the tiling's range
    by_key = {}
    for c in cases:
        by_key.setdefault((c["fam"], c["dpl"], c["w"]), []).append(c["end"])
        lo, cap = RANGES[(c["dpl"], c["w"])]
        assert lo <= c["dim"] <= cap, c
    assert set(by_key) == {(fam, d, w) for (d, w) in SC.TILINGS for fam in SC.FAMILIES if not (fam in ADAPTING and d * 64 * w > 256)}
    assert all(sorted(v) == ["bottom", "top"] for v in by_key.values())
    assert {c["dim"] for c in cases if c["end"] == "bottom"} == {2, 129, 257, 513, 1025, 2049}
    # ragged and full tiles both occur at one and at several wavefronts per chain
    for multi in (False, True):
        tops = [c["dim"] % (c["dpl"] * 64 * c["w"]) == 0 for c in cases if c["end"] == "top" and (c["w"] > 1) == multi]
        assert any(tops) and not all(tops)
    assert not H.REFUSED or set(H.REFUSED) <= {H.tiling_id(c) for c in cases}


def test_run_sizes_are_the_short_ones():
    """The callback is Python on both sides: 12 warm-up draws + 8 to depth 4, except the adapting families (dim <= 256), which keep the
    package's own sizes (LowRank MCLMC: half its warm-up); MCLMC with the step size that is stable on the coupled density."""
    for c in H.hostcb_cases():
        s, draws, adapting = H.make_run(c)
        assert s.num_chains == H.N_CHAINS == 3
        if adapting:
            assert c["fam"] in ADAPTING and c["dim"] <= 256
            # (LowRank MCLMC calls the estimator after every warm-up draw: half the warm-up keeps a case to a few seconds)
            assert (s.num_tune, draws) == ((50, 55) if c["fam"] == "lr_mclmc" else (100, 110))
            assert s.adapt_options.mass_matrix_update_freq == 5 or c["fam"] == "lr_mclmc"
            continue
        assert (s.num_tune, draws) == (12, 20)
        if c["fam"] == "mclmc":
            assert (s.step_size, s.momentum_decoherence_length) == (0.05, 1.0)
        else:
            assert s.maxdepth == 4
        assert SC.family_of(s) == (["lr_frozen", "lr_adapt"] if c["fam"] == "lr_frozen" else [c["fam"]])


def test_the_density_is_not_permutation_invariant_and_couples_across_borders():
    import numpy as np
    rng = np.random.default_rng(1)
    x = rng.normal(size=300)
    lp, g = H.coupled(0, x)
    # the gradient is the log-density's (central differences), also across a lane border (elements 127 | 128) and at both ends
    for i in (0, 1, 127, 128, 255, 256, 299):
        e = np.zeros(300)
        e[i] = 1e-5
        assert abs((H.coupled(0, x + e)[0] - H.coupled(0, x - e)[0]) / 2e-5 - g[i]) < 1e-6 * max(1.0, abs(g[i]))
    # swapping two neighbours (what a wrong slot-to-word mapping does) changes logp and the gradient: weights differ by index
    y = x.copy()
    y[[128, 129]] = y[[129, 128]]
    lp2, g2 = H.coupled(0, y)
    assert lp2 != lp and not np.array_equal(np.sort(g2), np.sort(g))
    # ... even where the random-walk term cannot see it (a constant vector)
    c = np.full(300, 0.5)
    c2 = c.copy()
    c2[7] = 0.75
    c3 = c.copy()
    c3[8] = 0.75
    assert H.coupled(0, c2)[0] != H.coupled(0, c3)[0]
    # its first statement copies its argument
    x0 = x.copy()
    H.coupled(0, x)
    assert np.array_equal(x, x0)


def test_taxonomy_cases_cover_the_multi_wavefront_tilings_at_a_ragged_top():
    cases = H.taxonomy_cases()
    assert len({H.taxonomy_id(c) for c in cases}) == len(cases) == 8
    assert {(c["kind"], c["dpl"], c["w"]) for c in cases} == {(k, d, w) for k in ("recoverable", "fatal") for (d, w) in [(16, 1), (8, 2), (4, 4), (16, 4)]}
    for c in cases:
        cap = c["dpl"] * 64 * c["w"]
        assert c["dim"] == cap - 3 and RANGES[(c["dpl"], c["w"])][0] <= c["dim"] < cap
        # the thread that owns the last coordinate (csrc/nuts_kernels.hpp elem_index: element 2 (m 64 W + thread) + b): in the last wavefront,
        # not thread 0, which rings and polls
        thread = ((c["dim"] - 1) % (128 * c["w"])) // 2
        assert thread // 64 == c["w"] - 1 and thread % 64 >= 60


def test_package_list_still_has_its_pinned_length():
    assert len(SC.cases()) == 349 and len([c for c in SC.cases() if c["dens"] == "iid"]) == 88
    assert "hostcb" not in SC.DENSITIES and "hostcb" not in SC.KIND_NAME.values()
