"""nm_stats_columns and nm_diagnose_stats (sampler diagnostics on the device; defined by this repository, include/nuts_amd.h, DESIGN
§31) without a GPU: the layout of the two structures, the constants, the arguments both calls refuse before any device call, and the
numpy restatement of the definitions (tests/diag_ref.py) against values worked out by hand and against ArviZ's bfmi formula."""
import ctypes as C
import os
import re

import numpy as np

import nuts_rs_amd as N
from nuts_rs_amd import _lib

import diag_ref

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "nuts_amd.h")
STATS, OUT, A1, A2, A3, A4, A5, A6, A7 = (0x10000000 * i for i in range(1, 10))          # never read: far apart, so nothing overlaps
U = np.uint64(2**64 - 1)


def _define(header, name):
    return int(re.search(r"#define\s+" + name + r"\b\s+(\d+)", header).group(1))


def test_structure_sizes_symbols_and_constants():
    assert C.sizeof(_lib.NmDiagSpec) == 8 * 8 and C.sizeof(_lib.NmDiagOutputs) == 10 * 8
    header = open(HEADER).read()
    for cname, mirror, words in (("nm_diag_spec", _lib.NmDiagSpec, 8), ("nm_diag_outputs", _lib.NmDiagOutputs, 10)):
        body = header.split("typedef struct " + cname + " {")[1].split("} " + cname)[0]
        fields = re.findall(r"(\w+)(?:\[(\d+)\])?;", re.sub(r"/\*.*?\*/", "", body))          # every field is one 8-byte word, or an array of them
        assert [n for n, _ in fields] == [n for n, _ in mirror._fields_], cname
        assert sum(int(k or 1) for _, k in fields) == words
    L = N.load_library()
    assert L.nm_abi_version() == 20 and _define(header, "NM_ABI_VERSION") == 20          # purely additive
    for name in ("nm_stats_columns", "nm_diagnose_stats", "nm_diag_last_error"):
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name)
    names = sorted(set(re.findall(r"#define\s+(NM_DIAG_\w+|NM_STAT_WORDS)\b", header)))
    assert len(names) == 1 + 3 + 5 + 6 + 6 + 8 + 3
    for name in names:
        assert _define(header, name) == getattr(_lib, name), name
    assert _lib.NM_STAT_WORDS * 8 == N.STATS_DTYPE.itemsize == 8 * len(N.STATS_DTYPE.names)
    # the columns of the outputs in ABI order are the names the Python surface and the restatement use
    from nuts_rs_amd import sampler
    for prefix, cols, ref_cols in (("NM_DIAG_C_", sampler.DIAG_CHAIN_COUNTS, diag_ref.CHAIN_COUNTS), ("NM_DIAG_V_", sampler.DIAG_CHAIN_VALUES, diag_ref.CHAIN_VALUES),
                                   ("NM_DIAG_P_", sampler.DIAG_POOLED_COUNTS, diag_ref.POOLED_COUNTS), ("NM_DIAG_PV_", sampler.DIAG_POOLED_VALUES, diag_ref.POOLED_VALUES)):
        assert cols == ref_cols
        for i, col in enumerate(cols):
            assert getattr(_lib, prefix + col.upper()) == i, col
    assert (_lib.NM_DIAG_CHAIN_COUNTS, _lib.NM_DIAG_CHAIN_VALUES, _lib.NM_DIAG_POOLED_COUNTS, _lib.NM_DIAG_POOLED_VALUES) == (6, 6, 8, 3)
    assert _lib.NM_DIAG_DEPTH_BINS == diag_ref.DEPTH_BINS == 32 and diag_ref.CHUNK == N.NM_SUMMARY_CHUNK_CHAINS and diag_ref.STAT_WORDS == _lib.NM_STAT_WORDS
    assert (N.NM_DIAG_ALL, N.NM_DIAG_SAMPLING, N.NM_DIAG_TUNING) == (diag_ref.ALL, diag_ref.SAMPLING, diag_ref.TUNING) == (0, 1, 2)
    assert callable(N.stats_columns) and callable(N.sampler_diagnostics) and N.SamplerDiagnostics.__dataclass_fields__["bfmi"]
    # the header says which words are doubles and which are signed: the dtype of the mirror agrees
    kinds = {"f": set(), "i": set(), "u": set()}
    for i, name in enumerate(N.STATS_DTYPE.names):
        kinds[N.STATS_DTYPE[name].kind].add(i)
    assert kinds["f"] == set(range(9, 19)) | {22, 23} and kinds["i"] == {7, 8, 20}
    import dataclasses
    assert len(dataclasses.fields(N.Summary)) == 13 and N.Summary.sampler is None          # attached, not a field


def _diag(spec=(20, 4, 0, 16, 0.3), stats=STATS, outputs=(A1, A2, A3, A4, A5, A6, A7)):
    """the status of a call whose arguments must be refused before anything touches the device (the pointers are never read)"""
    L = N.load_library()
    s = None if spec is None else _lib.NmDiagSpec(*spec)
    o = None if outputs is None else _lib.NmDiagOutputs(*(p or None for p in outputs))
    return L.nm_diagnose_stats(C.byref(s) if s is not None else None, C.c_void_p(stats or None), C.byref(o) if o is not None else None, None)


def test_diagnose_refuses_invalid_arguments_without_a_device():
    L = N.load_library()
    assert _diag(None) == 1
    assert _diag(stats=0) == 1
    assert _diag(outputs=None) == 1
    assert _diag(outputs=(0,) * 7) == 1                                        # every output null
    assert b"nm_diagnose_stats" in L.nm_diag_last_error()
    assert _diag((0, 4, 0, 16, 0.3)) == 1
    assert _diag((20, 0, 0, 16, 0.3)) == 1
    assert _diag((20, 4, 3, 16, 0.3)) == 1                                     # phase > 2
    assert _diag((20, 4, 2**63, 16, 0.3)) == 1
    assert _diag((20, 4, 0, 1, 0.3), outputs=(A1, A2, A3, A4, A5, 0, A7)) == 1          # max_events > 0 without d_events
    assert _diag((20, 4, 0, 16, float("nan"))) == 1
    assert _diag((2**16, 2**16, 0, 16, 0.3)) == 1                              # 2^32 records
    assert _diag((2**32, 1, 0, 16, 0.3)) == 1
    assert _diag((2**40, 2**40, 0, 16, 0.3)) == 1                              # (the product does not fit 64 bits)
    assert b"nm_diagnose_stats" in L.nm_diag_last_error()


def _columns(n_rows=10, fields=(15, 14), stats=STATS, out=OUT, n_fields=None):
    L = N.load_library()
    f = np.array(fields, dtype=np.uint64)
    return L.nm_stats_columns(n_rows, len(f) if n_fields is None else n_fields, f.ctypes.data if fields is not None and len(f) else None,
                              C.c_void_p(stats or None), C.c_void_p(out or None), None)


def test_columns_refuses_invalid_arguments_without_a_device():
    L = N.load_library()
    assert _columns(fields=()) == 1                                            # null fields
    assert _columns(stats=0) == 1
    assert _columns(out=0) == 1
    assert _columns(n_rows=0) == 1
    assert _columns(fields=(1,) * 25, n_fields=0) == 1
    assert _columns(fields=(1,) * 25) == 1                                     # n_fields above NM_STAT_WORDS
    assert _columns(fields=(15, 24)) == 1                                      # the index of no word
    assert _columns(fields=(2**63,)) == 1
    nbytes = 10 * 192
    assert _columns(out=STATS) == 1                                            # in place
    assert _columns(out=STATS + nbytes - 8) == 1                               # the records' last word
    assert _columns(out=STATS - 10 * 2 * 8 + 8) == 1                           # the output's last word is the records' first
    assert b"nm_stats_columns" in L.nm_diag_last_error()


def _records(n_draws, n_chains):
    st = np.zeros((n_draws, n_chains), dtype=N.STATS_DTYPE)
    st["draw"] = np.arange(n_draws, dtype=np.uint64)[:, None]
    st["chain"] = np.arange(n_chains, dtype=np.uint64)[None, :]
    return st


def test_restatement_by_hand():
    """3 draws x 2 chains.  Chain 0: energies 1, 3, 8 (all sampling), accept 0.5, 1.0, 0.75, logp -1, -2, -6, depths 2, 5, 40, one
    divergence at t = 1, steps 3, 31, 7.  Chain 1: the first row tuning, the second sampling, the third unwritten."""
    st = _records(3, 2)
    st["energy"][:, 0], st["mean_tree_accept"][:, 0], st["logp"][:, 0] = [1.0, 3.0, 8.0], [0.5, 1.0, 0.75], [-1.0, -2.0, -6.0]
    st["depth"][:, 0], st["n_steps"][:, 0], st["step_size"][:, 0] = [2, 5, 40], [3, 31, 7], [0.5, 0.25, 0.125]
    st["diverging"][1, 0], st["maxdepth_reached"][2, 0] = 1, 1
    st["energy"][:, 1], st["tuning"][0, 1], st["step_size"][:, 1], st["depth"][:, 1] = [2.0, 5.0, 0.0], 1, [1.0, 2.0, 0.0], [1, 1, 0]
    st["diverging"][0, 1] = 1
    st.view(np.uint8).reshape(3, 2, 192)[2, 1] = 0xFF                           # unwritten
    d = diag_ref.diagnose(st, diag_ref.ALL, max_events=8, bfmi_threshold=1.0)
    assert d.chain_counts[0].tolist() == [3, 1, 1, 41, 40, 0]
    assert d.chain_counts[1].tolist() == [2, 1, 0, 0, 1, 2**64 - 1]            # its last row is unwritten: the status says so
    # chain 0: mean 4, var ((-3)^2 + (-1)^2 + 4^2) / 3 = 26 / 3, diffs 2, 5: (4 + 25) / 2 = 14.5; bfmi = 14.5 / (26 / 3)
    assert d.chain_values[0].tolist() == [2.25 / 3.0, 4.0, 26.0 / 3.0, 14.5 / (26.0 / 3.0), -3.0, 0.125]
    # chain 1 (all phases): energies 2, 5: mean 3.5, var 2.25, one diff 3: 9 / 1 / 2.25 = 4
    assert d.chain_values[1].tolist() == [0.0, 3.5, 2.25, 4.0, 0.0, 2.0]
    assert d.pooled_counts.tolist() == [1, 3, 1, 1, 41, 1, 0, 0]               # chain 1 is not healthy; 1.67 is not < 1.0
    assert d.pooled_values.tolist() == [0.75, 0.125, 14.5 / (26.0 / 3.0)]
    hist = np.zeros(32, dtype=np.uint64)
    hist[[2, 5, 31]] = 1                                                       # depth 40 lands in the last bin
    assert (d.depth_hist == hist).all()
    assert d.n_events == 2 and d.events.tolist() == [[0, 1], [1, 0]]           # (t, c), t first — and the unhealthy chain's event too
    one = diag_ref.diagnose(st, diag_ref.ALL, max_events=1)
    assert one.n_events == 2 and one.events.tolist() == [[0, 1]]
    assert diag_ref.diagnose(st, diag_ref.ALL, max_events=0).events.shape == (0, 2)
    s = diag_ref.diagnose(st, diag_ref.SAMPLING, max_events=8, bfmi_threshold=2.0)
    assert s.chain_counts[1].tolist() == [1, 0, 0, 0, 1, 2**64 - 1] and s.events.tolist() == [[1, 0]]
    assert s.pooled_counts.tolist() == [1, 3, 1, 1, 41, 1, 1, 0]               # 1.67 < 2.0
    t = diag_ref.diagnose(st, diag_ref.TUNING, max_events=8)
    assert t.chain_counts[:, 0].tolist() == [0, 1] and t.events.tolist() == [[0, 1]] and t.pooled_counts.tolist() == [1, 0, 0, 0, 0, 0, 0, 1]
    cols = diag_ref.stats_columns(st, ["energy", "depth", "chain_status", "energy"])
    assert cols.shape == (3, 2, 4) and cols[:, 0, 0].tolist() == [1.0, 3.0, 8.0] and cols[2, 0, 1] == 40.0 and (cols[:, :, 0] == cols[:, :, 3])[:2].all()
    assert (cols[2, 1].view(np.uint64) == 0x7FF8000000000000).all() and cols[1, 1, 2] == 0.0


def test_restatement_against_the_arviz_formula():
    """ArviZ's bfmi: mean(diff(E)^2) / var(E) per chain (ddof 0).  The restatement sums serially where numpy sums pairwise: bound
    n x 2^-52 relative per sum (n = 200 terms, a first-order bound of serial and pairwise summation alike), three sums and two divisions."""
    rng = np.random.default_rng(31)
    st = _records(200, 5)
    st["energy"] = np.cumsum(rng.normal(size=(200, 5)), axis=0) * 0.3 + rng.normal(size=(200, 5)) + 40.0
    st["mean_tree_accept"] = rng.uniform(0.5, 1.0, size=(200, 5))
    d = diag_ref.diagnose(st, diag_ref.ALL)
    e = st["energy"]
    want = np.mean(np.diff(e, axis=0) ** 2, axis=0) / np.var(e, axis=0)
    rel = np.abs(d.chain_values[:, 3] - want) / want
    print("bfmi against the ArviZ formula: worst relative difference", rel.max())
    assert (rel <= 5 * 200 * 2.0**-52).all()
    assert np.allclose(d.chain_values[:, 2], np.var(e, axis=0), rtol=1e-12) and np.allclose(d.chain_values[:, 0], st["mean_tree_accept"].mean(axis=0), rtol=1e-13)
    assert (d.chain_counts[:, 0] == 200).all() and d.pooled_counts[0] == 5 and d.pooled_values[2] == d.chain_values[:, 3].min()


def test_no_rows_and_one_row():
    """k = 0 and k = 1 are what IEEE arithmetic gives, stored as the one NaN"""
    nan = 0x7FF8000000000000
    st = _records(2, 3)
    st["energy"], st["step_size"], st["mean_tree_accept"], st["logp"] = 7.0, 0.5, 0.875, -3.0
    raw = st.view(np.uint8).reshape(2, 3, 192)
    raw[:, 0] = 0xFF                                                            # chain 0: never started
    raw[1, 1] = 0xFF                                                            # chain 1: one row
    d = diag_ref.diagnose(st, diag_ref.ALL)
    assert d.chain_counts[0].tolist() == [0, 0, 0, 0, 0, 2**64 - 1] and (d.chain_values[0].view(np.uint64) == nan).all()
    assert d.chain_counts[1, 0] == 1
    assert d.chain_values[1].view(np.uint64).tolist() == [np.float64(0.875).view(np.uint64), np.float64(7.0).view(np.uint64), 0, nan,
                                                          np.float64(-3.0).view(np.uint64), np.float64(0.5).view(np.uint64)]
    assert d.chain_values[2, 3].view(np.uint64) == nan and d.chain_values[2, 2] == 0.0          # two equal energies: 0 / 0
    assert d.pooled_counts.tolist() == [1, 2, 0, 0, 0, 0, 0, 1] and d.pooled_values.view(np.uint64).tolist()[2] == np.float64(np.inf).view(np.uint64)
    none = diag_ref.diagnose(st, diag_ref.TUNING)                               # nothing selected anywhere, one healthy chain
    assert (none.chain_counts[:, 0] == 0).all() and (none.chain_values.view(np.uint64) == nan).all()
    assert none.pooled_values.view(np.uint64).tolist() == [nan, nan, np.float64(np.inf).view(np.uint64)]
    raw[:] = 0xFF                                                               # no healthy chain: 0 / 0
    assert diag_ref.diagnose(st).pooled_values.view(np.uint64).tolist() == [nan, nan, np.float64(np.inf).view(np.uint64)]
