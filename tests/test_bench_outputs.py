"""bench.py's plain run and --dump-outputs: a plain run times exactly --steps steps (one repeat) and leaves the extra measurements to
--full; --dump-outputs writes the last timed step's positions and statistics as float64 .npy files, within 64 MB, the same from run
to run for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from nuts_rs_amd import _lib  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_one_repeat_full_keeps_five(monkeypatch):
    a = _parse(monkeypatch, "--steps", "7")
    assert (a.steps, a.repeats, a.full, a.dump_outputs) == (7, 1, False, None)
    assert _parse(monkeypatch, "--full").repeats == 5
    assert _parse(monkeypatch, "--full", "--repeats", "2").repeats == 2
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--dump-outputs", "x", "--no-record")


def _dump(tmp_path, n_chains, dim):
    import torch
    rng = np.random.default_rng(1)
    pos = torch.from_numpy(rng.normal(size=(n_chains, dim)))
    st = np.zeros(n_chains, dtype=_lib.STATS_DTYPE)
    st["chain"] = np.arange(n_chains)
    st["step_size"] = rng.uniform(size=n_chains)
    st["index_in_trajectory"] = -rng.integers(0, 9, size=n_chains)
    for f in bench.DUMP_SKIP_STATS:                      # what the engine writes there for a NUTS draw: NaN = none
        st[f] = np.nan
    bench.dump_outputs(str(tmp_path), pos, st)
    files = sorted(os.listdir(tmp_path))
    loaded = {f[:-4]: np.load(tmp_path / f) for f in files}
    return pos.numpy(), st, loaded, sum(os.path.getsize(tmp_path / f) for f in files)


def test_dump_outputs_writes_the_defined_fields_in_float64(tmp_path):
    pos, st, got, size = _dump(tmp_path, 96, 40)
    fields = [f for f in _lib.STATS_DTYPE.names if f not in bench.DUMP_SKIP_STATS]
    assert len(fields) == len(_lib.STATS_DTYPE.names) - 3
    assert set(got) == {"position"} | {"stats_" + f for f in fields}
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in got.values())
    assert (got["position"] == pos).all() and got["position"].shape == (96, 40)
    for f in fields:
        assert (got["stats_" + f] == st[f].astype(np.float64)).all()
    assert size < 64e6


def test_dump_outputs_samples_the_same_chains_in_every_file_when_large(tmp_path):
    pos, st, got, size = _dump(tmp_path, 9000, 1024)          # 9000 x (1024 + 21) doubles: 75 MB before sampling
    assert size <= 64e6
    rows = got["stats_chain"].astype(np.int64)
    assert 0 < rows.size < 9000 and (np.diff(rows) > 0).all()
    assert (got["position"] == pos[rows]).all() and (got["stats_step_size"] == st["step_size"][rows]).all()
    again = tmp_path / "again"
    bench.dump_outputs(str(again), __import__("torch").from_numpy(pos), st)
    assert (np.load(again / "stats_chain.npy") == got["stats_chain"]).all()          # a fixed sample


@pytest.mark.gpu
def test_plain_bench_times_its_steps_and_dumps_the_same_outputs(tmp_path):
    steps, warmup, tune = 6, 2, 30
    lines = []
    for tag in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                            "--chains", "64", "--dim", "128", "--num-tune", str(tune), "--dump-outputs", str(tmp_path / tag)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
        lines.append(json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")][-1]))
    d = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d
    assert d["steps"] == steps and d["repeats"]["n"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert "roofline" not in d and "cpu_baseline" not in d and "other_configs" not in d      # --full only
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b")) and "position.npy" in files
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float64 and x.shape == y.shape and (x.view(np.uint64) == y.view(np.uint64)).all(), f
        assert np.isfinite(x).all(), f
    assert np.load(tmp_path / "a" / "position.npy").shape == (64, 128)
    assert (np.load(tmp_path / "a" / "stats_draw.npy") == tune + warmup + steps - 1).all()    # exactly `steps` timed draws, once
    assert (np.load(tmp_path / "a" / "stats_n_steps.npy") > 0).all()
