"""bench.py's plain run and ``--dump-outputs``.

A plain run prints the headline line without the ``--full`` blocks, and
``--dump-outputs DIR`` writes the tables of the last timed step as float64
``.npy`` files -- whole when they fit the budget, else the elements at fixed
seeded indices -- identical from run to run."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("cpu_baseline", "cpu_reference_path", "cpu_reference_path_all_cores", "dropin",
             "materialised_flows", "host_boundary", "pipelined", "gpu_over_cpu")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    import torch
    b = _bench()
    small = torch.arange(-6, 6, dtype=torch.int32).view(3, 4)
    big = torch.arange(1000, dtype=torch.int16)
    monkeypatch.setattr(b, "DUMP_BUDGET", 2 * 8 * 100)      # 100 float64 elements per array
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), {"small": small, "big": big})
    a = np.load(tmp_path / "a" / "small.npy")
    assert a.dtype == np.float64 and np.array_equal(a, small.numpy())
    assert not (tmp_path / "a" / "small.index.npy").exists()
    s, idx = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "a" / "big.index.npy")
    assert s.dtype == np.float64 and s.shape == idx.shape == (50,)
    assert np.array_equal(s, big.numpy()[idx.astype(np.int64)])
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 2 * 8 * 100 + 3 * 128
    for f in ("small.npy", "big.npy", "big.index.npy"):     # the same sample every run
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


@pytest.mark.gpu
def test_plain_run_dumps_last_step_tables(tmp_path):
    from oracle import oracle as O
    from sdnmpi_amd import topologies as T
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", "3", "--warmup", "1", "--fabric", "fat_tree:8",
                        "--layout", "int32", "--dump-outputs", str(tmp_path)],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "routes/s" and line["higher_is_better"] is True
    assert line["roofline"]["kernel_ms"] > 0
    assert not [k for k in FULL_ONLY if k in line] and line["single_step_ms"] is None
    fabric = T.fat_tree(8)
    csr = fabric.csr()
    srcs = np.unique(fabric.host_table()[0]).astype(np.int32)
    parent, port, _ = O.dfs_tables(csr, srcs)
    assert sorted(os.listdir(tmp_path)) == ["parent.npy", "port.npy"]
    got_parent, got_port = np.load(tmp_path / "parent.npy"), np.load(tmp_path / "port.npy")
    assert got_parent.dtype == np.float64 and got_parent.shape == (len(srcs), csr.V)
    assert np.array_equal(got_parent, parent) and np.array_equal(got_port, port)
