"""CPU: the pieces of bench.py that decide what a run computes and writes, without a GPU.

* the benchmark's terrain is synth.mountain_tile's, bit for bit (bench.terrain_tile builds it in
  bands on host threads and shuffles it with one gather);
* --dump-outputs writes float32 / float64 arrays, samples long arrays with a fixed seed and stays
  under its 64 MB cap even when every array of a graph is sampled;
* --steps sets the number of timed steps: a run that would time none is refused before any GPU work.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    import bench as b
    return b


@pytest.mark.parametrize("win", [(0, 400, 0, 400), (123, 611, 57, 390), (1589, 1700, 1551, 1554),
                                 (10, 12, 0, 100)])
def test_terrain_is_mountain_tile(bench, synth, win):
    ref = synth.mountain_tile(*win, seed=20250418)
    got = bench.terrain_tile(*win, seed=20250418)
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


class _Graph:
    def __init__(self, V, E, seed=0):
        r = np.random.default_rng(seed)
        self.xyz = r.standard_normal((V, 3)).astype(np.float32)
        self.state = r.integers(-1, 2, V).astype(np.int32)
        self.cid = np.arange(V, dtype=np.int32)
        self.rowptr = np.linspace(0, E, V + 1).astype(np.int32)
        self.col = r.integers(0, V, E).astype(np.int32)
        self.w = r.random(E).astype(np.float32)
        self.dist = r.random(E).astype(np.float32)
        self.V, self.E = V, E


def test_dump_types_and_seeded_sample(bench, tmp_path):
    g = _Graph(300, 5000)
    n = bench.write_outputs(str(tmp_path / "a"), bench.graph_outputs(g), max_rows=1000)
    bench.write_outputs(str(tmp_path / "b"), bench.graph_outputs(g), max_rows=1000)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(f"{k}.npy" for k in ("sizes", "xyz", "state", "cid", "rowptr", "col", "w", "dist"))
    total = 0
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f
        total += a.nbytes
    assert total == n
    assert np.load(tmp_path / "a" / "sizes.npy").tolist() == [300.0, 5000.0]
    assert np.array_equal(np.load(tmp_path / "a" / "xyz.npy"), g.xyz)          # short: all rows, float32
    assert np.array_equal(np.load(tmp_path / "a" / "rowptr.npy"), g.rowptr)     # integers: exact in float64
    rows = bench.dump_rows(5000, 1000)
    assert rows.shape == (1000,) and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "col.npy"), g.col[rows].astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "a" / "w.npy"), g.w[rows])
    assert bench.dump_rows(1000, 1000) is None


def test_dump_stays_under_the_cap_when_everything_is_sampled(bench, tmp_path):
    g = _Graph(bench.DUMP_ROWS + 7, bench.DUMP_ROWS + 11)
    n = bench.write_outputs(str(tmp_path), bench.graph_outputs(g))
    on_disk = sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path))
    assert n <= bench.DUMP_BYTES and on_disk <= bench.DUMP_BYTES, (n, on_disk)


def test_steps_must_time_something():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr, r.stderr
    h = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert h.returncode == 0 and "--full" in h.stdout and "--dump-outputs" in h.stdout
