"""bench.py's plain run and --dump-outputs: the arrays it writes (CPU, with a
stand-in context), and on the GPU a small plain run repeated -- the same line
fields, the same arrays, and the dispatch list the library itself returns."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

NAMES = ("dispatch_lead", "dispatch_trail", "dispatch_count")


class FakeContext:
    def __init__(self, n, big=False):
        rng = np.random.default_rng(7)
        top = (1 << 30) if big else 100000
        self.d = tuple(rng.integers(1, top, size=n).astype(np.int32) for _ in range(3))

    def dispatch(self):
        return self.d


def stats_of(n):
    return {"kmers": 48600000, "buckets": 2400000, "role_pairs": (1 << 40) + 1, "pairs": 9000000, "dispatched": n,
            "aligned": 0, "ovl_records": 0, "dp_cells": 0, "id_mode": 2, "flags": 1}


def test_dump_writes_the_whole_dispatch_exactly(tmp_path):
    ov = FakeContext(5000)
    bench.dump_outputs(str(tmp_path / "d"), ov, stats_of(5000))
    assert sorted(os.listdir(tmp_path / "d")) == sorted(n + ".npy" for n in NAMES + ("stats",))
    for name, want in zip(NAMES, ov.d):
        got = np.load(tmp_path / "d" / (name + ".npy"))
        assert got.dtype == np.float32  # ids below 2^24: exact in float32
        np.testing.assert_array_equal(got.astype(np.int64), want)
    st = np.load(tmp_path / "d" / "stats.npy")
    assert st.dtype == np.float64  # role pairs pass 2^24
    assert [int(x) for x in st] == [stats_of(5000)[k] for k in bench.DUMP_STATS]


def test_dump_keeps_large_values_in_float64(tmp_path):
    ov = FakeContext(1000, big=True)
    bench.dump_outputs(str(tmp_path), ov, stats_of(1000), suffix="_rank1")
    for name, want in zip(NAMES, ov.d):
        got = np.load(tmp_path / (name + "_rank1.npy"))
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got.astype(np.int64), want)


def test_dump_samples_a_list_over_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 32 * 1000)  # room for 1,000 entries
    ov = FakeContext(4321)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), ov, stats_of(4321))
    idx = np.load(tmp_path / "a" / "dispatch_sample_index.npy").astype(np.int64)
    assert len(idx) == 1000 and len(set(idx)) == 1000 and (np.diff(idx) > 0).all() and idx[-1] < 4321
    total = 0
    for f in os.listdir(tmp_path / "a"):
        total += os.path.getsize(tmp_path / "a" / f)
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))  # fixed sample
    assert total <= 32 * 1000 + 5 * 128 + 64  # the budget, the .npy headers, the stats
    for name, want in zip(NAMES, ov.d):
        np.testing.assert_array_equal(np.load(tmp_path / "a" / (name + ".npy")).astype(np.int64), want[idx])


def test_default_budget_is_under_64_mb():
    assert bench.DUMP_BUDGET_BYTES + (1 << 20) <= 64 * 1000 * 1000


def run_bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + [str(a) for a in args],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_every_time(tmp_path):
    import saoverlap as sao
    small = ("--reads", 4000, "--steps", 3, "--warmup", 1)
    a = run_bench(*small, "--dump-outputs", tmp_path / "a")
    b = run_bench(*small, "--dump-outputs", tmp_path / "b")
    for line in (a, b):
        assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
        assert line["unit"] == "candidate k-mer pairs/s" and line["higher_is_better"] is True
        assert line["dtype"] == "int32" and line["ms_per_step"] > 0
        # value is role pairs per second of the timed steps (both rounded in the line)
        assert line["value"] == pytest.approx(line["per_gpu"]["role_pairs"] / (line["ms_per_step"] * 1e-3), rel=0.01)
        for k in ("cpu_baseline", "roofline", "stage_ms_per_step", "aligned_read_pairs_per_s", "config0"):
            assert k not in line  # --full only
    assert a["per_gpu"] == b["per_gpu"]
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(n + ".npy" for n in NAMES + ("stats",)) == sorted(os.listdir(tmp_path / "b"))
    for f in files:
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    # the dumped arrays are the library's dispatch of the same reads
    bases, offsets = bench.synth_workload(4000, 500, 4000 * 500 // 20, 0.5, seed=1)
    with sao.Overlapper(kmer_size=15, id_mode=sao.SA_IDS_WIDE) as ov:
        ov.add_packed(bases.tobytes(), offsets)
        ov.build()
        want, st = ov.dispatch(), ov.stats()
    assert len(want[0]) == st["dispatched"] > 1000
    for name, w in zip(NAMES, want):
        np.testing.assert_array_equal(np.load(tmp_path / "a" / (name + ".npy")).astype(np.int64), w)
    assert [int(x) for x in np.load(tmp_path / "a" / "stats.npy")] == [st[k] for k in bench.DUMP_STATS]
