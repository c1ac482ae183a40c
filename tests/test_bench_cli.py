"""bench.py's command line: a plain run times the headline alone, `--full`
adds every other leg, `--dump-outputs DIR` writes the last timed step's CRCs.

CPU: the option defaults and dump_outputs on host tensors (exact float64,
the seeded sample of a large result).  GPU: one plain run of the benchmark
itself with a dump, its CRCs against the reference-built config-2 golden.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def bench():
    import bench
    return bench


def _parse(bench, argv, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_full_and_dump_are_off_by_default(bench, monkeypatch):
    a = _parse(bench, ["--gpus", "1", "--steps", "7", "--warmup", "3"], monkeypatch)
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 3)
    a = _parse(bench, ["--full", "--dump-outputs", "d"], monkeypatch)
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_is_exact_float64(bench, tmp_path):
    want = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x6104AC89], dtype=np.uint32)
    files = bench.dump_outputs(str(tmp_path / "d"), torch.from_numpy(want.view(np.int32)), 0)
    assert files == {"crc32c.npy": want.size}
    got = np.load(tmp_path / "d" / "crc32c.npy")
    assert got.dtype == np.float64 and np.array_equal(got.astype(np.uint32), want)
    files = bench.dump_outputs(str(tmp_path / "d"), torch.from_numpy(want.view(np.int32)), 3)
    assert files == {"crc32c_rank3.npy": want.size}


def test_dump_outputs_samples_a_large_result(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_VALUES", 1000)
    vals = torch.arange(5000, dtype=torch.int32) * 7
    for d in ("a", "b"):
        files = bench.dump_outputs(str(tmp_path / d), vals, 0)
        assert files == {"crc32c_index.npy": 1000, "crc32c.npy": 1000}
    idx = np.load(tmp_path / "a" / "crc32c_index.npy")
    got = np.load(tmp_path / "a" / "crc32c.npy")
    assert idx.dtype == got.dtype == np.float64
    assert np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < 5000
    assert np.array_equal(got, idx * 7)
    assert np.array_equal(idx, np.load(tmp_path / "b" / "crc32c_index.npy"))  # the same sample in every run
    # at the shipped cap a sampled dump (values + indices, 8 B each) stays under 64 MB
    monkeypatch.undo()
    assert bench.DUMP_MAX_VALUES * 16 + 1024 <= 64 * 10**6


@pytest.mark.gpu
def test_plain_run_dumps_the_golden_crcs(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nvlevelz_amd import crc32c
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 2 and line["ms_per_step"] > 0
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u32"
    assert abs(line["value"] - 100_000 * 4096 / (line["ms_per_step"] * 1e-3) / 2**30) <= 0.01 * line["value"]
    for leg in ("cfg5", "e2e", "shims"):  # --full only
        assert leg not in line
    assert line["cpu_baseline"] is None and "read_ceiling" not in line["roofline"]
    got = np.load(out / "crc32c.npy")
    assert got.dtype == np.float64 and got.shape == (100_000,)
    crcs = got.astype(np.uint32)
    g = load_golden("configs")["cfg2"]
    assert int(crcs[0]) == g["crc_first"][0] and int(crcs[-1]) == g["crc_last"]
    assert crc32c.value(np.ascontiguousarray(crcs, dtype="<u4").tobytes()) == g["digest"]
