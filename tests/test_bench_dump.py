"""CPU test: bench.py --dump-outputs writes the last timed step's result record
(divide[256], n_root | overflow << 32, total) as exact float64 arrays."""
import numpy as np

import bench


def test_dump_outputs_roundtrip(tmp_path):
    rec = np.zeros(258, np.uint64)
    rec[:20] = np.arange(1, 21, dtype=np.uint64) * np.uint64(164136725)  # counts above 2^31
    rec[256] = np.uint64(20)
    rec[257] = rec[:256].sum(dtype=np.uint64)
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), rec)
    got = {p.name: np.load(p) for p in out.iterdir()}
    assert sorted(got) == ["divide.npy", "n_root.npy", "total.npy"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert (got["divide.npy"].astype(np.uint64) == rec[:256]).all()
    assert got["n_root.npy"].tolist() == [20.0]
    assert got["total.npy"].astype(np.uint64).tolist() == [int(rec[257])]


def test_plain_run_is_headline_only(monkeypatch):
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, "")
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"
