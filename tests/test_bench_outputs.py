"""bench.py --dump-outputs (CPU): the writer behind every mode's dump. Scalars and arrays
come back as float64 .npy files, absent results are left out, ranks get their own files,
and an output beyond its share of the size limit is a fixed seeded sample."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_dump_outputs_files(tmp_path):
    import bench
    d = str(tmp_path / "dump")
    dv = np.arange(5, dtype=np.float32)
    bench.dump_outputs(d, {"logpdf": -12.5, "dv": dv, "absent": None})
    assert sorted(os.listdir(d)) == ["dv.npy", "logpdf.npy"]
    lp = np.load(os.path.join(d, "logpdf.npy"))
    assert lp.dtype == np.float64 and lp.shape == (1,) and lp[0] == -12.5
    got = np.load(os.path.join(d, "dv.npy"))
    assert got.dtype == np.float64 and np.array_equal(got, dv)
    bench.dump_outputs(d, {"logpdf": 1.0}, rank=1, world=2)
    assert np.load(os.path.join(d, "logpdf_rank1.npy"))[0] == 1.0
    bench.dump_outputs(None, {"logpdf": 1.0})  # no --dump-outputs: nothing to do


def test_dump_outputs_sample_is_bounded_and_fixed(tmp_path, monkeypatch):
    import bench
    limit = 2 * (bench.DUMP_HEADER_BYTES + 8 * 32)  # two files of 32 doubles and a header each
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", limit)
    big = np.random.default_rng(1).standard_normal(1000)
    small = np.arange(3.0)
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), {"big": big, "small": small})
    a, b = (np.load(str(tmp_path / n / "big.npy")) for n in ("a", "b"))
    assert a.size == 32 and np.array_equal(a, b)  # two outputs share the limit; same sample every run
    assert np.all(np.isin(a, big))
    assert np.array_equal(np.load(str(tmp_path / "a" / "small.npy")), small)
    total = sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a")))
    assert total <= limit  # headers included
