"""bench.py's multi-GPU line fields on the CPU (no GPU): the scaling evidence the driver's SCALE run carries —
the RCCL communicator's own rank count (dk_comm_count), each rank's kernel time and shard, the gather period and
the collective's time — built by bench.scale_fields from what every rank reports."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


class FakeRccl:
    """Stands in for demikernel_amd.Comm: count() is dk_comm_count on the communicator."""

    def __init__(self, n):
        self.n = n

    def count(self):
        return self.n


class FakeTorchStandIn:  # shard.TorchCountsAllreduce has no count(): not the product collective
    pass


def rows(world):
    return [{"rank": r, "kernel_ms_per_step": 0.14 + 0.001 * r, "wall_ms_per_step": 0.15, "frames": 1000 + r,
             "frame_bytes": 10 ** 6, "gpu": {"device_index": r, "name": "gpu"}} for r in reversed(range(world))]


def test_rccl_line_proves_rank_count():
    f = bench.scale_fields(8, FakeRccl(8), rows(8), [0.008, 0.009], 8)
    assert f["rccl_nranks"] == 8 and f["world_size"] == 8 and f["collective_kind"].startswith("rccl")
    assert [r["rank"] for r in f["per_rank"]] == list(range(8))  # sorted by rank whatever the gather order
    assert f["gather_every"] == 8 and abs(f["collective_ms_avg"] - 8.5) < 1e-9
    assert f["kernel_ms_per_step_max"] == 0.147 and f["kernel_ms_per_step_min"] == 0.14


def test_test_mode_line_names_the_stand_in():
    f = bench.scale_fields(2, FakeTorchStandIn(), rows(2), [0.001], 8)
    assert f["rccl_nranks"] is None and "TEST ONLY" in f["collective_kind"]
    assert len(f["per_rank"]) == 2


def test_single_gpu_line():
    f = bench.scale_fields(1, None, rows(1), [], 8)
    assert f["rccl_nranks"] is None and f["collective_kind"] == "none" and f["gather_every"] is None
    assert f["collective_ms_avg"] is None and len(f["per_rank"]) == 1


def test_missized_communicator_is_refused():
    """an RCCL communicator that does not hold every rank exits non-zero (status 4), never a line."""
    import pytest

    for nranks, world in ((1, 8), (4, 8), (8, 4)):
        with pytest.raises(SystemExit) as e:
            bench.scale_fields(world, FakeRccl(nranks), rows(world), [0.008], 8)
        assert e.value.code == 4
    bench.check_comm_size(2, 2)  # the right size passes


class FakeReceiver:  # stands in for shard.ShardedReceiver after drain(): counts() gives the accumulated counters
    def __init__(self, res):
        self.res = res

    def counts(self):
        return self.res.t["flow_counts"], self.res.t["verdict_counts"]


def _results(n, nflows, seed):
    import numpy as np
    import torch

    from demikernel_amd import RxResults

    res = RxResults(n, nflows)
    rng = np.random.default_rng(seed)
    for k, v in res.t.items():  # every bit pattern, the top bit included: u32 / u64 storage seen through int32 / int64
        hi = 2 ** 32 if v.dtype == torch.int32 else 2 ** 53
        a = rng.integers(0, hi, v.numel(), dtype=np.uint64)
        v.copy_(torch.from_numpy(a.astype(np.uint32).view(np.int32) if v.dtype == torch.int32 else a.view(np.int64)))
    return res


def test_dump_outputs_whole_arrays(tmp_path):
    """--dump-outputs: every result array and both counters as float64 .npy, value for value (u32 is exact in f64)."""
    import numpy as np

    res = _results(1000, 37, 1)
    bench.dump_outputs(str(tmp_path / "d"), res, FakeReceiver(res))
    exp = res.to_numpy()
    names = sorted(p.name for p in (tmp_path / "d").iterdir())
    assert names == sorted([k + ".npy" for k in exp] + ["frame_index.npy"])
    for k, v in exp.items():
        got = np.load(tmp_path / "d" / (k + ".npy"))
        assert got.dtype == np.float64 and got.shape == v.shape and np.array_equal(got, v.astype(np.float64))
        assert np.array_equal(got.astype(v.dtype), v)
    assert np.array_equal(np.load(tmp_path / "d" / "frame_index.npy"), np.arange(1000))


def test_dump_outputs_samples_past_the_size_limit(tmp_path, monkeypatch):
    """Past the byte limit the same seeded frames are taken from every per-frame array, run after run, and the files
    stay within the limit; the counters are always whole."""
    import numpy as np

    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 16384)
    res = _results(5001, 11, 2)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), res, FakeReceiver(res))
    files = list((tmp_path / "a").iterdir())
    assert sum(np.load(f).nbytes for f in files) <= 16384
    idx = np.load(tmp_path / "a" / "frame_index.npy").astype(np.int64)
    assert 0 < len(idx) < 5001 and np.all(np.diff(idx) > 0) and idx[-1] < 5001
    exp = res.to_numpy()
    for f in files:
        a = np.load(f)
        assert np.array_equal(a, np.load(tmp_path / "b" / f.name))
        k = f.name[:-4]
        if k in ("flow_counts", "verdict_counts"):
            assert np.array_equal(a, exp[k].astype(np.float64))
        elif k != "frame_index":
            assert np.array_equal(a, exp[k][idx].astype(np.float64))
