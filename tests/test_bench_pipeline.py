"""bench.py's Pipeline (the RH_ASYNC step loop): every submitted call is settled exactly once, in order, at most
PIPELINE_DEPTH + 1 are in flight, stats come back for the steps that asked for them, an error raised by a settle frees
the call, and several prepared calls are used round-robin.  A fake call object stands in for the C ABI (no GPU).  Also the
options of a plain run and what --dump-outputs writes, on the oracle's batches."""
import os

import pytest

import bench


class FakeStats:
    def __init__(self, d):
        self.d = d

    def as_dict(self):
        return dict(self.d)


class FakeCall:
    def __init__(self, name, fail_at=None):
        self.name, self.fail_at = name, fail_at
        self.next, self.in_flight, self.max_in_flight = 0, set(), 0
        self.waited, self.freed = [], []
        self.stats = FakeStats({})

    def run(self, want_stats):
        h = (self.name, self.next)
        self.next += 1
        self.in_flight.add(h)
        self.max_in_flight = max(self.max_in_flight, len(self.in_flight))
        return h

    def wait(self, h, want):
        assert h in self.in_flight
        self.waited.append(h)
        if self.fail_at is not None and h[1] == self.fail_at:
            raise ValueError("malformed record")
        if want:
            self.stats = FakeStats({"records": 7, "emit_kernel_ms": 1.0 + h[1]})

    def output_bytes(self, h):
        return 1234

    def free(self, h):
        self.in_flight.remove(h)
        self.freed.append(h)


def test_calls_are_settled_in_order_with_bounded_depth():
    c = FakeCall("a")
    info = {}
    p = bench.Pipeline(c, info)
    got = []
    for i in range(10):
        got += p.submit(i % 3 == 0)
    got += p.drain()
    assert c.waited == c.freed == [("a", i) for i in range(10)]
    assert c.max_in_flight == bench.PIPELINE_DEPTH + 1 and not c.in_flight
    assert [g["emit_kernel_ms"] for g in got] == [1.0, 4.0, 7.0, 10.0] and info["output_bytes"] == 1234


def test_round_robin_over_streams_and_error_frees_the_call():
    a, b = FakeCall("a"), FakeCall("b", fail_at=1)
    p = bench.Pipeline([a, b], {})
    for _ in range(3):
        p.submit(False)
    assert a.next == 2 and b.next == 1
    p.submit(False)                       # b's second call (index 1) is submitted ...
    with pytest.raises(ValueError):
        p.drain()                         # ... and fails when it is settled
    assert ("b", 1) in b.freed            # freed although its wait raised


def test_hold_last_keeps_the_final_call_of_a_drain_unfreed():
    """--dump-outputs: the timed region's final drain settles every call but leaves the last one to the caller."""
    c = FakeCall("a")
    p = bench.Pipeline(c, {})
    for _ in range(6):
        p.submit(False)
    p.hold_last = True
    p.drain()
    assert c.waited == [("a", i) for i in range(6)]
    assert p.held == (c, ("a", 5)) and c.in_flight == {("a", 5)} and c.freed == [("a", i) for i in range(5)]


def test_full_is_off_by_default_and_dump_outputs_takes_a_directory():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse_args(["--steps", "3", "--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out" and a.steps == 3


def _oracle_batches(workload, n):
    from avrogen import fastgen
    from avrogen.schemas import SCHEMAS
    from oracle import c_walker
    data, offsets = fastgen.generate(workload, n)
    return c_walker.decode_packed(c_walker.CompiledSchema(SCHEMAS[workload]), data, offsets, 8, threaded=True)


@pytest.mark.parametrize("workload", ["full", "cfg3", "flat4"])
def test_dump_outputs_writes_a_fixed_sample_as_float_arrays(tmp_path, workload):
    """The arrays --dump-outputs writes: float32 / float64 only, within the size bound, the same files and values from run to
    run, and the values of the batches (checked against the rows pyarrow reads back for a few columns)."""
    import numpy as np
    import pyarrow as pa
    batches = _oracle_batches(workload, 50_000)
    info = bench.dump_outputs(batches, str(tmp_path / "a"))
    again = bench.dump_outputs(_oracle_batches(workload, 50_000), str(tmp_path / "b"))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b")) and len(files) == info["arrays"]
    assert info["rows"] == 50_000 and info["rows_sampled"] == min(50_000, bench.DUMP_ROWS) and info["bytes"] <= bench.DUMP_LIMIT
    arrs = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    for f, v in arrs.items():
        assert v.dtype in (np.float32, np.float64), f
        assert np.array_equal(v, np.load(tmp_path / "b" / (f + ".npy"))), f
    assert sum(v.nbytes for v in arrs.values()) == info["bytes"]
    assert arrs["chunk_rows"].tolist() == [b.num_rows for b in batches]
    rows = pa.Table.from_batches(batches).take(pa.array(arrs["sample_rows"].astype(np.int64))).to_pylist()
    if workload == "flat4":
        assert arrs["i"].tolist() == [r["i"] for r in rows] and arrs["d"].tolist() == [r["d"] for r in rows]
        assert [int(h) * 2 ** 32 + int(lo) for h, lo in arrs["l"]] == [r["l"] for r in rows]
    else:
        lens, raw = arrs["name.len"].astype(np.int64), arrs["name.bytes"].astype(np.uint8).tobytes()
        pos = np.concatenate(([0], np.cumsum(lens)))
        names = [raw[pos[i]: pos[i + 1]].decode() if ok else None for i, ok in enumerate(arrs["name.valid"])]
        assert names == [r["name"] for r in rows]
        assert arrs["age.valid"].tolist() == [float(r["age"] is not None) for r in rows]
    if workload == "full":
        codes = {f.name: c for f, c in zip(batches[0].schema.field("status").type, batches[0].schema.field("status").type.type_codes)}
        assert arrs["status.int"].tolist() == [r["status"] for r, c in zip(rows, arrs["status.type"]) if c == codes["int"]]
        lens = arrs["emails.len"].astype(np.int64)
        assert lens.tolist() == [len(r["emails"]) for r in rows] and len(arrs["emails.item.len"]) == lens.sum()


def test_dump_outputs_halves_the_sample_to_fit_the_bound(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT", 200_000)
    info = bench.dump_outputs(_oracle_batches("full", 20_000), str(tmp_path))
    assert info["bytes"] <= 200_000 and info["rows_sampled"] < 20_000
