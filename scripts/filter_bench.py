"""Row filters against the unfiltered call IN THE SAME JOB (bench.py does not know `where=`).

    python scripts/filter_bench.py [--records 10000000] [--reps 3] [--host-records 10000000] [--out profiles/filter_10m.json]

`--records` records of the `full` workload, 8 chunks, specialised kernels, one MI355X.  Three predicates, chosen by what they keep:
about 1 % (`age == 50`), about 50 % (`age >= 18`: `age` is null in half of the records and a null matches no comparison) and
100 % (`created_at > 0`: no single comparison on `age` keeps a null).
Device part: the wall time of the device-resident call (`deserialize_to_device`'s road, `rh_decode_device_where`) against the
yardstick of the same job, the unfiltered device call (`rh_decode_device`), with the filter's and the compaction's kernel times
(`rh_filter_last`) and the decode's own (rh_stats).  Host part: `deserialize_array_threaded(..., where=)` (list[bytes] in,
RecordBatches out) against the unfiltered call followed by a pyarrow `filter` of every batch.
Every figure is the median of `--reps` calls after one warm call.  No ratio is asserted: the file is what the prose quotes,
the rows where the filter loses included.  One JSON object on stdout, also written to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PREDICATES = [("1pct", ("age", "==", 50)), ("50pct", ("age", ">=", 18)), ("100pct", ("created_at", ">", 0))]


def _med(xs):
    return {"ms": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-records", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_10m.json"))
    a = ap.parse_args()

    import numpy as np
    import pyarrow.compute as pc
    import torch  # first: the engine shares torch's HIP runtime
    from avrogen import fastgen
    from avrogen.schemas import SCHEMAS
    import pyruhvro_amd as P
    from pyruhvro_amd import cabi

    schema = SCHEMAS["full"]
    out = {"workload": "full", "records": a.records, "chunks": 8, "reps": a.reps, "warm_calls": 1, "kernel_key_full": cabi.kernel_key(schema),
           "predicates": {k: list(v) for k, v in PREDICATES}, "device": {}, "host": {}}
    data, offsets = fastgen.generate("full", a.records)
    out["input_bytes"] = int(offsets[-1])
    d_data = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda:0")
    d_data[: len(data)].copy_(torch.from_numpy(data))
    d_off = torch.from_numpy(offsets.view(np.int64)).to("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()

    def device_call(where):
        t0 = time.perf_counter()
        r = cabi.decode_device(d_data.data_ptr(), d_off.data_ptr(), int(offsets[-1]), a.records, schema, 8, device=0, stream=stream,
                               kernel=cabi.KERNEL_SPECIALIZED, where=where)
        wall = (time.perf_counter() - t0) * 1e3
        st, kept, nbytes = r.stats, r.kept, r.output_bytes
        r.free()
        return wall, st, kept, nbytes

    for _ in range(3):      # size history, kernels loaded
        device_call(None)
    for name, where in [("unfiltered", None)] + PREDICATES:
        device_call(where)
        rows = [device_call(where) for _ in range(a.reps)]
        d = {"wall": _med([r[0] for r in rows]), "decode_kernels_ms": statistics.median(r[1]["size_kernel_ms"] + r[1]["scan_kernel_ms"] + r[1]["emit_kernel_ms"] for r in rows),
             "kept": int(rows[-1][2]), "kept_fraction": rows[-1][2] / a.records, "output_bytes": int(rows[-1][3])}
        if where is not None:
            last = cabi.filter_last()
            d["filter_kernel_ms"], d["compaction_kernels_ms"] = last["filter_ms"], last["gather_ms"]
        out["device"][name] = d
    base = out["device"]["unfiltered"]
    out["device_spread"] = (base["wall"]["max"] - base["wall"]["min"]) / base["wall"]["ms"]
    for d in out["device"].values():
        d["vs_unfiltered"] = d["wall"]["ms"] / base["wall"]["ms"]
    del d_data, d_off
    torch.cuda.empty_cache()

    if a.host_records:
        n = a.host_records
        recs = fastgen.split(data, offsets) if n == a.records else fastgen.split(*fastgen.generate("full", n))
        del data, offsets
        old = P.set_kernel_mode("specialized")
        res = {}

        def timed(f):
            f()
            ts = []
            rows = 0
            for _ in range(a.reps):
                t0 = time.perf_counter()
                b = f()
                ts.append((time.perf_counter() - t0) * 1e3)
                rows = sum(x.num_rows for x in b)
                del b
            return _med(ts), rows

        res["unfiltered"], _ = timed(lambda: P.deserialize_array_threaded(recs, schema, 8))
        for name, where in PREDICATES:
            col, op, k = where
            fn = {"==": pc.equal, ">=": pc.greater_equal, ">": pc.greater}[op]
            t_where, rows_where = timed(lambda: P.deserialize_array_threaded(recs, schema, 8, where=where))
            t_arrow, rows_arrow = timed(lambda: [b.filter(fn(b.column(col), k)) for b in P.deserialize_array_threaded(recs, schema, 8)])
            assert rows_where == rows_arrow, (name, rows_where, rows_arrow)
            res[name] = {"where": t_where, "decode_then_pyarrow_filter": t_arrow, "rows": rows_where,
                         "where_vs_pyarrow": t_where["ms"] / t_arrow["ms"]}
        P.set_kernel_mode(old)
        out["host"] = {"records": n, "calls": res}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
