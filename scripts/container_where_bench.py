"""Row filters in the container read against what the parent could do, IN THE SAME JOB (bench.py does not know containers).

    python scripts/container_where_bench.py [--records 10000000] [--reps 3] [--out profiles/container_where_10m.json]

`--records` records of the `full` workload, 8 chunks, specialised kernels, one MI355X, host in -> host out.  Three files of the
same records -- `null` with ~64 KB blocks, `null` with ~1 MB blocks, `deflate` with ~64 KB blocks read with inflate="device" --
and the three predicates of scripts/filter_bench.py, chosen by what they keep: about 1 % (`age == 50`), about 50 % (`age >= 18`)
and 100 % (`created_at > 0`).  Per file and predicate, alternated, medians of `--reps` calls after one warm call of each:
  where      read_container_where(file, W, 8): end to end, with the kernel times of rh_container_where_last -- rh_k_split_where,
             and the compaction (offsets + gather; 0 where everything is kept)
  yardstick  read_container(file, 8) followed by a pyarrow `filter` of every batch: end to end, with rh_k_split's time on the same
             file (rh_split_last_ms) -- the price of the predicate inside the walk is the difference of the two split times
  mask       filter_container(file, W): the split and the predicate alone
Once per predicate, on the same records as a device-resident list: rh_k_filter's time (rh_filter_last) -- the pass over every
record that the fusion avoids.  No ratio is asserted: the file is what the prose quotes, the rows where the filter loses included.
One JSON object on stdout, also written to --out; the Markdown table of DESIGN.md 14.4 on stderr.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PREDICATES = [("1pct", ("age", "==", 50)), ("50pct", ("age", ">=", 18)), ("100pct", ("created_at", ">", 0))]
FILES = [("null_64k", 64 << 10, "null", None), ("null_1m", 1 << 20, "null", None), ("deflate_64k_device", 64 << 10, "deflate", "device")]


def _med(xs):
    return {"ms": statistics.median(xs), "min": min(xs), "max": max(xs)}


def container_of(schema: str, data, offsets, block_bytes: int, codec: str) -> tuple:
    """The packed records (payload + n + 1 offsets) as a container whose blocks end at the record boundaries nearest a grid of
    `block_bytes` -> (bytes, number of blocks).  (scripts/container_bench.py's file, its boundaries found in one vectorised search.)"""
    import zlib
    import numpy as np
    from container_bench import SYNC, _zz
    out = bytearray(b"Obj\x01" + _zz(2))
    for k, v in ((b"avro.schema", schema.encode()), (b"avro.codec", codec.encode())):
        out += _zz(len(k)) + k + _zz(len(v)) + v
    out += _zz(0) + SYNC
    n = len(offsets) - 1
    grid = np.arange(0, int(offsets[-1]), block_bytes, dtype=np.uint64)
    edges = np.unique(np.append(np.searchsorted(offsets, grid, side="left"), n)).tolist()
    if edges[0] != 0:
        edges.insert(0, 0)
    mv = memoryview(data)
    offs = offsets.tolist() if n < 1 << 16 else None
    for r0, r1 in zip(edges[:-1], edges[1:]):
        lo, hi = (offs[r0], offs[r1]) if offs else (int(offsets[r0]), int(offsets[r1]))
        payload = mv[lo:hi]
        if codec == "deflate":
            c = zlib.compressobj(1, zlib.DEFLATED, -15)
            payload = c.compress(payload) + c.flush()
        out += _zz(r1 - r0) + _zz(len(payload))
        out += payload
        out += SYNC
    return bytes(out), len(edges) - 1


def table(out: dict) -> str:
    rows = ["| file | blocks | predicate | kept | where: end to end ms (min - max) | read + pyarrow filter ms (min - max) | where / yardstick | "
            "rh_k_split_where ms | rh_k_split ms | compaction ms | filter_container ms | rh_k_filter on the list ms |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for fname, f in out["files"].items():
        for pname, d in f["predicates"].items():
            w, y = d["where"]["wall"], d["yardstick"]["wall"]
            rows.append(f"| {fname} | {f['blocks']} | {pname} | {100 * d['kept_fraction']:.1f} % | {w['ms']:.0f} ({w['min']:.0f} - {w['max']:.0f}) | "
                        f"{y['ms']:.0f} ({y['min']:.0f} - {y['max']:.0f}) | {d['where_vs_yardstick']:.2f} | {d['where']['split_where_ms']:.2f} | "
                        f"{d['yardstick']['split_ms']:.2f} | {d['where']['compaction_ms']:.2f} | {d['mask']['wall']['ms']:.0f} | "
                        f"{out['list_filter_kernel_ms'][pname]:.2f} |")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "container_where_10m.json"))
    ap.add_argument("--files", default=",".join(f[0] for f in FILES), help="which of the files to measure (a comma-separated subset)")
    a = ap.parse_args()

    import numpy as np
    import pyarrow.compute as pc
    import torch  # first: the engine shares torch's HIP runtime
    from avrogen import fastgen
    from avrogen.schemas import SCHEMAS
    import pyruhvro_amd as P
    from pyruhvro_amd import cabi

    t_start = time.perf_counter()

    def note(what):      # progress on stderr: minutes of host work (generating, framing, deflating) lie between the figures
        print(f"[{time.perf_counter() - t_start:6.1f} s] {what}", file=sys.stderr, flush=True)

    schema = SCHEMAS["full"]
    note(f"generating {a.records} records")
    data, offsets = fastgen.generate("full", a.records)
    out = {"workload": "full", "records": a.records, "payload_bytes": int(offsets[-1]), "chunks": 8, "reps": a.reps, "warm_calls": 1,
           "kernel_key_full": cabi.kernel_key(schema), "predicates": {k: list(v) for k, v in PREDICATES}, "list_filter_kernel_ms": {}, "files": {}}
    old = P.set_kernel_mode("specialized")

    # rh_k_filter on the same records as a device-resident list: the pass the fusion avoids
    note("rh_k_filter on the list")
    d_data = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda:0")
    d_data[: len(data)].copy_(torch.from_numpy(data))
    d_off = torch.from_numpy(offsets.view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    list_masks = {}
    for name, where in PREDICATES:
        ts = []
        for rep in range(-1, a.reps):
            m = cabi.filter_device(d_data.data_ptr(), d_off.data_ptr(), int(offsets[-1]), a.records, schema, where, device=0)
            if rep >= 0:
                ts.append(cabi.filter_last()["filter_ms"])
        out["list_filter_kernel_ms"][name] = statistics.median(ts)
        list_masks[name] = m
    del d_data, d_off
    torch.cuda.empty_cache()

    for label, block_bytes, codec, inflate in FILES:
        if label not in a.files.split(","):
            continue
        note(f"{label}: framing")
        blob, nb = container_of(schema, data, offsets, block_bytes, codec)
        note(f"{label}: {nb} blocks, {len(blob)} bytes")
        kw = {"inflate": inflate} if inflate else {}
        f = {"blocks": nb, "file_bytes": len(blob), "codec": codec, "inflate": inflate or "-", "predicates": {}}
        for name, where in PREDICATES:
            col, op, k = where
            fn = {"==": pc.equal, ">=": pc.greater_equal, ">": pc.greater}[op]
            calls = {"where": lambda: P.read_container_where(blob, where, 8, **kw),
                     "yardstick": lambda: [b.filter(fn(b.column(col), k)) for b in P.read_container(blob, 8, **kw)],
                     "mask": lambda: P.filter_container(blob, where, **kw)}
            walls = {c: [] for c in calls}
            kern = {c: [] for c in calls}
            rows = {}
            for rep in range(-1, a.reps):      # (rep -1: every call once, warm, and compared)
                for cname, call in calls.items():
                    t0 = time.perf_counter()
                    b = call()
                    ms = (time.perf_counter() - t0) * 1e3
                    note(f"{label} {name} {cname}: {ms:.0f} ms")
                    if rep < 0:
                        rows[cname] = int(b.sum()) if cname == "mask" else sum(x.num_rows for x in b)
                        if cname == "mask":
                            assert np.array_equal(b, list_masks[name]), (label, name)
                    else:
                        walls[cname].append(ms)
                        kern[cname].append(dict(cabi.container_where_last(), split_last_ms=cabi.split_last_ms()))
                    del b
            assert rows["where"] == rows["yardstick"] == rows["mask"], (label, name, rows)
            d = {"kept": rows["where"], "kept_fraction": rows["where"] / a.records,
                 "where": {"wall": _med(walls["where"]), "split_where_ms": statistics.median(x["split_ms"] for x in kern["where"]),
                           "compaction_ms": statistics.median(x["gather_ms"] for x in kern["where"])},
                 "yardstick": {"wall": _med(walls["yardstick"]), "split_ms": statistics.median(x["split_last_ms"] for x in kern["yardstick"])},
                 "mask": {"wall": _med(walls["mask"]), "split_where_ms": statistics.median(x["split_ms"] for x in kern["mask"])}}
            d["where_vs_yardstick"] = d["where"]["wall"]["ms"] / d["yardstick"]["wall"]["ms"]
            d["split_where_vs_split"] = d["where"]["split_where_ms"] / d["yardstick"]["split_ms"]
            f["predicates"][name] = d
        out["files"][label] = f
        del blob
    P.set_kernel_mode(old)
    note("done")
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(table(out), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
