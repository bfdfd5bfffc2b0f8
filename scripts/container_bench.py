"""Container reads against the list and BinaryArray paths IN THE SAME RUN (bench.py does not know containers).

    python scripts/container_bench.py [--records 10000000] [--reps 7] [--out profiles/container_full10m.json]

`--records` records of the `full` workload, 8 chunks, specialised kernels, warm, host in -> host out:
  list          deserialize_array_threaded(list[bytes])         the yardsticks: unchanged paths, with their run-to-run spread
  binary_array  deserialize_binary_array(BinaryArray)
  null_64k      read_container of the same records as a `null` container with ~64 KB blocks
  null_1m       ... with ~1 MB blocks
  deflate_64k   ... as a `deflate` container with ~64 KB blocks (inflated on the host with zlib, then the same blocks call)
Every figure is the median of `--reps` calls: end-to-end wall time, and for the container reads the split kernel's own GPU time
(rh_split_last_ms) next to the decode kernels' (size, scan, emit: rh_stats), and the host's share of one blocks call: inflating,
the upload of the file (rh_stats.h2d_ms) and the export of the results to host memory (d2h_ms).  No threshold: the table prices the split walk.
`--inflate` measures instead the two roads of a `deflate` file ("Deflate blocks on the device"): the same records at
~64 KB and ~1 MB blocks, read_container(inflate="host") and (inflate="device") alternated in one job, medians of 3, with the two
inflate kernels' GPU times (rh_inflate_last) and the split's beside them -> profiles/container_inflate_10m.json.
`--tolerant` measures instead the tolerant read against the strict one IN ONE JOB, alternated: the `null` file of
~64 KB blocks read by read_container, the same clean file by read_container_tolerant, and the same file with 1 % of its blocks
damaged (12 bytes of 0xFF in the middle of the payload) by read_container_tolerant; medians of `--reps` (default 5) with min and
max, the salvage's own kernel times (rh_salvage_last) beside them -> profiles/container_salvage_10m.json.  No threshold.
`--deflate` measures instead the two roads of a `deflate` WRITE: the records as one RecordBatch written by
write_container(codec="deflate") at block_rows 512 and 4096, deflate="host" and deflate="device" alternated in one job, medians of 3
after one warm call of each, with the two deflate kernels' GPU times (rh_deflate_last) and both roads' file sizes
-> profiles/container_deflate_10m.json.  No threshold: the yardstick is the host row of the same job.
One JSON object on stdout, also written to --out; the Markdown table on stderr and into DESIGN.md 14, between its two marker
lines (--design '' leaves the document alone; --from-json FILE rewrites the table from an earlier run's JSON without measuring).
"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SYNC = bytes(range(16))


def _zz(n: int) -> bytes:
    z = n << 1
    out = bytearray()
    while z >= 0x80:
        out.append((z & 0x7F) | 0x80)
        z >>= 7
    out.append(z)
    return bytes(out)


def container_of(schema: str, data, offsets, block_bytes: int, codec: str) -> tuple:
    """The packed records (payload + n + 1 offsets) as a container of blocks of about `block_bytes` -> (bytes, number of blocks)."""
    import numpy as np
    out = bytearray(b"Obj\x01" + _zz(2))
    for k, v in ((b"avro.schema", schema.encode()), (b"avro.codec", codec.encode())):
        out += _zz(len(k)) + k + _zz(len(v)) + v
    out += _zz(0) + SYNC
    n = len(offsets) - 1
    mv = memoryview(data)
    r0, nb = 0, 0
    while r0 < n:
        r1 = int(np.searchsorted(offsets, int(offsets[r0]) + block_bytes, side="right")) - 1
        r1 = min(max(r1, r0 + 1), n)
        payload = mv[int(offsets[r0]):int(offsets[r1])]
        if codec == "deflate":
            c = zlib.compressobj(1, zlib.DEFLATED, -15)
            payload = c.compress(payload) + c.flush()
        out += _zz(r1 - r0) + _zz(len(payload))
        out += payload
        out += SYNC
        r0 = r1
        nb += 1
    return bytes(out), nb


BEGIN, END = "<!-- container_bench: table -->", "<!-- container_bench: end -->"


def table(out: dict) -> str:
    lst = out["calls"]["list"]["wall_ms"]
    rows = ["| input | blocks | end to end ms (min - max) | vs list | split ms | split / end to end | size / scan / emit ms | inflate / upload / export ms |",
            "|---|---|---|---|---|---|---|---|"]
    for name, d in out["calls"].items():
        k = (f"{d['split_ms']:.2f} | {100 * d['split_share_of_wall']:.1f} % | {d['size_ms']:.2f} / {d['scan_ms']:.2f} / {d['emit_ms']:.2f} | "
             f"{d['inflate_ms']:.0f} / {d['upload_ms']:.0f} / {d['export_ms']:.0f}" if "split_ms" in d else "- | - | - | -")
        rows.append(f"| {name} | {d.get('blocks', '-')} | {d['wall_ms']:.0f} ({d['wall_ms_min']:.0f} - {d['wall_ms_max']:.0f}) | "
                    f"{d['wall_ms'] / lst:.2f} | {k} |")
    return "\n".join(rows)


def report(out: dict, design: str) -> None:
    """The Markdown table on stderr, and between the two marker lines of DESIGN.md 14."""
    t = table(out)
    print(t, file=sys.stderr)
    if design:
        text = open(design).read()
        i, j = text.index(BEGIN) + len(BEGIN), text.index(END)
        open(design, "w").write(text[:i] + "\n" + t + "\n" + text[j:])


def inflate_rows(a) -> int:
    """The two roads of a deflate container, alternated: the yardstick is the host row of the same job."""
    import numpy as np
    import torch  # noqa: F401  first: the engine shares torch's HIP runtime
    from avrogen import fastgen
    from avrogen.schemas import SCHEMAS
    import pyruhvro_amd as P
    from pyruhvro_amd import cabi

    t_start = time.perf_counter()

    def note(what):
        print(f"[{time.perf_counter() - t_start:6.1f} s] {what}", file=sys.stderr, flush=True)

    schema = SCHEMAS["full"]
    note(f"generating {a.records} records")
    data, offsets = fastgen.generate("full", a.records)
    reps = 3
    out = {"workload": "full", "records": a.records, "payload_bytes": int(offsets[-1]), "chunks": 8, "reps": reps, "codec": "deflate", "rows": {}}
    old = P.set_kernel_mode("specialized")
    for label, block_bytes in (("deflate_64k", 64 << 10), ("deflate_1m", 1 << 20)):
        note(f"{label}: deflating")
        blob, nb = container_of(schema, data, offsets, block_bytes, "deflate")
        note(f"{label}: {nb} blocks, {len(blob)} bytes")
        walls = {"host": [], "device": []}
        kern = []
        first = {}
        for rep in range(-1, reps):      # (rep -1: both roads once, warm, and compared)
            for road in ("host", "device"):
                t0 = time.perf_counter()
                b = P.read_container(blob, 8, inflate=road)
                ms = (time.perf_counter() - t0) * 1e3
                note(f"{label}: {road} {ms:.0f} ms")
                if rep < 0:
                    first[road] = b
                    continue
                del b
                walls[road].append(ms)
                if road == "device":
                    kern.append(dict(cabi.inflate_last(), split_ms=cabi.split_last_ms()))
                else:
                    kern.append({"host_split_ms": cabi.split_last_ms()})
            if rep < 0:
                assert all(x.equals(y) for x, y in zip(first["host"], first["device"])) and len(first["host"]) == len(first["device"])
                first.clear()
        row = {"blocks": nb, "file_bytes": len(blob)}
        for road in ("host", "device"):
            w = walls[road]
            row[road] = {"wall_ms": statistics.median(w), "wall_ms_min": min(w), "wall_ms_max": max(w)}
        dev = [k for k in kern if "size_ms" in k]
        row["host"]["split_ms"] = statistics.median(k["host_split_ms"] for k in kern if "host_split_ms" in k)
        row["device"].update({"inflate_size_kernel_ms": statistics.median(k["size_ms"] for k in dev),
                              "inflate_emit_kernel_ms": statistics.median(k["emit_ms"] for k in dev),
                              "split_ms": statistics.median(k["split_ms"] for k in dev),
                              "in_bytes": dev[0]["in_bytes"], "out_bytes": dev[0]["out_bytes"]})
        row["device_over_host"] = row["device"]["wall_ms"] / row["host"]["wall_ms"]
        out["rows"][label] = row
        del blob
    P.set_kernel_mode(old)
    note("done")
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    return 0


def deflate_rows(a) -> int:
    """The two roads of a deflate write, alternated: the yardstick is the host row of the same job."""
    import numpy as np
    import pyarrow as pa
    import torch  # noqa: F401  first: the engine shares torch's HIP runtime
    from avrogen import fastgen
    from avrogen.schemas import SCHEMAS
    import pyruhvro_amd as P
    from pyruhvro_amd import cabi

    t_start = time.perf_counter()

    def note(what):
        print(f"[{time.perf_counter() - t_start:6.1f} s] {what}", file=sys.stderr, flush=True)

    schema = SCHEMAS["full"]
    note(f"generating {a.records} records")
    data, offsets = fastgen.generate("full", a.records)
    old = P.set_kernel_mode("specialized")
    arr = pa.LargeBinaryArray.from_buffers(pa.large_binary(), a.records, [None, pa.py_buffer(offsets.view(np.int64)), pa.py_buffer(data)])
    batch = P.deserialize_binary_array(arr, schema, 1)[0]
    del arr, data
    note(f"one batch of {batch.num_rows} rows")
    reps = 3
    out = {"workload": "full", "records": a.records, "payload_bytes": int(offsets[-1]), "reps": reps, "codec": "deflate", "rows": {}}
    for block_rows in (512, 4096):
        label = f"block_rows_{block_rows}"
        walls = {"host": [], "device": []}
        kern, sizes = [], {}
        for rep in range(-1, reps):      # (rep -1: both roads once, warm, and read back)
            for road in ("host", "device"):
                t0 = time.perf_counter()
                blob = P.write_container(batch, schema, codec="deflate", block_rows=block_rows, sync=SYNC, deflate=road)
                ms = (time.perf_counter() - t0) * 1e3
                note(f"{label}: {road} {ms:.0f} ms, {len(blob)} bytes")
                if rep < 0:
                    sizes[road] = len(blob)
                    back = P.read_container(blob, 1, inflate="device")
                    assert len(back) == 1 and back[0].equals(batch), f"{label}: the {road} road's file does not read back"
                    del back
                else:
                    walls[road].append(ms)
                    if road == "device":
                        kern.append(cabi.deflate_last())
                del blob
        row = {"blocks": -(-a.records // block_rows)}
        for road in ("host", "device"):
            w = walls[road]
            row[road] = {"wall_ms": statistics.median(w), "wall_ms_min": min(w), "wall_ms_max": max(w), "file_bytes": sizes[road]}
        row["device"].update({"deflate_kernel_ms": statistics.median(k["deflate_ms"] for k in kern),
                              "gather_kernel_ms": statistics.median(k["gather_ms"] for k in kern),
                              "in_bytes": kern[0]["in_bytes"], "out_bytes": kern[0]["out_bytes"]})
        row["device_over_host"] = row["device"]["wall_ms"] / row["host"]["wall_ms"]
        row["device_file_over_host_file"] = sizes["device"] / sizes["host"]
        out["rows"][label] = row
    P.set_kernel_mode(old)
    note("done")
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    return 0


def tolerant_rows(a) -> int:
    """Strict, tolerant on the clean file, tolerant on the damaged file: alternated, the yardstick is the strict row of the same job."""
    import numpy as np
    import torch  # noqa: F401  first: the engine shares torch's HIP runtime
    from avrogen import fastgen
    from avrogen.schemas import SCHEMAS
    import pyruhvro_amd as P
    from pyruhvro_amd import cabi

    t_start = time.perf_counter()

    def note(what):
        print(f"[{time.perf_counter() - t_start:6.1f} s] {what}", file=sys.stderr, flush=True)

    schema = SCHEMAS["full"]
    note(f"generating {a.records} records")
    data, offsets = fastgen.generate("full", a.records)
    blob, nb = container_of(schema, data, offsets, 64 << 10, "null")
    del data
    info = P.container_info(blob)
    dirty = bytearray(blob)
    hit = list(range(50, nb, 100))                       # 1 % of the blocks
    for b in hit:
        mid = (int(info._start[b]) + int(info._end[b])) // 2
        dirty[mid:mid + 12] = b"\xff" * 12
    dirty = bytes(dirty)
    note(f"{nb} blocks, {len(blob)} bytes, {len(hit)} blocks damaged")
    reps = a.reps
    out = {"workload": "full", "records": a.records, "chunks": 8, "reps": reps, "codec": "null", "blocks": nb, "file_bytes": len(blob),
           "damaged_blocks": len(hit), "rows": {}}
    old = P.set_kernel_mode("specialized")
    calls = {"strict": lambda: (P.read_container(blob, 8), []),
             "tolerant_clean": lambda: P.read_container_tolerant(blob, 8),
             "tolerant_dirty": lambda: P.read_container_tolerant(dirty, 8, max_errors=nb)}
    walls = {k: [] for k in calls}
    last = {k: [] for k in calls}
    facts = {}
    for rep in range(-1, reps):                          # (rep -1: every read once, warm)
        for name, fn in calls.items():
            t0 = time.perf_counter()
            batches, errors = fn()
            ms = (time.perf_counter() - t0) * 1e3
            note(f"{name}: {ms:.0f} ms")
            if rep < 0:
                facts[name] = {"rows": sum(b.num_rows for b in batches), "errors": len(errors), "records_lost": sum(e.lost or 0 for e in errors)}
            else:
                walls[name].append(ms)
                last[name].append(dict(cabi.salvage_last(), split_last_ms=cabi.split_last_ms()))
            del batches, errors
    assert facts["tolerant_clean"] == {"rows": a.records, "errors": 0, "records_lost": 0}
    assert facts["tolerant_dirty"]["rows"] + facts["tolerant_dirty"]["records_lost"] == a.records
    for name in calls:
        w = walls[name]
        row = dict(facts[name], wall_ms=statistics.median(w), wall_ms_min=min(w), wall_ms_max=max(w))
        row["spread"] = (row["wall_ms_max"] - row["wall_ms_min"]) / row["wall_ms"]
        row["split_ms"] = statistics.median(k["split_last_ms"] for k in last[name])
        if name != "strict":
            row["gather_ms"] = statistics.median(k["gather_ms"] for k in last[name])
            row["bytes_gathered"] = last[name][0]["bytes_gathered"]
            row["blocks_reported"] = last[name][0]["blocks_reported"]
        out["rows"][name] = row
    for name in ("tolerant_clean", "tolerant_dirty"):
        out["rows"][name]["over_strict"] = out["rows"][name]["wall_ms"] / out["rows"]["strict"]["wall_ms"]
    P.set_kernel_mode(old)
    note("done")
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tolerant", action="store_true", help="the strict and the tolerant read of a clean and of a damaged file (see above); --out defaults to profiles/container_salvage_10m.json")
    ap.add_argument("--inflate", action="store_true", help="the host and the device road of a deflate file (see above); --out defaults to profiles/container_inflate_10m.json")
    ap.add_argument("--deflate", action="store_true", help="the host and the device road of a deflate write (see above); --out defaults to profiles/container_deflate_10m.json")
    ap.add_argument("--design", default=os.path.join(ROOT, "DESIGN.md"), help="the document whose table is rewritten ('' = none)")
    ap.add_argument("--from-json", default=None, help="no measurement: the table of an earlier run's JSON")
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "container_full10m.json"))
    a = ap.parse_args()
    if a.tolerant:
        if a.out == ap.get_default("out"):
            a.out = os.path.join(ROOT, "profiles", "container_salvage_10m.json")
        if a.reps == ap.get_default("reps"):
            a.reps = 5
        return tolerant_rows(a)
    if a.inflate:
        if a.out == ap.get_default("out"):
            a.out = os.path.join(ROOT, "profiles", "container_inflate_10m.json")
        return inflate_rows(a)
    if a.deflate:
        if a.out == ap.get_default("out"):
            a.out = os.path.join(ROOT, "profiles", "container_deflate_10m.json")
        return deflate_rows(a)
    if a.from_json:
        report(json.load(open(a.from_json)), a.design)
        return 0

    import numpy as np
    import pyarrow as pa
    import torch  # noqa: F401  first: the engine shares torch's HIP runtime
    from avrogen import fastgen
    from avrogen.schemas import SCHEMAS
    import pyruhvro_amd as P
    from pyruhvro_amd import cabi

    t_start = time.perf_counter()

    def note(what):      # progress on stderr: the 10M run is minutes of host work (generating, framing, deflating) between figures
        print(f"[{time.perf_counter() - t_start:6.1f} s] {what}", file=sys.stderr, flush=True)

    schema = SCHEMAS["full"]
    note(f"generating {a.records} records")
    data, offsets = fastgen.generate("full", a.records)
    out = {"workload": "full", "records": a.records, "payload_bytes": int(offsets[-1]), "chunks": 8, "reps": a.reps, "calls": {}}
    old = P.set_kernel_mode("specialized")

    def timed(fn, reps):
        for _ in range(2):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            b = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
            del b
        d = {"wall_ms": statistics.median(ts), "wall_ms_min": min(ts), "wall_ms_max": max(ts)}
        d["spread"] = (d["wall_ms_max"] - d["wall_ms_min"]) / d["wall_ms"]
        return d

    note("list")
    recs = fastgen.split(data, offsets)
    out["calls"]["list"] = timed(lambda: P.deserialize_array_threaded(recs, schema, 8), a.reps)
    del recs
    note("binary_array")
    arr = pa.LargeBinaryArray.from_buffers(pa.large_binary(), a.records, [None, pa.py_buffer(offsets.view(np.int64)), pa.py_buffer(data)])
    out["calls"]["binary_array"] = timed(lambda: P.deserialize_binary_array(arr, schema, 8), a.reps)
    del arr

    for label, block_bytes, codec, reps in (("null_64k", 64 << 10, "null", a.reps), ("null_1m", 1 << 20, "null", a.reps),
                                            ("deflate_64k", 64 << 10, "deflate", max(3, a.reps // 2))):
        note(label)
        blob, nb = container_of(schema, data, offsets, block_bytes, codec)
        note(f"{label}: {nb} blocks, {len(blob)} bytes")
        info = P.container_info(blob)
        assert (info.num_blocks, info.num_records) == (nb, a.records)
        buf = np.frombuffer(blob, dtype=np.uint8)

        def kernels():      # the blocks call alone, for the kernels' own times (the deflate file: its inflated blocks)
            from pyruhvro_amd import container as CT
            t0 = time.perf_counter()
            b, start, end = (CT._inflate(buf, info) if codec == "deflate" else (buf, info._start, info._end))
            inflate_ms = (time.perf_counter() - t0) * 1e3
            _, st = cabi.decode_blocks(b, start, end, info._first, schema, 8, kernel=cabi.KERNEL_SPECIALIZED, want_stats=True)
            return {"split_ms": cabi.split_last_ms(), "size_ms": st["size_kernel_ms"], "scan_ms": st["scan_kernel_ms"], "emit_ms": st["emit_kernel_ms"],
                    "inflate_ms": inflate_ms, "upload_ms": st["h2d_ms"], "export_ms": st["d2h_ms"], "blocks_call_ms": st["total_ms"]}
        d = timed(lambda: P.read_container(blob, 8), reps)
        ks = [kernels() for _ in range(3)]
        for key in ks[0]:
            d[key] = statistics.median(k[key] for k in ks)
        d.update({"blocks": nb, "file_bytes": len(blob), "vs_list": d["wall_ms"] / out["calls"]["list"]["wall_ms"],
                  "split_share_of_wall": d["split_ms"] / d["wall_ms"]})
        out["calls"][label] = d
        del blob, buf
    P.set_kernel_mode(old)
    note("done")

    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    report(out, a.design)
    return 0


if __name__ == "__main__":
    sys.exit(main())
