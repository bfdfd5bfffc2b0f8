"""Framed messages against the two yardsticks of the SAME JOB (bench.py does not know framing).

    python scripts/frame_bench.py [--records 10000000] [--reps 3] [--out profiles/frame_10m.json]

`--records` records of the `full` workload behind Confluent headers, one writer id and four ids dealt evenly, 8 chunks, specialised
kernels, one MI355X.  Timed, list[bytes] in and RecordBatches out:
  framed          `deserialize_framed(messages, {id: schema, ...}, 8)`
  unframed        `deserialize_array_threaded(payloads, schema, 8)` on the pre-stripped payloads, the stripping not counted
  python_road     what a user does today, in full: slice every message, read and group the ids, one call per group
and beside them where the framed call's time goes: packing the list in Python, the split alone on the packed list (the one-piece
upload and the four kernels), the split alone on device-resident input, and the kernels' own times (`rh_frame_last`).
Every figure is the median of `--reps` calls after one warm call.  No ratio is asserted: the file is what the prose quotes,
whichever way it comes out.  One JSON object on stdout, also written to --out.
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


def _med(xs):
    return {"ms": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_10m.json"))
    a = ap.parse_args()

    import numpy as np
    import torch  # first: the engine shares torch's HIP runtime
    from avrogen import fastgen
    from avrogen.schemas import SCHEMAS
    import pyruhvro_amd as P
    from pyruhvro_amd import cabi

    schema = SCHEMAS["full"]
    n = a.records
    out = {"workload": "full", "framing": "confluent", "records": n, "chunks": 8, "reps": a.reps, "warm_calls": 1,
           "kernel_key_full": cabi.kernel_key(schema), "calls": {}}
    payloads = fastgen.split(*fastgen.generate("full", n))
    out["payload_bytes"] = sum(len(r) for r in payloads)
    old = P.set_kernel_mode("specialized")

    def timed(f):
        f()
        ts, rows = [], 0
        for _ in range(a.reps):
            t0 = time.perf_counter()
            b = f()
            ts.append((time.perf_counter() - t0) * 1e3)
            rows = b
        return _med(ts), rows

    def rows_of(batches):
        return sum(x.num_rows for x in batches)

    out["calls"]["unframed"], rows = timed(lambda: rows_of(P.deserialize_array_threaded(payloads, schema, 8)))
    assert rows == n

    def python_road(msgs):      # slice, read and group the ids, one call per group, the row indices kept
        stripped = [m[5:] for m in msgs]
        groups = {}
        for i, m in enumerate(msgs):
            groups.setdefault(int.from_bytes(m[1:5], "big"), []).append(i)
        total = 0
        for wire in sorted(groups):
            idx = groups[wire]
            recs = stripped if len(idx) == len(msgs) else [stripped[i] for i in idx]
            total += rows_of(P.deserialize_array_threaded(recs, schema, 8))
        return total

    for name, ids in (("one_id", [7]), ("four_ids", [7, 0x01000000, 0x7FFFFFFF, 0xFFFFFFF0])):
        heads = [b"\x00" + w.to_bytes(4, "big") for w in ids]
        msgs = [heads[i % len(ids)] + r for i, r in enumerate(payloads)]
        schemas = {w: schema for w in ids}
        d = {"ids": len(ids)}
        d["framed"], rows = timed(lambda: sum(rows_of(g.batches) for g in P.deserialize_framed(msgs, schemas, 8).groups))
        assert rows == n
        last = cabi.frame_last()
        d["kernels_ms"] = {"classify": last["classify_ms"], "scan_offsets": last["scan_offsets_ms"], "gather": last["gather_ms"]}
        d["python_road"], rows = timed(lambda: python_road(msgs))
        assert rows == n
        # where the framed call's time goes
        d["pack_in_python"], _ = timed(lambda: len(P._pack_records(msgs)[1]))
        data, offs = P._pack_records(msgs)
        d["message_bytes"] = int(offs[-1])

        def split_packed():
            sp = cabi.FrameSplit.packed(data, offs, sorted(ids), 0)
            c = sp.count(0)
            sp.free()
            return c
        d["split_of_the_packed_list"], _ = timed(split_packed)
        d_data = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda:0")
        d_data[: len(data)].copy_(torch.from_numpy(data))
        d_off = torch.from_numpy(offs.view(np.int64)).to("cuda:0")
        torch.cuda.synchronize()

        def split_device():
            sp = cabi.FrameSplit.device(d_data.data_ptr(), d_off.data_ptr(), int(offs[-1]), n, sorted(ids), 0, device=0)
            c = sp.count(0)
            sp.free()
            return c
        d["split_device_resident"], _ = timed(split_device)
        last = cabi.frame_last()
        d["kernels_device_resident_ms"] = {"classify": last["classify_ms"], "scan_offsets": last["scan_offsets_ms"], "gather": last["gather_ms"]}
        del d_data, d_off, data, offs, msgs
        torch.cuda.empty_cache()
        d["framed_vs_unframed"] = d["framed"]["ms"] / out["calls"]["unframed"]["ms"]
        d["framed_vs_python_road"] = d["framed"]["ms"] / d["python_road"]["ms"]
        out["calls"][name] = d
    P.set_kernel_mode(old)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
