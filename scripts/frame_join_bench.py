"""The framed write against the road a user has today, in the SAME JOB (bench.py does not know framing).

    python scripts/frame_join_bench.py [--records 10000000] [--reps 3] [--out profiles/frame_join_10m.json]

`--records` records of the `full` workload as RecordBatches (8 per group), written as Confluent messages: one writer id, the rows
in order, and four ids dealt evenly with indices.  8 chunks, specialised kernels, one MI355X.  Timed, RecordBatches (in memory of
Arrow's own) in:
  serialize_framed   `serialize_framed(groups, 8)` -> BinaryArrays of finished messages; and the same plus `to_pylist()` of every
                     array, for a producer that wants one `bytes` per message
  python_road        what a user does today, in full: `serialize_record_batch` per batch of every group, one `header + bytes` per
                     message in Python, placement by the indices -> list[bytes]; and the same plus `pa.array` of the chunks
and beside them where the call's time goes: the encodes alone with the result left in HBM (`rh_encode_to_device`), the join alone
on those results (`rh_frame_join`, its copy to the host included), and the three stage times of the join's kernels
(`rh_frame_join_last`).  Every figure is the median of `--reps` calls after one warm call.  No ratio is asserted: the file is what
the prose quotes, whichever way it comes out.  One JSON object on stdout, also written to --out.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_join_10m.json"))
    a = ap.parse_args()

    import numpy as np
    import pyarrow as pa
    import torch  # noqa: F401  first: the engine shares torch's HIP runtime
    from avrogen import fastgen
    from avrogen.schemas import SCHEMAS
    import pyruhvro_amd as P
    from pyruhvro_amd import cabi

    schema = SCHEMAS["full"]
    n, k = a.records, 8
    out = {"workload": "full", "framing": "confluent", "records": n, "chunks": k, "batches_per_group": 8, "input_batches": "copies in Arrow-owned memory", "reps": a.reps, "warm_calls": 1,
           "kernel_key_full_encode": cabi.kernel_key(schema, True), "calls": {}}
    payloads = fastgen.split(*fastgen.generate("full", n))
    out["datum_bytes"] = sum(len(r) for r in payloads)
    old = P.set_kernel_mode("specialized")

    def timed(f):
        print("  timing ...", file=sys.stderr, flush=True)
        f()
        ts, last = [], None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            last = f()
            ts.append((time.perf_counter() - t0) * 1e3)
        return _med(ts), last

    def python_road(groups, as_arrays):      # serialize_record_batch per batch, header + bytes per message, placement by the indices
        msgs = [None] * n
        at = 0
        for wire, text, batches, idx in groups:
            head = b"\x00" + wire.to_bytes(4, "big")
            datums = [d for b in batches for arr in P.serialize_record_batch(b, text, k) for d in arr.to_pylist()]
            if idx is None:
                msgs[at:at + len(datums)] = [head + d for d in datums]
                at += len(datums)
            else:
                for p, d in zip(idx.tolist(), datums):
                    msgs[p] = head + d
        if not as_arrays:
            return len(msgs)
        sz = n // k
        return sum(len(pa.array(msgs[c * sz:(n if c == k - 1 else (c + 1) * sz)], type=pa.binary())) for c in range(k))

    for name, ids in (("one_id", [7]), ("four_ids", [7, 0x01000000, 0x7FFFFFFF, 0xFFFFFFF0])):
        m = len(ids)
        groups = []
        for j, wire in enumerate(ids):
            # the batches are copied into memory of Arrow's own, as a producer's are: batches that still live in the engine's pinned
            # result memory use up its budget (RUHVRO_HIP_PINNED_RESULT_MB), and the messages then come back through pageable memory
            batches = [pa.ipc.read_record_batch(b.serialize(), b.schema) for b in P.deserialize_array_threaded(payloads[j::m], schema, 8)]
            groups.append((wire, schema, batches, None if m == 1 else np.arange(j, n, m, dtype=np.int64)))
        d = {"ids": m, "indices": m > 1}
        print(name, file=sys.stderr, flush=True)
        d["serialize_framed"], rows = timed(lambda: sum(len(x) for x in P.serialize_framed(groups, k)))
        assert rows == n
        last = cabi.frame_join_last()
        d["kernels_ms"] = {"lengths": last["lengths_ms"], "scan": last["scan_ms"], "gather": last["gather_ms"]}
        d["serialize_framed_to_pylist"], rows = timed(lambda: sum(len(x.to_pylist()) for x in P.serialize_framed(groups, k)))
        assert rows == n
        d["python_road"], rows = timed(lambda: python_road(groups, False))
        assert rows == n
        d["python_road_to_arrays"], rows = timed(lambda: python_road(groups, True))
        assert rows == n
        # the two roads give the same messages (checked on the first and the last chunk)
        ours = P.serialize_framed(groups, k)
        heads = {j: b"\x00" + w.to_bytes(4, "big") for j, w in enumerate(ids)}
        for c, lo in ((0, 0), (k - 1, (k - 1) * (n // k))):
            got = ours[c].to_pylist()
            assert all(got[i] == heads[(lo + i) % m] + payloads[lo + i] for i in range(0, len(got), 997)), "the framed write differs from the road"
        d["message_bytes"] = sum(x.nbytes for x in ours) - 4 * (n + k)
        del ours

        # where the call's time goes: the encodes alone, then the join alone on their results
        def encodes():
            return [[cabi.encode_to_device(b, text, 1, kernel=cabi.KERNEL_SPECIALIZED) for b in batches] for _w, text, batches, _i in groups]

        def free(encs):
            for es in encs:
                for e in es:
                    e.free()
            return len(encs)
        d["encodes_to_device"], _ = timed(lambda: free(encodes()))
        encs = encodes()
        sources = []
        for (wire, _t, batches, idx), es in zip(groups, encs):
            at = 0
            for b, e in zip(batches, es):
                sources.append((e, 0, wire, None if idx is None else idx[at:at + b.num_rows]))
                at += b.num_rows

        def join():
            j = cabi.frame_join(sources, 0, n, k)
            rows = sum(len(x) for x in j.to_host())
            j.free()
            return rows
        d["join_and_copy_to_host"], rows = timed(join)
        assert rows == n

        def join_only():
            j = cabi.frame_join(sources, 0, n, k)
            c = j.chunks
            j.free()
            return c
        d["join_device_resident"], _ = timed(join_only)
        free(encs)
        del sources, encs, groups
        d["serialize_framed_vs_python_road"] = d["serialize_framed_to_pylist"]["ms"] / d["python_road"]["ms"]
        d["serialize_framed_vs_python_road_to_arrays"] = d["serialize_framed"]["ms"] / d["python_road_to_arrays"]["ms"]
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
