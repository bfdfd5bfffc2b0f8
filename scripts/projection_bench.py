"""Column projection against the full decode IN THE SAME RUN (bench.py does not know projections).

    python scripts/projection_bench.py [--records 10000000] [--reps 20] [--host-records 1000000,10000000] [--out profiles/projection_full10m.json]

Device-resident part: `--records` records of the `full` workload, 8 chunks, specialised kernels, warm; per call the kernels' own
HIP-event times (size, scan, emit: rh_stats) and the Arrow bytes produced, for the full decode and for three projections.
Host part: `deserialize_array_threaded` (list[bytes] in, RecordBatches out) for the full decode and two projections.
Every figure is the median of `--reps` calls; `spread` is (max - min) / median of the full decode's kernel time, the run-to-run
noise a projection's figure has to be read against.  A projection that is slower than the full decode beyond that spread
is a bug: the script says so and exits with status 1.  One JSON object on stdout, also written to --out.
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

PROJECTIONS = [None, ["created_at", "age"], ["name", "created_at", "class"], ["emails", "phone_numbers"]]
HOST_PROJECTIONS = [None, ["created_at", "age"], ["name", "created_at", "class"]]


def _label(cols):
    return "full" if cols is None else "+".join(cols)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-records", default="1000000,10000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "projection_full10m.json"))
    a = ap.parse_args()

    import numpy as np
    import torch  # first: the engine shares torch's HIP runtime
    from avrogen import fastgen
    from avrogen.schemas import SCHEMAS
    import pyruhvro_amd as P
    from pyruhvro_amd import cabi

    schema = SCHEMAS["full"]
    out = {"workload": "full", "records": a.records, "chunks": 8, "reps": a.reps, "kernel_key_full": cabi.kernel_key(schema), "device": {}, "host": {}}
    data, offsets = fastgen.generate("full", a.records)
    d_data = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda:0")
    d_data[: len(data)].copy_(torch.from_numpy(data))
    d_off = torch.from_numpy(offsets.view(np.int64)).to("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    bad = []
    for cols in PROJECTIONS:
        call = cabi.PreparedDeviceDecode(d_data.data_ptr(), d_off.data_ptr(), int(offsets[-1]), a.records, schema, 8, device=0, stream=stream,
                                         kernel=cabi.KERNEL_SPECIALIZED, columns=cols)
        for _ in range(3):                       # size history, kernels loaded
            call.free(call.run())
        rows = []
        nbytes = 0
        for _ in range(a.reps):
            h = call.run(want_stats=True)
            st = call.stats
            rows.append((st.size_kernel_ms, st.scan_kernel_ms, st.emit_kernel_ms))
            nbytes = call.output_bytes(h)
            call.free(h)
        tot = [sum(r) for r in rows]
        out["device"][_label(cols)] = {
            "size_ms": statistics.median(r[0] for r in rows), "scan_ms": statistics.median(r[1] for r in rows),
            "emit_ms": statistics.median(r[2] for r in rows), "kernels_ms": statistics.median(tot), "kernels_ms_min": min(tot),
            "kernels_ms_max": max(tot), "output_bytes": int(nbytes)}
    full = out["device"]["full"]
    spread = (full["kernels_ms_max"] - full["kernels_ms_min"]) / full["kernels_ms"]
    out["device_spread"] = spread
    for name, d in out["device"].items():
        d["vs_full"] = d["kernels_ms"] / full["kernels_ms"]
        if name != "full" and d["kernels_ms"] > full["kernels_ms"] * (1 + spread):
            bad.append(f"device {name}: {d['kernels_ms']:.3f} ms > full {full['kernels_ms']:.3f} ms")
    del d_data, d_off

    old = P.set_kernel_mode("specialized")
    for n in [int(x) for x in a.host_records.split(",") if x]:
        recs = fastgen.split(*fastgen.generate("full", n)) if n != a.records else fastgen.split(data, offsets)
        res = {}
        for cols in HOST_PROJECTIONS:
            for _ in range(2):
                P.deserialize_array_threaded(recs, schema, 8, columns=cols)
            ts = []
            for _ in range(max(5, a.reps if n <= 1_000_000 else a.reps // 2)):
                t0 = time.perf_counter()
                b = P.deserialize_array_threaded(recs, schema, 8, columns=cols)
                ts.append((time.perf_counter() - t0) * 1e3)
                del b
            res[_label(cols)] = {"wall_ms": statistics.median(ts), "wall_ms_min": min(ts), "wall_ms_max": max(ts)}
        f = res["full"]
        hs = (f["wall_ms_max"] - f["wall_ms_min"]) / f["wall_ms"]
        for name, d in res.items():
            d["vs_full"] = d["wall_ms"] / f["wall_ms"]
            if name != "full" and d["wall_ms"] > f["wall_ms"] * (1 + hs):
                bad.append(f"host {n} {name}: {d['wall_ms']:.2f} ms > full {f['wall_ms']:.2f} ms")
        out["host"][str(n)] = {"spread": hs, "calls": res}
        del recs
    P.set_kernel_mode(old)
    out["slower_than_full"] = bad
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
