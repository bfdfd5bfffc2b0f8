"""Reader schemas against the plain writer decode IN THE SAME RUN (bench.py does not know reader schemas).

    python scripts/resolution_bench.py [--records 10000000] [--reps 20] [--out profiles/resolution_full10m.json]

`--records` records of the `full` workload, 8 chunks, device-resident, specialised kernels, warm; per call the kernels' own
HIP-event times (size, scan, emit: rh_stats) and the Arrow bytes produced, for the plain decode and three resolved decodes:
  promote       age int -> long, created_at long -> double; nothing dropped or added
  drop          the reader lacks `emails` and `preferences`
  promote+add   `promote` plus two added fields (a nullable long defaulting to null, a string defaulting to "unknown")
Every figure is the median of `--reps` calls; `spread` is (max - min) / median of the plain decode's kernel time, the run-to-run
noise a resolved figure has to be read against.  No threshold: the figures are reported, DESIGN.md 13 discusses them.
One JSON object on stdout, also written to --out.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from avrogen.schemas import SCHEMAS  # noqa: E402

WRITER = SCHEMAS["full"]


def readers() -> dict:
    def promoted():
        j = json.loads(WRITER)
        for f in j["fields"]:
            if f["name"] == "age":
                f["type"] = ["null", "long"]
            if f["name"] == "created_at":
                f["type"] = "double"
        return j
    a = promoted()
    b = json.loads(WRITER)
    b["fields"] = [f for f in b["fields"] if f["name"] not in ("emails", "preferences")]
    c = promoted()
    c["fields"] += [{"name": "score", "type": ["null", "long"], "default": None}, {"name": "source", "type": "string", "default": "unknown"}]
    return {"promote": json.dumps(a), "drop": json.dumps(b), "promote+add": json.dumps(c)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resolution_full10m.json"))
    a = ap.parse_args()

    import numpy as np
    import torch  # first: the engine shares torch's HIP runtime
    from avrogen import fastgen
    from pyruhvro_amd import cabi

    out = {"workload": "full", "records": a.records, "chunks": 8, "reps": a.reps, "kernel_key_full": cabi.kernel_key(WRITER), "device": {}}
    data, offsets = fastgen.generate("full", a.records)
    d_data = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda:0")
    d_data[: len(data)].copy_(torch.from_numpy(data))
    d_off = torch.from_numpy(offsets.view(np.int64)).to("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    for name, reader in [("plain", None)] + list(readers().items()):
        call = cabi.PreparedDeviceDecode(d_data.data_ptr(), d_off.data_ptr(), int(offsets[-1]), a.records, WRITER, 8, device=0, stream=stream,
                                         kernel=cabi.KERNEL_SPECIALIZED, reader_schema=reader)
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
        out["device"][name] = {
            "size_ms": statistics.median(r[0] for r in rows), "scan_ms": statistics.median(r[1] for r in rows),
            "emit_ms": statistics.median(r[2] for r in rows), "kernels_ms": statistics.median(tot), "kernels_ms_min": min(tot),
            "kernels_ms_max": max(tot), "output_bytes": int(nbytes)}
    plain = out["device"]["plain"]
    out["device_spread"] = (plain["kernels_ms_max"] - plain["kernels_ms_min"]) / plain["kernels_ms"]
    for d in out["device"].values():
        d["vs_plain"] = d["kernels_ms"] / plain["kernels_ms"]
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
