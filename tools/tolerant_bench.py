"""Tolerant decode next to the strict decode IN THE SAME RUN (bench.py does not know the tolerant entry points).

    python tools/tolerant_bench.py [--records 10000000] [--reps 10] [--out profiles/tolerant_decode.txt]

Device-resident `full` workload, 8 chunks, specialised kernels, warm.  Wall time per call (the calls are synchronous), median of
--reps: the strict call and the tolerant call on clean input (the same kernels: the criterion is that the engine counters move
alike, the two times are recorded without a threshold), then the same input with 10 and with 1,000 truncated records: the
validation alone (rh_validate_device: the validation kernel and the read-back of its list), the whole tolerant call, and the
strict call that fails -- the gather and the second decode are what is left of the total."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tolerant_decode.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch  # first: the engine shares torch's HIP runtime
    from avrogen import fastgen
    from avrogen.schemas import SCHEMAS
    from pyruhvro_amd import cabi

    schema, n = SCHEMAS["full"], a.records
    data, offsets = fastgen.generate("full", n)
    lines = [f"tolerant decode, `full` workload, {n} records, 8 chunks, device-resident, specialised kernels, kernel key {cabi.kernel_key(schema)}",
             f"wall ms per synchronous call: median (min .. max) of {a.reps}"]

    def upload(dat, offs):
        d = torch.zeros(len(dat) + 64, dtype=torch.uint8, device="cuda:0")
        d[: len(dat)].copy_(torch.from_numpy(np.ascontiguousarray(dat)))
        return d, torch.from_numpy(offs.view(np.int64).copy()).to("cuda:0")

    def calls(d, o, end):
        args = (d.data_ptr(), o.data_ptr(), end, n, schema, 8)
        kw = dict(device=0, kernel=cabi.KERNEL_SPECIALIZED, want_stats=False)
        return (lambda: cabi.decode_device(*args, **kw).free(), lambda: cabi.decode_device_tolerant(*args, **kw).free(),
                lambda: cabi.validate_device(d.data_ptr(), o.data_ptr(), end, n, schema, max_errors=4096, device=0))

    d, o = upload(data, offsets)
    strict, tolerant, validate = calls(d, o, int(offsets[-1]))
    for _ in range(3):
        strict()
    c0 = cabi.engine_counters(); strict(); c1 = cabi.engine_counters(); tolerant(); c2 = cabi.engine_counters()
    same = all(c1[k] - c0[k] == c2[k] - c1[k] for k in c0 if not k.startswith("tolerant"))
    lines.append("clean  strict    %.3f (%.3f .. %.3f)" % _median_ms(strict, a.reps))
    lines.append("clean  tolerant  %.3f (%.3f .. %.3f)   engine counters move as the strict call's: %s" % (*_median_ms(tolerant, a.reps), same))
    lines.append("clean  validate  %.3f (%.3f .. %.3f)   (validation alone, 0 malformed records)" % _median_ms(validate, a.reps))
    for nbad in (10, 1000):
        lens = np.diff(offsets).astype(np.int64)
        keep = lens.copy()
        bad = np.linspace(0, n - 1, nbad).astype(np.int64)
        keep[bad] = lens[bad] // 2                       # cut in the middle
        idx = np.repeat(offsets[:-1].astype(np.int64), keep) + (np.arange(int(keep.sum())) - np.repeat(np.cumsum(keep) - keep, keep))
        offs2 = np.concatenate([[0], np.cumsum(keep)]).astype(np.uint64)
        d2, o2 = upload(data[idx], offs2)
        strict2, tolerant2, validate2 = calls(d2, o2, int(offs2[-1]))
        found = len(validate2())

        def failing():
            try:
                strict2()
            except ValueError:
                pass
        lines.append(f"dirty {nbad:5d} cut records ({found} malformed):")
        lines.append("       strict (fails)  %.3f (%.3f .. %.3f)" % _median_ms(failing, a.reps))
        lines.append("       validate        %.3f (%.3f .. %.3f)" % _median_ms(validate2, a.reps))
        lines.append("       tolerant total  %.3f (%.3f .. %.3f)   (failing strict call + validation + gather + second strict call)" % _median_ms(tolerant2, a.reps))
        del d2, o2
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
