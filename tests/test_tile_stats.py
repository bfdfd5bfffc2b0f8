"""The call's tile statistics (rh_engine_counters: tiles, careful_tiles, over_window_tiles, subtiled_tiles, rewalked_waves) are
summed on the device by the scan launch (kernels.hip tile_stats_commit): workgroup (counter, chunk) of rh_k_scan_layout takes a
1/K slice of its chunk's tile flags; a call that has a size pass and nothing to scan (K == 0) gets rh_k_tile_stats.  Every
expected value below follows from the input -- the offsets array, or the positions of the records that leave the fast wire
forms -- never from a run of the engine, and every buffer of every case is compared with the oracle."""
import numpy as np
import pytest

import cases
from arrow_compare import assert_batches_identical
from avrogen import fastgen
from avrogen.schemas import SCHEMAS
from oracle import c_walker

import pyruhvro_amd as P
from pyruhvro_amd import cabi

KERNELS = {"generic": cabi.KERNEL_GENERIC, "specialized": cabi.KERNEL_SPECIALIZED}
STATS = ("tiles", "careful_tiles", "over_window_tiles", "subtiled_tiles", "rewalked_waves")
T = 256            # records per tile of both kernel forms (program.h kBlock; none of the schemas below is wide)
WIN = 8192


@pytest.fixture(params=sorted(KERNELS))
def kernel(request):
    old = P.set_kernel_mode(request.param)
    yield KERNELS[request.param]
    P.set_kernel_mode(old)


def _geometry(n, k):
    """(first record, records) of every tile of a call of n records in k chunks, in tile order: chunks of n // k rows, the last
    one takes the rest; the tiles of a chunk start at the chunk's first record."""
    k = max(1, min(k, n))
    sz = n // k
    out = []
    for c in range(k):
        r0 = c * sz
        rows = sz if c < k - 1 else n - (k - 1) * sz
        for t0 in range(0, rows, T):
            out.append((r0 + t0, min(T, rows - t0)))
    return out


def _over_window(offsets, n, k, win=WIN):
    o = offsets.astype(np.int64)
    return sum(1 for r0, m in _geometry(n, k) if int(o[r0 + m]) - (int(o[r0]) & ~15) > win)


def _upload(data, offsets):
    import torch
    d_data = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda:0")
    d_data[: len(data)].copy_(torch.from_numpy(data.copy()))
    d_off = torch.from_numpy(offsets.view(np.int64).copy()).to("cuda:0")
    return d_data, d_off


def _device_calls(dev, offsets, schema, k, kernel, exp, calls, columns=None):
    """`calls` decodes of the same device-resident input -> the counter deltas of each.  Every call's buffers are the oracle's.
    (A schema's first call takes two submissions and counts no statistics: callers look at the later ones.)"""
    import torch
    d_data, d_off = dev
    n = len(offsets) - 1
    deltas = []
    for _ in range(calls):
        c0 = cabi.engine_counters()
        r = cabi.decode_device(d_data.data_ptr(), d_off.data_ptr(), int(offsets[-1]), n, schema, k, device=0,
                               stream=torch.cuda.current_stream().cuda_stream, kernel=kernel, columns=columns)
        got = r.to_host()
        r.free()
        c1 = cabi.engine_counters()
        assert len(got) == len(exp)
        for g, e in zip(got, exp):
            assert_batches_identical(g, e)
        deltas.append({key: c1[key] - c0[key] for key in c1})
    return deltas


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 8])
def test_friendly_records_count_tiles_and_nothing_else(k, kernel):
    n = 100_003
    data, offsets = fastgen.generate("full", n)
    exp = c_walker.decode_packed(c_walker.CompiledSchema(SCHEMAS["full"]), data, offsets, k, threaded=True)
    deltas = _device_calls(_upload(data, offsets), offsets, SCHEMAS["full"], k, kernel, exp, 3)
    for d in deltas[1:]:
        print("friendly", k, {s: d[s] for s in STATS})
        assert d["tiles"] == len(_geometry(n, k))
        assert d["careful_tiles"] == 0 and d["over_window_tiles"] == 0 and d["subtiled_tiles"] == 0 and d["rewalked_waves"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3, 8])
def test_tiles_past_the_window_are_counted_exactly_once(k, kernel, monkeypatch):
    """Skewed record sizes, an 8 KiB window, a record count that is no multiple of the tile size (the last chunk is short and
    ends in a ragged tile): the slices of the K x k scan workgroups cover every tile once."""
    monkeypatch.setenv("RUHVRO_HIP_WIN_BYTES", str(WIN))
    monkeypatch.setenv("RUHVRO_HIP_RANGED", "1")
    n = 60_013
    data, offsets = fastgen.generate("full_skewed", n)
    want = _over_window(offsets, n, k)
    assert want > 0                                    # (records of ~400 bytes: in fact every tile is past an 8 KiB window)
    exp = c_walker.decode_packed(c_walker.CompiledSchema(SCHEMAS["full_skewed"]), data, offsets, k, threaded=True)
    deltas = _device_calls(_upload(data, offsets), offsets, SCHEMAS["full_skewed"], k, kernel, exp, 3)
    for d in deltas[1:]:
        print("over-window", k, "expected", want, {s: d[s] for s in STATS})
        assert d["tiles"] == len(_geometry(n, k))
        assert d["over_window_tiles"] == want
        if kernel == cabi.KERNEL_SPECIALIZED:
            assert d["subtiled_tiles"] == want


def _varint(z, width=0):
    b = bytearray()
    while True:
        more = (z >> 7) != 0 or len(b) + 1 < width
        b.append((z & 0x7F) | (0x80 if more else 0))
        z >>= 7
        if not more:
            return bytes(b)


def _zz(v):
    return _varint(((v << 1) ^ (v >> 63)) & ((1 << 64) - 1))


def _padded_schema():
    return [c for c in cases.wide_form_cases() if c[0] == "padded_at_form_widths"][0][1]


def _small_record(r, text=b"abc", len_width=1):
    """A record of _padded_schema(): ~20 bytes, every varint inside the fast wire forms unless len_width says otherwise."""
    out = b"\x02" + _zz(r * 77 - 4000) + b"\x02" + _zz((r - 100) * (1 << 33))
    out += b"\x02" + _varint(2 * len(text), len_width) + text
    out += _zz(2) + _zz(r & 63) + _zz(-(r & 63)) + _zz(0)
    return out + _zz(r % 3)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3, 8])
def test_a_mix_of_tiles_inside_and_past_the_window(k, kernel, monkeypatch):
    """Long-string records: tiles of ~5 KB fit the 8 KiB window, a 9,000-byte string every 1,700 records puts its tile past it."""
    monkeypatch.setenv("RUHVRO_HIP_WIN_BYTES", str(WIN))
    monkeypatch.setenv("RUHVRO_HIP_RANGED", "1")
    schema = _padded_schema()
    n = 20_011
    recs = [_small_record(r, b"L" * 9000 if r % 1700 == 5 else b"abc") for r in range(n)]
    data, offsets = c_walker.pack(recs)
    want = _over_window(offsets, n, k)
    assert 0 < want < len(_geometry(n, k)) // 4          # (a mix: most tiles fit the window)
    exp = c_walker.decode_threaded(recs, schema, k)
    deltas = _device_calls(_upload(data, offsets), offsets, schema, k, kernel, exp, 3)
    for d in deltas[1:]:
        print("mix", k, "expected", want, {s: d[s] for s in STATS})
        assert d["tiles"] == len(_geometry(n, k))
        assert d["over_window_tiles"] == want
        if kernel == cabi.KERNEL_SPECIALIZED:
            assert d["subtiled_tiles"] == want


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3])
def test_rewalked_wavefronts_are_counted_where_the_records_are(k, kernel):
    """The schema of cases.wide_form_cases()'s padded records.  Every record stays inside the fast wire forms except a handful
    whose string length is a FOUR-byte varint (the form reads three): the wavefront of such a record is walked twice and its
    tile takes the careful emit walk.  Expected: the distinct (tile, wavefront) and the distinct tiles of those records."""
    schema = _padded_schema()
    n = 20_011
    beyond = {70, 75, 130, 131, 2_400, 6_700, 6_763, 6_764, 13_400, 19_999, 20_010}
    recs = [_small_record(r, len_width=4 if r in beyond else 1) for r in range(n)]
    data, offsets = c_walker.pack(recs)
    kk = max(1, min(k, n))
    sz = n // kk
    waves, tiles = set(), set()
    for r in beyond:
        c = min(r // sz, kk - 1)
        rr = r - c * sz
        tiles.add((c, rr // T))
        waves.add((c, rr // T, (rr % T) // 64))
    exp = c_walker.decode_threaded(recs, schema, k)
    deltas = _device_calls(_upload(data, offsets), offsets, schema, k, kernel, exp, 3)
    for d in deltas[1:]:
        print("re-walk", k, "expected", len(waves), len(tiles), {s: d[s] for s in STATS})
        assert d["tiles"] == len(_geometry(n, k))
        assert d["rewalked_waves"] == len(waves)
        assert d["careful_tiles"] == len(tiles)
        assert d["over_window_tiles"] == 0 and d["subtiled_tiles"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 5])
def test_a_size_pass_with_nothing_to_scan(k, kernel, monkeypatch):
    """Fixed-width columns only of a schema with strings: no counter (K == 0), so no scan launch, but the size pass stays and
    meets tiles past the window: rh_k_tile_stats sums their flags."""
    monkeypatch.setenv("RUHVRO_HIP_WIN_BYTES", str(WIN))
    monkeypatch.setenv("RUHVRO_HIP_RANGED", "1")
    cols = ["created_at", "age"]
    n = 300_011                                          # (1,172 tiles: two reduction workgroups when k == 1)
    data, offsets = fastgen.generate("full_skewed", n)
    want = _over_window(offsets, n, k)
    assert want > 0
    full = c_walker.decode_packed(c_walker.CompiledSchema(SCHEMAS["full_skewed"]), data, offsets, k, threaded=True)
    exp = [b.select(cols) for b in full]
    deltas = _device_calls(_upload(data, offsets), offsets, SCHEMAS["full_skewed"], k, kernel, exp, 3, columns=cols)
    for d in deltas[1:]:
        print("K == 0", k, "expected", want, {s: d[s] for s in STATS})
        assert d["tiles"] == len(_geometry(n, k))
        assert d["over_window_tiles"] == want
        if kernel == cabi.KERNEL_SPECIALIZED:
            assert d["subtiled_tiles"] == want


@pytest.mark.gpu
def test_a_refused_attempt_counts_nothing(monkeypatch):
    """RUHVRO_HIP_RANGED=0, AUTO kernels, tiles past the window: the specialised size kernel refuses every call (LF_NEED_RANGED)
    and leaves the flag words of those tiles unwritten; the engine repeats the call on the generic kernels.  The counters advance
    by the generic run's values alone -- its tiles, the over-window tiles the offsets give, no sub-tiled tile (the generic kernels
    have no ranges) -- and by the same amount for every call."""
    monkeypatch.setenv("RUHVRO_HIP_RANGED", "0")
    monkeypatch.setenv("RUHVRO_HIP_WIN_BYTES", str(WIN))
    old = P.set_kernel_mode("auto")
    try:
        n, k = 60_013, 4
        data, offsets = fastgen.generate("full_skewed", n)
        cabi.prebuild(SCHEMAS["full_skewed"])
        want = _over_window(offsets, n, k)
        assert want > 0
        exp = c_walker.decode_packed(c_walker.CompiledSchema(SCHEMAS["full_skewed"]), data, offsets, k, threaded=True)
        deltas = _device_calls(_upload(data, offsets), offsets, SCHEMAS["full_skewed"], k, cabi.KERNEL_AUTO, exp, 4)
        for d in deltas[1:]:
            print("refused", "expected", want, {s: d[s] for s in STATS}, "retries", d["ranged_retries"])
            assert d["ranged_retries"] == 1
            assert d["tiles"] == len(_geometry(n, k))
            assert d["over_window_tiles"] == want
            assert d["subtiled_tiles"] == 0
        assert {s: deltas[2][s] for s in STATS} == {s: deltas[1][s] for s in STATS} == {s: deltas[3][s] for s in STATS}
        two = {s: deltas[2][s] + deltas[3][s] for s in STATS}
        assert two == {s: 2 * deltas[1][s] for s in STATS}
    finally:
        P.set_kernel_mode(old)
