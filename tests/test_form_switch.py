"""AUTO kernels and tiles past the LDS window: the hand-overs between the kernel forms.

A call in the default kernel mode starts on the specialised size / emit kernels.  They stage a tile's bytes in an LDS window sized
from the call's MEAN record (8,192 bytes at least); a tile that does not fit is the ranged pair's (rh_spec_size_r /
rh_spec_emit_r), which AUTO launches only when the schema's history says so.  Without the pair such a tile is
  * K > 0 (variable-length output: a size pass runs): refused by the size kernel (LF_NEED_RANGED), the call repeated on the generic
    kernels (ranged_retries);
  * K == 0 (fixed-width columns only: no size pass): walked from global memory by the emit kernel itself, which counts it
    (over_window_tiles), so that the schema's next calls launch the pair.
The inputs (cases.form_switch_cases) go past the window with no test hook: a run of 768 large records between small ones.  Every
result is compared buffer for buffer with oracle.c_walker, every error message with the oracle's; no result is compared with
another result of the engine.  Every test proves through rh_engine_counters that the call took the road it aims at, and -- AUTO
runs a schema whose kernels are not loaded on the generic ones -- that it started on the specialised kernels: a first call on
small records reports `specialized == 1`, or the call counts a ranged retry, which only the specialised size kernel raises."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
from arrow_compare import assert_batches_identical
from avrogen import fastgen, synth
from avrogen.schemas import SCHEMAS
from oracle import c_walker, py_walker
from test_tile_stats import T, _geometry, _over_window, _upload

import pyruhvro_amd as P
from pyruhvro_amd import cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"auto": cabi.KERNEL_AUTO, "specialized": cabi.KERNEL_SPECIALIZED, "generic": cabi.KERNEL_GENERIC}
KS = (1, 3, 7)
MIN_WIN = 8192


def _case(name, tag=""):
    for c in cases.form_switch_cases(tag):
        if c[0] == name:
            return c[1], c[2]
    raise KeyError(name)


def _small(kind):
    """Sound records of the case outside its run of large ones: every tile of them fits the smallest window."""
    lo, hi = cases.BIG_RUN[kind]
    return _case(kind)[1][hi + 232: hi + 232 + 4000]


def _window(offsets):
    """The LDS window of an unsplit call on this input: max(8192, mean * 256 * 1.15 + 2048), the mean rounded as the engine does."""
    n = len(offsets) - 1
    avg = int(offsets[-1]) // n + 1
    return max(MIN_WIN, (avg * T * 115 // 100 + 2048 + 15) & ~15)


def _delta(c0, c1=None):
    c1 = c1 or cabi.engine_counters()
    return {key: c1[key] - c0[key] for key in c1}


def _same(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        g.validate(full=True)
        assert_batches_identical(g, e)


def _oracle_error(recs, schema, k):
    with pytest.raises(ValueError) as e:
        c_walker.decode_threaded(recs, schema, k)
    return str(e.value)


def _starts_specialised(kind, schema, surface="cabi"):
    """The kernels are in the cache (prebuild) and a call on small records alone runs on them: the AUTO call that follows starts on
    the specialised kernels, with a size history (a single-submission call) and no history of tiles past the window."""
    cabi.prebuild(schema)
    small = _small(kind)
    exp = c_walker.decode_threaded(small, schema, 2)
    c0 = cabi.engine_counters()
    if surface == "python":
        old = P.set_kernel_mode("auto")
        try:
            got, st = P.deserialize_array_threaded_with_stats(small, schema, 2)
        finally:
            P.set_kernel_mode(old)
    else:
        data, offsets = c_walker.pack(small)
        got, st = cabi.decode_packed(data, offsets, schema, 2, want_stats=True, kernel=cabi.KERNEL_AUTO)
    _same(got, exp)
    d = _delta(c0)
    assert st["specialized"] == 1, st
    assert d["ranged_retries"] == 0 and d["over_window_tiles"] == 0, d


def _device_call(dev, offsets, schema, k, mode, **kw):
    import torch
    d_data, d_off = dev
    return cabi.decode_device(d_data.data_ptr(), d_off.data_ptr(), int(offsets[-1]), len(offsets) - 1, schema, k, device=0,
                              stream=torch.cuda.current_stream().cuda_stream, kernel=mode, **kw)


# ---- CPU: the inputs are what the tests say they are ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.form_switch_cases(), ids=lambda c: c[0])
def test_the_inputs_go_past_the_smallest_window_and_the_oracles_agree(case):
    """From the packed offsets, 256-record tiles from every chunk start for every k the GPU tests use: at least two tiles exceed
    8,192 bytes; for longs8 and id_str the mean record keeps the window AT 8,192 bytes (mean * 256 * 1.15 + 2048 < 8192; the
    nullable form stays below it as well).  Both oracles give the same batches -- or the same message for the damaged lists."""
    name, schema, recs = case
    offsets = np.zeros(len(recs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in recs])
    n = len(recs)
    for k in KS + (2, 4):
        assert _over_window(offsets, n, k, MIN_WIN) >= 2, (name, k)
    mean = int(offsets[-1]) / n
    print(name, "records", n, "mean", round(mean, 2), "window", _window(offsets), "tiles past it (k = 1)", _over_window(offsets, n, 1, MIN_WIN))
    if name in ("longs8", "id_str"):
        assert mean * 256 * 1.15 + 2048 < MIN_WIN
    assert _window(offsets) == MIN_WIN
    if "_damaged" in name:
        kind = name[: name.index("_damaged")]
        with pytest.raises(ValueError) as a:
            c_walker.decode(recs, schema)
        with pytest.raises(ValueError) as b:
            py_walker.decode(recs, schema)
        assert str(a.value) == str(b.value)
        low = 100 if kind == "id_str" else 5300
        sound = list(_case(kind)[1])
        sound[low] = recs[low]                              # the lower malformed record alone: the same message
        with pytest.raises(ValueError) as c:
            c_walker.decode(sound, schema)
        assert str(c.value) == str(a.value)
        high = 3000 if kind == "id_str" else 9000
        sound = list(_case(kind)[1])
        sound[high] = recs[high]
        with pytest.raises(ValueError) as d:
            c_walker.decode(sound, schema)
        # ... and the higher one's is another, so that a test can tell which record was reported -- except for the two CUT records
        # of longs8_damaged (a long column has one message for every cut): longs8_damaged_apart is there for that
        assert (str(d.value) != str(a.value)) == (name != "longs8_damaged"), (str(d.value), str(a.value))
    else:
        assert_batches_identical(c_walker.decode(recs, schema), py_walker.decode(recs, schema))


# ---- 1. K == 0 past the window ---------------------------------------------------------------------------------------------------
def _k_zero_calls(kind, mode_name, k, tag, monkeypatch):
    """Every entry point on one K == 0 case.  The three roads -- device-resident calls, asynchronous ones, host calls -- decode
    schema objects of their own (tag, tag + "a", tag + "h"), so that in AUTO each of them makes the call that has no history of
    tiles past the window (the emit kernel walks them itself) AND the calls behind it (the history launches the ranged pair,
    which is in the kernel cache)."""
    mode = MODES[mode_name]
    recs = _case(kind)[1]
    data, offsets = c_walker.pack(recs)
    n = len(recs)
    want = _over_window(offsets, n, k, _window(offsets))
    assert want >= 2
    exp = c_walker.decode_threaded(recs, cases.form_switch_schema(kind), k)
    auto = mode == cabi.KERNEL_AUTO

    def met(d, what, call=None, exact=True):
        print(kind, mode_name, k, what, call, {s: d[s] for s in ("fused_calls", "two_sync_calls", "over_window_tiles", "subtiled_tiles", "ranged_retries")},
              "expected", want)
        assert d["ranged_retries"] == 0
        assert d["over_window_tiles"] > 0, "the call met no tile past the window"
        if exact:
            assert d["over_window_tiles"] == want
        if mode == cabi.KERNEL_GENERIC or (auto and call == 0):
            assert d["subtiled_tiles"] == 0            # walked from global memory in one piece
        elif exact:
            assert d["subtiled_tiles"] == want         # the ranged pair
        return d

    dev = _upload(data, offsets)
    for asynchronous in (False, True):
        schema = cases.form_switch_schema(kind, tag + ("a" if asynchronous else ""))
        if auto:
            _starts_specialised(kind, schema)
        for i in range(3):
            c0 = cabi.engine_counters()
            r = _device_call(dev, offsets, schema, k, mode, asynchronous=asynchronous)
            if asynchronous:
                r.wait()
            got = r.to_host()
            r.free()
            d = _delta(c0)
            _same(got, exp)
            met(d, f"decode_device async={asynchronous}", i)
            assert d["fused_calls"] == 1 or not auto
    # (the host calls' window is sized like the device-resident call's, from the same payload; only "some" is asserted of them)
    schema = cases.form_switch_schema(kind, tag + "h")
    if auto:
        _starts_specialised(kind, schema)
    for i in range(2):
        c0 = cabi.engine_counters()
        got = cabi.decode_packed(data, offsets, schema, k, kernel=mode)
        d = _delta(c0)
        _same(got, exp)
        met(d, "decode_packed", i, exact=False)
    if auto:
        _starts_specialised(kind, schema, "python")
    old = P.set_kernel_mode(mode_name)
    try:
        for i in range(2):
            c0 = cabi.engine_counters()
            got = P.deserialize_array_threaded(recs, schema, k)
            d = _delta(c0)
            _same(got, exp)
            met(d, "deserialize_array_threaded", i, exact=False)
    finally:
        P.set_kernel_mode(old)
    # two submissions, and never the pair: the emit kernel of the second submission walks the tiles past the window
    schema = cases.form_switch_schema(kind, tag)
    monkeypatch.setenv("RUHVRO_HIP_TWO_SYNC", "1")
    if mode != cabi.KERNEL_GENERIC:
        monkeypatch.setenv("RUHVRO_HIP_RANGED", "0")
    c0 = cabi.engine_counters()
    r = _device_call(dev, offsets, schema, k, mode)
    got = r.to_host()
    st = r.stats
    r.free()
    d = _delta(c0)
    _same(got, exp)
    met(d, "decode_device, two submissions", 0 if auto else None, exact=False)
    assert d["two_sync_calls"] == 1 and d["fused_calls"] == 0 and d["over_window_tiles"] == want and d["subtiled_tiles"] == 0
    assert st["specialized"] == (0 if mode == cabi.KERNEL_GENERIC else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind", ["longs8", "longs8_nullable"])
@pytest.mark.parametrize("mode_name", sorted(MODES))
def test_k_zero_past_the_window(mode_name, kind, k, monkeypatch):
    """Eight long columns (plain and nullable: validity bitmaps, null counts), 20,000 records of 8 - 16 bytes and 768 of 80: the
    window is 8,192 bytes and the tiles of the large records are 20 KB.  No counter, so no size pass: nobody refuses the call, and
    the emit kernel of the tiles that fit must not leave such a tile out.  Every entry point, AUTO / SPECIALIZED / GENERIC; three
    device-resident calls in a row (synchronous, then asynchronous) so that the call without history and the calls the history
    drives both run, and one call in two submissions.  over_window_tiles advances by the number of tiles the offsets put past
    the window -- counted by the emit kernels themselves, no size pass is added -- and by as many subtiled_tiles when the
    ranged pair ran."""
    _k_zero_calls(kind, mode_name, k, f"_{mode_name[0]}{k}", monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("mode_name", ["auto", "specialized"])
def test_k_zero_past_a_hooked_window(mode_name, monkeypatch):
    """flat4 (int, long, double, boolean: tiles of 6,144 bytes at most) behind RUHVRO_HIP_WIN_BYTES=4096, and the eight longs behind
    the hook at 8192: the same roads with the window set by hand.  (flat4's schema object is shared with other tests, so its
    history is not known here: the first AUTO call may or may not launch the ranged pair; the buffers and the count hold either
    way.)"""
    import struct
    from avrogen.encoder import zigzag
    mode = MODES[mode_name]
    monkeypatch.setenv("RUHVRO_HIP_WIN_BYTES", "4096")
    schema = SCHEMAS["flat4"]
    # 24 bytes per record in [7000, 7768) -- a five-byte int, a ten-byte long -- and 11 elsewhere: tiles of 6,144 and 2,816 bytes
    recs = []
    for r in range(20_011):
        big = 7000 <= r < 7768
        i = (-1) ** r * ((1 << 30) + r) if big else r % 64
        v = (-1) ** r * ((1 << 62) + 1 + r) if big else -(r % 64)
        recs.append(zigzag(i) + zigzag(v) + struct.pack("<d", r * 0.25) + bytes([r & 1]))
    data, offsets = c_walker.pack(recs)
    n = len(recs)
    assert max(len(x) for x in recs) == 24 and min(len(x) for x in recs) == 11
    want = _over_window(offsets, n, 3, 4096)
    assert want >= 2
    exp = c_walker.decode_threaded(recs, schema, 3)
    cabi.prebuild(schema)
    dev = _upload(data, offsets)
    for i in range(3):
        c0 = cabi.engine_counters()
        r = _device_call(dev, offsets, schema, 3, mode)
        got = r.to_host()
        st = r.stats
        r.free()
        d = _delta(c0)
        print("flat4", mode_name, i, d["over_window_tiles"], d["subtiled_tiles"], "expected", want)
        _same(got, exp)
        assert st["specialized"] == 1
        assert d["over_window_tiles"] == want and d["ranged_retries"] == 0
    monkeypatch.setenv("RUHVRO_HIP_WIN_BYTES", "8192")
    _k_zero_calls("longs8", mode_name, 3, f"_{mode_name[0]}_hook", monkeypatch)


@pytest.mark.gpu
def test_k_zero_past_the_window_with_poisoned_pools():
    """RUHVRO_HIP_POISON=1 is read once per process (engine_internal.h Pool), so the K == 0 cases run once more in a process of
    their own with every pooled block handed out as 0xA5: a tile that is left out shows the poison, not the zeros or the previous
    call's rows of a recycled arena."""
    env = dict(os.environ, RUHVRO_HIP_POISON="1", RUHVRO_HIP_SKIP_WARM="1")
    p = subprocess.run([sys.executable, "-m", "pytest", "tests/test_form_switch.py", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "test_k_zero_past_the_window and not poisoned"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-1500:]
    assert " passed" in p.stdout and "skipped" not in p.stdout, p.stdout[-1500:]


# ---- 2. flat schemas whose tiles all fit keep their launch sequence ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode_name", ["auto", "specialized"])
@pytest.mark.parametrize("which", ["flat4", "longs8_small"])
def test_flat_schemas_whose_tiles_fit_keep_their_launch_sequence(which, mode_name):
    """No size pass, no retry, nothing counted: a schema without variable-length output whose tiles all fit the window is launched
    as before -- layout, emit, publish in one submission from its second call on (the first call of a schema takes two)."""
    mode = MODES[mode_name]
    if which == "flat4":
        schema = SCHEMAS["flat4"]
        data, offsets = fastgen.generate("flat4", 50_000)
    else:
        schema, recs = _case("longs8", "_flat")
        data, offsets = c_walker.pack(recs[:5000] + recs[5768:])
    n = len(offsets) - 1
    assert _over_window(offsets, n, 4, _window(offsets)) == 0
    exp = c_walker.decode_packed(c_walker.CompiledSchema(schema), data, offsets, 4, threaded=True)
    cabi.prebuild(schema)
    dev = _upload(data, offsets)
    for i in range(4):
        c0 = cabi.engine_counters()
        r = _device_call(dev, offsets, schema, 4, mode)
        got = r.to_host()
        st = r.stats
        r.free()
        d = _delta(c0)
        _same(got, exp)
        print(which, mode_name, i, st["size_kernel_ms"], {s: d[s] for s in ("fused_calls", "two_sync_calls", "over_window_tiles", "ranged_retries")})
        assert st["specialized"] == 1 and st["size_kernel_ms"] == 0.0 and st["scan_kernel_ms"] == 0.0
        assert d["ranged_retries"] == 0 and d["over_window_tiles"] == 0 and d["subtiled_tiles"] == 0 and d["capacity_retries"] == 0
        if i > 0:
            assert d["fused_calls"] == 1 and d["two_sync_calls"] == 0
        else:
            assert d["fused_calls"] + d["two_sync_calls"] == 1


# ---- 3. the lowest failing record wins across a refusal ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("when", ["first_call", "later_call"])
@pytest.mark.parametrize("surface", ["python", "device_async"])
def test_the_lowest_failing_record_wins_across_a_refusal(surface, when, monkeypatch):
    """id_str, record 100 cut inside its string (a tile past the window, which the size kernel refuses unwalked) and record 3000
    with a negative length (a tile that fits, which it walks): the message is the oracle's, record 100's.  AUTO with
    RUHVRO_HIP_RANGED=0.  first_call: the schema object's first call (two submissions) -- that it started on the specialised
    kernels is proved by the ranged retry it counts, which only their size kernel raises; later_call: behind a call on small
    records that reports specialized == 1 (one submission)."""
    tag = {"first_call": "_first", "later_call": "_later"}[when]
    schema, recs = _case("id_str_damaged", tag)
    k = 3
    want = _oracle_error(recs, schema, k)
    assert want == _oracle_error([r if i != 3000 else _case("id_str")[1][3000] for i, r in enumerate(recs)], schema, k)      # record 100's
    cabi.prebuild(schema)
    if when == "later_call":
        _starts_specialised("id_str", schema, "python" if surface == "python" else "cabi")
    monkeypatch.setenv("RUHVRO_HIP_RANGED", "0")
    c0 = cabi.engine_counters()
    if surface == "python":
        old = P.set_kernel_mode("auto")
        try:
            with pytest.raises(ValueError) as g:
                P.deserialize_array_threaded(recs, schema, k)
        finally:
            P.set_kernel_mode(old)
        print("python", when, repr(str(g.value)), "oracle", repr(want))
        assert str(g.value) == want
    else:
        data, offsets = c_walker.pack(recs)
        dev = _upload(data, offsets)
        r = None
        with pytest.raises(ValueError) as g:
            r = _device_call(dev, offsets, schema, k, cabi.KERNEL_AUTO, asynchronous=True)
            r.wait()
        print("device_async", when, repr(str(g.value)), "oracle", repr(want))
        assert str(g.value) == want
        if r is not None:                      # (a first call is settled inside rh_decode_device: no result to ask)
            with pytest.raises(ValueError) as g2:
                r.to_host()
            assert str(g2.value) == want
            r.free()
    d = _delta(c0)
    assert d["ranged_retries"] == 1, d
    assert (d["two_sync_calls"] >= 1) if when == "first_call" else (d["fused_calls"] >= 1), d


@pytest.mark.gpu
@pytest.mark.parametrize("mode_name", ["auto", "specialized"])
@pytest.mark.parametrize("surface", ["python", "device_async"])
@pytest.mark.parametrize("damaged", ["longs8_damaged", "longs8_damaged_apart"])
def test_the_lowest_failing_record_of_a_schema_without_counters(damaged, surface, mode_name):
    """longs8, record 5300 cut in the middle of a varint inside a tile past the window, record 9000 cut inside a tile that fits
    (longs8_damaged_apart: an over-long varint there, whose message is another -- two cuts of a long column read the same).
    No size pass: the emit kernels write first_bad, and the one that walks the tile past the window must have walked it."""
    schema, recs = _case(damaged, "_later")
    k = 3
    want = _oracle_error(recs, schema, k)
    assert want == _oracle_error([r if i != 9000 else _case("longs8")[1][9000] for i, r in enumerate(recs)], schema, k)       # record 5300's
    if mode_name == "auto":
        _starts_specialised("longs8", schema, "python" if surface == "python" else "cabi")
    if surface == "python":
        old = P.set_kernel_mode(mode_name)
        try:
            with pytest.raises(ValueError) as g:
                P.deserialize_array_threaded(recs, schema, k)
        finally:
            P.set_kernel_mode(old)
    else:
        data, offsets = c_walker.pack(recs)
        dev = _upload(data, offsets)
        r = None
        with pytest.raises(ValueError) as g:
            r = _device_call(dev, offsets, schema, k, MODES[mode_name], asynchronous=True)
            r.wait()
        if r is not None:
            with pytest.raises(ValueError) as g2:
                r.to_host()
            assert str(g2.value) == want
            r.free()
    print(surface, mode_name, repr(str(g.value)), "oracle", repr(want))
    assert str(g.value) == want


# ---- 4. single pass, then two pass, then the generic kernels ----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["id_str", "full_skewed"])
def test_single_pass_then_two_pass_then_generic(which, monkeypatch):
    """A single-pass call that outgrows a capacity is repeated in the two-pass form; that repeat, launched without the ranged pair,
    meets a tile past the window and is itself repeated on the generic kernels -- in a synchronous call and in the settlement of
    an asynchronous one."""
    if which == "id_str":
        schema, recs = _case("id_str", "_single")
        data, offsets = c_walker.pack(recs)
        exp = c_walker.decode_threaded(recs, schema, 3)
    else:
        monkeypatch.setenv("RUHVRO_HIP_WIN_BYTES", "8192")
        # (the full schema under a name of its own: the size and capacity history of SCHEMAS["full"] -- the single pass's
        #  cool-down after other tests' fail-overs among it -- is shared by every test that decodes that schema text)
        schema = cases.form_switch_full_skewed_schema()
        data, offsets = fastgen.generate("full_skewed", 30_011)
        exp = c_walker.decode_packed(c_walker.CompiledSchema(schema), data, offsets, 3, threaded=True)
    dev = _upload(data, offsets)
    # the single-pass kernel loaded, the per-row history of this input recorded
    r = _device_call(dev, offsets, schema, 3, cabi.KERNEL_SPECIALIZED, single_pass=True)
    _same(r.to_host(), exp)
    r.free()
    monkeypatch.setenv("RUHVRO_HIP_RANGED", "0")
    monkeypatch.setenv("RUHVRO_HIP_SINGLE_SLACK_PERMILLE", "700")
    for asynchronous in (False, True):
        c0 = cabi.engine_counters()
        r = _device_call(dev, offsets, schema, 3, cabi.KERNEL_AUTO, single_pass=True, asynchronous=asynchronous)
        if asynchronous:
            r.wait()
        got = r.to_host()
        r.free()
        d = _delta(c0)
        print(which, "async" if asynchronous else "sync", {s: d[s] for s in ("single_pass_calls", "single_pass_failovers", "ranged_retries")})
        _same(got, exp)
        assert d["single_pass_calls"] == 1 and d["single_pass_failovers"] == 1 and d["ranged_retries"] == 1, d


@pytest.mark.gpu
def test_single_pass_then_two_pass_then_wide_index(monkeypatch):
    """A single-pass call whose child row domain outgrows its capacity (the capacities stop below RUHVRO_HIP_NARROW_ROWS) is
    repeated in the two-pass form; that repeat finds the domain at the bound of 32-bit indexing and is itself repeated on the
    generic kernels -- in a synchronous call and in the settlement of an asynchronous one.  The full schema under names of its
    own, 6,000 records in 3 chunks: 2,000 rows per chunk < 2,500 <= ~3,000 child rows per chunk.

    One schema object per call.  With one object for both, the second call never starts on the single pass (measured on the commit
    before the ladder became one function: single_pass_calls 0, single_pass_failovers 0, wide_fallbacks 1, batches identical): the first call's
    fail-over is a real LF_CAPACITY one, so the schema sits its next eight calls out (try_single's cool-down)."""
    recs = synth.records("full", 6000, seed=2)
    data, offsets = c_walker.pack(recs)
    exp = c_walker.decode_threaded(recs, cases.form_switch_full_wide_index_schema(), 3)
    dev = _upload(data, offsets)
    for asynchronous in (False, True):
        schema = cases.form_switch_full_wide_index_schema("_async" if asynchronous else "")
        monkeypatch.delenv("RUHVRO_HIP_NARROW_ROWS", raising=False)
        # the single-pass kernel loaded, the per-row history of this input recorded
        r = _device_call(dev, offsets, schema, 3, cabi.KERNEL_SPECIALIZED, single_pass=True)
        _same(r.to_host(), exp)
        r.free()
        monkeypatch.setenv("RUHVRO_HIP_NARROW_ROWS", "2500")
        c0 = cabi.engine_counters()
        r = _device_call(dev, offsets, schema, 3, cabi.KERNEL_AUTO, single_pass=True, asynchronous=asynchronous)
        if asynchronous:
            r.wait()
        got = r.to_host()
        st = r.stats
        r.free()
        d = _delta(c0)
        print("async" if asynchronous else "sync", {s: d[s] for s in ("single_pass_calls", "single_pass_failovers", "wide_fallbacks", "ranged_retries")},
              "specialized", st["specialized"])
        _same(got, exp)
        assert d["single_pass_calls"] == 1 and d["single_pass_failovers"] == 1 and d["wide_fallbacks"] == 1 and d["ranged_retries"] == 0, d
        assert st["specialized"] == 0, st


# ---- 5. split calls ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["id_str", "longs8", "id_str_damaged"])
def test_split_calls_past_the_window(name, monkeypatch):
    """The call dealt to internal streams (RUHVRO_HIP_INTERNAL_STREAMS=4 from 1,000 records on), AUTO, no ranged pair: a group of
    id_str whose size kernel refuses is repeated on the generic kernels on its own; the groups of longs8 walk their tiles past the
    window themselves; the damaged list reports the oracle's record."""
    kind = name[: -len("_damaged")] if name.endswith("_damaged") else name
    schema, recs = _case(name, "_split")
    k = 7
    data, offsets = c_walker.pack(recs)
    _starts_specialised(kind, schema)
    monkeypatch.setenv("RUHVRO_HIP_RANGED", "0")
    monkeypatch.setenv("RUHVRO_HIP_INTERNAL_STREAMS", "4")
    monkeypatch.setenv("RUHVRO_HIP_SPLIT_MIN", "1000")
    dev = _upload(data, offsets)
    for asynchronous in (False, True):
        c0 = cabi.engine_counters()
        if name.endswith("_damaged"):
            want = _oracle_error(recs, schema, k)
            r = None
            with pytest.raises(ValueError) as g:
                r = _device_call(dev, offsets, schema, k, cabi.KERNEL_AUTO, want_stats=False, asynchronous=asynchronous)
                r.wait()
            assert str(g.value) == want
            if r is not None:
                r.free()
        else:
            r = _device_call(dev, offsets, schema, k, cabi.KERNEL_AUTO, want_stats=False, asynchronous=asynchronous)
            if asynchronous:
                r.wait()
            got = r.to_host()
            r.free()
            _same(got, c_walker.decode_threaded(recs, schema, k))
        d = _delta(c0)
        print(name, "async" if asynchronous else "sync", {s: d[s] for s in ("split_calls", "ranged_retries", "over_window_tiles")})
        assert d["split_calls"] > 0
        if kind == "id_str":
            assert d["ranged_retries"] >= 1
        else:
            assert d["ranged_retries"] == 0 and d["over_window_tiles"] >= 2


# ---- 6. history -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["id_str", "longs8"])
def test_the_history_brings_the_ranged_pair(kind):
    """The first AUTO call that meets tiles past the window does without the pair: id_str is refused and repeated once
    (ranged_retries == 1); longs8 needs no repeat -- its emit kernel walks such tiles from global memory, an in-kernel fallback
    that needs no pair, so ranged_retries stays 0 from the first call on -- and counts them.  Both feed the schema's history.
    rh_schema_kernels_ready does not cover the pair, so one SPECIALIZED call loads it; the AUTO calls behind it launch it: no
    retry, every tile past the window walked in ranges."""
    schema, recs = _case(kind, "_history")
    k = 3
    data, offsets = c_walker.pack(recs)
    want = _over_window(offsets, len(recs), k, _window(offsets))
    assert want >= 2
    exp = c_walker.decode_threaded(recs, schema, k)
    _starts_specialised(kind, schema)
    dev = _upload(data, offsets)

    def call(mode):
        c0 = cabi.engine_counters()
        r = _device_call(dev, offsets, schema, k, mode)
        got = r.to_host()
        st = r.stats
        r.free()
        d = _delta(c0)
        print(kind, mode, {s: d[s] for s in ("fused_calls", "over_window_tiles", "subtiled_tiles", "ranged_retries")}, "expected", want)
        _same(got, exp)
        return d, st

    d, st = call(cabi.KERNEL_AUTO)
    assert d["ranged_retries"] == (1 if kind == "id_str" else 0)
    assert d["over_window_tiles"] == want and d["subtiled_tiles"] == 0
    d, st = call(cabi.KERNEL_SPECIALIZED)
    assert d["ranged_retries"] == 0 and d["over_window_tiles"] == want and d["subtiled_tiles"] == want
    for _ in range(3):
        d, st = call(cabi.KERNEL_AUTO)
        assert st["specialized"] == 1
        assert d["ranged_retries"] == 0
        assert d["subtiled_tiles"] == d["over_window_tiles"] == want
