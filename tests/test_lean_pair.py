"""The lean pair: rh_spec_size / rh_spec_emit compiled from the default source behind `#define RH_V_LEN16 1` and
`#define RH_V_INT28 1` (walk.h's narrow single-read forms), and the engine's choice between it and the default (wide) pair per
(schema, device) -- include/ruhvro_hip.h, engine_device_call.cpp lean_select / launch_probe / lean_learn.

Correctness never depends on the choice: every result below is compared with oracle.c_walker, whichever pair ran, and the road
a call took is read from rh_lean_counters / rh_schema_lean_state (accessors of their own: rh_engine_counters keeps its layout).
The GPU tests lower RUHVRO_HIP_LEAN_MIN_RECORDS to 256 so that a few tiles qualify; each schema handle below is a fresh one
(the schema text with a trailing run of newline-blank pairs), so its selection state starts undecided."""
import os
import subprocess
import sys

import numpy as np
import pytest

from arrow_compare import assert_batches_identical
from avrogen import synth
from avrogen.encoder import to_datum
from avrogen.schemas import SCHEMAS
from oracle import c_walker
from oracle.avro_schema import parse_schema

from pyruhvro_amd import cabi
from conftest import ROOT

DEFINES = "#define RH_V_LEN16 1\n#define RH_V_INT28 1\n"
T = 256                        # records per tile (program.h kBlock; the schemas decoded here are not wide)
_fresh = [0]


def _handle(name="full"):
    """The named schema as a text no other test uses (the others append runs of blanks, of tabs or two newlines to get a handle
    of their own; a shared handle would carry this file's size history into their first call): a schema handle, and a
    selection state, of its own."""
    _fresh[0] += 1
    return SCHEMAS[name] + "\n " * _fresh[0]


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the generator and the C ABI
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["full", "cfg3"])
def test_lean_source_is_the_default_source_behind_the_two_defines(name, monkeypatch):
    """The two define lines follow the generator's header line, as RUHVRO_HIP_VARIANT's do; the lean source is byte for byte
    what RUHVRO_HIP_VARIANT=LEN16,INT28 generates (same text, same kernel-cache key), whatever the variable holds when the lean
    source is asked for.  Behind the defines the text is the default source, except where the generator itself sizes a fused
    head read by the form widths (specialize.cpp head_bytes: 2-byte lengths, 4-byte ints) -- the same lines the variable moves."""
    monkeypatch.delenv("RUHVRO_HIP_VARIANT", raising=False)
    default = cabi.kernel_source(SCHEMAS[name])
    lean = cabi.lean_kernel_source(SCHEMAS[name])
    head, rest = default.split("\n", 1)
    assert lean.startswith(head + "\n" + DEFINES)
    assert "RH_V_" not in default
    body = lean[len(head) + 1 + len(DEFINES):]
    assert body.count("\n") == rest.count("\n")
    differing = [(a, b) for a, b in zip(rest.split("\n"), body.split("\n")) if a != b]
    assert all("h_" in a and "h_" in b for a, b in differing)        # (handler calls only: their look-ahead template arguments)
    key = cabi.lean_kernel_key(SCHEMAS[name])
    monkeypatch.setenv("RUHVRO_HIP_VARIANT", "LEN16,INT28")
    assert cabi.kernel_source(SCHEMAS[name]) == lean
    assert cabi.kernel_key(SCHEMAS[name]) == key
    assert cabi.lean_kernel_source(SCHEMAS[name]) == lean           # (no define twice)
    monkeypatch.setenv("RUHVRO_HIP_VARIANT", "INT28")
    assert cabi.lean_kernel_source(SCHEMAS[name]) == head + "\n#define RH_V_INT28 1\n#define RH_V_LEN16 1\n" + body


def test_default_kernel_keys_are_unchanged_by_the_feature(monkeypatch):
    """rh_schema_kernel_key / rh_schema_kernel_source keep describing the default kernels: the keys the committed traffic stamp
    and the other test files pin, before and after the lean flavour was generated, and different from the lean key."""
    import json
    monkeypatch.delenv("RUHVRO_HIP_VARIANT", raising=False)
    pinned = {"full": "d4e730578ea82b76"}
    before = {n: cabi.kernel_key(SCHEMAS[n]) for n in ("full", "cfg3", "flat4")}
    src = {n: cabi.kernel_source(SCHEMAS[n]) for n in before}
    for n in before:
        lean_key = cabi.lean_kernel_key(SCHEMAS[n])
        cabi.lean_kernel_source(SCHEMAS[n])
        assert cabi.kernel_key(SCHEMAS[n]) == before[n] and cabi.kernel_source(SCHEMAS[n]) == src[n]
        assert lean_key != before[n]
    assert before["full"] == pinned["full"]
    assert json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json")))["_kernel_key"] == before["full"]
    assert cabi.lib().rh_abi_version() == 7
    assert cabi.ENGINE_COUNTERS[-2:] == ("tolerant_calls", "tolerant_repairs") and len(cabi.engine_counters()) == 17


def test_no_lean_flavour_without_a_size_pass_or_for_a_wide_schema():
    for name in ("flat4", "wide97", "wide200"):
        assert cabi.lean_kernel_source(SCHEMAS[name]) is None, name
        assert cabi.lean_kernel_key(SCHEMAS[name]) is None, name
        assert cabi.lean_state(SCHEMAS[name], 0) == cabi.LEAN_NONE, name
        assert cabi.lean_ready(SCHEMAS[name]) is False
    assert cabi.lean_state(_handle("cfg3"), 0) == cabi.LEAN_UNDECIDED


def test_the_lean_pair_of_cfg3_compiles_for_gfx950(tmp_path):
    """An empty kernel cache of its own, the prebuild of a fresh process (hiprtc, gfx950, no GPU): with
    RUHVRO_HIP_PREBUILD_LEAN=1 the lean pair's two code objects are compiled next to the default kernels, with 0 (the default:
    tests/test_specialize.py pins what a plain prebuild leaves in the cache) they are not."""
    code = ("import sys; from pyruhvro_amd import cabi; from avrogen.schemas import SCHEMAS; s = SCHEMAS['cfg3']\n"
            "assert not cabi.lean_ready(s)\n"
            "cabi.prebuild(s)\n"
            "print('ready', int(cabi.lean_ready(s)), int(cabi.kernels_ready(s)))\n")
    counts = {}
    for lean in ("0", "1"):
        d = tmp_path / ("cache" + lean)
        d.mkdir()
        env = dict(os.environ, RUHVRO_HIP_KERNEL_CACHE=str(d), RUHVRO_HIP_PREBUILD_LEAN=lean, RUHVRO_HIP_PREBUILD_FUSED="0",
                   RUHVRO_HIP_PREBUILD_RANGED="0")
        env.pop("RUHVRO_HIP_VARIANT", None)
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.split()[-3:] == ["ready", lean, "1"]
        counts[lean] = len([f for f in os.listdir(d) if f.endswith(".hsaco")])
    assert counts["1"] == counts["0"] + 2


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
_data = {}


def _friendly():
    """1,024 records of the benchmark generator (ints below 2^27, lengths below 8 KiB) and the oracle's batches of their
    3 chunks (341 + 341 + 342 rows: a ragged last chunk, two tiles each)."""
    if "friendly" not in _data:
        vals = [synth.gen_full(7, i) for i in range(1024)]
        recs = [to_datum(parse_schema(SCHEMAS["full"]), v) for v in vals]
        _data["friendly"] = (vals, recs, c_walker.decode_threaded(recs, SCHEMAS["full"], 3))
    return _data["friendly"]


EDGE_ROWS = {256 + 64 + 3: ("age", (1 << 27) - 1), 256 + 64 + 4: ("age", 1 << 27),
             256 + 64 + 5: ("name", "n" * 8191), 256 + 64 + 6: ("name", "N" * 8192)}


def _edges():
    """512 friendly records, one chunk, and in the second wavefront of the SECOND tile one record at each edge of the narrow
    forms: an int of 2^27 - 1 (four bytes on the wire: inside) against 2^27 (five), a string of 8,191 bytes (a two-byte length:
    inside) against 8,192 (three)."""
    if "edges" not in _data:
        vals = [dict(v) for v in _friendly()[0][:512]]
        for row, (field, value) in EDGE_ROWS.items():
            vals[row][field] = value
        recs = [to_datum(parse_schema(SCHEMAS["full"]), v) for v in vals]
        _data["edges"] = (recs, c_walker.decode_threaded(recs, SCHEMAS["full"], 1))
    return _data["edges"]


def _upload(recs):
    import torch
    data, offsets = c_walker.pack(recs)
    d_data = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda:0")
    d_data[: len(data)].copy_(torch.from_numpy(data.copy()))
    d_off = torch.from_numpy(offsets.view(np.int64).copy()).to("cuda:0")
    return d_data, d_off, offsets


def _call(dev, schema, k, exp=None, asynchronous=False):
    """One AUTO-mode device-resident decode -> (deltas of rh_engine_counters, deltas of rh_lean_counters); the buffers are the
    oracle's when `exp` is given."""
    import torch
    d_data, d_off, offsets = dev
    e0, l0 = cabi.engine_counters(), cabi.lean_counters()
    r = cabi.decode_device(d_data.data_ptr(), d_off.data_ptr(), int(offsets[-1]), len(offsets) - 1, schema, k, device=0,
                           stream=torch.cuda.current_stream().cuda_stream, kernel=cabi.KERNEL_AUTO, asynchronous=asynchronous)
    try:
        if asynchronous:
            r.wait()
        got = r.to_host()
    finally:
        r.free()
    e1, l1 = cabi.engine_counters(), cabi.lean_counters()
    if exp is not None:
        assert len(got) == len(exp)
        for g, e in zip(got, exp):
            assert_batches_identical(g, e)
    return {key: e1[key] - e0[key] for key in e1}, {key: l1[key] - l0[key] for key in l1}


@pytest.fixture
def lean_env(monkeypatch):
    monkeypatch.setenv("RUHVRO_HIP_LEAN_MIN_RECORDS", "256")
    monkeypatch.delenv("RUHVRO_HIP_LEAN", raising=False)
    monkeypatch.delenv("RUHVRO_HIP_VARIANT", raising=False)
    # the edge records put ~16 KB of strings into one tile: a window that holds it, so that the tile is walked by the pair
    # under test and not handed to the ranged kernels
    monkeypatch.setenv("RUHVRO_HIP_WIN_BYTES", str(64 * 1024))
    monkeypatch.setenv("RUHVRO_HIP_PREBUILD_LEAN", "1")
    cabi.prebuild(SCHEMAS["full"])
    return monkeypatch


@pytest.mark.gpu
def test_forced_lean_on_friendly_records(lean_env):
    """RUHVRO_HIP_LEAN=1: every qualifying call launches the lean pair (a schema's first call lays its arena out on the host and
    stays wide).  Friendly records, 3 chunks with a ragged last one: identical buffers, no re-walk, no careful tile."""
    lean_env.setenv("RUHVRO_HIP_LEAN", "1")
    _, recs, exp = _friendly()
    dev, schema = _upload(recs), _handle()
    _call(dev, schema, 3, exp)
    for _ in range(2):
        e, l = _call(dev, schema, 3, exp)
        print("forced lean, friendly", {k: e[k] for k in ("tiles", "careful_tiles", "rewalked_waves")}, l)
        assert l["lean_calls"] == 1 and l["probes"] == 0 and l["fallbacks"] == 0
        assert e["tiles"] == 6 and e["careful_tiles"] == 0 and e["rewalked_waves"] == 0 and e["over_window_tiles"] == 0
    lean_env.setenv("RUHVRO_HIP_LEAN", "0")
    e, l = _call(dev, schema, 3, exp)
    assert l["lean_calls"] == 0 and l["probes"] == 0


@pytest.mark.gpu
def test_forced_lean_at_the_edges_of_the_narrow_forms(lean_env):
    """The records just inside the narrow forms are read by them; the two just outside re-walk their wavefront (all four share
    one) and flag their tile, which the emit kernel then walks carefully: identical buffers, one careful tile and one re-walked
    wavefront where the wide pair counts none, and the schema is wide afterwards."""
    recs, exp = _edges()
    dev, schema = _upload(recs), _handle()
    lean_env.setenv("RUHVRO_HIP_LEAN", "0")              # (never, and no probe: the schema stays undecided)
    _call(dev, schema, 1, exp)                           # (the schema's first call: two submissions, no statistics)
    e, l = _call(dev, schema, 1, exp)
    assert l["lean_calls"] == 0
    assert e["tiles"] == 2 and e["careful_tiles"] == 0 and e["rewalked_waves"] == 0 and e["over_window_tiles"] == 0
    lean_env.setenv("RUHVRO_HIP_LEAN", "1")
    e, l = _call(dev, schema, 1, exp)
    print("forced lean, edges", {k: e[k] for k in ("tiles", "careful_tiles", "rewalked_waves")}, l)
    assert l["lean_calls"] == 1 and l["fallbacks"] == 1
    assert e["tiles"] == 2 and e["careful_tiles"] == 1 and e["rewalked_waves"] == 1 and e["over_window_tiles"] == 0
    assert cabi.lean_state(schema, 0) == cabi.LEAN_WIDE
    # the same records without the two outside the forms: nothing leaves the narrow forms
    inside = list(recs)
    for row, (field, value) in EDGE_ROWS.items():
        if value in (1 << 27, "N" * 8192):
            inside[row] = _friendly()[1][row]
    schema2 = _handle()
    dev2, exp2 = _upload(inside), c_walker.decode_threaded(inside, SCHEMAS["full"], 1)
    _call(dev2, schema2, 1, exp2)
    e, l = _call(dev2, schema2, 1, exp2)
    assert l["lean_calls"] == 1 and l["fallbacks"] == 0 and e["careful_tiles"] == 0 and e["rewalked_waves"] == 0


@pytest.mark.gpu
def test_forced_lean_reports_the_lowest_malformed_record_like_the_wide_pair(lean_env):
    """Two malformed records with different messages (a truncated record at row 600, eleven continuation bytes at row 900): the
    lean call and the wide call raise the oracle's message -- the lower record's."""
    import torch
    _, recs, _ = _friendly()
    bad = list(recs)
    bad[600] = bad[600][: len(bad[600]) // 2]
    bad[900] = b"\x80" * 11
    only_later = list(recs)
    only_later[900] = bad[900]
    with pytest.raises(ValueError) as eo:
        c_walker.decode_threaded(bad, SCHEMAS["full"], 3)
    with pytest.raises(ValueError) as el:
        c_walker.decode_threaded(only_later, SCHEMAS["full"], 3)
    assert str(eo.value) != str(el.value)
    schema = _handle()
    _call(_upload(recs), schema, 3)                      # (a size history first: the calls below are single submissions)
    dev = _upload(bad)
    msgs = {}
    for force in ("0", "1"):
        lean_env.setenv("RUHVRO_HIP_LEAN", force)
        l0 = cabi.lean_counters()
        with pytest.raises(ValueError) as ei:
            cabi.decode_device(dev[0].data_ptr(), dev[1].data_ptr(), int(dev[2][-1]), len(bad), schema, 3, device=0,
                               stream=torch.cuda.current_stream().cuda_stream, kernel=cabi.KERNEL_AUTO)
        msgs[force] = str(ei.value)
        assert cabi.lean_counters()["lean_calls"] - l0["lean_calls"] == int(force)
    assert msgs["0"] == msgs["1"] == str(eo.value)


def _wide_batch():
    """The friendly records with one int of 2^27 in the second chunk."""
    if "wide" not in _data:
        vals = [dict(v) for v in _friendly()[0]]
        vals[500]["age"] = 1 << 27
        recs = [to_datum(parse_schema(SCHEMAS["full"]), v) for v in vals]
        _data["wide"] = (recs, c_walker.decode_threaded(recs, SCHEMAS["full"], 3))
    return _data["wide"]


def _auto_sequence(asynchronous):
    _, recs, exp = _friendly()
    wide_recs, wide_exp = _wide_batch()
    dev, dev_wide, schema = _upload(recs), _upload(wide_recs), _handle()
    assert cabi.lean_state(schema, 0) == cabi.LEAN_UNDECIDED
    # the first qualifying call runs on the wide pair and probes its own tiles with the lean size kernel: clean
    e, l = _call(dev, schema, 3, exp, asynchronous)
    assert l["probes"] == 1 and l["probes_clean"] == 1 and l["lean_calls"] == 0
    assert e["tiles"] == 0 and e["careful_tiles"] == 0          # (the probe's tiles are nobody's statistics; a first call counts none)
    assert cabi.lean_state(schema, 0) == cabi.LEAN_LEAN
    for _ in range(2):
        e, l = _call(dev, schema, 3, exp, asynchronous)
        assert l["lean_calls"] == 1 and l["probes"] == 0 and l["async_settled"] == int(asynchronous)
        assert e["tiles"] == 6 and e["careful_tiles"] == 0 and e["rewalked_waves"] == 0
    # one batch outside the narrow forms: still the oracle's buffers, and the schema falls back
    e, l = _call(dev_wide, schema, 3, wide_exp, asynchronous)
    print("auto, the wide batch", {k: e[k] for k in ("tiles", "careful_tiles", "rewalked_waves")}, l)
    assert l["lean_calls"] == 1 and l["fallbacks"] == 1
    assert e["careful_tiles"] == 1 and e["rewalked_waves"] == 1
    assert cabi.lean_state(schema, 0) == cabi.LEAN_WIDE
    # the next calls are served by the wide pair -- the same batch included, which it reads without a re-walk -- and none probes
    for d, x in ((dev_wide, wide_exp), (dev, exp), (dev, exp)):
        e, l = _call(d, schema, 3, x, asynchronous)
        assert l["lean_calls"] == 0 and l["probes"] == 0 and l["fallbacks"] == 0
        assert e["tiles"] == 6 and e["careful_tiles"] == 0 and e["rewalked_waves"] == 0
    assert cabi.lean_state(schema, 0) == cabi.LEAN_WIDE
    # ... for eight qualifying calls; then a probe (clean on the friendly records) and the lean pair again
    for _ in range(5):
        _call(dev, schema, 3, exp, asynchronous)
    e, l = _call(dev, schema, 3, exp, asynchronous)
    assert l["probes"] == 1 and l["probes_clean"] == 1 and l["lean_calls"] == 0
    e, l = _call(dev, schema, 3, exp, asynchronous)
    assert l["lean_calls"] == 1 and cabi.lean_state(schema, 0) == cabi.LEAN_LEAN
    # a dirty probe keeps the schema wide
    schema2 = _handle()
    e, l = _call(dev_wide, schema2, 3, wide_exp, asynchronous)
    assert l["probes"] == 1 and l["probes_dirty"] == 1 and cabi.lean_state(schema2, 0) == cabi.LEAN_WIDE
    e, l = _call(dev_wide, schema2, 3, wide_exp, asynchronous)
    assert l["lean_calls"] == 0 and l["probes"] == 0 and e["careful_tiles"] == 0 and e["rewalked_waves"] == 0


@pytest.mark.gpu
def test_auto_goes_lean_falls_back_and_returns(lean_env):
    _auto_sequence(False)


@pytest.mark.gpu
def test_auto_falls_back_when_the_calls_are_asynchronous(lean_env):
    """The same sequence with RH_ASYNC: the lean call is settled by rh_device_result_wait, which is where its statistics move
    the schema back."""
    _auto_sequence(True)


@pytest.mark.gpu
def test_the_other_roads_of_a_lean_call(lean_env):
    """A lean call whose reserved arena is too small re-runs its tail with the lean emit kernel (LF_CAPACITY); one that meets a
    tile past the LDS window is refused and repeated on the generic kernels (NeedRanged), asynchronous or not -- the oracle's
    buffers every time."""
    import torch
    from avrogen import fastgen
    lean_env.setenv("RUHVRO_HIP_LEAN", "1")
    # 40,000 records: ~7 MB of Arrow buffers, beyond the fixed 1 MiB slack of the arena reservation
    data, offsets = fastgen.generate("full", 40_000)
    exp = c_walker.decode_packed(c_walker.CompiledSchema(SCHEMAS["full"]), data, offsets, 3, threaded=True)
    d_data = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda:0")
    d_data[: len(data)].copy_(torch.from_numpy(data.copy()))
    dev = (d_data, torch.from_numpy(offsets.view(np.int64).copy()).to("cuda:0"), offsets)
    schema = _handle()
    _call(dev, schema, 3, exp)
    lean_env.setenv("RUHVRO_HIP_ARENA_PERMILLE", "1")      # "history": 0.001 output bytes per input byte
    e, l = _call(dev, schema, 3, exp)
    assert l["lean_calls"] == 1 and l["capacity_tails"] == 1 and e["capacity_retries"] == 1
    assert e["careful_tiles"] == 0 and e["rewalked_waves"] == 0
    lean_env.delenv("RUHVRO_HIP_ARENA_PERMILLE")
    # an 8 KiB window, no ranged pair: the edge tile (16 KB of strings) is past it
    lean_env.setenv("RUHVRO_HIP_WIN_BYTES", "8192")
    lean_env.setenv("RUHVRO_HIP_RANGED", "0")
    erecs, eexp = _edges()
    edev = _upload(erecs)
    for asynchronous in (False, True):
        schema2 = _handle()
        lean_env.setenv("RUHVRO_HIP_WIN_BYTES", str(64 * 1024))
        _call(edev, schema2, 1, eexp)
        lean_env.setenv("RUHVRO_HIP_WIN_BYTES", "8192")
        e, l = _call(edev, schema2, 1, eexp, asynchronous)
        print("lean, refused", asynchronous, l, "ranged_retries", e["ranged_retries"])
        assert l["lean_calls"] == 1 and l["need_ranged"] == 1 and e["ranged_retries"] == 1
        assert l["reruns"] == int(asynchronous)
        assert cabi.lean_state(schema2, 0) == cabi.LEAN_WIDE


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["flat4", "wide97"])
def test_schemas_without_a_lean_pair_never_go_lean(name, lean_env):
    lean_env.setenv("RUHVRO_HIP_LEAN", "1")
    recs = synth.records(name, 1024, seed=5)
    exp = c_walker.decode_threaded(recs, SCHEMAS[name], 3)
    dev, schema = _upload(recs), _handle(name)
    for _ in range(3):
        e, l = _call(dev, schema, 3, exp)
        assert all(v == 0 for v in l.values()), l
    assert cabi.lean_state(schema, 0) == cabi.LEAN_NONE
