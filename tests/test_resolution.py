"""Reader schemas: ``reader_schema=R`` decodes records written with schema W into the evolved schema R.

The contract, for every W, every R the resolver accepts, record list and k:

    decode(recs, W, k, reader_schema=R) == oracle_decode([to_datum(R, resolve(W, R, value_i)) for i], R, k)      buffer for buffer
    result.schema == arrow_schema(R)                                                                              metadata included

The expected value is always the ORACLE's decode under R of the re-encoded resolved values (tests/resolve_cases.py) -- never the
engine's own output.  A malformed record raises the plain W decode's message."""
import json
import os

import numpy as np
import pytest

import random_cases
import resolve_cases as RC
from arrow_compare import assert_batches_identical
from avrogen import synth
from avrogen.schemas import SCHEMAS
from oracle import c_walker
from oracle.avro_schema import parse_schema

import pyruhvro_amd as P
from pyruhvro_amd import cabi
from test_projection import PARENT_KEYS

KERNELS = {"generic": cabi.KERNEL_GENERIC, "specialized": cabi.KERNEL_SPECIALIZED}
FULL = SCHEMAS["full"]


@pytest.fixture(params=sorted(KERNELS))
def kernel(request):
    old = P.set_kernel_mode(request.param)
    yield KERNELS[request.param]
    P.set_kernel_mode(old)


def _same(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        g.validate(full=True)
        assert g.schema.equals(e.schema, check_metadata=True)
        assert_batches_identical(g, e)
        for a, b in zip(g.columns, e.columns):      # the absence or presence of validity buffers is the oracle's
            assert (a.buffers()[0] is None) == (b.buffers()[0] is None)
            assert a.null_count == b.null_count


def _oracle(recs, rj, k):
    """The oracle's decode under the reader schema: the C walker, or -- readers with `bytes`, which the reference's gate
    rejects -- the Python walker in its extended form, chunked by the reference's rule (deserialize.rs:53-58)."""
    from oracle import py_walker
    from oracle.avro_schema import SchemaError
    try:
        return c_walker.decode_threaded(recs, rj, k)
    except SchemaError:
        n = len(recs)
        k = min(max(k, 1), max(n, 1))
        sz = n // k
        return [py_walker.decode(recs[c * sz: (c + 1) * sz if c + 1 < k else n], rj, extended=True) for c in range(k)]


def _check(wj, rj, values, k, **kw):
    recs = RC.writer_records(wj, values)
    exp = _oracle(RC.reader_records(wj, rj, values), rj, k)
    got = P.deserialize_array_threaded(recs, wj, k, reader_schema=rj, **kw)
    _same(got, exp if "columns" not in kw else [b.select(kw["columns"]) for b in exp])
    return recs, exp


def _full_values(n, name="full", seed=11):
    gen = {"full": synth.gen_full, "full_skewed": synth.gen_full_skewed}[name]
    return [gen(seed, i) for i in range(n)]


NESTED_W = json.dumps({"type": "record", "name": "Outer", "fields": [
    {"name": "id", "type": "long"},
    {"name": "in", "type": {"type": "record", "name": "In", "fields": [{"name": "x", "type": "int"}, {"name": "y", "type": "string"}]}}]})
NESTED_R = RC.make_reader(NESTED_W, promote=lambda k: {"int": "double"}.get(k))


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wj,rj", [(FULL, RC.FULL_MIXED), (SCHEMAS["t_union"], RC.make_reader(SCHEMAS["t_union"], add=[(0, RC.ADD_ALL[0])])),
                                   (SCHEMAS["array_and_map"], RC.make_reader(SCHEMAS["array_and_map"], promote=lambda k: {"int": "long", "string": "bytes"}.get(k))),
                                   (NESTED_W, NESTED_R), (RC.PROMO_W, RC.promo_reader("a")), (RC.DEF_W, RC.def_readers()["spread"])])
def test_arrow_schema_is_the_readers(wj, rj):
    got = P.arrow_schema(wj, reader_schema=rj)
    exp = P.arrow_schema(rj)
    assert got.equals(exp, check_metadata=True)
    for f, g in zip(exp, got):
        assert f.equals(g, check_metadata=True)
    assert got.equals(cabi.Schema.get(wj, None, rj).arrow_schema, check_metadata=True)


def _rec(fields, name="R"):
    return json.dumps({"type": "record", "name": name, "fields": fields})


REFUSALS = [
    ("missing default", _rec([{"name": "a", "type": "int"}]), _rec([{"name": "a", "type": "int"}, {"name": "zz", "type": "int"}]), "zz"),
    ("record default", _rec([{"name": "a", "type": "int"}]),
     _rec([{"name": "a", "type": "int"}, {"name": "zz", "type": {"type": "record", "name": "Q", "fields": [{"name": "q", "type": "int"}]}, "default": {"q": 1}}]), "zz"),
    ("array default", _rec([{"name": "a", "type": "int"}]), _rec([{"name": "a", "type": "int"}, {"name": "zz", "type": {"type": "array", "items": "int"}, "default": []}]), "zz"),
    ("map default", _rec([{"name": "a", "type": "int"}]), _rec([{"name": "a", "type": "int"}, {"name": "zz", "type": {"type": "map", "values": "int"}, "default": {}}]), "zz"),
    ("fixed default", _rec([{"name": "a", "type": "int"}]), _rec([{"name": "a", "type": "int"}, {"name": "zz", "type": {"type": "fixed", "name": "F4", "size": 4}, "default": "abcd"}]), "zz"),
    ("nested add", NESTED_W, NESTED_W.replace('{"name": "y", "type": "string"}', '{"name": "y", "type": "string"}, {"name": "z", "type": "int", "default": 0}'), "in"),
    ("nested drop", NESTED_W, NESTED_W.replace(', {"name": "y", "type": "string"}', ''), "in"),
    ("nested reorder", NESTED_W, NESTED_W.replace('{"name": "x", "type": "int"}, {"name": "y", "type": "string"}', '{"name": "y", "type": "string"}, {"name": "x", "type": "int"}'), "in"),
    ("make nullable", _rec([{"name": "a", "type": "int"}]), _rec([{"name": "a", "type": ["null", "int"]}]), "'a'"),
    ("make non-nullable", _rec([{"name": "a", "type": ["null", "int"]}]), _rec([{"name": "a", "type": "int"}]), "'a'"),
    ("union first match", _rec([{"name": "u", "type": ["long", "int"]}]), _rec([{"name": "u", "type": ["long", "double"]}]), "'u'"),
    ("enum symbols", _rec([{"name": "e", "type": {"type": "enum", "name": "E", "symbols": ["A", "B"]}}]),
     _rec([{"name": "e", "type": {"type": "enum", "name": "E", "symbols": ["A", "B", "C"]}}]), "'e'"),
    ("enum default symbol", _rec([{"name": "a", "type": "int"}]),
     _rec([{"name": "a", "type": "int"}, {"name": "e", "type": {"type": "enum", "name": "E", "symbols": ["A", "B"]}, "default": "Z"}]), "'e'"),
    ("record name", _rec([{"name": "a", "type": "int"}]), _rec([{"name": "a", "type": "int"}], name="Other"), "Other"),
    ("long to int", _rec([{"name": "a", "type": "long"}]), _rec([{"name": "a", "type": "int"}]), "'a'"),
    ("string to int", _rec([{"name": "a", "type": "string"}]), _rec([{"name": "a", "type": "int"}]), "'a'"),
    ("deep non-promotable", _rec([{"name": "m", "type": {"type": "map", "values": {"type": "array", "items": "double"}}}]),
     _rec([{"name": "m", "type": {"type": "map", "values": {"type": "array", "items": "float"}}}]), "'m{}[]'"),
]


@pytest.mark.parametrize("what,wj,rj,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_start_with_reader_schema_and_name_the_field(what, wj, rj, word):
    for f in (lambda: P.arrow_schema(wj, reader_schema=rj),
              lambda: P.deserialize_array([b""], wj, reader_schema=rj),      # (raised before any GPU work)
              lambda: cabi.kernel_key(wj, reader_schema=rj)):
        with pytest.raises(ValueError) as e:
            f()
        assert str(e.value).startswith("reader schema: "), str(e.value)
        assert word in str(e.value), str(e.value)
    if what.endswith("default") and what != "missing default":
        with pytest.raises(ValueError, match="not supported yet"):
            P.arrow_schema(wj, reader_schema=rj)
    if what.startswith("nested"):
        with pytest.raises(ValueError, match="nested record resolution is not supported"):
            P.arrow_schema(wj, reader_schema=rj)


def test_kernel_keys():
    assert cabi.lib().rh_abi_version() == 7
    assert hasattr(cabi.lib(), "rh_schema_resolve")
    for name, key in PARENT_KEYS.items():
        assert cabi.kernel_key(SCHEMAS[name]) == key
    assert cabi.kernel_key(FULL, reader_schema=RC.FULL_MIXED) != PARENT_KEYS["full"]
    assert cabi.kernel_key(FULL, reader_schema=RC.FULL_MIXED) != cabi.kernel_key(FULL, reader_schema=RC.FULL_FIXED_ONLY)
    # a reader text equal to the writer's is a plain compile of the writer: its key, no resolved header
    assert cabi.kernel_key(FULL, reader_schema=FULL) == PARENT_KEYS["full"]
    assert "walk_resolve.h" not in cabi.kernel_source(FULL, reader_schema=FULL)
    assert "walk_resolve.h" not in cabi.kernel_source(FULL) and "walk_resolve.h" not in cabi.kernel_source(FULL, columns=["age"])
    src = cabi.kernel_source(FULL, reader_schema=RC.FULL_MIXED)
    assert "walk_resolve.h" in src and "h_fixed_p<" in src and "run_const<" in src


def test_program_shape_of_a_resolved_schema():
    import re
    src = cabi.kernel_source(FULL, reader_schema=RC.FULL_FIXED_ONLY)
    m = re.search(r"static constexpr int K = (\d+), KL = (\d+), NDOM = (\d+), NBUF = (\d+), NNODES = (\d+)", src)
    # created_at (double), d_int (default), age (validity + long): no counter, no child row domain
    assert tuple(map(int, m.groups())) == (0, 0, 1, 4, 4)
    assert "spec_flat.h" not in src                      # strings were dropped: the call keeps its size pass
    assert "spec_flat.h" in cabi.kernel_source(RC.FLAT_W, reader_schema=RC.FLAT_R)


@pytest.mark.parametrize("wj,rj", [(FULL, RC.FULL_MIXED), (RC.FLAT_W, RC.FLAT_R)], ids=["size_pass", "k0"])
def test_generated_source_compiles_for_gfx950(wj, rj, tmp_path, monkeypatch):
    monkeypatch.setenv("RUHVRO_HIP_KERNEL_CACHE", str(tmp_path))
    monkeypatch.setenv("RUHVRO_HIP_PREBUILD_FUSED", "0")
    monkeypatch.setenv("RUHVRO_HIP_PREBUILD_RANGED", "0")
    s = cabi.Schema(wj, None, rj)                         # (a schema object of its own: nothing of it is loaded yet)
    cached, err = cabi.C.c_int(), cabi.C.c_char_p()
    rc = cabi.lib().rh_schema_prebuild(s.handle, cabi.C.byref(cached), cabi.C.byref(err))
    assert rc == cabi.RH_OK, err.value
    assert cached.value == 0
    assert any(f.endswith(".hsaco") for f in os.listdir(tmp_path))


def test_encode_and_tolerant_entry_points_refuse_a_resolved_schema():
    import pyarrow as pa
    rj = RC.FULL_MIXED
    for f in (lambda: P.deserialize_array_tolerant([b""], FULL, reader_schema=rj),
              lambda: P.deserialize_array_threaded_tolerant([b""], FULL, 1, reader_schema=rj),
              lambda: P.deserialize_binary_array_tolerant(pa.array([b""], pa.binary()), FULL, 1, reader_schema=rj),
              lambda: P.validate_records([b""], FULL, reader_schema=rj),
              lambda: P.deserialize_to_device([b""], FULL, 1, on_error="placeholder", reader_schema=rj),
              lambda: P.serialize_record_batch(pa.record_batch([pa.array([1])], names=["x"]), FULL, 1, reader_schema=rj)):
        with pytest.raises(ValueError, match="reader schema"):
            f()
    # the C ABI: RH_ERR_ARGUMENT before any device work
    L, C = cabi.lib(), cabi.C
    h = cabi.Schema.get(FULL, None, rj).handle
    off = np.zeros(2, dtype=np.uint64)
    data = np.zeros(16, dtype=np.uint8)
    err, out, bad = C.c_char_p(), C.c_void_p(), C.c_uint64()
    L.rh_validate_packed.restype = C.c_int
    rc = L.rh_validate_packed(C.c_void_p(h), C.c_void_p(data.ctypes.data), C.c_void_p(off.ctypes.data), C.c_uint64(1), None, C.c_uint64(8),
                              C.byref(out), C.byref(bad), C.byref(err))
    assert rc == cabi.RH_ERR_ARGUMENT and b"resolved schema" in err.value
    assert cabi.kernels_ready(FULL, reader_schema=rj) in (True, False)
    with pytest.raises((RuntimeError, ValueError)):
        cabi.kernel_key(FULL, encode=True, reader_schema=rj)


def test_known_resolutions_lists_what_the_gpu_tests_decode():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import known_schemas
    assert set(known_schemas.known_resolutions()) >= set(RC.resolution_cases())


def test_value_resolution_rounds_once():
    w, r = parse_schema('"long"'), parse_schema('"float"')
    v = (1 << 60) + (1 << 36) + 1
    assert RC.resolve(w, r, v) != float(np.float32(float(v)))      # through a double: another float
    assert RC.resolve(w, r, v) == float(np.array(v, np.int64).astype(np.float32))


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(RC.PROMO_PICKS))
@pytest.mark.parametrize("k", [1, 3])
def test_promotions(kernel, which, k):
    _check(RC.PROMO_W, RC.promo_reader(which), RC.promo_values(700), k)


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(RC.def_readers()))
@pytest.mark.parametrize("k", [1, 3, 5])
def test_defaults(kernel, which, k):
    _check(RC.DEF_W, RC.def_readers()[which], RC.def_values(700), k)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", RC.RANDOM_SEEDS)
def test_drop_reorder_add_promote_on_random_schemas(kernel, seed):
    import random
    wj = random_cases.random_schema(seed)
    rj = RC.mutate(wj, seed)
    w = parse_schema(wj)
    r = random.Random(seed * 31 + 7)
    _check(wj, rj, [random_cases._rand_value(r, w) for _ in range(700)], 3)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
@pytest.mark.parametrize("k", [1, 4])
def test_chunk_semantics(kernel, n, k):
    _check(FULL, RC.FULL_MIXED, _full_values(n), k)


def _delta(c0):
    now = cabi.engine_counters()
    return {k: now[k] - c0[k] for k in now if isinstance(now[k], int)}


@pytest.mark.gpu
def test_path_ranged_pair(kernel):
    c0 = cabi.engine_counters()
    _check(FULL, RC.FULL_MIXED, _full_values(2000, "full_skewed"), 2)
    if kernel == cabi.KERNEL_SPECIALIZED:
        assert _delta(c0)["over_window_tiles"] > 0


@pytest.mark.gpu
def test_path_k0_with_size_pass(kernel):
    _check(FULL, RC.FULL_FIXED_ONLY, _full_values(1500), 3)


@pytest.mark.gpu
def test_path_k0_without_size_pass(kernel):
    _check(RC.FLAT_W, RC.FLAT_R, RC.flat_values(1500), 3)


@pytest.mark.gpu
def test_path_wide_build(kernel):
    gen = synth.gen_wide(97)
    _check(SCHEMAS["wide97"], RC.wide97_reader(), [gen(5, i) for i in range(300)], 2)


@pytest.mark.gpu
def test_path_sliding_range(kernel):
    c0 = cabi.engine_counters()
    _check(RC.SLIDE_W, RC.SLIDE_R, RC.slide_values(), 2)
    if kernel == cabi.KERNEL_SPECIALIZED:
        assert _delta(c0)["over_window_tiles"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", RC.error_cases(), ids=[c[0] for c in RC.error_cases()])
@pytest.mark.parametrize("reader", RC.ERROR_READERS)
def test_errors_are_the_plain_decodes(kernel, case, reader):
    name, wj, goods, bad, msg = case
    rj = RC.error_reader(wj, reader)
    recs = goods + [bad] + goods
    with pytest.raises(ValueError) as plain:
        P.deserialize_array_threaded(recs, wj, 2)
    with pytest.raises(ValueError) as e:
        P.deserialize_array_threaded(recs, wj, 2, reader_schema=rj)
    assert str(e.value) == str(plain.value) and msg in str(e.value)


@pytest.mark.gpu
def test_binary_array_and_columns_compose(kernel):
    import pyarrow as pa
    values = _full_values(700)
    recs = RC.writer_records(FULL, values)
    exp = _oracle(RC.reader_records(FULL, RC.FULL_MIXED, values), RC.FULL_MIXED, 3)
    _same(P.deserialize_binary_array(pa.array(recs, pa.binary()), FULL, 3, reader_schema=RC.FULL_MIXED), exp)
    cols = ["d_str", "age", "class", "d_null"]
    _same(P.deserialize_array_threaded(recs, FULL, 3, reader_schema=RC.FULL_MIXED, columns=cols), [b.select(cols) for b in exp])
    _same([P.deserialize_array(recs, FULL, reader_schema=RC.FULL_MIXED)], _oracle(RC.reader_records(FULL, RC.FULL_MIXED, values), RC.FULL_MIXED, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["sync", "async", "single_pass"])
def test_device_path(kernel, form):
    import torch
    values = _full_values(700)
    recs = RC.writer_records(FULL, values)
    rj = RC.FULL_MIXED
    exp = _oracle(RC.reader_records(FULL, rj, values), rj, 2)
    if form == "sync":
        dec = P.deserialize_to_device(recs, FULL, 2, reader_schema=rj)
        b = dec.batches[0]
        t = torch.from_dlpack(b.column("created_at").values)
        assert t.dtype == torch.float64
        assert np.array_equal(t.cpu().numpy().view(np.uint64), np.frombuffer(exp[0].column("created_at").buffers()[1], np.uint64, count=exp[0].num_rows))
        n = exp[0].num_rows
        off = torch.from_dlpack(b.column("d_str").offsets).cpu().numpy()
        assert np.array_equal(off[:n + 1], np.arange(n + 1) * 7)
        assert bytes(torch.from_dlpack(b.column("d_str").data).cpu().numpy()[:7 * n]) == b"unknown" * n
        return
    from pyruhvro_amd.device import _DevMem, _pack
    data, offs = _pack(recs)
    md = _DevMem(len(data) + 64).upload(np.ascontiguousarray(data))
    mo = _DevMem(8 * len(offs)).upload(np.ascontiguousarray(offs))
    try:
        r = cabi.decode_device(md.ptr.value, mo.ptr.value, int(offs[-1]), len(recs), FULL, 2, kernel=kernel, reader_schema=rj,
                               asynchronous=form == "async", single_pass=form == "single_pass")
        if form == "async":
            r.wait()
        _same(r.to_host(), exp)
    finally:
        md.free()
        mo.free()


@pytest.mark.gpu
def test_two_logical_shards_on_one_device(kernel):
    values = _full_values(900)
    recs = RC.writer_records(FULL, values)
    exp = _oracle(RC.reader_records(FULL, RC.FULL_MIXED, values), RC.FULL_MIXED, 4)
    old = P.set_devices([0, 0])
    try:
        _same(P.deserialize_array_threaded(recs, FULL, 4, reader_schema=RC.FULL_MIXED), exp)
    finally:
        P.set_devices(old)


@pytest.mark.gpu
def test_kernels_ready_and_prebuild_of_a_resolved_pair():
    # (through the ctypes wrapper: once `pyruhvro_amd.prebuild`, the module, has been imported it shadows the package's function)
    assert cabi.prebuild(FULL, reader_schema=RC.FULL_MIXED) is True          # scripts/known_schemas.py compiled it: nothing to do
    assert P.kernels_ready(FULL, timeout_ms=60000, reader_schema=RC.FULL_MIXED) is True
