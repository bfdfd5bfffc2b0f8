"""Row filters on the GPU: ``where=W`` decodes only the records that match.

The contract, for every writer schema S, record list, k and predicate W the front end accepts:

    decode(recs, S, k, where=W, **kw) == decode([recs[i] for i in range(n) if keep_W(value_i)], S, k, **kw)      buffer for buffer

The expected value is always the ORACLE's: its decode of the records that a Python evaluation of the oracle's full decode keeps
(tests/filter_cases.py) -- never the engine's own unfiltered decode.  A malformed record raises the plain decode's message for the
lowest failing record of the whole list, whatever the predicate says about it."""
import json

import numpy as np
import pytest

import cases
import filter_cases as FC
import resolve_cases as RC
from arrow_compare import assert_batches_identical
from avrogen import synth
from avrogen.encoder import to_datum
from avrogen.schemas import SCHEMAS
from oracle import c_walker
from oracle.avro_schema import parse_schema
from test_projection import error_projection_cases

import pyruhvro_amd as P
from pyruhvro_amd import cabi

pytestmark = pytest.mark.gpu

KERNELS = {"generic": cabi.KERNEL_GENERIC, "specialized": cabi.KERNEL_SPECIALIZED}
FULL = SCHEMAS["full"]


@pytest.fixture(autouse=True)
def _generic_unless_asked():
    """The filter has one kernel form; the decode behind it runs on the generic kernels here, so that no schema of this file needs
    a specialised kernel compiled (the two schemas that have theirs prebuilt take the `kernel` fixture)."""
    old = P.set_kernel_mode("generic")
    yield
    P.set_kernel_mode(old)


@pytest.fixture(params=sorted(KERNELS))
def kernel(request, _generic_unless_asked):
    old = P.set_kernel_mode(request.param)
    yield KERNELS[request.param]
    P.set_kernel_mode(old)


def _same(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        g.validate(full=True)
        assert g.schema.equals(e.schema, check_metadata=True)
        assert_batches_identical(g, e)


def _check(recs, schema, where, k, mask=None):
    recs = list(recs)
    if mask is None:
        mask = FC.oracle_mask(recs, schema, where)
    got_mask = P.filter_records(recs, schema, where)
    assert got_mask.dtype == np.bool_ and got_mask.shape == (len(recs),)
    assert np.array_equal(got_mask, mask), np.flatnonzero(got_mask != mask)[:10]
    _same(P.deserialize_array_threaded(recs, schema, k, where=where), FC.oracle_filtered(recs, schema, where, k, mask))
    return mask


# ---- every kind x operator over the edge values ------------------------------------------------------------------------------------
KINDS_N = 257


@pytest.mark.parametrize("field,kind,form", FC.KINDS_FIELDS, ids=[f[0] for f in FC.KINDS_FIELDS])
def test_every_kind_and_operator_over_the_edge_values(field, kind, form):
    recs = list(FC.kinds_records(KINDS_N))
    full = FC.oracle_decode(recs, FC.KINDS_SCHEMA, 1)[0]
    col = full.column(field)
    import pyarrow as pa
    if pa.types.is_temporal(col.type):
        col = col.cast(pa.int32() if col.type.bit_width == 32 else pa.int64())
    vals = col.to_pylist()
    seen = set()
    for op in FC.KIND_OPS[kind] + ("is_null", "not_null"):
        comparands = [None] if op.endswith("null") else FC.KIND_COMPARANDS[kind]
        for j, k in enumerate(comparands):
            where = (field, op) if k is None else (field, op, k)
            exp = np.array([FC.value_keeps(v, op, k) for v in vals], dtype=bool)
            got = P.filter_records(recs, FC.KINDS_SCHEMA, where)
            assert np.array_equal(got, exp), (where, np.flatnonzero(got != exp)[:8])
            seen.add(int(exp.sum()))
            if j == 0:      # the decode behind one comparand per operator
                _same(P.deserialize_array_threaded(recs, FC.KINDS_SCHEMA, 2, where=where),
                      FC.oracle_filtered(recs, FC.KINDS_SCHEMA, where, 2, exp))
    assert len(seen) > 2      # (the cases are no all-or-nothing masks)
    if form == "plain":
        assert not P.filter_records(recs, FC.KINDS_SCHEMA, (field, "is_null")).any()
        assert P.filter_records(recs, FC.KINDS_SCHEMA, (field, "not_null")).all()


def test_a_null_fails_every_comparison_not_equal_included():
    recs = list(FC.kinds_records(KINDS_N))
    nulls = ~FC.oracle_mask(recs, FC.KINDS_SCHEMA, ("long_null_first", "not_null"))
    assert nulls.any()
    for op in FC.ORDERED:
        assert not (P.filter_records(recs, FC.KINDS_SCHEMA, ("long_null_first", op, 5)) & nulls).any()
    nan = P.filter_records(recs, FC.KINDS_SCHEMA, ("double_plain", "!=", float("nan")))
    assert nan.all()
    assert not P.filter_records(recs, FC.KINDS_SCHEMA, ("double_plain", "==", float("nan"))).any()
    zero = P.filter_records(recs, FC.KINDS_SCHEMA, ("double_plain", "==", 0.0))
    assert np.array_equal(zero, FC.oracle_mask(recs, FC.KINDS_SCHEMA, ("double_plain", "==", -0.0))) and zero.sum() >= 2


# ---- the two prebuilt schemas on both kernel forms ----------------------------------------------------------------------------------
def test_full_on_both_kernel_forms(kernel):
    recs = synth.records("full", 1500)
    for where, k in ((("age", ">=", 50), 3), ([("age", "not_null"), ("class", "==", "B"), ("created_at", ">", 1_741_000_000)], 8),
                     (("name", "<", "h"), 1), (("age", "is_null"), 4)):
        mask = _check(recs, FULL, where, k)
        assert 0 < mask.sum() < len(recs)


def test_nullable_primitives_on_both_kernel_forms(kernel):
    recs = synth.records("nullable_primitives", 1000)
    s = SCHEMAS["nullable_primitives"]
    for where, k in ((("i", ">", 300), 2), (("s", ">=", "row-5"), 3), (("b", "==", True), 1), ([("d", "<=", 1000.5), ("l", "!=", 28)], 5),
                     (("s", "is_null"), 2)):
        mask = _check(recs, s, where, k)
        assert 0 < mask.sum() < len(recs)


# ---- sizes x masks: wavefront and tile edges, misaligned gathers -----------------------------------------------------------------
ONE_STRING = json.dumps({"type": "record", "name": "S1", "fields": [{"name": "s", "type": "string"}]})
MASKS = ("all", "none", "first", "last", "alternating", "run")


def _mask(n, which):
    i = np.arange(n)
    return {"all": i >= 0, "none": i < 0, "first": i == 0, "last": i == n - 1, "alternating": i % 2 == 0, "run": (i >= 250) & (i < 262)}[which]


def _one_string_records(n, mask):
    """Records of 1 to 40 bytes and a few over 64: a dropped record is the empty string (1 byte) or starts with 'd', a kept one
    starts with 'k' -- the predicate is s >= "k"."""
    s = parse_schema(ONE_STRING)
    out = []
    for i in range(n):
        ln = 64 + i % 90 if i % 29 == 7 else (i * 7) % 39
        text = ("k" + "x" * ln) if mask[i] else ("" if i % 3 == 0 else "d" + "y" * ln)
        out.append(to_datum(s, {"s": text[:39] if ln < 64 else text}))
    return out


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1024])
def test_sizes_and_masks(n):
    for which in MASKS:
        mask = _mask(n, which)
        recs = _one_string_records(n, mask)
        where = ("s", ">=", "k")
        if n:
            lens = [len(r) for r in recs]
            assert min(lens) >= 1 and (n < 64 or max(lens) > 64)
        got = P.filter_records(recs, ONE_STRING, where)
        assert np.array_equal(got, mask), (n, which)
        assert np.array_equal(FC.oracle_mask(recs, ONE_STRING, where), mask)
        for k in (1, 3):
            _same(P.deserialize_array_threaded(recs, ONE_STRING, k, where=where), FC.oracle_filtered(recs, ONE_STRING, where, k, mask))
        last = cabi.filter_last()
        assert last["n"] == n and last["kept"] == int(mask.sum())


def test_nothing_kept_is_the_decode_of_the_empty_list():
    recs = synth.records("full", 300)
    got = P.deserialize_array_threaded(recs, FULL, 4, where=("age", ">", 1000))
    _same(got, c_walker.decode_threaded([], FULL, 4))
    assert len(got) == 1 and got[0].num_rows == 0
    _same([P.deserialize_array(recs, FULL, where=("age", ">", 1000))], c_walker.decode_threaded([], FULL, 1))


# ---- a tile past the LDS window: the walk from global memory evaluates the predicate ---------------------------------------------
@pytest.mark.parametrize("window", [None, 8192])
def test_tiles_past_the_lds_window(window, monkeypatch):
    schema, recs = cases.long_string_case()
    if window:
        monkeypatch.setenv("RUHVRO_HIP_WIN_BYTES", str(window))
    if window:      # every full tile is larger than the window: walked from global memory
        assert min(sum(len(r) for r in recs[i:i + 256]) for i in range(0, len(recs) - 255, 256)) > window
    for where in (("a", ">=", "P"), [("b", "not_null"), ("z", "<", "a")], ("b", "==", ""), [("a", "!=", ""), ("z", ">", "0"), ("b", "<", "~")]):
        mask = _check(recs, schema, where, 3)
        assert 0 < mask.sum() < len(recs)


# ---- chunking, term counts, a range ----------------------------------------------------------------------------------------------
def test_chunking_applies_to_the_kept_records():
    recs = synth.records("full", 700)
    where = [("age", ">=", 30), ("age", "<", 45)]      # a range on one field
    mask = FC.oracle_mask(recs, FULL, where)
    kept = int(mask.sum())
    assert 5 < kept < 700
    for k in (1, 3, kept, kept + 5):
        got = P.deserialize_array_threaded(recs, FULL, k, where=where)
        assert len(got) == min(max(k, 1), kept)
        _same(got, FC.oracle_filtered(recs, FULL, where, k, mask))
    _same(P.deserialize_array_threaded_spawn(recs, FULL, 3, where=where), FC.oracle_filtered(recs, FULL, where, 3, mask))
    _same([P.deserialize_array(recs, FULL, where=where)], FC.oracle_filtered(recs, FULL, where, 1, mask))


def test_two_and_eight_terms():
    recs = synth.records("full", 900)
    two = [("age", "not_null"), ("class", "!=", "A")]
    eight = [("age", ">=", 20), ("age", "<=", 75), ("age", "!=", 33), ("name", "not_null"), ("name", ">", "b"), ("name", "<", "y"),
             ("created_at", ">=", 1_726_000_000), ("class", "!=", "C")]
    for where in (two, eight):
        mask = _check(recs, FULL, where, 4)
        assert 0 < mask.sum() < len(recs)


# ---- composition -------------------------------------------------------------------------------------------------------------------
def test_columns_without_the_predicate_field():
    recs = synth.records("full", 800)
    where, cols = [("age", ">=", 40), ("class", "==", "A")], ["created_at", "name", "emails"]
    exp = [b.select(cols) for b in FC.oracle_filtered(recs, FULL, where, 3)]
    assert 0 < sum(b.num_rows for b in exp) < 800
    _same(P.deserialize_array_threaded(recs, FULL, 3, columns=cols, where=where), exp)


def test_a_reader_schema_that_drops_the_predicate_field():
    values = RC.def_values(600)
    recs = RC.writer_records(RC.DEF_W, values)
    reader = RC.make_reader(RC.DEF_W, keep=["name", "id"], add=[(1, RC.ADD_ALL[2])])
    where = [("n", ">=", 100), ("n", "<", 400)]
    mask = FC.oracle_mask(recs, RC.DEF_W, where)
    assert mask.sum() == 300
    kept_values = [v for v, m in zip(values, mask) if m]
    exp = c_walker.decode_threaded(RC.reader_records(RC.DEF_W, reader, kept_values), reader, 4)
    _same(P.deserialize_array_threaded(recs, RC.DEF_W, 4, reader_schema=reader, where=where), exp)
    # ... and with columns= of the reader on top
    _same(P.deserialize_array_threaded(recs, RC.DEF_W, 4, reader_schema=reader, columns=["id"], where=where), [b.select(["id"]) for b in exp])


def test_binary_array_and_device_forms():
    import pyarrow as pa
    import torch
    recs = synth.records("full", 1000)
    where = [("age", "<", 60), ("class", "!=", "B")]
    mask = FC.oracle_mask(recs, FULL, where)
    exp = FC.oracle_filtered(recs, FULL, where, 3, mask)
    _same(P.deserialize_binary_array(pa.array(recs, type=pa.binary()), FULL, 3, where=where), exp)
    _same(P.deserialize_binary_array(pa.array(recs, type=pa.large_binary()), FULL, 3, where=where), exp)
    dec = P.deserialize_to_device(recs, FULL, 3, where=where)
    assert dec.kept == int(mask.sum())
    assert [b.num_rows for b in dec.batches] == [e.num_rows for e in exp]
    for b, e in zip(dec.batches, exp):
        t = torch.from_dlpack(b.column("created_at").values)
        assert t.dtype == torch.int64 and t.cpu().numpy().tolist() == e.column("created_at").to_pylist()
    _same(dec.to_host(), exp)
    # the C ABI's slice form and device form
    data, offsets = c_walker.pack(recs)
    ptrs = np.array([data.ctypes.data + int(o) for o in offsets[:-1]], dtype=np.uint64)
    lens = np.diff(offsets).astype(np.uint64)
    _same(cabi.decode_slices(ptrs, lens, FULL, 3, kernel=cabi.KERNEL_GENERIC, where=where), exp)
    d_data = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda:0")
    d_data[: len(data)].copy_(torch.from_numpy(data.copy()))
    d_off = torch.from_numpy(offsets.view(np.int64).copy()).to("cuda:0")
    torch.cuda.synchronize()
    got = cabi.filter_device(d_data.data_ptr(), d_off.data_ptr(), int(offsets[-1]), len(recs), FULL, where, device=0)
    assert np.array_equal(got, mask)


def test_the_refusals_of_the_filtered_calls():
    recs = synth.records("full", 64)
    data, offsets = c_walker.pack(recs)
    with pytest.raises(ValueError, match="where: .*devices"):
        cabi.decode_packed(data, offsets, FULL, 2, devices=[0, 0], where=("age", ">", 1))
    with pytest.raises(ValueError, match="where: .*RH_ASYNC"):
        cabi.decode_device(0, 0, 0, 0, FULL, 1, asynchronous=True, where=("age", ">", 1))
    with pytest.raises(ValueError, match="where: .*another writer schema"):
        import ctypes as C
        s = cabi.Schema.get(SCHEMAS["nullable_primitives"])
        f = cabi.Filter.get(FULL, ("age", ">", 1))
        arr, out_k, err = (cabi.ArrowArray * 2)(), C.c_uint32(), C.c_char_p()
        opts, _k = cabi.make_opts()
        rc = cabi._filter_sym("rh_decode_packed_where")(s.handle, data.ctypes.data, offsets.ctypes.data, len(recs), 2, C.byref(opts), arr,
                                                        C.byref(out_k), None, C.byref(err), f.handle, None)
        assert rc == cabi.RH_ERR_ARGUMENT
        cabi._raise(rc, err)


# ---- errors: the strict call's message for the lowest bad record, whatever the predicate says ------------------------------------
ERRORS = error_projection_cases()


@pytest.mark.parametrize("name,schema,goods,bad,message", ERRORS, ids=[c[0] for c in ERRORS])
def test_a_malformed_record_raises_the_strict_message(name, schema, goods, bad, message):
    n = 300
    base = [goods[i % len(goods)] for i in range(n)]
    keep_all, drop_all = ("zz_tail", "==", 7), ("zz_tail", "!=", 7)
    for at in (0, n // 2, n - 1):
        recs = list(base)
        recs[at] = bad
        with pytest.raises(ValueError) as strict:
            P.deserialize_array_threaded(recs, schema, 2)
        assert str(strict.value) == message
        for where in (keep_all, drop_all):      # the neighbours kept, the neighbours dropped
            for f in (lambda: P.deserialize_array_threaded(recs, schema, 2, where=where), lambda: P.filter_records(recs, schema, where),
                      lambda: P.deserialize_array(recs, schema, columns=["zz_tail"], where=where)):
                with pytest.raises(ValueError) as e:
                    f()
                assert str(e.value) == message, (at, where)


FLAT_ERRORS = [c for c in ERRORS if c[0] in ("bad_bool", "eob_f32", "neg_strlen", "eob_string")]


@pytest.mark.parametrize("name,schema,goods,bad,message", FLAT_ERRORS, ids=[c[0] for c in FLAT_ERRORS])
def test_a_malformed_record_whose_predicate_field_is_readable(name, schema, goods, bad, message):
    """The bad record's first field (`i` = 1) is intact: a predicate on it would keep the record, another would drop it.  Either
    way the record fails the call -- the walk is the full careful walk of every record."""
    recs = [goods[0]] * 100 + [bad] + [goods[0]] * 99
    for where in (("i", "==", 1), ("i", "!=", 1), ("i", ">", 5)):
        with pytest.raises(ValueError) as e:
            P.deserialize_array_threaded(recs, schema, 3, where=where)
        assert str(e.value) == message


def test_two_bad_records_give_the_lower_one():
    by_name = {c[0]: c for c in ERRORS}
    _, schema, goods, bad_bool, msg_bool = by_name["bad_bool"]
    _, _, _, bad_f32, msg_f32 = by_name["eob_f32"]
    recs = [goods[0]] * 600
    recs[411], recs[97] = bad_bool, bad_f32
    for where in (("zz_tail", "==", 7), ("zz_tail", "<", 0)):
        with pytest.raises(ValueError) as e:
            P.deserialize_array_threaded(recs, schema, 2, where=where)
        assert str(e.value) == msg_f32
    recs[97], recs[411] = bad_bool, bad_f32
    with pytest.raises(ValueError) as e:
        P.filter_records(recs, schema, ("zz_tail", "==", 7))
    assert str(e.value) == msg_bool
    # more malformed records than the kernel lists: the lowest one all the same
    many = [bad_bool if i % 3 == 1 else goods[0] for i in range(600)]
    many[1] = bad_f32
    with pytest.raises(ValueError) as e:
        P.deserialize_array_threaded(many, schema, 2, where=("zz_tail", "==", 7))
    assert str(e.value) == msg_f32


# ---- everything kept: the strict road, untouched ----------------------------------------------------------------------------------
def test_everything_kept_decodes_the_input_where_it_is(kernel):
    import torch
    recs = synth.records("full", 2000)
    data, offsets = c_walker.pack(recs)
    exp = c_walker.decode_threaded(recs, FULL, 4)
    d_data = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda:0")
    d_data[: len(data)].copy_(torch.from_numpy(data.copy()))
    d_off = torch.from_numpy(offsets.view(np.int64).copy()).to("cuda:0")
    torch.cuda.synchronize()

    def call(**kw):
        r = cabi.decode_device(d_data.data_ptr(), d_off.data_ptr(), int(offsets[-1]), len(recs), FULL, 4, device=0, kernel=kernel, **kw)
        try:
            return r.to_host(), r.kept
        finally:
            r.free()
    call()      # (a schema's first call is laid out on the host: not the call to compare)
    c0 = cabi.engine_counters()
    plain, _ = call()
    c1 = cabi.engine_counters()
    got, kept = call(where=("created_at", ">", 0))
    c2 = cabi.engine_counters()
    assert kept == 2000
    _same(plain, exp)
    _same(got, exp)
    d_plain = {k: c1[k] - c0[k] for k in c0}
    d_where = {k: c2[k] - c1[k] for k in c0}
    for k in ("fused_calls", "two_sync_calls", "capacity_retries", "wide_fallbacks", "split_calls", "single_pass_calls", "tiles", "careful_tiles",
              "over_window_tiles", "rewalked_waves", "tolerant_calls", "tolerant_repairs"):
        assert d_where[k] == d_plain[k], (k, d_plain, d_where)
    last = cabi.filter_last()
    assert last["n"] == 2000 and last["kept"] == 2000 and last["gather_ms"] == 0 and last["filter_ms"] > 0
    # one record dropped: the gather ran
    cabi.decode_packed(data, offsets, FULL, 4, kernel=kernel, where=("created_at", "!=", int(exp[0].column("created_at")[0].as_py())))
    last = cabi.filter_last()
    assert 0 < last["kept"] < 2000 and last["gather_ms"] > 0
