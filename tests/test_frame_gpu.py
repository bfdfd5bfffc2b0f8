"""Framed messages on the GPU: ``deserialize_framed`` splits Kafka-framed Avro by writer schema id and decodes every group.

The contract, for every group g of the result:

    g.batches == deserialize_array_threaded([messages[i][h:] for i in g.indices], g.schema, k, columns=..., reader_schema=...)      buffer for buffer

with g.indices exactly the ascending positions whose header carries g.id.  The expected value is always plain Python's
(``int.from_bytes`` on the header, tests/frame_cases.py) and the ORACLE's decode of the stripped payloads -- never anything the engine
returns."""
import json

import numpy as np
import pyarrow as pa
import pytest

import cases
import frame_cases as FR
import resolve_cases as RC
from arrow_compare import assert_batches_identical
from avrogen import synth
from avrogen.encoder import to_datum
from avrogen.schemas import SCHEMAS
from oracle import c_walker
from oracle.avro_schema import parse_schema

import pyruhvro_amd as P
from pyruhvro_amd import cabi

pytestmark = pytest.mark.gpu

KERNELS = {"generic": cabi.KERNEL_GENERIC, "specialized": cabi.KERNEL_SPECIALIZED}
FULL = SCHEMAS["full"]


@pytest.fixture(autouse=True)
def _generic_unless_asked():
    """The split has one kernel form; the decodes behind it run on the generic kernels here, so that no schema of this file needs a
    specialised kernel compiled (the one test on `full`, whose kernels the build prebuilds, takes the `kernel` fixture)."""
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


def _check(messages, schemas, framing, k, unknown="raise", decode=None, **kw):
    """One framed call against the contract; returns the result."""
    res = P.deserialize_framed(messages, schemas, k, framing=framing, unknown=unknown, **kw)
    exp, (unk_i, unk_id) = FR.expected_groups(messages, schemas, framing, k, decode)
    assert len(res.groups) == len(exp) == len(schemas)
    seen = []
    for g, (wire, text, idx, batches) in zip(res.groups, exp):
        assert g.id == wire and g.schema == text
        assert g.indices.dtype == np.int64 and np.array_equal(g.indices, idx), (wire, g.indices[:8], idx[:8])
        _same(g.batches, batches)
        assert sum(b.num_rows for b in g.batches) == len(idx)
        seen.append(g.indices)
    assert res.unknown_indices.dtype == np.int64 and np.array_equal(res.unknown_indices, unk_i)
    assert np.array_equal(np.asarray(res.unknown_ids, dtype=np.uint64), unk_id)
    allidx = np.sort(np.concatenate(seen + [res.unknown_indices]))
    assert np.array_equal(allidx, np.arange(len(messages)))      # the groups and the unknowns partition range(n)
    return res


# ---- partition edges ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", FR.CLASS_COUNTS)
@pytest.mark.parametrize("framing", FR.FRAMINGS)
@pytest.mark.parametrize("n", [n for n in FR.SIZES if n > 0])
def test_partition_edges(n, framing, m):
    for pattern in FR.PATTERNS:
        msgs, ids = FR.pattern_messages(framing, n, m, pattern)
        exp_cls = FR.classify(msgs, ids, framing)
        got = P.frame_split(msgs, ids, framing=framing)
        assert got.dtype == np.int16 and got.shape == (n,)
        assert np.array_equal(got, exp_cls), (pattern, np.flatnonzero(got != exp_cls)[:10])
        last = cabi.frame_last()
        assert last["n"] == n and last["classify_ms"] > 0 and last["gather_ms"] == 0
        unknown = "skip" if (exp_cls < 0).any() else "raise"
        for k in (1, 3):
            _check(msgs, FR.schemas_for(ids), framing, k, unknown=unknown)
        assert cabi.frame_last()["gather_ms"] > 0


@pytest.mark.parametrize("framing", FR.FRAMINGS)
def test_no_messages_give_m_empty_groups(framing):
    for m in FR.CLASS_COUNTS:
        ids = FR.id_list(framing, m)
        schemas = FR.schemas_for(ids)
        for k in (1, 3):
            res = _check([], schemas, framing, k)
            assert [g.id for g in res.groups] == sorted(ids)
            for g in res.groups:
                assert len(g.indices) == 0
                _same(g.batches, c_walker.decode_threaded([], g.schema, k))
        got = P.frame_split([], ids, framing=framing)
        assert got.dtype == np.int16 and got.shape == (0,)


# ---- id byte order and width -----------------------------------------------------------------------------------------------------------
def test_confluent_ids_are_big_endian_and_32_bits_wide():
    da, db = FR._datums(400)
    ids = [1, 0x01000000, 0x80000000, 0xFFFFFFFF, 0x7FFFFFFF, 0]      # 1 and 0x01000000: the same bytes in the other order
    schemas = FR.schemas_for(ids)
    order = sorted(ids)
    msgs = [FR.frame("confluent", order[(i * 5) % 6], (da, db)[((i * 5) % 6) % 2][i]) for i in range(400)]
    assert msgs[1][:5] == b"\x00" + order[5].to_bytes(4, "big")
    res = _check(msgs, schemas, "confluent", 2)
    assert [g.id for g in res.groups] == order and all(len(g.indices) for g in res.groups)
    assert np.array_equal(P.frame_split(msgs, ids), FR.classify(msgs, ids, "confluent"))
    # only one of the two byte orders is in schemas: the other is unknown
    res = _check(msgs, {1: schemas[1]}, "confluent", 1, unknown="skip")
    assert set(res.unknown_ids.tolist()) == set(order) - {1}


def test_single_object_fingerprints_are_little_endian_and_64_bits_wide():
    da, db = FR._datums(300)
    fa, fb = P.schema_fingerprint(FR.SCHEMA_A), P.schema_fingerprint(FR.SCHEMA_B)
    assert fa != fb
    # the real fingerprints of the two schemas, and neighbours that differ from them in one end byte only
    schemas = {fa: FR.SCHEMA_A, fb: FR.SCHEMA_B, fa ^ 1: FR.SCHEMA_A, fa ^ (1 << 63): FR.SCHEMA_A, fb ^ (0x80 << 56): FR.SCHEMA_B, fb ^ 0x80: FR.SCHEMA_B}
    wire = list(schemas)
    msgs = [FR.frame("single_object", wire[i % 6], (da if schemas[wire[i % 6]] == FR.SCHEMA_A else db)[i]) for i in range(300)]
    assert msgs[0][2:10] == fa.to_bytes(8, "little")
    res = _check(msgs, schemas, "single_object", 3)
    assert all(len(g.indices) == 50 for g in res.groups)
    # Java's signed fingerprints: a negative key is its unsigned twin
    signed = {(w - (1 << 64) if w >= 1 << 63 else w): s for w, s in schemas.items()}
    assert any(w < 0 for w in signed)
    res2 = P.deserialize_framed(msgs, signed, 3, framing="single_object")
    assert [g.id for g in res2.groups] == [g.id for g in res.groups]
    for a, b in zip(res2.groups, res.groups):
        assert np.array_equal(a.indices, b.indices)
        _same(a.batches, b.batches)
    # frame_split: positions in sorted(ids) as they were given, negative keys first
    keys = list(signed)
    pos = {k: p for p, k in enumerate(sorted(keys))}
    exp = np.array([pos[keys[i % 6]] for i in range(300)], dtype=np.int16)
    assert np.array_equal(P.frame_split(msgs, keys, framing="single_object"), exp)


# ---- payload edges for the gather ------------------------------------------------------------------------------------------------------
NULLS = json.dumps({"type": "record", "name": "Nn", "fields": [{"name": "a", "type": "null"}, {"name": "b", "type": "null"}]})


@pytest.mark.parametrize("framing", FR.FRAMINGS)
def test_a_datum_of_zero_bytes_is_the_bare_header(framing):
    """No oracle decodes a record of `null` fields (the reference's gate refuses it): the expected batches are plain pyarrow."""
    da, _ = FR._datums(300)
    msgs = [FR.frame(framing, 9, b"") if i % 3 else FR.frame(framing, 4, da[i]) for i in range(300)]
    assert min(len(m) for m in msgs) == FR.HEADER[framing]

    def decode(recs, schema, k):
        if schema != NULLS:
            return c_walker.decode_threaded(recs, schema, k)
        assert all(r == b"" for r in recs)
        n = len(recs)
        kk = min(max(k, 1), max(n, 1))
        rows = [n // kk] * (kk - 1) + [n - (n // kk) * (kk - 1)]
        return [pa.RecordBatch.from_arrays([pa.nulls(r), pa.nulls(r)], names=["a", "b"]) for r in rows]
    for k in (1, 3):
        res = P.deserialize_framed(msgs, {9: NULLS, 4: FR.SCHEMA_A}, k, framing=framing)
        exp, _unk = FR.expected_groups(msgs, {9: NULLS, 4: FR.SCHEMA_A}, framing, k, decode)
        for g, (wire, text, idx, batches) in zip(res.groups, exp):
            assert g.id == wire and np.array_equal(g.indices, idx)
            assert [b.num_rows for b in g.batches] == [b.num_rows for b in batches]
            if text == NULLS:
                for b in g.batches:
                    assert b.schema.names == ["a", "b"] and all(pa.types.is_null(c.type) and len(c) == b.num_rows for c in b.columns)
            else:
                _same(g.batches, batches)
    # every message the bare header
    bare = [FR.frame(framing, 9, b"")] * 257
    res = P.deserialize_framed(bare, {9: NULLS}, 2, framing=framing)
    assert np.array_equal(res.groups[0].indices, np.arange(257)) and [b.num_rows for b in res.groups[0].batches] == [128, 129]


@pytest.mark.parametrize("framing", FR.FRAMINGS)
def test_payloads_around_the_vector_width_in_one_tile(framing):
    s = parse_schema(FR.SCHEMA_A)
    lens = [1, 15, 16, 17, 31, 33, 4096]
    payloads = [to_datum(s, {"s": "".join(chr(97 + (j * 7 + L) % 26) for j in range(L - 1 if L < 65 else L - 2))}) for L in lens]
    assert [len(p) for p in payloads] == lens
    ids = [7, 8, 9]
    schemas = {w: FR.SCHEMA_A for w in ids}
    for shift in range(3):
        msgs = [FR.frame(framing, ids[(i + shift) % 3 if i % 5 else 0], payloads[(i * 3 + shift) % 7]) for i in range(200)]
        _check(msgs, schemas, framing, 1 + shift)


def test_seventy_thousand_messages_over_three_ids():
    """More than 256 tiles: the scan of the tile tables crosses its own block edge.  Lengths from avrogen.synth."""
    base = synth.records("full", 2000)
    n = 70_000
    assert (n + 255) // 256 > 256
    ids = [3, 0x01000000, 0xFFFFFFF0]
    msgs = [FR.frame("confluent", ids[(i * i + i // 300) % 3], base[i % 2000]) for i in range(n)]
    res = _check(msgs, {w: FULL for w in ids}, "confluent", 4)
    assert min(len(g.indices) for g in res.groups) > 20_000
    assert cabi.frame_last()["n"] == n


# ---- errors -----------------------------------------------------------------------------------------------------------------------------
def _raises(message, f):
    with pytest.raises(ValueError) as e:
        f()
    assert str(e.value) == message, (str(e.value), message)


def _good(framing, n, ids):
    da, db = FR._datums(max(n, 1))
    order = sorted(ids)
    return [FR.frame(framing, order[i % len(ids)], (da, db)[(i % len(ids)) % 2][i]) for i in range(n)]


@pytest.mark.parametrize("framing", FR.FRAMINGS)
def test_framing_failures(framing):
    h = FR.HEADER[framing]
    ids = FR.id_list(framing, 3)
    schemas = FR.schemas_for(ids)
    n = 600
    good = _good(framing, n, ids)
    ok = good[5]
    bad = {"empty": b"", "one byte": ok[:1], "header less one": ok[:h - 1], "first marker byte": bytes([ok[0] ^ 0x01]) + ok[1:],
           "unknown id": FR.frame(framing, FR.unknown_id(framing, 1), ok[h:])}
    if framing == "single_object":
        bad["second marker byte"] = ok[:1] + b"\x02" + ok[2:]
    for what, msg in bad.items():
        for at in (0, n - 1, 255, 256, 300):      # the first, the last, either side of a tile edge
            msgs = list(good)
            msgs[at] = msg
            message = FR.framing_error(msgs, ids, framing)
            assert message is not None and message.startswith(f"framed: message {at} "), (what, message)
            _raises(message, lambda: P.deserialize_framed(msgs, schemas, 2, framing=framing))
            if what == "unknown id":      # skipped and reported; frame_split says -1
                res = _check(msgs, schemas, framing, 2, unknown="skip")
                assert res.unknown_indices.tolist() == [at] and res.unknown_ids.tolist() == [FR.unknown_id(framing, 1)]
                assert P.frame_split(msgs, ids, framing=framing)[at] == -1
            else:                         # short or mis-marked messages raise whatever `unknown` says
                _raises(message, lambda: P.deserialize_framed(msgs, schemas, 2, framing=framing, unknown="skip"))
                _raises(message, lambda: P.frame_split(msgs, ids, framing=framing))
    assert FR.framing_error(good, ids, framing) is None


@pytest.mark.parametrize("framing", FR.FRAMINGS)
def test_two_failures_in_one_list_the_lower_index_wins(framing):
    h = FR.HEADER[framing]
    ids = FR.id_list(framing, 2)
    schemas = FR.schemas_for(ids)
    good = _good(framing, 700, ids)
    short, marker = good[0][:h - 2], b"\x55" + good[0][1:]
    unknown = FR.frame(framing, FR.unknown_id(framing, 0), good[0][h:])
    for lo, hi in ((97, 411), (255, 256), (3, 699)):
        for a, b in ((short, marker), (marker, short), (unknown, short), (short, unknown), (marker, unknown), (unknown, marker)):
            msgs = list(good)
            msgs[lo], msgs[hi] = a, b
            message = FR.framing_error(msgs, ids, framing)
            assert message.startswith(f"framed: message {lo} ")
            _raises(message, lambda: P.deserialize_framed(msgs, schemas, 3, framing=framing))
            # with the unknown ids skipped, the lowest of the OTHER failures decides
            skipped = FR.framing_error(msgs, ids, framing, unknown="skip")
            assert skipped.startswith(f"framed: message {hi if a is unknown else lo} ")
            _raises(skipped, lambda: P.deserialize_framed(msgs, schemas, 3, framing=framing, unknown="skip"))


def test_a_truncated_payload_in_the_second_of_three_groups():
    by_name = {c[0]: c for c in cases.error_cases()}
    _, flat, goods, bad, _msg = by_name["eob_string"]
    da, _db = FR._datums(300)
    ids = [10, 20, 30]
    schemas = {10: FR.SCHEMA_A, 20: flat, 30: FR.SCHEMA_A}
    msgs = [FR.frame("confluent", ids[i % 3], goods[0] if i % 3 == 1 else da[i]) for i in range(300)]
    msgs[151] = FR.frame("confluent", 20, bad)
    second = [m[5:] for i, m in enumerate(msgs) if i % 3 == 1]
    with pytest.raises(ValueError) as oracle:
        c_walker.decode_threaded(second, flat, 2)
    with pytest.raises(ValueError) as strict:
        P.deserialize_array_threaded(second, flat, 2)
    assert str(strict.value) == str(oracle.value)
    _raises("framed: schema id 20: " + str(oracle.value), lambda: P.deserialize_framed(msgs, schemas, 2))
    # a framing failure behind it still comes first: framing is judged over the whole list before anything is decoded
    msgs[299] = msgs[299][:3]
    _raises("framed: message 299 is 3 bytes, shorter than the 5-byte confluent header", lambda: P.deserialize_framed(msgs, schemas, 2))


# ---- composition --------------------------------------------------------------------------------------------------------------------------
def test_two_writer_versions_under_one_reader_schema():
    """Version 1 of the record, and version 2 with a field added with a default and an `int` promoted to `long`; version 2 is the
    reader: two writer versions, one table."""
    v1 = RC.DEF_W
    v2 = RC.make_reader(RC.DEF_W, promote=lambda k: {"int": "long"}.get(k), add=[(1, RC.ADD_ALL[2])])
    assert json.loads(v2)["fields"][1]["name"] == "d_int" and json.loads(v2)["fields"][3]["type"] == "long"
    values = RC.def_values(500)
    recs1 = RC.writer_records(v1, values)
    values2 = [dict(v, d_int=7 * k - 3, n=(1 << 40) + k) for k, v in enumerate(values)]
    recs2 = RC.writer_records(v2, values2)
    pick = [(i * 7 + i // 64) % 3 != 0 for i in range(500)]      # True: version 1
    msgs = [FR.frame("confluent", 1 if p else 2, (recs1 if p else recs2)[i]) for i, p in enumerate(pick)]
    idx1 = [i for i, p in enumerate(pick) if p]
    idx2 = [i for i, p in enumerate(pick) if not p]
    for k in (1, 4):
        exp1 = c_walker.decode_threaded(RC.reader_records(v1, v2, [values[i] for i in idx1]), v2, k)
        exp2 = c_walker.decode_threaded([recs2[i] for i in idx2], v2, k)
        res = P.deserialize_framed(msgs, {1: v1, 2: v2}, k, reader_schema=v2)
        g1, g2 = res.groups
        assert g1.indices.tolist() == idx1 and g2.indices.tolist() == idx2
        _same(g1.batches, exp1)
        _same(g2.batches, exp2)
        for g in res.groups:
            assert all(b.schema.equals(P.arrow_schema(v2), check_metadata=True) for b in g.batches)
        # columns= on top of that
        cols = ["n", "d_int"]
        res = P.deserialize_framed(msgs, {1: v1, 2: v2}, k, reader_schema=v2, columns=cols)
        _same(res.groups[0].batches, [b.select(cols) for b in exp1])
        _same(res.groups[1].batches, [b.select(cols) for b in exp2])
    # columns= alone, every group its own writer schema
    res = P.deserialize_framed(msgs, {1: v1, 2: v2}, 2, columns=["id"])
    _same(res.groups[0].batches, [b.select(["id"]) for b in c_walker.decode_threaded([recs1[i] for i in idx1], v1, 2)])
    _same(res.groups[1].batches, [b.select(["id"]) for b in c_walker.decode_threaded([recs2[i] for i in idx2], v2, 2)])


def test_full_on_both_kernel_forms_two_ids_one_schema(kernel):
    recs = synth.records("full", 1100)
    ids = [41, 0x80000001]
    msgs = [FR.frame("confluent", ids[(i // 5) % 2], r) for i, r in enumerate(recs)]
    for k in (1, 8):
        res = _check(msgs, {w: FULL for w in ids}, "confluent", k)
        assert [len(g.indices) for g in res.groups] == [550, 550]


# ---- nothing else moved -------------------------------------------------------------------------------------------------------------------
COUNTERS = ("fused_calls", "two_sync_calls", "capacity_retries", "wide_fallbacks", "split_calls", "single_pass_calls", "tiles", "careful_tiles",
            "over_window_tiles", "rewalked_waves", "tolerant_calls", "tolerant_repairs")


def test_nothing_else_moved():
    import torch
    recs = synth.records("full", 1500)
    ids = [5, 6]
    msgs = [FR.frame("confluent", ids[i % 2], r) for i, r in enumerate(recs)]
    groups = [[r for i, r in enumerate(recs) if i % 2 == c] for c in range(2)]
    exp = [c_walker.decode_threaded(g, FULL, 3) for g in groups]

    def plain():      # the plain device-resident calls behind the two groups
        out = []
        for g in groups:
            data, offsets = c_walker.pack(g)
            d_data = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda:0")
            d_data[: len(data)].copy_(torch.from_numpy(data.copy()))
            d_off = torch.from_numpy(offsets.view(np.int64).copy()).to("cuda:0")
            torch.cuda.synchronize()
            r = cabi.decode_device(d_data.data_ptr(), d_off.data_ptr(), int(offsets[-1]), len(g), FULL, 3, device=0, kernel=cabi.KERNEL_GENERIC)
            try:
                out.append(r.to_host())
            finally:
                r.free()
        return out

    def framed():
        return [g.batches for g in P.deserialize_framed(msgs, {5: FULL, 6: FULL}, 3).groups]
    plain()      # (a schema's first call is laid out on the host: not the call to compare)
    c0, l0 = cabi.engine_counters(), cabi.lean_counters()
    got_plain = plain()
    c1, l1 = cabi.engine_counters(), cabi.lean_counters()
    got_framed = framed()
    c2, l2 = cabi.engine_counters(), cabi.lean_counters()
    for got in (got_plain, got_framed):
        for g, e in zip(got, exp):
            _same(g, e)
    for name in COUNTERS:
        assert c2[name] - c1[name] == c1[name] - c0[name], (name, c0[name], c1[name], c2[name])
    for name in l0:
        assert l2[name] - l1[name] == l1[name] - l0[name], (name, l0[name], l1[name], l2[name])
    # ... and an ordinary call of the same payloads still matches the oracle
    _same(P.deserialize_array_threaded(recs, FULL, 3), c_walker.decode_threaded(recs, FULL, 3))
    _same(P.deserialize_array_threaded(groups[1], FULL, 3), exp[1])


def test_the_refusals_of_the_framed_calls():
    msgs = _good("confluent", 64, [1, 2])
    old = P.set_devices([0, 0])
    try:
        with pytest.raises(ValueError, match="framed: .*one device"):
            P.deserialize_framed(msgs, FR.schemas_for([1, 2]), 2)
        with pytest.raises(ValueError, match="framed: .*one device"):
            P.frame_split(msgs, [1, 2])
    finally:
        P.set_devices(old)
    data, offsets = c_walker.pack(msgs)
    import ctypes as C
    ids = np.array([1, 2], dtype=np.uint64)
    opts, _keep = cabi.make_opts()
    opts.flags |= cabi.RH_ASYNC
    out, err = C.c_void_p(), C.c_char_p()
    rc = cabi._frame_sym("rh_frame_split_packed")(data.ctypes.data, offsets.ctypes.data, len(msgs), ids.ctypes.data, 2, 0, 0, C.byref(opts),
                                                  C.byref(out), C.byref(err))
    assert rc == cabi.RH_ERR_ARGUMENT and not out.value
    assert "RH_ASYNC" in cabi._take_err(err)
    # a class decodes once: its result owns the payloads
    sp = cabi.FrameSplit.packed(data, offsets, [1, 2], 0)
    try:
        assert sp.count(0) == sp.count(1) == 32 and sp.count(2) == 0
        _same(sp.decode(0, FR.SCHEMA_A, 2, kernel=cabi.KERNEL_GENERIC), c_walker.decode_threaded([m[5:] for m in msgs[0::2]], FR.SCHEMA_A, 2))
        with pytest.raises(ValueError, match="framed: .*decoded already"):
            sp.decode(0, FR.SCHEMA_A, 2)
    finally:
        sp.free()


def test_the_device_entry_takes_device_pointers():
    import torch
    msgs, ids = FR.pattern_messages("single_object", 700, 3, "random")
    data, offsets = c_walker.pack(msgs)
    d_data = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda:0")
    d_data[: len(data)].copy_(torch.from_numpy(data.copy()))
    d_off = torch.from_numpy(offsets.view(np.int64).copy()).to("cuda:0")
    torch.cuda.synchronize()
    sp = cabi.FrameSplit.device(d_data.data_ptr(), d_off.data_ptr(), int(offsets[-1]), len(msgs), sorted(ids), 1, cabi.FRAME_SKIP_UNKNOWN, device=0)
    try:
        schemas = FR.schemas_for(ids)
        exp, (unk_i, _unk_id) = FR.expected_groups(msgs, schemas, "single_object", 2)
        assert np.array_equal(sp.classes(), FR.classify(msgs, ids, "single_object"))
        for c, (wire, text, idx, batches) in enumerate(exp):
            assert np.array_equal(sp.indices(c), idx)
            _same(sp.decode(c, text, 2, kernel=cabi.KERNEL_GENERIC), batches)
        assert np.array_equal(sp.indices(3), unk_i)
    finally:
        sp.free()
