"""Framed writes on the GPU: ``serialize_framed`` encodes the record batches of several writer schemas, puts the datums into message
order and stamps the headers on the device.

The contract: message p of the result is ``header(framing, wire id of its group) + datum``, the datum byte for byte what
``serialize_record_batch`` produces for that row, and the arrays are cut as ``serialize_record_batch`` cuts n rows.  The expected
value is always plain Python's (``frame_cases.frame`` / ``int.to_bytes`` for the header) and the ORACLE's (``oracle.py_encoder`` for
the datums, ``oracle.c_walker`` for the batches) -- never anything the engine returns."""
import ctypes as C
import json

import numpy as np
import pyarrow as pa
import pytest

import container_cases as CC
import frame_cases as FR
from avrogen import synth
from avrogen.encoder import to_datum
from avrogen.schemas import SCHEMAS
from oracle import c_walker, py_encoder
from oracle.avro_schema import parse_schema

import pyruhvro_amd as P
from pyruhvro_amd import cabi

pytestmark = pytest.mark.gpu

KERNELS = {"generic": cabi.KERNEL_GENERIC, "specialized": cabi.KERNEL_SPECIALIZED}
FULL = SCHEMAS["full"]
SIX_PATTERNS = ("all one class", "alternating classes", "runs ending on wavefront edges", "runs ending on tile edges",
                "a class seen only in the last message", "a class never seen")


@pytest.fixture(autouse=True)
def _generic_unless_asked():
    """The join has one kernel form; the encodes in front of it run on the generic kernels here, so that no schema of this file needs
    a specialised kernel compiled (the tests on `full`, whose kernels the build prebuilds, take the `kernel` fixture)."""
    old = P.set_kernel_mode("generic")
    yield
    P.set_kernel_mode(old)


@pytest.fixture(params=sorted(KERNELS))
def kernel(request, _generic_unless_asked):
    old = P.set_kernel_mode(request.param)
    yield KERNELS[request.param]
    P.set_kernel_mode(old)


# ---- the right-hand side, in plain Python ------------------------------------------------------------------------------------------------
def _chunks(n, k):
    """[(lo, hi)]: how serialize_record_batch cuts n rows into clamp(k, 1, max(n, 1)) arrays."""
    kk = max(1, min(k, max(n, 1)))
    sz = n // kk
    return [(c * sz, n if c == kk - 1 else (c + 1) * sz) for c in range(kk)]


def _same(got, msgs, k):
    """`got` is exactly `msgs` cut by the rule: type, offsets that start at 0, a data buffer that holds the messages and nothing else."""
    cuts = _chunks(len(msgs), k)
    assert len(got) == len(cuts), (len(got), len(cuts))
    for g, (lo, hi) in zip(got, cuts):
        assert g.type == pa.binary()
        g.validate(full=True)
        assert g.null_count == 0 and g.offset == 0 and len(g) == hi - lo
        want = [bytes(m) for m in msgs[lo:hi]]
        assert g.equals(pa.array(want, type=pa.binary())), (lo, hi)
        go = np.frombuffer(g.buffers()[1], dtype=np.int32, count=len(g) + 1)
        assert np.array_equal(go, np.concatenate([[0], np.cumsum([len(m) for m in want], dtype=np.int64)]))
        data = g.buffers()[2]
        assert bytes(data)[:int(go[-1])] == b"".join(want) if data is not None else go[-1] == 0
    assert [bytes(m) for a in got for m in a.to_pylist()] == [bytes(m) for m in msgs]


def _oracle_datums(batches, schema):
    return [d for b in batches for d in py_encoder.serialize_record_batch(b, schema, 1)[0].to_pylist()]


# ---- 1. merge against the oracle ---------------------------------------------------------------------------------------------------------
def _merge(framing, n, m, pattern):
    msgs, ids = FR.pattern_messages(framing, n, m, pattern)
    exp, _unknown = FR.expected_groups(msgs, FR.schemas_for(ids), framing, 3)
    h = FR.HEADER[framing]
    for wire, text, idx, batches in exp:      # the precondition, on the oracle alone: decode then encode returns these datums
        assert _oracle_datums(batches, text) == [bytes(msgs[i][h:]) for i in idx], (pattern, wire)
    groups = [(wire, text, batches, idx) for wire, text, idx, batches in exp]
    for k in (1, 3):
        _same(P.serialize_framed(groups, k, framing=framing), msgs, k)


@pytest.mark.parametrize("framing", FR.FRAMINGS)
@pytest.mark.parametrize("n", FR.SIZES)
def test_the_merge_returns_the_messages(n, framing):
    for pattern in SIX_PATTERNS:
        _merge(framing, n, 3, pattern)
    if n:
        last = cabi.frame_join_last()
        assert last["n"] == n and last["lengths_ms"] > 0 and last["scan_ms"] > 0 and last["gather_ms"] > 0


@pytest.mark.parametrize("m", (1, 2, 32))
@pytest.mark.parametrize("n", (257, 1100))
def test_the_merge_of_1_2_and_32_groups(n, m):
    for framing in FR.FRAMINGS:
        _merge(framing, n, m, "alternating classes")


# ---- 2. engine round trip ----------------------------------------------------------------------------------------------------------------
def test_the_engine_round_trip(kernel):
    recs = synth.records("full", 1500, seed=5)
    for framing, ids in (("confluent", (7, 0x80000001)), ("single_object", (P.schema_fingerprint(FULL), 3))):
        msgs = [FR.frame(framing, ids[(i * 7 // 3) % 2], r) for i, r in enumerate(recs)]
        res = P.deserialize_framed(msgs, {ids[0]: FULL, ids[1]: FULL}, 3, framing=framing)
        assert all(len(g.indices) for g in res.groups)
        _same(P.serialize_framed(res.groups, 3, framing=framing), msgs, 3)


# ---- 3. no indices -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("full", "array_and_map", "t_union", "nullable_primitives"))
def test_one_group_one_batch_without_indices(name):
    schema = SCHEMAS[name]
    batch = c_walker.decode(list(CC.records_of(name, 1500)), schema)
    datums = _oracle_datums([batch], schema)
    assert len(datums) == 1500
    for framing, wire in (("confluent", 0x01020304), ("single_object", 0x1122334455667788)):
        msgs = [FR.frame(framing, wire, d) for d in datums]
        for k in (1, 4):
            _same(P.serialize_framed([(wire, schema, batch)], k, framing=framing), msgs, k)


def test_groups_without_indices_keep_the_given_order():
    groups, msgs = [], []
    for wire, (name, rows) in zip((9, 2, 5), (("nullable_primitives", 300), ("array_and_map", 70), ("nullable_primitives", 257))):
        batches = c_walker.decode_threaded(list(CC.records_of(name, rows)), SCHEMAS[name], 2)      # a list of two batches
        groups.append((wire, SCHEMAS[name], batches))
        msgs += [FR.frame("confluent", wire, d) for d in _oracle_datums(batches, SCHEMAS[name])]
    for k in (1, 3):
        _same(P.serialize_framed(groups, k), msgs, k)
    # a FramedGroup without indices is the same group
    _same(P.serialize_framed([P.FramedGroup(w, s, None, b) for w, s, b in groups], 2), msgs, 2)


# ---- 4. lengths and alignments -----------------------------------------------------------------------------------------------------------
def _string_of_datum_length(t):
    """The text whose SCHEMA_A datum is t bytes: the length prefix is one byte below 64 characters and two from there (so no datum
    of this schema is 65 bytes long: SCHEMA_B below covers that length)."""
    return "z" * (t - 1) if t <= 64 else "z" * (t - 2)


@pytest.mark.parametrize("framing", FR.FRAMINGS)
def test_every_datum_length_meets_every_destination_alignment(framing):
    h = FR.HEADER[framing]
    a, b = parse_schema(FR.SCHEMA_A), parse_schema(FR.SCHEMA_B)
    lengths = [t for t in range(1, 301) if t != 65]
    # 16 rounds of every length in turn; a filler in front of round r makes the round start at alignment r
    texts, at = [], 0
    for r in range(16):
        f = next(f for f in range(1, 17) if (at + h + f) % 16 == r)
        texts.append(_string_of_datum_length(f))
        at += h + f
        for t in lengths:
            texts.append(_string_of_datum_length(t))
            at += h + t
    texts.append("L" * 99_997)                                             # one datum of 100,000 bytes among them
    recs_a = [to_datum(a, {"s": t}) for t in texts]
    assert len(recs_a[-1]) == 100_000
    # SCHEMA_B: a 65-byte datum and a 2-byte one in turn, 16 times (the pair moves the destination by an odd number of bytes)
    recs_b = [to_datum(b, {"l": 0, "s": "q" * 62}) if i % 2 == 0 else to_datum(b, {"l": 0, "s": None}) for i in range(32)]
    assert len(recs_b[0]) == 65 and len(recs_b[1]) == 2
    batch_a, batch_b = c_walker.decode(recs_a, FR.SCHEMA_A), c_walker.decode(recs_b, FR.SCHEMA_B)
    da, db = _oracle_datums([batch_a], FR.SCHEMA_A), _oracle_datums([batch_b], FR.SCHEMA_B)
    assert da == recs_a and db == recs_b
    msgs = [FR.frame(framing, 11, d) for d in da] + [FR.frame(framing, 4, d) for d in db]
    met, at = set(), 0
    for m in msgs:
        met.add((at % 16, len(m) - h))
        at += len(m)
    assert {(al, t) for al in range(16) for t in range(1, 301)} <= met      # (one chunk: its data starts 16-byte aligned)
    _same(P.serialize_framed([(11, FR.SCHEMA_A, batch_a), (4, FR.SCHEMA_B, batch_b)], 1, framing=framing), msgs, 1)
    _same(P.serialize_framed([(11, FR.SCHEMA_A, batch_a), (4, FR.SCHEMA_B, batch_b)], 2, framing=framing), msgs, 2)


ONLY_NULL = json.dumps({"type": "record", "name": "OnlyNull", "fields": [{"name": "n", "type": "null"}]})
NO_FIELDS = json.dumps({"type": "record", "name": "NoFields", "fields": []})


@pytest.mark.parametrize("framing", FR.FRAMINGS)
def test_datums_of_no_bytes_give_messages_that_are_their_header_alone(framing):
    """A record schema with no fields is refused by the schema front end (as the reference refuses it), so it cannot reach the
    device: the refusal is checked, and the datums of 0 bytes come from a record whose one field is `null`."""
    plain = None
    try:
        P.serialize_record_batch(pa.RecordBatch.from_arrays([pa.nulls(3)], names=["n"]), NO_FIELDS, 1)
    except ValueError as e:
        plain = str(e)
    assert plain is not None
    with pytest.raises(ValueError) as ei:
        P.serialize_framed([(3, NO_FIELDS, pa.RecordBatch.from_arrays([pa.nulls(3)], names=["n"]))], 1, framing=framing)
    assert str(ei.value) == f"framed: schema id 3: {plain}"
    batch = pa.RecordBatch.from_arrays([pa.nulls(301)], names=["n"])
    assert _oracle_datums([batch], ONLY_NULL) == [b""] * 301
    other = c_walker.decode(list(CC.records_of("nullable_primitives", 40)), SCHEMAS["nullable_primitives"])
    msgs = [FR.frame(framing, 6, b"")] * 301 + [FR.frame(framing, 2, d) for d in _oracle_datums([other], SCHEMAS["nullable_primitives"])]
    assert all(len(m) == FR.HEADER[framing] for m in msgs[:301])
    for k in (1, 3):
        _same(P.serialize_framed([(6, ONLY_NULL, batch), (2, SCHEMAS["nullable_primitives"], other)], k, framing=framing), msgs, k)
    _same(P.serialize_framed([(6, ONLY_NULL, batch)], 2, framing=framing), msgs[:301], 2)


# ---- 5. id edges -------------------------------------------------------------------------------------------------------------------------
def test_the_header_bytes_of_every_id_edge():
    batch = c_walker.decode(list(CC.records_of("nullable_primitives", 20)), SCHEMAS["nullable_primitives"])
    datums = _oracle_datums([batch], SCHEMAS["nullable_primitives"])
    for framing, edges in (("confluent", FR.CONFLUENT_EDGES), ("single_object", FR.SINGLE_EDGES + [-2, -(1 << 63) + 1])):
        msgs = []
        for key in edges:
            wire = key % (1 << 64)
            head = b"\x00" + wire.to_bytes(4, "big") if framing == "confluent" else b"\xc3\x01" + wire.to_bytes(8, "little")
            msgs += [head + d for d in datums]
        got = P.serialize_framed([(key, SCHEMAS["nullable_primitives"], batch) for key in edges], 2, framing=framing)
        _same(got, msgs, 2)


# ---- 6. empty ground ---------------------------------------------------------------------------------------------------------------------
def test_empty_ground():
    empty_a = c_walker.decode([], FR.SCHEMA_A)
    assert empty_a.num_rows == 0
    batch_b = c_walker.decode(list(FR._datums(70)[1]), FR.SCHEMA_B)
    msgs_b = [FR.frame("confluent", 2, d) for d in _oracle_datums([batch_b], FR.SCHEMA_B)]
    none = np.zeros(0, dtype=np.int64)
    for k in (1, 3):
        # n = 0: what an empty batch gives
        exp = py_encoder.serialize_record_batch(empty_a, FR.SCHEMA_A, k)
        assert len(exp) == 1 and len(exp[0]) == 0
        for groups in ([(1, FR.SCHEMA_A, [])], [(1, FR.SCHEMA_A, empty_a)], [(1, FR.SCHEMA_A, [empty_a, empty_a]), (2, FR.SCHEMA_B, [])],
                       [(1, FR.SCHEMA_A, [], none), (2, FR.SCHEMA_B, [], [])]):
            _same(P.serialize_framed(groups, k), [], k)
        # a group of no rows beside a group that has rows, in either place, with and without indices
        _same(P.serialize_framed([(1, FR.SCHEMA_A, []), (2, FR.SCHEMA_B, batch_b)], k), msgs_b, k)
        _same(P.serialize_framed([(2, FR.SCHEMA_B, batch_b), (1, FR.SCHEMA_A, empty_a)], k), msgs_b, k)
        _same(P.serialize_framed([(2, FR.SCHEMA_B, [batch_b], np.arange(70)), (1, FR.SCHEMA_A, [empty_a], none)], k), msgs_b, k)
        _same(P.serialize_framed([(1, FR.SCHEMA_A, [], none), (2, FR.SCHEMA_B, [batch_b.slice(0, 0), batch_b], np.arange(70))], k), msgs_b, k)


# ---- 7. errors that need the device ------------------------------------------------------------------------------------------------------
def test_a_batch_the_encoder_refuses_for_its_data():
    s = SCHEMAS["t_enum"]
    syms = ["A"] * 700
    syms[431] = "Z"
    bad = pa.RecordBatch.from_arrays([pa.array(syms)], names=["e"])
    good = pa.RecordBatch.from_arrays([pa.array(["A"] * 700)], names=["e"])
    with pytest.raises(ValueError) as eo:
        py_encoder.serialize_record_batch(bad, s, 1)
    other = c_walker.decode(list(FR._datums(10)[0]), FR.SCHEMA_A)
    for framing in FR.FRAMINGS:
        with pytest.raises(ValueError) as ei:
            P.serialize_framed([(3, FR.SCHEMA_A, other), (12, s, [good, bad])], 2, framing=framing)
        assert str(ei.value) == f"framed: schema id 12: {eo.value}"
        msgs = [FR.frame(framing, 3, d) for d in _oracle_datums([other], FR.SCHEMA_A)] + [FR.frame(framing, 12, d) for d in _oracle_datums([good], s)]
        _same(P.serialize_framed([(3, FR.SCHEMA_A, other), (12, s, [good])], 2, framing=framing), msgs, 2)      # a correct call succeeds afterwards


@pytest.mark.parametrize("n", (65, 1100))
def test_indices_that_are_no_permutation(n):
    msgs, ids = FR.pattern_messages("confluent", n, 3, "alternating classes")
    exp, _unknown = FR.expected_groups(msgs, FR.schemas_for(ids), "confluent", 2)
    exp = exp[::-1]      # given descending by id: the checks report ascending by wire id all the same
    good = [idx.copy() for _w, _t, idx, _b in exp]
    by_id = {wire: j for j, (wire, _t, _i, _b) in enumerate(exp)}
    low, high = min(by_id), max(by_id)
    last_tile = (n - 1) // 256 * 256

    def call(indices):
        keep = [i.copy() for i in indices]
        try:
            return P.serialize_framed([(wire, text, batches, idx) for (wire, text, _i, batches), idx in zip(exp, indices)], 2)
        finally:
            for a, b in zip(indices, keep):
                assert np.array_equal(a, b)      # the inputs are not modified

    def fails(indices, message):
        with pytest.raises(ValueError) as ei:
            call(indices)
        assert str(ei.value) == message, str(ei.value)
        _same(call(good), msgs, 2)      # ... and a correct call succeeds afterwards

    def edit(wire, row, value):
        out = [i.copy() for i in good]
        out[by_id[wire]][row] = value
        return out

    for first in (True, False):      # the offender in the first / in the last tile
        # a position named twice (its old position is a hole above it / below it)
        g = good[by_id[low]]
        row, src = (1, 0) if first else (len(g) - 1, len(g) - 2)
        assert (g[row] < 256 and g[src] < 256) if first else (g[row] >= last_tile and g[src] >= last_tile)
        fails(edit(low, row, g[src]), f"framed: position {g[src]} is named more than once")
        # a hole below every position named twice
        row, src = (0, 1) if first else (len(g) - 2, len(g) - 1)
        fails(edit(low, row, g[src]), f"framed: position {g[row]} is never named")
        # out of range: the first by wire id and row decides, before any duplicate is looked at
        for v in (n, -1, 1 << 40):
            bad = edit(low, 1 if first else len(g) - 1, v)
            bad[by_id[high]][0] = -7                     # (a later group's, although that group is given first)
            bad[by_id[low]][len(g) - 1 if first else 0] = g[2]      # (and a duplicate)
            fails(bad, f"framed: schema id {low}: index {v} is outside 0 .. {n - 1}")
    fails(edit(high, 0, n + 3), f"framed: schema id {high}: index {n + 3} is outside 0 .. {n - 1}")


def test_rh_async_is_refused():
    batch = c_walker.decode(list(FR._datums(10)[0]), FR.SCHEMA_A)
    enc = cabi.encode_to_device(batch, FR.SCHEMA_A, 1, kernel=cabi.KERNEL_GENERIC)
    try:
        with pytest.raises(ValueError, match="framed: .*RH_ASYNC"):
            cabi.frame_join([(enc, 0, 1, None)], 0, 10, 1, flags=cabi.RH_ASYNC)
        with pytest.raises(ValueError, match="framed: .*one device"):
            cabi.frame_join([(enc, 0, 1, None)], 0, 10, 1, devices=[0, 0])
        with pytest.raises(ValueError, match="framed: the sources have 10 rows, the call says 11"):
            cabi.frame_join([(enc, 0, 1, None)], 0, 11, 1)
    finally:
        enc.free()


# ---- 8. the C result ---------------------------------------------------------------------------------------------------------------------
def test_the_c_result(kernel):
    recs = synth.records("full", 1500, seed=9)
    batches = c_walker.decode_threaded(recs, FULL, 2)
    rows = [b.num_rows for b in batches]
    idx = [np.arange(0, 2 * rows[0], 2, dtype=np.int64), np.concatenate([np.arange(1, 2 * rows[0], 2), np.arange(2 * rows[0], 1500)]).astype(np.int64)]
    assert sorted(np.concatenate(idx).tolist()) == list(range(1500))
    py = P.serialize_framed([(21, FULL, batches[0], idx[0]), (22, FULL, batches[1], idx[1])], 3)
    datums = _oracle_datums(batches, FULL)
    msgs = [None] * 1500
    for j, p in enumerate(np.concatenate(idx).tolist()):
        msgs[p] = FR.frame("confluent", 21 if j < rows[0] else 22, datums[j])
    _same(py, msgs, 3)
    encs = [cabi.encode_to_device(b, FULL, 2, kernel=kernel) for b in batches]      # two chunks each: a source is one chunk
    try:
        sources = []
        for e, wire, ix in zip(encs, (21, 22), idx):
            assert e.chunks == 2
            half = len(ix) // 2
            sources += [(e, 0, wire, ix[:half]), (e, 1, wire, ix[half:])]
        joined = cabi.frame_join(sources, cabi.FRAMINGS["confluent"], 1500, 3)
        try:
            assert joined.chunks == 3
            host = joined.to_host()
            assert len(host) == len(py) and all(h.equals(p) for h, p in zip(host, py))
            _same(host, msgs, 3)
            assert joined.output_bytes == sum(4 * (len(a) + 1) + sum(len(m) for m in a.to_pylist()) for a in py)
            for c in range(3):
                d = joined.export(c)
                assert d.device_type == 10 and d.device_id == 0 and not d.sync_event      # ARROW_DEVICE_ROCM
                assert d.array.length == len(py[c]) and d.array.n_buffers == 3 and d.array.null_count == 0 and d.array.offset == 0
                assert d.array.buffers[1] and d.array.buffers[2]
                C.CFUNCTYPE(None, C.POINTER(cabi.ArrowArray))(d.array.release)(C.byref(d.array))
            last = cabi.frame_join_last()
            assert last["n"] == 1500 and min(last["lengths_ms"], last["scan_ms"], last["gather_ms"]) > 0
        finally:
            joined.free()
    finally:
        for e in encs:
            e.free()
