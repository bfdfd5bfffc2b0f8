"""Tolerant decode on the GPU.  The contract, for every entry point and both kernel forms:

    batches, errors = tolerant(recs, schema, k)
    batches == oracle(recs with placeholder_datum(schema) in the place of every malformed record, schema, k)   buffer for buffer
    errors  == [(i, what the oracle raises for [recs[i]] alone) for every malformed i], ascending

Expected values come from the oracle (oracle.c_walker), never from the engine's strict path.  Needs an MI355X."""
import functools
import random

import numpy as np
import pyarrow as pa
import pytest

import cases
import hipmem
import random_cases
from arrow_compare import assert_batches_identical
from avrogen import synth
from avrogen.schemas import SCHEMAS
from oracle import c_walker

import pyruhvro_amd as P
from pyruhvro_amd import cabi

pytestmark = pytest.mark.gpu

KERNELS = {"generic": cabi.KERNEL_GENERIC, "specialized": cabi.KERNEL_SPECIALIZED}


@pytest.fixture(params=sorted(KERNELS), autouse=True)
def kernel(request):
    """Every test runs on both kernel forms: set_kernel_mode applies to the strict runs inside a tolerant call."""
    old = P.set_kernel_mode(request.param)
    yield KERNELS[request.param]
    P.set_kernel_mode(old)


@functools.lru_cache(maxsize=None)
def _message(rec, schema):
    """What the strict decode raises when `rec` is the lowest failing record -- None for a well-formed one.  From the oracle."""
    try:
        c_walker.decode_threaded([rec], schema, 1)
        return None
    except ValueError as e:
        return str(e)


def _expect(recs, schema, k, bad_idx):
    ph = P.placeholder_datum(schema)
    bad = set(bad_idx)
    return c_walker.decode_threaded([ph if i in bad else r for i, r in enumerate(recs)], schema, k)


def _same(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        g.validate(full=True)
        assert g.schema.equals(e.schema, check_metadata=True)
        assert_batches_identical(g, e)


def _errors(recs, schema, bad_idx):
    out = [(i, _message(recs[i], schema)) for i in sorted(bad_idx)]
    assert all(m is not None for _, m in out)
    return out


def _check(recs, schema, k, bad_idx, **kw):
    got, errors = P.deserialize_array_threaded_tolerant(recs, schema, k, **kw)
    _same(got, _expect(recs, schema, k, bad_idx))
    assert [tuple(e) for e in errors] == _errors(recs, schema, bad_idx)
    assert all(isinstance(e, P.RecordError) for e in errors)


def _with_bad(good, bad, n, at):
    recs = [good[i % len(good)] for i in range(n)]
    for i in at:
        recs[i] = bad
    return recs


# ---------------------------------------------------------------------------------------------------------------------
N = 700
PLACEMENTS = [(0,), (63,), (64,), (255,), (256,), (N - 1,),
              (70, 100),                     # two in one wavefront
              (300, 301, 511),               # three in one tile: the strict machinery keeps only the lowest of these
              (233, 465),                    # k = 3: first and last record of the middle chunk
              (232, 466, 699)]               # ... last of the first chunk, first and last of the last one


@pytest.mark.parametrize("case", cases.error_cases(), ids=lambda c: c[0])
def test_every_error_case_at_every_place(case):
    _, schema, good, bad, message = case
    assert _message(bad, schema) == message
    for k in (1, 3):
        for at in PLACEMENTS:
            _check(_with_bad(good, bad, N, at), schema, k, at)


def _mixed():
    schema = SCHEMAS["flat_primitives"]
    by = {c[0]: c for c in cases.error_cases()}
    picks = ["eob_varint", "varint_too_long", "eob_f64", "bad_bool", "neg_strlen"]
    recs = synth.records("flat_primitives", 600)
    at = [5, 64, 65, 300, 599]
    for i, name in zip(at, picks):
        assert by[name][1] == schema
        recs[i] = by[name][3]
    return schema, recs, at


def test_mixed_errors_in_one_list():
    schema, recs, at = _mixed()
    assert len({_message(recs[i], schema) for i in at}) == 5
    for k in (1, 4):
        _check(recs, schema, k, at)


def test_validate_records_alone():
    schema, recs, at = _mixed()
    _, errors = P.deserialize_array_threaded_tolerant(recs, schema, 2)
    assert P.validate_records(recs, schema) == errors == [P.RecordError(*e) for e in _errors(recs, schema, at)]
    assert P.validate_records(synth.records("flat_primitives", 600), schema) == []
    # more than max_errors: the lowest ones, and the exact count
    data, offsets = c_walker.pack(recs)
    listed, total = cabi.validate_packed(data, offsets, schema, max_errors=2, want_total=True)
    assert listed == errors[:2] and total == 5
    ptrs = np.array([data.ctypes.data + int(o) for o in offsets[:-1]], dtype=np.uint64)
    assert cabi.validate_slices(ptrs, np.diff(offsets), schema) == errors
    d_data, d_off = hipmem.upload_packed(data, offsets)
    assert cabi.validate_device(d_data.ptr, d_off.ptr, int(offsets[-1]), len(recs), schema, device=0) == errors


def test_all_bad_and_overflow():
    schema = SCHEMAS["flat_primitives"]
    recs = [b""] * 300
    _check(recs, schema, 3, range(300), max_errors=300)
    with pytest.raises(ValueError) as e:
        P.deserialize_array_threaded_tolerant(recs, schema, 3, max_errors=299)
    assert str(e.value) == "unexpected end of buffer"
    with pytest.raises(ValueError) as e:
        P.deserialize_array_tolerant(recs, schema, max_errors=0)
    assert str(e.value) == "unexpected end of buffer"


def _delta(f):
    before = cabi.engine_counters()
    out = f()
    after = cabi.engine_counters()
    return out, {k: after[k] - before[k] for k in after}


def test_clean_input_costs_a_strict_call(kernel):
    schema = SCHEMAS["full"]
    recs = synth.records("full", 1500)
    data, offsets = c_walker.pack(recs)
    exp = c_walker.decode_threaded(recs, schema, 3)
    cabi.decode_packed(data, offsets, schema, 3, kernel=kernel)          # (the schema's first call takes another road)
    strict, d_strict = _delta(lambda: cabi.decode_packed(data, offsets, schema, 3, kernel=kernel))
    (got, errors), d_tol = _delta(lambda: cabi.decode_packed_tolerant(data, offsets, schema, 3, kernel=kernel))
    _same(strict, exp)
    _same(got, exp)
    assert errors == []
    assert d_strict["tolerant_calls"] == 0 and d_strict["tolerant_repairs"] == 0
    assert d_tol["tolerant_calls"] == 1 and d_tol["tolerant_repairs"] == 0
    for name in cabi.ENGINE_COUNTERS:
        if not name.startswith("tolerant"):
            assert d_tol[name] == d_strict[name], name
    # a dirty call counts its repair
    recs[7] = recs[7][:3]
    assert _message(recs[7], schema) is not None
    _, d_dirty = _delta(lambda: P.deserialize_array_threaded_tolerant(recs, schema, 3))
    assert d_dirty["tolerant_calls"] == 1 and d_dirty["tolerant_repairs"] == 1


def _truncations(recs, schema, at, seed):
    """recs with the records at `at` truncated at a random byte -- only truncations that the oracle rejects (checked here, on
    the CPU); -> (recs, the indices that are malformed now)."""
    r = random.Random(seed)
    recs = list(recs)
    bad = []
    for i in at:
        for _ in range(64):
            cut = recs[i][:r.randrange(len(recs[i]))] if recs[i] else recs[i]
            if _message(cut, schema) is not None:
                recs[i] = cut
                bad.append(i)
                break
    return recs, bad


def _schema_case(name):
    if name.startswith("random"):
        return random_cases.random_case(int(name[6:]), 600)
    if name == "t_nullable_nested":
        (c,) = [c for c in cases.differential_cases() if c[1] == SCHEMAS[name]]
        return c[1], [c[2][i % len(c[2])] for i in range(600)]
    return SCHEMAS[name], synth.records(name, 600)


@pytest.mark.parametrize("name", ["full", "array_and_map", "t_nullable_nested", "wide97", "flat4", "random3", "random11"])
def test_schemas_with_truncated_records(name):
    schema, recs = _schema_case(name)
    recs, bad = _truncations(recs, schema, [63, 64, 257, 599], seed=len(name))
    assert len(bad) >= 3, "the truncations of this case are meant to be malformed"
    for k in (1, 5):
        _check(recs, schema, k, bad)


def test_past_the_window(monkeypatch):
    """Tiles past an 8 KiB window are walked from global memory by the validation kernel, as by the generic decode kernels."""
    schema, recs = cases.long_string_case(n=600)
    monkeypatch.setenv("RUHVRO_HIP_WIN_BYTES", "8192")
    offs = np.cumsum([0] + [len(r) for r in recs])
    over = [t for t in range(0, 600, 256) if offs[min(t + 256, 600)] - offs[t] > 8192]
    assert over, "no tile of this input goes past the window"
    at = sorted({over[0] + 1, over[0] + 70, over[-1] + 40})
    recs, bad = _truncations(recs, schema, at, seed=2)
    assert bad
    _check(recs, schema, 2, bad)


def test_a_record_larger_than_the_window():
    schema = SCHEMAS["flat_primitives"]
    small = synth.records("flat_primitives", 300)
    head = small[0][:small[0].rindex(b"row-0") - 1]                  # the five fixed fields of row 0
    big = head + bytes([0xC0, 0x9A, 0x0C]) + b"x" * 100000           # zigzag(100000) = c0 9a 0c
    assert _message(big, schema) is None and _message(big[:-1], schema) == "unexpected end of buffer (string)"
    recs = list(small)
    recs[10] = big
    recs[150] = big[:-1]
    recs[151] = b""
    _check(recs, schema, 2, [150, 151])


# ---------------------------------------------------------------------------------------------------------------------
def _full_dirty():
    schema = SCHEMAS["full"]
    recs, bad = _truncations(synth.records("full", 700), schema, [0, 100, 101, 699], seed=9)
    assert len(bad) >= 3
    return schema, recs, bad


def test_entry_points(kernel):
    schema, recs, bad = _full_dirty()
    want = [P.RecordError(*e) for e in _errors(recs, schema, bad)]
    exp1, exp3 = _expect(recs, schema, 1, bad), _expect(recs, schema, 3, bad)
    got, errors = P.deserialize_array_tolerant(recs, schema)
    _same([got], exp1)
    assert errors == want
    got, errors = P.deserialize_binary_array_tolerant(pa.array(recs, type=pa.binary()), schema, 3)
    _same(got, exp3)
    assert errors == want
    data, offsets = c_walker.pack(recs)
    got, errors = cabi.decode_packed_tolerant(data, offsets, schema, 3, kernel=kernel)
    _same(got, exp3)
    assert errors == want
    ptrs = np.array([data.ctypes.data + int(o) for o in offsets[:-1]], dtype=np.uint64)
    got, errors = cabi.decode_slices_tolerant(ptrs, np.diff(offsets), schema, 3, kernel=kernel)
    _same(got, exp3)
    assert errors == want
    dec = P.deserialize_to_device(recs, schema, 3, on_error="placeholder")
    assert dec.errors == want
    _same(dec.to_host(), exp3)
    clean = synth.records("full", 300)
    assert P.deserialize_to_device(clean, schema, 2, on_error="placeholder").errors == []
    assert P.deserialize_to_device(clean, schema, 2).errors == []
    with pytest.raises(ValueError) as e:
        P.deserialize_to_device(recs, schema, 3)
    assert str(e.value) == want[0].message


def test_projection_with_the_damage_in_a_dropped_field():
    schema = SCHEMAS["full"]
    cols = ["created_at", "name"]
    recs = synth.records("full", 600)
    # cut in the middle: `name`, the first field, is intact and the walk fails inside one of the dropped fields behind it
    bad = [3, 64, 598]
    for i in bad:
        recs[i] = recs[i][:len(recs[i]) // 2]
        assert recs[i].startswith(synth.records("full", 1, start=i)[0][:8]) and _message(recs[i], schema) is not None
    assert len(bad) == 3
    got, errors = P.deserialize_array_threaded_tolerant(recs, schema, 2, columns=cols)
    _same(got, [b.select(cols) for b in _expect(recs, schema, 2, bad)])
    assert [tuple(e) for e in errors] == _errors(recs, schema, bad)


def test_device_gather(kernel):
    """Records of 0..40 bytes, so that every 16-byte alignment of source and destination occurs; the placeholder (one byte: an
    empty array) shorter and longer than the records it replaces; malformed records first, last and next to each other."""
    schema = SCHEMAS["t_array_str"]
    r = random.Random(4)
    enc = lambda tags: b"".join(bytes([2]) + bytes([2 * len(t)]) + t for t in tags) + b"\x00"      # noqa: E731 - one block per item
    recs = []
    for i in range(1500):
        want = r.randrange(1, 41)
        tags, left = [], want - 1
        while left >= 2:
            ln = min(r.randrange(0, 12), left - 2)
            tags.append(bytes(r.randrange(97, 123) for _ in range(ln)))
            left -= 2 + ln
        recs.append(enc(tags))
    assert {len(x) for x in recs} >= set(range(2, 41)) - {2} and all(_message(x, schema) is None for x in recs[:50])
    bad = [0, 1, 2, 77, 640, 641, 1000, 1498, 1499]
    for j, i in enumerate(bad):
        recs[i] = b"" if j % 3 == 0 else recs[i][:-1] if j % 3 == 1 else recs[i][:1]
        assert _message(recs[i], schema) is not None
    data, offsets = c_walker.pack(recs)
    d_data, d_off = hipmem.upload_packed(data, offsets)
    for k in (1, 4):
        res = cabi.decode_device_tolerant(d_data.ptr, d_off.ptr, int(offsets[-1]), len(recs), schema, k, device=0, kernel=kernel)
        assert res.errors == [P.RecordError(*e) for e in _errors(recs, schema, bad)]
        _same(res.to_host(), _expect(recs, schema, k, bad))
        res.free()
    # the input was not touched: the strict call still fails on record 0
    with pytest.raises(ValueError) as e:
        cabi.decode_device(d_data.ptr, d_off.ptr, int(offsets[-1]), len(recs), schema, 1, device=0, kernel=kernel)
    assert str(e.value) == _message(recs[0], schema)
