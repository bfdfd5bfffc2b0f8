"""Tolerant decode under random damage, and the edges of its host logic that tests/test_tolerant_gpu.py does not reach.

The contract is that file's: for every entry point and both kernel forms

    errors  == [(i, what the oracle raises for [recs[i]] alone) for every malformed i], ascending
    batches == oracle(recs with placeholder_datum(schema) in the place of every malformed record)      buffer for buffer

Here the records are damaged at random (tests/damage.py: bit flips, cuts, junk, over-long varints, huge counts) in seventeen
schemas, so the validation kernel's walk has to agree with the oracle on EVERY record of a list, not on the lowest malformed
one.  Every expectation comes from the oracle (oracle.c_walker; oracle.py_walker in its extended form for the schemas that one
refuses), never from the engine's strict path; every comparison is exact.  The first three tests need no GPU: they check that
the inputs are what the GPU tests below take them to be.  (Two of them ask placeholder_datum for a schema's placeholder, which
is host code of the native library: like the project's other non-GPU tests they need the built extension, and no device.)"""
import functools
import random

import numpy as np
import pyarrow as pa
import pytest

import cases
import damage as D
import hipmem
from arrow_compare import assert_batches_identical
from avrogen import synth
from avrogen.schemas import SCHEMAS
from oracle import avro_schema as S
from oracle import c_walker

import pyruhvro_amd as P
from pyruhvro_amd import cabi

KERNELS = {"generic": cabi.KERNEL_GENERIC, "specialized": cabi.KERNEL_SPECIALIZED}


@pytest.fixture(params=sorted(KERNELS))
def kernel(request):
    """As in test_tolerant_gpu.py: set_kernel_mode applies to the strict runs inside a tolerant call."""
    old = P.set_kernel_mode(request.param)
    yield KERNELS[request.param]
    P.set_kernel_mode(old)


def on_gpu(f):
    """Every GPU test runs on both kernel forms."""
    return pytest.mark.gpu(pytest.mark.usefixtures("kernel")(f))


def _full_validation(batch):
    try:
        batch.validate(full=True)
        return None
    except pa.ArrowInvalid as e:
        return str(e)


def _same(got, exp):
    """Buffer for buffer the oracle's batches.  A record that is damaged but well-formed may carry a string that is not UTF-8 or
    a decimal beyond its precision -- the walk checks neither, in the reference, the oracle or here -- so validate(full=True)
    is asked of the engine's batch outright wherever the oracle's batch passes it, and has to give the oracle's complaint where
    it does not."""
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        g.validate()
        assert g.schema.equals(e.schema, check_metadata=True)
        assert_batches_identical(g, e)
        why = _full_validation(e)
        if why is None:
            g.validate(full=True)
        else:
            assert _full_validation(g) == why


@functools.lru_cache(maxsize=None)
def _expected(name, k):
    """The oracle's decode of a case's dirty list with the placeholder at every malformed index (once per case and k)."""
    d = D.dirty_case(name)
    return d.oracle(D.patched(d.recs, d.verdicts, P.placeholder_datum(d.schema)), d.schema, k)


def _want(d):
    return [(i, d.verdicts[i]) for i in sorted(d.verdicts)]


def _same_errors(d, got, what):
    want = _want(d)
    assert [tuple(e) for e in got] == want, what + ": " + D.explain(d.name, d.seed, d.recs, want, got)
    assert all(isinstance(e, P.RecordError) for e in got)


def _strict_device_raises(d_data, d_off, offsets, n, schema, kernel, message):
    with pytest.raises(ValueError) as e:
        cabi.decode_device(d_data.ptr, d_off.ptr, int(offsets[-1]), n, schema, 1, device=0, kernel=kernel)
    assert str(e.value) == message


def _check_everything(d, ks, kernel, expected):
    """validate_records, validate_device, the host tolerant decode for every k of `ks`, the device one for the last k, and the
    strict device call on the input afterwards.  expected(k) -> the oracle's batches."""
    _same_errors(d, P.validate_records(d.recs, d.schema), "validate_records")
    data, offsets = c_walker.pack(d.recs)
    d_data, d_off = hipmem.upload_packed(data, offsets)
    n = len(d.recs)
    _same_errors(d, cabi.validate_device(d_data.ptr, d_off.ptr, int(offsets[-1]), n, d.schema, device=0), "validate_device")
    for k in ks:
        got, errors = P.deserialize_array_threaded_tolerant(d.recs, d.schema, k)
        _same_errors(d, errors, f"deserialize_array_threaded_tolerant, k = {k}")
        _same(got, expected(k))
    res = cabi.decode_device_tolerant(d_data.ptr, d_off.ptr, int(offsets[-1]), n, d.schema, ks[-1], device=0, kernel=kernel)
    _same_errors(d, res.errors, f"decode_device_tolerant, k = {ks[-1]}")
    _same(res.to_host(), expected(ks[-1]))
    res.free()
    # the input was not touched
    _strict_device_raises(d_data, d_off, offsets, n, d.schema, kernel, d.verdicts[min(d.verdicts)])


# ---------------------------------------------------------------------------------------------------------------------
# the inputs (no GPU)
@pytest.mark.parametrize("name", sorted(D.FUZZ_CASES))
def test_the_inputs_are_not_trivial(name):
    """Of a case's damaged records between 25 % and 90 % are malformed and the rest damaged but well-formed, with three distinct
    messages at least; the clean list decodes; the layout of dirty_list is what it says."""
    d = D.dirty_case(name)
    d.oracle(d.clean, d.schema, 1)
    hit = set(d.damaged)
    assert len(d.recs) == D.N and set(range(64)) | {255, 256, D.N - 1} <= hit and not hit & set(range(64, 128))
    assert all(d.recs[i] == d.clean[i] for i in range(D.N) if i not in hit)
    share = len(d.verdicts) / len(d.damaged)
    assert 0.25 <= share <= 0.90, (name, d.seed, share)
    assert len(set(d.verdicts.values())) >= (2 if name in D.TWO_MESSAGE_CASES else 3), (name, set(d.verdicts.values()))
    # bitmap words of every shape: all ones is likely only in records 0-63, so ask for many malformed ones there
    assert sum(i < 64 for i in d.verdicts) >= 16
    if name == "n4":           # the errors of the N4 leaf types all occur
        assert {"invalid uuid string", "unexpected end of buffer (fixed)"} <= set(d.verdicts.values())
        assert any(m.startswith("decimal value of") for m in d.verdicts.values())
    if name == "duration":
        assert any(m.startswith("duration with") for m in d.verdicts.values())
    if name == "union_no_null":    # no null branch: the placeholder is branch 0 plus its payload, and the oracle takes it
        ph = P.placeholder_datum(d.schema)
        assert ph == bytes(4) and len(ph) > 1 and D.message(ph, d.schema, d.oracle) is None
        assert "null" not in [v.kind for v in S.parse_schema(d.schema).fields[0].schema.variants]
        assert {r[0] for r in d.clean} == {0, 2, 4}      # every branch occurs, each with a payload


def test_damage_takes_every_form():
    rng = random.Random(1)
    rec = bytes(range(1, 41))
    out = {D.damage(rec, rng) for _ in range(400)}
    huge = b"\xff\xff\xff\xff\x0f"
    assert any(len(x) == len(rec) and sum(bin(a ^ b).count("1") for a, b in zip(x, rec)) == 1 for x in out)      # one bit
    assert any(len(x) < len(rec) and rec.startswith(x) for x in out)                                                 # a cut
    assert any(len(rec) < len(x) <= len(rec) + 4 and b"\x80" * 10 not in x and not x.endswith(huge) for x in out)      # junk
    assert any(len(x) == len(rec) and sum(a != b for a, b in zip(x, rec)) == 1 and set(x) - set(rec) <= {0x80, 0xFF, 0x7F, 0} for x in out)
    assert any(b"\x80" * 10 in x for x in out) and any(x.endswith(huge) for x in out)
    assert D.damage(b"", rng) != b""
    assert D.dirty_list([rec] * D.N, 3) == D.dirty_list([rec] * D.N, 3)


WIN = 8192


def _tiles_past(recs, win=WIN):
    """The 256-record tiles of a list whose bytes, from the 16-byte boundary below their first one, do not fit `win`: the
    validation kernel walks those from global memory and every other one from LDS."""
    offs = np.cumsum([0] + [len(r) for r in recs])
    return {t for t in range(0, len(recs), 256) if int(offs[min(t + 256, len(recs))]) - (int(offs[t]) & ~15) > win}


@functools.lru_cache(maxsize=None)
def _window_case():
    """cases.long_string_case(600) with its 88 shortest records moved to the end: as the list comes, each of its three tiles is
    far past an 8 KiB window (the smallest, the last 88 records, has 20 KB); like this the last one fits.  40 records damaged in
    the tiles past the window, 40 in the one inside."""
    schema, recs = cases.long_string_case(n=600)
    short = set(sorted(range(600), key=lambda i: (len(recs[i]), i))[:88])
    recs = [r for i, r in enumerate(recs) if i not in short] + [recs[i] for i in sorted(short)]
    past = _tiles_past(recs)
    rng = random.Random(11)
    at_past = rng.sample([i for i in range(600) if i - i % 256 in past], 40)
    at_in = rng.sample([i for i in range(600) if i - i % 256 not in past], 40)
    clean = list(recs)
    for i in sorted(at_past + at_in):
        recs[i] = D.damage(recs[i], rng)
    hit = sorted(at_past + at_in)
    v = D.verdicts(recs, hit, schema, D.c_oracle)
    return D.Dirty("long_strings", 11, schema, D.c_oracle, clean, recs, hit, v), sorted(at_past), sorted(at_in)


@functools.lru_cache(maxsize=None)
def _window_expected(k):
    d, _, _ = _window_case()
    return d.oracle(D.patched(d.recs, d.verdicts, P.placeholder_datum(d.schema)), d.schema, k)


def test_the_placements_are_what_the_gpu_tests_need():
    # tiles past the window and tiles inside it, with malformed records in both -- after the damage, which moves the tile sizes
    d, at_past, at_in = _window_case()
    past = _tiles_past(d.recs)
    assert past == {0, 256} == _tiles_past(d.clean)
    assert len(at_past) == len(at_in) == 40
    assert all(i - i % 256 in past for i in at_past) and all(i - i % 256 not in past for i in at_in)
    assert sum(i in d.verdicts for i in at_past) >= 5 and sum(i in d.verdicts for i in at_in) >= 5
    c_walker.decode_threaded(d.clean, d.schema, 1)
    # rh_k_patch_scan scans 256 block sums per round: more than 256 blocks of 256 records for a second round
    recs, bad = _scan_case()
    assert (len(recs) + 255) // 256 == 274 > 256 and bad == [0, 255, 256, 65535, 65536, 65537, 69999]
    assert {len(r) for i, r in enumerate(recs) if i not in bad} == {1, 3, 4, 5}
    # rh_k_patch_gather writes a placeholder 64 bytes per trip: more than 128 bytes for a third trip, and longer than what it replaces
    ph = P.placeholder_datum(D.LONG_PLACEHOLDER_SCHEMA)
    assert ph == bytes(138) and D.message(ph, D.LONG_PLACEHOLDER_SCHEMA, D.py_oracle) is None
    recs, bad = _long_placeholder_case()
    assert all(len(recs[i]) < len(ph) for i in bad) and {len(r) for r in recs} >= set(range(138, 179))
    assert bad == [0, 100, 101, 150, 299]            # first, adjacent, alone in the wavefront of records 128-191, last
    # two validation groups: more than 2^20 records
    assert HOST_N > 1 << 20 and HOST_BAD == [3, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, HOST_N - 1]


# ---------------------------------------------------------------------------------------------------------------------
@on_gpu
@pytest.mark.parametrize("name", sorted(D.FUZZ_CASES))
def test_every_record_gets_the_oracles_verdict(name, kernel):
    d = D.dirty_case(name)
    _check_everything(d, (1, 3), kernel, lambda k: _expected(name, k))


@on_gpu
@pytest.mark.parametrize("cols", [["created_at", "name"], ["emails", "phone_numbers"]], ids="-".join)
def test_projection_over_damage(cols):
    """The validation walks every field of the full schema, whatever the projection: the errors are the full decode's."""
    d = D.dirty_case("full")
    got, errors = P.deserialize_array_threaded_tolerant(d.recs, d.schema, 3, columns=cols)
    _same_errors(d, errors, f"columns = {cols}")
    _same(got, [b.select(cols) for b in _expected("full", 3)])


@on_gpu
def test_damage_in_tiles_past_the_window(monkeypatch, kernel):
    """Tiles past an 8 KiB window are walked from global memory by the validation kernel, the others from LDS: every kind of
    damage in both (test_past_the_window of test_tolerant_gpu.py has three cuts, past the window only)."""
    d, _, _ = _window_case()
    monkeypatch.setenv("RUHVRO_HIP_WIN_BYTES", str(WIN))
    _check_everything(d, (2,), kernel, _window_expected)


ENC = lambda tags: b"".join(bytes([2]) + bytes([2 * len(t)]) + t for t in tags) + b"\x00"      # noqa: E731 - test_device_gather's: one block per item


@functools.lru_cache(maxsize=None)
def _scan_case():
    """70,000 t_array_str records of 1, 3, 4 or 5 bytes (ENC has no record of 2): 274 blocks of 256, the smallest number of
    records at which rh_k_patch_scan goes round twice.  Malformed records at both ends, around the end of the first block and
    around the 65,536 records of the scan's first round."""
    r = random.Random(6)
    forms = [ENC([]), ENC([b""]), ENC([b"a"]), ENC([b"ab"])]
    recs = [forms[r.randrange(4)] for _ in range(70000)]
    bad = [0, 255, 256, 65535, 65536, 65537, 69999]
    for j, i in enumerate(bad):
        recs[i] = b"\x02" if j % 2 == 0 else ENC([b"ab"])[:3 + j % 2]
    return recs, bad


def _device_case(schema, recs, bad, oracle, ks, kernel):
    """Device input: validate_device and decode_device_tolerant for every k of `ks`; the strict call afterwards."""
    msg = {i: D.message(recs[i], schema, oracle) for i in bad}
    assert all(m is not None for m in msg.values())
    want = [P.RecordError(i, msg[i]) for i in bad]
    data, offsets = c_walker.pack(recs)
    d_data, d_off = hipmem.upload_packed(data, offsets)
    n = len(recs)
    assert cabi.validate_device(d_data.ptr, d_off.ptr, int(offsets[-1]), n, schema, device=0) == want
    fixed = D.patched(recs, bad, P.placeholder_datum(schema))
    for k in ks:
        res = cabi.decode_device_tolerant(d_data.ptr, d_off.ptr, int(offsets[-1]), n, schema, k, device=0, kernel=kernel)
        assert res.errors == want
        _same(res.to_host(), oracle(fixed, schema, k))
        res.free()
    _strict_device_raises(d_data, d_off, offsets, n, schema, kernel, msg[bad[0]])


@on_gpu
def test_patch_scan_second_round(kernel):
    recs, bad = _scan_case()
    _device_case(SCHEMAS["t_array_str"], recs, bad, D.c_oracle, (1, 4), kernel)


@functools.lru_cache(maxsize=None)
def _cut_case():
    schema = SCHEMAS["flat_primitives"]
    by = {c[0]: c for c in cases.error_cases()}
    recs = synth.records("flat_primitives", 700)
    bad = [5, 63, 64, 200, 255, 256, 699]
    for i, name in zip(bad, ["eob_varint", "varint_too_long", "eob_f32", "eob_f64", "bad_bool", "neg_strlen", "eob_string"]):
        assert by[name][1] == schema
        recs[i] = by[name][3]
    want = [P.RecordError(i, D.message(recs[i], schema, D.c_oracle)) for i in bad]
    assert len({e.message for e in want}) == 7
    return schema, recs, bad, want


@on_gpu
def test_the_lowest_max_errors_at_every_cut(kernel):
    """More malformed records than max_errors: a second validation pass lists the lowest ones, bounded by the record behind
    them.  With these seven that bound falls inside a bitmap word (63, 200), on a word boundary (64), on the last record of a
    tile (255), on a tile boundary (256) and on the last record (699); max_errors = 0 lists nothing and still counts."""
    schema, recs, bad, want = _cut_case()
    data, offsets = c_walker.pack(recs)
    d_data, d_off = hipmem.upload_packed(data, offsets)
    dev = (d_data.ptr, d_off.ptr, int(offsets[-1]), len(recs))
    for cap in range(9):
        listed, total = cabi.validate_device(*dev, schema, max_errors=cap, device=0, want_total=True)
        assert (listed, total) == (want[:min(cap, 7)], 7), cap
        listed, total = cabi.validate_packed(data, offsets, schema, max_errors=cap, want_total=True)
        assert (listed, total) == (want[:min(cap, 7)], 7), cap
    fixed = D.patched(recs, bad, P.placeholder_datum(schema))
    for cap in range(8):
        if cap < 7:
            with pytest.raises(ValueError) as e:
                P.deserialize_array_threaded_tolerant(recs, schema, 2, max_errors=cap)
            assert str(e.value) == want[0].message
            with pytest.raises(ValueError) as e:
                cabi.decode_device_tolerant(*dev, schema, 2, device=0, kernel=kernel, max_errors=cap)
            assert str(e.value) == want[0].message
        else:
            got, errors = P.deserialize_array_threaded_tolerant(recs, schema, 2, max_errors=cap)
            assert errors == want
            _same(got, c_walker.decode_threaded(fixed, schema, 2))
            res = cabi.decode_device_tolerant(*dev, schema, 2, device=0, kernel=kernel, max_errors=cap)
            assert res.errors == want
            _same(res.to_host(), c_walker.decode_threaded(fixed, schema, 2))
            res.free()


HOST_N = (1 << 20) + 200
HOST_BAD = [3, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, HOST_N - 1]


@functools.lru_cache(maxsize=None)
def _host_groups_expected():
    return c_walker.decode_threaded([b"\x00"] * HOST_N, SCHEMAS["t_array_str"], 2)      # (the placeholder is b"\x00", the good record)


@on_gpu
def test_host_validation_groups():
    """Host records are validated in groups of 2^20: malformed records on both sides of the group boundary, and a list that
    fills up in the first group and has to list nothing, but count, in the second."""
    schema = SCHEMAS["t_array_str"]
    assert P.placeholder_datum(schema) == b"\x00"
    recs = [b"\x00"] * HOST_N
    for i in HOST_BAD:
        recs[i] = b"\x02"
    assert D.message(b"\x00", schema, D.c_oracle) is None
    strict = D.message(b"\x02", schema, D.c_oracle)
    want = [P.RecordError(i, strict) for i in HOST_BAD]
    assert P.validate_records(recs, schema) == want
    data, offsets = c_walker.pack(recs)
    assert cabi.validate_packed(data, offsets, schema, max_errors=3, want_total=True) == (want[:3], 5)
    assert cabi.validate_packed(data, offsets, schema, max_errors=1, want_total=True) == (want[:1], 5)
    with pytest.raises(ValueError) as e:
        P.deserialize_array_threaded_tolerant(recs, schema, 2, max_errors=4)
    assert str(e.value) == strict
    got, errors = P.deserialize_array_threaded_tolerant(recs, schema, 2)
    assert errors == want
    _same(got, _host_groups_expected())


@functools.lru_cache(maxsize=None)
def _long_placeholder_case():
    """300 records of 138 + (0..40) bytes; the malformed ones are cuts shorter than the 138 bytes of the placeholder."""
    r = random.Random(8)
    recs = []
    for i in range(300):
        ln = i % 41
        recs.append(bytes(r.randrange(256) for _ in range(137)) + bytes([2 * ln]) + bytes(r.randrange(97, 123) for _ in range(ln)))
    bad = [0, 100, 101, 150, 299]
    for i, cut in zip(bad, [0, 50, 120, 137, 99]):
        recs[i] = recs[i][:cut]
    return recs, bad


@on_gpu
def test_gather_with_a_long_placeholder(kernel):
    recs, bad = _long_placeholder_case()
    _device_case(D.LONG_PLACEHOLDER_SCHEMA, recs, bad, D.py_oracle, (1, 3), kernel)
