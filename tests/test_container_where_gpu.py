"""Row filters in the container read, on the GPU: ``read_container_where`` / ``read_container_where_to_device`` / ``filter_container``.

The contract, for every container file F with writer schema S, every predicate W the front end accepts and every k:

    read_container_where(F, W, k, **kw) == deserialize_array_threaded([r for r in records_of(F) if keep_W(r)], S, k, **kw)
    filter_container(F, W)              == numpy bool[n], element i = keep_W(records_of(F)[i])

The files are written by the tests' own writer (tests/container_cases.py) from records this file holds, and the expected values
are the ORACLE's: its decode of the records that a Python evaluation of its full decode keeps (tests/filter_cases.py) -- never
anything the engine returns.  A malformed record or block raises what ``read_container`` raises, whatever the predicate says."""
import functools

import numpy as np
import pytest

import container_cases as CC
import filter_cases as FC
import resolve_cases as RC
from arrow_compare import assert_batches_identical
from avrogen import synth
from avrogen.schemas import SCHEMAS
from oracle import c_walker

import pyruhvro_amd as P
from pyruhvro_amd import cabi

pytestmark = pytest.mark.gpu

FULL = SCHEMAS["full"]
N = 508
assert sum(CC.RAGGED) == N and len(CC.RAGGED) == 77


@pytest.fixture(autouse=True)
def _generic_kernels():
    """The split has one kernel form; the decode behind it runs on the generic kernels, so that no schema of this file needs a
    specialised kernel compiled."""
    old = P.set_kernel_mode("generic")
    yield
    P.set_kernel_mode(old)


def _same(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        g.validate(full=True)
        assert g.schema.equals(e.schema, check_metadata=True)
        assert_batches_identical(g, e)


def _recs():
    return list(CC.records_of("full", N))


@functools.lru_cache(maxsize=None)
def _first_and_last_created_at():
    col = FC.oracle_decode(_recs(), FULL, 1)[0].column("created_at").to_pylist()
    assert col.count(col[0]) == 1 and col.count(col[-1]) == 1
    return col[0], col[-1]


# predicate -> the records of records_of("full", 508) it keeps (counted on the oracle; None: one record, checked below)
PREDICATES = {
    "age>=30": (("age", ">=", 30), 198),
    "age is_null": (("age", "is_null"), 261),
    "created_at>0": (("created_at", ">", 0), 508),
    "class==B": (("class", "==", "B"), 183),
    "name<m": (("name", "<", "m"), 111),
    "18<=age<65": ([("age", ">=", 18), ("age", "<", 65)], 178),
    "age==-12345": (("age", "==", -12345), 0),
    "record 0 only": (None, 1),
    "record 507 only": (None, 1),
}


def _where(pred):
    if pred == "record 0 only":
        return ("created_at", "==", _first_and_last_created_at()[0])
    if pred == "record 507 only":
        return ("created_at", "==", _first_and_last_created_at()[1])
    return PREDICATES[pred][0]


@functools.lru_cache(maxsize=None)
def _mask(pred):
    """The oracle's mask of a predicate over the 508 records: computed once, shared, never modified."""
    mask = FC.oracle_mask(_recs(), FULL, _where(pred))
    mask.setflags(write=False)
    assert int(mask.sum()) == PREDICATES[pred][1], (pred, int(mask.sum()))
    if pred == "record 0 only":
        assert mask[0]
    if pred == "record 507 only":
        assert mask[N - 1]
    return mask


@functools.lru_cache(maxsize=None)
def _expected(pred, k):
    return FC.oracle_filtered(_recs(), FULL, _where(pred), k, _mask(pred))


LAYOUTS = {
    "ragged": CC.RAGGED,                          # empty blocks, a 300-record block over five keep words beside idle lanes
    "ones": [1] * N,                              # two workgroups, up to 64 lanes ORing into one word
    "one_block": [N],                             # one lane owns every word
    "word_edges": [64, 128, 63, 65, 188],
}


@functools.lru_cache(maxsize=None)
def _file(layout, codec="null"):
    return CC.write(FULL, CC.split(_recs(), LAYOUTS[layout]), codec)


# ---- 1. layouts x masks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pred", list(PREDICATES))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_layouts_and_masks(layout, pred):
    blob, where, mask = _file(layout), _where(pred), _mask(pred)
    got = P.filter_container(blob, where)
    assert got.dtype == np.bool_ and got.shape == (N,)
    assert np.array_equal(got, mask), np.flatnonzero(got != mask)[:10]
    last = cabi.container_where_last()
    assert last["n"] == N and last["kept"] == int(mask.sum()) and last["gather_ms"] == 0 and last["split_ms"] > 0
    for k in (1, 3):
        _same(P.read_container_where(blob, where, k), _expected(pred, k))
        last = cabi.container_where_last()
        assert last["n"] == N and last["kept"] == int(mask.sum())
        if mask.all():      # the untouched road: the uploaded buffer decoded where it is, no compaction launch
            assert last["kept"] == last["n"] and last["gather_ms"] == 0
        else:
            assert last["gather_ms"] > 0


# ---- 2. every kind and form: unaligned 8-byte reads through a block-based source, 10-byte varints, 255- and 300-byte values --------
KINDS_N = 192


def _ragged_counts(n):
    counts = [0, 1, 70, 1, 0, 64, 2]
    i = 0
    while sum(counts) < n:
        counts.append(min((i * 7) % 5, n - sum(counts)))
        i += 1
    assert sum(counts) == n
    return counts


@functools.lru_cache(maxsize=None)
def _kinds():
    recs = list(FC.kinds_records(KINDS_N))
    full = FC.oracle_decode(recs, FC.KINDS_SCHEMA, 1)[0]
    return CC.write(FC.KINDS_SCHEMA, CC.split(recs, _ragged_counts(KINDS_N))), full


@pytest.mark.parametrize("field,kind,form", FC.KINDS_FIELDS, ids=[f[0] for f in FC.KINDS_FIELDS])
def test_every_kind_and_form(field, kind, form):
    import pyarrow as pa
    blob, full = _kinds()
    col = full.column(field)
    if pa.types.is_temporal(col.type):
        col = col.cast(pa.int32() if col.type.bit_width == 32 else pa.int64())
    vals = col.to_pylist()
    ops = FC.KIND_OPS[kind]
    cases = [(ops[j % len(ops)], k) for j, k in enumerate(FC.KIND_COMPARANDS[kind])] + [("is_null", None)]
    kept = set()
    for op, k in cases:
        where = (field, op) if k is None else (field, op, k)
        exp = np.array([FC.value_keeps(v, op, k) for v in vals], dtype=bool)
        got = P.filter_container(blob, where)
        assert np.array_equal(got, exp), (where, np.flatnonzero(got != exp)[:8])
        kept.add(int(exp.sum()))
    assert len(kept) > 1      # (the cases are not one mask)


# ---- 3. terms behind lists ---------------------------------------------------------------------------------------------------------
def test_terms_on_both_sides_of_the_arrays_and_maps():
    blob, recs = _file("ragged"), _recs()
    lo, hi = sorted(_first_and_last_created_at())
    mid = (lo + hi) // 2
    eight = [("age", ">=", 20), ("age", "<=", 75), ("age", "!=", 33), ("name", "not_null"), ("name", ">", "b"), ("name", "<", "y"),
             ("created_at", ">=", lo + 1), ("class", "!=", "C")]
    for where in ([("class", "!=", "A"), ("name", "not_null")],                  # the last filterable field and the first
                  [("created_at", ">=", lo + (mid - lo) // 2), ("created_at", "<", mid), ("name", "is_null")],      # a range on one field
                  eight):
        mask = FC.oracle_mask(recs, FULL, where)
        assert 0 < mask.sum() < N, where
        assert np.array_equal(P.filter_container(blob, where), mask)
        _same(P.read_container_where(blob, where, 2), FC.oracle_filtered(recs, FULL, where, 2, mask))


# ---- 4. codecs and roads --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inflate", ["host", "device"])
def test_a_deflate_file_on_both_roads(inflate):
    blob = _file("ragged", "deflate")
    assert P.container_info(blob).codec == "deflate"
    for pred in ("age>=30", "created_at>0", "age==-12345", "record 507 only"):
        assert np.array_equal(P.filter_container(blob, _where(pred), inflate=inflate), _mask(pred))
        got = P.read_container_where(blob, _where(pred), 3, inflate=inflate)
        _same(got, _expected(pred, 3))
        _same(got, P.read_container_where(_file("ragged"), _where(pred), 3))


# ---- 5. columns= / reader_schema= -----------------------------------------------------------------------------------------------------
def test_columns_without_the_predicate_field():
    where, cols = [("age", ">=", 40), ("class", "==", "A")], ["created_at", "name", "emails"]
    exp = [b.select(cols) for b in FC.oracle_filtered(_recs(), FULL, where, 3)]
    assert 0 < sum(b.num_rows for b in exp) < N
    for layout in ("ragged", "ones"):
        _same(P.read_container_where(_file(layout), where, 3, columns=cols), exp)
    _same(P.read_container_where(_file("ragged", "deflate"), where, 3, columns=cols, inflate="device"), exp)


def test_a_reader_schema():
    recs = _recs()
    values = [synth.gen_full(20260921, i) for i in range(N)]
    assert RC.writer_records(FULL, values) == recs
    where = [("age", "not_null"), ("class", "!=", "B")]      # `class` and `age` are kept and promoted by the reader, `age` to long
    mask = FC.oracle_mask(recs, FULL, where)
    assert 0 < mask.sum() < N
    kept_values = [v for v, m in zip(values, mask) if m]
    exp = FC.oracle_decode(RC.reader_records(FULL, RC.FULL_MIXED, kept_values), RC.FULL_MIXED, 3)
    _same(P.read_container_where(_file("ragged"), where, 3, reader_schema=RC.FULL_MIXED), exp)
    # ... with columns= of the reader on top, the predicate's fields not among them
    _same(P.read_container_where(_file("word_edges"), where, 3, reader_schema=RC.FULL_MIXED, columns=["name", "emails"]),
          [b.select(["name", "emails"]) for b in exp])


# ---- 6. the device form ---------------------------------------------------------------------------------------------------------------
def test_to_device_equals_the_host_call():
    for pred in ("age>=30", "created_at>0", "age==-12345"):
        for blob, kw in ((_file("ragged"), {}), (_file("ragged", "deflate"), {"inflate": "device"})):
            dec = P.read_container_where_to_device(blob, _where(pred), 3, **kw)
            assert dec.kept == int(_mask(pred).sum())
            assert [b.num_rows for b in dec.batches] == [e.num_rows for e in _expected(pred, 3)]
            host = dec.to_host()
            _same(host, _expected(pred, 3))
            _same(host, P.read_container_where(blob, _where(pred), 3, **kw))
            dec.free()


# ---- 7. errors: read_container's message, whatever the predicate says ----------------------------------------------------------------
def _oracle_message(recs, schema=FULL):
    with pytest.raises(ValueError) as e:
        c_walker.decode_threaded(list(recs), schema, 1)
    return str(e.value)


# the damaged record's `age` is intact and in front of the damage: exactly one of the first two matches it; `created_at` lies
# behind the damage of two of the kinds: every record matches the third, none the fourth
ERROR_PREDICATES = [("age", "not_null"), ("age", "is_null"), ("created_at", ">", 0), ("created_at", "<", 0)]
BAD_AT = 150      # the 150th of the 300 records of block 2 of the ragged file


def _raises(blob, message, **kw):
    with pytest.raises(ValueError) as e:
        P.read_container(blob, 1, **kw)
    assert str(e.value) == message
    for where in ERROR_PREDICATES:
        for f in (lambda: P.read_container_where(blob, where, 2, **kw), lambda: P.filter_container(blob, where, **kw),
                  lambda: P.read_container_where_to_device(blob, where, 1, **kw)):
            with pytest.raises(ValueError) as e:
                f()
            assert str(e.value) == message, where


@pytest.mark.parametrize("kind", sorted(CC.DAMAGE_MESSAGES))
def test_record_errors(kind):
    recs = _recs()
    bad = CC.damaged_full(kind, BAD_AT)
    recs[BAD_AT] = bad
    # the precondition, on the oracle alone: the verdict does not depend on where the damaged record ends
    alone = _oracle_message([bad])
    assert alone == CC.DAMAGE_MESSAGES[kind]
    assert _oracle_message([bad + b"".join(recs[BAD_AT + 1:BAD_AT + 20])]) == alone
    assert _oracle_message(recs) == alone
    first = np.cumsum([0] + CC.RAGGED)
    assert first[2] < BAD_AT < first[3] - 1
    blocks = CC.split(recs, CC.RAGGED)
    _raises(CC.write(FULL, blocks), alone)
    _raises(CC.write(FULL, blocks, "deflate"), alone, inflate="device")


def test_block_count_errors_and_the_lowest_of_two():
    recs = _recs()
    blocks = CC.split(recs, CC.RAGGED)
    hdr = CC.header(FULL, "null")

    def file_with(short_block, bad_record=None, kind="enum"):
        out = [hdr]
        at = 0
        for b, blk in enumerate(blocks):
            blk = list(blk)
            if bad_record is not None and at <= bad_record < at + len(blk):
                blk[bad_record - at] = CC.damaged_full(kind, bad_record)
            out.append(CC.block(blk, count=len(blk) - 1 if b == short_block else None))
            at += len(blk)
        return b"".join(out)

    def end_message(b):
        size = sum(map(len, blocks[b]))
        return f"container: block {b}: its {len(blocks[b]) - 1} records end at byte {size - len(blocks[b][-1])} of {size}"

    assert (len(blocks[2]), len(blocks[5])) == (300, 64)
    _raises(file_with(5), end_message(5))                 # a block whose header claims one record fewer than it holds
    _raises(file_with(2), end_message(2))
    first = np.cumsum([0] + CC.RAGGED)
    in5 = int(first[5]) + 10
    assert first[5] <= in5 < first[6]
    # two damaged blocks: the lowest wins, either kind first
    _raises(file_with(2, bad_record=in5), end_message(2))
    _raises(file_with(5, bad_record=BAD_AT), CC.DAMAGE_MESSAGES["enum"])
    _raises(file_with(None, bad_record=in5, kind="bool"), CC.DAMAGE_MESSAGES["bool"])


# ---- 8. empty shapes and the trailing bytes of a block's last record --------------------------------------------------------------
@pytest.mark.parametrize("blocks", [[], [[], [], []]], ids=["no_blocks", "only_empty_blocks"])
def test_empty_shapes(blocks):
    for codec, kw in (("null", {}), ("deflate", {"inflate": "device"}), ("deflate", {"inflate": "host"})):
        blob = CC.write(FULL, blocks, codec)
        assert P.container_info(blob).num_records == 0
        for where in (("age", ">=", 30), ("created_at", ">", 0)):
            mask = P.filter_container(blob, where, **kw)
            assert mask.dtype == np.bool_ and mask.shape == (0,)
            for k in (1, 4):
                got = P.read_container_where(blob, where, k, **kw)
                assert len(got) == 1 and got[0].num_rows == 0
                _same(got, c_walker.decode_threaded([], FULL, k))
    dec = P.read_container_where_to_device(CC.write(FULL, blocks), ("age", ">=", 30), 2)
    assert dec.kept == 0
    _same(dec.to_host(), c_walker.decode_threaded([], FULL, 2))


def test_nothing_kept_is_the_decode_of_the_empty_list():
    for k in (1, 4):
        got = P.read_container_where(_file("ragged"), _where("age==-12345"), k)
        assert len(got) == 1 and got[0].num_rows == 0
        _same(got, c_walker.decode_threaded([], FULL, k))


def test_the_last_record_of_every_block_alone():
    """The last record of a `null` block runs on over the sync marker and the next block's header: the gather copies those bytes
    with the record and the decoder ignores them.  Keep exactly the last record of every block."""
    recs = _recs()
    counts = [c for c in CC.RAGGED]
    last = np.zeros(N, dtype=bool)
    at = 0
    for c in counts:
        at += c
        if c:
            last[at - 1] = True
    col = FC.oracle_decode(recs, FULL, 1)[0].column("created_at").to_pylist()
    assert len(set(col)) == N
    # (at most 8 terms: the last records of the first blocks that hold one, by their unique created_at -- ANDed terms keep one
    #  record each, so the file is read once per record and the results are compared one by one)
    picks = [int(i) for i in np.flatnonzero(last)[:4]] + [int(np.flatnonzero(last)[-1])]
    for i in picks:
        where = ("created_at", "==", col[i])
        mask = P.filter_container(_file("ragged"), where)
        assert mask.sum() == 1 and mask[i]
        _same(P.read_container_where(_file("ragged"), where, 1), c_walker.decode_threaded([recs[i]], FULL, 1))
    # ... and a predicate that keeps a run up to a block's end and drops the next block's first records
    edge = int(np.flatnonzero(last)[1])      # the last of the 300-record block
    where = [("created_at", ">=", min(col[edge - 2:edge + 1])), ("created_at", "<=", max(col[edge - 2:edge + 1]))]
    mask = FC.oracle_mask(recs, FULL, where)
    assert mask[edge]
    assert np.array_equal(P.filter_container(_file("ragged"), where), mask)
    _same(P.read_container_where(_file("ragged"), where, 2), FC.oracle_filtered(recs, FULL, where, 2, mask))
