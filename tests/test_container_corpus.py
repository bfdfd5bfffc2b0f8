"""Container reads on every schema family the decoder is tested on: the block split (``rh_k_split``,
``rh_k_split_salvage``) finds every record boundary itself, so every corpus of tests/cases.py, tests/random_cases.py,
tests/test_n4_types.py and tests/test_named_refs.py goes through ``read_container`` here, in three block layouts, and the edges
only that kernel has are met on purpose: lanes that diverge inside deep multi-block lists, the minimum-record-bytes refusal, records
of zero bytes, malformed records at wavefront and workgroup edges.

The contract is the one of tests/test_container.py:

    read_container(F, k) == oracle(records_of(F), W, k)      buffer for buffer, batch for batch

The files are written by the tests' own writer (tests/container_cases.py) around the corpus schema text as it is; the expected
batches are the ORACLE's decode of the records put into the file and the messages are those of ``cases.error_cases()`` -- never the
engine's own output.  tests/container_corpus.py states which records are repaired or subset, and why; nothing else is left out."""
import functools
import json

import pytest

import cases
import container_cases as CC
import container_corpus as K
from avrogen.encoder import Blocks, to_datum
from avrogen.schemas import SCHEMAS
from oracle import avro_schema as S
from oracle import py_encoder

import pyruhvro_amd as P
from pyruhvro_amd import cabi
from test_resolution import _same

KERNELS = {"generic": cabi.KERNEL_GENERIC, "specialized": cabi.KERNEL_SPECIALIZED}
CASE_IDS = list(K.CASE_IDS)
EDGE_LANES = (0, 63, 64, 255, 256)      # wavefront and workgroup edges of a 256-lane workgroup


@pytest.fixture(params=sorted(KERNELS))
def kernel(request):
    old = P.set_kernel_mode(request.param)
    yield KERNELS[request.param]
    P.set_kernel_mode(old)


@pytest.fixture
def generic():
    """The schemas this file invents run on the generic kernels only: no test waits for a compile."""
    old = P.set_kernel_mode("generic")
    yield cabi.KERNEL_GENERIC
    P.set_kernel_mode(old)


@pytest.fixture(scope="module", autouse=True)
def _release():
    """Nothing is generated on import or for a test that does not use it (container_corpus builds a family when a test first asks
    for one of its cases); what the tests of this file shared -- records, files, expected batches -- is dropped when the last ends."""
    yield
    K.clear()
    for f in (_nested_case, _errors, _round_trip_inputs, _diverging_kinds):
        f.cache_clear()


def _raises(fn, *a, **kw) -> str:
    with pytest.raises(ValueError) as e:
        fn(*a, **kw)
    return str(e.value)


# ---- 1. CPU: the corpus is fit for a container --------------------------------------------------------------------------------------
def test_every_record_is_consumed_to_its_last_byte():
    """A record may go into a container only if the walk ends on its last byte: the oracle must refuse it with that byte cut off.
    Exactly the records of container_corpus.REPAIRS fail that (26 of 20,505); with their tail taken off they pass."""
    tails = {}
    total = 0
    for c in K.raw_corpus():
        for i, r in enumerate(c.records):
            total += 1
            if not r or K.oracle_accepts([r[:-1]], c.schema):
                tails[(c.id, i)] = None
    assert set(tails) == set(K.REPAIRS), sorted(set(tails) ^ set(K.REPAIRS))
    assert total == sum(len(c.records) for c in K.raw_corpus()) > 20_000
    raw = {c.id: c for c in K.raw_corpus()}
    for c in K.repaired_corpus():
        assert len(c.records) == len(raw[c.id].records)
        for i, (r, r0) in enumerate(zip(c.records, raw[c.id].records)):
            if (c.id, i) in K.REPAIRS:
                assert r0 == r + K.REPAIRS[(c.id, i)]
                assert K.oracle_accepts([r], c.schema) and not K.oracle_accepts([r[:-1]], c.schema)
            else:
                assert r is r0 or r == r0


def test_the_subset_rule_and_the_size_caps():
    repaired = {c.id: c for c in K.repaired_corpus()}
    assert [c.id for c in K.corpus()] == list(repaired) == CASE_IDS and {c.family for c in K.corpus()} == set(K.FAMILIES)
    for c in K.corpus():
        full = repaired[c.id].records
        if c.id in K.SUBSET_CASES:
            assert len(full) > K.SUBSET_HEAD
            assert c.records[:K.SUBSET_HEAD] == full[:K.SUBSET_HEAD] and len(c.records) == K.SUBSET_HEAD + 1
            assert len(c.records[-1]) == max(map(len, full)) > K.BLOCK_CAP
        else:
            assert c.records == full                       # nothing else is left out
        for layout in K.LAYOUTS:
            recs = K.layout_records(c, layout)
            blocks = K.blocks_of(c, layout)
            assert [r for b in blocks for r in b] == list(recs)                  # every record, in order
            assert sum(map(len, recs)) <= K.FILE_CAP, (c.id, layout)
            for b in blocks:
                assert len(b) == 1 or sum(map(len, b)) <= K.BLOCK_CAP, (c.id, layout)
            if layout == "ones":
                assert all(len(b) == 1 for b in blocks) and recs[:len(c.records)] == c.records
                assert len(blocks) >= K.ONES_BLOCKS or sum(map(len, c.records)) * -(-K.ONES_BLOCKS // len(c.records)) > K.FILE_CAP
            else:
                assert recs == c.records
            if layout == "ragged":      # the counts of the cycle, except where the cap or the end of the records closed a block early
                for i, b in enumerate(blocks[:-1]):
                    want = K.RAGGED_COUNTS[i % len(K.RAGGED_COUNTS)]
                    assert len(b) == want or (len(b) < want and sum(map(len, b)) + len(recs[sum(map(len, blocks[:i + 1]))]) > K.BLOCK_CAP)
            if layout == "one_block" and sum(map(len, recs)) <= K.BLOCK_CAP:
                assert len(blocks) == 1
            parsed = CC.read(K.file_of(c.id, layout))
            assert parsed.schema == c.schema and [(n, p) for n, p in parsed.blocks] == [(len(b), b"".join(b)) for b in blocks]
    # the giant records sit in blocks of their own
    for cid in ("giant_record/giant_arrays", "giant_record/giant_nested"):
        for layout in K.LAYOUTS:
            for b in K.blocks_of(K.case(cid), layout):
                assert len(b) <= 1 or max(map(len, b)) <= K.BLOCK_CAP


def test_the_shortest_datum_of_every_schema_on_the_oracle():
    """container_corpus.min_datum states the rule; here the oracle accepts the datum, alone and 65 times over, and refuses it one
    byte short."""
    assert len(K.min_schemas()) >= 60
    for name, schema in K.min_schemas():
        d = K.min_record(schema)
        assert d and K.oracle_accepts([d], schema) and K.oracle_accepts([d] * 65, schema), name
        assert not K.oracle_accepts([d[:-1]], schema), name
        assert K.oracle([d] * 65, schema, 1)[0].num_rows == 65
    assert set(MIN_BYTES_UNDER) <= {n for n, _ in K.min_schemas()}


# ---- 2. GPU: every corpus case through the container road ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("layout", K.LAYOUTS)
@pytest.mark.parametrize("cid", CASE_IDS)
def test_corpus_layouts(kernel, cid, layout, k):
    blob = K.file_of(cid, layout)
    info = P.container_info(blob)
    assert info.schema == K.case(cid).schema and info.num_records == len(K.layout_records(K.case(cid), layout))
    assert info.num_blocks == len(K.blocks_of(K.case(cid), layout))
    _same(P.read_container(blob, k), K.expected(cid, layout, k))


@pytest.mark.gpu
@pytest.mark.parametrize("road", ["host", "device"])
@pytest.mark.parametrize("cid", CASE_IDS)
def test_corpus_deflate_on_both_inflate_roads(kernel, cid, road):
    blob = K.file_of(cid, "ragged", "deflate")
    assert P.container_info(blob).codec == "deflate"
    _same(P.read_container(blob, 3, inflate=road), K.expected(cid, "ragged", 3))


@pytest.mark.gpu
@pytest.mark.parametrize("cid", CASE_IDS)
def test_corpus_tolerant_read_of_a_sound_file(kernel, cid):
    got, errors = P.read_container_tolerant(K.file_of(cid, "ragged"), 3)
    assert errors == []
    last = cabi.salvage_last()
    assert last["bytes_gathered"] == 0 and last["blocks_reported"] == 0
    _same(got, K.expected(cid, "ragged", 3))


# one layout per family for the device-resident form
DEVICE_LAYOUT = {f: K.LAYOUTS[i % len(K.LAYOUTS)] for i, f in enumerate(K.FAMILIES)}


@pytest.mark.gpu
@pytest.mark.parametrize("cid", CASE_IDS)
def test_corpus_device_resident(kernel, cid):
    layout = DEVICE_LAYOUT[K.case(cid).family]
    dec = P.read_container_to_device(K.file_of(cid, layout), 3)
    exp = K.expected(cid, layout, 3)
    assert [b.num_rows for b in dec.batches] == [b.num_rows for b in exp]
    _same(dec.to_host(), exp)
    dec.free()


# ---- 3. GPU: edges that only this kernel has ----------------------------------------------------------------------------------------
I64MIN = CC.zz(-(1 << 63))
ARRAY_STR = SCHEMAS["t_array_str"]
# An array of `null` items: the items take no bytes on the wire (Builder::min_bytes of AV_NULL is 0), so every block count of
# the list takes the exact path of h_list_next / list_next_slow (`op.buf2 == 0`), whose trip count nothing but the count bounds.
# Both sides take the schema: the oracle decodes it to list<item: null>.  This file invents it: generic kernels only.
ARRAY_NULL = '{"type":"record","name":"ZN","fields":[{"name":"a","type":{"type":"array","items":"null"}},{"name":"t","type":"int"}]}'
ZERO_WIDTH_MAX = 0xFFFFFF      # walk.h list_next_slow: a larger block count of zero-width items is E_LIST_RANGE


@functools.lru_cache(maxsize=None)
def _nested_case():
    return next(c for c in cases.nesting_cases() if c[0] == "nested_lists")


def _array_str_kinds():
    """The five blocks of the diverging-neighbours pattern on t_array_str (the records of cases.wire_cases)."""
    wire = {c[0]: c for c in cases.wire_cases()}
    sa = S.parse_schema(ARRAY_STR)
    blocks_70 = wire["array_blocks"][2][1]
    assert blocks_70 == to_datum(sa, {"tags": Blocks([(["x"] * 70, False), (["y"] * 3, True)])})
    short = [to_datum(sa, {"tags": [f"t{i}"] * (i % 3)}) for i in range(64)]
    return [[], [to_datum(sa, {"tags": []})], [blocks_70], list(wire["array_block_count_i64_min"][2]), short]


def _nested_kinds():
    """The same five on the nested-list schema of cases.nesting_cases: a 70-item positive block of inner lists followed by a
    negative-count block, the i64::MIN forms at both list levels, 64 of the case's own short records."""
    nested = _nested_case()
    sn = S.parse_schema(nested[1])
    inner = lambda j: Blocks([([None, f"s{j}"], j % 2 == 0), ([f"t{j}"] * (1 + j % 3), True)])      # noqa: E731
    deep = to_datum(sn, {"ll": Blocks([([inner(j) for j in range(70)], False), ([inner(70), [], ["z"]], True)]),
                         "lr": Blocks([([None, {"flag": True, "v": 5, "m": Blocks([([("k", None), ("l", True)], True)])}], True), ([None], False)]),
                         "id": 70})
    item = lambda s: CC.zz(1) + CC.zz(len(s)) + s      # noqa: E731      (the string branch of ["null", "string"])
    inner1 = CC.zz(1) + item(b"p") + I64MIN + CC.zz(123456) + CC.zz(0)           # one item, an empty i64::MIN block, the end
    inner2 = I64MIN + CC.zz(0) + I64MIN + CC.zz(5) + CC.zz(0)                      # two empty blocks, the end
    i64min = [I64MIN + CC.zz(5) + CC.zz(2) + inner1 + inner2 + CC.zz(0) + CC.zz(0) + CC.zz(7),
              CC.zz(1) + inner2 + I64MIN + CC.zz(0) + CC.zz(0) + I64MIN + CC.zz(9) + CC.zz(0) + CC.zz(8),
              to_datum(sn, {"ll": [["plain"]], "lr": [], "id": 9})]
    return [[], [to_datum(sn, {"ll": [], "lr": [], "id": 1})], [deep], i64min, list(nested[2][:60]) + list(nested[2][:4])]


def _null_items(*blocks, t=0) -> bytes:
    """An ARRAY_NULL record: (count, byte size or None) per block of the array -- a negative count is written with its byte
    size, which the decoders ignore (fast_decode.rs:689-700), i64::MIN is an empty block -- then the terminator and `t`."""
    return b"".join(CC.zz(n) + (b"" if size is None else CC.zz(size)) for n, size in blocks) + CC.zz(0) + CC.zz(t)


def _array_null_kinds():
    """The same five on ARRAY_NULL: the 70-item positive block is followed by a negative-count block whose byte size is the truth
    (0); the i64::MIN forms are those of array_block_count_i64_min with the item bytes gone."""
    m = -(1 << 63)
    i64min = [_null_items((m, 5), (2, None), t=7), _null_items((1, None), (m, 0), (m, 123456), t=8), _null_items((1, None), t=9)]
    short = [_null_items(*[(i % 3, None)] * (1 if i % 3 else 0), t=i - 30) for i in range(64)]
    return [[], [_null_items(t=1)], [_null_items((70, None), (-3, 0), t=70)], i64min, short]


@functools.lru_cache(maxsize=None)
def _diverging_kinds(which):
    """-> (schema, the five kinds of block): built once, never modified"""
    schema, kinds = {"array_str": lambda: (ARRAY_STR, _array_str_kinds()), "nested_lists": lambda: (_nested_case()[1], _nested_kinds()),
                     "array_null": lambda: (ARRAY_NULL, _array_null_kinds())}[which]()
    assert len(kinds) == 5 and kinds[0] == [] and len(kinds[1]) == len(kinds[2]) == 1 and len(kinds[3]) == 3 and len(kinds[4]) == 64
    return schema, kinds


def _diverging(which, rotation):
    """-> (schema, kinds, the 260 blocks of one rotation): adjacent lanes of one wavefront hold, in turn: an empty block, a record
    with an empty array, a 70-item positive block followed by a negative-count block, the i64::MIN forms, a block of 64 short
    records -- so a lane inside a multi-block list sits next to lanes that are idle, finished, or in a different block of the
    same list.  Over the five rotations every lane of EDGE_LANES holds every one of the five."""
    schema, kinds = _diverging_kinds(which)
    blocks = [kinds[(b + rotation) % 5] for b in range(260)]
    assert len(blocks) > max(EDGE_LANES)
    return schema, kinds, blocks


def _check_diverging_reads(which, rotation, codec):
    schema, _, blocks = _diverging(which, rotation)
    recs = [r for b in blocks for r in b]
    blob = CC.write(schema, blocks, codec)
    for k in (1, 3):
        _same(P.read_container(blob, k), K.oracle(recs, schema, k))


def _check_diverging_tolerant(which, rotation):
    schema, _, blocks = _diverging(which, rotation)
    got, errors = P.read_container_tolerant(CC.write(schema, blocks), 2)
    assert errors == []
    _same(got, K.oracle([r for b in blocks for r in b], schema, 2))


def _check_diverging_failed_lane(which, rotation, bad):
    """... and next to a lane that has FAILED: one edge lane holds a malformed record between two good ones.  Its verdict does not
    depend on where it ends (the precondition, on the oracle); the strict read raises it, the tolerant read keeps the record in
    front of it and every other block while the failed lane sits the rest of the walk out."""
    schema, kinds, blocks = _diverging(which, rotation)
    lane = EDGE_LANES[rotation]
    good = kinds[1][0]
    message = K.oracle_message([bad], schema)
    assert message == K.oracle_message([bad + good + CC.SYNC], schema) and "end of buffer" not in message
    damaged = list(blocks)
    damaged[lane] = [good, bad, good]
    blob = CC.write(schema, damaged)
    assert _raises(P.read_container, blob, 1) == message
    got, errors = P.read_container_tolerant(blob, 2)
    assert [(e.block, e.kept, e.lost, e.message) for e in errors] == [(lane, 1, 2, message)]
    damaged[lane] = [good]
    _same(got, K.oracle([r for b in damaged for r in b], schema, 2))


# (one read per k in a test, one test per codec: a test of this file is to cost no more than one of tests/test_container.py)
@pytest.mark.gpu
@pytest.mark.parametrize("codec", ["null", "deflate"])
@pytest.mark.parametrize("rotation", range(5))
@pytest.mark.parametrize("which", ["array_str", "nested_lists"])
def test_diverging_neighbours(kernel, which, rotation, codec):
    _check_diverging_reads(which, rotation, codec)


@pytest.mark.gpu
@pytest.mark.parametrize("rotation", range(5))
@pytest.mark.parametrize("which", ["array_str", "nested_lists"])
def test_diverging_neighbours_tolerant(kernel, which, rotation):
    _check_diverging_tolerant(which, rotation)


@pytest.mark.gpu
@pytest.mark.parametrize("rotation", range(5))
@pytest.mark.parametrize("which", ["array_str", "nested_lists"])
def test_diverging_neighbours_and_a_failed_lane(kernel, which, rotation):
    # a negative string length / union branch 5
    _check_diverging_failed_lane(which, rotation, CC.zz(1) + (CC.zz(-3) if which == "array_str" else CC.zz(1) + CC.zz(5)))


# Zero-width list items.
def _array_null_records():
    """Positive counts, negative counts with byte sizes (true and untrue), several blocks, i64::MIN counts, counts of one, two and
    three varint bytes, the empty array.  A lane makes one trip per item, measured at a few microseconds each, so the one count of
    three bytes is the smallest there is (8,192 items, in record 7 alone), far below ZERO_WIDTH_MAX."""
    m = -(1 << 63)
    forms = [[(3, None)], [(-4, 0)], [(3, None), (-2, 77), (70, None)], [(m, 5), (2, None), (m, 0)], [], [(64, None)], [(-100, 0)],
             [(300, None)], [(1, None)] * 9, [(m, 0)], [(-1, 1), (1, None), (-1, 0)]]
    once = {7: [(8192, None)]}
    return tuple(_null_items(*once.get(i, forms[i % len(forms)]), t=i * 37 - 500) for i in range(300))


def test_the_zero_width_items_on_the_oracle():
    recs = _array_null_records()
    got = K.oracle(recs, ARRAY_NULL, 1)[0]
    assert str(got.schema.field("a").type) == "list<item: null>" == str(P.arrow_schema(ARRAY_NULL).field("a").type)
    assert [len(x) for x in got.column(0).to_pylist()][:11] == [3, 4, 75, 2, 0, 64, 100, 8192, 9, 0, 3]
    assert got.column(1).to_pylist() == [i * 37 - 500 for i in range(300)]
    assert all(not K.oracle_accepts([r[:-1]], ARRAY_NULL) for r in recs)
    for rotation in range(5):
        schema, _, blocks = _diverging("array_null", rotation)
        assert K.oracle([r for b in blocks for r in b], schema, 1)[0].num_rows == 52 * (0 + 1 + 1 + 3 + 64)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("road", ["null", "deflate", "tolerant"])
@pytest.mark.parametrize("layout", K.LAYOUTS)
def test_zero_width_items_layouts(generic, layout, road, k):
    c = K.Case("invented/array_null", "invented", ARRAY_NULL, _array_null_records())
    recs, blocks = K.layout_records(c, layout), K.blocks_of(c, layout)
    assert [r for b in blocks for r in b] == list(recs)
    if road == "tolerant":
        got, errors = P.read_container_tolerant(CC.write(ARRAY_NULL, blocks), k)
        assert errors == []
    else:
        got = P.read_container(CC.write(ARRAY_NULL, blocks, road), k)
    _same(got, K.oracle(recs, ARRAY_NULL, k))


@pytest.mark.gpu
@pytest.mark.parametrize("codec", ["null", "deflate"])
@pytest.mark.parametrize("rotation", range(5))
def test_zero_width_items_diverging_neighbours(generic, rotation, codec):
    _check_diverging_reads("array_null", rotation, codec)


@pytest.mark.gpu
@pytest.mark.parametrize("rotation", range(5))
def test_zero_width_items_diverging_neighbours_tolerant(generic, rotation):
    _check_diverging_tolerant("array_null", rotation)


@pytest.mark.gpu
@pytest.mark.parametrize("rotation", range(5))
def test_zero_width_items_diverging_neighbours_and_a_failed_lane(generic, rotation):
    _check_diverging_failed_lane("array_null", rotation, CC.zz(1) + CC.zz(0) + b"\xff" * 10)      # `t`: a varint of more than ten bytes


@pytest.mark.gpu
@pytest.mark.parametrize("lane", [63, 64, 256])
@pytest.mark.parametrize("count", [ZERO_WIDTH_MAX + 1, -(ZERO_WIDTH_MAX + 1), 1 << 40])
def test_a_block_count_of_zero_width_items_beyond_the_range(generic, count, lane):
    """The one limit of the list walk that the reference does not have (program.h E_LIST_RANGE: "no reference message"): the text
    is the engine's own, engine_kernels.cpp format_error.  The oracle has no such limit -- it is not asked for 16 million items --
    so what is asserted is the documented refusal, not a value."""
    good = _array_null_records()[11:]      # (the records behind the one long list)
    blocks = [list(good[b % 250:b % 250 + 5 + b % 17]) for b in range(300)]
    blocks[lane] = [good[0], _null_items((count, 0 if count < 0 else None), t=1), good[1]]
    message = f"array/map block count {abs(count)} of zero-width items exceeds the supported range"
    for codec in ("null", "deflate"):
        assert _raises(P.read_container, CC.write(ARRAY_NULL, blocks, codec), 1) == message
    got, errors = P.read_container_tolerant(CC.write(ARRAY_NULL, blocks), 2)
    assert [(e.block, e.kept, e.lost, e.message) for e in errors] == [(lane, 1, 2, message)]
    blocks[lane] = [good[0]]
    _same(got, K.oracle([r for b in blocks for r in b], ARRAY_NULL, 2))


# Minimum record bytes.  Builder::min_bytes (schema.cpp) bounds a block's record count before the launch: count x min > size is
# refused.  Under-counting a schema's minimum is legal (the walk finds out), over-counting refuses a valid file.  Which of the
# two each schema gives, recorded: the schemas below under-count (min_bytes takes a uuid string as one byte, the shortest uuid
# text is 33: the N4 schema's shortest record is 59 bytes, counted as 27); every other schema of the corpus is counted exactly.
# (In the corpus `fixed`, a decimal and a uuid on a fixed stand outside a list or union only in that N4 schema, where 32 bytes of
# under-count would hide an over-count of theirs: EXACT below pins them, kind by kind.)
MIN_BYTES_UNDER = ("n4/n4",)


def test_one_record_more_than_a_block_of_shortest_records_holds():
    """Not `gpu`: where min_bytes is exact, count + 1 is refused before any device work, by the host and the device-resident read."""
    for name, schema in K.min_schemas():
        if name in MIN_BYTES_UNDER:
            continue
        d = K.min_record(schema)
        blob = CC.header(schema, "null") + CC.block([d] * 65, count=66)
        for fn in (P.read_container, P.read_container_to_device):
            assert _raises(fn, blob, 1) == f"container: block 0: 66 records cannot be in its {65 * len(d)} bytes", name


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_IDS)
def test_a_block_of_shortest_records(kernel, name):
    """65 shortest records under an exact header read equal to the oracle: a kind whose minimum is over-counted fails here.  With
    count + 1 in the header the file is refused: before the launch (`records cannot be in its ... bytes`) where the minimum is
    exact; where it under-counts, the walk's 66th record starts on the block's last byte and DESIGN 14 "Errors" holds: "a
    record that runs out of bytes fails at the block's end instead of its own", with "what the list decode raises for it" --
    the oracle's message for an empty 66th record.  (`its N records end at byte` is the text of a count that is too LOW; a count
    that is too high cannot give it, the lane runs out of bytes first.)"""
    schema = K.case(name).schema
    d = K.min_record(schema)
    recs = [d] * 65
    blob = CC.write(schema, [recs])
    for k in (1, 3):
        _same(P.read_container(blob, k), K.oracle(recs, schema, k))
    size = 65 * len(d)
    msg = _raises(P.read_container, CC.header(schema, "null") + CC.block(recs, count=66), 1)
    if name in MIN_BYTES_UNDER:
        assert msg == K.oracle_message(recs + [b""], schema)
    else:
        assert msg == f"container: block 0: 66 records cannot be in its {size} bytes"
    # one record fewer than the block holds: the text of test_container.test_block_count_errors
    msg = _raises(P.read_container, CC.header(schema, "null") + CC.block(recs, count=64), 1)
    assert msg == f"container: block 0: its 64 records end at byte {size - len(d)} of {size}"


# Builder::min_bytes, kind by kind.  One record schema per kind the function has a case for, with that kind as its only field, and
# one whose fields are all of them, a nested record among them (record = sum).  Every datum of such a schema has one length, below
# 66 bytes, so the two assertions pin the function from both sides: 65 records under an exact header are read (min <= length: an
# over-count of one byte refuses the file), 66 claimed in the same bytes are refused before the launch (66 x min > 65 x length:
# min >= length).  These schemas are this file's own: generic kernels only.
_fixed = lambda name, size, **kw: dict({"type": "fixed", "name": name, "size": size}, **kw)      # noqa: E731
EXACT = {      # kind -> (the field's type, its bytes on the wire)
    "float": ("float", 4),
    "double": ("double", 8),
    "fixed": (_fixed("F5", 5), 5),
    "decimal_on_fixed": (_fixed("D7", 7, logicalType="decimal", precision=16, scale=2), 7),
    "uuid_on_fixed": (_fixed("U16", 16, logicalType="uuid"), 16),
    "duration": (_fixed("Du12", 12, logicalType="duration"), 12),
}


def _exact_schema(kind):
    """-> (schema text, bytes of a record)"""
    if kind != "record_sum":
        return json.dumps({"type": "record", "name": "X_" + kind, "fields": [{"name": "v", "type": EXACT[kind][0]}]}), EXACT[kind][1]
    inner = {"type": "record", "name": "In", "fields": [{"name": k, "type": EXACT[k][0]} for k in ("fixed", "double", "duration")]}
    fields = [{"name": "f", "type": "float"}, {"name": "in", "type": inner}, {"name": "df", "type": EXACT["decimal_on_fixed"][0]},
              {"name": "uf", "type": EXACT["uuid_on_fixed"][0]}, {"name": "i", "type": "int"}]
    return json.dumps({"type": "record", "name": "X_sum", "fields": fields}), 4 + (5 + 8 + 12) + 7 + 16 + 1


def _exact_records(kind):
    """65 records of the schema's one length: the shortest datum of the rule (zeros) first, then bytes that tell the records and
    their fields apart (a duration keeps its months at 0: no other has a value in Duration(ms))."""
    def value(k, i, salt=0):
        if i == 0:
            return bytes(EXACT[k][1])
        if k == "duration":
            return bytes(4) + (i + salt).to_bytes(4, "little") + (i * 7919).to_bytes(4, "little")
        raw = bytes((i + salt + j) % 127 for j in range(EXACT[k][1]))      # (a float or double of these bytes is a finite number)
        return bytes([raw[0] % 32]) + raw[1:] if k == "decimal_on_fixed" else raw      # big-endian, below 10^16: the precision
    if kind != "record_sum":
        return [value(kind, i) for i in range(65)]
    return [b"".join(value(k, i, n) for n, k in enumerate(("float", "fixed", "double", "duration", "decimal_on_fixed", "uuid_on_fixed")))
            + CC.zz(i % 64) for i in range(65)]


EXACT_KINDS = sorted(EXACT) + ["record_sum"]


@pytest.mark.parametrize("kind", EXACT_KINDS)
def test_min_bytes_of_a_kind_is_not_under_counted(generic, kind):
    """Not `gpu`: the oracle takes the records and their length is the shortest datum's; one record more than the block holds is
    refused before any device work."""
    schema, size = _exact_schema(kind)
    recs = _exact_records(kind)
    assert recs[0] == K.min_record(schema) and {len(r) for r in recs} == {size} and size < 66 and len(recs) == 65
    assert K.oracle(recs, schema, 1)[0].num_rows == 65 and not K.oracle_accepts(recs[:-1] + [recs[-1][:-1]], schema)
    blob = CC.header(schema, "null") + CC.block(recs, count=66)
    for fn in (P.read_container, P.read_container_to_device):
        assert _raises(fn, blob, 1) == f"container: block 0: 66 records cannot be in its {65 * size} bytes"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", EXACT_KINDS)
def test_min_bytes_of_a_kind_is_not_over_counted(generic, kind):
    schema, size = _exact_schema(kind)
    recs = _exact_records(kind)
    for codec in ("null", "deflate"):
        blob = CC.write(schema, [recs], codec)
        for k in (1, 3):
            _same(P.read_container(blob, k), K.oracle(recs, schema, k))
    got, errors = P.read_container_tolerant(CC.write(schema, [recs]), 1)
    assert errors == []
    _same(got, K.oracle(recs, schema, 1))
    msg = _raises(P.read_container, CC.header(schema, "null") + CC.block(recs, count=64), 1)
    assert msg == f"container: block 0: its 64 records end at byte {64 * size} of {65 * size}"


# Zero-byte RECORDS.  The oracle decodes EMPTY from b"" to a struct<> column, but the engine refuses a record without fields at any
# level, as the reference does when it finishes such a decoder (fast_decode.rs:634) -- so no container of zero-byte records of a
# schema that BOTH sides take exists: a record of `null` fields, the other schema whose records are empty, is taken by the engine
# and not by the oracle (pyarrow has no non-nullable null field).  That holds for records only: zero-width list ITEMS that both
# sides take exist (ARRAY_NULL above).  What is left to assert for records: both roads refuse the schemas of empty records with
# the list path's text, and the count limit of a schema whose records may be empty fires (its text is the engine's).
EMPTY = '{"type":"record","name":"E","fields":[{"name":"r","type":{"type":"record","name":"I","fields":[]}}]}'
EMPTY_ITEMS = json.dumps({"type": "record", "name": "EI", "fields": [
    {"name": "a", "type": {"type": "array", "items": {"type": "record", "name": "I", "fields": []}}}, {"name": "t", "type": "int"}]})
NULLS = '{"type":"record","name":"Z","fields":[{"name":"n","type":"null"}]}'


def test_schemas_of_empty_records_are_refused_on_both_roads_with_one_text(generic):
    text = "RecordDecoder produced a record with 0 fields"
    assert K.oracle([b""] * 3, EMPTY, 1)[0].num_rows == 3                   # (the oracle is the lenient side)
    for schema, rec in ((EMPTY, b""), (EMPTY_ITEMS, CC.zz(2) + CC.zz(0) + CC.zz(5))):
        counts = [0, 1, 1000, 64]
        blob = CC.write(schema, [[rec] * c for c in counts])
        assert P.container_info(blob).num_records == sum(counts)
        assert _raises(P.arrow_schema, schema) == text
        assert _raises(P.deserialize_array_threaded, [rec] * 3, schema, 1) == text
        for fn in (P.read_container, P.read_container_to_device, P.read_container_tolerant):
            assert _raises(fn, blob, 1) == text
            assert _raises(fn, CC.write(schema, [[rec] * c for c in counts], "deflate"), 1) == text


def test_the_count_limit_of_a_schema_whose_records_may_be_empty(generic):
    limit = 1 << 24
    with pytest.raises(ValueError):
        K.oracle([b""], NULLS, 1)                                             # (no oracle for this schema: the text below is the engine's)
    for counts in ([limit + 1], [limit, 0, 1]):
        blob = CC.header(NULLS, "null") + b"".join(CC.block([], count=c) for c in counts)
        assert P.container_info(blob).num_records == limit + 1
        for fn in (P.read_container, P.read_container_to_device, P.read_container_tolerant):
            msg = _raises(fn, blob, 1)
            assert msg == f"container: {limit + 1} records of a schema whose records may be empty: at most {limit} in one call"


# Record errors whose verdict does not depend on where the record ends, at wavefront and workgroup edges.  (The names are written
# out so that collecting the tests generates nothing; test_the_error_cases_are_all_placed holds them against the table.)
ANYWHERE = ("bad_bool", "bad_branch", "bad_branch_neg", "enum_negative", "enum_oor", "neg_strlen", "union_neg", "union_oor", "varint_too_long")
AT_THE_END = ("array_huge_count", "array_item_eob", "array_unterminated", "eob_bool", "eob_f32", "eob_f64", "eob_mid_varint", "eob_string",
              "eob_varint")


@functools.lru_cache(maxsize=None)
def _errors():
    return {c[0]: c for c in cases.error_cases()}


def test_the_error_cases_are_all_placed():
    names = sorted(_errors())
    assert sorted(ANYWHERE + AT_THE_END) == names
    assert list(ANYWHERE) == [n for n in names if n in ("bad_bool", "neg_strlen", "varint_too_long") or n.startswith(("enum_", "bad_branch", "union_"))]
    assert list(AT_THE_END) == [n for n in names if n.startswith(("eob_", "array_"))]


@pytest.mark.gpu
@pytest.mark.parametrize("lane", [63, 64, 256])
@pytest.mark.parametrize("name", ANYWHERE)
def test_record_errors_at_lane_edges(kernel, name, lane):
    _, schema, goods, bad, message = _errors()[name]
    goods = list(goods)
    # the neighbours hold longer blocks: they walk on long after the lane of the bad record has stopped
    blocks = [(goods * 8)[:5 + b % 17] for b in range(300)]
    blocks[lane] = goods[:2] + [bad] + goods[:2]
    blob = CC.write(schema, blocks)
    # the precondition, on the oracle alone: the verdict does not depend on where the damaged record ends
    at = blob.index(b"".join(blocks[lane])) + sum(map(len, goods[:2]))
    assert blob[at:at + len(bad)] == bad
    assert K.oracle_message([bad], schema) == message == K.oracle_message([blob[at:at + len(bad) + 64]], schema)
    assert _raises(P.read_container, blob, 1) == message
    assert _raises(P.read_container, CC.write(schema, blocks, "deflate"), 1) == message
    assert _raises(P.read_container_to_device, blob, 2) == message


@pytest.mark.gpu
@pytest.mark.parametrize("name", AT_THE_END)
def test_a_record_that_runs_out_of_bytes_at_the_end_of_the_file(kernel, name):
    """DESIGN 14 "Errors": "the message of a malformed record is what the list decode raises for it (`format_error`) whenever the
    failure does not depend on where the record ends [...]; a record that runs out of bytes fails at the block's end instead of
    its own."  For the LAST record of a block the two ends are one, so the message is the table's."""
    _, schema, goods, bad, message = _errors()[name]
    goods = list(goods)
    last = goods * 8 + [bad]
    assert K.oracle_message(last, schema) == message
    # (the last block is long enough for the count the header claims -- count x min_record_bytes <= size -- so the walk is what
    #  meets the record: behind three good records the refusal of the count, which comes before the launch, would be first)
    assert len(last) * len(K.min_record(schema)) <= sum(map(len, last))
    blocks = [(goods * 8)[:5 + b % 17] for b in range(70)] + [last]
    for codec in ("null", "deflate"):
        assert _raises(P.read_container, CC.write(schema, blocks, codec), 1) == message


# The writer's files through the reader, and through the tests' own reader and the oracle.
ROUND_TRIP = {f"seed_{seed}": "random/seed_%02d" % seed for seed in range(8)}      # name -> the corpus case whose schema and records it takes
ROUND_TRIP["n4"] = "n4/n4"


@functools.lru_cache(maxsize=None)
def _round_trip_inputs(name):
    """-> (schema, the oracle's batch of the case's records, the oracle encoder's datums of that batch): computed once, never
    modified"""
    c = K.case(ROUND_TRIP[name])
    batch = K.oracle(c.records, c.schema, 1)[0]
    datums = [x for a in py_encoder.serialize_record_batch(batch, c.schema, 1, extended=True) for x in a.to_pylist()]
    _same(K.oracle(datums, c.schema, 1), [batch])
    return c.schema, batch, datums


@pytest.mark.gpu
@pytest.mark.parametrize("codec", ["null", "deflate"])
@pytest.mark.parametrize("block_rows", [1, 7, 4096])
@pytest.mark.parametrize("name", sorted(ROUND_TRIP))
def test_writer_round_trip(kernel, name, block_rows, codec):
    schema, batch, datums = _round_trip_inputs(name)
    n = batch.num_rows
    blob = P.write_container(batch, schema, codec=codec, block_rows=block_rows)
    _same(P.read_container(blob), [batch])
    # the tests' own reader: the payloads are the oracle encoder's datums, which the oracle decodes to the same batch
    got = CC.read(blob)
    assert got.schema == schema and got.codec == codec
    assert [cnt for cnt, _ in got.blocks] == [min(block_rows, n - i) for i in range(0, n, block_rows)]
    at = 0
    for cnt, payload in got.blocks:
        assert payload == b"".join(datums[at:at + cnt])
        at += cnt
    assert at == n
