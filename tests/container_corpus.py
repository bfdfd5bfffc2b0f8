"""The inputs of tests/test_container_corpus.py: every (schema, records) corpus the list path is tested on, made fit for an Avro
object container and dealt to blocks.  Plain Python over the oracle: nothing here touches the code under test or a GPU.

  corpus()                        every Case(id, family, schema, records), repaired and subset by the rules below
  raw_corpus()                    the same cases before the repair
  blocks_of(case, layout)         the case's records dealt to blocks: "ones", "ragged", "one_block"
  oracle(records, schema, k)      the expected batches: the oracle's decode of those records
  min_datum(schema)               the shortest valid datum of a schema, by the rule written at the function

THE RULES.  They are all of them: no case and no record is left out for any other reason.

  Repair.   In a container nothing bounds a record but the walk, so a record with bytes behind its datum cannot be put into one.
            REPAIRS lists the records of the corpus that carry such a tail (the 4-byte tail of cases.wire_cases "array_blocks" and
            the 3-byte tail random_cases.random_case appends for about half of its seeds) with the number of bytes taken off.
  Subset.   SUBSET_CASES ("wide_forms", "giant_arrays", "giant_nested": 24 MB, 6.7 MB and 2 MB of records) take their first 64
            records plus their largest record.  DESIGN 14 measures a split lane at about 4 MB/s, and a test may take a few seconds.
  Blocks.   A block that is not a single record holds at most BLOCK_CAP (256 KB) of payload: a layout closes a block early
            instead of passing the cap, so a record larger than the cap sits in a block of its own (every giant record does).
  Files.    A file holds at most FILE_CAP (4 MB) of payload; the CPU test asserts both caps on every file.
  Layouts.  ones       one record per block; a case of fewer than 257 records is cycled until it has 257 blocks (a workgroup of
                       the split kernel is 256 lanes), unless that would pass FILE_CAP: then every record once.
            ragged     block counts cycle through RAGGED_COUNTS; the last block takes what is left.
            one_block  all records in one block (in as few blocks as BLOCK_CAP allows).
"""
from __future__ import annotations

import functools
from collections import namedtuple
from typing import Dict, List, Sequence, Tuple

import cases
import container_cases as CC
import random_cases
from avrogen.encoder import to_datum
from oracle import avro_schema as S
from oracle import c_walker, py_walker

Case = namedtuple("Case", ["id", "family", "schema", "records"])

BLOCK_CAP = 256 * 1024
FILE_CAP = 4 * 1024 * 1024
RAGGED_COUNTS = (0, 1, 9, 0, 64, 2, 3)
LAYOUTS = ("ones", "ragged", "one_block")
ONES_BLOCKS = 257
SUBSET_CASES = ("wide_form/wide_forms", "giant_record/giant_arrays", "giant_record/giant_nested")
SUBSET_HEAD = 64
RANDOM_RECORDS = 300

# (case id, record index) -> bytes behind the datum, taken off.  Found with the oracle (test_every_record_is_consumed_to_its_last_byte
# asserts that these, and only these, decode with their last byte cut off).
REPAIRS: Dict[Tuple[str, int], bytes] = {("wire/array_blocks", 3): b"\xde\xad\xbe\xef"}
REPAIRS.update({(f"random/seed_{seed:02d}", index): b"\x01\x02\x03" for seed, index in (
    (0, 92), (1, 31), (2, 101), (6, 229), (7, 187), (11, 141), (13, 18), (14, 254), (15, 76), (17, 61), (18, 171), (19, 249),
    (20, 218), (21, 63), (22, 96), (23, 117), (25, 25), (28, 203), (31, 197), (32, 139), (33, 77), (35, 244), (36, 103), (37, 144),
    (38, 49))})


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _on_c_walker(schema: str) -> bool:
    """The C walker restates the reference, whose gate rejects the N4 types and named-type references; for those the oracle is
    its Python walker in the extended form (as in tests/test_n4_types.py, tests/test_named_refs.py, tests/test_gpu_parity.py)."""
    return S.is_supported(S.parse_schema(schema))


@functools.lru_cache(maxsize=None)
def _compiled(schema: str):
    return c_walker.CompiledSchema(schema)


def oracle(records: Sequence[bytes], schema: str, k: int):
    """The oracle's k batches of the records (the reference's chunk rule, deserialize.rs:53-58)."""
    records = list(records)
    if _on_c_walker(schema):
        return c_walker.decode_threaded(records, schema, k)
    n = len(records)
    k = min(max(k, 1), max(n, 1))
    sz = n // k
    return [py_walker.decode(records[c * sz: (c + 1) * sz if c + 1 < k else n], schema, extended=True) for c in range(k)]


def oracle_accepts(records: Sequence[bytes], schema: str) -> bool:
    """Whether the oracle decodes the records (nothing is assembled on the C walker: this runs once per record of the corpus)."""
    try:
        if _on_c_walker(schema):
            data, offsets = c_walker.pack(records)
            c_walker.decode_packed(_compiled(schema), data, offsets, 1, threaded=False, materialize=False)
        else:
            py_walker.decode(list(records), schema, extended=True)
        return True
    except ValueError:
        return False


def oracle_message(records: Sequence[bytes], schema: str) -> str:
    try:
        oracle(records, schema, 1)
    except ValueError as e:
        return str(e)
    raise AssertionError("the oracle accepts the records")


# ---- the corpus ------------------------------------------------------------------------------------------------------------------
# Every family is generated when a test first asks for one of its cases, not on import and not for a test that does not use it
# (wide_forms alone is 24 MB of records); clear() drops everything this module holds, the test file calls it when its last test ends.
def _table_family(family: str, table) -> List[Case]:
    return [Case(f"{family}/{c[0]}", family, c[1], tuple(c[2])) for c in table()]


def _random_family() -> List[Case]:
    out = []
    for seed in range(random_cases.PREBUILT_SEEDS):
        schema, recs = random_cases.random_case(seed, RANDOM_RECORDS)
        out.append(Case(f"random/seed_{seed:02d}", "random", schema, tuple(recs)))
    return out


def _n4_family() -> List[Case]:
    import test_n4_types as N4
    return [Case("n4/n4", "n4", N4.SCHEMA, tuple(N4._records(300))),
            Case("n4/duration", "n4", N4.DUR_SCHEMA, tuple(N4._dur_records(300)))]


def _named_refs_family() -> List[Case]:
    import test_named_refs as NR
    tree = S.parse_schema(NR.WITH_REFS, resolve_refs=True)
    return [Case("named_refs/with_refs", "named_refs", NR.WITH_REFS, tuple(to_datum(tree, r) for r in NR._rows(300)))]


_GENERATORS = {
    "wire": lambda: _table_family("wire", cases.wire_cases), "nesting": lambda: _table_family("nesting", cases.nesting_cases),
    "differential": lambda: _table_family("differential", cases.differential_cases),
    "dense_list": lambda: _table_family("dense_list", cases.dense_list_cases),
    "enum_form": lambda: _table_family("enum_form", cases.enum_form_cases),
    "wide_counter": lambda: _table_family("wide_counter", cases.wide_counter_cases),
    "wide_form": lambda: _table_family("wide_form", cases.wide_form_cases),
    "giant_record": lambda: _table_family("giant_record", cases.giant_record_cases),
    "deep_nesting": lambda: _table_family("deep_nesting", cases.deep_nesting_cases),
    "random": _random_family, "n4": _n4_family, "named_refs": _named_refs_family,
}


@functools.lru_cache(maxsize=None)
def raw_family(family: str) -> Tuple[Case, ...]:
    out = tuple(_GENERATORS[family]())
    assert len({c.id for c in out}) == len(out) and all(c.family == family for c in out)
    return out


def raw_corpus() -> Tuple[Case, ...]:
    return tuple(c for family in FAMILIES for c in raw_family(family))


def _subset(records: Sequence[bytes]) -> Tuple[bytes, ...]:
    head = list(records[:SUBSET_HEAD])
    largest = max(range(len(records)), key=lambda i: len(records[i]))
    return tuple(head + ([records[largest]] if largest >= SUBSET_HEAD else []))


@functools.lru_cache(maxsize=None)
def repaired_family(family: str) -> Tuple[Case, ...]:
    """Every record of every case of the family, the tails of REPAIRS taken off."""
    out = []
    for c in raw_family(family):
        recs = list(c.records)
        for (cid, i), tail in REPAIRS.items():
            if cid == c.id:
                assert recs[i].endswith(tail), (cid, i)
                recs[i] = recs[i][:-len(tail)]
        out.append(c._replace(records=tuple(recs)))
    return tuple(out)


def repaired_corpus() -> Tuple[Case, ...]:
    return tuple(c for family in FAMILIES for c in repaired_family(family))


@functools.lru_cache(maxsize=None)
def _family(family: str) -> Dict[str, Case]:
    return {c.id: c._replace(records=_subset(c.records)) if c.id in SUBSET_CASES else c for c in repaired_family(family)}


def corpus() -> Tuple[Case, ...]:
    return tuple(c for family in FAMILIES for c in _family(family).values())


def case(cid: str) -> Case:
    return _family(cid.split("/")[0])[cid]


def clear() -> None:
    """Drop every record, file and expected batch this module holds."""
    for f in (raw_family, repaired_family, _family, file_of, expected, min_schemas, _compiled):
        f.cache_clear()


FAMILIES = ("wire", "nesting", "differential", "dense_list", "enum_form", "wide_counter", "wide_form", "giant_record", "deep_nesting",
            "random", "n4", "named_refs")

# The ids of corpus(), written out so that collecting the tests generates no record (test_the_subset_rule_and_the_size_caps
# asserts that this is corpus()'s list).
CASE_NAMES = {
    "wire": ("array_blocks", "array_block_count_i64_min", "map_blocks", "null_orders", "extremes", "strings", "noncanonical_varints"),
    "nesting": ("union_of_containers", "nested_lists", "nullable_containers", "deep_nullfill"),
    "differential": ("flat_primitives", "nullable_primitives", "enum", "nested_record", "nullable_nested_record", "multi_variant_union",
                     "array_of_string", "empty_array", "map_of_string", "test_enum"),
    "dense_list": ("dense_long_lists", "dense_skewed", "dense_multiblock_positive", "dense_two_byte_counts", "dense_record_items",
                   "dense_nullable_and_n4"),
    "enum_form": ("enum_forms",),
    "wide_counter": ("wide_70_counters", "wide_96_counters"),
    "wide_form": ("wide_forms", "padded_at_form_widths"),
    "giant_record": ("giant_arrays", "giant_nested"),
    "deep_nesting": ("lists_12_deep", "nullable_records_36_deep", "unions_10_deep"),
    "random": tuple(f"seed_{seed:02d}" for seed in range(random_cases.PREBUILT_SEEDS)),
    "n4": ("n4", "duration"),
    "named_refs": ("with_refs",),
}
CASE_IDS = tuple(f"{family}/{name}" for family in FAMILIES for name in CASE_NAMES[family])


# ---- layouts ---------------------------------------------------------------------------------------------------------------------
def _deal(records: Sequence[bytes], counts) -> List[List[bytes]]:
    """The records dealt to blocks of `counts` records (an iterator; when it ends the last block takes the rest); a block is
    closed early instead of passing BLOCK_CAP."""
    out, at, n = [], 0, len(records)
    counts = iter(counts)
    while at < n:
        want = next(counts, n - at)
        blk, size = [], 0
        while len(blk) < want and at < n and (not blk or size + len(records[at]) <= BLOCK_CAP):
            blk.append(records[at])
            size += len(records[at])
            at += 1
        out.append(blk)
    return out


def layout_records(c: Case, layout: str) -> Tuple[bytes, ...]:
    recs = c.records
    if layout == "ones" and 0 < len(recs) < ONES_BLOCKS:
        reps = -(-ONES_BLOCKS // len(recs))
        if reps * sum(map(len, recs)) <= FILE_CAP:
            return tuple((recs * reps)[:ONES_BLOCKS])
    return recs


def blocks_of(c: Case, layout: str) -> List[List[bytes]]:
    recs = layout_records(c, layout)
    if layout == "ones":
        return [[r] for r in recs]
    if layout == "ragged":
        def cycle():
            while True:
                yield from RAGGED_COUNTS
        # (the cycle never ends, so _deal's "rest" is not used: the last block is simply cut short by the end of the records)
        return _deal(recs, cycle())
    if layout == "one_block":
        return _deal(recs, iter(()))
    raise KeyError(layout)


@functools.lru_cache(maxsize=8)
def file_of(cid: str, layout: str, codec: str = "null") -> bytes:
    """(The tests of one case follow each other, so a few files are kept; a file is cheap to write again.)"""
    c = case(cid)
    return CC.write(c.schema, blocks_of(c, layout), codec)


@functools.lru_cache(maxsize=None)
def expected(cid: str, layout: str, k: int):
    """The oracle's batches for the records of a layout's file: computed once, shared, never modified; clear() drops them."""
    c = case(cid)
    return oracle(layout_records(c, layout), c.schema, k)


# ---- the shortest valid datum ----------------------------------------------------------------------------------------------------
def min_datum(s: S.AvroSchema) -> bytes:
    """THE RULE: a union takes its null branch where it has one, otherwise the branch whose index + datum is shortest (the first
    of equals); string, bytes, array and map are empty (one zero byte); int, long, boolean and their logical types are the zero
    varint / byte; an enum is its first symbol; fixed, float and double are raw zeros; a record is its fields one behind the
    other.  The logical types on top: a decimal or uuid on a fixed is that fixed, a duration its 12 bytes; a decimal on bytes is
    empty bytes (the oracle reads them as zero); a uuid on a string is 32 hex digits, the shortest text that names one."""
    k = s.kind
    if k == "null":
        return b""
    if k == "record":
        return b"".join(min_datum(f.schema) for f in s.fields)
    if k == "union":
        for i, v in enumerate(s.variants):
            if v.kind == "null":
                return CC.zz(i)
        return min((CC.zz(i) + min_datum(v) for i, v in enumerate(s.variants)), key=len)
    if k == "float":
        return bytes(4)
    if k == "double":
        return bytes(8)
    if k == "fixed":
        return bytes(s.size)
    if k == "duration":
        return bytes(12)
    if k == "decimal":
        return bytes(s.items.size) if s.items.kind == "fixed" else b"\x00"
    if k == "uuid":
        return bytes(16) if s.items.kind == "fixed" else CC.zz(32) + b"0" * 32
    return b"\x00"


def min_record(schema: str) -> bytes:
    return min_datum(S.parse_schema(schema, resolve_refs=True))


@functools.lru_cache(maxsize=None)
def min_schemas() -> Tuple[Tuple[str, str], ...]:
    """(name, schema) of every distinct schema text of the corpus, named after the first case that uses it."""
    seen, out = set(), []
    for c in corpus():
        if c.schema not in seen:
            seen.add(c.schema)
            out.append((c.id, c.schema))
    return tuple(out)
