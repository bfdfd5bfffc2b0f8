"""Random damage to well-formed records, and what the oracle says about every damaged record: the inputs of
tests/test_tolerant_fuzz.py.  Nothing here touches a GPU.

  damage(rec, rng)             one of six kinds of damage to one record
  dirty_list(recs, seed)       1024 records (four tiles) with damaged records in every shape of a bitmap word
  verdicts(...)                {index: the oracle's message} for the damaged records that are malformed now
  FUZZ_CASES                   name -> builder of (schema, 1024 clean records); fuzz_case(name) builds and caches
  dirty_case(name)             the dirty list of a case with its verdicts, built once and shared by every test

The oracle is oracle.c_walker; for the schemas it refuses (the N4 leaf types, named-type references) oracle.py_walker
in its extended form, which restates the Avro specification for them."""
from __future__ import annotations

import functools
import json
import random
from collections import namedtuple
from typing import Callable, Dict, List, Sequence, Tuple

import cases
import random_cases
import test_n4_types
import test_named_refs
from avrogen import synth
from avrogen.encoder import to_datum
from avrogen.schemas import SCHEMAS
from oracle import avro_schema as S
from oracle import c_walker, py_walker

N = 1024            # records of a fuzz case: four tiles of 256, sixteen bitmap words
DAMAGE_KINDS = 6


def damage(rec: bytes, rng: random.Random) -> bytes:
    """One of six, picked by rng: flip one bit; cut at a random byte; insert 1-4 random bytes at a random place; overwrite one
    byte with one of 80 FF 7F 01 00; overwrite a span of 10 bytes with 80 x 10 (a varint that is too long; a span that starts less
    than 10 bytes before the end makes the record longer); replace everything from a random position on with FF FF FF FF 0F (a
    huge length or count).  An empty record can only take the insertion."""
    b = bytearray(rec)
    how = rng.randrange(DAMAGE_KINDS) if b else 2
    if how == 0:
        b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
    elif how == 1:
        del b[rng.randrange(len(b)):]
    elif how == 2:
        pos = rng.randrange(len(b) + 1)
        b[pos:pos] = bytes(rng.randrange(256) for _ in range(rng.randint(1, 4)))
    elif how == 3:
        b[rng.randrange(len(b))] = rng.choice([0x80, 0xFF, 0x7F, 0x01, 0x00])
    elif how == 4:
        pos = rng.randrange(len(b))
        b[pos:pos + 10] = b"\x80" * 10
    else:
        del b[rng.randrange(len(b)):]
        b += b"\xFF\xFF\xFF\xFF\x0F"
    return bytes(b)


def dirty_list(recs: Sequence[bytes], seed: int) -> Tuple[List[bytes], List[int]]:
    """-> (recs with damage, the damaged indices ascending).  Records 0-63 all damaged (a whole wavefront: a bitmap word of
    ones), 64-127 untouched (a word of zeros), 255, 256 and 1023 damaged (the last bit of a word and of a tile, the first of
    the next, the last of the list), every other record with probability 1/4."""
    assert len(recs) == N
    rng = random.Random(seed)
    out = list(recs)
    hit = []
    for i in range(N):
        if i < 64 or i in (255, 256, N - 1):
            take = True
        elif i < 128:
            take = False
        else:
            take = rng.random() < 0.25
        if take:
            out[i] = damage(out[i], rng)
            hit.append(i)
    return out, hit


# ---------------------------------------------------------------------------------------------------------------------
# the two oracles: (records, schema, k) -> k batches, ValueError(message of the lowest malformed record)
def c_oracle(recs, schema, k):
    return c_walker.decode_threaded(recs, schema, k)


def chunk_bounds(n: int, k: int) -> List[Tuple[int, int]]:
    """deserialize.rs:53-68: k chunks of n // k rows, the last one takes the rest."""
    kk = max(1, min(k, n))
    sz = n // kk
    return [(i * sz, (i + 1) * sz if i + 1 < kk else n) for i in range(kk)]


def py_oracle(recs, schema, k):
    return [py_walker.decode(recs[lo:hi], schema, extended=True) for lo, hi in chunk_bounds(len(recs), k)]


def oracle_for(schema: str) -> Callable:
    return c_oracle if S.is_supported(S.parse_schema(schema)) else py_oracle


def message(rec: bytes, schema: str, oracle: Callable):
    """What the strict decode raises when `rec` is the lowest malformed record; None for a well-formed one."""
    try:
        oracle([rec], schema, 1)
        return None
    except ValueError as e:
        return str(e)


def verdicts(recs: Sequence[bytes], damaged_idx: Sequence[int], schema: str, oracle: Callable) -> Dict[int, str]:
    """{i: the oracle's message for recs[i] decoded alone} for the damaged records; the ones it still accepts are left out.
    (The undamaged records are not asked about one by one: the caller decodes the clean list once.)"""
    seen: Dict[bytes, object] = {}
    out = {}
    for i in damaged_idx:
        r = recs[i]
        if r not in seen:
            seen[r] = message(r, schema, oracle)
        if seen[r] is not None:
            out[i] = seen[r]
    return out


# ---------------------------------------------------------------------------------------------------------------------
def _cycled(recs):
    return [recs[i % len(recs)] for i in range(N)]


def _differential(schema_name):
    def build():
        (c,) = [c for c in cases.differential_cases() if c[1] == SCHEMAS[schema_name]]
        return c[1], _cycled(c[2])
    return build


def _named_refs():
    tree = S.parse_schema(test_named_refs.WITH_REFS, resolve_refs=True)
    return test_named_refs.WITH_REFS, [to_datum(tree, r) for r in test_named_refs._rows(N)]


# A union WITHOUT a null branch: every branch has a payload, so the placeholder is branch 0 plus that branch's own placeholder
# (a record of an int and a string: 00 00 00) and is longer than one byte.  No table of cases.py has such a union.  (Listed in
# scripts/known_schemas.py, so that its specialised kernels are built ahead.)
UNION_NO_NULL_SCHEMA = json.dumps({"type": "record", "name": "UN", "fields": [
    {"name": "u", "type": [{"type": "record", "name": "UR", "fields": [{"name": "a", "type": "int"}, {"name": "b", "type": "string"}]},
                           {"type": "array", "items": "long"}, "string"]},
    {"name": "tail", "type": "long"}]})


def _union_no_null():
    vals = []
    for i in range(N):
        u = [{"a": i * 37 - 900, "b": f"b-{i}" * (i % 4)}, [j * j - i for j in range(i % 5)], f"s{i}" * (i % 7)][i % 3]
        vals.append({"u": u, "tail": i * 1001 - 500})
    return UNION_NO_NULL_SCHEMA, cases._enc(UNION_NO_NULL_SCHEMA, vals)


def _from(table, name):
    def build():
        (c,) = [c for c in table() if c[0] == name]
        return c[1], _cycled(c[2])
    return build


FUZZ_CASES: Dict[str, Callable[[], Tuple[str, List[bytes]]]] = {
    "full": lambda: (SCHEMAS["full"], synth.records("full", N)),
    "array_and_map": lambda: (SCHEMAS["array_and_map"], synth.records("array_and_map", N)),
    "nested_struct": lambda: (SCHEMAS["nested_struct"], synth.records("nested_struct", N)),
    "wide97": lambda: (SCHEMAS["wide97"], synth.records("wide97", N)),
    "t_union": _differential("t_union"),
    "t_enum": _differential("t_enum"),
    "t_map_str": _differential("t_map_str"),
    "t_nullable_nested": _differential("t_nullable_nested"),
    "random3": lambda: random_cases.random_case(3, N),
    "random11": lambda: random_cases.random_case(11, N),
    "random20": lambda: random_cases.random_case(20, N),
    "n4": lambda: (test_n4_types.SCHEMA, test_n4_types._records(N)),                 # fixed, decimal, uuid: E_DECIMAL, E_UUID, E_EOB_FIXED
    "duration": lambda: (test_n4_types.DUR_SCHEMA, test_n4_types._dur_records(N)),   # E_DURATION
    "named_refs": _named_refs,
    "union_of_containers": _from(cases.nesting_cases, "union_of_containers"),      # record / array as variants of an N-variant union
    "union_no_null": _union_no_null,                                                # the placeholder is branch 0 plus a payload
    "lists_12_deep": _from(cases.deep_nesting_cases, "lists_12_deep"),               # rem[12][256]: 12 KiB of LDS in front of the window
}
assert all(s < random_cases.PREBUILT_SEEDS for s in (3, 11, 20))

# The seed of each case's damage.  7 wherever it puts the case inside the band that test_the_inputs_are_not_trivial asserts
# (25-90 % of the damaged records malformed); another one where it does not.
SEEDS: Dict[str, int] = {name: 7 for name in FUZZ_CASES}

# Cases of which the test asks two distinct messages and not three, because their oracle has only two to give.
TWO_MESSAGE_CASES: Dict[str, str] = {}


@functools.lru_cache(maxsize=None)
def fuzz_case(name: str):
    schema, recs = FUZZ_CASES[name]()
    assert len(recs) == N
    return schema, recs


Dirty = namedtuple("Dirty", ["name", "seed", "schema", "oracle", "clean", "recs", "damaged", "verdicts"])


@functools.lru_cache(maxsize=None)
def dirty_case(name: str) -> Dirty:
    schema, clean = fuzz_case(name)
    recs, hit = dirty_list(clean, SEEDS[name])
    oracle = oracle_for(schema)
    return Dirty(name, SEEDS[name], schema, oracle, clean, recs, hit, verdicts(recs, hit, schema, oracle))


def patched(recs: Sequence[bytes], bad, placeholder: bytes) -> List[bytes]:
    bad = set(bad)
    return [placeholder if i in bad else r for i, r in enumerate(recs)]


def explain(d_name, seed, recs, want, got) -> str:
    """The first difference between two [(index, message)] lists, for an assertion message."""
    want, got = [tuple(e) for e in want], [tuple(e) for e in got]
    w, g = dict(want), dict(got)
    for i in sorted(set(w) | set(g)):
        if w.get(i) != g.get(i):
            return (f"case {d_name}, seed {seed}, record {i} = {bytes(recs[i]).hex()}: expected {w.get(i)!r}, got {g.get(i)!r} "
                    f"({len(want)} malformed records expected, {len(got)} listed)")
    return f"case {d_name}, seed {seed}: the same records and messages in another order: {got[:8]} ..."


# ---------------------------------------------------------------------------------------------------------------------
# test_gather_with_a_long_placeholder: fixed(100) + fixed(37) + the empty string = a placeholder of 138 bytes, more than two trips
# of rh_k_patch_gather's 64-lane loop.  (Listed in scripts/known_schemas.py, so that its specialised kernels are built ahead.)
LONG_PLACEHOLDER_SCHEMA = json.dumps({"type": "record", "name": "LP", "fields": [
    {"name": "a", "type": {"type": "fixed", "name": "A100", "size": 100}},
    {"name": "b", "type": {"type": "fixed", "name": "B37", "size": 37}},
    {"name": "s", "type": "string"}]})
