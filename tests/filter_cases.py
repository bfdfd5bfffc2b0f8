"""Shared inputs of the row-filter tests (tests/test_filter.py, tests/test_filter_gpu.py): the schema that holds every
filterable kind, its edge values, and the plain Python statement of what a predicate keeps -- evaluated on the values the
ORACLE decodes, never on anything the engine returns."""
from __future__ import annotations

import functools
import json
import struct

import numpy as np
import pyarrow as pa

from oracle import c_walker
from oracle.avro_schema import SchemaError, parse_schema
from avrogen.encoder import to_datum

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
ENUM_SYMBOLS = ["clubs", "hearts", "spades", "a_much_longer_symbol"]


def _f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


# edge values by kind (the CPU check's: tools/filter_check.cpp)
INTS = [I32_MIN, I32_MAX, 0, -1, 1, 63, 64, -65, 127, 128, (1 << 24) + 1, -(1 << 28) - 1, 123456789]               # 1 .. 5 byte varints
LONGS = [I64_MIN, I64_MAX, 0, -1, 1, (1 << 53) + 1, -((1 << 53) + 1), 1 << 34, (1 << 62), -(1 << 48) - 3, I32_MIN, I32_MAX + 1, 5]      # up to 10 bytes
FLOATS = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), _f32(3.4028234663852886e38), _f32(1.1754943508222875e-38), _f32(1e-45),
          1.5, -2.75, _f32(0.1), 16777216.0, -1.0]
DOUBLES = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1.7976931348623157e308, 2.2250738585072014e-308, 5e-324, 1.5, -2.75, 0.1,
           9007199254740993.0, -1.0]
STRINGS = ["", "a", "ab", "abc", "abd", "b", "é", "ÿÿ", "a\u0000", "x" * 254, "x" * 255, "x" * 256, "x" * 254 + "y", "\U0001F600", "ab" * 40]
BYTES = [b"", b"a", b"ab", b"abc", b"\x00", b"\x7f", b"\x80", b"\xff", b"a\x80", b"a\x00", b"x" * 255, b"x" * 300, b"\xff" * 255, b"\xc3\xa9"]
BOOLS = [True, False, False, True, True]

KIND_VALUES = {"int": INTS, "long": LONGS, "float": FLOATS, "double": DOUBLES, "boolean": BOOLS, "string": STRINGS, "bytes": BYTES,
               "enum": ENUM_SYMBOLS, "date": INTS, "ts": LONGS}
# comparands the tests try per kind (a few of the edge values, and values between them)
KIND_COMPARANDS = {"int": [I32_MIN, 0, 64, I32_MAX, I64_MAX], "long": [I64_MIN, -1, 1 << 34, I64_MAX], "float": [0.0, float("nan"), 1.5, float("inf"), 0.1, 2],
                   "double": [-0.0, float("nan"), 0.1, float("-inf"), -1], "boolean": [True, False], "string": ["", "ab", "abc", "x" * 255, "é", b"b"],
                   "bytes": [b"", b"a", b"\x80", b"x" * 255, b"\xff" * 255, "ab"], "enum": ["clubs", "a_much_longer_symbol"],
                   "date": [0, 127], "ts": [0, 1 << 34]}
ORDERED = ("==", "!=", "<", "<=", ">", ">=")
KIND_OPS = {k: (("==", "!=") if k in ("boolean", "enum") else ORDERED) for k in KIND_VALUES}


def _type_of(kind, form):
    return {"enum": {"type": "enum", "name": "Suit_" + form, "symbols": ENUM_SYMBOLS}, "date": {"type": "int", "logicalType": "date"},
            "ts": {"type": "long", "logicalType": "timestamp-micros"}}.get(kind, kind)


def _kinds_schema():
    fields = []
    for kind in KIND_VALUES:
        for form in ("plain", "null_first", "null_last"):
            tt = _type_of(kind, form)
            typ = tt if form == "plain" else ["null", tt] if form == "null_first" else [tt, "null"]
            fields.append({"name": f"{kind}_{form}", "type": typ})
    fields.append({"name": "arr", "type": {"type": "array", "items": "string"}})
    fields.append({"name": "tail", "type": "long"})
    return json.dumps({"type": "record", "name": "Kinds", "fields": fields})


KINDS_SCHEMA = _kinds_schema()
KINDS_FIELDS = [(f"{kind}_{form}", kind, form) for kind in KIND_VALUES for form in ("plain", "null_first", "null_last")]


def kinds_values(n):
    out = []
    for i in range(n):
        v = {}
        for j, kind in enumerate(KIND_VALUES):
            vals = KIND_VALUES[kind]
            x = vals[(i + j) % len(vals)]
            v[f"{kind}_plain"] = x
            v[f"{kind}_null_first"] = None if (i + j) % 3 == 0 else vals[(i * 5 + j) % len(vals)]
            v[f"{kind}_null_last"] = None if (i + 2 * j) % 4 == 1 else vals[(i * 3 + j) % len(vals)]
        v["arr"] = ["t%d" % i] * (i % 3)
        v["tail"] = i
        out.append(v)
    return out


@functools.lru_cache(maxsize=None)
def kinds_records(n):
    s = parse_schema(KINDS_SCHEMA)
    return tuple(to_datum(s, v) for v in kinds_values(n))


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def oracle_decode(recs, schema, k):
    """The oracle's decode: the C walker, or -- schemas with `bytes`, which the reference's gate rejects -- the Python walker in
    its extended form, chunked by the reference's rule (deserialize.rs:53-58)."""
    from oracle import py_walker
    recs = list(recs)
    try:
        return c_walker.decode_threaded(recs, schema, k)
    except SchemaError:
        n = len(recs)
        k = min(max(k, 1), max(n, 1))
        sz = n // k
        return [py_walker.decode(recs[c * sz: (c + 1) * sz if c + 1 < k else n], schema, extended=True) for c in range(k)]


def _as_bytes(x):
    return x.encode("utf-8") if isinstance(x, str) else bytes(x)


def value_keeps(v, op, k):
    """What one term keeps, on the decoded value `v` (None = null)."""
    if op == "is_null":
        return v is None
    if op == "not_null":
        return v is not None
    if v is None:
        return False
    if isinstance(v, (str, bytes)):
        v, k = _as_bytes(v), _as_bytes(k)      # unsigned bytewise order (Python's order of bytes); an enum's symbol text: == / != only
    elif isinstance(v, float):
        k = float(k)
    return {"==": v == k, "!=": v != k, "<": v < k, "<=": v <= k, ">": v > k, ">=": v >= k}[op]


def terms_of(where):
    terms = [where] if isinstance(where[0], str) else list(where)
    return [(t[0], t[1], t[2] if len(t) == 3 else None) for t in terms]


def oracle_mask(recs, schema, where) -> np.ndarray:
    """numpy bool[n]: keep_W on the values the oracle decodes under the writer schema."""
    n = len(recs)
    mask = np.ones(n, dtype=bool)
    if n == 0:
        return mask
    full = oracle_decode(recs, schema, 1)[0]
    for name, op, k in terms_of(where):
        arr = full.column(name)
        if pa.types.is_temporal(arr.type):       # date / time-* / timestamp-*: the raw int the wire carries
            arr = arr.cast(pa.int32() if arr.type.bit_width == 32 else pa.int64())
        col = arr.to_pylist()
        mask &= np.array([value_keeps(v, op, k) for v in col], dtype=bool)
    return mask


def oracle_filtered(recs, schema, where, k, mask=None):
    """The contract's right-hand side: the oracle's decode of the kept records, in k chunks."""
    if mask is None:
        mask = oracle_mask(recs, schema, where)
    return oracle_decode([r for r, m in zip(recs, mask) if m], schema, k)
