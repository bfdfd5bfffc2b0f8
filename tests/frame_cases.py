"""Shared inputs of the framed-message tests (tests/test_frame.py, tests/test_frame_gpu.py): how a message is framed, the plain
Python statement of the split (``int.from_bytes`` on the header), the class patterns of tools/frame_check.cpp, and the contract's
right-hand side -- the ORACLE's decode of the stripped payloads of every group, never anything the engine returns."""
from __future__ import annotations

import functools
import json

import numpy as np

from oracle import c_walker
from oracle.avro_schema import parse_schema
from avrogen.encoder import to_datum

HEADER = {"confluent": 5, "single_object": 10}
FRAMINGS = ("confluent", "single_object")


def frame(framing: str, wire_id: int, payload: bytes) -> bytes:
    if framing == "confluent":
        return b"\x00" + int(wire_id).to_bytes(4, "big") + payload
    return b"\xc3\x01" + int(wire_id).to_bytes(8, "little") + payload


def verdict(msg: bytes, framing: str):
    """("short", len) | ("marker",) | ("id", wire id) -- the three framing checks in the order the call judges them."""
    h = HEADER[framing]
    if len(msg) < h:
        return ("short", len(msg))
    if framing == "confluent":
        if msg[0] != 0:
            return ("marker",)
        return ("id", int.from_bytes(msg[1:5], "big"))
    if msg[0] != 0xC3 or msg[1] != 0x01:
        return ("marker",)
    return ("id", int.from_bytes(msg[2:10], "little"))


def framing_error(messages, ids, framing, unknown="raise"):
    """The message the call must raise for this list, or None: the lowest index that fails any of the three checks decides."""
    h = HEADER[framing]
    known = set(ids)
    for i, m in enumerate(messages):
        v = verdict(m, framing)
        if v[0] == "short":
            return f"framed: message {i} is {v[1]} bytes, shorter than the {h}-byte {framing} header"
        if v[0] == "marker":
            return f"framed: message {i} does not start with the {framing} marker"
        if v[1] not in known and unknown == "raise":
            return f"framed: message {i} carries schema id {v[1]}, which is not in schemas"
    return None


def classify(messages, ids, framing) -> np.ndarray:
    """numpy int16[n]: the position of every message's id in sorted(ids), -1 for an id that is not among them."""
    pos = {w: p for p, w in enumerate(sorted(ids))}
    out = np.empty(len(messages), dtype=np.int16)
    for i, m in enumerate(messages):
        v = verdict(m, framing)
        assert v[0] == "id", (i, v)
        out[i] = pos.get(v[1], -1)
    return out


def expected_groups(messages, schemas, framing, k, decode=None):
    """[(wire id, schema text, indices int64[], oracle batches)] ascending by id, and the unknown (indices, ids).  `decode`:
    (payload list, schema text, k) -> batches; the C walker by default."""
    h = HEADER[framing]
    decode = decode or (lambda recs, schema, kk: c_walker.decode_threaded(recs, schema, kk))
    by = {w: [] for w in schemas}
    unk_i, unk_id = [], []
    for i, m in enumerate(messages):
        v = verdict(m, framing)
        assert v[0] == "id", (i, v)
        if v[1] in by:
            by[v[1]].append(i)
        else:
            unk_i.append(i)
            unk_id.append(v[1])
    groups = []
    for w in sorted(schemas):
        idx = by[w]
        groups.append((w, schemas[w], np.array(idx, dtype=np.int64), decode([bytes(messages[i][h:]) for i in idx], schemas[w], k)))
    return groups, (np.array(unk_i, dtype=np.int64), np.array(unk_id, dtype=np.uint64))


# ---- ids: the edges of tools/frame_check.cpp ------------------------------------------------------------------------------------------
CONFLUENT_EDGES = [0, 1, 0x01000000, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
SINGLE_EDGES = [0x1122334455667700, 0x1122334455667701, 0x9122334455667700, 0, 0x8000000000000000, (1 << 64) - 1]


def id_list(framing: str, m: int):
    edges = CONFLUENT_EDGES if framing == "confluent" else SINGLE_EDGES
    ids = list(edges[:m])
    x = 1000 if framing == "confluent" else 0x0100000000000000
    while len(ids) < m:
        ids.append(x)
        x += 7 if framing == "confluent" else 0x0100000000000007
    return ids


def unknown_id(framing: str, salt: int) -> int:
    return 0x100 + (salt % 3) * 0x10000 if framing == "confluent" else 0x1122334455667702 + (salt % 3) * 0x0100000000000000


# ---- two small schemas, dealt to the ids in turn ---------------------------------------------------------------------------------------
SCHEMA_A = json.dumps({"type": "record", "name": "FrA", "fields": [{"name": "s", "type": "string"}]})
SCHEMA_B = json.dumps({"type": "record", "name": "FrB", "fields": [{"name": "l", "type": "long"}, {"name": "s", "type": ["null", "string"]}]})


def schemas_for(ids):
    """{wire id: schema text}: the ids in ascending order take SCHEMA_A and SCHEMA_B in turn."""
    return {w: (SCHEMA_A, SCHEMA_B)[p % 2] for p, w in enumerate(sorted(ids))}


@functools.lru_cache(maxsize=None)
def _datums(n):
    a, b = parse_schema(SCHEMA_A), parse_schema(SCHEMA_B)
    # payloads of 1 .. 40 bytes and a few over 64
    text = ["x" * (64 + i % 90) if i % 37 == 9 else "y" * ((i * 7) % 40) for i in range(n)]
    return (tuple(to_datum(a, {"s": t}) for t in text),
            tuple(to_datum(b, {"l": i * 1_000_003 - 5, "s": None if i % 3 == 0 else t}) for i, t in enumerate(text)))


# what message i is: a position in sorted(ids), or -1 = an unknown id
PATTERNS = {
    "all one class": lambda i, n, m: m - 1,
    "alternating classes": lambda i, n, m: i % m,
    "runs ending on wavefront edges": lambda i, n, m: (i // 64) % m,
    "runs ending on tile edges": lambda i, n, m: (i // 256) % m,
    "a class seen only in the last message": lambda i, n, m: m - 1 if i + 1 == n else 0,
    "a class never seen": lambda i, n, m: i % (m - 1) if m > 1 else 0,
    "unknown ids sprinkled in": lambda i, n, m: -1 if i % 7 == 3 else (i * 5) % m,
    "random": lambda i, n, m: ((i * 2654435761 + 12345) >> 7) % (m + 1) - 1,
}
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1024, 1100)
CLASS_COUNTS = (1, 2, 3, 32)


def pattern_messages(framing, n, m, pattern):
    """(messages, ids): n framed messages whose classes follow the pattern; a message of class p carries a datum of the schema
    schemas_for(ids) gives sorted(ids)[p]."""
    ids = id_list(framing, m)
    order = sorted(ids)
    da, db = _datums(max(n, 1))
    f = PATTERNS[pattern]
    out = []
    for i in range(n):
        p = f(i, n, m)
        if p < 0:
            out.append(frame(framing, unknown_id(framing, i), da[i]))
        else:
            out.append(frame(framing, order[p], (da, db)[p % 2][i]))
    return out, ids
