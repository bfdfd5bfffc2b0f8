"""The container tests' OWN Avro object container writer and reader (Avro 1.11 "Object Container Files"), and the inputs of
tests/test_container.py.  Plain Python, nothing here touches the code under test or a GPU: expected values are the oracle's
decode of the records this writer put into the file.

  write(schema, blocks, ...)      a container from lists of records, one list per block
  read(blob)                      -> Parsed(schema, codec, sync, metadata, blocks=[(count, payload)])
  records_of(name, n)             n records of a schema of avrogen.schemas.SCHEMAS
  split(records, counts)          the records dealt to blocks of those sizes
  LAYOUTS                         name -> block sizes
"""
from __future__ import annotations

import functools
import json
import zlib
from collections import namedtuple
from typing import Dict, List, Optional, Sequence

from avrogen import synth
from avrogen.encoder import to_datum
from avrogen.schemas import SCHEMAS
from oracle import c_walker
from oracle.avro_schema import parse_schema

MAGIC = b"Obj\x01"
SYNC = bytes(range(0xA0, 0xB0))


def zz(n: int) -> bytes:
    """zigzag varint of a long"""
    z = (n << 1) ^ (n >> 63)
    out = bytearray()
    while z >= 0x80:
        out.append((z & 0x7F) | 0x80)
        z >>= 7
    out.append(z)
    return bytes(out)


def _entry(k: str, v: bytes) -> bytes:
    kb = k.encode()
    return zz(len(kb)) + kb + zz(len(v)) + v


def header(schema: Optional[str], codec: Optional[str] = None, metadata: Optional[Dict[str, bytes]] = None, sync: bytes = SYNC,
           map_blocks: int = 1, negative_counts: bool = False, magic: bytes = MAGIC) -> bytes:
    """The file header.  `map_blocks`: the metadata map written in that many map blocks; `negative_counts`: every map block in
    its (-count, byte size) form.  codec None = no avro.codec entry; schema None = no avro.schema entry."""
    entries = []
    if schema is not None:
        entries.append(_entry("avro.schema", schema.encode()))
    if codec is not None:
        entries.append(_entry("avro.codec", codec.encode()))
    entries += [_entry(k, v) for k, v in (metadata or {}).items()]
    out = bytearray(magic)
    per = max(1, -(-len(entries) // max(map_blocks, 1)))
    for i in range(0, len(entries), per):
        body = b"".join(entries[i:i + per])
        cnt = len(entries[i:i + per])
        out += (zz(-cnt) + zz(len(body))) if negative_counts else zz(cnt)
        out += body
    out += zz(0) + sync
    return bytes(out)


def block(records: Sequence[bytes], codec: str = "null", sync: bytes = SYNC, count: Optional[int] = None) -> bytes:
    """One block.  `count`: what the block header claims (default: the truth)."""
    payload = b"".join(records)
    if codec == "deflate":
        c = zlib.compressobj(wbits=-15)
        payload = c.compress(payload) + c.flush()
    return zz(len(records) if count is None else count) + zz(len(payload)) + payload + sync


def write(schema: str, blocks: Sequence[Sequence[bytes]], codec: str = "null", metadata=None, sync: bytes = SYNC, **hdr) -> bytes:
    return header(schema, codec, metadata, sync, **hdr) + b"".join(block(b, codec, sync) for b in blocks)


Parsed = namedtuple("Parsed", ["schema", "codec", "sync", "metadata", "blocks"])


class _R:
    def __init__(self, b):
        self.b, self.at = b, 0

    def long(self) -> int:
        r = shift = 0
        while True:
            x = self.b[self.at]
            self.at += 1
            r |= (x & 0x7F) << shift
            if not x & 0x80:
                return (r >> 1) ^ -(r & 1)
            shift += 7

    def take(self, n: int) -> bytes:
        assert 0 <= n <= len(self.b) - self.at
        out = bytes(self.b[self.at:self.at + n])
        self.at += n
        return out


def read(blob: bytes) -> Parsed:
    """-> the header's fields and [(record count, uncompressed payload)] per block"""
    r = _R(blob)
    assert r.take(4) == MAGIC
    meta = {}
    while True:
        cnt = r.long()
        if cnt == 0:
            break
        if cnt < 0:
            cnt = -cnt
            r.long()
        for _ in range(cnt):
            k = r.take(r.long()).decode()
            meta[k] = r.take(r.long())
    sync = r.take(16)
    schema = meta.pop("avro.schema").decode()
    codec = meta.pop("avro.codec", b"null").decode()
    blocks = []
    while r.at < len(blob):
        cnt = r.long()
        payload = r.take(r.long())
        assert r.take(16) == sync
        blocks.append((cnt, zlib.decompress(payload, -15) if codec == "deflate" else payload))
    return Parsed(schema, codec, sync, meta, blocks)


# ---- inputs --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def records_of(name: str, n: int) -> tuple:
    if name == "t_union":
        s = parse_schema(SCHEMAS[name])
        return tuple(to_datum(s, {"u": [None, f"s-{i}" * (i % 5), i * 11 - 70, i % 8 == 3][i % 4]}) for i in range(n))
    return tuple(synth.records(name, n))


@functools.lru_cache(maxsize=None)
def expected(name: str, n: int, k: int):
    """The oracle's batches for records_of(name, n): computed once, shared, never modified."""
    return c_walker.decode_threaded(list(records_of(name, n)), SCHEMAS[name], k)


def split(records: Sequence[bytes], counts: Sequence[int]) -> List[List[bytes]]:
    assert sum(counts) == len(records)
    out, at = [], 0
    for c in counts:
        out.append(list(records[at:at + c]))
        at += c
    return out


RAGGED = [0, 1, 300, 1, 0, 64, 2] + [(i * 7) % 5 for i in range(70)]       # 77 blocks: empty ones, one full lane among nearly idle ones
LAYOUTS: Dict[str, List[int]] = {
    "one_block": [500],
    "ones_63": [1] * 63, "ones_64": [1] * 64, "ones_65": [1] * 65, "ones_257": [1] * 257,      # wavefront and workgroup edges
    "ragged": RAGGED,
    "no_blocks": [],
    "one_empty_block": [0],
}

# ---- damage to `full` records whose verdict does not depend on where the record ends -----------------------------------------
FULL_PARSED = parse_schema(SCHEMAS["full"])
_full_fields = json.loads(SCHEMAS["full"])["fields"]
_status_at = [f["name"] for f in _full_fields].index("status")
FULL_HEAD_PARSED = parse_schema(json.dumps({"type": "record", "name": "User", "fields": _full_fields[:_status_at]}))      # the fields in front of `status`


def damaged_full(kind: str, row: int) -> bytes:
    """Record `row` of the `full` generator (a row with preferences) damaged: "bool" -- preferences.newsletter = 2; "union" --
    the branch of `status` = 7; "enum" -- the index of `class` = 5."""
    v = synth.gen_full(20260921, row)
    while v["preferences"] is None:
        row += 1
        v = synth.gen_full(20260921, row)
    rec = bytearray(to_datum(FULL_PARSED, v))
    at = len(to_datum(FULL_HEAD_PARSED, v))      # the branch byte of `status`
    if kind == "bool":
        rec[at - 1] = 2
    elif kind == "union":
        rec[at] = zz(7)[0]
    elif kind == "enum":
        rec[-1] = zz(5)[0]
    else:
        raise KeyError(kind)
    return bytes(rec)


DAMAGE_MESSAGES = {"bool": "invalid boolean byte: 2", "union": "union branch index out of range: 7", "enum": "enum index 5 out of range"}
