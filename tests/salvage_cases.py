"""Inputs of tests/test_container_tolerant.py: damaged Avro object container files put together piece by piece, with what a
tolerant read must keep and report known from HOW the file was built -- never from the code under test.  Plain Python over
tests/container_cases.py (imported, not edited); nothing here touches a GPU.

  Block(records, ...)        one framed block: the records written, the count claimed, how many of them are kept, the message
  Junk(raw, message)         bytes in which no block can be framed: one gap (the piece must end so that framing resumes behind it)
  assemble(schema, pieces)   -> File(blob, kept, errors): the file, the records a tolerant read keeps, the entries it reports
"""
from __future__ import annotations

import zlib
from collections import namedtuple
from typing import List, Optional, Sequence

import container_cases as CC

File = namedtuple("File", ["blob", "kept", "errors", "offsets"])


class Block:
    """A framed block.  `records`: what is written (a damaged record among them, perhaps); `count`: what the header claims
    (default: len(records)); `kept`: how many leading records a tolerant read keeps (default: all -- then the block is not
    reported unless `message` is given); `stream`: the compressed payload to write instead of the deflated records."""

    def __init__(self, records: Sequence[bytes], count: Optional[int] = None, kept: Optional[int] = None, message: Optional[str] = None,
                 stream: Optional[bytes] = None, lost: Optional[int] = None):
        self.records = list(records)
        self.count = len(self.records) if count is None else count
        self.kept = len(self.records) if kept is None else kept
        self.message = message
        self.stream = stream
        self.lost = self.count - self.kept if lost is None else lost
        self.reported = message is not None

    def bytes(self, codec: str) -> bytes:
        payload = b"".join(self.records)
        if self.stream is not None:
            payload = self.stream
        elif codec == "deflate":
            c = zlib.compressobj(wbits=-15)
            payload = c.compress(payload) + c.flush()
        return CC.zz(self.count) + CC.zz(len(payload)) + payload + CC.SYNC


class Junk:
    """A gap: `raw` bytes that frame no block.  `message`: what the strict scan says at its first byte, with `{b}` for the
    number of blocks framed in front of it."""

    def __init__(self, raw: bytes, message: str):
        self.raw, self.message = raw, message


def assemble(schema: str, pieces, codec: str = "null") -> File:
    """The file of `pieces`, and what a tolerant read gives for it: the kept records in file order, and the entries
    (block, offset, length, kept, lost, message) ascending by offset.  A message may hold `{b}`: the block's index."""
    out = bytearray(CC.header(schema, codec))
    kept: List[bytes] = []
    errors = []
    offsets = []
    b = 0
    for p in pieces:
        at = len(out)
        offsets.append(at)
        if isinstance(p, Junk):
            out += p.raw
            errors.append((None, at, len(p.raw), 0, None, p.message.format(b=b)))
            continue
        raw = p.bytes(codec)
        out += raw
        kept += p.records[:p.kept]
        if p.reported:
            errors.append((b, at, len(raw), p.kept, p.lost, p.message.format(b=b)))
        b += 1
    return File(bytes(out), kept, errors, offsets)


def broken_marker(block: Block, codec: str = "null") -> bytes:
    """The block's bytes with the last byte of its sync marker flipped: the raw of a Junk -- if a sound block follows, the gap
    swallows that one too (give Junk the bytes of both)."""
    raw = bytearray(block.bytes(codec))
    raw[-1] ^= 0x01
    return bytes(raw)
