"""Inputs of tests/test_container_inflate.py: raw-deflate streams (RFC 1951) assembled by hand with a small bit writer, zlib's
own streams, and damaged ones.  Plain Python, nothing here touches the code under test or a GPU: the expected bytes and verdicts
of every stream are those of Python's ``zlib`` (``classify``).

  BitW, Coder                     a bit writer, and the symbols of one deflate block in a given pair of codes
  HAND                            name -> hand-assembled stream, at the edges of the format
  zlib_made()                     [(label, stream, payload)] at several levels and strategies
  classify(stream)                -> (class, bytes or None, trailing): zlib's verdict
  damage_cases()                  every single-bit flip and every prefix of one dynamic-Huffman stream, prefixes of refused flips
"""
from __future__ import annotations

import functools
import random
import zlib
from typing import Dict, List, Sequence, Tuple

OK, MALFORMED, TRUNCATED, TRAILING, TOO_LARGE = 0, 1, 2, 3, 4      # rh_inflate_status.code

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class BitW:
    def __init__(self):
        self.out = bytearray()
        self.acc = self.n = 0

    def put(self, v: int, bits: int) -> None:
        """`bits` bits of v, least significant first"""
        for i in range(bits):
            self.acc |= ((v >> i) & 1) << self.n
            self.n += 1
            if self.n == 8:
                self.out.append(self.acc)
                self.acc = self.n = 0

    def huff(self, code: int, bits: int) -> None:
        """a Huffman code: most significant bit first"""
        for i in reversed(range(bits)):
            self.put((code >> i) & 1, 1)

    def align(self) -> None:
        if self.n:
            self.put(0, 8 - self.n)

    def done(self) -> bytes:
        self.align()
        return bytes(self.out)


def canonical(lens: Sequence[int]) -> List[int]:
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    codes = [0] * len(lens)
    for i, l in enumerate(lens):
        if l:
            codes[i] = nxt[l]
            nxt[l] += 1
    return codes


def lens_of(n: int, symlens: Dict[int, int]) -> List[int]:
    out = [0] * n
    for s, l in symlens.items():
        out[s] = l
    return out


class Coder:
    """The symbols of one block in a pair of codes: fixed(), or set() + header()."""

    def __init__(self, w: BitW):
        self.w = w

    def set(self, ll: Sequence[int], dl: Sequence[int]) -> "Coder":
        self.ll, self.dl, self.lc, self.dc = list(ll), list(dl), canonical(ll), canonical(dl)
        return self

    def fixed(self, final: bool = True) -> "Coder":
        self.w.put(1 if final else 0, 1)
        self.w.put(1, 2)
        return self.set([8 if i < 144 else 9 if i < 256 else 7 if i < 280 else 8 for i in range(288)], [5] * 32)

    def sym(self, s: int) -> None:
        self.w.huff(self.lc[s], self.ll[s])

    def lit(self, b: bytes) -> None:
        for x in b:
            self.sym(x)

    def dist(self, d: int) -> None:
        c = max(i for i in range(30) if DIST_BASE[i] <= d)
        self.w.huff(self.dc[c], self.dl[c])
        self.w.put(d - DIST_BASE[c], DIST_EXTRA[c])

    def match(self, length: int, d: int, sym: int = None) -> None:
        c = sym - 257 if sym is not None else max(i for i in range(29) if LEN_BASE[i] <= length)
        self.sym(257 + c)
        self.w.put(length - LEN_BASE[c], LEN_EXTRA[c])
        self.dist(d)

    def header(self, final: bool = True) -> bool:
        """The dynamic header of the codes of set(): the lengths of both codes run-length coded as ONE sequence, so a repeat may
        run from the literal/length lengths into the distance lengths.  -> whether one did."""
        w = self.w
        cl = [4] * 13 + [5] * 6      # a complete code for the 19 code-length symbols
        cc = canonical(cl)
        w.put(1 if final else 0, 1)
        w.put(2, 2)
        w.put(len(self.ll) - 257, 5)
        w.put(len(self.dl) - 1, 5)
        w.put(15, 4)
        for i in range(19):
            w.put(cl[CLEN_ORDER[i]], 3)
        seq = self.ll + self.dl
        crossed, i, nl = False, 0, len(self.ll)
        while i < len(seq):
            run = 1
            while i + run < len(seq) and seq[i + run] == seq[i]:
                run += 1
            if seq[i] == 0 and run >= 3:
                r = min(run, 138)
                if r >= 11:
                    w.huff(cc[18], cl[18])
                    w.put(r - 11, 7)
                else:
                    w.huff(cc[17], cl[17])
                    w.put(r - 3, 3)
                crossed |= i < nl < i + r
                i += r
            elif seq[i] != 0 and run >= 4:
                w.huff(cc[seq[i]], cl[seq[i]])
                r = min(run - 1, 6)
                w.huff(cc[16], cl[16])
                w.put(r - 3, 2)
                crossed |= i < nl <= i + r
                i += 1 + r
            else:
                w.huff(cc[seq[i]], cl[seq[i]])
                i += 1
        return crossed


def stored(data: bytes, final: bool = True) -> bytes:
    w = BitW()
    w.put(1 if final else 0, 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put(len(data) ^ 0xFFFF, 16)
    return bytes(w.out) + data


def noise(n: int, seed: int = 20260921) -> bytes:
    return random.Random(seed).randbytes(n)


def _hand() -> Dict[str, bytes]:
    h = {}
    h["stored_0"] = stored(b"")
    w = BitW(); c = Coder(w).fixed(); c.sym(256)
    h["fixed_eob_only"] = w.done()
    h["stored_65535"] = stored(noise(65535, 1))
    w = BitW(); c = Coder(w).fixed(); c.match(258, 32768); c.sym(256)
    h["stored_32768_then_258_at_32768"] = stored(noise(32768, 2), final=False) + w.done()
    for d in (1, 2, 3):
        w = BitW(); c = Coder(w).fixed(); c.lit(b"xyz"); c.match(258, d); c.lit(b"!"); c.match(258, d); c.sym(256)
        h[f"258_at_distance_{d}"] = w.done()
    for s in (285, 284):
        w = BitW(); c = Coder(w).fixed(); c.lit(b"ab"); c.match(258, 2, sym=s); c.sym(256)
        h[f"258_as_symbol_{s}"] = w.done()
    w = BitW(); c = Coder(w).set(lens_of(261, {97: 2, 98: 2, 256: 2, 260: 2}), lens_of(4, {3: 1}))
    c.header(); c.lit(b"abab"); c.match(6, 4); c.sym(256)
    h["dynamic_one_distance_code_of_length_1"] = w.done()
    w = BitW(); c = Coder(w).set(lens_of(257, {97: 1, 98: 2, 256: 2}), [0])
    c.header(); c.lit(b"abba"); c.sym(256)
    h["dynamic_no_distance_code"] = w.done()
    ll = lens_of(257, {97 + i: i + 1 for i in range(14)})
    ll[97 + 14] = ll[256] = 15
    w = BitW(); c = Coder(w).set(ll, [1, 1])
    c.header(); c.lit(b"abcdefghijklmnoonmlkjihgfedcba"); c.sym(256)
    h["dynamic_15_bit_code"] = w.done()
    w = BitW(); c = Coder(w).set(lens_of(258, {97: 2, 98: 2, 256: 2, 257: 2}), [2, 2, 2, 2])
    assert c.header(), "the repeat did not cross the HLIT boundary"
    c.lit(b"abab"); c.match(3, 4); c.match(3, 1); c.sym(256)
    h["dynamic_repeat_across_hlit"] = w.done()
    # many deflate blocks, sync and full flushes between the pieces, ending off a byte boundary
    t = text(9000)
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    s = b""
    for a, b, f in ((0, 1000, zlib.Z_SYNC_FLUSH), (1000, 1001, zlib.Z_FULL_FLUSH), (1001, 4000, zlib.Z_SYNC_FLUSH), (4000, 7777, zlib.Z_FULL_FLUSH)):
        s += z.compress(t[a:b]) + z.flush(f)
    w = BitW(); c = Coder(w).fixed(); c.lit(b"end"); c.match(10, 500); c.sym(256)      # (3 + 3 * 8 + 7 + 5 + 7 + 7 = 53 bits: the stream ends off a byte boundary)
    assert w.n != 0
    h["many_deflate_blocks"] = s + w.done()
    return h


def text(n: int, seed: int = 7) -> bytes:
    r = random.Random(seed)
    out = bytearray()
    i = 0
    while len(out) < n:
        out += b'{"name":"user-%d","age":%d,"emails":["u%d@example.org"],"status":%s}' % (
            i * 7919 % 1000, r.randrange(90), r.randrange(50), b"null" if i % 3 else b'"%s"' % bytes([97 + r.randrange(26)]) * (1 + r.randrange(9)))
        i += 1
    return bytes(out[:n])


HAND: Dict[str, bytes] = _hand()

STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "fixed": zlib.Z_FIXED, "rle": zlib.Z_RLE, "huffman_only": zlib.Z_HUFFMAN_ONLY}


def zlib_made(payloads: Dict[str, bytes]) -> List[Tuple[str, bytes, bytes]]:
    out = []
    for name, p in payloads.items():
        for level in (0, 1, 6, 9):
            for sname, strat in STRATEGIES.items():
                z = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strat)
                out.append((f"{name}/{level}/{sname}", z.compress(p) + z.flush(), p))
    return out


def classify(stream: bytes):
    """zlib's verdict on a raw-deflate stream -> (class, the bytes when the stream is whole, the trailing byte count)"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(stream)
    except zlib.error:
        return MALFORMED, None, 0
    if not d.eof:
        return TRUNCATED, None, 0
    if d.unused_data:
        return TRAILING, out, len(d.unused_data)
    return OK, out, 0


@functools.lru_cache(maxsize=None)
def damage_cases(stream: bytes):
    """-> (flips, prefixes, prefixes_of_refused): every single-bit flip of `stream`, every proper prefix of it, and every proper
    prefix of a dozen of the flipped streams that zlib refuses (spread over the stream)."""
    flips = []
    for i in range(len(stream)):
        for bit in range(8):
            g = bytearray(stream)
            g[i] ^= 1 << bit
            flips.append(bytes(g))
    prefixes = [stream[:cut] for cut in range(len(stream))]
    refused = [f for f in flips if classify(f)[0] == MALFORMED]
    step = max(1, len(refused) // 12)
    chosen = refused[::step][:12]
    return flips, prefixes, [f[:cut] for f in chosen for cut in range(len(f))]
