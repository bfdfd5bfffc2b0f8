"""Payloads for the deflate writer's tests (test_container_deflate.py): the smallest shapes at which a writer
can go wrong.  Nothing here comes from the engine: the bytes are made by ``random``, by deflate_cases (noise, text) and by the
oracle's encoder (container_cases.records_of)."""
from __future__ import annotations

import functools
import random
from typing import Dict

import container_cases as CC
from deflate_cases import noise, text

K = 32768      # the writer's segment (cabi.DEFLATE_SEGMENT; the tests check that the two agree)
LAYOUT_SCHEMAS = ("full", "array_and_map", "t_union", "nullable_primitives")
SIZE_PAYLOADS = LAYOUT_SCHEMAS + ("text_200000",)      # the five whose size is compared with zlib's


def _fibonacci(seed: int = 20261020) -> bytes:
    """byte frequencies 1, 1, 2, 3, 5, ... over 20 values, shuffled: an unlimited Huffman code would need 19 bits"""
    out, a, b = bytearray(), 1, 1
    for v in range(20):
        out += bytes([v * 11 + 3]) * a
        a, b = b, a + b
    out = list(out)
    random.Random(seed).shuffle(out)
    return bytes(out)


@functools.lru_cache(maxsize=None)
def payloads() -> Dict[str, bytes]:
    p = {}
    for n in (0, 1, 2, 3, 4):
        p[f"len_{n}"] = text(n)
    for n in (257, 258, 259, 260, 517):
        p[f"one_byte_{n}"] = b"A" * n                      # the longest match, and remainders shorter than a match
    p["ab_130"] = b"ab" * 130
    p["every_byte_twice"] = bytes(range(256)) * 2
    far = noise(32768, 11)
    p["distance_32768"] = far + far[:300]                  # usable by the format
    far = noise(32769, 12)
    p["distance_32769"] = far + far[:300]                  # not usable
    for n in (65535, 65536, 65537):
        p[f"noise_{n}"] = noise(n, n)                      # the stored LEN limit
    for n in (K - 1, K, K + 1, 2 * K + 3):
        p[f"text_{n}"] = text(n, n)                        # the segment joints
    p["zeros"] = bytes(3 * K + 5)
    p["fibonacci"] = _fibonacci()
    for name in LAYOUT_SCHEMAS:
        p[name] = b"".join(CC.records_of(name, 4096))      # one container block of 4,096 records
    p["text_200000"] = text(200000)
    return p
