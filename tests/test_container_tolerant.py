"""Tolerant container reads: ``read_container_tolerant`` / ``read_container_to_device_tolerant``, the salvage
scan behind them and the two kernels.

The contract, for every file F with writer schema W, and every k:

    batches == deserialize_array_threaded(kept_records(F), W, k, **kw)      buffer for buffer, batch for batch

The files are put together by tests/salvage_cases.py, which knows from HOW it damaged a file which records a tolerant read keeps
and which entries it reports; the expected batches are the ORACLE's decode of those records -- never the engine's output."""
import inspect
import os
import subprocess
import sys
import zlib

import numpy as np
import pyarrow as pa
import pytest

import container_cases as CC
import deflate_cases as DC
import resolve_cases as RC
import salvage_cases as SC
from avrogen import synth
from avrogen.encoder import to_datum
from avrogen.schemas import SCHEMAS
from oracle import c_walker
from oracle.avro_schema import parse_schema

import pyruhvro
import pyruhvro_amd as P
from pyruhvro_amd import cabi
from pyruhvro_amd import container as CT
from test_projection import PARENT_KEYS
from test_resolution import _oracle, _same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"generic": cabi.KERNEL_GENERIC, "specialized": cabi.KERNEL_SPECIALIZED}
FULL = SCHEMAS["full"]
NEW_SYMBOLS = ("rh_container_salvage", "rh_container_info_salvage", "rh_container_info_gap", "rh_block_status_message",
               "rh_decode_blocks_tolerant", "rh_decode_blocks_tolerant_device", "rh_salvage_last")
KINDS = sorted(CC.DAMAGE_MESSAGES)
EDGE_BLOCKS = (0, 63, 64, 255, 256)      # wavefront and workgroup edges, and the last block of a 257-block file


@pytest.fixture(params=sorted(KERNELS))
def kernel(request):
    old = P.set_kernel_mode(request.param)
    yield KERNELS[request.param]
    P.set_kernel_mode(old)


# ---- CPU: the salvage scan --------------------------------------------------------------------------------------------------------
def _salvage(blob):
    return cabi.container_salvage(np.frombuffer(blob, dtype=np.uint8))


def _three():
    recs = CC.records_of("full", 9)
    return CC.header(FULL, "null", {"who": b"test"}), [SC.Block(recs[i:i + 3]) for i in (0, 3, 6)]


def _tiles(s, n):
    """blocks and gaps, ascending, disjoint, tile [header_end, n)"""
    spans = [(int(h), int(e) + 16) for h, e in zip(s["header_offset"], s["end"])] + [(o, o + ln) for o, ln, _, _ in s["gaps"]]
    at = s["header_end"]
    for lo, hi in sorted(spans):
        assert lo == at and hi > lo
        at = hi
    assert at == n


def test_an_undamaged_file_scans_as_the_strict_scan_does():
    for layout in sorted(CC.LAYOUTS):
        counts = CC.LAYOUTS[layout]
        blob = CC.write(FULL, CC.split(CC.records_of("full", sum(counts)), counts))
        buf = np.frombuffer(blob, dtype=np.uint8)
        s, t = cabi.container_salvage(buf), cabi.container_scan(buf)
        for key in ("schema", "codec", "sync", "metadata"):
            assert s[key] == t[key]
        for key in ("start", "end", "first"):
            assert s[key].tolist() == t[key].tolist()
        assert s["gaps"] == [] and not s["refused"].any() and s["count"].tolist() == counts
        _tiles(s, len(blob))


def test_a_flipped_marker_byte_is_one_gap_that_swallows_that_block_and_the_next():
    hdr, blocks = _three()
    raw = [b.bytes("null") for b in blocks]
    blob = hdr + SC.broken_marker(blocks[0]) + raw[1] + raw[2]
    s = _salvage(blob)
    assert s["gaps"] == [(len(hdr), len(raw[0]) + len(raw[1]), 0, "container: block 0: sync marker mismatch")]
    assert s["header_offset"].tolist() == [len(hdr) + len(raw[0]) + len(raw[1])] and s["first"].tolist() == [0, 3]
    _tiles(s, len(blob))
    with pytest.raises(ValueError) as e:
        P.container_info(blob)
    assert str(e.value) == s["gaps"][0][3]


def test_damaged_block_headers():
    hdr, blocks = _three()
    raw = [b.bytes("null") for b in blocks]
    recs = blocks[1].records
    size = sum(map(len, recs))
    tail = b"".join(recs) + CC.SYNC
    # (what is written in block 1's place, the strict scan's words) -- each is one gap of exactly that block
    for bad, words in ((CC.zz(3) + CC.zz(size + 1) + tail, "sync marker mismatch"),          # a size one larger
                       (CC.zz(3) + CC.zz(size - 1) + tail, "sync marker mismatch"),          # ... and one smaller
                       (CC.zz(3) + CC.zz(1 << 40) + tail, f"size {1 << 40} runs past the end of the file"),
                       (CC.zz(-3) + CC.zz(size) + tail, "negative record count -3"),
                       (CC.zz(3) + CC.zz(-1) + tail, "negative size -1"),
                       (b"\xff" * 11 + tail, "truncated block header (bytes left after the last complete block)")):
        blob = hdr + raw[0] + bad + raw[2]
        s = _salvage(blob)
        assert s["gaps"] == [(len(hdr) + len(raw[0]), len(bad), 1, "container: block 1: " + words)]
        assert s["first"].tolist() == [0, 3, 6] and s["header_offset"].tolist() == [len(hdr), len(hdr) + len(raw[0]) + len(bad)]
        _tiles(s, len(blob))
        with pytest.raises(ValueError) as e:
            P.container_info(blob)
        assert str(e.value) == s["gaps"][0][3]
    # a gap at the very first block; two adjacent gaps; a marker-only tail
    neg = CC.zz(-3) + CC.zz(size) + tail
    s = _salvage(hdr + neg + raw[1] + raw[2])
    assert s["gaps"] == [(len(hdr), len(neg), 0, "container: block 0: negative record count -3")] and s["first"].tolist() == [0, 3, 6]
    s = _salvage(hdr + raw[0] + neg + neg + raw[2])
    at = len(hdr) + len(raw[0])
    assert s["gaps"] == [(at, len(neg), 1, "container: block 1: negative record count -3"), (at + len(neg), len(neg), 1, "container: block 1: negative record count -3")]
    assert s["first"].tolist() == [0, 3, 6]
    blob = hdr + b"".join(raw) + CC.SYNC
    s = _salvage(blob)
    assert s["gaps"] == [(len(blob) - 16, 16, 3, "container: block 3: truncated block header (bytes left after the last complete block)")]
    assert s["first"].tolist() == [0, 3, 6, 9]
    _tiles(s, len(blob))
    # a count the running total cannot take: the block is framed, refused, and counts as nothing
    big = CC.zz((1 << 62) + 1) + CC.zz(size) + tail
    s = _salvage(hdr + raw[0] + big + raw[2])
    assert s["gaps"] == [] and s["refused"].tolist() == [0, 1, 0] and s["first"].tolist() == [0, 3, 3, 6] and int(s["count"][1]) == (1 << 62) + 1


def test_a_file_cut_at_every_byte_of_its_last_block():
    hdr, blocks = _three()
    raw = [b.bytes("null") for b in blocks]
    blob = hdr + b"".join(raw)
    whole = len(hdr) + len(raw[0]) + len(raw[1])
    assert _salvage(blob[:whole])["gaps"] == []
    for cut in range(1, len(raw[2])):
        s = _salvage(blob[:whole + cut])
        assert s["first"].tolist() == [0, 3, 6]
        assert len(s["gaps"]) == 1 and s["gaps"][0][:3] == (whole, cut, 2) and s["gaps"][0][3].startswith("container: block 2: ")
        with pytest.raises(ValueError) as e:
            P.container_info(blob[:whole + cut])
        assert str(e.value) == s["gaps"][0][3]
    # a header that does not parse is not salvaged: what the strict scan raises
    for cut in (0, 3, 4, len(hdr) - 1):
        with pytest.raises(ValueError) as e:
            _salvage(blob[:cut])
        with pytest.raises(ValueError) as e2:
            P.container_info(blob[:cut])
        assert str(e.value) == str(e2.value)
    with pytest.raises(ValueError, match="^container: codec 'snappy' is not supported$"):
        P.read_container_tolerant(CC.header(FULL, "snappy"))
    with pytest.raises(ValueError, match="^container: inflate must be 'host' or 'device'$"):
        P.read_container_tolerant(blob, inflate="zlib")
    with pytest.raises(TypeError):
        P.read_container_tolerant(blob, "2")
    with pytest.raises(TypeError):
        P.read_container_tolerant(blob, max_errors="2")


def test_new_symbols_and_unchanged_ground():
    for name in NEW_SYMBOLS:
        assert getattr(cabi.lib(), name, None) is not None, name
    assert cabi.lib().rh_abi_version() == 7
    for name in ("full", "cfg3", "flat4"):
        assert cabi.kernel_key(SCHEMAS[name]) == PARENT_KEYS[name]


def test_signatures_are_keyword_only_on_both_module_names():
    for mod in (P, pyruhvro):
        for fn, lead in ((mod.read_container_tolerant, ["src", "num_chunks"]), (mod.read_container_to_device_tolerant, ["src", "num_chunks", "device"])):
            ps = inspect.signature(fn).parameters
            assert [n for n, p in ps.items() if p.kind == p.POSITIONAL_OR_KEYWORD] == lead
            assert [n for n, p in ps.items() if p.kind == p.KEYWORD_ONLY] == ["max_errors", "columns", "reader_schema", "inflate"]
            assert ps["max_errors"].default == 1024 and ps["num_chunks"].default == 1
        assert mod.BlockError._fields == ("block", "offset", "length", "kept", "lost", "message")
    assert pyruhvro.read_container_tolerant is P.read_container_tolerant
    assert pyruhvro.read_container_to_device_tolerant is P.read_container_to_device_tolerant


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
def _entries(errors):
    return [tuple(e) for e in errors]


def _check(f: SC.File, schema=FULL, ks=(1, 3), gathered=True, **kw):
    """The contract on one assembled file, for every k of `ks`."""
    for k in ks:
        got, errors = P.read_container_tolerant(f.blob, k, **kw)
        assert _entries(errors) == f.errors
        assert all(isinstance(e, P.BlockError) for e in errors)
        _same(got, c_walker.decode_threaded(list(f.kept), schema, k))
        last = cabi.salvage_last()
        assert (last["bytes_gathered"] > 0) == (gathered and len(f.kept) > 0)
    return errors


def _strict_message(blob, **kw):
    with pytest.raises(ValueError) as e:
        P.read_container(blob, 1, **kw)
    return str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(CC.LAYOUTS))
def test_clean_files(kernel, layout):
    counts = CC.LAYOUTS[layout]
    n = sum(counts)
    for name in ("full", "t_union"):
        blob = CC.write(SCHEMAS[name], CC.split(CC.records_of(name, n), counts))
        for k in (1, 3):
            got, errors = P.read_container_tolerant(blob, k)
            assert errors == []
            _same(got, P.read_container(blob, k))
            _same(got, CC.expected(name, n, k))
            assert cabi.salvage_last()["bytes_gathered"] == 0 and cabi.salvage_last()["blocks_reported"] == 0
    blob = CC.write(FULL, CC.split(CC.records_of("full", n), counts), "deflate")
    for road in ("host", "device"):
        got, errors = P.read_container_tolerant(blob, 2, inflate=road)
        assert errors == [] and cabi.salvage_last()["bytes_gathered"] == 0
        _same(got, CC.expected("full", n, 2))


def _damage(blocks, b, j, kind):
    """Block b of `blocks` (lists of records) with its record j damaged -> the SC.Block that says so."""
    recs = list(blocks[b])
    recs[j] = CC.damaged_full(kind, 1000 + 7 * b + j)
    return SC.Block(recs, kept=j, message=CC.DAMAGE_MESSAGES[kind])


def _pieces(blocks, damaged):
    return [damaged.get(b) or SC.Block(recs) for b, recs in enumerate(blocks)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_one_damaged_record_at_the_wavefront_and_workgroup_edges(kernel, kind):
    blocks = CC.split(CC.records_of("full", 3 * 257), [3] * 257)
    # the precondition, on the oracle alone: the verdict of the damaged record does not depend on what follows it
    bad = CC.damaged_full(kind, 1000)
    for recs in ([bad], [bad + b"".join(blocks[1])]):
        with pytest.raises(ValueError) as e:
            c_walker.decode_threaded(recs, FULL, 1)
        assert str(e.value) == CC.DAMAGE_MESSAGES[kind]
    # one damaged block at a time: j = 0, the middle record, the last record, by turns; the message is the strict read's
    for i, b in enumerate(EDGE_BLOCKS):
        j = (i + KINDS.index(kind)) % 3
        f = SC.assemble(FULL, _pieces(blocks, {b: _damage(blocks, b, j, kind)}))
        errors = _check(f, ks=(1,) if i else (1, 3))
        assert (errors[0].block, errors[0].kept, errors[0].lost) == (b, j, 3 - j)
        assert errors[0].message == CC.DAMAGE_MESSAGES[kind] == _strict_message(f.blob)
    # all of them in one file, and two adjacent ones (63 and 64: the last lane of a wavefront and the first of the next)
    f = SC.assemble(FULL, _pieces(blocks, {b: _damage(blocks, b, (i + 1) % 3, kind) for i, b in enumerate(EDGE_BLOCKS)}))
    errors = _check(f, ks=(1, 8))
    assert [e.block for e in errors] == list(EDGE_BLOCKS) and len(f.kept) == 3 * 257 - sum(e.lost for e in errors)


@pytest.mark.gpu
def test_larger_blocks_empty_neighbours_and_files_that_keep_nothing(kernel):
    counts = [1, 300, 1, 0, 0, 5, 0, 2]
    blocks = CC.split(CC.records_of("full", sum(counts)), counts)
    # a single-record block, the middle of a 300-record block, the last record of a block between empty ones
    for b, j in ((0, 0), (1, 150), (1, 299), (5, 4), (5, 0)):
        f = SC.assemble(FULL, _pieces(blocks, {b: _damage(blocks, b, j, "union")}))
        errors = _check(f)
        assert (errors[0].block, errors[0].kept, errors[0].lost, errors[0].message) == (b, j, counts[b] - j, _strict_message(f.blob))
    f = SC.assemble(FULL, _pieces(blocks, {0: _damage(blocks, 0, 0, "bool"), 1: _damage(blocks, 1, 17, "enum"), 2: _damage(blocks, 2, 0, "union")}))
    _check(f)
    # every block damaged at its first record: nothing is kept -- what the list call gives for no records
    blocks = CC.split(CC.records_of("full", 6), [2, 2, 2])
    f = SC.assemble(FULL, _pieces(blocks, {b: _damage(blocks, b, 0, KINDS[b]) for b in range(3)}))
    assert f.kept == []
    _check(f, ks=(1, 3))
    for k in (1, 3):
        _same(P.read_container_tolerant(f.blob, k)[0], P.deserialize_array_threaded([], FULL, k))


@pytest.mark.gpu
def test_counts(kernel):
    recs = list(CC.records_of("full", 60))
    mid = recs[20:40]
    size = sum(map(len, mid))

    def file(block):
        return SC.assemble(FULL, [SC.Block(recs[:20]), block, SC.Block(recs[40:])])
    # one less than the truth: every claimed record is kept, the block is reported for the bytes behind them
    f = file(SC.Block(mid, count=19, kept=19, lost=0, message=f"container: block 1: its 19 records end at byte {size - len(mid[-1])} of {size}"))
    _check(f)
    assert f.errors[0][5] == _strict_message(f.blob)
    # one more: the true records are kept; record 20 runs out of bytes at the block's end
    probe = file(SC.Block(mid, count=21, kept=20, message="?"))
    f = file(SC.Block(mid, count=21, kept=20, lost=1, message=_strict_message(probe.blob)))
    _check(f)
    # an empty block that holds bytes
    f = file(SC.Block(mid[:1], count=0, kept=0, lost=0, message=f"container: block 1: its 0 records end at byte 0 of {len(mid[0])}"))
    _check(f)
    assert f.errors[0][5] == _strict_message(f.blob)
    # a count the bytes cannot hold: dropped without a walk
    f = file(SC.Block(mid, count=1 << 40, kept=0, message=f"container: block 1: {1 << 40} records cannot be in its {size} bytes"))
    _check(f)
    assert f.errors[0][5] == _strict_message(f.blob) and f.errors[0][4] == 1 << 40
    for road in ("host", "device"):
        g = SC.assemble(FULL, [SC.Block(recs[:20]), SC.Block(mid, count=1 << 40, kept=0, message=f"container: block 1: {1 << 40} records cannot be in its {size} bytes"),
                               SC.Block(recs[40:])], "deflate")
        _check(g, inflate=road)
    # a count the running total cannot take
    f = file(SC.Block(mid, count=(1 << 62) + 1, kept=0, message="container: block 1: record count out of range"))
    _check(f)
    assert f.errors[0][5] == _strict_message(f.blob)


T_UNION = SCHEMAS["t_union"]
_TU = parse_schema(T_UNION)


def _tu(value) -> bytes:
    return to_datum(_TU, {"u": value})


def _tu_of_length(n: int) -> bytes:
    rec = _tu(None) if n == 1 else _tu("x" * (n - 2) if n < 66 else "y" * (n - 3))
    assert len(rec) == n
    return rec


@pytest.mark.gpu
def test_gather_alignment(kernel):
    bad = b"\x0e"                                   # branch 7 of a 4-branch union
    with pytest.raises(ValueError) as e:
        c_walker.decode_threaded([bad], T_UNION, 1)
    message = str(e.value)
    lengths = list(range(1, 34)) + [5000] + list(range(1, 31))        # 64 damaged blocks: every misalignment four times
    pieces = []
    at = len(CC.header(T_UNION, "null"))
    for i, n in enumerate(lengths):
        # a sound filler block of one or two records, sized so that the damaged block's payload starts at misalignment i % 16
        head = 2 if n + 1 < 64 else 3                # the damaged block's count and size varints
        m = (i % 16 - (at + 20 + head)) % 16
        filler = [_tu("f" * m)] if i % 2 else [_tu(True), _tu("f" * (m - 2) if m >= 2 else "f" * (m + 14))]
        fb = SC.Block(filler)
        at += len(fb.bytes("null"))
        blk = SC.Block([_tu_of_length(n), bad], kept=1, message=message)
        pieces += [fb, blk]
        at += len(blk.bytes("null"))
    f = SC.assemble(T_UNION, pieces)
    # the coverage, on the scan's table alone, before the engine is called
    s = _salvage(f.blob)
    assert s["gaps"] == [] and len(s["start"]) == 128
    runs = [(int(s["start"][b]) % 16, lengths[b // 2]) for b in range(1, 128, 2)]
    assert {mis for mis, _ in runs} == set(range(16))
    assert {n for _, n in runs} >= set(range(1, 34)) and max(n for _, n in runs) > 4096
    assert message == _strict_message(f.blob)
    _check(f, T_UNION, ks=(1, 3, 8))
    # fewer kept records than chunks
    f = SC.assemble(T_UNION, [SC.Block([_tu(5), bad, _tu(6)], kept=1, message=message), SC.Block([_tu("ab"), _tu(None)])])
    assert len(f.kept) == 3
    _check(f, T_UNION, ks=(8,))


def _streams(recs):
    """-> the block's sound stream and (stream, host words or None, device words) of a truncated one, one with trailing bytes and one refused by rule"""
    z = zlib.compressobj(wbits=-15)
    body = z.compress(b"".join(recs)) + z.flush()
    cut, behind = body[:-3], body + b"\x00\x01"
    rule = next(s for s in DC.damage_cases(body)[0] if DC.classify(s)[0] == DC.MALFORMED)
    assert DC.classify(body)[0] == DC.OK and DC.classify(cut)[0] == DC.TRUNCATED and DC.classify(behind)[0] == DC.TRAILING
    return [(cut, "the stream ends before its final block"), (behind, "2 bytes behind the end of the stream"), (rule, None)]


@pytest.mark.gpu
def test_deflate_both_roads(kernel, monkeypatch):
    blocks = CC.split(CC.records_of("full", 3 * 257), [3] * 257)
    hdr = CC.header(FULL, "deflate")

    def one(b, stream):      # the file in which block b's stream is the only damage
        return hdr + b"".join(SC.Block(r, stream=stream if i == b else None).bytes("deflate") for i, r in enumerate(blocks))
    # what each road's strict read says of every damaged stream, before zlib is taken away: the words are fixed where both roads
    # word them, a stream refused by rule has each road's own reason
    damaged, words = {}, {"host": {}, "device": {}}
    for i, b in enumerate(EDGE_BLOCKS):
        stream, fixed = _streams(blocks[b])[i % 3]
        for road in ("host", "device"):
            words[road][b] = _strict_message(one(b, stream), inflate=road)
            assert words[road][b].startswith(f"container: block {b}: deflate: ")
            if fixed:
                assert words[road][b] == f"container: block {b}: deflate: {fixed}"
        damaged[b] = stream
    damaged_rec = _damage(blocks, 100, 1, "enum")
    results = {}
    for road in ("host", "device"):
        pieces = _pieces(blocks, {b: SC.Block(blocks[b], kept=0, stream=s, message=words[road][b]) for b, s in damaged.items()})
        pieces[100] = damaged_rec
        f = SC.assemble(FULL, pieces, "deflate")
        if road == "device":
            def no_zlib(*a, **kw):
                raise AssertionError("the device road called the host's inflate")
            monkeypatch.setattr(CT, "_inflate", no_zlib)
            monkeypatch.setattr(CT.zlib, "decompressobj", no_zlib)
        results[road] = (f, _check(f, ks=(1, 3), inflate=road))
        monkeypatch.undo()
    (fh, eh), (fd, ed) = results["host"], results["device"]
    assert fh.blob == fd.blob and fh.kept == fd.kept
    assert [tuple(e)[:5] for e in eh] == [tuple(e)[:5] for e in ed]
    # identical messages wherever the strict roads' messages are identical (a stream refused by rule carries each road's reason)
    for a, b in zip(eh, ed):
        assert (a.message == b.message) == (words["host"].get(a.block) == words["device"].get(a.block))


@pytest.mark.gpu
def test_framing_and_payload_damage_in_one_file(kernel):
    recs = list(CC.records_of("full", 70))
    b = [SC.Block(recs[i:i + 10]) for i in range(0, 70, 10)]
    bad = list(recs[40:50])
    bad[6] = CC.damaged_full("bool", 46)
    tail = b[6].bytes("null")[:-5]
    pieces = [b[0],
              SC.Junk(SC.broken_marker(b[1]) + b[2].bytes("null"), "container: block {b}: sync marker mismatch"),      # swallows block 2 too
              b[3],
              SC.Block(bad, kept=6, message=CC.DAMAGE_MESSAGES["bool"]),
              b[5],
              SC.Junk(tail, "container: block {b}: truncated sync marker (bytes left after the last complete block)")]
    f = SC.assemble(FULL, pieces)
    assert [e[0] for e in f.errors] == [None, 2, None] and f.kept == recs[:10] + recs[30:46] + recs[50:60]
    errors = _check(f)
    assert [e.offset for e in errors] == sorted(e.offset for e in errors)
    assert errors[0] == P.BlockError(None, f.offsets[1], len(pieces[1].raw), 0, None, "container: block 1: sync marker mismatch")
    assert errors[2].lost is None and errors[2].offset + errors[2].length == len(f.blob)
    # the same with deflate blocks, a refused stream in place of the damaged record, on both roads
    z = zlib.compressobj(wbits=-15)
    body = z.compress(b"".join(recs[40:50])) + z.flush()
    pieces[3] = SC.Block(recs[40:50], kept=0, stream=body[:-3], message="container: block {b}: deflate: the stream ends before its final block")
    pieces[1] = SC.Junk(SC.broken_marker(b[1], "deflate") + b[2].bytes("deflate"), "container: block {b}: sync marker mismatch")
    pieces[5] = SC.Junk(b[6].bytes("deflate")[:-5], "container: block {b}: truncated sync marker (bytes left after the last complete block)")
    f = SC.assemble(FULL, pieces, "deflate")
    for road in ("host", "device"):
        _check(f, inflate=road)


@pytest.mark.gpu
def test_max_errors(kernel):
    blocks = CC.split(CC.records_of("full", 40), [10] * 4)
    f = SC.assemble(FULL, _pieces(blocks, {1: _damage(blocks, 1, 4, "enum"), 2: _damage(blocks, 2, 0, "bool")}) +
                    [SC.Junk(b"\x02", "container: block {b}: truncated block header (bytes left after the last complete block)")])
    assert len(f.errors) == 3
    _check(f, max_errors=3)
    for limit in (2, 0):
        with pytest.raises(ValueError) as e:
            P.read_container_tolerant(f.blob, 2, max_errors=limit)
        assert str(e.value) == _strict_message(f.blob) == "container: block 4: truncated block header (bytes left after the last complete block)"
    # without the gap the strict error is the lowest record's
    f = SC.assemble(FULL, _pieces(blocks, {1: _damage(blocks, 1, 4, "enum"), 2: _damage(blocks, 2, 0, "bool")}))
    _check(f, max_errors=2)
    with pytest.raises(ValueError) as e:
        P.read_container_tolerant(f.blob, 2, max_errors=1)
    assert str(e.value) == _strict_message(f.blob) == CC.DAMAGE_MESSAGES["enum"]
    with pytest.raises(ValueError) as e:
        P.read_container_to_device_tolerant(f.blob, 2, max_errors=1)
    assert str(e.value) == CC.DAMAGE_MESSAGES["enum"]


@pytest.mark.gpu
def test_composition(kernel):
    import torch
    n = 120
    recs = list(CC.records_of("full", n))
    values = [synth.gen_full(20260921, i) for i in range(n)]
    assert RC.writer_records(FULL, values) == recs
    blocks = CC.split(recs, [30] * 4)
    f = SC.assemble(FULL, _pieces(blocks, {1: _damage(blocks, 1, 12, "union"), 3: _damage(blocks, 3, 29, "enum")}))
    keep = list(range(0, 42)) + list(range(60, 119))
    assert f.kept == [recs[i] for i in keep]
    cols = ["created_at", "name"]
    exp = c_walker.decode_threaded(f.kept, FULL, 3)
    got, errors = P.read_container_tolerant(f.blob, 3, columns=cols)
    assert _entries(errors) == f.errors
    _same(got, [b.select(cols) for b in exp])
    got, errors = P.read_container_tolerant(f.blob, 3, reader_schema=RC.FULL_MIXED)
    assert _entries(errors) == f.errors
    _same(got, _oracle(RC.reader_records(FULL, RC.FULL_MIXED, [values[i] for i in keep]), RC.FULL_MIXED, 3))
    dec = P.read_container_to_device_tolerant(f.blob, 3, device=0)
    assert _entries(dec.errors) == f.errors
    assert [b.num_rows for b in dec.batches] == [b.num_rows for b in exp]
    for g, e in zip(dec.batches, exp):      # a DLPack column over the engine's buffer
        t = torch.from_dlpack(g.column("created_at").values)
        assert t.cpu().numpy().tolist() == e.column("created_at").cast(pa.int64()).to_pylist()
    _same(dec.to_host(), exp)
    dec.free()
    dec = P.read_container_to_device_tolerant(SC.assemble(FULL, _pieces(blocks, {}), "deflate").blob, 2, inflate="device")
    assert dec.errors == []
    _same(dec.to_host(), CC.expected("full", n, 2))


@pytest.mark.gpu
def test_record_damage_under_poisoned_pools(monkeypatch):
    """RUHVRO_HIP_POISON=1 (pooled memory handed out as 0xA5; read once per process, so the cases run in a process of their own):
    the pad bytes behind every gathered run and the bytes behind the gathered buffer must not matter."""
    monkeypatch.setenv("RUHVRO_HIP_POISON", "1")
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_container_tolerant.py"), "-m", "gpu", "-q", "-x", "-k",
                        "test_one_damaged_record_at_the_wavefront_and_workgroup_edges or test_gather_alignment"], cwd=ROOT,
                       env=dict(os.environ), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and " passed" in p.stdout, p.stdout[-2500:] + p.stderr[-1500:]


@pytest.mark.gpu
def test_single_bit_flips_in_one_block(kernel):
    """No verdict is asserted (the tree has no CPU split oracle): the call returns, every other block's rows and the rows in front
    of the flipped record are the oracle's, and a block keeps no more than it claims."""
    counts = [20, 30, 25]
    recs = list(CC.records_of("full", sum(counts)))
    blocks = CC.split(recs, counts)
    f = SC.assemble(FULL, [SC.Block(b) for b in blocks])
    exp = pa.Table.from_batches(c_walker.decode_threaded(recs, FULL, 1))
    payload_at = f.offsets[1] + len(CC.zz(30)) + len(CC.zz(sum(map(len, blocks[1]))))
    ends = np.cumsum([len(r) for r in blocks[1]])
    size = int(ends[-1])
    for i in range(64):
        pos, bit = (i * 2654435761) % size, (i * 5) % 8        # fixed, spread over the payload
        r = int(np.searchsorted(ends, pos, side="right"))        # the record the flipped byte belongs to
        blob = bytearray(f.blob)
        blob[payload_at + pos] ^= 1 << bit
        got, errors = P.read_container_tolerant(bytes(blob), 1)
        assert all(e.block == 1 for e in errors) and len(errors) <= 1
        kept = errors[0].kept if errors else 30
        assert r <= kept <= 30
        t = pa.Table.from_batches(got)
        assert t.num_rows == 20 + kept + 25
        assert t.slice(0, 20 + r).equals(exp.slice(0, 20 + r))
        assert t.slice(20 + kept).equals(exp.slice(50))
