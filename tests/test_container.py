"""Avro object container files: ``container_info`` / ``read_container`` / ``read_container_to_device`` / ``write_container``.

The contract, for every container file F with writer schema W, and every k:

    read_container(F, k, **kw) == deserialize_array_threaded(records_of(F), W, k, **kw)      buffer for buffer, batch for batch

The files are written by the tests' own writer (tests/container_cases.py) and the expected batches are the ORACLE's decode of
the records that writer put into the file -- never the engine's own output."""
import mmap
import os
import zlib

import numpy as np
import pyarrow as pa
import pytest

import container_cases as CC
import resolve_cases as RC
from arrow_compare import assert_batches_identical
from avrogen import synth
from avrogen.encoder import to_datum
from avrogen.schemas import SCHEMAS
from oracle import c_walker

import pyruhvro
import pyruhvro_amd as P
from pyruhvro_amd import cabi
from test_projection import PARENT_KEYS
from test_resolution import _oracle, _same

KERNELS = {"generic": cabi.KERNEL_GENERIC, "specialized": cabi.KERNEL_SPECIALIZED}
FULL = SCHEMAS["full"]
LAYOUT_SCHEMAS = ("full", "array_and_map", "t_union", "nullable_primitives")


@pytest.fixture(params=sorted(KERNELS))
def kernel(request):
    old = P.set_kernel_mode(request.param)
    yield KERNELS[request.param]
    P.set_kernel_mode(old)


def _file(name, layout, codec="null", **kw):
    counts = CC.LAYOUTS[layout]
    return CC.write(SCHEMAS[name], CC.split(CC.records_of(name, sum(counts)), counts), codec, **kw), sum(counts)


# ---- CPU: framing ---------------------------------------------------------------------------------------------------------------
def _three_blocks():
    recs = CC.records_of("full", 9)
    return CC.header(FULL, "null", {"who": b"test"}), [CC.block(recs[i:i + 3]) for i in (0, 3, 6)]


def _refused(blob, word=None):
    with pytest.raises(ValueError) as e:
        P.container_info(blob)
    assert str(e.value).startswith("container: "), str(e.value)
    if word is not None:
        assert word in str(e.value), str(e.value)
    return str(e.value)


def test_info_of_a_valid_file():
    hdr, blocks = _three_blocks()
    info = P.container_info(hdr + b"".join(blocks))
    assert info.schema == FULL and info.codec == "null" and info.sync == CC.SYNC
    assert info.metadata == {"who": b"test"}
    assert (info.num_blocks, info.num_records) == (3, 9)
    assert pyruhvro.container_info is P.container_info and pyruhvro.read_container is P.read_container
    assert pyruhvro.read_container_to_device is P.read_container_to_device and pyruhvro.write_container is P.write_container


def test_every_cut_of_the_header_and_of_the_first_blocks_framing_is_refused():
    hdr, blocks = _three_blocks()
    blob = hdr + b"".join(blocks)
    for cut in range(len(hdr)):                                        # every byte of the header
        _refused(blob[:cut])
    assert P.container_info(blob[:len(hdr)]).num_blocks == 0           # (the whole header and nothing else: a file of zero blocks)
    first = blocks[0]
    size = sum(map(len, CC.records_of("full", 9)[:3]))
    framing = len(CC.zz(3) + CC.zz(size))                              # count + size
    assert first[:framing] == CC.zz(3) + CC.zz(size) and len(first) == framing + size + 16
    cuts = list(range(1, framing + 1)) + list(range(len(first) - 16, len(first)))   # its count, its size, its sync marker
    for cut in cuts:
        msg = _refused(blob[:len(hdr) + cut], "block 0")
        assert msg.startswith("container: block 0: ")
    # cut inside a LATER block: the message names it
    _refused(blob[:len(hdr) + len(blocks[0]) + len(blocks[1]) + 5], "block 2")


def test_header_shapes():
    recs = CC.records_of("full", 4)
    body = CC.block(recs)
    # the metadata map in two blocks, each with a negative count and a byte size
    blob = CC.header(FULL, "null", {"a": b"1", "b": b"\x00\xff"}, map_blocks=2, negative_counts=True) + body
    info = P.container_info(blob)
    assert info.schema == FULL and info.metadata == {"a": b"1", "b": b"\x00\xff"} and info.num_records == 4
    blob = CC.header(FULL, "deflate", {"a": b"1", "b": b"2", "c": b""}, map_blocks=4) + CC.block(recs, "deflate")
    info = P.container_info(blob)
    assert info.codec == "deflate" and info.metadata == {"a": b"1", "b": b"2", "c": b""}
    assert P.container_info(CC.header(FULL, None) + body).codec == "null"           # no avro.codec: null
    # a count-0 block and a file of zero blocks are legal
    info = P.container_info(CC.header(FULL, "null") + CC.block([]) + body + CC.block([]))
    assert (info.num_blocks, info.num_records) == (3, 4)
    info = P.container_info(CC.header(FULL, "null"))
    assert (info.num_blocks, info.num_records) == (0, 0)


def test_malformed_shapes_are_refused():
    recs = CC.records_of("full", 4)
    hdr, body = CC.header(FULL, "null"), CC.block(recs)
    _refused(b"", "truncated header")
    _refused(b"Obj\x02" + hdr[4:] + body, "bad magic")
    _refused(b"PAR1" + b"\x00" * 64, "bad magic")
    _refused(CC.header(None, "null") + body, "avro.schema")
    assert _refused(CC.header(FULL, "snappy") + body) == "container: codec 'snappy' is not supported"
    _refused(CC.header(FULL, "zstandard"), "'zstandard'")
    payload = b"".join(recs)
    _refused(hdr + CC.zz(-4) + CC.zz(len(payload)) + payload + CC.SYNC, "block 0")        # negative count
    _refused(hdr + CC.zz(4) + CC.zz(-1) + payload + CC.SYNC, "block 0")                   # negative size
    _refused(hdr + body + CC.zz(4) + CC.zz(len(payload) + 17) + payload + CC.SYNC, "block 1")      # size past the end of the file
    _refused(hdr + CC.zz(4) + CC.zz(1 << 62) + payload + CC.SYNC, "block 0")
    _refused(hdr + body + CC.block(recs, sync=bytes(16)) + body, "block 1")               # sync mismatch at block 1
    _refused(hdr + body + b"\x00", "block 1")                                             # bytes left after the last complete block
    _refused(hdr + body + body[:-1], "block 1")
    # the metadata map: an entry count or a length that the file cannot hold
    _refused(CC.MAGIC + CC.zz(1 << 40) + hdr[5:], "truncated header")
    _refused(CC.MAGIC + CC.zz(1) + CC.zz(1 << 40) + b"avro.schema", "truncated header")
    _refused(CC.MAGIC + b"\xff" * 11, "truncated header")                                 # a varint that never ends


def test_read_container_refuses_a_malformed_file_before_any_device_work():
    with pytest.raises(ValueError, match="^container: "):
        P.read_container(b"Obj\x01\x00")
    with pytest.raises(ValueError, match="^container: codec 'snappy'"):
        P.read_container(CC.header(FULL, "snappy"))
    with pytest.raises(TypeError):
        P.read_container(12)
    with pytest.raises(TypeError):
        P.read_container(CC.header(FULL, "null"), "2")
    with pytest.raises(ValueError, match="^container: block 1: deflate: "):                # a block that does not inflate
        recs = CC.records_of("full", 4)
        P.read_container(CC.header(FULL, "deflate") + CC.block(recs, "deflate") + CC.zz(4) + CC.zz(5) + b"\xff" * 5 + CC.SYNC)


def test_deflate_blocks_inflate_in_steps_and_up_to_the_block_limit(monkeypatch):
    from pyruhvro_amd import container as CT
    blob, n = _file("full", "ragged", "deflate")
    payloads = [p for _, p in CC.read(blob).blocks]
    monkeypatch.setattr(CT, "_INFLATE_STEP", 7)                        # many steps per block, input left over between them
    buf, info = CT._scan(blob)
    out, start, end = CT._inflate(buf, info)
    assert bytes(out) == b"".join(payloads)
    assert [int(e - s) for s, e in zip(start, end)] == list(map(len, payloads)) and int(end[-1]) == len(out)
    # a block may inflate to less than the limit, never to it: refused at the limit, whatever the stream still holds
    biggest = max(map(len, payloads))
    monkeypatch.setattr(CT, "MAX_BLOCK_BYTES", biggest + 1)
    assert bytes(CT._inflate(buf, info)[0]) == b"".join(payloads)
    monkeypatch.setattr(CT, "MAX_BLOCK_BYTES", biggest)
    b = max(range(len(payloads)), key=lambda i: len(payloads[i]))
    with pytest.raises(ValueError, match=f"^container: block {b}: deflate: it inflates to {biggest} bytes or more"):
        P.read_container(blob)
    # a stream cut short, and bytes behind a stream's end
    recs = CC.records_of("full", 4)
    good = CC.block(recs, "deflate")
    c = zlib.compressobj(wbits=-15)
    body = c.compress(b"".join(recs)) + c.flush()
    assert good == CC.zz(4) + CC.zz(len(body)) + body + CC.SYNC
    for bad, word in ((body[:-3], "ends before its final block"), (body + b"\x00\x01", "2 bytes behind the end")):
        with pytest.raises(ValueError, match="^container: block 1: deflate: .*" + word):
            P.read_container(CC.header(FULL, "deflate") + good + CC.zz(4) + CC.zz(len(bad)) + bad + CC.SYNC)


def test_unchanged_ground():
    for name in ("full", "cfg3", "flat4"):
        assert cabi.kernel_key(SCHEMAS[name]) == PARENT_KEYS[name]
    assert cabi.lib().rh_abi_version() == 7


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(CC.LAYOUTS))
@pytest.mark.parametrize("name", LAYOUT_SCHEMAS)
def test_block_layouts(kernel, name, layout):
    blob, n = _file(name, layout)
    info = P.container_info(blob)
    assert (info.num_blocks, info.num_records) == (len(CC.LAYOUTS[layout]), n)
    for k in (1, 3):
        _same(P.read_container(blob, k), CC.expected(name, n, k))


@pytest.mark.gpu
@pytest.mark.parametrize("name", LAYOUT_SCHEMAS)
def test_both_codecs(kernel, name):
    # null: the file ends right behind a sync marker.  deflate: the inflated blocks are uploaded back to back, so the last
    # record's last byte is the last byte of the buffer -- nothing is readable behind it
    for codec in ("null", "deflate"):
        blob, n = _file(name, "ragged", codec)
        assert P.container_info(blob).codec == codec
        _same(P.read_container(blob, 3), CC.expected(name, n, 3))


@pytest.mark.gpu
def test_block_header_varints(kernel):
    # one block whose count needs a 2-byte varint and whose size needs 3
    n = 300
    recs = CC.records_of("full", n)
    blob = CC.write(FULL, [recs])
    hdr = len(CC.header(FULL, "null"))
    assert len(CC.zz(n)) == 2 and len(CC.zz(sum(map(len, recs)))) == 3
    assert blob[hdr:hdr + 5] == CC.zz(n) + CC.zz(sum(map(len, recs)))
    _same(P.read_container(blob, 2), CC.expected("full", n, 2))


@pytest.mark.gpu
def test_one_150_kb_record_between_small_blocks(kernel):
    small = list(CC.records_of("full", 40))
    v = synth.gen_full(1, 1)
    v["name"] = "n" * 150_000
    big = to_datum(CC.FULL_PARSED, v)
    recs = small[:20] + [big] + small[20:]
    blob = CC.write(FULL, [recs[:7], recs[7:20], [big], recs[21:30], recs[30:]])
    for k in (1, 3):
        _same(P.read_container(blob, k), c_walker.decode_threaded(recs, FULL, k))


@pytest.mark.gpu
def test_composition(kernel):
    blob, n = _file("full", "ragged")
    recs = list(CC.records_of("full", n))
    cols = ["created_at", "name"]
    _same(P.read_container(blob, 3, columns=cols), [b.select(cols) for b in CC.expected("full", n, 3)])
    values = [synth.gen_full(20260921, i) for i in range(n)]
    assert RC.writer_records(FULL, values) == recs
    _same(P.read_container(blob, 3, reader_schema=RC.FULL_MIXED), _oracle(RC.reader_records(FULL, RC.FULL_MIXED, values), RC.FULL_MIXED, 3))
    for kw in ({}, {"columns": cols}):
        dec = P.read_container_to_device(blob, 3, **kw)
        assert [b.num_rows for b in dec.batches] == [b.num_rows for b in CC.expected("full", n, 3)]
        exp = CC.expected("full", n, 3)
        _same(dec.to_host(), exp if not kw else [b.select(cols) for b in exp])
        dec.free()
    dec = P.read_container_to_device(_file("full", "ragged", "deflate")[0], 3, device=0)
    _same(dec.to_host(), CC.expected("full", n, 3))


@pytest.mark.gpu
def test_every_src_type(kernel, tmp_path):
    blob, n = _file("array_and_map", "ragged")
    exp = CC.expected("array_and_map", n, 2)
    path = tmp_path / "ragged.avro"
    path.write_bytes(blob)
    odd = bytearray(b"\x5a" * 3 + blob + b"\xa5" * 5)
    with open(path, "rb") as f:
        mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
    srcs = [str(path), path, mm, bytearray(blob), np.frombuffer(blob, dtype=np.uint8), memoryview(odd)[3:3 + len(blob)], blob]
    for src in srcs:
        assert P.container_info(src).num_records == n
        _same(P.read_container(src, 2), exp)
    mm.close()


def _oracle_message(recs, schema=FULL):
    with pytest.raises(ValueError) as e:
        c_walker.decode_threaded(list(recs), schema, 1)
    return str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(CC.DAMAGE_MESSAGES))
def test_record_errors(kernel, kind):
    recs = list(CC.records_of("full", 200))
    bad = CC.damaged_full(kind, 77)
    recs[77] = bad
    blocks = CC.split(recs, [10, 60, 30, 100])           # record 77 is the 8th of 30 in block 2
    # the precondition, on the oracle alone: the verdict does not depend on where the damaged record ends
    alone = _oracle_message([bad])
    assert alone == CC.DAMAGE_MESSAGES[kind]
    assert _oracle_message([bad + b"".join(recs[78:100])]) == alone
    blob = CC.write(FULL, blocks)
    with pytest.raises(ValueError) as e_list:
        P.deserialize_array_threaded(recs, FULL, 1)
    assert str(e_list.value) == alone
    for codec in ("null", "deflate"):
        with pytest.raises(ValueError) as e:
            P.read_container(CC.write(FULL, blocks, codec), 1)
        assert str(e.value) == str(e_list.value)
    with pytest.raises(ValueError) as e:
        P.read_container_to_device(blob, 2)
    assert str(e.value) == alone
    with pytest.raises(ValueError) as e:                 # the damage is in a dropped field
        P.read_container(blob, 1, columns=["created_at", "name"])
    assert str(e.value) == alone


@pytest.mark.gpu
def test_the_lower_of_two_damaged_records_is_reported(kernel):
    # block 0 holds 150 records and block 1 ten: record 140 (lane 0, its 141st iteration) is met long after record 152
    # (lane 1, its 3rd iteration), and has the lower index.  Then the other way round.
    for lo_kind, hi_kind in (("enum", "bool"), ("union", "enum")):
        recs = list(CC.records_of("full", 200))
        recs[140] = CC.damaged_full(lo_kind, 140)
        recs[152] = CC.damaged_full(hi_kind, 152)
        assert _oracle_message(recs) == CC.DAMAGE_MESSAGES[lo_kind] != CC.DAMAGE_MESSAGES[hi_kind]
        for counts in ([150, 10, 40], [141, 50, 9]):
            with pytest.raises(ValueError) as e:
                P.read_container(CC.write(FULL, CC.split(recs, counts)), 1)
            assert str(e.value) == CC.DAMAGE_MESSAGES[lo_kind]


@pytest.mark.gpu
def test_block_count_errors(kernel):
    recs = list(CC.records_of("full", 60))
    hdr = CC.header(FULL, "null")
    b0, b2 = CC.block(recs[:20]), CC.block(recs[40:])
    mid = recs[20:40]
    size = sum(map(len, mid))
    # one record fewer than the block holds
    blob = hdr + b0 + CC.block(mid, count=19) + b2
    with pytest.raises(ValueError) as e:
        P.read_container(blob, 1)
    assert str(e.value) == f"container: block 1: its 19 records end at byte {size - len(mid[-1])} of {size}"
    # one record more: it raises, in either form
    with pytest.raises(ValueError):
        P.read_container(hdr + b0 + CC.block(mid, count=21) + b2, 1)
    # a record error in a lower record wins over a block error
    bad = list(recs)
    bad[5] = CC.damaged_full("enum", 5)
    with pytest.raises(ValueError) as e:
        P.read_container(hdr + CC.block(bad[:20]) + CC.block(mid, count=19) + b2, 1)
    assert str(e.value) == CC.DAMAGE_MESSAGES["enum"]
    # ... and a block error wins over a record error in a later block
    bad = list(recs)
    bad[45] = CC.damaged_full("enum", 45)
    with pytest.raises(ValueError) as e:
        P.read_container(hdr + b0 + CC.block(mid, count=19) + CC.block(bad[40:]), 1)
    assert str(e.value).startswith("container: block 1: its 19 records end at byte ")
    # an empty block that holds bytes
    with pytest.raises(ValueError, match="^container: block 1: its 0 records end at byte 0 of "):
        P.read_container(hdr + b0 + CC.block(mid[:1], count=0) + b2, 1)
    # a count the block's bytes cannot hold is refused before the kernel runs
    with pytest.raises(ValueError, match="^container: block 1: "):
        P.read_container(hdr + b0 + CC.block(mid, count=1 << 40) + b2, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("codec", ["null", "deflate"])
@pytest.mark.parametrize("block_rows", [1, 3, 4096])
def test_writer(codec, block_rows):
    n = 50
    batch = CC.expected("full", n, 1)[0]
    meta = {"writer": b"test \x00\xff", "note": "text"}
    sync = bytes(range(16))
    blob = P.write_container(batch, FULL, codec=codec, block_rows=block_rows, sync=sync, metadata=meta)
    assert isinstance(blob, bytes)
    got = CC.read(blob)
    assert got.schema == FULL and got.codec == codec and got.sync == sync
    assert got.metadata == {"writer": b"test \x00\xff", "note": b"text"}
    want = P.serialize_record_batch(batch, FULL, 1)[0].to_pylist()
    assert [c for c, _ in got.blocks] == [min(block_rows, n - i) for i in range(0, n, block_rows)]
    at = 0
    for cnt, payload in got.blocks:
        assert payload == b"".join(want[at:at + cnt])
        at += cnt
    assert at == n
    info = P.container_info(blob)
    assert info.metadata == got.metadata and info.schema == FULL and info.codec == codec and info.sync == sync
    assert CC.read(P.write_container(batch.slice(0, 0), FULL, codec=codec)).blocks == []
    assert P.write_container(batch, FULL, sync=sync) != P.write_container(batch, FULL)      # (a random marker by default)


@pytest.mark.gpu
def test_writer_arguments():
    batch = CC.expected("full", 5, 1)[0]
    for kw in ({"codec": "snappy"}, {"block_rows": 0}, {"sync": b"short"}, {"metadata": {"avro.codec": b"x"}}):
        with pytest.raises(ValueError, match="^container: "):
            P.write_container(batch, FULL, **kw)


@pytest.mark.gpu
def test_round_trip(kernel):
    n = 500
    batch = CC.expected("full", n, 1)[0]
    for codec, rows in (("null", 64), ("deflate", 4096)):
        got = P.read_container(P.write_container(batch, FULL, codec=codec, block_rows=rows), 1)
        _same(got, [batch])
