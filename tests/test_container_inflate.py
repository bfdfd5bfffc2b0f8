"""Deflate blocks inflated on the device: ``read_container(..., inflate="device")``, ``rh_decode_cblocks`` and
``rh_inflate_blocks``.  Expected bytes and verdicts are those of Python's ``zlib`` (deflate_cases.classify) and of the oracle
(container_cases.expected), never the engine's.  Many streams ride as the blocks of ONE rh_inflate_blocks call."""
import inspect
import zlib

import numpy as np
import pytest

import container_cases as CC
import deflate_cases as DC
import resolve_cases as RC
from avrogen import synth
from avrogen.schemas import SCHEMAS
from test_projection import PARENT_KEYS
from test_resolution import _oracle, _same

import pyruhvro
import pyruhvro_amd as P
from pyruhvro_amd import cabi
from pyruhvro_amd import container as CT

FULL = SCHEMAS["full"]
LAYOUT_SCHEMAS = ("full", "array_and_map", "t_union", "nullable_primitives")
NEW_SYMBOLS = ("rh_decode_cblocks", "rh_decode_cblocks_device", "rh_inflate_blocks", "rh_inflate_last")


def _file(name, layout, **kw):
    counts = CC.LAYOUTS[layout]
    return CC.write(SCHEMAS[name], CC.split(CC.records_of(name, sum(counts)), counts), "deflate", **kw), sum(counts)


def _raw_block(count, payload):
    """a container block around a payload that is taken as it is"""
    return CC.zz(count) + CC.zz(len(payload)) + payload + CC.SYNC


# ---- CPU --------------------------------------------------------------------------------------------------------------------------
def test_the_inflate_argument_is_validated_before_anything_else(monkeypatch):
    null_file = CC.header(FULL, "null")
    for blob in (null_file, CC.header(FULL, "deflate"), b"Obj\x01\x00"):
        for fn in (P.read_container, P.read_container_to_device, pyruhvro.read_container):
            for bad in ("gpu", "", "Device", 1, b"host"):
                with pytest.raises(ValueError) as e:
                    fn(blob, 1, inflate=bad)
                assert str(e.value) == "container: inflate must be 'host' or 'device'"
    monkeypatch.setenv("RUHVRO_HIP_INFLATE", "zlib")
    with pytest.raises(ValueError) as e:
        P.read_container(null_file)
    assert str(e.value) == "container: inflate must be 'host' or 'device'"
    # the argument wins over the environment, and either road scans the file before any device work
    for road in ("host", "device"):
        with pytest.raises(ValueError, match="^container: codec 'snappy'"):
            P.read_container(CC.header(FULL, "snappy"), inflate=road)
        monkeypatch.setenv("RUHVRO_HIP_INFLATE", road)
        with pytest.raises(ValueError, match="^container: (?!inflate)"):
            P.read_container(b"Obj\x01\x00")
        with pytest.raises(TypeError):
            P.read_container(null_file, "2")
    monkeypatch.setenv("RUHVRO_HIP_INFLATE", "")
    assert CT._inflate_road(None) == "host"
    monkeypatch.delenv("RUHVRO_HIP_INFLATE")
    assert CT._inflate_road(None) == "host" and CT._inflate_road("device") == "device"
    for fn in (P.read_container, P.read_container_to_device, pyruhvro.read_container, pyruhvro.read_container_to_device):
        par = inspect.signature(fn).parameters["inflate"]
        assert par.default is None and par.kind is inspect.Parameter.KEYWORD_ONLY


def test_new_symbols_and_unchanged_ground():
    for name in NEW_SYMBOLS:
        assert getattr(cabi.lib(), name, None) is not None, name
    for name in ("decode_cblocks", "decode_cblocks_device", "inflate_blocks", "inflate_last"):
        assert callable(getattr(cabi, name))
    assert (cabi.CODEC_NULL, cabi.CODEC_DEFLATE) == (0, 1)
    assert cabi.lib().rh_abi_version() == 7
    for name in ("full", "cfg3", "flat4"):
        assert cabi.kernel_key(SCHEMAS[name]) == PARENT_KEYS[name]


# ---- GPU: the inflate step alone ---------------------------------------------------------------------------------------------------
def _inflate_all(streams, **kw):
    """every stream as one block of one rh_inflate_blocks call -> per stream (code, bytes, detail)"""
    lens = np.array([len(s) for s in streams], dtype=np.uint64)
    end = np.cumsum(lens, dtype=np.uint64)
    start = end - lens
    out, o_start, o_end, status = cabi.inflate_blocks(np.frombuffer(b"".join(streams), dtype=np.uint8), start, end, **kw)
    assert len(out) == (int(o_end[-1]) if len(streams) else 0)
    return [(int(status["code"][i]), out[int(o_start[i]):int(o_end[i])], int(status["detail"][i]), int(status["reason"][i])) for i in range(len(streams))]


def _assert_as_zlib(streams, labels=None):
    got = _inflate_all(streams)
    seen = {}
    for i, (s, (code, data, detail, reason)) in enumerate(zip(streams, got)):
        what = labels[i] if labels else f"stream {i}"
        z_code, z_data, z_trailing = DC.classify(s)
        seen[z_code] = seen.get(z_code, 0) + 1
        assert code == z_code, (what, code, reason, z_code)
        if z_code == DC.OK:
            assert data == z_data, what
        else:
            assert data == b"", what      # a failing block contributes no byte
        if z_code == DC.TRAILING:
            assert detail == z_trailing, what
        if z_code == DC.MALFORMED:
            assert 1 <= reason <= 11, what
    return seen


@pytest.mark.gpu
def test_hand_assembled_streams():
    names = sorted(DC.HAND)
    for n in names:      # the precondition, on zlib alone: every one is a whole stream
        assert DC.classify(DC.HAND[n])[0] == DC.OK, n
    assert len(DC.classify(DC.HAND["stored_65535"])[1]) == 65535 and DC.classify(DC.HAND["stored_0"])[1] == b""
    far = DC.classify(DC.HAND["stored_32768_then_258_at_32768"])[1]
    assert len(far) == 32768 + 258 and far[32768:] == far[:258]
    assert DC.classify(DC.HAND["258_as_symbol_284"])[1] == DC.classify(DC.HAND["258_as_symbol_285"])[1] == b"ab" * 130
    assert _assert_as_zlib([DC.HAND[n] for n in names], names) == {DC.OK: len(names)}


@pytest.mark.gpu
def test_zlib_made_streams():
    twice, thrice = DC.noise(40_000, 3), DC.noise(30_000, 5)
    payloads = {name: b"".join(CC.records_of(name, 200)) for name in LAYOUT_SCHEMAS}
    # thrice: matches 30,000 back (a piece written 40,000 back is out of deflate's reach), and 90,000 bytes pass a 32 KiB history twice
    payloads.update({"zeros": bytes(100_000), "noise": DC.noise(70_000, 4), "twice": twice + twice, "thrice": thrice * 3})
    made = DC.zlib_made(payloads)
    assert len(made) == 8 * 16
    assert len([s for label, s, _ in made if label == "noise/0/default"][0]) == 70_000 + 2 * 5      # two stored blocks
    assert len([s for label, s, _ in made if label == "thrice/9/default"][0]) < 32_000             # the second and third piece are matches
    for label, s, p in made:
        assert DC.classify(s) == (DC.OK, p, 0), label
    assert _assert_as_zlib([s for _, s, _ in made], [label for label, _, _ in made]) == {DC.OK: len(made)}


@pytest.mark.gpu
def test_damage_every_flip_and_every_prefix():
    z = zlib.compressobj(9, zlib.DEFLATED, -15)
    stream = z.compress(b"".join(CC.records_of("array_and_map", 20))) + z.flush()
    assert (stream[0] & 7) == 5      # one final dynamic block
    flips, prefixes, of_refused = DC.damage_cases(stream)
    assert len(flips) == 8 * len(stream) and len(prefixes) == len(stream)
    # the preconditions, on zlib alone
    classes = [DC.classify(f)[0] for f in flips]
    assert all(classes.count(c) > 0 for c in (DC.OK, DC.MALFORMED, DC.TRUNCATED, DC.TRAILING)), [classes.count(c) for c in range(4)]
    assert all(DC.classify(p)[0] == DC.TRUNCATED for p in prefixes)
    assert len(of_refused) >= 12 * (len(stream) - 1)
    seen = _assert_as_zlib(flips + prefixes + of_refused)
    assert sum(seen.values()) == len(flips) + len(prefixes) + len(of_refused)      # no case left out


@pytest.mark.gpu
def test_the_limit_of_the_inflate_step():
    streams = [DC.HAND["stored_65535"], DC.HAND["258_at_distance_1"], DC.HAND["stored_0"]]
    sizes = [len(DC.classify(s)[1]) for s in streams]
    assert sizes == [65535, 520, 0]
    assert [g[0] for g in _inflate_all(streams, max_block_bytes=65536)] == [DC.OK] * 3
    got = _inflate_all(streams, max_block_bytes=65535)
    assert [g[0] for g in got] == [DC.TOO_LARGE, DC.OK, DC.OK] and got[0][2] == 65535 and got[0][1] == b""
    assert [g[0] for g in _inflate_all(streams, max_block_bytes=520)] == [DC.TOO_LARGE, DC.TOO_LARGE, DC.OK]
    assert _inflate_all([]) == []


# ---- GPU: through read_container ---------------------------------------------------------------------------------------------------
@pytest.fixture(params=["generic", "specialized"])
def kernel(request):
    old = P.set_kernel_mode(request.param)
    yield request.param
    P.set_kernel_mode(old)


def _layouts(name, layout):
    blob, n = _file(name, layout)
    info = P.container_info(blob)
    assert (info.codec, info.num_blocks, info.num_records) == ("deflate", len(CC.LAYOUTS[layout]), n)
    for k in (1, 3):
        _same(P.read_container(blob, k, inflate="device"), CC.expected(name, n, k))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(CC.LAYOUTS))
def test_block_layouts_full(kernel, layout):
    _layouts("full", layout)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(CC.LAYOUTS))
@pytest.mark.parametrize("name", LAYOUT_SCHEMAS[1:])
def test_block_layouts(name, layout):
    _layouts(name, layout)


def _message(blob, **kw):
    with pytest.raises(ValueError) as e:
        P.read_container(blob, 1, **kw)
    return str(e.value)


@pytest.mark.gpu
def test_deflate_errors_name_the_lowest_block_and_come_first():
    recs = list(CC.records_of("full", 40))
    hdr = CC.header(FULL, "deflate")
    good = [CC.block(recs[i:i + 10], "deflate") for i in (0, 10, 20, 30)]
    z = zlib.compressobj(wbits=-15)
    body = z.compress(b"".join(recs[10:20])) + z.flush()
    cut, behind, type3 = _raw_block(10, body[:-3]), _raw_block(10, body + b"\x00\x01"), _raw_block(10, b"\xff" * 5)
    # the three messages the host road words: the same words, from zlib's own verdict
    for bad, words in ((cut, "the stream ends before its final block"), (behind, "2 bytes behind the end of the stream")):
        blob = hdr + good[0] + bad + good[2] + good[3]
        assert _message(blob, inflate="host") == f"container: block 1: deflate: {words}"
        assert _message(blob, inflate="device") == f"container: block 1: deflate: {words}"
    # a malformed stream: our reason behind the same prefix
    blob = hdr + good[0] + good[1] + type3 + good[3]
    assert _message(blob, inflate="host").startswith("container: block 2: deflate: ")
    assert _message(blob, inflate="device") == "container: block 2: deflate: block type 3"
    # of two damaged blocks the lower is named, whichever kind it is
    assert _message(hdr + good[0] + cut + type3 + good[3], inflate="device") == "container: block 1: deflate: the stream ends before its final block"
    assert _message(hdr + type3 + good[1] + good[2] + cut, inflate="device") == "container: block 0: deflate: block type 3"
    # ... even when an earlier block holds a malformed record: every block is inflated before any record is walked
    bad_recs = list(recs)
    bad_recs[3] = CC.damaged_full("enum", 3)
    for road in ("host", "device"):
        assert _message(hdr + CC.block(bad_recs[:10], "deflate") + good[1] + behind + good[3], inflate=road) == \
            "container: block 2: deflate: 2 bytes behind the end of the stream"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(CC.DAMAGE_MESSAGES))
def test_record_errors(kernel, kind):
    recs = list(CC.records_of("full", 200))
    recs[77] = CC.damaged_full(kind, 77)
    blob = CC.write(FULL, CC.split(recs, [10, 60, 30, 100]), "deflate")
    with pytest.raises(ValueError) as e_list:
        P.deserialize_array_threaded(recs, FULL, 1)
    assert str(e_list.value) == CC.DAMAGE_MESSAGES[kind]
    assert _message(blob, inflate="device") == CC.DAMAGE_MESSAGES[kind]
    with pytest.raises(ValueError) as e:
        P.read_container_to_device(blob, 2, inflate="device")
    assert str(e.value) == CC.DAMAGE_MESSAGES[kind]


@pytest.mark.gpu
def test_the_block_limit_and_the_header_count(monkeypatch):
    blob, n = _file("full", "ragged")
    payloads = [p for _, p in CC.read(blob).blocks]
    biggest = max(map(len, payloads))
    monkeypatch.setattr(CT, "MAX_BLOCK_BYTES", biggest + 1)
    _same(P.read_container(blob, 2, inflate="device"), CC.expected("full", n, 2))
    monkeypatch.setattr(CT, "MAX_BLOCK_BYTES", biggest)
    b = max(range(len(payloads)), key=lambda i: len(payloads[i]))
    words = f"container: block {b}: deflate: it inflates to {biggest} bytes or more (a block of 4 GiB - 16 bytes or more is not supported)"
    assert _message(blob, inflate="host") == words
    assert _message(blob, inflate="device") == words
    monkeypatch.undo()
    # a header count that the inflated bytes cannot hold
    recs = list(CC.records_of("full", 60))
    hdr = CC.header(FULL, "deflate")
    mid = recs[20:40]
    blob = hdr + CC.block(recs[:20], "deflate") + CC.block(mid, "deflate", count=1 << 40) + CC.block(recs[40:], "deflate")
    size = sum(map(len, mid))
    assert _message(blob, inflate="device") == f"container: block 1: {1 << 40} records cannot be in its {size} bytes"
    assert _message(blob, inflate="host") == _message(blob, inflate="device")
    # one record fewer than the block holds: the split's own verdict, on the inflated bytes
    blob = hdr + CC.block(recs[:20], "deflate") + CC.block(mid, "deflate", count=19) + CC.block(recs[40:], "deflate")
    assert _message(blob, inflate="device") == f"container: block 1: its 19 records end at byte {size - len(mid[-1])} of {size}"


@pytest.mark.gpu
def test_composition(kernel, monkeypatch):
    blob, n = _file("full", "ragged")
    info = P.container_info(blob)
    payloads = [p for _, p in CC.read(blob).blocks]
    exp = CC.expected("full", n, 3)

    def no_zlib(*a, **kw):
        raise AssertionError("the device road called the host's inflate")
    monkeypatch.setattr(CT, "_inflate", no_zlib)
    monkeypatch.setattr(CT.zlib, "decompressobj", no_zlib)
    _same(P.read_container(blob, 3, inflate="device"), exp)
    last = cabi.inflate_last()
    assert last["out_bytes"] == sum(map(len, payloads))
    assert last["in_bytes"] == int((info._end - info._start).sum())
    assert last["size_ms"] > 0 and last["emit_ms"] > 0
    cols = ["created_at", "name"]
    _same(P.read_container(blob, 3, columns=cols, inflate="device"), [b.select(cols) for b in exp])
    values = [synth.gen_full(20260921, i) for i in range(n)]
    assert RC.writer_records(FULL, values) == list(CC.records_of("full", n))
    _same(P.read_container(blob, 3, reader_schema=RC.FULL_MIXED, inflate="device"),
          _oracle(RC.reader_records(FULL, RC.FULL_MIXED, values), RC.FULL_MIXED, 3))
    for kw in ({}, {"columns": cols}):
        dec = P.read_container_to_device(blob, 3, inflate="device", **kw)
        assert [b.num_rows for b in dec.batches] == [b.num_rows for b in exp]
        _same(dec.to_host(), exp if not kw else [b.select(cols) for b in exp])
        dec.free()
    # the environment chooses the road of a call that does not
    monkeypatch.setenv("RUHVRO_HIP_INFLATE", "device")
    _same(pyruhvro.read_container(blob, 3), exp)
    with pytest.raises(AssertionError):
        P.read_container(blob, 3, inflate="host")
    # a null file: the argument changes nothing
    null_blob = CC.write(FULL, CC.split(CC.records_of("full", n), CC.LAYOUTS["ragged"]))
    _same(P.read_container(null_blob, 3, inflate="device"), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("block_rows", [1, 3, 4096])
def test_writer_round_trip(block_rows):
    n = 300
    batch = CC.expected("full", n, 1)[0]
    blob = P.write_container(batch, FULL, codec="deflate", block_rows=block_rows)
    assert P.container_info(blob).codec == "deflate" and P.container_info(blob).num_blocks == -(-n // block_rows)
    _same(P.read_container(blob, 1, inflate="device"), [batch])


@pytest.mark.gpu
def test_the_c_entry_point_takes_both_codecs():
    blob, n = _file("array_and_map", "ragged")
    info = P.container_info(blob)
    buf = np.frombuffer(blob, dtype=np.uint8)
    exp = CC.expected("array_and_map", n, 2)
    _same(cabi.decode_cblocks(buf, info._start, info._end, info._first, info.schema, 2, cabi.CODEC_DEFLATE), exp)
    inflated, start, end = CT._inflate(buf, info)
    _same(cabi.decode_cblocks(inflated, start, end, info._first, info.schema, 2, cabi.CODEC_NULL), exp)
    with pytest.raises(ValueError, match="codec must be"):
        cabi.decode_cblocks(buf, info._start, info._end, info._first, info.schema, 2, 2)
