"""Deflate blocks written on the device: ``write_container(..., deflate="device")``, ``rh_deflate_blocks`` and
its host twin.  Expected bytes are those of Python's ``zlib`` (what it inflates a stream to, what it compresses a payload to)
and of the oracle (container_cases.expected), never the engine's.  Many payloads ride as the blocks of ONE rh_deflate_blocks
call."""
import functools
import inspect
import zlib

import numpy as np
import pytest

import container_cases as CC
import deflate_payloads as DP
from avrogen.schemas import SCHEMAS
from test_projection import PARENT_KEYS
from test_resolution import _same

import pyruhvro
import pyruhvro_amd as P
from pyruhvro_amd import cabi
from pyruhvro_amd import container as CT

FULL = SCHEMAS["full"]
NEW_SYMBOLS = ("rh_deflate_blocks", "rh_deflate_blocks_host", "rh_deflate_bound", "rh_deflate_last")
STRATEGIES = (0, 1, 2, 3)      # cabi.DEFLATE_AUTO / STORED / FIXED / DYNAMIC
# The largest of the five ratios (this writer, AUTO) / (zlib level 1), measured with tools/deflate_check --ratio, plus 0.02
# (0.9864, 1.0445, 1.0560, 1.0734 and 1.1838 for text_200000).  The writer is deterministic: the margin is for
# a later retune of the hash, not for noise.
SIZE_C = 1.1838 + 0.02


def _table(payloads):
    lens = np.array([len(p) for p in payloads], dtype=np.uint64)
    end = np.cumsum(lens, dtype=np.uint64)
    return np.frombuffer(b"".join(payloads) or b"\x00", dtype=np.uint8)[:int(lens.sum())], end - lens, end


def _streams(fn, payloads, strategy):
    data, start, end = _table(payloads)
    blob, o_start, o_end = fn(data, start, end, strategy)
    assert len(blob) == (int(o_end[-1]) if len(payloads) else 0)
    assert all(int(o_start[i]) == (int(o_end[i - 1]) if i else 0) for i in range(len(payloads)))      # back to back
    return [blob[int(o_start[i]):int(o_end[i])] for i in range(len(payloads))]


@functools.lru_cache(maxsize=None)
def _host(strategy):
    """every payload x this strategy through rh_deflate_blocks_host, once"""
    return _streams(cabi.deflate_blocks_host, list(DP.payloads().values()), strategy)


def _assert_zlib_reads(streams, strategy):
    for (name, payload), s in zip(DP.payloads().items(), streams):
        d = zlib.decompressobj(-15)
        assert d.decompress(s) == payload, (name, strategy)
        assert d.eof and d.unused_data == b"", (name, strategy)
        assert len(s) <= cabi.deflate_bound(len(payload)), (name, strategy, len(s))


def _zlib_level_1(payload, strategy=zlib.Z_DEFAULT_STRATEGY):
    z = zlib.compressobj(1, zlib.DEFLATED, -15, 8, strategy)
    return len(z.compress(payload) + z.flush())


def _assert_sizes(streams):
    """AUTO: the dynamic code is chosen and works (smaller than zlib's fixed-code output), and the file is one a user wants"""
    by_name = dict(zip(DP.payloads(), streams))
    for name in DP.SIZE_PAYLOADS:
        payload, got = DP.payloads()[name], len(by_name[name])
        fixed, default = _zlib_level_1(payload, zlib.Z_FIXED), _zlib_level_1(payload)
        print(f"{name}: {len(payload)} bytes -> {got}; zlib level 1 {default} (ratio {got / default:.4f}), Z_FIXED {fixed}")
        assert got < fixed, name
        assert got <= SIZE_C * default, name


# ---- CPU --------------------------------------------------------------------------------------------------------------------------
def test_the_deflate_argument_is_validated_before_anything_else(monkeypatch):
    batch = CC.expected("full", 5, 1)[0]
    for fn in (P.write_container, pyruhvro.write_container):
        par = inspect.signature(fn).parameters["deflate"]
        assert par.default is None and par.kind is inspect.Parameter.KEYWORD_ONLY
        for codec in ("null", "deflate"):
            for bad in ("gpu", "", "Device", 1, b"host"):
                with pytest.raises(ValueError) as e:
                    fn(batch, FULL, codec=codec, deflate=bad)
                assert str(e.value) == "container: deflate must be 'host' or 'device'"
    monkeypatch.setenv("RUHVRO_HIP_DEFLATE", "zlib")
    with pytest.raises(ValueError) as e:
        P.write_container(batch, FULL)
    assert str(e.value) == "container: deflate must be 'host' or 'device'"
    # the argument wins over the environment, and either road checks the other arguments before any device work
    for road in ("host", "device"):
        with pytest.raises(ValueError, match="^container: codec 'snappy'"):
            P.write_container(batch, FULL, codec="snappy", deflate=road)
        monkeypatch.setenv("RUHVRO_HIP_DEFLATE", road)
        with pytest.raises(ValueError, match="^container: block_rows"):
            P.write_container(batch, FULL, codec="deflate", block_rows=0)
    monkeypatch.setenv("RUHVRO_HIP_DEFLATE", "")
    assert CT._deflate_road(None) == "host"
    monkeypatch.delenv("RUHVRO_HIP_DEFLATE")
    assert CT._deflate_road(None) == "host" and CT._deflate_road("device") == "device"


def test_new_symbols_and_unchanged_ground():
    for name in NEW_SYMBOLS:
        assert getattr(cabi.lib(), name, None) is not None, name
    for name in ("deflate_blocks", "deflate_blocks_host", "deflate_bound", "deflate_last"):
        assert callable(getattr(cabi, name))
    assert (cabi.DEFLATE_AUTO, cabi.DEFLATE_STORED, cabi.DEFLATE_FIXED, cabi.DEFLATE_DYNAMIC) == (0, 1, 2, 3)
    assert cabi.lib().rh_abi_version() == 7
    for name in ("full", "cfg3", "flat4"):
        assert cabi.kernel_key(SCHEMAS[name]) == PARENT_KEYS[name]


def test_the_bound():
    assert cabi.DEFLATE_SEGMENT == DP.K and 16384 <= DP.K <= 65536
    for n in (0, 1, 5, DP.K - 1, DP.K, DP.K + 1, 65535, 65536, 3 * DP.K + 5, 10**6, (1 << 32) - 17):
        assert n < cabi.deflate_bound(n) <= n + 16 * (n // 32768 + 1), n
    # one marker and one stored header more for every segment begun
    assert cabi.deflate_bound(DP.K + 1) - cabi.deflate_bound(DP.K) == 11


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_the_host_form_writes_streams_zlib_reads(strategy):
    streams = _host(strategy)
    _assert_zlib_reads(streams, strategy)
    by_name = dict(zip(DP.payloads(), streams))
    # an empty payload is one valid final block: zlib's own `03 00` where the fixed code may be chosen (a dynamic header alone is
    # larger than the slot of an empty segment, so DYNAMIC writes it stored)
    assert by_name["len_0"] == (b"\x03\x00" if strategy in (cabi.DEFLATE_AUTO, cabi.DEFLATE_FIXED) else b"\x01\x00\x00\xff\xff")
    first_type = {name: (s[0] >> 1) & 3 for name, s in by_name.items()}
    if strategy == cabi.DEFLATE_STORED:
        assert set(first_type.values()) == {0}
    if strategy == cabi.DEFLATE_FIXED:
        assert first_type["full"] == 1 and first_type["noise_65536"] == 0      # (noise under the fixed code would pass the bound)
    if strategy == cabi.DEFLATE_DYNAMIC:
        assert first_type["full"] == 2 and first_type["ab_130"] == 2 and first_type["zeros"] == 2
    if strategy == cabi.DEFLATE_AUTO:
        assert first_type["full"] == 2 and first_type["noise_65536"] == 0
        # every segment but the last ends with the marker: the joints of a three-segment payload are where the bound allows
        assert by_name["noise_65537"].count(b"\x00\x00\xff\xff") >= 2
        _assert_sizes(streams)


def test_a_bad_table_is_refused_before_anything_else():
    data = np.zeros(10, dtype=np.uint8)
    for fn in (cabi.deflate_blocks_host, cabi.deflate_blocks):      # (the device call checks its table before it looks for a device)
        for start, end in (([5], [3]), ([0], [11]), ([0, 4], [6, 8])):
            with pytest.raises(ValueError, match="^container: block [01]: its bytes are outside the buffer or out of order$"):
                fn(data, np.array(start, dtype=np.uint64), np.array(end, dtype=np.uint64))
        with pytest.raises(ValueError, match="^container: deflate strategy 4"):
            fn(data, np.array([0], dtype=np.uint64), np.array([10], dtype=np.uint64), 4)
        with pytest.raises(ValueError, match="as many starts as ends"):
            fn(data, np.array([0], dtype=np.uint64), np.array([], dtype=np.uint64))
    assert _streams(cabi.deflate_blocks_host, [], 0) == []


# ---- GPU: the deflate step alone ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_the_kernels_write_the_host_forms_bytes(strategy):
    payloads = list(DP.payloads().values())
    got = _streams(cabi.deflate_blocks, payloads, strategy)
    want = _host(strategy)
    for name, g, w in zip(DP.payloads(), got, want):
        assert g == w, (name, strategy, len(g), len(w))
    assert _streams(cabi.deflate_blocks, payloads, strategy) == got      # and again
    _assert_zlib_reads(got, strategy)
    data, start, end = _table(got)
    out, o_start, o_end, status = cabi.inflate_blocks(data, start, end)
    assert not status["code"].any(), (strategy, status["code"].nonzero())
    for i, (name, payload) in enumerate(DP.payloads().items()):
        assert out[int(o_start[i]):int(o_end[i])] == payload, (name, strategy)
    if strategy == cabi.DEFLATE_AUTO:
        _assert_sizes(got)
        last = cabi.deflate_last()
        assert last["in_bytes"] == sum(map(len, payloads)) and last["out_bytes"] == sum(map(len, got))
        assert last["deflate_ms"] > 0 and last["gather_ms"] > 0
    assert _streams(cabi.deflate_blocks, [], strategy) == []


# ---- GPU: through write_container --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("block_rows", [1, 3, 4096])
def test_writer(block_rows, monkeypatch):
    n = 300
    batch = CC.expected("full", n, 1)[0]
    sync = bytes(range(16, 32))
    meta = {"writer": b"test \x00\xff"}
    kw = dict(codec="deflate", block_rows=block_rows, sync=sync, metadata=meta)
    host = P.write_container(batch, FULL, **kw)
    null = P.write_container(batch, FULL, block_rows=block_rows, sync=sync)

    def no_zlib(*a, **k):
        raise AssertionError("the device road called the host's deflate")
    monkeypatch.setattr(CT.zlib, "compressobj", no_zlib)
    blob = P.write_container(batch, FULL, deflate="device", **kw)
    assert isinstance(blob, bytes)
    got, want = CC.read(blob), CC.read(host)
    assert (got.schema, got.codec, got.sync, got.metadata) == (want.schema, want.codec, want.sync, want.metadata) == (FULL, "deflate", sync, meta)
    assert [c for c, _ in got.blocks] == [min(block_rows, n - i) for i in range(0, n, block_rows)]
    assert got.blocks == want.blocks
    info = P.container_info(blob)
    last = cabi.deflate_last()
    assert last["in_bytes"] == sum(len(p) for _, p in got.blocks) and last["out_bytes"] == int((info._end - info._start).sum())
    assert last["deflate_ms"] > 0 and last["gather_ms"] > 0
    for road in ("host", "device"):
        _same(P.read_container(blob, 1, inflate=road), [batch])
    # the environment alone selects the road; the argument wins over it
    monkeypatch.setenv("RUHVRO_HIP_DEFLATE", "device")
    assert pyruhvro.write_container(batch, FULL, **kw) == blob
    with pytest.raises(AssertionError):
        P.write_container(batch, FULL, deflate="host", **kw)
    # codec="null": the argument changes nothing; an empty batch writes no block
    assert P.write_container(batch, FULL, block_rows=block_rows, sync=sync, deflate="device") == null
    monkeypatch.delenv("RUHVRO_HIP_DEFLATE")
    assert P.write_container(batch, FULL, block_rows=block_rows, sync=sync, deflate="device") == null
    empty = P.write_container(batch.slice(0, 0), FULL, codec="deflate", deflate="device", sync=sync)
    assert CC.read(empty).blocks == [] and empty == P.write_container(batch.slice(0, 0), FULL, codec="deflate", deflate="host", sync=sync)
