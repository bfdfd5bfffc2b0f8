"""Avro object container files (``.avro``): read them on the GPU, write them around the GPU encoder.

    info = pyruhvro.container_info("events.avro")                   # header + block table, no device work
    batches = pyruhvro.read_container("events.avro", 8)              # == deserialize_array_threaded(records_of(file), info.schema, 8)
    dec = pyruhvro.read_container_to_device(buf, 8)                  # as deserialize_to_device
    blob = pyruhvro.write_container(batch, schema, codec="deflate")  # bytes
    batches = pyruhvro.read_container_where("events.avro", ("age", ">=", 30), 8)   # only the matching records
    mask = pyruhvro.filter_container("events.avro", ("age", ">=", 30))             # numpy bool[num_records]

A container block says "N records, M bytes" and nothing says where record j starts.  The file is uploaded as it is and a
split kernel -- one lane per block -- walks the records with the writer's schema (the file's own, from its header) to find
their offsets; the ordinary decode then runs on them.  ``columns=`` and ``reader_schema=`` mean what they mean for
``deserialize_array_threaded``.  Codecs: ``null`` and ``deflate``; anything else is refused.  A ``deflate`` file is inflated
either here with ``zlib``, block by block, into one buffer (``inflate="host"``, the default), or on the device: the
compressed file is uploaded as it is and two kernels inflate its blocks, one wavefront per block (``inflate="device"``, or
``RUHVRO_HIP_INFLATE=device`` in the environment).  Both roads accept the same streams and raise the same messages.
``write_container(..., codec="deflate", deflate="device")`` (or ``RUHVRO_HIP_DEFLATE=device``) compresses the blocks on the
device as well, 32 KiB segments in parallel; the default ``"host"`` is ``zlib`` on the calling thread.

    batches, errors = pyruhvro.read_container_tolerant("events.avro", 8)   # what a damaged file still holds, and what it lost

The ``*_tolerant`` functions of the record lists do not take containers -- a malformed record loses its block's boundaries, so
there is nothing to put a placeholder into.  ``read_container_tolerant`` / ``read_container_to_device_tolerant`` salvage at the
granularity the format provides instead: every sound block is kept, the records in front of a malformed one
are kept, the read resynchronises on the file's sync marker where a block cannot be framed, and every loss is reported as a
``BlockError``.
"""
from __future__ import annotations

import os
import zlib
from collections import namedtuple
from typing import Dict, Optional

MAGIC = b"Obj\x01"
MAX_BLOCK_BYTES = 0xFFFFFFF0      # the engine refuses a block of 4 GiB - 16 bytes or more; a deflate block is not inflated past it
_INFLATE_STEP = 16 << 20


class ContainerInfo:
    """Header and block table of a container: ``schema`` (the writer's, str), ``codec``, ``sync`` (16 bytes), ``metadata``
    (the header's other entries, ``dict[str, bytes]``), ``num_blocks``, ``num_records``."""

    def __init__(self, scan: dict):
        self.schema: str = scan["schema"]
        self.codec: str = scan["codec"]
        self.sync: bytes = scan["sync"]
        self.metadata: Dict[str, bytes] = scan["metadata"]
        self._start, self._end, self._first = scan["start"], scan["end"], scan["first"]
        self.num_blocks: int = len(self._start)
        self.num_records: int = int(self._first[-1])

    def __repr__(self):
        return f"ContainerInfo({self.num_records} records in {self.num_blocks} blocks, codec {self.codec!r})"


def _bytes_of(src):
    """`src` -> a uint8 numpy array over its bytes (no copy).  A str / os.PathLike is a path: the file is mapped."""
    import numpy as np
    if isinstance(src, (str, os.PathLike)):
        import mmap
        with open(src, "rb") as f:
            if os.fstat(f.fileno()).st_size == 0:
                return np.zeros(0, dtype=np.uint8)
            src = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)      # (the mapping outlives the descriptor)
    try:
        mv = memoryview(src)
    except TypeError:
        raise TypeError("argument 'src': expected a bytes-like object or a path") from None
    if not mv.c_contiguous:
        raise TypeError("argument 'src': expected a contiguous buffer")
    return np.frombuffer(mv, dtype=np.uint8) if mv.nbytes else np.zeros(0, dtype=np.uint8)


def _scan(src):
    from . import cabi
    buf = _bytes_of(src)
    return buf, ContainerInfo(cabi.container_scan(buf))


def container_info(src) -> ContainerInfo:
    """The header and the block table of the container in ``src`` (any buffer-protocol object, or a path).  Raises
    ``ValueError`` starting with ``container: `` for a malformed file, before any device work."""
    return _scan(src)[1]


def _inflate_block(mv, b: int, lo: int, hi: int, out: bytearray) -> None:
    """Block b, the raw deflate stream mv[lo:hi], inflated onto `out` in steps.  A stream that is refused raises the
    ValueError of the strict read; `out` then holds a part of the block, which the caller cuts off."""
    d = zlib.decompressobj(-15)
    at = len(out)
    data = mv[lo:hi]
    try:
        while not d.eof:
            piece = d.decompress(data, min(_INFLATE_STEP, MAX_BLOCK_BYTES - (len(out) - at)))
            if not piece and not d.unconsumed_tail and not d.eof:
                raise ValueError(f"container: block {b}: deflate: the stream ends before its final block")
            out += piece
            if len(out) - at >= MAX_BLOCK_BYTES:
                raise ValueError(f"container: block {b}: deflate: it inflates to {MAX_BLOCK_BYTES} bytes or more "
                                 "(a block of 4 GiB - 16 bytes or more is not supported)")
            data = d.unconsumed_tail
    except zlib.error as e:
        raise ValueError(f"container: block {b}: deflate: {e}") from None
    if d.unused_data:
        raise ValueError(f"container: block {b}: deflate: {len(d.unused_data)} bytes behind the end of the stream")


def _inflate(buf, info: ContainerInfo, errors=None):
    """A deflate container -> (one buffer of its inflated blocks back to back, the new starts and ends).  `errors`: a dict
    that takes {block: message} for the streams that are refused -- such a block is empty -- instead of the first one raising."""
    import numpy as np
    mv = memoryview(buf)
    out = bytearray()      # every block inflates straight into it, in steps: no second copy, and no block past the limit
    start = np.zeros(info.num_blocks, dtype=np.uint64)
    end = np.zeros(info.num_blocks, dtype=np.uint64)
    for b in range(info.num_blocks):
        at = len(out)
        if errors is None:
            _inflate_block(mv, b, int(info._start[b]), int(info._end[b]), out)
        elif b not in errors:      # (a block that is dropped already is not inflated)
            try:
                _inflate_block(mv, b, int(info._start[b]), int(info._end[b]), out)
            except ValueError as e:
                errors[b] = str(e)
                del out[at:]
        start[b], end[b] = at, len(out)
    return np.frombuffer(out, dtype=np.uint8) if out else np.zeros(0, dtype=np.uint8), start, end


def _inflate_road(inflate) -> str:
    """``inflate=`` of a read: "host" or "device"; None reads RUHVRO_HIP_INFLATE (per call) and falls back to "host"."""
    if inflate is None:
        inflate = os.environ.get("RUHVRO_HIP_INFLATE") or "host"
    if inflate not in ("host", "device"):
        raise ValueError("container: inflate must be 'host' or 'device'")
    return inflate


def _blocks(src, num_chunks, columns, reader_schema, inflate=None):
    """-> (info, buf, start, end, on_device): on_device = the blocks are still deflated, for the device to inflate."""
    import pyruhvro_amd as P
    road = _inflate_road(inflate)                            # ValueError before any device work, for a `null` file too
    P._check_chunks(num_chunks)
    buf, info = _scan(src)                                   # ValueError "container: ..." before any device work
    P._get_schema(info.schema, columns, reader_schema)       # ValueError on a schema outside the decoder's subset, like every entry point
    if info.codec == "deflate" and road == "device":
        return info, buf, info._start, info._end, True
    if info.codec == "deflate":
        buf, start, end = _inflate(buf, info)
    else:
        start, end = info._start, info._end
    return info, buf, start, end, False


def read_container(src, num_chunks=1, *, columns=None, reader_schema=None, inflate=None):
    """Extension.  The records of the Avro object container ``src`` (a buffer-protocol object -- ``bytes``, ``bytearray``,
    ``memoryview``, ``mmap``, a numpy ``uint8`` array -- or a ``str`` / ``os.PathLike`` path, which is mapped) decoded into
    ``list[pyarrow.RecordBatch]``: exactly ``deserialize_array_threaded(records, info.schema, num_chunks, ...)`` over the
    file's records, without splitting them on the CPU.  The writer schema is the file's.  A malformed record raises what that
    call raises for it; a malformed file raises ``ValueError`` starting with ``container: ``.  ``inflate``: where a ``deflate``
    file's blocks are inflated -- ``"host"`` (``zlib``), ``"device"`` (the GPU), ``None`` = ``RUHVRO_HIP_INFLATE`` or ``"host"``."""
    import pyruhvro_amd as P
    from . import cabi
    info, buf, start, end, on_device = _blocks(src, num_chunks, columns, reader_schema, inflate)
    if on_device:
        return cabi.decode_cblocks(buf, start, end, info._first, info.schema, num_chunks, cabi.CODEC_DEFLATE, MAX_BLOCK_BYTES,
                                   kernel=P._kernel_mode, columns=columns, reader_schema=reader_schema)
    return cabi.decode_blocks(buf, start, end, info._first, info.schema, num_chunks, kernel=P._kernel_mode, columns=columns,
                              reader_schema=reader_schema)


def read_container_to_device(src, num_chunks=1, device: int = -1, *, columns=None, reader_schema=None, inflate=None):
    """Extension.  ``read_container`` with the Arrow buffers left in HBM: a ``DeviceDecode`` as ``deserialize_to_device``
    returns (``.batches``, ``.to_host()``, every buffer a DLPack producer)."""
    import pyruhvro_amd as P
    from . import cabi
    from .device import DeviceDecode
    info, buf, start, end, on_device = _blocks(src, num_chunks, columns, reader_schema, inflate)
    if on_device:
        r = cabi.decode_cblocks_device(buf, start, end, info._first, info.schema, num_chunks, cabi.CODEC_DEFLATE, MAX_BLOCK_BYTES,
                                       device=device, kernel=P._kernel_mode, columns=columns, reader_schema=reader_schema)
    else:
        r = cabi.decode_blocks_device(buf, start, end, info._first, info.schema, num_chunks, device=device, kernel=P._kernel_mode,
                                      columns=columns, reader_schema=reader_schema)
    return DeviceDecode(r, cabi.Schema.get(info.schema, columns, reader_schema).arrow_schema)


def _blocks_where(src, where, num_chunks, columns, reader_schema, inflate):
    """`_blocks`, then the predicate compiled against the file's writer schema: TypeError for a `where` that is no tuple or list,
    ValueError "where: ..." for what rh_filter_compile refuses -- behind the file's own errors, before any device work."""
    from . import cabi
    out = _blocks(src, num_chunks, columns, reader_schema, inflate)
    if cabi.check_where(where) is None:
        raise TypeError("argument 'where': expected a term (name, op, value) or a list of terms")
    cabi.Filter.get(out[0].schema, where)
    return out


def read_container_where(src, where, num_chunks=1, *, columns=None, reader_schema=None, inflate=None):
    """Extension.  ``read_container`` of the records that match a predicate: exactly ``deserialize_array_threaded([r for r in
    records if keep(r)], info.schema, num_chunks, ...)`` over the file's records, in file order.  ``where`` is what
    ``deserialize_array``'s ``where=`` takes -- a term ``(name, op, value)`` or a list of up to 8, ANDed -- and names top-level
    fields of the file's writer schema, whether or not ``columns`` / ``reader_schema`` build them.  The records are chosen in
    the walk that finds their offsets, before anything is decoded; the chunking applies to the kept records,
    and nothing kept gives what a decode of the empty list gives.  A malformed record or block raises what ``read_container``
    raises for the file, whether or not the record would have matched."""
    import pyruhvro_amd as P
    from . import cabi
    info, buf, start, end, on_device = _blocks_where(src, where, num_chunks, columns, reader_schema, inflate)
    return cabi.decode_blocks_where(buf, start, end, info._first, info.schema, where, num_chunks, cabi.CODEC_DEFLATE if on_device else None,
                                    MAX_BLOCK_BYTES, kernel=P._kernel_mode, columns=columns, reader_schema=reader_schema)


def read_container_where_to_device(src, where, num_chunks=1, device: int = -1, *, columns=None, reader_schema=None, inflate=None):
    """Extension.  ``read_container_where`` with the Arrow buffers left in HBM: a ``DeviceDecode`` as ``read_container_to_device``
    returns; its ``.kept`` is the number of records the predicate kept."""
    import pyruhvro_amd as P
    from . import cabi
    from .device import DeviceDecode
    info, buf, start, end, on_device = _blocks_where(src, where, num_chunks, columns, reader_schema, inflate)
    r = cabi.decode_blocks_where(buf, start, end, info._first, info.schema, where, num_chunks, cabi.CODEC_DEFLATE if on_device else None,
                                 MAX_BLOCK_BYTES, device=device, kernel=P._kernel_mode, columns=columns, reader_schema=reader_schema,
                                 to_device=True)
    return DeviceDecode(r, cabi.Schema.get(info.schema, columns, reader_schema).arrow_schema)


def filter_container(src, where, *, inflate=None):
    """Extension.  The row filter of ``read_container_where`` alone -- the split and the predicate, no decode: a numpy
    ``bool[info.num_records]``, True where the file's record is kept (the twin of ``filter_records``)."""
    from . import cabi
    info, buf, start, end, on_device = _blocks_where(src, where, 1, None, None, inflate)
    return cabi.filter_blocks(buf, start, end, info._first, info.schema, where, cabi.CODEC_DEFLATE if on_device else None, MAX_BLOCK_BYTES)


BlockError = namedtuple("BlockError", ["block", "offset", "length", "kept", "lost", "message"])
BlockError.__doc__ = """One entry of a tolerant container read's ``errors``.  A damaged block: ``block`` = its index among the blocks that
were framed, ``offset`` = the first byte of its header, ``length`` = header + payload + marker, ``kept`` / ``lost`` = the records
of it that are in the batches / that are not, ``message`` = what ``read_container`` raises for a file in which this is the only
damage.  A gap -- bytes in which no block could be framed: ``block`` and ``lost`` are None, ``kept`` is 0, ``message`` = what
the framing scan says where the gap begins."""


def _salvage(src, num_chunks, columns, reader_schema, inflate, max_errors):
    """The tolerant read up to the engine call -> (info, engine arguments, entries known here, claimed counts, table)."""
    import numpy as np
    import pyruhvro_amd as P
    from . import cabi
    from .device import check_max_errors
    road = _inflate_road(inflate)
    P._check_chunks(num_chunks)
    max_errors = check_max_errors(max_errors)
    buf = _bytes_of(src)
    scan = cabi.container_salvage(buf)                       # ValueError "container: ..." for a header that does not parse
    info = ContainerInfo(scan)
    P._get_schema(info.schema, columns, reader_schema)
    nb = info.num_blocks
    count, hoff = scan["count"], scan["header_offset"]
    entries = [BlockError(None, off, length, 0, None, msg) for off, length, _, msg in scan["gaps"]]
    messages = {int(b): f"container: block {int(b)}: record count out of range" for b in np.flatnonzero(scan["refused"])}
    start, end, codec, data = info._start, info._end, cabi.CODEC_NULL, buf
    if info.codec == "deflate" and road == "device":
        codec = cabi.CODEC_DEFLATE
    elif info.codec == "deflate":
        data, start, end = _inflate(buf, info, messages)
    dropped = np.zeros(nb, dtype=np.uint8)
    for b, msg in messages.items():
        dropped[b] = 1
        entries.append(BlockError(b, int(hoff[b]), int(info._end[b]) + 16 - int(hoff[b]), 0, int(count[b]), msg))
    return info, (data, start, end, info._first, dropped, codec, len(scan["gaps"]), max_errors), entries, count, hoff


def _block_errors(info, status, entries, count, hoff):
    """The engine's per-block status -> the entries it adds, merged with those known before the call, ascending by offset."""
    import numpy as np
    from . import cabi
    for b in np.flatnonzero(status["code"]):
        b = int(b)
        st = status[b]
        if int(st["code"]) == cabi.BLOCK_DROPPED:
            continue                                         # (listed already: its message was made here)
        kept = int(st["kept"])
        entries.append(BlockError(b, int(hoff[b]), int(info._end[b]) + 16 - int(hoff[b]), kept, int(count[b]) - kept,
                                  cabi.block_status_message(b, st, int(count[b]))))
    return sorted(entries, key=lambda e: e.offset)


def _too_many(src, num_chunks, columns, reader_schema, inflate):
    """More than max_errors entries: the strict call's error, the lowest one -- from the strict call itself."""
    read_container(src, num_chunks, columns=columns, reader_schema=reader_schema, inflate=inflate)
    raise RuntimeError("internal error: the strict read accepts a file in which the tolerant read reports damage")


def read_container_tolerant(src, num_chunks=1, *, max_errors=1024, columns=None, reader_schema=None, inflate=None):
    """Extension.  ``read_container`` that damage in the file does not abort: ``(list[pyarrow.RecordBatch], errors)``.  The
    batches are exactly ``deserialize_array_threaded(kept, info.schema, num_chunks, ...)`` over the records that are kept, in
    file order: every record of a sound block, and records ``0 .. j - 1`` of a block whose record ``j`` is malformed (nothing
    behind a malformed record of the same block can be recovered: nothing says where the next one starts).  Rows are dropped,
    not replaced.  A block whose count or deflate stream is refused keeps nothing.  Where no block can be framed -- a damaged
    block header or sync marker, a file cut short -- the read goes on behind the next occurrence of the file's sync marker and
    the bytes skipped are a gap.  ``errors``: one ``BlockError`` per damaged block and per gap, ascending by offset; more than
    ``max_errors`` of them raise what ``read_container`` raises.  A header that does not parse raises as it does there."""
    import pyruhvro_amd as P
    from . import cabi
    info, (data, start, end, first, dropped, codec, gaps, max_errors), entries, count, hoff = _salvage(src, num_chunks, columns, reader_schema,
                                                                                                      inflate, max_errors)
    batches, status = cabi.decode_blocks_tolerant(data, start, end, first, info.schema, num_chunks, codec, MAX_BLOCK_BYTES, dropped, max_errors,
                                                  gaps, kernel=P._kernel_mode, columns=columns, reader_schema=reader_schema)
    if batches is None:
        _too_many(src, num_chunks, columns, reader_schema, inflate)
    return batches, _block_errors(info, status, entries, count, hoff)


def read_container_to_device_tolerant(src, num_chunks=1, device: int = -1, *, max_errors=1024, columns=None, reader_schema=None, inflate=None):
    """Extension.  ``read_container_tolerant`` with the Arrow buffers left in HBM: a ``DeviceDecode`` as
    ``read_container_to_device`` returns, its ``.errors`` the list of ``BlockError``."""
    import pyruhvro_amd as P
    from . import cabi
    from .device import DeviceDecode
    info, (data, start, end, first, dropped, codec, gaps, max_errors), entries, count, hoff = _salvage(src, num_chunks, columns, reader_schema,
                                                                                                      inflate, max_errors)
    r, status = cabi.decode_blocks_tolerant_device(data, start, end, first, info.schema, num_chunks, codec, MAX_BLOCK_BYTES, dropped, max_errors,
                                                   gaps, device=device, kernel=P._kernel_mode, columns=columns, reader_schema=reader_schema)
    if r is None:
        _too_many(src, num_chunks, columns, reader_schema, inflate)
    dec = DeviceDecode(r, cabi.Schema.get(info.schema, columns, reader_schema).arrow_schema)
    dec.errors = _block_errors(info, status, entries, count, hoff)
    return dec


def _put_long(out: bytearray, v: int) -> None:
    z = (v << 1) ^ (v >> 63)
    while z >= 0x80:
        out.append((z & 0x7F) | 0x80)
        z >>= 7
    out.append(z)


def _put_bytes(out: bytearray, b: bytes) -> None:
    _put_long(out, len(b))
    out += b


def _deflate_road(deflate) -> str:
    """``deflate=`` of a write: "host" or "device"; None reads RUHVRO_HIP_DEFLATE (per call) and falls back to "host"."""
    if deflate is None:
        deflate = os.environ.get("RUHVRO_HIP_DEFLATE") or "host"
    if deflate not in ("host", "device"):
        raise ValueError("container: deflate must be 'host' or 'device'")
    return deflate


def write_container(batch, schema, *, codec: str = "null", block_rows: int = 4096, sync: Optional[bytes] = None, metadata=None,
                    deflate=None) -> bytes:
    """Extension.  ``batch`` (a ``pyarrow.RecordBatch``) as an Avro object container: host framing around
    ``serialize_record_batch`` (the GPU encoder).  One block per ``block_rows`` rows; the header carries ``schema`` verbatim,
    the codec (``"null"`` or ``"deflate"``) and the caller's ``metadata`` (``{str: bytes or str}``; the ``avro.`` names are the
    format's own).  ``sync``: the 16-byte marker, random by default.  ``deflate``: where a ``deflate`` file's blocks are
    compressed -- ``"host"`` (``zlib``, block by block on the calling thread), ``"device"`` (the GPU: every block in one call,
    32 KiB segments in parallel; raw RFC 1951 streams any inflater reads, not the bytes ``zlib`` would write), ``None`` =
    ``RUHVRO_HIP_DEFLATE`` or ``"host"``."""
    import numpy as np
    import pyruhvro_amd as P
    road = _deflate_road(deflate)                                # ValueError before any device work, for codec="null" too
    if not isinstance(schema, str):
        raise TypeError("argument 'schema': expected str")
    if codec not in ("null", "deflate"):
        raise ValueError(f"container: codec {codec!r} is not supported")
    if not isinstance(block_rows, int) or isinstance(block_rows, bool):
        raise TypeError("argument 'block_rows': expected int")
    if block_rows < 1:
        raise ValueError("container: block_rows must be at least 1")
    sync = os.urandom(16) if sync is None else bytes(sync)
    if len(sync) != 16:
        raise ValueError("container: the sync marker is 16 bytes")
    entries = [(b"avro.schema", schema.encode("utf-8")), (b"avro.codec", codec.encode())]
    for k, v in (metadata or {}).items():
        if not isinstance(k, str):
            raise TypeError("argument 'metadata': keys are str")
        if k.startswith("avro."):
            raise ValueError(f"container: metadata key {k!r} is reserved by the format")
        if isinstance(v, str):
            v = v.encode("utf-8")
        if not isinstance(v, (bytes, bytearray, memoryview)):
            raise TypeError(f"argument 'metadata': the value of {k!r} is neither bytes nor str")
        entries.append((k.encode("utf-8"), bytes(v)))
    records = P.serialize_record_batch(batch, schema, 1)[0]      # one BinaryArray, one datum per row

    out = bytearray(MAGIC)
    _put_long(out, len(entries))
    for k, v in entries:
        _put_bytes(out, k)
        _put_bytes(out, v)
    _put_long(out, 0)
    out += sync

    n = len(records)
    if n:
        import pyarrow as pa
        if pa.types.is_binary(records.type):
            off_t = np.int32
        elif pa.types.is_large_binary(records.type):
            off_t = np.int64
        else:
            raise TypeError(f"container: serialize_record_batch returned {records.type}, not a binary array")
        bufs = records.buffers()
        offs = np.frombuffer(bufs[1], dtype=off_t, count=records.offset + n + 1)[records.offset:]
        data = memoryview(bufs[2]) if bufs[2] is not None else memoryview(b"")
        if codec == "deflate" and road == "device":              # every block's payload in one call; zlib is not called
            from . import cabi
            edges = offs[np.append(np.arange(0, n, block_rows), n)].astype(np.uint64)
            raw = np.frombuffer(data, dtype=np.uint8) if data.nbytes else np.zeros(0, dtype=np.uint8)
            blob, c_start, c_end = cabi.deflate_blocks(raw, edges[:-1], edges[1:])
            blob = memoryview(blob)
        for b, r0 in enumerate(range(0, n, block_rows)):
            r1 = min(r0 + block_rows, n)
            payload = data[int(offs[r0]):int(offs[r1])]
            if codec == "deflate" and road == "device":
                payload = blob[int(c_start[b]):int(c_end[b])]
            elif codec == "deflate":
                c = zlib.compressobj(wbits=-15)
                payload = c.compress(payload) + c.flush()
            _put_long(out, r1 - r0)
            _put_long(out, len(payload))
            out += payload
            out += sync
    return bytes(out)
