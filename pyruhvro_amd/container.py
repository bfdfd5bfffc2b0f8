"""Avro object container files (``.avro``): read them on the GPU, write them around the GPU encoder.

    info = pyruhvro.container_info("events.avro")                   # header + block table, no device work
    batches = pyruhvro.read_container("events.avro", 8)              # == deserialize_array_threaded(records_of(file), info.schema, 8)
    dec = pyruhvro.read_container_to_device(buf, 8)                  # as deserialize_to_device
    blob = pyruhvro.write_container(batch, schema, codec="deflate")  # bytes

A container block says "N records, M bytes" and nothing says where record j starts.  The file is uploaded as it is and a
split kernel -- one lane per block -- walks the records with the writer's schema (the file's own, from its header) to find
their offsets; the ordinary decode then runs on them.  ``columns=`` and ``reader_schema=`` mean what they mean for
``deserialize_array_threaded``.  Codecs: ``null`` and ``deflate``; anything else is refused.  A ``deflate`` file is inflated
either here with ``zlib``, block by block, into one buffer (``inflate="host"``, the default), or on the device: the
compressed file is uploaded as it is and two kernels inflate its blocks, one wavefront per block (``inflate="device"``, or
``RUHVRO_HIP_INFLATE=device`` in the environment).  Both roads accept the same streams and raise the same messages.  The
tolerant functions do not take containers: a malformed record loses its block's boundaries.
"""
from __future__ import annotations

import os
import zlib
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


def _inflate(buf, info: ContainerInfo):
    """A deflate container -> (one buffer of its inflated blocks back to back, the new starts and ends)."""
    import numpy as np
    mv = memoryview(buf)
    out = bytearray()      # every block inflates straight into it, in steps: no second copy, and no block past the limit
    start = np.zeros(info.num_blocks, dtype=np.uint64)
    end = np.zeros(info.num_blocks, dtype=np.uint64)
    for b in range(info.num_blocks):
        d = zlib.decompressobj(-15)
        at = len(out)
        data = mv[int(info._start[b]):int(info._end[b])]
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


def _put_long(out: bytearray, v: int) -> None:
    z = (v << 1) ^ (v >> 63)
    while z >= 0x80:
        out.append((z & 0x7F) | 0x80)
        z >>= 7
    out.append(z)


def _put_bytes(out: bytearray, b: bytes) -> None:
    _put_long(out, len(b))
    out += b


def write_container(batch, schema, *, codec: str = "null", block_rows: int = 4096, sync: Optional[bytes] = None, metadata=None) -> bytes:
    """Extension.  ``batch`` (a ``pyarrow.RecordBatch``) as an Avro object container: host framing around
    ``serialize_record_batch`` (the GPU encoder).  One block per ``block_rows`` rows; the header carries ``schema`` verbatim,
    the codec (``"null"`` or ``"deflate"``) and the caller's ``metadata`` (``{str: bytes or str}``; the ``avro.`` names are the
    format's own).  ``sync``: the 16-byte marker, random by default."""
    import numpy as np
    import pyruhvro_amd as P
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
        for r0 in range(0, n, block_rows):
            r1 = min(r0 + block_rows, n)
            payload = data[int(offs[r0]):int(offs[r1])]
            if codec == "deflate":
                c = zlib.compressobj(wbits=-15)
                payload = c.compress(payload) + c.flush()
            _put_long(out, r1 - r0)
            _put_long(out, len(payload))
            out += payload
            out += sync
    return bytes(out)
