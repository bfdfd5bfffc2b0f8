"""pyruhvro_amd -- MI355X-native Avro -> Arrow direct decode behind pyruhvro's Python surface.

Same function names, positional signatures, return types and error behaviour
as the reference's PyO3 module (``/src/lib.rs:56-158`` of Tyler-Sch/pyruhvro):

    deserialize_array(list, schema) -> pyarrow.RecordBatch
    deserialize_array_threaded(list, schema, num_chunks) -> list[pyarrow.RecordBatch]
    deserialize_array_threaded_spawn(list, schema, num_chunks) -> list[pyarrow.RecordBatch]
    serialize_record_batch(batch, schema, num_chunks) -> list[pyarrow.BinaryArray]   (Arrow -> Avro, also on the GPU)
    serialize_record_batch_spawn(...)                                                 same

Several GPUs: ``set_devices([0, 1, ...])`` (or ``PYRUHVRO_DEVICES=0,1,...`` in the environment) deals the
``num_chunks`` output chunks to those devices in contiguous runs, so every returned batch is produced by one GPU and
the result does not depend on how many there are (the reference deals its chunks to a thread pool the same way,
``ruhvro/src/deserialize.rs:92-120``).

The decode runs in hand-written HIP kernels on the GPU through the C ABI in
``include/ruhvro_hip.h`` (``libruhvro_hip.so``).  There is no CPU decode path in
this package: without the native library or without a HIP device the calls
raise ``RuntimeError``.

If the process also uses PyTorch-ROCm, import torch BEFORE this package so both
share torch's bundled HIP runtime (same SONAME, first one loaded wins).
"""
from __future__ import annotations

import os
import threading
from typing import List

import pyarrow as pa

_HERE = os.path.dirname(os.path.abspath(__file__))

try:
    from . import _pyruhvro as _native  # noqa: F401
except ImportError as _e:  # pragma: no cover - exercised only on an unbuilt tree
    _native = None
    _native_error = _e


def _require_native():
    if _native is None:
        raise RuntimeError(
            "pyruhvro_amd: native extension not built (run `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `python pyruhvro_amd/_build.py`): {_native_error}")
    return _native


# Schema cache keyed by the exact schema string, unbounded -- src/lib.rs:35-54.
_cache_lock = threading.Lock()
_cache: dict = {}


class _Compiled:
    __slots__ = ("capsule", "arrow_schema")

    def __init__(self, capsule, arrow_schema):
        self.capsule = capsule
        self.arrow_schema = arrow_schema


def _check_columns(columns):
    from .cabi import check_columns
    return check_columns(columns)


def _get_schema(schema: str, columns=None, reader_schema=None) -> _Compiled:
    """The compiled schema, or -- `columns`: a tuple of distinct top-level field names -- its projection onto those columns,
    or -- `reader_schema`: Avro JSON -- the writer schema `schema` resolved into that reader schema, `columns` then naming
    reader fields (cached by (schema, reader_schema, columns): each is a schema of its own, with its own kernels and size
    history)."""
    if not isinstance(schema, str):
        raise TypeError("argument 'schema': expected str")
    columns = _check_columns(columns)         # ValueError before any native work
    if reader_schema is not None and not isinstance(reader_schema, str):
        raise TypeError("argument 'reader_schema': expected str or None")
    key = (schema if columns is None else (schema, columns)) if reader_schema is None else (schema, reader_schema, columns)
    with _cache_lock:
        hit = _cache.get(key)
    if hit is not None:
        return hit
    nat = _require_native()
    if reader_schema is not None:
        from .cabi import reader_columns
        cap = nat.resolve_schema(_get_schema(schema).capsule, reader_columns(reader_schema, columns))   # ValueError "reader schema: ..."
    elif columns is None:
        cap = nat.compile_schema(schema)      # ValueError on a bad / unsupported schema (src/lib.rs:52)
    else:
        cap = nat.project_schema(_get_schema(schema).capsule, columns)   # ValueError: unknown / dotted name
    addr = nat.export_schema(cap)
    try:
        st = pa.DataType._import_from_c(addr)  # "+s" struct whose fields are the batch columns
    finally:
        nat.free_struct(addr)
    comp = _Compiled(cap, pa.schema(list(st)))
    with _cache_lock:
        return _cache.setdefault(key, comp)


def arrow_schema(schema: str, *, columns=None, reader_schema=None) -> pa.Schema:
    """Arrow schema the decode produces for this Avro schema (schema_translate.rs:19-37); `columns`: of the projection
    onto those top-level fields, in that order; `reader_schema`: of the decode of `schema`-written records into it."""
    return _get_schema(schema, columns, reader_schema).arrow_schema


KERNEL_AUTO, KERNEL_GENERIC, KERNEL_SPECIALIZED = 0, 1, 2
_kernel_mode = KERNEL_AUTO


def set_kernel_mode(mode) -> int:
    """Which HIP kernel form decodes: "auto" (default: schema-specialised kernels for large calls or when the
    code object is cached, generic schema-program interpreter otherwise), "generic" or "specialized".
    Both run on the GPU and produce identical buffers.  Returns the previous mode."""
    global _kernel_mode
    names = {"auto": KERNEL_AUTO, "generic": KERNEL_GENERIC, "specialized": KERNEL_SPECIALIZED}
    new = names[mode] if isinstance(mode, str) else int(mode)
    if new not in (0, 1, 2):
        raise ValueError("kernel mode must be auto, generic or specialized")
    old, _kernel_mode = _kernel_mode, new
    return old


_devices = None      # None: the current HIP device; else the ordinals the chunks are dealt to


def _env_devices():
    e = os.environ.get("PYRUHVRO_DEVICES", "").strip()
    if not e:
        return None
    try:
        return [int(x) for x in e.split(",") if x.strip() != ""]
    except ValueError:
        raise ValueError(f"PYRUHVRO_DEVICES: expected comma-separated device ordinals, got {e!r}") from None


def set_devices(devices):
    """Deal the chunks of every later decode call to these HIP devices (a sequence of ordinals; an ordinal may repeat
    to run several logical shards on one GPU; ``None`` = back to the current device / ``PYRUHVRO_DEVICES``).
    Returns the previous setting."""
    global _devices
    old = _devices
    if devices is None:
        _devices = None
    else:
        devs = [int(d) for d in devices]
        if not devs:
            raise ValueError("set_devices: empty device list")
        _devices = devs
    return old


def _current_devices():
    return _devices if _devices is not None else _env_devices()


def _decode_where(list_, schema: str, num_chunks: int, columns, reader_schema, where):
    """The filtered strict decode: the list packed on the host and uploaded in one piece (rh_decode_packed_where; not the pinned,
    pipelined list path of the unfiltered call)."""
    from . import cabi
    cabi.check_where(where)                    # TypeError / ValueError before any native work
    _get_schema(schema, columns, reader_schema)
    _check_chunks(num_chunks)
    cabi.Filter.get(schema, where)             # ValueError "where: ..." before the list is touched
    data, offs = _pack_records(list_)
    return cabi.decode_packed(data, offs, schema, num_chunks, kernel=_kernel_mode, devices=_current_devices(), columns=columns,
                              reader_schema=reader_schema, where=where)


def _decode(list_, schema: str, num_chunks: int, want_stats: bool = False, device: int = -1, stream: int = 0, columns=None,
            reader_schema=None, where=None):
    if where is not None:
        return _decode_where(list_, schema, num_chunks, columns, reader_schema, where), None
    comp = _get_schema(schema, columns, reader_schema)
    nat = _require_native()
    if not isinstance(num_chunks, int) or isinstance(num_chunks, bool):
        raise TypeError("argument 'num_chunks': expected int")
    if num_chunks < 0:
        raise OverflowError("can't convert negative int to unsigned")  # usize extraction in PyO3
    devs = _current_devices() if device < 0 and not stream else None
    addrs, stats = nat.decode(comp.capsule, list_, num_chunks, device, stream, want_stats, _kernel_mode, devs)
    out: List[pa.RecordBatch] = []
    try:
        for i, a in enumerate(addrs):
            out.append(pa.RecordBatch._import_from_c(a, comp.arrow_schema))
            nat.free_struct(a)     # content was moved into pyarrow, only the shell is left
            addrs[i] = 0
    finally:
        for a in addrs:
            if a:
                nat.release_array(a)
    return out, stats


def deserialize_array(list, schema, *, columns=None, reader_schema=None, where=None):  # noqa: A002 - the reference's parameter name
    """src/lib.rs:56-71 -> ruhvro::deserialize::per_datum_deserialize (deserialize.rs:25-30).

    ``columns`` (keyword only, an extension): decode only these top-level fields, in this order -- the batch equals the
    full decode's ``.select(columns)`` buffer for buffer; the other columns are neither built nor copied.  A malformed
    record still raises the full decode's error, whichever field it damages.

    ``reader_schema`` (keyword only, an extension): ``schema`` is the schema the records were WRITTEN with and the batch is
    in this Avro schema -- fields matched by name, writer fields it lacks dropped, fields the writer lacks filled with their
    ``default``, columns in its order, int / long / float promoted, string <-> bytes (DESIGN.md 13 for the rules and what is
    refused, with a ``ValueError`` that starts with ``reader schema:``).  ``columns`` then names reader fields.

    ``where`` (keyword only, an extension): decode only the records that match a predicate -- one term ``(name, op, value)`` or a
    list of up to 8 terms, ANDed; ``op`` is one of ``== != < <= > >= is_null not_null``; ``name`` is a top-level field of the
    WRITER schema, whether or not ``columns`` / ``reader_schema`` build it.  The batch equals the decode of the matching
    records alone, buffer for buffer; the records are chosen on the GPU before anything is decoded.  A null matches no
    comparison.  A malformed record raises the plain decode's error, whatever the predicate says about it (DESIGN.md 15
    for the field kinds and what is refused, with a ``ValueError`` that starts with ``where:``)."""
    return _decode(list, schema, 1, columns=columns, reader_schema=reader_schema, where=where)[0][0]


def deserialize_array_threaded(list, schema, num_chunks, *, columns=None, reader_schema=None, where=None):  # noqa: A002
    """src/lib.rs:73-89 -> per_datum_deserialize_threaded (deserialize.rs:76-121):
    ``clamp(num_chunks, 1, max(len(list), 1))`` batches, chunk order preserved.  ``columns`` / ``reader_schema`` / ``where``: see
    deserialize_array (the chunking applies to the records ``where`` keeps)."""
    return _decode(list, schema, num_chunks, columns=columns, reader_schema=reader_schema, where=where)[0]


def deserialize_array_threaded_spawn(list, schema, num_chunks, *, columns=None, reader_schema=None, where=None):  # noqa: A002
    """src/lib.rs:108-128 -- same results as deserialize_array_threaded (deserialize.rs:127-170)."""
    return _decode(list, schema, num_chunks, columns=columns, reader_schema=reader_schema, where=where)[0]


def deserialize_array_threaded_with_stats(list, schema, num_chunks, device: int = -1, *, columns=None, reader_schema=None):  # noqa: A002
    """Extension: also returns the engine's per-stage timings (rh_stats)."""
    return _decode(list, schema, num_chunks, want_stats=True, device=device, columns=columns, reader_schema=reader_schema)


def last_decode_profile():
    """Extension: where this thread's most recent ``deserialize_array*`` call spent its time at the CPython boundary --
    set-up, list extraction, the rest of the engine call, the total, and how long the call held the GIL (milliseconds)."""
    _require_native()
    return _native.last_decode_profile()


def deserialize_binary_array(array, schema, num_chunks, *, columns=None, reader_schema=None, where=None):
    """Extension: the same decode for records that already sit in an Arrow
    ``BinaryArray`` / ``LargeBinaryArray`` (one record per element) -- the form the reference packs its
    list into internally (deserialize.rs:90).  Zero-copy on the payload: no per-``bytes`` extraction
    under the GIL.  Returns ``list[pyarrow.RecordBatch]`` with the chunking of deserialize_array_threaded.  ``where``: see
    deserialize_array."""
    import numpy as np
    from . import cabi
    cabi.check_where(where)
    if isinstance(array, pa.ChunkedArray):
        array = array.combine_chunks() if array.num_chunks != 1 else array.chunk(0)
    if not isinstance(array, (pa.BinaryArray, pa.LargeBinaryArray)):
        raise TypeError("argument 'array': expected a pyarrow BinaryArray or LargeBinaryArray")
    if array.null_count:
        raise ValueError("null records cannot be decoded")
    if not isinstance(num_chunks, int) or isinstance(num_chunks, bool):
        raise TypeError("argument 'num_chunks': expected int")
    if num_chunks < 0:
        raise OverflowError("can't convert negative int to unsigned")
    _get_schema(schema, columns, reader_schema)          # ValueError on a bad / unsupported schema, like every entry point
    n = len(array)
    bufs = array.buffers()
    odt = np.int64 if isinstance(array, pa.LargeBinaryArray) else np.int32
    offs = np.frombuffer(bufs[1], dtype=odt, count=array.offset + n + 1)[array.offset:]
    base = int(offs[0]) if n else 0
    end = int(offs[-1]) if n else 0
    data = (np.frombuffer(bufs[2], dtype=np.uint8, count=end)[base:] if bufs[2] is not None and end > base
            else np.zeros(1, dtype=np.uint8))
    offsets = (offs.astype(np.uint64) - np.uint64(base)) if n else np.zeros(1, dtype=np.uint64)
    return cabi.decode_packed(data, offsets, schema, num_chunks, kernel=_kernel_mode, devices=_current_devices(), columns=columns,
                              reader_schema=reader_schema, where=where)


def _check_chunks(num_chunks):
    if not isinstance(num_chunks, int) or isinstance(num_chunks, bool):
        raise TypeError("argument 'num_chunks': expected int")
    if num_chunks < 0:
        raise OverflowError("can't convert negative int to unsigned")


def _pack_records(records):
    """list[bytes] or a pyarrow (Large)BinaryArray -> (payload, offsets) with at least one addressable payload byte."""
    import numpy as np
    from .device import _pack
    if isinstance(records, (list, tuple)):
        for r in records:
            if not isinstance(r, (bytes, bytearray, memoryview)):
                raise TypeError("argument 'list': expected a list of bytes")
    data, offs = _pack(records)
    return (data if len(data) else np.zeros(1, dtype=np.uint8)), offs


def placeholder_datum(schema) -> bytes:
    """Extension.  The datum a tolerant decode puts in the place of a malformed record: the shortest datum of the schema that the
    strict decoder accepts -- null wherever the schema allows null, zero / empty elsewhere ("Tolerant decode")."""
    from . import cabi
    _get_schema(schema)
    return cabi.placeholder_datum(schema)


def validate_records(list, schema, *, max_errors=1024, reader_schema=None):  # noqa: A002
    """Extension.  ALL malformed records of the list as ``[RecordError(index, message)]``, ascending by index (the ``max_errors``
    lowest when there are more): ``message`` is what ``deserialize_array`` raises when that record is the first malformed one."""
    from . import cabi
    from .device import check_max_errors
    cabi.refuse_reader_schema(reader_schema, "validate_records")
    _get_schema(schema)
    data, offs = _pack_records(list)
    return cabi.validate_packed(data, offs, schema, check_max_errors(max_errors), devices=_current_devices())


def filter_records(list, schema, where):  # noqa: A002
    """Extension.  The row filter alone (see ``deserialize_array``'s ``where``): a numpy ``bool[len(list)]``, True where the record
    matches.  A malformed record raises what ``deserialize_array`` raises for the lowest failing record."""
    from . import cabi
    if cabi.check_where(where) is None:
        raise TypeError("argument 'where': expected a term (name, op, value) or a list of terms")
    _get_schema(schema)
    cabi.Filter.get(schema, where)
    data, offs = _pack_records(list)
    return cabi.filter_packed(data, offs, schema, where, devices=_current_devices())


def _decode_tolerant(records, schema, num_chunks, columns, max_errors, reader_schema=None):
    from . import cabi
    cabi.refuse_reader_schema(reader_schema, "a tolerant decode")
    from .device import check_max_errors
    _check_chunks(num_chunks)
    _get_schema(schema, columns)
    data, offs = _pack_records(records)
    return cabi.decode_packed_tolerant(data, offs, schema, num_chunks, kernel=_kernel_mode, devices=_current_devices(),
                                       columns=columns, max_errors=check_max_errors(max_errors))


def deserialize_array_tolerant(list, schema, *, columns=None, max_errors=1024, reader_schema=None):  # noqa: A002
    """Extension.  ``deserialize_array`` that a malformed record does not abort: returns ``(batch, errors)`` where the batch has
    ``placeholder_datum(schema)`` decoded in the place of every malformed record (same row count) and ``errors`` lists all of
    them as ``RecordError(index, message)``.  More than ``max_errors`` malformed records raise what ``deserialize_array``
    raises.  Clean input costs what the strict call costs."""
    batches, errors = _decode_tolerant(list, schema, 1, columns, max_errors, reader_schema)
    return batches[0], errors


def deserialize_array_threaded_tolerant(list, schema, num_chunks, *, columns=None, max_errors=1024, reader_schema=None):  # noqa: A002
    """Extension.  ``deserialize_array_threaded`` in the tolerant form: ``(list[RecordBatch], errors)``, the chunking unchanged."""
    return _decode_tolerant(list, schema, num_chunks, columns, max_errors, reader_schema)


def deserialize_binary_array_tolerant(array, schema, num_chunks, *, columns=None, max_errors=1024, reader_schema=None):
    """Extension.  ``deserialize_binary_array`` in the tolerant form: ``(list[RecordBatch], errors)``."""
    if isinstance(array, pa.ChunkedArray):
        array = array.combine_chunks() if array.num_chunks != 1 else array.chunk(0)
    if not isinstance(array, (pa.BinaryArray, pa.LargeBinaryArray)):
        raise TypeError("argument 'array': expected a pyarrow BinaryArray or LargeBinaryArray")
    return _decode_tolerant(array, schema, num_chunks, columns, max_errors, reader_schema)


def _encode(data, schema: str, num_chunks: int, want_stats: bool = False, device: int = -1, stream: int = 0, reader_schema=None):
    import ctypes
    if reader_schema is not None:
        raise ValueError("reader schema: serialize_* does not take reader_schema= (schema resolution is strict-decode only)")
    comp = _get_schema(schema)                 # (always the full schema: projection is decode only)
    nat = _require_native()
    if isinstance(data, pa.RecordBatch):
        sa = data.to_struct_array()
    elif isinstance(data, pa.StructArray):
        sa = data
    else:
        raise TypeError("argument 'data': expected a pyarrow RecordBatch")
    if not isinstance(num_chunks, int) or isinstance(num_chunks, bool):
        raise TypeError("argument 'num_chunks': expected int")
    if num_chunks < 0:
        raise OverflowError("can't convert negative int to unsigned")
    c_arr = ctypes.create_string_buffer(80)        # struct ArrowArray
    c_sch = ctypes.create_string_buffer(72)        # struct ArrowSchema
    sa._export_to_c(ctypes.addressof(c_arr), ctypes.addressof(c_sch))
    addrs, stats = nat.encode(comp.capsule, ctypes.addressof(c_arr), ctypes.addressof(c_sch), num_chunks,
                              device, stream, want_stats, _kernel_mode)   # releases the two exported structs
    out = []
    try:
        for i, a in enumerate(addrs):
            out.append(pa.Array._import_from_c(a, pa.binary()))
            nat.free_struct(a)
            addrs[i] = 0
    finally:
        for a in addrs:
            if a:
                nat.release_array(a)
    return out, stats


def serialize_record_batch(data, schema, num_chunks, *, reader_schema=None):
    """src/lib.rs:91-106 -> ruhvro::serialize::serialize_record_batch (serialize.rs:38-67) with the fast encoder
    (fast_encode.rs:27-53): ``clamp(num_chunks, 1, max(rows, 1))`` BinaryArrays, one Avro datum per row, columns
    matched to the schema's fields by name.  Runs on the GPU (rh_encode)."""
    return _encode(data, schema, num_chunks, reader_schema=reader_schema)[0]


def serialize_record_batch_spawn(data, schema, num_chunks, *, reader_schema=None):
    """src/lib.rs:130-148 -- same results as serialize_record_batch (serialize.rs:70-99)."""
    return _encode(data, schema, num_chunks, reader_schema=reader_schema)[0]


def serialize_record_batch_with_stats(data, schema, num_chunks, device: int = -1, *, reader_schema=None):
    """Extension: also returns the engine's per-stage timings (rh_stats)."""
    return _encode(data, schema, num_chunks, want_stats=True, device=device, reader_schema=reader_schema)


def device_count() -> int:
    return _require_native().device_count()


def deserialize_to_device(records, schema, num_chunks, device: int = -1, stream: int = 0, *, columns=None, on_error="raise",
                          max_errors=1024, reader_schema=None, where=None):
    """Extension: the same decode with the Arrow buffers left in HBM, every buffer a DLPack producer
    (``torch.from_dlpack(dec.batches[0].column("created_at").values)`` is an int64 tensor over the engine's memory, no copy).
    ``on_error="placeholder"``: the tolerant form -- the result's ``.errors`` lists the malformed records that were replaced by
    ``placeholder_datum(schema)``; with ``"raise"`` (the default) ``.errors`` is ``[]``.  ``where``: only the matching records
    (see ``deserialize_array``; not with ``on_error="placeholder"``); the result's ``.kept`` says how many.  See
    ``pyruhvro_amd.device``."""
    from .device import deserialize_to_device as f
    return f(records, schema, num_chunks, device=device, stream=stream, kernel=_kernel_mode, columns=columns, on_error=on_error,
             max_errors=max_errors, reader_schema=reader_schema, where=where)


def kernels_ready(schema: str, encode: bool = False, timeout_ms: int = 0, *, columns=None, reader_schema=None) -> bool:
    """Extension.  A schema this process has not met is decoded by the generic kernels at once while the kernels specialised
    to it compile in the background (the reference's cost of a new schema is a JSON parse, ``src/lib.rs:39-54``; a hiprtc
    compile is seconds).  True when they are there -- the next call runs on them; waits up to ``timeout_ms`` for running
    compile jobs.  Raises ``RuntimeError`` if the compile failed (calls keep working on the generic kernels)."""
    return bool(_require_native().kernels_ready(_get_schema(schema, columns, reader_schema).capsule, bool(encode), int(timeout_ms)))


def prebuild(schema: str, *, columns=None, reader_schema=None) -> bool:
    """Extension.  Compile this schema's specialised kernels now (all of them, side by side) and wait: for services that
    want their first batch at full speed.  The code objects land in the kernel cache (``RUHVRO_HIP_KERNEL_CACHE`` or
    ``pyruhvro_amd/_kcache``), where later processes find them.  True when nothing had to be compiled."""
    return bool(_require_native().prebuild(_get_schema(schema, columns, reader_schema).capsule))


__all__ = [
    "deserialize_array", "deserialize_array_threaded", "deserialize_array_threaded_spawn",
    "serialize_record_batch_with_stats",
    "serialize_record_batch", "serialize_record_batch_spawn", "arrow_schema", "device_count", "set_kernel_mode",
    "deserialize_binary_array", "set_devices", "kernels_ready", "prebuild", "deserialize_to_device",
    "placeholder_datum", "validate_records", "filter_records", "RecordError", "deserialize_array_tolerant", "deserialize_array_threaded_tolerant",
    "deserialize_binary_array_tolerant",
    "container_info", "read_container", "read_container_to_device", "write_container", "ContainerInfo",
    "read_container_tolerant", "read_container_to_device_tolerant", "BlockError",
    "read_container_where", "read_container_where_to_device", "filter_container",
    "deserialize_framed", "frame_split", "schema_fingerprint", "FramedGroup", "FramedResult", "serialize_framed",
]

from .container import ContainerInfo, container_info, read_container, read_container_to_device, write_container  # noqa: E402
from .container import BlockError, read_container_tolerant, read_container_to_device_tolerant  # noqa: E402
from .container import filter_container, read_container_where, read_container_where_to_device  # noqa: E402
from .framing import FramedGroup, FramedResult, deserialize_framed, frame_split, schema_fingerprint, serialize_framed  # noqa: E402


def __getattr__(name):      # (RecordError lives beside the ctypes wrappers that build it; cabi needs numpy, imported on first use)
    if name == "RecordError":
        from .cabi import RecordError
        return RecordError
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
