"""ctypes view of the C ABI in include/ruhvro_hip.h (libruhvro_hip.so).

Used by bench.py (device-resident decode on torch-owned memory), by the
packed-input Python entry point, and by the tests that exercise the ABI
directly.  Nothing here decodes on the CPU.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple
from typing import List, Optional

import numpy as np
import pyarrow as pa

_HERE = os.path.dirname(os.path.abspath(__file__))
# RUHVRO_HIP_LIB: another build of the same library (the sanitizer build of _build.build_sanitized); never a fallback
LIB_PATH = os.environ.get("RUHVRO_HIP_LIB") or os.path.join(_HERE, "libruhvro_hip.so")

RH_OK, RH_ERR_SCHEMA, RH_ERR_DECODE, RH_ERR_RUNTIME, RH_ERR_ARGUMENT = range(5)


class RhStats(C.Structure):
    _fields_ = [("records", C.c_uint64), ("input_bytes", C.c_uint64), ("output_bytes", C.c_uint64),
                ("chunks", C.c_uint32), ("blocks", C.c_uint32), ("pack_ms", C.c_float), ("h2d_ms", C.c_float),
                ("size_kernel_ms", C.c_float), ("scan_kernel_ms", C.c_float), ("emit_kernel_ms", C.c_float),
                ("d2h_ms", C.c_float), ("total_ms", C.c_float), ("specialized", C.c_uint32), ("lds_bytes", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RhOpts(C.Structure):
    """rh_opts (ABI version 5: `struct_size` took the place of ABI 3's must-be-zero `reserved0`).  Build with make_opts()."""
    _fields_ = [("device", C.c_int32), ("flags", C.c_int32), ("stream", C.c_void_p),
                ("devices", C.POINTER(C.c_int32)), ("n_devices", C.c_uint32), ("struct_size", C.c_uint32),
                ("chunk_rows", C.c_uint64), ("device_stats", C.POINTER(RhStats)),
                ("ready", C.POINTER(C.c_uint64)), ("gathered", C.POINTER(C.c_uint64))]   # streaming hand-over (rh_decode): NULL = off


def make_opts(device: int = -1, kernel: int = 0, stream=None, devices=None, chunk_rows: int = 0):
    """-> (RhOpts, keepalive).  `devices`: sequence of HIP ordinals to shard the chunks over (repeats allowed);
    per-shard stats land in keepalive["device_stats"]."""
    o = RhOpts()
    o.struct_size = C.sizeof(RhOpts)
    o.device, o.flags, o.stream = device, kernel, stream or None
    o.chunk_rows = chunk_rows
    keep = {}
    if devices:
        arr = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        st = (RhStats * len(devices))()
        o.devices = C.cast(arr, C.POINTER(C.c_int32))
        o.n_devices = len(devices)
        o.device_stats = C.cast(st, C.POINTER(RhStats))
        keep["devices"], keep["device_stats"] = arr, st
    return o, keep


class ArrowArray(C.Structure):
    pass


ArrowArray._fields_ = [("length", C.c_int64), ("null_count", C.c_int64), ("offset", C.c_int64),
                       ("n_buffers", C.c_int64), ("n_children", C.c_int64), ("buffers", C.POINTER(C.c_void_p)),
                       ("children", C.POINTER(C.POINTER(ArrowArray))), ("dictionary", C.POINTER(ArrowArray)),
                       ("release", C.c_void_p), ("private_data", C.c_void_p)]


class ArrowSchema(C.Structure):
    pass


ArrowSchema._fields_ = [("format", C.c_char_p), ("name", C.c_char_p), ("metadata", C.c_void_p), ("flags", C.c_int64),
                        ("n_children", C.c_int64), ("children", C.POINTER(C.POINTER(ArrowSchema))),
                        ("dictionary", C.POINTER(ArrowSchema)), ("release", C.c_void_p), ("private_data", C.c_void_p)]


class ArrowDeviceArray(C.Structure):
    _fields_ = [("array", ArrowArray), ("device_id", C.c_int64), ("device_type", C.c_int32),
                ("sync_event", C.c_void_p), ("reserved", C.c_int64 * 3)]


_lib = None


def lib():
    """Load libruhvro_hip.so (raises OSError if it was not built -- there is no fallback)."""
    global _lib
    if _lib is None:
        L = C.CDLL(LIB_PATH)
        L.rh_schema_compile.restype = C.c_void_p
        L.rh_schema_compile.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_char_p)]
        L.rh_schema_free.argtypes = [C.c_void_p]
        L.rh_schema_project.restype = C.c_void_p      # (no ABI version bump: present in every build that has projection)
        L.rh_schema_project.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_char_p)]
        L.rh_schema_resolve.restype = C.c_void_p      # (likewise: present in every build that has reader schemas)
        L.rh_schema_resolve.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_char_p)]
        L.rh_schema_export.argtypes = [C.c_void_p, C.POINTER(ArrowSchema)]
        L.rh_clamp_chunks.restype = C.c_uint32
        L.rh_clamp_chunks.argtypes = [C.c_uint64, C.c_uint64]
        L.rh_shard_chunks.restype = None
        L.rh_shard_chunks.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.rh_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(RhOpts),
                                C.POINTER(ArrowArray), C.POINTER(C.c_uint32), C.POINTER(RhStats), C.POINTER(C.c_char_p)]
        L.rh_decode_packed.argtypes = L.rh_decode.argtypes
        L.rh_decode_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                                       C.POINTER(RhOpts), C.POINTER(C.c_void_p), C.POINTER(RhStats),
                                       C.POINTER(C.c_char_p)]
        L.rh_device_result_wait.argtypes = [C.c_void_p, C.POINTER(RhStats), C.POINTER(C.c_char_p)]
        L.rh_device_result_chunks.restype = C.c_uint32
        L.rh_device_result_chunks.argtypes = [C.c_void_p]
        L.rh_device_result_output_bytes.restype = C.c_uint64
        L.rh_device_result_output_bytes.argtypes = [C.c_void_p]
        L.rh_device_result_export.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(ArrowDeviceArray)]
        L.rh_device_result_to_host.argtypes = [C.c_void_p, C.POINTER(ArrowArray), C.POINTER(C.c_char_p)]
        L.rh_device_result_free.argtypes = [C.c_void_p]
        L.rh_device_result_buffers.restype = C.c_uint32
        L.rh_device_result_buffers.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint32]
        L.rh_free_string.argtypes = [C.c_void_p]
        L.rh_schema_kernel_source.restype = C.c_void_p
        L.rh_schema_kernel_source.argtypes = [C.c_void_p]
        L.rh_schema_encode_kernel_source.restype = C.c_void_p
        L.rh_schema_encode_kernel_source.argtypes = [C.c_void_p]
        L.rh_schema_kernel_key.restype = C.c_void_p
        L.rh_schema_kernel_key.argtypes = [C.c_void_p, C.c_int]
        L.rh_schema_prebuild.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_char_p)]
        L.rh_schema_kernels_ready.restype = C.c_int
        L.rh_schema_kernels_ready.argtypes = [C.c_void_p, C.c_int, C.c_long, C.POINTER(C.c_char_p)]
        L.rh_abi_version.restype = C.c_int
        L.rh_current_device.restype = C.c_int
        L.rh_device_count.restype = C.c_int
        L.rh_encode_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(RhOpts), C.POINTER(C.c_void_p),
                                       C.POINTER(RhStats), C.POINTER(C.c_char_p)]
        L.rh_device_encoded_chunks.restype = C.c_uint32
        L.rh_device_encoded_chunks.argtypes = [C.c_void_p]
        L.rh_device_encoded_output_bytes.restype = C.c_uint64
        L.rh_device_encoded_output_bytes.argtypes = [C.c_void_p]
        L.rh_device_encoded_export.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(ArrowDeviceArray)]
        L.rh_device_encoded_to_host.argtypes = [C.c_void_p, C.POINTER(ArrowArray), C.POINTER(C.c_char_p)]
        L.rh_device_encoded_free.argtypes = [C.c_void_p]
        L.rh_engine_counters.restype = C.c_uint32
        L.rh_engine_counters.argtypes = [C.POINTER(C.c_uint64), C.c_uint32]
        # tolerant decode (no ABI version bump: present in every build that has it)
        L.rh_schema_placeholder.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.rh_record_errors_count.restype = C.c_uint64
        L.rh_record_errors_count.argtypes = [C.c_void_p]
        L.rh_record_errors_get.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_char_p)]
        L.rh_record_errors_free.argtypes = [C.c_void_p]
        L.rh_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(RhOpts), C.c_uint64,
                                  C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_char_p)]
        L.rh_validate_packed.argtypes = L.rh_validate.argtypes
        L.rh_validate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(RhOpts), C.c_uint64,
                                         C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_char_p)]
        L.rh_decode_tolerant.argtypes = L.rh_decode.argtypes + [C.c_uint64, C.POINTER(C.c_void_p)]
        L.rh_decode_packed_tolerant.argtypes = L.rh_decode_tolerant.argtypes
        L.rh_decode_device_tolerant.argtypes = L.rh_decode_device.argtypes + [C.c_uint64, C.POINTER(C.c_void_p)]
        _lib = L
    return _lib


ENGINE_COUNTERS = ("fused_calls", "two_sync_calls", "capacity_retries", "wide_fallbacks", "offset32_errors", "split_calls", "single_pass_calls", "single_pass_failovers", "background_compiles",
                   "tiles", "careful_tiles", "over_window_tiles", "rewalked_waves", "subtiled_tiles", "ranged_retries",
                   "tolerant_calls", "tolerant_repairs")


def engine_counters() -> dict:
    """Process-wide counters of the engine's rarely taken branches (rh_engine_counters), by name."""
    buf = (C.c_uint64 * len(ENGINE_COUNTERS))()
    n = lib().rh_engine_counters(buf, len(ENGINE_COUNTERS))
    assert n == len(ENGINE_COUNTERS)
    return {name: int(buf[i]) for i, name in enumerate(ENGINE_COUNTERS)}


def _take_err(err: C.c_char_p) -> str:
    msg = err.value.decode("utf-8", "replace") if err.value else "ruhvro_hip error"
    if err.value is not None:
        lib().rh_free_string(C.cast(err, C.c_void_p))
    return msg


def _raise(rc: int, err: C.c_char_p):
    msg = _take_err(err)
    if rc in (RH_ERR_SCHEMA, RH_ERR_DECODE, RH_ERR_ARGUMENT):
        raise ValueError(msg)
    raise RuntimeError(msg)


def check_columns(columns):
    """The `columns=` argument of the decode entry points -> None (every column) or a tuple of distinct str.  Raises
    ValueError naming the offender (empty list, a non-str entry, a duplicate) before any native call; unknown and dotted
    names are refused by rh_schema_project, which knows the schema."""
    if columns is None:
        return None
    if isinstance(columns, (str, bytes)):
        raise ValueError(f"columns: expected a list of top-level field names, got {columns!r}")
    cols = tuple(columns)
    if not cols:
        raise ValueError("columns: the projection is empty (name at least one top-level field, or pass None for all)")
    seen = set()
    for i, c in enumerate(cols):
        if not isinstance(c, str):
            raise ValueError(f"columns: entry {i} ({c!r}) is not a str")
        if c in seen:
            raise ValueError(f"columns: duplicate field '{c}'")
        seen.add(c)
    return cols


def check_reader_schema(reader_schema):
    """The `reader_schema=` argument of the strict decode entry points -> None or the Avro JSON text."""
    if reader_schema is not None and not isinstance(reader_schema, str):
        raise TypeError("argument 'reader_schema': expected str or None")
    return reader_schema


def refuse_reader_schema(reader_schema, what: str):
    """The entry points that do not resolve (tolerant decode, validation, encode) say so before any native work."""
    if reader_schema is not None:
        raise ValueError(f"reader schema: {what} does not take reader_schema= (schema resolution is strict-decode only)")


def reader_columns(reader_schema: str, columns) -> str:
    """`columns=` composed with `reader_schema=`: the reader schema with its top-level fields pruned to `columns` and put in
    that order, so that the resolved decode equals the whole reader's decode followed by ``.select(columns)``."""
    if columns is None:
        return reader_schema
    import json
    try:
        j = json.loads(reader_schema)
    except ValueError as e:
        raise ValueError(f"reader schema: Failed to parse schema from JSON: {e}") from None
    if not isinstance(j, dict) or not isinstance(j.get("fields"), list):
        raise ValueError("reader schema: the top-level schema must be a record")
    by_name = {f.get("name"): f for f in j["fields"] if isinstance(f, dict)}
    for c in columns:
        if c not in by_name:
            if "." in c:
                raise ValueError(f"columns: '{c}' is a dotted path: only top-level fields can be selected")
            raise ValueError(f"columns: unknown top-level field '{c}' of the reader schema")
    j["fields"] = [by_name[c] for c in columns]
    return json.dumps(j)


class Schema:
    """Compiled schema handle (rh_schema*) + the pyarrow schema of its batches.  `columns`: the projection onto those
    top-level fields (rh_schema_project), an independent schema with its own kernels and size history.  `reader_schema`:
    `schema_json` is the writer's and the batches are the reader's (rh_schema_resolve); `columns` then names reader fields."""

    _cache: dict = {}

    def __init__(self, schema_json: str, columns=None, reader_schema=None):
        L = lib()
        err = C.c_char_p()
        if reader_schema is not None:
            raw = reader_columns(reader_schema, columns).encode()
            self.handle = L.rh_schema_resolve(Schema.get(schema_json).handle, raw, len(raw), C.byref(err))
        elif columns is None:
            raw = schema_json.encode()
            self.handle = L.rh_schema_compile(raw, len(raw), C.byref(err))
        else:
            names = (C.c_char_p * len(columns))(*[c.encode() for c in columns])
            self.handle = L.rh_schema_project(Schema.get(schema_json).handle, names, len(columns), C.byref(err))
        if not self.handle:
            _raise(RH_ERR_SCHEMA, err)
        cs = ArrowSchema()
        if L.rh_schema_export(self.handle, C.byref(cs)) != RH_OK:
            raise RuntimeError("rh_schema_export failed")
        st = pa.DataType._import_from_c(C.addressof(cs))
        self.arrow_schema = pa.schema(list(st))

    @classmethod
    def get(cls, schema_json: str, columns=None, reader_schema=None) -> "Schema":
        columns = check_columns(columns)
        reader_schema = check_reader_schema(reader_schema)
        key = (schema_json if columns is None else (schema_json, columns)) if reader_schema is None else (schema_json, reader_schema, columns)
        s = cls._cache.get(key)
        if s is None:
            s = cls._cache[key] = cls(schema_json, columns, reader_schema)
        return s


def _import_chunks(arr, k: int, schema: pa.Schema) -> List[pa.RecordBatch]:
    return [pa.RecordBatch._import_from_c(C.addressof(arr[i]), schema) for i in range(k)]


KERNEL_AUTO, KERNEL_GENERIC, KERNEL_SPECIALIZED = 0, 1, 2
RH_TWO_PASS = 16  # rh_opts.flags: rh_decode_device takes the two-pass form (size pass, scan, emit pass) even where the single-pass form would run
RH_SINGLE_PASS = 32  # rh_opts.flags: rh_decode_device prefers the single-pass form (one kernel sizes, scans across tiles, emits)
RH_ASYNC = 8      # rh_opts.flags: rh_decode_device returns once the call is on the stream (rh_device_result_wait settles it)


def kernel_source(schema_json: str, columns=None, reader_schema=None) -> str:
    """HIP source of the schema-specialised kernels (rh_schema_kernel_source)."""
    L = lib()
    p = L.rh_schema_kernel_source(Schema.get(schema_json, columns, reader_schema).handle)
    if not p:
        raise RuntimeError("rh_schema_kernel_source failed")
    try:
        return C.string_at(p).decode()
    finally:
        L.rh_free_string(p)


def kernel_key(schema_json: str, encode: bool = False, columns=None, reader_schema=None) -> str:
    """Content hash of the schema's specialised kernel pair (rh_schema_kernel_key): the kernel-cache key."""
    L = lib()
    p = L.rh_schema_kernel_key(Schema.get(schema_json, columns, reader_schema).handle, 1 if encode else 0)
    if not p:
        raise RuntimeError("rh_schema_kernel_key failed")
    try:
        return C.string_at(p).decode()
    finally:
        L.rh_free_string(p)


# The lean pair (include/ruhvro_hip.h): symbols added without a change of the ABI version, so they are looked up by name
# when first asked for -- a library built before them answers "no lean pair".
LEAN_COUNTERS = ("lean_calls", "probes", "probes_clean", "probes_dirty", "fallbacks", "reruns", "need_ranged", "need_wide_index",
                 "two_pass_repeats", "capacity_tails", "async_settled")
LEAN_NONE, LEAN_UNDECIDED, LEAN_LEAN, LEAN_WIDE = -1, 0, 1, 2


def _lean_sym(name: str, restype, argtypes):
    f = getattr(lib(), name, None)          # (ctypes: dlsym)
    if f is not None:
        f.restype, f.argtypes = restype, argtypes
    return f


def _lean_string(name: str, schema_json: str, columns=None, reader_schema=None):
    f = _lean_sym(name, C.c_void_p, [C.c_void_p])
    p = f(Schema.get(schema_json, columns, reader_schema).handle) if f else None
    if not p:
        return None
    try:
        return C.string_at(p).decode()
    finally:
        lib().rh_free_string(p)


def lean_kernel_source(schema_json: str, columns=None, reader_schema=None):
    """HIP source of the schema's lean pair (rh_schema_lean_kernel_source), or None when the schema has none."""
    return _lean_string("rh_schema_lean_kernel_source", schema_json, columns, reader_schema)


def lean_kernel_key(schema_json: str, columns=None, reader_schema=None):
    """Kernel-cache key of the lean source (rh_schema_lean_kernel_key), or None."""
    return _lean_string("rh_schema_lean_kernel_key", schema_json, columns, reader_schema)


def lean_state(schema_json: str, device: int = 0, columns=None, reader_schema=None) -> int:
    """rh_schema_lean_state: LEAN_NONE / LEAN_UNDECIDED / LEAN_LEAN / LEAN_WIDE of this schema on `device`."""
    f = _lean_sym("rh_schema_lean_state", C.c_int, [C.c_void_p, C.c_int])
    return int(f(Schema.get(schema_json, columns, reader_schema).handle, device)) if f else LEAN_NONE


def lean_ready(schema_json: str, timeout_ms: int = 0) -> bool:
    """rh_schema_lean_ready: True when the lean pair's code objects are there."""
    f = _lean_sym("rh_schema_lean_ready", C.c_int, [C.c_void_p, C.c_long, C.POINTER(C.c_char_p)])
    if f is None:
        return False
    err = C.c_char_p()
    rc = f(Schema.get(schema_json).handle, int(timeout_ms), C.byref(err))
    if rc == -1:
        _raise(RH_ERR_RUNTIME, err)
    return rc == 1


def lean_counters() -> dict:
    """rh_lean_counters by name: the roads of the lean pair (none of them moves rh_engine_counters)."""
    f = _lean_sym("rh_lean_counters", C.c_uint32, [C.POINTER(C.c_uint64), C.c_uint32])
    buf = (C.c_uint64 * len(LEAN_COUNTERS))()
    if f is not None:
        assert f(buf, len(LEAN_COUNTERS)) == len(LEAN_COUNTERS)
    return {name: int(buf[i]) for i, name in enumerate(LEAN_COUNTERS)}


def encode_kernel_source(schema_json: str) -> str:
    """HIP source of the schema-specialised Arrow -> Avro kernels (rh_schema_encode_kernel_source)."""
    L = lib()
    p = L.rh_schema_encode_kernel_source(Schema.get(schema_json).handle)
    if not p:
        raise RuntimeError("rh_schema_encode_kernel_source failed")
    try:
        return C.string_at(p).decode()
    finally:
        L.rh_free_string(p)


def prebuild(schema_json: str, columns=None, reader_schema=None) -> bool:
    """Compile the schema-specialised kernels into the on-disk kernel cache (hiprtc; no GPU needed).
    Returns True when the code object was already cached."""
    L = lib()
    cached = C.c_int()
    err = C.c_char_p()
    rc = L.rh_schema_prebuild(Schema.get(schema_json, columns, reader_schema).handle, C.byref(cached), C.byref(err))
    if rc != RH_OK:
        _raise(rc, err)
    return bool(cached.value)


def kernels_ready(schema_json: str, encode: bool = False, timeout_ms: int = 0, columns=None, reader_schema=None) -> bool:
    """rh_schema_kernels_ready: True when the schema's specialised kernels are there (the next call runs on them), False while
    their compile jobs are still running after `timeout_ms` (or nobody asked for them); raises when the compile failed."""
    err = C.c_char_p()
    rc = lib().rh_schema_kernels_ready(Schema.get(schema_json, columns, reader_schema).handle, 1 if encode else 0, int(timeout_ms), C.byref(err))
    if rc < 0:
        _raise(RH_ERR_RUNTIME, err)
    return rc == 1


def shard_chunks(n: int, num_chunks: int, n_shards: int, shard: int):
    """rh_shard_chunks -> (chunk_lo, chunk_hi, row_lo, row_hi): the multi-GPU deal of whole reference chunks."""
    c0, c1, r0, r1 = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64()
    lib().rh_shard_chunks(n, num_chunks, n_shards, shard, C.byref(c0), C.byref(c1), C.byref(r0), C.byref(r1))
    return c0.value, c1.value, r0.value, r1.value


def decode_packed(data: np.ndarray, offsets: np.ndarray, schema_json: str, num_chunks: int,
                  device: int = -1, want_stats: bool = False, kernel: int = KERNEL_AUTO, devices=None, *, columns=None, reader_schema=None,
                  where=None):
    """rh_decode_packed: one contiguous payload + u64 offsets (host memory) -> list[RecordBatch].
    `devices`: shard the chunks over these HIP devices (rh_opts.devices); with want_stats the stats dict then carries
    the per-shard stats under "device_stats".  `where`: rh_decode_packed_where (a row filter, see check_where)."""
    L = lib()
    flt = Filter.get(schema_json, where) if where is not None else None      # ValueError "where: ..." before any device work
    s = Schema.get(schema_json, columns, reader_schema)
    data = np.ascontiguousarray(data, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    k = L.rh_clamp_chunks(n, num_chunks)
    arr = (ArrowArray * k)()
    out_k = C.c_uint32()
    st = RhStats()
    err = C.c_char_p()
    opts, keep = make_opts(device, kernel, None, devices)
    if flt is not None:
        rc = _filter_sym("rh_decode_packed_where")(s.handle, data.ctypes.data, offsets.ctypes.data, n, num_chunks, C.byref(opts), arr,
                                                   C.byref(out_k), C.byref(st), C.byref(err), flt.handle, None)
    else:
        rc = L.rh_decode_packed(s.handle, data.ctypes.data, offsets.ctypes.data, n, num_chunks, C.byref(opts), arr,
                                C.byref(out_k), C.byref(st), C.byref(err))
    if rc != RH_OK:
        _raise(rc, err)
    out = _import_chunks(arr, out_k.value, s.arrow_schema)
    if not want_stats:
        return out
    d = st.as_dict()
    if devices:
        d["device_stats"] = [x.as_dict() for x in keep["device_stats"]]
    return out, d


def decode_slices(ptrs: np.ndarray, lens: np.ndarray, schema_json: str, num_chunks: int,
                  device: int = -1, want_stats: bool = False, kernel: int = KERNEL_AUTO, devices=None, *, columns=None, reader_schema=None,
                  where=None):
    """rh_decode: one (pointer, length) pair per record, the form the CPython boundary extracts from list[bytes]
    (u64 addresses / u64 lengths; the caller keeps the pointed-to memory alive) -> list[RecordBatch].  `where`: rh_decode_where."""
    L = lib()
    flt = Filter.get(schema_json, where) if where is not None else None
    s = Schema.get(schema_json, columns, reader_schema)
    ptrs = np.ascontiguousarray(ptrs, dtype=np.uint64)
    lens = np.ascontiguousarray(lens, dtype=np.uint64)
    n = len(ptrs)
    k = L.rh_clamp_chunks(n, num_chunks)
    arr = (ArrowArray * k)()
    out_k = C.c_uint32()
    st = RhStats()
    err = C.c_char_p()
    opts, keep = make_opts(device, kernel, None, devices)
    if flt is not None:
        rc = _filter_sym("rh_decode_where")(s.handle, ptrs.ctypes.data, lens.ctypes.data, n, num_chunks, C.byref(opts), arr,
                                            C.byref(out_k), C.byref(st), C.byref(err), flt.handle, None)
    else:
        rc = L.rh_decode(s.handle, ptrs.ctypes.data, lens.ctypes.data, n, num_chunks, C.byref(opts), arr,
                         C.byref(out_k), C.byref(st), C.byref(err))
    if rc != RH_OK:
        _raise(rc, err)
    out = _import_chunks(arr, out_k.value, s.arrow_schema)
    return (out, st.as_dict()) if want_stats else out


# Row filters (include/ruhvro_hip.h): symbols added without a change of the ABI version, looked up by name.
class RhFilterTerm(C.Structure):
    _fields_ = [("name", C.c_char_p), ("op", C.c_char_p), ("value_kind", C.c_int32), ("reserved", C.c_int32), ("i", C.c_int64),
                ("d", C.c_double), ("bytes", C.c_char_p), ("len", C.c_uint64)]


FILTER_VALUE_NONE, FILTER_VALUE_INT, FILTER_VALUE_DOUBLE, FILTER_VALUE_BOOL, FILTER_VALUE_BYTES, FILTER_VALUE_BIGINT = range(6)
FILTER_SYMBOLS = ("rh_filter_compile", "rh_filter_free", "rh_filter_packed", "rh_filter_device", "rh_decode_where",
                  "rh_decode_packed_where", "rh_decode_device_where", "rh_filter_last")


def _filter_sym(name: str):
    f = getattr(lib(), name, None)          # (ctypes: dlsym)
    if f is None:
        raise RuntimeError(f"libruhvro_hip.so has no {name}: the library was built before row filters")
    if f.argtypes is None:
        L = lib()
        f.restype, f.argtypes = {
            "rh_filter_compile": (C.c_int, [C.c_void_p, C.POINTER(RhFilterTerm), C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_char_p)]),
            "rh_filter_free": (None, [C.c_void_p]),
            "rh_filter_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(RhOpts), C.c_void_p,
                                           C.POINTER(C.c_uint64), C.POINTER(C.c_char_p)]),
            "rh_filter_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(RhOpts), C.c_void_p,
                                           C.POINTER(C.c_uint64), C.POINTER(C.c_char_p)]),
            "rh_decode_where": (C.c_int, L.rh_decode.argtypes + [C.c_void_p, C.POINTER(C.c_uint64)]),
            "rh_decode_packed_where": (C.c_int, L.rh_decode.argtypes + [C.c_void_p, C.POINTER(C.c_uint64)]),
            "rh_decode_device_where": (C.c_int, L.rh_decode_device.argtypes + [C.c_void_p, C.POINTER(C.c_uint64)]),
            "rh_filter_last": (None, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        }[name]
    return f


def check_where(where):
    """The `where=` argument of the strict decode entry points -> None (no filter) or a tuple of terms (name, op, value).
    One term ``(name, op, value)`` / ``(name, "is_null")`` or a list / tuple of terms, ANDed.  TypeError for anything that is
    not a tuple or a list; ValueError ("where: ...") for a term of another shape.  What the terms may say is decided by
    rh_filter_compile, which knows the schema."""
    if where is None:
        return None
    if not isinstance(where, (tuple, list)):
        raise TypeError("argument 'where': expected a term (name, op, value) or a list of terms, or None")
    terms = [where] if (len(where) in (2, 3) and isinstance(where[0], str)) else list(where)
    out = []
    for k, t in enumerate(terms):
        if not isinstance(t, (tuple, list)) or len(t) not in (2, 3) or not isinstance(t[0], str) or not isinstance(t[1], str):
            raise ValueError(f"where: term {k} ({t!r}) is not (name, op, value) or (name, 'is_null' / 'not_null')")
        out.append((t[0], t[1], t[2] if len(t) == 3 else None))
    return tuple(out)


def _filter_term(name: str, op: str, value) -> RhFilterTerm:
    t = RhFilterTerm()
    t.name, t.op = name.encode(), op.encode()
    if value is None:
        t.value_kind = FILTER_VALUE_NONE
    elif isinstance(value, (bool, np.bool_)):
        t.value_kind, t.i = FILTER_VALUE_BOOL, int(bool(value))
    elif isinstance(value, (int, np.integer)):
        value = int(value)
        try:
            t.d = float(value)
        except OverflowError:
            t.d = float("inf") if value > 0 else float("-inf")
        if -(1 << 63) <= value < (1 << 63):
            t.value_kind, t.i = FILTER_VALUE_INT, value
        else:
            t.value_kind = FILTER_VALUE_BIGINT
    elif isinstance(value, (float, np.floating)):
        t.value_kind, t.d = FILTER_VALUE_DOUBLE, float(value)
    elif isinstance(value, (str, bytes, bytearray)):
        raw = value.encode("utf-8") if isinstance(value, str) else bytes(value)
        t.value_kind, t.bytes, t.len = FILTER_VALUE_BYTES, raw, len(raw)
    else:
        raise ValueError(f"where: field '{name}': a value of type {type(value).__name__} cannot be compared with")
    return t


class Filter:
    """Compiled predicate (rh_filter*) of one writer schema; cached by (schema, terms)."""

    _cache: dict = {}

    def __init__(self, schema_json: str, terms):
        arr = (RhFilterTerm * max(len(terms), 1))(*[_filter_term(*t) for t in terms])
        out, err = C.c_void_p(), C.c_char_p()
        rc = _filter_sym("rh_filter_compile")(Schema.get(schema_json).handle, arr, len(terms), C.byref(out), C.byref(err))
        if rc != RH_OK:
            _raise(rc, err)
        self.handle = out.value

    @classmethod
    def get(cls, schema_json: str, where) -> "Filter":
        terms = check_where(where)
        if terms is None:
            raise ValueError("where: no predicate")
        key = (schema_json, tuple((n, o, type(v).__name__, repr(v)) for n, o, v in terms))
        f = cls._cache.get(key)
        if f is None:
            f = cls._cache[key] = cls(schema_json, terms)
        return f


def _keep_mask(words: np.ndarray, n: int) -> np.ndarray:
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)


def filter_packed(data: np.ndarray, offsets: np.ndarray, schema_json: str, where, device: int = -1, devices=None) -> np.ndarray:
    """rh_filter_packed: the filter kernel alone -> numpy bool[n], True where the record is kept.  A malformed record raises
    the strict decode's message for the lowest failing record."""
    flt = Filter.get(schema_json, where)
    data = np.ascontiguousarray(data, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    words = np.zeros(max((n + 63) // 64, 1), dtype=np.uint64)
    kept, err = C.c_uint64(), C.c_char_p()
    opts, _keep = make_opts(device, 0, None, devices)
    rc = _filter_sym("rh_filter_packed")(flt.handle, data.ctypes.data, offsets.ctypes.data, n, C.byref(opts), words.ctypes.data,
                                         C.byref(kept), C.byref(err))
    if rc != RH_OK:
        _raise(rc, err)
    mask = _keep_mask(words, n)
    assert int(mask.sum()) == kept.value
    return mask


def filter_device(d_data: int, d_offsets: int, data_len: int, n: int, schema_json: str, where, device: int = -1, stream: int = 0) -> np.ndarray:
    """rh_filter_device on raw device pointers -> numpy bool[n] (host memory)."""
    flt = Filter.get(schema_json, where)
    words = np.zeros(max((n + 63) // 64, 1), dtype=np.uint64)
    kept, err = C.c_uint64(), C.c_char_p()
    opts, _keep = make_opts(device, 0, stream, None)
    rc = _filter_sym("rh_filter_device")(flt.handle, d_data, d_offsets, data_len, n, C.byref(opts), words.ctypes.data, C.byref(kept),
                                         C.byref(err))
    if rc != RH_OK:
        _raise(rc, err)
    return _keep_mask(words, n)


def filter_last() -> dict:
    """rh_filter_last: the most recent filtered call of this process."""
    f_ms, g_ms, n, kept = C.c_float(), C.c_float(), C.c_uint64(), C.c_uint64()
    _filter_sym("rh_filter_last")(C.byref(f_ms), C.byref(g_ms), C.byref(n), C.byref(kept))
    return {"filter_ms": f_ms.value, "gather_ms": g_ms.value, "n": int(n.value), "kept": int(kept.value)}


# Framed messages (include/ruhvro_hip.h): symbols added without a change of the ABI version, looked up by name.
FRAMINGS = {"confluent": 0, "single_object": 1}
FRAME_SKIP_UNKNOWN, FRAME_CLASSIFY_ONLY = 1, 2
FRAME_UNKNOWN = 0xFD      # the verdict byte of a well-framed message whose id is not in the call's list
FRAME_SYMBOLS = ("rh_frame_split_packed", "rh_frame_split_device", "rh_frame_split_count", "rh_frame_split_classes",
                 "rh_frame_split_indices", "rh_frame_decode_class", "rh_frame_split_free", "rh_frame_last")


def _frame_sym(name: str):
    f = getattr(lib(), name, None)
    if f is None:
        raise RuntimeError(f"libruhvro_hip.so has no {name}: the library was built before framed messages")
    if f.argtypes is None:
        tail = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(RhOpts), C.POINTER(C.c_void_p), C.POINTER(C.c_char_p)]
        f.restype, f.argtypes = {
            "rh_frame_split_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64] + tail),
            "rh_frame_split_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64] + tail),
            "rh_frame_split_count": (C.c_uint64, [C.c_void_p, C.c_uint32]),
            "rh_frame_split_classes": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p)]),
            "rh_frame_split_indices": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_char_p)]),
            "rh_frame_decode_class": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(RhOpts), C.POINTER(ArrowArray),
                                                C.POINTER(C.c_uint32), C.POINTER(RhStats), C.POINTER(C.c_char_p)]),
            "rh_frame_split_free": (None, [C.c_void_p]),
            "rh_frame_last": (None, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint64)]),
        }[name]
    return f


class FrameSplit:
    """rh_frame_split*: framed messages checked, partitioned by wire id and stripped of their headers on the device.  `ids`: the
    call's wire ids, ascending and distinct (unsigned).  Class c is the messages that carry ids[c]; class len(ids) the messages
    of unknown ids (only with FRAME_SKIP_UNKNOWN; indices, no payload)."""

    def __init__(self, handle, n: int, ids, flags: int):
        self.handle, self.n, self.ids, self.flags = handle, n, tuple(ids), flags

    @classmethod
    def _make(cls, sym: str, lead, n: int, ids, framing: int, flags: int, device: int, kernel: int, devices, stream=None):
        arr = np.ascontiguousarray(ids, dtype=np.uint64)
        out, err = C.c_void_p(), C.c_char_p()
        opts, _keep = make_opts(device, kernel, stream, devices)
        rc = _frame_sym(sym)(*lead, n, arr.ctypes.data, len(arr), framing, flags, C.byref(opts), C.byref(out), C.byref(err))
        if rc != RH_OK:
            _raise(rc, err)
        return cls(out.value, n, [int(x) for x in arr], flags)

    @classmethod
    def packed(cls, data: np.ndarray, offsets: np.ndarray, ids, framing: int, flags: int = 0, device: int = -1, kernel: int = 0,
               devices=None) -> "FrameSplit":
        """rh_frame_split_packed: one contiguous payload + u64 offsets (host memory)."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        return cls._make("rh_frame_split_packed", (data.ctypes.data, offsets.ctypes.data), len(offsets) - 1, ids, framing, flags, device,
                         kernel, devices)

    @classmethod
    def device(cls, d_data: int, d_offsets: int, data_len: int, n: int, ids, framing: int, flags: int = 0, device: int = -1,
               stream: int = 0) -> "FrameSplit":
        """rh_frame_split_device on raw device pointers (rh_decode_device's input)."""
        return cls._make("rh_frame_split_device", (d_data, d_offsets, data_len), n, ids, framing, flags, device, 0, None, stream)

    def count(self, c: int) -> int:
        return int(_frame_sym("rh_frame_split_count")(self.handle, c))

    def classes(self) -> np.ndarray:
        """numpy int16[n]: the class of every message, -1 for an unknown id."""
        raw = np.zeros(max(self.n, 1), dtype=np.uint8)
        err = C.c_char_p()
        rc = _frame_sym("rh_frame_split_classes")(self.handle, raw.ctypes.data, C.byref(err))
        if rc != RH_OK:
            _raise(rc, err)
        out = raw[:self.n].astype(np.int16)
        out[raw[:self.n] == FRAME_UNKNOWN] = -1
        return out

    def indices(self, c: int) -> np.ndarray:
        """numpy int64[count(c)]: class c's ascending positions in the input."""
        out = np.zeros(self.count(c), dtype=np.int64)
        err = C.c_char_p()
        rc = _frame_sym("rh_frame_split_indices")(self.handle, c, out.ctypes.data, C.byref(err))
        if rc != RH_OK:
            _raise(rc, err)
        return out

    def decode(self, c: int, schema_json: str, num_chunks: int, device: int = -1, kernel: int = KERNEL_AUTO, want_stats: bool = False, *,
               columns=None, reader_schema=None):
        """rh_frame_decode_class: the strict decode of class c's payloads with its schema -> list[RecordBatch].  Once per class."""
        s = Schema.get(schema_json, columns, reader_schema)
        k = lib().rh_clamp_chunks(self.count(c), num_chunks)
        arr = (ArrowArray * k)()
        out_k, st, err = C.c_uint32(), RhStats(), C.c_char_p()
        opts, _keep = make_opts(device, kernel, None, None)
        rc = _frame_sym("rh_frame_decode_class")(self.handle, c, s.handle, num_chunks, C.byref(opts), arr, C.byref(out_k), C.byref(st),
                                                 C.byref(err))
        if rc != RH_OK:
            _raise(rc, err)
        out = _import_chunks(arr, out_k.value, s.arrow_schema)
        return (out, st.as_dict()) if want_stats else out

    def free(self):
        if self.handle:
            _frame_sym("rh_frame_split_free")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def frame_last() -> dict:
    """rh_frame_last: GPU time of the most recent split of this process, kernel by kernel."""
    c_ms, s_ms, g_ms, n = C.c_float(), C.c_float(), C.c_float(), C.c_uint64()
    _frame_sym("rh_frame_last")(C.byref(c_ms), C.byref(s_ms), C.byref(g_ms), C.byref(n))
    return {"classify_ms": c_ms.value, "scan_offsets_ms": s_ms.value, "gather_ms": g_ms.value, "n": int(n.value)}


# One malformed record of a tolerant / validation call: its index in the call's input and the message the strict call raises
# when that record is the lowest failing one.
RecordError = namedtuple("RecordError", ["index", "message"])


def placeholder_datum(schema_json: str) -> bytes:
    """rh_schema_placeholder: the datum a tolerant call puts in the place of a malformed record."""
    p, n = C.c_void_p(), C.c_uint64()
    if lib().rh_schema_placeholder(Schema.get(schema_json).handle, C.byref(p), C.byref(n)) != RH_OK:
        raise RuntimeError("rh_schema_placeholder failed")
    return C.string_at(p, n.value) if n.value else b""


def _take_errors(handle: C.c_void_p) -> list:
    """An rh_record_errors list -> [RecordError]; frees the list."""
    L = lib()
    if not handle.value:
        return []
    try:
        out = []
        idx, code, msg = C.c_uint64(), C.c_int(), C.c_char_p()
        for i in range(L.rh_record_errors_count(handle)):
            if L.rh_record_errors_get(handle, i, C.byref(idx), C.byref(code), C.byref(msg)) != RH_OK:
                raise RuntimeError("rh_record_errors_get failed")
            out.append(RecordError(int(idx.value), msg.value.decode("utf-8", "replace")))
        return out
    finally:
        L.rh_record_errors_free(handle)


def _validate(fn, lead, schema_json: str, max_errors: int, device: int, devices=None, stream=None, want_total: bool = False):
    s = Schema.get(schema_json)
    out, total, err = C.c_void_p(), C.c_uint64(), C.c_char_p()
    opts, _keep = make_opts(device, 0, stream, devices)
    rc = fn(s.handle, *lead, C.byref(opts), max_errors, C.byref(out), C.byref(total), C.byref(err))
    if rc != RH_OK:
        _raise(rc, err)
    errors = _take_errors(out)
    return (errors, int(total.value)) if want_total else errors


def validate_packed(data: np.ndarray, offsets: np.ndarray, schema_json: str, max_errors: int = 1024, device: int = -1,
                    devices=None, want_total: bool = False):
    """rh_validate_packed -> [RecordError] of ALL malformed records (the max_errors lowest when there are more); with
    want_total also their exact number."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    return _validate(lib().rh_validate_packed, (data.ctypes.data, offsets.ctypes.data, len(offsets) - 1), schema_json, max_errors,
                     device, devices, None, want_total)


def validate_slices(ptrs: np.ndarray, lens: np.ndarray, schema_json: str, max_errors: int = 1024, device: int = -1,
                    devices=None, want_total: bool = False):
    """rh_validate: one (pointer, length) pair per record."""
    ptrs = np.ascontiguousarray(ptrs, dtype=np.uint64)
    lens = np.ascontiguousarray(lens, dtype=np.uint64)
    return _validate(lib().rh_validate, (ptrs.ctypes.data, lens.ctypes.data, len(ptrs)), schema_json, max_errors, device, devices,
                     None, want_total)


def validate_device(d_data: int, d_offsets: int, data_len: int, n: int, schema_json: str, max_errors: int = 1024, device: int = -1,
                    stream: int = 0, want_total: bool = False):
    """rh_validate_device on raw device pointers."""
    return _validate(lib().rh_validate_device, (d_data, d_offsets, data_len, n), schema_json, max_errors, device, None, stream,
                     want_total)


def _decode_host_tolerant(fn, a, b, n, schema_json, num_chunks, device, kernel, devices, columns, max_errors, flags=0):
    L = lib()
    s = Schema.get(schema_json, columns)
    k = L.rh_clamp_chunks(n, num_chunks)
    arr = (ArrowArray * k)()
    out_k, st, err, errs = C.c_uint32(), RhStats(), C.c_char_p(), C.c_void_p()
    opts, _keep = make_opts(device, kernel | flags, None, devices)
    rc = fn(s.handle, a, b, n, num_chunks, C.byref(opts), arr, C.byref(out_k), C.byref(st), C.byref(err), max_errors, C.byref(errs))
    if rc != RH_OK:
        _raise(rc, err)
    return _import_chunks(arr, out_k.value, s.arrow_schema), _take_errors(errs)


def decode_packed_tolerant(data: np.ndarray, offsets: np.ndarray, schema_json: str, num_chunks: int, device: int = -1,
                           kernel: int = 0, devices=None, *, columns=None, max_errors: int = 1024, flags: int = 0):
    """rh_decode_packed_tolerant -> (list[RecordBatch], [RecordError]): the strict call's batches with the placeholder datum in
    the place of every malformed record, and all of those records."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    return _decode_host_tolerant(lib().rh_decode_packed_tolerant, data.ctypes.data, offsets.ctypes.data, len(offsets) - 1,
                                 schema_json, num_chunks, device, kernel, devices, columns, max_errors, flags)


def decode_slices_tolerant(ptrs: np.ndarray, lens: np.ndarray, schema_json: str, num_chunks: int, device: int = -1,
                           kernel: int = 0, devices=None, *, columns=None, max_errors: int = 1024, flags: int = 0):
    """rh_decode_tolerant: one (pointer, length) pair per record -> (list[RecordBatch], [RecordError])."""
    ptrs = np.ascontiguousarray(ptrs, dtype=np.uint64)
    lens = np.ascontiguousarray(lens, dtype=np.uint64)
    return _decode_host_tolerant(lib().rh_decode_tolerant, ptrs.ctypes.data, lens.ctypes.data, len(ptrs), schema_json, num_chunks,
                                 device, kernel, devices, columns, max_errors, flags)


class DeviceResult:
    """Owns an rh_device_result (Arrow buffers resident in HBM)."""

    errors: list = []      # a tolerant call's malformed records (decode_device_tolerant); [] for a strict call

    def __init__(self, handle, schema: Schema, stats: dict):
        self.handle = handle
        self.schema = schema
        self.stats = stats

    @property
    def chunks(self) -> int:
        return lib().rh_device_result_chunks(self.handle)

    @property
    def output_bytes(self) -> int:
        return lib().rh_device_result_output_bytes(self.handle)

    def export(self, chunk: int) -> "ArrowDeviceArray":
        """Chunk `chunk` as an ArrowDeviceArray view (device pointers); release it through array.release."""
        out = ArrowDeviceArray()
        if lib().rh_device_result_export(self.handle, chunk, C.byref(out)) != RH_OK:
            raise RuntimeError("rh_device_result_export failed")
        return out

    def wait(self) -> "DeviceResult":
        """rh_device_result_wait: settle an asynchronous call (raises what the synchronous call would have raised)."""
        st = RhStats()
        err = C.c_char_p()
        rc = lib().rh_device_result_wait(self.handle, C.byref(st), C.byref(err))
        if rc != RH_OK:
            _raise(rc, err)
        if getattr(self, "_want_stats", False) and st.records:
            self.stats = st.as_dict()
        return self

    def to_host(self) -> List[pa.RecordBatch]:
        k = self.chunks
        arr = (ArrowArray * k)()
        err = C.c_char_p()
        rc = lib().rh_device_result_to_host(self.handle, arr, C.byref(err))
        if rc != RH_OK:
            _raise(rc, err)
        return _import_chunks(arr, k, self.schema.arrow_schema)

    def free(self):
        if self.handle:
            lib().rh_device_result_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceEncoded:
    """Owns an rh_device_encoded (k BinaryArrays of Avro datums resident in HBM)."""

    def __init__(self, handle, stats: dict):
        self.handle = handle
        self.stats = stats

    @property
    def chunks(self) -> int:
        return lib().rh_device_encoded_chunks(self.handle)

    @property
    def output_bytes(self) -> int:
        return lib().rh_device_encoded_output_bytes(self.handle)

    def export(self, chunk: int) -> "ArrowDeviceArray":
        out = ArrowDeviceArray()
        if lib().rh_device_encoded_export(self.handle, chunk, C.byref(out)) != RH_OK:
            raise RuntimeError("rh_device_encoded_export failed")
        return out

    def to_host(self) -> List[pa.Array]:
        k = self.chunks
        arr = (ArrowArray * k)()
        err = C.c_char_p()
        rc = lib().rh_device_encoded_to_host(self.handle, arr, C.byref(err))
        if rc != RH_OK:
            _raise(rc, err)
        return [pa.Array._import_from_c(C.addressof(arr[i]), pa.binary()) for i in range(k)]

    def free(self):
        if self.handle:
            lib().rh_device_encoded_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def schema_struct(schema_json: str) -> "ArrowSchema":
    """The schema's batches as an Arrow C ArrowSchema ("+s" struct; the caller releases it)."""
    cs = ArrowSchema()
    if lib().rh_schema_export(Schema.get(schema_json).handle, C.byref(cs)) != RH_OK:
        raise RuntimeError("rh_schema_export failed")
    return cs


def encode_device(batch_array_addr: int, batch_schema_addr: int, schema_json: str, num_chunks: int, device: int = -1,
                  stream: int = 0, want_stats: bool = True, kernel: int = KERNEL_AUTO) -> DeviceEncoded:
    """rh_encode_device: `batch_array_addr` is the address of a struct ArrowArray whose buffer pointers are DEVICE
    pointers (e.g. ctypes.addressof(device_result_export.array)); `batch_schema_addr` of its ArrowSchema."""
    L = lib()
    s = Schema.get(schema_json)
    out = C.c_void_p()
    st = RhStats()
    err = C.c_char_p()
    opts, _keep = make_opts(device, kernel, stream, None, 0)
    rc = L.rh_encode_device(s.handle, batch_array_addr, batch_schema_addr, num_chunks, C.byref(opts), C.byref(out),
                            C.byref(st) if want_stats else None, C.byref(err))
    if rc != RH_OK:
        _raise(rc, err)
    return DeviceEncoded(out.value, st.as_dict())


# Framed messages, the write side (include/ruhvro_hip.h): symbols added without a change of the ABI version.
FRAME_JOIN_SYMBOLS = ("rh_encode_to_device", "rh_frame_join", "rh_frame_join_last")


class RhFrameSource(C.Structure):
    """rh_frame_source: one chunk of a device-resident encode result, the wire id its messages carry, its rows' destinations."""
    _fields_ = [("enc", C.c_void_p), ("chunk", C.c_uint32), ("pad", C.c_uint32), ("id", C.c_uint64), ("indices", C.c_void_p)]


def _frame_join_sym(name: str):
    f = getattr(lib(), name, None)
    if f is None:
        raise RuntimeError(f"libruhvro_hip.so has no {name}: the library was built before framed writes")
    if f.argtypes is None:
        f.restype, f.argtypes = {
            "rh_encode_to_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(RhOpts), C.POINTER(C.c_void_p),
                                              C.POINTER(RhStats), C.POINTER(C.c_char_p)]),
            "rh_frame_join": (C.c_int, [C.POINTER(RhFrameSource), C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(RhOpts),
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_char_p)]),
            "rh_frame_join_last": (None, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint64)]),
        }[name]
    return f


def encode_to_device(batch, schema_json: str, num_chunks: int, device: int = -1, kernel: int = KERNEL_AUTO, devices=None,
                     want_stats: bool = False) -> DeviceEncoded:
    """rh_encode_to_device: a host RecordBatch (or StructArray) encoded with the result left in HBM."""
    s = Schema.get(schema_json)
    sa = batch.to_struct_array() if isinstance(batch, pa.RecordBatch) else batch
    c_arr, c_sch = ArrowArray(), ArrowSchema()
    sa._export_to_c(C.addressof(c_arr), C.addressof(c_sch))
    out, st, err = C.c_void_p(), RhStats(), C.c_char_p()
    opts, _keep = make_opts(device, kernel, None, devices)
    try:
        rc = _frame_join_sym("rh_encode_to_device")(s.handle, C.addressof(c_arr), C.addressof(c_sch), num_chunks, C.byref(opts),
                                                    C.byref(out), C.byref(st) if want_stats else None, C.byref(err))
    finally:
        if c_arr.release:         # (the engine copies what it reads: the exported structs are the caller's to release)
            C.CFUNCTYPE(None, C.POINTER(ArrowArray))(c_arr.release)(C.byref(c_arr))
        if c_sch.release:
            C.CFUNCTYPE(None, C.POINTER(ArrowSchema))(c_sch.release)(C.byref(c_sch))
    if rc != RH_OK:
        _raise(rc, err)
    return DeviceEncoded(out.value, st.as_dict() if want_stats else {})


def frame_join(sources, framing: int, n: int, num_chunks: int, device: int = -1, devices=None, flags: int = 0) -> DeviceEncoded:
    """rh_frame_join.  `sources`: (DeviceEncoded, chunk, wire id, indices) in order; indices: None or a contiguous numpy int64 array
    with one entry per row of that chunk.  -> a DeviceEncoded of rh_clamp_chunks(n, num_chunks) BinaryArrays of framed messages."""
    arr = (RhFrameSource * max(len(sources), 1))()
    keep = []
    for i, (enc, chunk, wire, indices) in enumerate(sources):
        arr[i].enc, arr[i].chunk, arr[i].pad, arr[i].id = enc.handle, chunk, 0, wire
        if indices is not None:
            idx = np.ascontiguousarray(indices, dtype=np.int64)
            keep.append(idx)
            arr[i].indices = idx.ctypes.data if len(idx) else None
    out, err = C.c_void_p(), C.c_char_p()
    opts, _keep = make_opts(device, flags, None, devices)
    rc = _frame_join_sym("rh_frame_join")(arr, len(sources), framing, n, num_chunks, C.byref(opts), C.byref(out), C.byref(err))
    if rc != RH_OK:
        _raise(rc, err)
    return DeviceEncoded(out.value, {})


def frame_join_last() -> dict:
    """rh_frame_join_last: GPU time of the most recent join of this process, stage by stage."""
    l_ms, s_ms, g_ms, n = C.c_float(), C.c_float(), C.c_float(), C.c_uint64()
    _frame_join_sym("rh_frame_join_last")(C.byref(l_ms), C.byref(s_ms), C.byref(g_ms), C.byref(n))
    return {"lengths_ms": l_ms.value, "scan_ms": s_ms.value, "gather_ms": g_ms.value, "n": int(n.value)}


def decode_device(d_data: int, d_offsets: int, data_len: int, n: int, schema_json: str, num_chunks: int,
                  device: int = -1, stream: int = 0, want_stats: bool = True, kernel: int = KERNEL_AUTO,
                  chunk_rows: int = 0, asynchronous: bool = False, two_pass: bool = False, single_pass: bool = False,
                  *, columns=None, reader_schema=None, where=None) -> DeviceResult:
    """rh_decode_device on raw device pointers (e.g. torch tensors' data_ptr()).  chunk_rows: explicit geometry
    for a range of a larger call's chunks (rh_opts.chunk_rows).  asynchronous: RH_ASYNC -- the result is returned
    unsettled (DeviceResult.wait() settles it and fills .stats; every accessor settles implicitly).  `where`:
    rh_decode_device_where (a row filter, see check_where); the result's `.kept` is the number of records it kept."""
    L = lib()
    flt = Filter.get(schema_json, where) if where is not None else None
    s = Schema.get(schema_json, columns, reader_schema)
    out = C.c_void_p()
    st = RhStats()
    err = C.c_char_p()
    opts, _keep = make_opts(device, kernel | (RH_ASYNC if asynchronous else 0) | (RH_TWO_PASS if two_pass else 0) |
                            (RH_SINGLE_PASS if single_pass else 0), stream, None, chunk_rows)
    kept = C.c_uint64(n)
    if flt is not None:
        rc = _filter_sym("rh_decode_device_where")(s.handle, d_data, d_offsets, data_len, n, num_chunks, C.byref(opts), C.byref(out),
                                                   C.byref(st) if want_stats else None, C.byref(err), flt.handle, C.byref(kept))
    else:
        rc = L.rh_decode_device(s.handle, d_data, d_offsets, data_len, n, num_chunks, C.byref(opts), C.byref(out),
                                C.byref(st) if want_stats else None, C.byref(err))
    if rc != RH_OK:
        _raise(rc, err)
    r = DeviceResult(out.value, s, st.as_dict())
    r._want_stats = want_stats
    r.kept = int(kept.value)
    return r


def decode_device_tolerant(d_data: int, d_offsets: int, data_len: int, n: int, schema_json: str, num_chunks: int,
                           device: int = -1, stream: int = 0, want_stats: bool = True, kernel: int = KERNEL_AUTO,
                           chunk_rows: int = 0, *, columns=None, max_errors: int = 1024, flags: int = 0) -> DeviceResult:
    """rh_decode_device_tolerant: decode_device with the placeholder datum in the place of every malformed record; the
    result's `.errors` lists those records.  A repaired call's result owns the patched input it decoded."""
    L = lib()
    s = Schema.get(schema_json, columns)
    out, st, err, errs = C.c_void_p(), RhStats(), C.c_char_p(), C.c_void_p()
    opts, _keep = make_opts(device, kernel | flags, stream, None, chunk_rows)
    rc = L.rh_decode_device_tolerant(s.handle, d_data, d_offsets, data_len, n, num_chunks, C.byref(opts), C.byref(out),
                                     C.byref(st) if want_stats else None, C.byref(err), max_errors, C.byref(errs))
    if rc != RH_OK:
        _raise(rc, err)
    r = DeviceResult(out.value, s, st.as_dict())
    r._want_stats = want_stats
    r.errors = _take_errors(errs)
    return r


class PreparedDeviceDecode:
    """One rh_decode_device call with every ctypes argument built ONCE: a loop that repeats the call pays the C entry
    point only (what a C caller pays), not ~15 us of Python argument marshalling per call -- which is the size of a
    whole 1M-record call's fixed cost.  run() -> opaque result handle (free it with free()); `stats` is refilled by
    every run(want_stats=True)."""

    def __init__(self, d_data: int, d_offsets: int, data_len: int, n: int, schema_json: str, num_chunks: int,
                 device: int = -1, stream: int = 0, kernel: int = KERNEL_AUTO, chunk_rows: int = 0, asynchronous: bool = False,
                 two_pass: bool = False, single_pass: bool = False, *, columns=None, reader_schema=None):
        self._L = lib()
        self._schema = Schema.get(schema_json, columns, reader_schema)
        self._opts, self._keep = make_opts(device, kernel | (RH_ASYNC if asynchronous else 0) | (RH_TWO_PASS if two_pass else 0) |
                                           (RH_SINGLE_PASS if single_pass else 0), stream, None, chunk_rows)
        self._wait = self._L.rh_device_result_wait
        self.stats = RhStats()
        self._out = C.c_void_p()
        self._err = C.c_char_p()
        self._args = (self._schema.handle, C.c_void_p(d_data), C.c_void_p(d_offsets), C.c_uint64(data_len), C.c_uint64(n),
                      C.c_uint64(num_chunks), C.byref(self._opts), C.byref(self._out))
        self._st = C.byref(self.stats)
        self._e = C.byref(self._err)
        self._fn = self._L.rh_decode_device
        self._free = self._L.rh_device_result_free

    def run(self, want_stats: bool = False) -> int:
        rc = self._fn(*self._args, self._st if want_stats else None, self._e)
        if rc != RH_OK:
            _raise(rc, self._err)
        return self._out.value

    def wait(self, handle: int, want_stats: bool = False) -> None:
        """Settle an asynchronous run() (rh_device_result_wait): raises what the synchronous call would have raised;
        `stats` is refilled when the run asked for them."""
        rc = self._wait(handle, self._st if want_stats else None, self._e)
        if rc != RH_OK:
            _raise(rc, self._err)

    def output_bytes(self, handle: int) -> int:
        return int(self._L.rh_device_result_output_bytes(handle))

    def free(self, handle: int) -> None:
        self._free(handle)


    def to_host(self, handle: int) -> List[pa.RecordBatch]:
        """rh_device_result_to_host of a run()'s result (settles an asynchronous one first); the handle stays the caller's
        to free."""
        k = int(self._L.rh_device_result_chunks(handle))
        arr = (ArrowArray * k)()
        rc = self._L.rh_device_result_to_host(handle, arr, self._e)
        if rc != RH_OK:
            _raise(rc, self._err)
        return _import_chunks(arr, k, self._schema.arrow_schema)


# Avro object container files (include/ruhvro_hip.h): symbols added without a change of the ABI version, looked
# up by name when first asked for.
def _container_sym(name: str, restype, argtypes):
    f = getattr(lib(), name, None)          # (ctypes: dlsym)
    if f is None:
        raise RuntimeError(f"libruhvro_hip.so has no {name}: the library was built before container reads")
    f.restype, f.argtypes = restype, argtypes
    return f


def _u8(buf) -> np.ndarray:
    a = np.ascontiguousarray(buf, dtype=np.uint8)
    return a if a.size else np.zeros(1, dtype=np.uint8)      # (an addressable byte; the length is passed separately)


def container_scan(buf: np.ndarray) -> dict:
    """rh_container_scan over a uint8 array -> {"schema", "codec", "sync", "metadata", "start", "end", "first"}: the header and
    the block table (uint64 arrays; first has one entry more than there are blocks, first[-1] = the number of records).  Raises
    ValueError("container: ...") for a malformed file.  Needs no device."""
    scan = _container_sym("rh_container_scan", C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_char_p)])
    n = int(np.asarray(buf).size)
    a = _u8(buf)
    info, err = C.c_void_p(), C.c_char_p()
    rc = scan(a.ctypes.data, n, C.byref(info), C.byref(err))
    if rc != RH_OK:
        _raise(rc, err)
    h = info.value
    try:
        slen = C.c_uint64()
        p = _container_sym("rh_container_info_schema", C.c_void_p, [C.c_void_p, C.POINTER(C.c_uint64)])(h, C.byref(slen))
        schema = C.string_at(p, slen.value).decode("utf-8")
        codec = C.string_at(_container_sym("rh_container_info_codec", C.c_void_p, [C.c_void_p])(h)).decode("utf-8", "replace")
        sync = C.string_at(_container_sym("rh_container_info_sync", C.c_void_p, [C.c_void_p])(h), 16)
        nb = int(_container_sym("rh_container_info_blocks", C.c_uint64, [C.c_void_p])(h))
        ps, pe, pf = C.c_void_p(), C.c_void_p(), C.c_void_p()
        table = _container_sym("rh_container_info_table", C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 3)
        if table(h, C.byref(ps), C.byref(pe), C.byref(pf)) != RH_OK:
            raise RuntimeError("rh_container_info_table failed")

        def arr(ptr, count):
            return np.frombuffer(C.string_at(ptr, 8 * count), dtype=np.uint64).copy() if count else np.zeros(0, dtype=np.uint64)
        start, end, first = arr(ps, nb), arr(pe, nb), arr(pf, nb + 1)
        meta = {}
        get = _container_sym("rh_container_info_metadata_get", C.c_int,
                             [C.c_void_p, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)])
        for k in range(_container_sym("rh_container_info_metadata_count", C.c_uint32, [C.c_void_p])(h)):
            key, val, vlen = C.c_char_p(), C.c_void_p(), C.c_uint64()
            if get(h, k, C.byref(key), C.byref(val), C.byref(vlen)) != RH_OK:
                raise RuntimeError("rh_container_info_metadata_get failed")
            meta[key.value.decode("utf-8", "replace")] = C.string_at(val, vlen.value) if vlen.value else b""
        return {"schema": schema, "codec": codec, "sync": sync, "metadata": meta, "start": start, "end": end, "first": first}
    finally:
        _container_sym("rh_container_info_free", None, [C.c_void_p])(h)


_BLOCKS_LEAD = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(RhOpts)]


def _blocks_args(data, start, end, first):
    n = int(np.asarray(data).size)
    data = _u8(data)
    start = np.ascontiguousarray(start, dtype=np.uint64)
    end = np.ascontiguousarray(end, dtype=np.uint64)
    first = np.ascontiguousarray(first, dtype=np.uint64)
    if len(start) != len(end) or len(first) != len(start) + 1:
        raise ValueError("container: the block table needs as many starts as ends and one more first-record index")
    one = np.zeros(1, dtype=np.uint64)
    return (data, start if len(start) else one, end if len(end) else one, first), n, len(start)


def decode_blocks(data, start, end, first, schema_json: str, num_chunks: int, device: int = -1, want_stats: bool = False,
                  kernel: int = KERNEL_AUTO, *, columns=None, reader_schema=None):
    """rh_decode_blocks: host bytes that hold uncompressed Avro container blocks at start[b] .. end[b], with first[b] the index
    of each block's first record -> list[RecordBatch], the batches of decode_packed over the same records."""
    s = Schema.get(schema_json, columns, reader_schema)
    fn = _container_sym("rh_decode_blocks", C.c_int, _BLOCKS_LEAD + [C.POINTER(ArrowArray), C.POINTER(C.c_uint32), C.POINTER(RhStats),
                                                                     C.POINTER(C.c_char_p)])
    keep, nbytes, nb = _blocks_args(data, start, end, first)
    n = int(keep[3][-1])
    k = lib().rh_clamp_chunks(n, num_chunks)
    arr = (ArrowArray * k)()
    out_k, st, err = C.c_uint32(), RhStats(), C.c_char_p()
    opts, _keep = make_opts(device, kernel)
    rc = fn(s.handle, keep[0].ctypes.data, nbytes, keep[1].ctypes.data, keep[2].ctypes.data, keep[3].ctypes.data, nb, num_chunks,
            C.byref(opts), arr, C.byref(out_k), C.byref(st), C.byref(err))
    if rc != RH_OK:
        _raise(rc, err)
    out = _import_chunks(arr, out_k.value, s.arrow_schema)
    return (out, st.as_dict()) if want_stats else out


def decode_blocks_device(data, start, end, first, schema_json: str, num_chunks: int, device: int = -1, stream: int = 0,
                         kernel: int = KERNEL_AUTO, *, columns=None, reader_schema=None) -> DeviceResult:
    """rh_decode_blocks_device: decode_blocks with the Arrow buffers left in HBM (the result owns the uploaded bytes too)."""
    s = Schema.get(schema_json, columns, reader_schema)
    fn = _container_sym("rh_decode_blocks_device", C.c_int, _BLOCKS_LEAD + [C.POINTER(C.c_void_p), C.POINTER(RhStats), C.POINTER(C.c_char_p)])
    keep, nbytes, nb = _blocks_args(data, start, end, first)
    out, st, err = C.c_void_p(), RhStats(), C.c_char_p()
    opts, _keep = make_opts(device, kernel, stream)
    rc = fn(s.handle, keep[0].ctypes.data, nbytes, keep[1].ctypes.data, keep[2].ctypes.data, keep[3].ctypes.data, nb, num_chunks,
            C.byref(opts), C.byref(out), C.byref(st), C.byref(err))
    if rc != RH_OK:
        _raise(rc, err)
    r = DeviceResult(out.value, s, st.as_dict())
    r._want_stats = True
    return r


def split_last_ms() -> float:
    """rh_split_last_ms: GPU time of the split kernel of this process's most recent container read."""
    return float(_container_sym("rh_split_last_ms", C.c_float, [])())


# Deflate blocks inflated on the device: added like the entry points above, looked up by symbol.
CODEC_NULL, CODEC_DEFLATE = 0, 1
INFLATE_OK, INFLATE_MALFORMED, INFLATE_TRUNCATED, INFLATE_TRAILING, INFLATE_TOO_LARGE = 0, 1, 2, 3, 4
_CBLOCKS_LEAD = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64,
                 C.POINTER(RhOpts)]


class InflateStatus(C.Structure):
    _fields_ = [("code", C.c_uint32), ("reason", C.c_uint32), ("detail", C.c_uint64)]


def decode_cblocks(data, start, end, first, schema_json: str, num_chunks: int, codec: int = CODEC_DEFLATE, max_block_bytes: int = 0,
                   device: int = -1, want_stats: bool = False, kernel: int = KERNEL_AUTO, *, columns=None, reader_schema=None):
    """rh_decode_cblocks: decode_blocks over the blocks of a container as they are in the file -- for CODEC_DEFLATE start[b] ..
    end[b] are the COMPRESSED payloads, inflated on the device."""
    s = Schema.get(schema_json, columns, reader_schema)
    fn = _container_sym("rh_decode_cblocks", C.c_int, _CBLOCKS_LEAD + [C.POINTER(ArrowArray), C.POINTER(C.c_uint32), C.POINTER(RhStats),
                                                                       C.POINTER(C.c_char_p)])
    keep, nbytes, nb = _blocks_args(data, start, end, first)
    n = int(keep[3][-1])
    k = lib().rh_clamp_chunks(n, num_chunks)
    arr = (ArrowArray * k)()
    out_k, st, err = C.c_uint32(), RhStats(), C.c_char_p()
    opts, _keep = make_opts(device, kernel)
    rc = fn(s.handle, keep[0].ctypes.data, nbytes, keep[1].ctypes.data, keep[2].ctypes.data, keep[3].ctypes.data, nb, codec,
            max_block_bytes, num_chunks, C.byref(opts), arr, C.byref(out_k), C.byref(st), C.byref(err))
    if rc != RH_OK:
        _raise(rc, err)
    out = _import_chunks(arr, out_k.value, s.arrow_schema)
    return (out, st.as_dict()) if want_stats else out


def decode_cblocks_device(data, start, end, first, schema_json: str, num_chunks: int, codec: int = CODEC_DEFLATE,
                          max_block_bytes: int = 0, device: int = -1, stream: int = 0, kernel: int = KERNEL_AUTO, *, columns=None,
                          reader_schema=None) -> DeviceResult:
    """rh_decode_cblocks_device: decode_cblocks with the Arrow buffers left in HBM (the result owns the inflated bytes too)."""
    s = Schema.get(schema_json, columns, reader_schema)
    fn = _container_sym("rh_decode_cblocks_device", C.c_int, _CBLOCKS_LEAD + [C.POINTER(C.c_void_p), C.POINTER(RhStats), C.POINTER(C.c_char_p)])
    keep, nbytes, nb = _blocks_args(data, start, end, first)
    out, st, err = C.c_void_p(), RhStats(), C.c_char_p()
    opts, _keep = make_opts(device, kernel, stream)
    rc = fn(s.handle, keep[0].ctypes.data, nbytes, keep[1].ctypes.data, keep[2].ctypes.data, keep[3].ctypes.data, nb, codec,
            max_block_bytes, num_chunks, C.byref(opts), C.byref(out), C.byref(st), C.byref(err))
    if rc != RH_OK:
        _raise(rc, err)
    r = DeviceResult(out.value, s, st.as_dict())
    r._want_stats = True
    return r


# Row filters in the container read: the blocks calls with a predicate, looked up by symbol like the rest.
CONTAINER_WHERE_SYMBOLS = ("rh_decode_blocks_where", "rh_decode_blocks_device_where", "rh_decode_cblocks_where", "rh_decode_cblocks_device_where",
                           "rh_filter_blocks", "rh_filter_cblocks", "rh_container_where_last")
_WHERE_TAIL = [C.c_void_p, C.POINTER(C.c_uint64)]


def decode_blocks_where(data, start, end, first, schema_json: str, where, num_chunks: int, codec=None, max_block_bytes: int = 0,
                        device: int = -1, want_stats: bool = False, kernel: int = KERNEL_AUTO, *, columns=None, reader_schema=None,
                        to_device: bool = False, stream: int = 0):
    """rh_decode_blocks_where / rh_decode_cblocks_where (codec given: start[b] .. end[b] are the payloads as they are in the file)
    -> list[RecordBatch] of the records `where` keeps; to_device: the `_device` twins -> DeviceResult, its `.kept` the number of
    records kept.  The predicate compiles first: ValueError "where: ..." before any device work."""
    flt = Filter.get(schema_json, where)
    s = Schema.get(schema_json, columns, reader_schema)
    lead = _BLOCKS_LEAD if codec is None else _CBLOCKS_LEAD
    name = ("rh_decode_blocks" if codec is None else "rh_decode_cblocks") + ("_device_where" if to_device else "_where")
    if to_device:
        fn = _container_sym(name, C.c_int, lead + [C.POINTER(C.c_void_p), C.POINTER(RhStats), C.POINTER(C.c_char_p)] + _WHERE_TAIL)
    else:
        fn = _container_sym(name, C.c_int, lead + [C.POINTER(ArrowArray), C.POINTER(C.c_uint32), C.POINTER(RhStats), C.POINTER(C.c_char_p)] +
                            _WHERE_TAIL)
    keep, nbytes, nb = _blocks_args(data, start, end, first)
    head = [s.handle, keep[0].ctypes.data, nbytes, keep[1].ctypes.data, keep[2].ctypes.data, keep[3].ctypes.data, nb]
    head += [num_chunks] if codec is None else [codec, max_block_bytes, num_chunks]
    st, err, kept = RhStats(), C.c_char_p(), C.c_uint64()
    opts, _keep = make_opts(device, kernel, stream if to_device else None)
    if to_device:
        out = C.c_void_p()
        rc = fn(*head, C.byref(opts), C.byref(out), C.byref(st), C.byref(err), flt.handle, C.byref(kept))
        if rc != RH_OK:
            _raise(rc, err)
        r = DeviceResult(out.value, s, st.as_dict())
        r._want_stats = True
        r.kept = int(kept.value)
        return r
    k = lib().rh_clamp_chunks(int(keep[3][-1]), num_chunks)
    arr = (ArrowArray * k)()
    out_k = C.c_uint32()
    rc = fn(*head, C.byref(opts), arr, C.byref(out_k), C.byref(st), C.byref(err), flt.handle, C.byref(kept))
    if rc != RH_OK:
        _raise(rc, err)
    out = _import_chunks(arr, out_k.value, s.arrow_schema)
    return (out, st.as_dict()) if want_stats else out


def filter_blocks(data, start, end, first, schema_json: str, where, codec=None, max_block_bytes: int = 0, device: int = -1) -> np.ndarray:
    """rh_filter_blocks / rh_filter_cblocks: the split and the predicate alone -> numpy bool[n], True where the file's record is
    kept.  A malformed record or block raises what the blocks call raises for it."""
    flt = Filter.get(schema_json, where)
    keep, nbytes, nb = _blocks_args(data, start, end, first)
    n = int(keep[3][-1])
    words = np.zeros(max((n + 63) // 64, 1), dtype=np.uint64)
    kept, err = C.c_uint64(), C.c_char_p()
    opts, _keep = make_opts(device, 0)
    head = [flt.handle, keep[0].ctypes.data, nbytes, keep[1].ctypes.data, keep[2].ctypes.data, keep[3].ctypes.data, nb]
    tail = [C.POINTER(RhOpts), C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_char_p)]
    if codec is None:
        fn = _container_sym("rh_filter_blocks", C.c_int, _BLOCKS_LEAD[:7] + tail)
    else:
        fn = _container_sym("rh_filter_cblocks", C.c_int, _BLOCKS_LEAD[:7] + [C.c_int, C.c_uint64] + tail)
        head += [codec, max_block_bytes]
    rc = fn(*head, C.byref(opts), words.ctypes.data, C.byref(kept), C.byref(err))
    if rc != RH_OK:
        _raise(rc, err)
    mask = _keep_mask(words, n)
    assert int(mask.sum()) == kept.value
    return mask


def container_where_last() -> dict:
    """rh_container_where_last: the most recent filtered container read of this process."""
    s_ms, g_ms, n, kept = C.c_float(), C.c_float(), C.c_uint64(), C.c_uint64()
    _container_sym("rh_container_where_last", None, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)])(
        C.byref(s_ms), C.byref(g_ms), C.byref(n), C.byref(kept))
    return {"split_ms": s_ms.value, "gather_ms": g_ms.value, "n": int(n.value), "kept": int(kept.value)}


def inflate_blocks(data, start, end, max_block_bytes: int = 0, device: int = -1):
    """rh_inflate_blocks: the raw-deflate streams at data[start[b] .. end[b]) inflated on the device -> (out, out_start, out_end,
    status): the accepted blocks back to back (bytes), where each lies (uint64 arrays; a failing block is empty), and one
    (code, reason, detail) per block (a structured array; code is one of INFLATE_*)."""
    fn = _container_sym("rh_inflate_blocks", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(RhOpts),
                                                       C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.POINTER(C.c_char_p)])
    n = int(np.asarray(data).size)
    data = _u8(data)
    start = np.ascontiguousarray(start, dtype=np.uint64)
    end = np.ascontiguousarray(end, dtype=np.uint64)
    if len(start) != len(end):
        raise ValueError("container: the block table needs as many starts as ends")
    nb = len(start)
    out_start, out_end = np.zeros(max(nb, 1), dtype=np.uint64), np.zeros(max(nb, 1), dtype=np.uint64)
    status = np.zeros(max(nb, 1), dtype=np.dtype([("code", np.uint32), ("reason", np.uint32), ("detail", np.uint64)]))
    one = np.zeros(1, dtype=np.uint64)
    out, out_len, err = C.c_void_p(), C.c_uint64(), C.c_char_p()
    opts, _keep = make_opts(device, KERNEL_AUTO)
    rc = fn(data.ctypes.data, n, (start if nb else one).ctypes.data, (end if nb else one).ctypes.data, nb, max_block_bytes, C.byref(opts),
            C.byref(out), C.byref(out_len), out_start.ctypes.data, out_end.ctypes.data, status.ctypes.data, C.byref(err))
    if rc != RH_OK:
        _raise(rc, err)
    try:
        blob = C.string_at(out.value, out_len.value) if out_len.value else b""
    finally:
        lib().rh_free_string(C.cast(out, C.c_void_p))
    return blob, out_start[:nb], out_end[:nb], status[:nb]


def inflate_last() -> dict:
    """rh_inflate_last: the most recent device inflate of this process -- GPU time of its two kernels, bytes in and out."""
    fn = _container_sym("rh_inflate_last", None, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)])
    a, b, c, d = C.c_float(), C.c_float(), C.c_uint64(), C.c_uint64()
    fn(C.byref(a), C.byref(b), C.byref(c), C.byref(d))
    return {"size_ms": a.value, "emit_ms": b.value, "in_bytes": c.value, "out_bytes": d.value}


# Deflate blocks written on the device: added like the entry points above, looked up by symbol.
DEFLATE_AUTO, DEFLATE_STORED, DEFLATE_FIXED, DEFLATE_DYNAMIC = 0, 1, 2, 3
DEFLATE_SEGMENT = 32768      # deflate_core.h kSegment: a payload is compressed in independent pieces of this many bytes
_DEFLATE_LEAD = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
_DEFLATE_TAIL = [C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p)]


def _deflate_call(fn, data, start, end, strategy, opts):
    if isinstance(data, (bytes, bytearray, memoryview)):
        data = np.frombuffer(data, dtype=np.uint8)
    n = int(np.asarray(data).size)
    data = _u8(data)
    start = np.ascontiguousarray(start, dtype=np.uint64)
    end = np.ascontiguousarray(end, dtype=np.uint64)
    if len(start) != len(end):
        raise ValueError("container: the block table needs as many starts as ends")
    nb = len(start)
    out_start, out_end = np.zeros(max(nb, 1), dtype=np.uint64), np.zeros(max(nb, 1), dtype=np.uint64)
    one = np.zeros(1, dtype=np.uint64)
    out, out_len, err = C.c_void_p(), C.c_uint64(), C.c_char_p()
    lead = (data.ctypes.data, n, (start if nb else one).ctypes.data, (end if nb else one).ctypes.data, nb, strategy)
    tail = (C.byref(out), C.byref(out_len), out_start.ctypes.data, out_end.ctypes.data, C.byref(err))
    rc = fn(*lead, *opts, *tail)
    if rc != RH_OK:
        _raise(rc, err)
    try:
        blob = C.string_at(out.value, out_len.value) if out_len.value else b""
    finally:
        lib().rh_free_string(C.cast(out, C.c_void_p))
    return blob, out_start[:nb], out_end[:nb]


def deflate_blocks(data, start, end, strategy: int = DEFLATE_AUTO, device: int = -1):
    """rh_deflate_blocks: the payloads at data[start[b] .. end[b]) each compressed on the device into one raw RFC 1951 stream ->
    (blob, out_start, out_end): the streams back to back (bytes) and where each lies (uint64 arrays).  strategy: DEFLATE_*."""
    fn = _container_sym("rh_deflate_blocks", C.c_int, _DEFLATE_LEAD + [C.POINTER(RhOpts)] + _DEFLATE_TAIL)
    opts, _keep = make_opts(device, KERNEL_AUTO)
    return _deflate_call(fn, data, start, end, strategy, (C.byref(opts),))


def deflate_blocks_host(data, start, end, strategy: int = DEFLATE_AUTO):
    """rh_deflate_blocks_host: deflate_blocks by the same stream logic on the calling thread -- the same bytes, no device."""
    fn = _container_sym("rh_deflate_blocks_host", C.c_int, _DEFLATE_LEAD + _DEFLATE_TAIL)
    return _deflate_call(fn, data, start, end, strategy, ())


def deflate_bound(n: int) -> int:
    """rh_deflate_bound: the largest size a stream for n bytes can take."""
    return int(_container_sym("rh_deflate_bound", C.c_uint64, [C.c_uint64])(n))


def deflate_last() -> dict:
    """rh_deflate_last: the most recent device deflate of this process -- GPU time of its two kernels, bytes in and out."""
    fn = _container_sym("rh_deflate_last", None, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)])
    a, b, c, d = C.c_float(), C.c_float(), C.c_uint64(), C.c_uint64()
    fn(C.byref(a), C.byref(b), C.byref(c), C.byref(d))
    return {"deflate_ms": a.value, "gather_ms": b.value, "in_bytes": c.value, "out_bytes": d.value}


# Tolerant container reads: added like the entry points above, looked up by symbol.
BLOCK_END, BLOCK_DROPPED, BLOCK_COUNT, BLOCK_TOO_LARGE, BLOCK_INFLATE = 0x100, 0x200, 0x201, 0x202, 0x300
BLOCK_STATUS = np.dtype([("code", np.uint32), ("aux", np.uint32), ("detail", np.int64), ("kept", np.uint64)])


def container_salvage(buf: np.ndarray) -> dict:
    """rh_container_salvage over a uint8 array -> container_scan's dict for the blocks that are framed, plus "header_end",
    "header_offset" / "count" (uint64 arrays, per block), "refused" (uint8, per block: 1 = record count out of range),
    "gaps" ([(offset, length, block, message)], ascending) and "steps".  Raises ValueError("container: ...") for a header that
    does not parse -- what container_scan raises.  Needs no device."""
    scan = _container_sym("rh_container_salvage", C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_char_p)])
    n = int(np.asarray(buf).size)
    a = _u8(buf)
    info, err = C.c_void_p(), C.c_char_p()
    rc = scan(a.ctypes.data, n, C.byref(info), C.byref(err))
    if rc != RH_OK:
        _raise(rc, err)
    h = info.value
    try:
        slen = C.c_uint64()
        p = _container_sym("rh_container_info_schema", C.c_void_p, [C.c_void_p, C.POINTER(C.c_uint64)])(h, C.byref(slen))
        schema = C.string_at(p, slen.value).decode("utf-8")
        codec = C.string_at(_container_sym("rh_container_info_codec", C.c_void_p, [C.c_void_p])(h)).decode("utf-8", "replace")
        sync = C.string_at(_container_sym("rh_container_info_sync", C.c_void_p, [C.c_void_p])(h), 16)
        nb = int(_container_sym("rh_container_info_blocks", C.c_uint64, [C.c_void_p])(h))
        ps, pe, pf = C.c_void_p(), C.c_void_p(), C.c_void_p()
        table = _container_sym("rh_container_info_table", C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 3)
        if table(h, C.byref(ps), C.byref(pe), C.byref(pf)) != RH_OK:
            raise RuntimeError("rh_container_info_table failed")
        hend, ph, pc, pr, ngaps, steps = C.c_uint64(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        more = _container_sym("rh_container_info_salvage", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)] + [C.POINTER(C.c_void_p)] * 3 +
                              [C.POINTER(C.c_uint64)] * 2)
        if more(h, C.byref(hend), C.byref(ph), C.byref(pc), C.byref(pr), C.byref(ngaps), C.byref(steps)) != RH_OK:
            raise RuntimeError("rh_container_info_salvage failed")

        def arr(ptr, count, dtype=np.uint64):
            size = np.dtype(dtype).itemsize * count
            return np.frombuffer(C.string_at(ptr, size), dtype=dtype).copy() if count else np.zeros(0, dtype=dtype)
        gap = _container_sym("rh_container_info_gap", C.c_int, [C.c_void_p, C.c_uint64] + [C.POINTER(C.c_uint64)] * 3 + [C.POINTER(C.c_char_p)])
        gaps = []
        for k in range(ngaps.value):
            off, ln, blk, msg = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_char_p()
            if gap(h, k, C.byref(off), C.byref(ln), C.byref(blk), C.byref(msg)) != RH_OK:
                raise RuntimeError("rh_container_info_gap failed")
            gaps.append((off.value, ln.value, blk.value, msg.value.decode("utf-8", "replace")))
        meta = {}
        get = _container_sym("rh_container_info_metadata_get", C.c_int,
                             [C.c_void_p, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)])
        for k in range(_container_sym("rh_container_info_metadata_count", C.c_uint32, [C.c_void_p])(h)):
            key, val, vlen = C.c_char_p(), C.c_void_p(), C.c_uint64()
            if get(h, k, C.byref(key), C.byref(val), C.byref(vlen)) != RH_OK:
                raise RuntimeError("rh_container_info_metadata_get failed")
            meta[key.value.decode("utf-8", "replace")] = C.string_at(val, vlen.value) if vlen.value else b""
        return {"schema": schema, "codec": codec, "sync": sync, "metadata": meta, "start": arr(ps, nb), "end": arr(pe, nb),
                "first": arr(pf, nb + 1), "header_end": hend.value, "header_offset": arr(ph, nb), "count": arr(pc, nb),
                "refused": arr(pr, nb, np.uint8), "gaps": gaps, "steps": steps.value}
    finally:
        _container_sym("rh_container_info_free", None, [C.c_void_p])(h)


def block_status_message(block: int, status, count: int) -> str:
    """rh_block_status_message: the message the strict call raises for block `block` whose status is `status` (one element of a
    BLOCK_STATUS array) and whose header claims `count` records."""
    fn = _container_sym("rh_block_status_message", C.c_int, [C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_char_p)])
    one = np.zeros(1, dtype=BLOCK_STATUS)
    one[0] = status
    msg = C.c_char_p()
    rc = fn(block, one.ctypes.data, count, C.byref(msg))
    if rc != RH_OK:
        _raise(rc, msg)
    try:
        return msg.value.decode("utf-8", "replace")
    finally:
        lib().rh_free_string(C.cast(msg, C.c_void_p))


_TBLOCKS_LEAD = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64,
                 C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(RhOpts)]


def _tolerant_args(data, start, end, first, dropped):
    keep, nbytes, nb = _blocks_args(data, start, end, first)
    drop = np.zeros(max(nb, 1), dtype=np.uint8)
    if dropped is not None:
        drop[:nb] = np.asarray(dropped, dtype=np.uint8)
    return keep, nbytes, nb, drop, np.zeros(max(nb, 1), dtype=BLOCK_STATUS)


def decode_blocks_tolerant(data, start, end, first, schema_json: str, num_chunks: int, codec: int = CODEC_NULL, max_block_bytes: int = 0,
                           dropped=None, max_errors: int = 1024, extra_errors: int = 0, device: int = -1, kernel: int = KERNEL_AUTO, *,
                           columns=None, reader_schema=None):
    """rh_decode_blocks_tolerant -> (list[RecordBatch], status): the batches of the records the blocks keep, and one
    BLOCK_STATUS per block.  (None, status) = more than max_errors reports."""
    s = Schema.get(schema_json, columns, reader_schema)
    fn = _container_sym("rh_decode_blocks_tolerant", C.c_int, _TBLOCKS_LEAD + [C.POINTER(ArrowArray), C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p,
                                                                              C.POINTER(C.c_int), C.POINTER(RhStats), C.POINTER(C.c_char_p)])
    keep, nbytes, nb, drop, status = _tolerant_args(data, start, end, first, dropped)
    cap = lib().rh_clamp_chunks(int(keep[3][-1]), num_chunks)
    arr = (ArrowArray * cap)()
    out_k, many, st, err = C.c_uint32(), C.c_int(), RhStats(), C.c_char_p()
    opts, _keep = make_opts(device, kernel)
    rc = fn(s.handle, keep[0].ctypes.data, nbytes, keep[1].ctypes.data, keep[2].ctypes.data, keep[3].ctypes.data, drop.ctypes.data, nb, codec,
            max_block_bytes, max_errors, extra_errors, num_chunks, C.byref(opts), arr, cap, C.byref(out_k), status.ctypes.data, C.byref(many),
            C.byref(st), C.byref(err))
    if rc != RH_OK:
        _raise(rc, err)
    if many.value:
        return None, status[:nb]
    return _import_chunks(arr, out_k.value, s.arrow_schema), status[:nb]


def decode_blocks_tolerant_device(data, start, end, first, schema_json: str, num_chunks: int, codec: int = CODEC_NULL,
                                  max_block_bytes: int = 0, dropped=None, max_errors: int = 1024, extra_errors: int = 0, device: int = -1,
                                  stream: int = 0, kernel: int = KERNEL_AUTO, *, columns=None, reader_schema=None):
    """rh_decode_blocks_tolerant_device -> (DeviceResult, status); (None, status) = more than max_errors reports."""
    s = Schema.get(schema_json, columns, reader_schema)
    fn = _container_sym("rh_decode_blocks_tolerant_device", C.c_int, _TBLOCKS_LEAD + [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(C.c_int),
                                                                                     C.POINTER(RhStats), C.POINTER(C.c_char_p)])
    keep, nbytes, nb, drop, status = _tolerant_args(data, start, end, first, dropped)
    out, many, st, err = C.c_void_p(), C.c_int(), RhStats(), C.c_char_p()
    opts, _keep = make_opts(device, kernel, stream)
    rc = fn(s.handle, keep[0].ctypes.data, nbytes, keep[1].ctypes.data, keep[2].ctypes.data, keep[3].ctypes.data, drop.ctypes.data, nb, codec,
            max_block_bytes, max_errors, extra_errors, num_chunks, C.byref(opts), C.byref(out), status.ctypes.data, C.byref(many), C.byref(st),
            C.byref(err))
    if rc != RH_OK:
        _raise(rc, err)
    if many.value:
        return None, status[:nb]
    r = DeviceResult(out.value, s, st.as_dict())
    r._want_stats = True
    return r, status[:nb]


def salvage_last() -> dict:
    """rh_salvage_last: the most recent tolerant container read of this process -- GPU time of its split and of its gather, the
    blocks it reported, the bytes it gathered (0 = no gather ran: the file's bytes were decoded where they were)."""
    fn = _container_sym("rh_salvage_last", None, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)])
    a, b, c, d = C.c_float(), C.c_float(), C.c_uint64(), C.c_uint64()
    fn(C.byref(a), C.byref(b), C.byref(c), C.byref(d))
    return {"split_ms": a.value, "gather_ms": b.value, "blocks_reported": c.value, "bytes_gathered": d.value}
