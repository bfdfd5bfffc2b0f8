"""Framed messages: Avro as a Kafka consumer holds it -- every datum behind a header that names its writer schema.

    framing="confluent"       00 | schema id, 4 bytes big-endian | datum                        (every schema-registry serializer)
    framing="single_object"   C3 01 | CRC-64-AVRO fingerprint, 8 bytes little-endian | datum    (Avro specification)

``deserialize_framed`` checks the framing, partitions the messages by writer schema and strips the headers on the GPU, then decodes
every group with its own writer schema through the unchanged strict decode.  ``frame_split`` is that split alone, as
``filter_records`` is the filter alone.  ``schema_fingerprint`` is the fingerprint a single-object header carries (host Python).
``serialize_framed`` is the way back: record batches of several writer schemas encoded, put into message order and
given their headers on the GPU."""
from __future__ import annotations

import json
from collections import namedtuple
from collections.abc import Mapping

import numpy as np

HEADER_BYTES = {"confluent": 5, "single_object": 10}
_ID_BITS = {"confluent": 32, "single_object": 64}
MAX_SCHEMAS = 32

# One writer schema of a framed call: its wire id (unsigned), the schema text it was given, the ascending positions in `messages`
# of the messages that carry the id (numpy int64), and their decode (list[pyarrow.RecordBatch]).
FramedGroup = namedtuple("FramedGroup", ["id", "schema", "indices", "batches"])
# groups: one per key of `schemas`, ascending by id, empty groups included.  unknown_indices / unknown_ids: the messages whose id is
# not in `schemas` (numpy int64 / uint64; empty unless unknown="skip").
FramedResult = namedtuple("FramedResult", ["groups", "unknown_indices", "unknown_ids"])


# ---- CRC-64-AVRO of the Parsing Canonical Form -------------------------------------------------------------------------------------
_PRIMITIVES = ("null", "boolean", "int", "long", "float", "double", "bytes", "string")
_EMPTY64 = 0xC15D213AA4D7A795
_crc_table = None


def _table():
    global _crc_table
    if _crc_table is None:
        t = []
        for i in range(256):
            fp = i
            for _ in range(8):
                fp = (fp >> 1) ^ (_EMPTY64 if fp & 1 else 0)
            t.append(fp)
        _crc_table = t
    return _crc_table


def crc64_avro(data: bytes) -> int:
    """The specification's table algorithm; the empty input gives 0xc15d213aa4d7a795."""
    t = _table()
    fp = _EMPTY64
    for b in data:
        fp = (fp >> 8) ^ t[(fp ^ b) & 0xFF]
    return fp


def _fullname(name, namespace):
    if not isinstance(name, str) or not name:
        raise ValueError("schema fingerprint: a named type has no name")
    if "." in name or not namespace:
        return name
    return namespace + "." + name


def _canonical(node, namespace, out):
    q = lambda s: json.dumps(s, ensure_ascii=False)      # noqa: E731
    if isinstance(node, str):
        out.append(q(node if node in _PRIMITIVES else _fullname(node, namespace)))
    elif isinstance(node, list):
        out.append("[")
        for i, branch in enumerate(node):
            if i:
                out.append(",")
            _canonical(branch, namespace, out)
        out.append("]")
    elif isinstance(node, dict):
        t = node.get("type")
        if isinstance(t, (dict, list)):         # {"type": {...}}: the inner schema stands for the whole
            _canonical(t, namespace, out)
        elif t in _PRIMITIVES:                  # attributes (logical types among them) are stripped: the simple form
            out.append(q(t))
        elif t == "array":
            out.append('{"type":"array","items":')
            _canonical(node.get("items"), namespace, out)
            out.append("}")
        elif t == "map":
            out.append('{"type":"map","values":')
            _canonical(node.get("values"), namespace, out)
            out.append("}")
        elif t in ("record", "error", "enum", "fixed"):
            name = node.get("name")
            full = _fullname(name, node.get("namespace", namespace))
            inner = full.rsplit(".", 1)[0] if "." in full else ""
            out.append('{"name":' + q(full) + ',"type":' + q(t))
            if t == "enum":
                out.append(',"symbols":[' + ",".join(q(s) for s in node.get("symbols", [])) + "]")
            elif t == "fixed":
                out.append(',"size":' + str(int(node.get("size"))))
            else:
                out.append(',"fields":[')
                for i, f in enumerate(node.get("fields", [])):
                    if i:
                        out.append(",")
                    out.append('{"name":' + q(f.get("name")) + ',"type":')
                    _canonical(f.get("type"), inner, out)
                    out.append("}")
                out.append("]")
            out.append("}")
        elif isinstance(t, str):                # {"type": "some.Name"}: a reference
            out.append(q(_fullname(t, namespace)))
        else:
            raise ValueError("schema fingerprint: a schema object has no type")
    else:
        raise ValueError(f"schema fingerprint: {node!r} is no schema")


def parsing_canonical_form(schema_json: str) -> str:
    """The Parsing Canonical Form of the Avro specification: primitives in their simple form, fullnames, only the attributes
    ``name, type, fields, symbols, items, values, size`` in that order, no whitespace."""
    if not isinstance(schema_json, str):
        raise TypeError("argument 'schema_json': expected str")
    try:
        node = json.loads(schema_json)
    except ValueError as e:
        raise ValueError(f"schema fingerprint: Failed to parse schema from JSON: {e}") from None
    out: list = []
    _canonical(node, "", out)
    return "".join(out)


def schema_fingerprint(schema_json: str) -> int:
    """CRC-64-AVRO of the schema's Parsing Canonical Form, as an unsigned int: the id an Avro single-object header carries."""
    return crc64_avro(parsing_canonical_form(schema_json).encode("utf-8"))


# ---- the arguments ---------------------------------------------------------------------------------------------------------------------
def _check_framing(framing):
    if framing not in HEADER_BYTES:
        raise ValueError(f"framed: unknown framing {framing!r} (one of 'confluent', 'single_object')")
    return framing


def _wire_id(key, framing):
    """A key of `schemas` -> the unsigned id the wire carries."""
    if not isinstance(key, (int, np.integer)) or isinstance(key, (bool, np.bool_)):
        raise ValueError(f"framed: schema id {key!r} is not an int")
    key = int(key)
    bits = _ID_BITS[framing]
    lo = -(1 << 63) if framing == "single_object" else 0
    if not lo <= key < (1 << bits):
        raise ValueError(f"framed: schema id {key} is out of range for the {framing} framing ({lo} .. 2**{bits}-1)")
    return key % (1 << bits)


def _wire_ids(keys, framing):
    keys = list(keys)
    if not 1 <= len(keys) <= MAX_SCHEMAS:
        raise ValueError("framed: 1 to 32 schemas per call")
    ids = [_wire_id(k, framing) for k in keys]
    if len(set(ids)) != len(ids):
        raise ValueError("framed: two keys of schemas are the same schema id on the wire")
    return ids


def _split(messages, ids, framing, flags):
    import pyruhvro_amd as P
    from . import cabi
    data, offs = P._pack_records(messages)
    return cabi.FrameSplit.packed(data, offs, sorted(ids), cabi.FRAMINGS[framing], flags, kernel=P._kernel_mode, devices=P._current_devices())


def frame_split(messages, ids, framing="confluent"):
    """Extension.  The split of ``deserialize_framed`` alone: a numpy ``int16[len(messages)]`` with the position of every message's
    id in ``sorted(ids)``, -1 for an id that is not among them.  A message shorter than the header or without the marker raises
    the ``framed: `` error of the lowest such message."""
    from . import cabi
    if not isinstance(messages, list):
        raise TypeError("argument 'messages': expected a list of bytes")
    _check_framing(framing)
    ids = list(ids)
    wire = _wire_ids(ids, framing)
    sp = _split(messages, wire, framing, cabi.FRAME_CLASSIFY_ONLY)
    try:
        cls = sp.classes()
    finally:
        sp.free()
    # the device's classes are positions in the ascending WIRE ids; a negative single-object key sorts elsewhere in sorted(ids)
    at = {w: p for p, (_k, w) in enumerate(sorted(zip(ids, wire)))}
    remap = np.array([at[w] for w in sorted(wire)] + [-1], dtype=np.int16)
    return remap[cls]


def deserialize_framed(messages, schemas, num_chunks, *, framing="confluent", columns=None, reader_schema=None, unknown="raise"):
    """Extension.  Decode framed messages of several writer schemas in one call.  ``schemas``: a mapping ``{id: writer_schema_json}``
    with 1 to 32 entries; ``framing``: ``"confluent"`` (ids 0 .. 2**32-1) or ``"single_object"`` (fingerprints 0 .. 2**64-1, a
    negative key is taken modulo 2**64, so Java's signed fingerprints work).  Returns a ``FramedResult``; for every group ``g``

        g.batches == deserialize_array_threaded([messages[i][h:] for i in g.indices], g.schema, num_chunks,
                                                columns=columns, reader_schema=reader_schema)

    buffer for buffer, where ``g.indices`` is exactly the ascending positions whose header carries ``g.id``.  Framing is judged
    over the whole list first: the lowest message that is shorter than the header, lacks the marker or -- with
    ``unknown="raise"`` -- carries an id that is not in ``schemas`` raises ``ValueError("framed: message {i} ...")``; with
    ``unknown="skip"`` the latter are left out and reported in ``unknown_indices`` / ``unknown_ids``.  A malformed payload raises
    ``framed: schema id {id}: `` and what the strict call on that group's payloads raises."""
    import pyruhvro_amd as P
    from . import cabi
    if not isinstance(messages, list):
        raise TypeError("argument 'messages': expected a list of bytes")
    if not isinstance(schemas, Mapping):
        raise TypeError("argument 'schemas': expected a mapping {id: writer schema JSON}")
    _check_framing(framing)
    if unknown not in ("raise", "skip"):
        raise ValueError(f"framed: unknown={unknown!r} (one of 'raise', 'skip')")
    keys = list(schemas)
    wire = _wire_ids(keys, framing)
    P._check_chunks(num_chunks)
    order = sorted(range(len(keys)), key=lambda j: wire[j])
    texts = [schemas[keys[j]] for j in order]
    for text in texts:                                   # ValueError on a bad / unsupported schema before any device work
        P._get_schema(text, columns, reader_schema)
    sp = _split(messages, wire, framing, cabi.FRAME_SKIP_UNKNOWN if unknown == "skip" else 0)
    try:
        m = len(order)
        indices = [sp.indices(c) for c in range(m)]
        unknown_indices = sp.indices(m)
        groups = []
        for c, j in enumerate(order):
            batches = sp.decode(c, texts[c], num_chunks, kernel=P._kernel_mode, columns=columns, reader_schema=reader_schema)
            groups.append(FramedGroup(wire[j], texts[c], indices[c], batches))
    finally:
        sp.free()
    h = HEADER_BYTES[framing]
    byteorder = "big" if framing == "confluent" else "little"
    first = 1 if framing == "confluent" else 2
    unknown_ids = np.array([int.from_bytes(bytes(messages[i][first:h]), byteorder) for i in unknown_indices], dtype=np.uint64)
    return FramedResult(groups, unknown_indices, unknown_ids)


# ---- the write side -----------------------------------------------------------------------------------------------------
def _group_parts(g, pos):
    """One entry of `groups` -> (key, schema text, [RecordBatch], indices int64[] or None)."""
    import pyarrow as pa
    if isinstance(g, FramedGroup):
        key, schema, indices, batches = g
    elif isinstance(g, tuple) and len(g) == 3:
        (key, schema, batches), indices = g, None
    elif isinstance(g, tuple) and len(g) == 4:
        key, schema, batches, indices = g
    else:
        raise TypeError(f"argument 'groups': group {pos} is not a FramedGroup, (id, schema, batches) or (id, schema, batches, indices)")
    if not isinstance(schema, str):
        raise TypeError(f"argument 'groups': group {pos}: the schema is not a str")
    if isinstance(batches, pa.RecordBatch):
        batches = [batches]
    if not isinstance(batches, (list, tuple)) or not all(isinstance(b, pa.RecordBatch) for b in batches):
        raise TypeError(f"argument 'groups': group {pos}: expected a pyarrow RecordBatch or a list of them")
    if indices is not None:
        try:
            arr = np.asarray(indices)
        except Exception:
            raise TypeError(f"argument 'groups': group {pos}: the indices are not an int64 array") from None
        if arr.ndim != 1 or (arr.size and arr.dtype.kind not in "iu"):
            raise TypeError(f"argument 'groups': group {pos}: the indices are not an int64 array")
        indices = np.ascontiguousarray(arr, dtype=np.int64)
    return key, schema, list(batches), indices


def serialize_framed(groups, num_chunks, *, framing="confluent"):
    """Extension.  The mirror of ``deserialize_framed``: record batches of several writer schemas become framed messages in one
    call.  ``groups``: a list of 1 to 32 groups, each a ``FramedGroup`` or a tuple ``(id, schema_json, batches)`` or
    ``(id, schema_json, batches, indices)``; ``batches`` is one RecordBatch or a list of them, ``indices`` None or one int64 per
    row of the group.  Without indices the messages are the groups' rows in the order given; with indices (on every group) row
    ``j`` of a group becomes message ``indices[j]``, and the indices together must be a permutation of ``range(n)``.  Returns what
    ``serialize_record_batch`` returns for a batch of ``n`` rows -- ``clamp(num_chunks, 1, max(n, 1))`` BinaryArrays -- where
    message ``p`` is the header of ``framing`` with the group's id followed by the datum ``serialize_record_batch`` produces for
    that row.  The rows are encoded, put into message order and given their headers on the GPU; the finished messages are what
    comes back.  Every refusal is a ``ValueError`` that starts with ``framed: ``."""
    import pyruhvro_amd as P
    from . import cabi
    if not isinstance(groups, list):
        raise TypeError("argument 'groups': expected a list of groups")
    _check_framing(framing)
    if not 1 <= len(groups) <= MAX_SCHEMAS:
        raise ValueError("framed: 1 to 32 groups per call")
    parts = [_group_parts(g, pos) for pos, g in enumerate(groups)]
    wire = _wire_ids([p[0] for p in parts], framing)
    P._check_chunks(num_chunks)
    if P._current_devices():
        raise ValueError("framed: a framed call runs on one device (set_devices / PYRUHVRO_DEVICES is refused)")
    for w, (_key, schema, _batches, _indices) in zip(wire, parts):
        try:
            P._get_schema(schema)
        except ValueError as e:
            raise ValueError(f"framed: schema id {w}: {e}") from None
    given = sum(p[3] is not None for p in parts)
    if given not in (0, len(parts)):
        raise ValueError("framed: indices are given for some groups and not for others")
    n = 0
    for w, (_key, _schema, batches, indices) in zip(wire, parts):
        rows = sum(b.num_rows for b in batches)
        if indices is not None and len(indices) != rows:
            raise ValueError(f"framed: schema id {w} has {rows} rows and {len(indices)} indices")
        n += rows
    # with indices the order of the groups does not show in the result: ascending by wire id, the order the index checks report in
    order = sorted(range(len(parts)), key=lambda j: wire[j]) if given else range(len(parts))
    encoded, sources = [], []
    try:
        for j in order:
            _key, schema, batches, indices = parts[j]
            at = 0
            for b in batches:
                try:
                    enc = cabi.encode_to_device(b, schema, 1, kernel=P._kernel_mode)
                except ValueError as e:
                    raise ValueError(f"framed: schema id {wire[j]}: {e}") from None
                encoded.append(enc)
                sources.append((enc, 0, wire[j], None if indices is None else indices[at:at + b.num_rows]))
                at += b.num_rows
        joined = cabi.frame_join(sources, cabi.FRAMINGS[framing], n, num_chunks)
        try:
            return joined.to_host()
        finally:
            joined.free()
    finally:
        for enc in encoded:
            enc.free()
