"""Drop-in module name: ``import pyruhvro`` resolves to the MI355X-native engine.

Same five functions as the reference's PyO3 module (src/lib.rs:150-158); the three decode functions also take the
keyword-only extensions ``columns=[...]`` (decode only those top-level fields) and ``reader_schema=`` (decode
writer-encoded records into an evolved schema) and ``where=`` (decode only the records that match a predicate;
``filter_records`` is that filter alone).  Beside them the tolerant decode: the
``*_tolerant`` functions replace malformed records by ``placeholder_datum(schema)`` and report all of them; and the Avro
object container files: ``container_info`` / ``read_container`` / ``read_container_to_device`` / ``write_container``, and
``read_container_tolerant`` / ``read_container_to_device_tolerant``, which salvage what a damaged file still holds, and ``read_container_where`` / ``read_container_where_to_device`` /
``filter_container``, which evaluate a ``where`` predicate in the walk that finds the file's records; and framed
messages as a Kafka consumer holds them (Confluent wire format, Avro single-object encoding): ``deserialize_framed`` splits them
by writer schema id on the GPU and decodes every group, ``frame_split`` is that split alone, ``schema_fingerprint`` the id a
single-object header carries, and ``serialize_framed`` the way back: record batches of several writer schemas encoded, put into
message order and given their headers on the GPU."""
from pyruhvro_amd import (  # noqa: F401
    deserialize_framed,
    serialize_framed,
    frame_split,
    schema_fingerprint,
    FramedGroup,
    FramedResult,
    container_info,
    read_container,
    read_container_to_device,
    read_container_tolerant,
    read_container_to_device_tolerant,
    BlockError,
    read_container_where,
    read_container_where_to_device,
    filter_container,
    write_container,
    deserialize_array_tolerant,
    deserialize_array_threaded_tolerant,
    deserialize_binary_array_tolerant,
    deserialize_to_device,
    placeholder_datum,
    validate_records,
    filter_records,
    deserialize_array,
    deserialize_array_threaded,
    deserialize_array_threaded_spawn,
    serialize_record_batch,
    serialize_record_batch_spawn,
)
from pyruhvro_amd.cabi import RecordError  # noqa: F401,E402

__all__ = [
    "deserialize_array", "deserialize_array_threaded", "deserialize_array_threaded_spawn", "serialize_record_batch",
    "serialize_record_batch_spawn", "deserialize_to_device", "placeholder_datum", "validate_records", "filter_records", "RecordError",
    "deserialize_array_tolerant", "deserialize_array_threaded_tolerant", "deserialize_binary_array_tolerant",
    "container_info", "read_container", "read_container_to_device", "write_container", "read_container_tolerant",
    "read_container_to_device_tolerant", "BlockError", "read_container_where", "read_container_where_to_device", "filter_container",
    "deserialize_framed", "frame_split", "schema_fingerprint", "FramedGroup", "FramedResult", "serialize_framed",
]
