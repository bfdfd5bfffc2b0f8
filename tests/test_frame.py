"""Framed messages, the part that needs no device: the entry points exist beside an unchanged ABI, every refusal that is raised
before any device work carries its exact message, ``schema_fingerprint`` is CRC-64-AVRO of the Parsing Canonical Form, and the
CPU check of csrc/frame_core.h builds and passes."""
import json
import subprocess

import pytest

import frame_cases as FR
from avrogen.schemas import SCHEMAS

import pyruhvro_amd as P
from pyruhvro_amd import cabi

FULL = SCHEMAS["full"]
MSG = [FR.frame("confluent", 1, b"\x00")]


def test_symbols_exist_and_the_abi_is_still_7():
    L = cabi.lib()
    assert L.rh_abi_version() == 7
    for name in cabi.FRAME_SYMBOLS:
        assert getattr(L, name, None) is not None, name
    import pyruhvro
    for name in ("frame_split", "deserialize_framed", "schema_fingerprint"):
        assert name in P.__all__ and name in pyruhvro.__all__
        assert getattr(pyruhvro, name) is getattr(P, name)
    for name in pyruhvro.__all__:      # (the drop-in module exports what it imported before it had an __all__, and nothing else)
        assert getattr(pyruhvro, name) is getattr(P, name), name
    public = {n for n in vars(pyruhvro) if not n.startswith("_") and not isinstance(getattr(pyruhvro, n), type(json))}
    assert public == set(pyruhvro.__all__), public ^ set(pyruhvro.__all__)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def _raises(exc, message, f):
    with pytest.raises(exc) as e:
        f()
    if message is not None:
        assert str(e.value) == message, str(e.value)
    return str(e.value)


def test_an_empty_mapping_or_more_than_32_schemas():
    for schemas in ({}, {i: FULL for i in range(33)}):
        _raises(ValueError, "framed: 1 to 32 schemas per call", lambda: P.deserialize_framed(MSG, schemas, 1))
    for ids in ([], list(range(33))):
        _raises(ValueError, "framed: 1 to 32 schemas per call", lambda: P.frame_split(MSG, ids))
    assert len({i: FULL for i in range(32)}) == 32      # (32 is accepted: the GPU tests run it)


@pytest.mark.parametrize("key", ["1", 1.0, True, None, (1,), b"\x01"], ids=["str", "float", "bool", "None", "tuple", "bytes"])
def test_a_key_that_is_not_an_int(key):
    msg = _raises(ValueError, None, lambda: P.deserialize_framed(MSG, {key: FULL}, 1))
    assert msg == f"framed: schema id {key!r} is not an int"
    for framing in FR.FRAMINGS:
        assert _raises(ValueError, None, lambda: P.frame_split(MSG, [key], framing=framing)) == msg


@pytest.mark.parametrize("framing,key", [("confluent", -1), ("confluent", 1 << 32), ("confluent", 1 << 63), ("single_object", 1 << 64),
                                         ("single_object", -(1 << 63) - 1)])
def test_a_key_out_of_range_for_the_framing(framing, key):
    lo, bits = (0, 32) if framing == "confluent" else (-(1 << 63), 64)
    message = f"framed: schema id {key} is out of range for the {framing} framing ({lo} .. 2**{bits}-1)"
    _raises(ValueError, message, lambda: P.deserialize_framed(MSG, {key: FULL}, 1, framing=framing))
    _raises(ValueError, message, lambda: P.frame_split(MSG, [key], framing=framing))


def test_keys_at_the_edges_of_the_range_are_accepted_up_to_the_device():
    from pyruhvro_amd import framing as F
    assert F._wire_ids([0, (1 << 32) - 1], "confluent") == [0, (1 << 32) - 1]
    assert F._wire_ids([0, (1 << 64) - 1, -(1 << 63)], "single_object") == [0, (1 << 64) - 1, 1 << 63]


def test_a_negative_single_object_key_equals_its_unsigned_twin():
    from pyruhvro_amd import framing as F
    fp = P.schema_fingerprint(FULL)
    signed = fp - (1 << 64) if fp >= 1 << 63 else fp
    assert F._wire_id(signed, "single_object") == fp == F._wire_id(fp, "single_object")
    assert F._wire_id(-1, "single_object") == (1 << 64) - 1 and F._wire_id(-(1 << 63), "single_object") == 1 << 63
    # ... and the two in one mapping are one id twice
    _raises(ValueError, "framed: two keys of schemas are the same schema id on the wire",
            lambda: P.deserialize_framed(MSG, {-1: FULL, (1 << 64) - 1: FULL}, 1, framing="single_object"))


def test_unknown_framing_and_unknown_values():
    _raises(ValueError, "framed: unknown framing 'kafka' (one of 'confluent', 'single_object')", lambda: P.deserialize_framed(MSG, {1: FULL}, 1, framing="kafka"))
    _raises(ValueError, "framed: unknown framing None (one of 'confluent', 'single_object')", lambda: P.frame_split(MSG, [1], framing=None))
    _raises(ValueError, "framed: unknown='drop' (one of 'raise', 'skip')", lambda: P.deserialize_framed(MSG, {1: FULL}, 1, unknown="drop"))


def test_type_errors():
    for schemas in ([(1, FULL)], FULL, None, {1}):
        _raises(TypeError, "argument 'schemas': expected a mapping {id: writer schema JSON}", lambda: P.deserialize_framed(MSG, schemas, 1))
    for messages in (tuple(MSG), MSG[0], None, iter(MSG)):
        _raises(TypeError, "argument 'messages': expected a list of bytes", lambda: P.deserialize_framed(messages, {1: FULL}, 1))
        _raises(TypeError, "argument 'messages': expected a list of bytes", lambda: P.frame_split(messages, [1]))
    _raises(TypeError, None, lambda: P.deserialize_framed(MSG, {1: FULL}, "2"))
    _raises(TypeError, None, lambda: P.deserialize_framed(MSG, {1: 5}, 1))
    _raises(OverflowError, None, lambda: P.deserialize_framed(MSG, {1: FULL}, -1))


def test_schema_errors_come_before_any_device_work():
    assert _raises(ValueError, None, lambda: P.deserialize_framed(MSG, {1: FULL, 2: "{nope"}, 1))
    assert _raises(ValueError, None, lambda: P.deserialize_framed(MSG, {1: FULL}, 1, columns=["nope"])).startswith("columns: ")
    assert _raises(ValueError, None, lambda: P.deserialize_framed(MSG, {1: FULL}, 1, reader_schema='"int"')).startswith("reader schema: ")


# ---- schema_fingerprint -----------------------------------------------------------------------------------------------------------------
PINNED = [('"null"', 7195948357588979594), ('"boolean"', 0x9F42FC78A4D4F764), ('"int"', 8247732601305521295), ('"string"', 0x8F014872634503C7),
          ('{"type":"fixed","name":"foo","size":15}', 1756455273707447556)]


@pytest.mark.parametrize("schema,value", PINNED, ids=[p[0][:16] for p in PINNED])
def test_pinned_fingerprints(schema, value):
    assert P.schema_fingerprint(schema) == value


def _crc64_bitwise(data: bytes) -> int:
    """CRC-64-AVRO bit by bit (no table): the reflected polynomial is the empty value itself."""
    empty = 0xC15D213AA4D7A795
    fp = empty
    for byte in data:
        fp ^= byte
        for _ in range(8):
            fp = (fp >> 1) ^ empty if fp & 1 else fp >> 1
    return fp


def test_canonicalisation():
    messy = """
    { "doc" : "a user",  "fields" : [
         {"type": {"type": "long", "logicalType": "timestamp-micros"}, "default": 0, "name": "at", "doc": "when", "order": "descending"},
         {"name": "who", "aliases": ["whom"], "type": ["null", {"type" : "string"}], "default": null},
         {"name": "kind", "type": {"symbols": ["A", "B"], "type": "enum", "name": "Kind", "doc": "k", "default": "A"}},
         {"name": "again", "type": "Kind"},
         {"name": "other", "type": {"type": "fixed", "size": 4, "namespace": "else.where", "name": "Four"}},
         {"name": "tags", "type": {"items": {"type": "int"}, "type": "array"}},
         {"name": "props", "type": {"values": "else.where.Four", "type": "map"}}
      ],
      "namespace" : "org.example", "aliases": ["Usr"], "type" : "record", "name" : "User" }
    """
    canonical = ('{"name":"org.example.User","type":"record","fields":['
                 '{"name":"at","type":"long"},'
                 '{"name":"who","type":["null","string"]},'
                 '{"name":"kind","type":{"name":"org.example.Kind","type":"enum","symbols":["A","B"]}},'
                 '{"name":"again","type":"org.example.Kind"},'
                 '{"name":"other","type":{"name":"else.where.Four","type":"fixed","size":4}},'
                 '{"name":"tags","type":{"type":"array","items":"int"}},'
                 '{"name":"props","type":{"type":"map","values":"else.where.Four"}}]}')
    from pyruhvro_amd.framing import parsing_canonical_form
    assert parsing_canonical_form(messy) == canonical
    assert P.schema_fingerprint(messy) == _crc64_bitwise(canonical.encode())
    assert P.schema_fingerprint(canonical) == P.schema_fingerprint(messy)
    assert _crc64_bitwise(b"") == 0xC15D213AA4D7A795
    for text, value in PINNED[:4]:
        assert _crc64_bitwise(text.encode()) == value
    assert P.schema_fingerprint('{"type": "int"}') == P.schema_fingerprint('"int"')
    assert P.schema_fingerprint(FULL) == _crc64_bitwise(parsing_canonical_form(FULL).encode())
    assert json.loads(parsing_canonical_form(FULL))["name"] == json.loads(FULL)["name"]


# ---- the CPU check -------------------------------------------------------------------------------------------------------------------------
def test_the_build_recipe_runs_frame_check():
    from pyruhvro_amd import _build
    exe = _build.build_frame_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("frame_check: ") and last.endswith(" 0 failures"), last
    assert "build_frame_check" in open(_build.ROOT + "/__graft_entry__.py").read()


def test_the_python_classification_of_the_test_cases_is_consistent():
    """frame_cases' own statement: the patterns give the classes they say, in both framings."""
    for framing in FR.FRAMINGS:
        for m in FR.CLASS_COUNTS:
            msgs, ids = FR.pattern_messages(framing, 300, m, "alternating classes")
            cls = FR.classify(msgs, ids, framing)
            assert cls.tolist() == [i % m for i in range(300)]
            assert FR.framing_error(msgs, ids, framing) is None
            msgs, ids = FR.pattern_messages(framing, 300, m, "unknown ids sprinkled in")
            assert FR.framing_error(msgs, ids, framing) == f"framed: message 3 carries schema id {FR.unknown_id(framing, 3)}, which is not in schemas"
            assert FR.framing_error(msgs, ids, framing, unknown="skip") is None
