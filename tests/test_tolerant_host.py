"""Tolerant decode, the parts that need no GPU: the placeholder datum (checked against the oracle: the strict decoder accepts
it and every nullable top-level column is null in it), its fixed bytes for a few schemas, the new symbols of the C ABI, the
kernel-cache keys that the feature must not move, and the argument errors."""
import ctypes as C
import json

import pytest

import random_cases
import test_n4_types
from avrogen.schemas import SCHEMAS
from oracle import c_walker
from test_projection import PARENT_KEYS

import pyruhvro
import pyruhvro_amd as P
from pyruhvro_amd import cabi


def _oracle_accepts(schema):
    try:
        c_walker.CompiledSchema(schema)
        return True
    except Exception:
        return False


ORACLE_SCHEMAS = sorted(k for k, v in SCHEMAS.items() if _oracle_accepts(v))
SEEDS = tuple(range(12))


def _check_placeholder(schema):
    ph = P.placeholder_datum(schema)
    batch, = c_walker.decode_threaded([ph] * 3, schema, 1)
    assert batch.num_rows == 3
    for field in json.loads(schema)["fields"]:
        t = field["type"]
        if isinstance(t, list) and "null" in t:
            # (to_pylist: an N-variant union is a sparse UnionArray, which has no validity of its own -- its null is the null branch)
            assert batch.column(field["name"]).to_pylist() == [None] * 3, field["name"]
    # the shortest datum: no prefix of it is one
    for cut in range(len(ph)):
        with pytest.raises(ValueError):
            c_walker.decode_threaded([ph[:cut]], schema, 1)


@pytest.mark.parametrize("name", ORACLE_SCHEMAS)
def test_the_oracle_accepts_the_placeholder(name):
    _check_placeholder(SCHEMAS[name])


@pytest.mark.parametrize("seed", SEEDS)
def test_the_oracle_accepts_the_placeholder_of_a_random_schema(seed):
    _check_placeholder(random_cases.random_schema(seed))


def test_placeholder_bytes():
    nil_uuid = (b"\x48" + b"00000000-0000-0000-0000-000000000000").hex()
    expected = {
        SCHEMAS["flat_primitives"]: "0000" + "00" * 4 + "00" * 8 + "00" + "00",      # int long float double boolean string
        SCHEMAS["t_union"]: "00",                                                     # ["null", string, int, boolean]
        SCHEMAS["t_nullable"]: "00" + "02",                                           # ["null", int], [string, "null"]
        SCHEMAS["array_and_map"]: "000000",
        # bytes, null, fixed(5), [fixed(3), null] -> 1, decimal on bytes, null, decimal on fixed(8), uuid text, null, time-millis,
        # null, array, map, null (of five branches), null record, string
        test_n4_types.SCHEMA: "00" + "00" + "00" * 5 + "02" + "0200" + "00" + "00" * 8 + nil_uuid + "00" + "00" + "00" + "00" + "00" + "00" + "00" + "00",
        json.dumps({"type": "record", "name": "U", "fields": [{"name": "u", "type": ["int", "string"]},
                                                             {"name": "v", "type": ["string", "int", "null"]}]}): "0000" + "04",
    }
    for schema, hexed in expected.items():
        assert P.placeholder_datum(schema).hex() == hexed, schema
    assert cabi.placeholder_datum(SCHEMAS["full"]) == P.placeholder_datum(SCHEMAS["full"]) == pyruhvro.placeholder_datum(SCHEMAS["full"])
    # a projection's placeholder is the full schema's: the patched record has every field
    h = cabi.Schema.get(SCHEMAS["full"], ("created_at", "name")).handle
    p, n = C.c_void_p(), C.c_uint64()
    assert cabi.lib().rh_schema_placeholder(h, C.byref(p), C.byref(n)) == 0
    assert C.string_at(p, n.value) == P.placeholder_datum(SCHEMAS["full"])


def test_symbols_and_abi_version():
    L = cabi.lib()
    assert L.rh_abi_version() == 7
    for sym in ("rh_schema_placeholder", "rh_record_errors_count", "rh_record_errors_get", "rh_record_errors_free", "rh_validate",
                "rh_validate_packed", "rh_validate_device", "rh_decode_tolerant", "rh_decode_packed_tolerant",
                "rh_decode_device_tolerant"):
        assert hasattr(L, sym), sym
    assert cabi.ENGINE_COUNTERS[-2:] == ("tolerant_calls", "tolerant_repairs")
    assert set(cabi.engine_counters()) == set(cabi.ENGINE_COUNTERS)
    for name in ("placeholder_datum", "validate_records", "deserialize_array_tolerant", "deserialize_array_threaded_tolerant",
                 "deserialize_binary_array_tolerant", "deserialize_to_device", "RecordError"):
        assert hasattr(P, name) and hasattr(pyruhvro, name), name
    assert P.RecordError(3, "m").index == 3 and P.RecordError(3, "m").message == "m"
    assert L.rh_record_errors_count(None) == 0


def test_kernel_keys_do_not_move():
    for name, key in PARENT_KEYS.items():
        assert cabi.kernel_key(SCHEMAS[name]) == key


def _outcome(f):
    try:
        f()
        return None
    except Exception as e:      # noqa: BLE001 - the point is to compare whatever the two calls raise
        return type(e), str(e)


def test_argument_errors():
    import numpy as np
    schema = SCHEMAS["flat_primitives"]
    good = cabi.placeholder_datum(schema)
    data, offsets = c_walker.pack([good, b"", good])
    # RH_ASYNC is refused before anything else happens, on every tolerant entry point
    for call in (lambda: cabi.decode_packed_tolerant(data, offsets, schema, 1, flags=cabi.RH_ASYNC),
                 lambda: cabi.decode_slices_tolerant(np.zeros(1, np.uint64), np.zeros(1, np.uint64), schema, 1, flags=cabi.RH_ASYNC),
                 lambda: cabi.decode_device_tolerant(0, 0, 0, 0, schema, 1, flags=cabi.RH_ASYNC)):
        with pytest.raises(ValueError, match="RH_ASYNC"):
            call()
    # max_errors = 0 is the strict call: the same outcome, whatever that is here (no device: the same RuntimeError)
    strict = _outcome(lambda: cabi.decode_packed(data, offsets, schema, 1))
    assert strict is not None
    assert _outcome(lambda: cabi.decode_packed_tolerant(data, offsets, schema, 1, max_errors=0)) == strict
    assert _outcome(lambda: P.deserialize_array_tolerant([good, b"", good], schema, max_errors=0)) == \
        _outcome(lambda: P.deserialize_array([good, b"", good], schema))
    with pytest.raises(TypeError):
        P.deserialize_array_tolerant([good], schema, max_errors="3")
    with pytest.raises(OverflowError):
        P.validate_records([good], schema, max_errors=-1)
    with pytest.raises(TypeError):
        P.deserialize_array_tolerant(["text"], schema)
    with pytest.raises(ValueError, match="on_error"):
        P.deserialize_to_device([good], schema, 1, on_error="drop")
    with pytest.raises(ValueError, match="columns"):
        P.deserialize_array_threaded_tolerant([good], schema, 1, columns=[])
