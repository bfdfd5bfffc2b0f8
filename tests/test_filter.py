"""Row filters, the part that needs no device: the entry points exist beside an unchanged ABI, the predicate front end
(rh_filter_compile) refuses what it must with a message that starts with ``where: `` and names the field, the kernel-cache
keys of the un-filtered schemas stay where they were, and the CPU check of csrc/filter_core.h builds and passes."""
import json
import subprocess

import pytest

import filter_cases as FC
from avrogen.schemas import SCHEMAS
from test_projection import PARENT_KEYS

import pyruhvro_amd as P
from pyruhvro_amd import cabi

FULL = SCHEMAS["full"]
KINDS = FC.KINDS_SCHEMA


def test_symbols_exist_and_the_abi_is_still_7():
    L = cabi.lib()
    assert L.rh_abi_version() == 7
    for name in cabi.FILTER_SYMBOLS:
        assert getattr(L, name, None) is not None, name
    assert "filter_records" in P.__all__
    import pyruhvro
    assert pyruhvro.filter_records is P.filter_records


ACCEPTED = [
    ("age", ">=", 30), ("age", "is_null"), ("age", "not_null", None), [("age", ">=", 18), ("age", "<", 65)], ("name", "<", "m"),
    ("name", "==", b"abc"), ("created_at", "!=", -(1 << 63)), ("class", "==", "B"), ("class", "!=", "A"), [("age", ">", 1)] * 8,
    ("name", "==", "x" * 255), ("age", "<", (1 << 63) - 1),
]


@pytest.mark.parametrize("where", ACCEPTED, ids=[repr(w)[:40] for w in ACCEPTED])
def test_accepted_predicates_compile(where):
    assert cabi.Filter.get(FULL, where).handle


def test_every_kind_compiles_with_its_operators():
    for field, kind, _form in FC.KINDS_FIELDS:
        for op in FC.KIND_OPS[kind]:
            for k in FC.KIND_COMPARANDS[kind]:
                assert cabi.Filter.get(KINDS, (field, op, k)).handle
        assert cabi.Filter.get(KINDS, (field, "is_null")).handle


FIXED_ETC = json.dumps({"type": "record", "name": "N4", "fields": [
    {"name": "fx", "type": {"type": "fixed", "name": "F4", "size": 4}},
    {"name": "dec", "type": {"type": "bytes", "logicalType": "decimal", "precision": 9, "scale": 2}},
    {"name": "uu", "type": {"type": "string", "logicalType": "uuid"}},
    {"name": "nfx", "type": ["null", "F4"]},
    {"name": "x", "type": "int"}]})

# (what, schema, where, words the message must hold)
REFUSALS = [
    ("unknown field", FULL, ("nope", "==", 1), ["'nope'", "unknown"]),
    ("dotted path", FULL, ("address.city", "==", "x"), ["'address.city'", "dotted"]),
    ("record", FULL, ("address", "is_null"), ["'address'", "record", "not supported yet"]),
    ("array", FULL, ("emails", "==", "x"), ["'emails'", "array", "not supported yet"]),
    ("map", FULL, ("phone_numbers", "not_null"), ["'phone_numbers'", "map", "not supported yet"]),
    ("N-variant union", FULL, ("status", "==", 1), ["'status'", "union", "not supported yet"]),
    ("fixed", FIXED_ETC, ("fx", "==", b"abcd"), ["'fx'", "not supported yet"]),
    ("nullable fixed", FIXED_ETC, ("nfx", "is_null"), ["'nfx'", "not supported yet"]),
    ("decimal", FIXED_ETC, ("dec", "==", 1), ["'dec'", "not supported yet"]),
    ("uuid", FIXED_ETC, ("uu", "==", "x"), ["'uu'", "not supported yet"]),
    ("unknown op", FULL, ("age", "=", 1), ["'age'", "operator"]),
    ("like", FULL, ("name", "like", "a%"), ["'name'", "operator"]),
    ("bool ordered", KINDS, ("boolean_plain", "<", True), ["'boolean_plain'", "'<'"]),
    ("enum ordered", FULL, ("class", ">=", "A"), ["'class'", "'>='"]),
    ("int vs bool", FULL, ("age", "==", True), ["'age'", "bool"]),
    ("int vs float", FULL, ("age", "==", 1.0), ["'age'", "int"]),
    ("int vs str", FULL, ("age", "==", "1"), ["'age'", "int"]),
    ("int out of range", FULL, ("created_at", "<", 1 << 63), ["'created_at'", "int64"]),
    ("int below range", FULL, ("age", ">", -(1 << 63) - 1), ["'age'", "int64"]),
    ("float vs bool", KINDS, ("double_plain", "==", False), ["'double_plain'", "float"]),
    ("float vs str", KINDS, ("float_null_first", "<", "1.5"), ["'float_null_first'", "float"]),
    ("bool vs int", KINDS, ("boolean_null_last", "==", 1), ["'boolean_null_last'", "bool"]),
    ("string vs int", FULL, ("name", "==", 5), ["'name'", "str"]),
    ("bytes vs float", KINDS, ("bytes_plain", "==", 1.5), ["'bytes_plain'", "bytes"]),
    ("enum vs int", FULL, ("class", "==", 1), ["'class'", "symbol"]),
    ("unknown symbol", FULL, ("class", "==", "Z"), ["'class'", "'Z'", "symbol"]),
    ("comparand over 255 bytes", FULL, ("name", "==", "x" * 256), ["'name'", "255"]),
    ("comparand over 255 bytes (utf-8)", FULL, ("name", "<", "é" * 128), ["'name'", "255"]),
    ("comparison with None", FULL, ("age", "==", None), ["'age'", "is_null"]),
    ("is_null with a value", FULL, ("age", "is_null", 3), ["'age'", "no value"]),
    ("a list value", FULL, ("age", "==", [1]), ["'age'", "list"]),
    ("zero terms", FULL, [], ["no terms"]),
    ("nine terms", FULL, [("age", ">", 1)] * 9, ["9 terms", "8"]),
    ("second term bad", FULL, [("age", ">", 1), ("zz", "==", 2)], ["'zz'"]),
]


@pytest.mark.parametrize("what,schema,where,words", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_start_with_where_and_name_the_field(what, schema, where, words):
    calls = [lambda: cabi.Filter.get(schema, where),
             lambda: P.deserialize_array([b""], schema, where=where),      # (raised before any device work)
             lambda: P.deserialize_array_threaded([b""], schema, 2, columns=[json.loads(schema)["fields"][-1]["name"]], where=where),
             lambda: P.filter_records([b""], schema, where)]
    for f in calls:
        with pytest.raises(ValueError) as e:
            f()
        msg = str(e.value)
        assert msg.startswith("where: "), msg
        for w in words:
            assert w in msg, (w, msg)


@pytest.mark.parametrize("where", ["age", 5, {"age": 1}, ("age", "==", 1).__iter__()], ids=["str", "int", "dict", "iterator"])
def test_a_where_that_is_no_tuple_or_list_is_a_type_error(where):
    for f in (lambda: P.deserialize_array([b""], FULL, where=where), lambda: P.deserialize_array_threaded_spawn([b""], FULL, 1, where=where),
              lambda: P.deserialize_to_device([b""], FULL, 1, where=where), lambda: P.filter_records([b""], FULL, where),
              lambda: cabi.check_where(where)):
        with pytest.raises(TypeError):
            f()


@pytest.mark.parametrize("where", [[("age",)], [("age", "==", 1, 2)], [5], [(1, "==", 2)]], ids=["one", "four", "int", "name"])
def test_a_term_of_another_shape_is_refused(where):
    with pytest.raises(ValueError) as e:
        cabi.check_where(where)
    assert str(e.value).startswith("where: ")


def test_a_projected_or_resolved_schema_is_no_writer():
    import ctypes as C
    import resolve_cases as RC
    f = cabi._filter_sym("rh_filter_compile")
    term = (cabi.RhFilterTerm * 1)(cabi._filter_term("age", ">", 1))
    for s in (cabi.Schema.get(FULL, ("age", "name")), cabi.Schema.get(FULL, None, RC.FULL_MIXED)):
        out, err = C.c_void_p(), C.c_char_p()
        assert f(s.handle, term, 1, C.byref(out), C.byref(err)) == cabi.RH_ERR_ARGUMENT
        assert not out.value
        assert cabi._take_err(err).startswith("where: ")


def test_the_entry_points_that_take_no_where():
    import inspect
    for fn in (P.deserialize_array_tolerant, P.deserialize_array_threaded_tolerant, P.deserialize_binary_array_tolerant, P.validate_records,
               P.serialize_record_batch, P.serialize_record_batch_spawn, P.read_container, P.read_container_to_device,
               P.read_container_tolerant, P.read_container_to_device_tolerant):
        assert "where" not in inspect.signature(fn).parameters, fn.__name__
    with pytest.raises(ValueError) as e:
        P.deserialize_to_device([b""], FULL, 1, on_error="placeholder", where=("age", ">", 1))
    assert str(e.value).startswith("where: ")


def test_parent_kernel_keys_are_unchanged():
    for name, key in PARENT_KEYS.items():
        assert cabi.kernel_key(SCHEMAS[name]) == key, name


def test_kernel_key_does_not_depend_on_where():
    before = {(n, enc): cabi.kernel_key(SCHEMAS[n], enc) for n in ("full", "nullable_primitives") for enc in (False, True)}
    proj = cabi.kernel_key(FULL, columns=["created_at", "name"])
    cabi.Filter.get(FULL, [("age", ">=", 21), ("class", "==", "C")])
    cabi.Filter.get(SCHEMAS["nullable_primitives"], ("s", "not_null"))
    assert {(n, enc): cabi.kernel_key(SCHEMAS[n], enc) for n, enc in before} == before
    assert cabi.kernel_key(FULL, columns=["created_at", "name"]) == proj
    assert cabi.kernel_source(FULL) == cabi.kernel_source(FULL)


def test_the_build_recipe_runs_filter_check():
    from pyruhvro_amd import _build
    exe = _build.build_filter_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("filter_check: ") and last.endswith(" 0 failures"), last
    assert "build_filter_check" in open(_build.ROOT + "/__graft_entry__.py").read()
