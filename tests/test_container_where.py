"""Row filters in the container read, the part that needs no device: ``read_container_where`` / ``read_container_where_to_device``
/ ``filter_container`` exist beside an unchanged ABI and four unchanged readers, the file's own errors come first, the predicate's
refusals (``where: ...``) next and both before any device work, and the CPU check of csrc/container_where_core.h builds and
passes."""
import inspect
import json
import subprocess

import pytest

import container_cases as CC
import filter_cases as FC
from avrogen.schemas import SCHEMAS

import pyruhvro
import pyruhvro_amd as P
from pyruhvro_amd import cabi

FULL = SCHEMAS["full"]
NEW_NAMES = ("read_container_where", "read_container_where_to_device", "filter_container")


def _sound_file(schema=FULL, name="full"):
    if schema is FULL:
        return CC.write(FULL, CC.split(CC.records_of("full", 12), [5, 0, 7]))
    return CC.write(schema, [list(FC.kinds_records(6))])


def test_symbols_exist_and_the_abi_is_still_7():
    L = cabi.lib()
    assert L.rh_abi_version() == 7
    assert set(cabi.CONTAINER_WHERE_SYMBOLS) >= {"rh_decode_blocks_where", "rh_decode_blocks_device_where", "rh_decode_cblocks_where",
                                                 "rh_decode_cblocks_device_where", "rh_filter_blocks", "rh_filter_cblocks",
                                                 "rh_container_where_last"}
    for name in cabi.CONTAINER_WHERE_SYMBOLS:
        assert getattr(L, name, None) is not None, name
    header = open(cabi._HERE + "/../include/ruhvro_hip.h").read()
    for name in cabi.CONTAINER_WHERE_SYMBOLS:
        assert name + "(" in header, name
    assert "#define RH_ABI_VERSION 7" in header


def test_the_names_are_in_both_alls():
    for name in NEW_NAMES:
        assert name in P.__all__ and name in pyruhvro.__all__, name
        assert getattr(pyruhvro, name) is getattr(P, name)
    assert list(inspect.signature(P.read_container_where).parameters) == ["src", "where", "num_chunks", "columns", "reader_schema", "inflate"]
    assert list(inspect.signature(P.read_container_where_to_device).parameters) == ["src", "where", "num_chunks", "device", "columns",
                                                                                    "reader_schema", "inflate"]
    assert list(inspect.signature(P.filter_container).parameters) == ["src", "where", "inflate"]
    for fn in (P.read_container_where, P.read_container_where_to_device, P.filter_container):
        kinds = {n: p.kind for n, p in inspect.signature(fn).parameters.items()}
        assert all(kinds[n] is inspect.Parameter.KEYWORD_ONLY for n in ("columns", "reader_schema", "inflate") if n in kinds)


def test_the_four_old_readers_still_take_no_where():
    for fn in (P.read_container, P.read_container_to_device, P.read_container_tolerant, P.read_container_to_device_tolerant):
        assert "where" not in inspect.signature(fn).parameters, fn.__name__
    assert list(inspect.signature(P.read_container).parameters) == ["src", "num_chunks", "columns", "reader_schema", "inflate"]
    assert list(inspect.signature(P.read_container_to_device).parameters) == ["src", "num_chunks", "device", "columns", "reader_schema", "inflate"]


# the rows of the list calls' refusals (tests/test_filter.py REFUSALS) that differ in kind, restated: (what, schema, where, words)
REFUSALS = [
    ("unknown field", FULL, ("nope", "==", 1), ["'nope'", "unknown"]),
    ("dotted path", FULL, ("address.city", "==", "x"), ["'address.city'", "dotted"]),
    ("record", FULL, ("address", "is_null"), ["'address'", "record", "not supported yet"]),
    ("array", FULL, ("emails", "==", "x"), ["'emails'", "array", "not supported yet"]),
    ("map", FULL, ("phone_numbers", "not_null"), ["'phone_numbers'", "map", "not supported yet"]),
    ("N-variant union", FULL, ("status", "==", 1), ["'status'", "union", "not supported yet"]),
    ("unknown op", FULL, ("age", "=", 1), ["'age'", "operator"]),
    ("bool ordered", FC.KINDS_SCHEMA, ("boolean_plain", "<", True), ["'boolean_plain'", "'<'"]),
    ("enum ordered", FULL, ("class", ">=", "A"), ["'class'", "'>='"]),
    ("int vs bool", FULL, ("age", "==", True), ["'age'", "bool"]),
    ("int vs float", FULL, ("age", "==", 1.0), ["'age'", "int"]),
    ("int out of range", FULL, ("created_at", "<", 1 << 63), ["'created_at'", "int64"]),
    ("float vs str", FC.KINDS_SCHEMA, ("float_null_first", "<", "1.5"), ["'float_null_first'", "float"]),
    ("string vs int", FULL, ("name", "==", 5), ["'name'", "str"]),
    ("bytes vs float", FC.KINDS_SCHEMA, ("bytes_plain", "==", 1.5), ["'bytes_plain'", "bytes"]),
    ("unknown symbol", FULL, ("class", "==", "Z"), ["'class'", "'Z'", "symbol"]),
    ("comparand over 255 bytes", FULL, ("name", "==", "x" * 256), ["'name'", "255"]),
    ("comparison with None", FULL, ("age", "==", None), ["'age'", "is_null"]),
    ("is_null with a value", FULL, ("age", "is_null", 3), ["'age'", "no value"]),
    ("a list value", FULL, ("age", "==", [1]), ["'age'", "list"]),
    ("zero terms", FULL, [], ["no terms"]),
    ("nine terms", FULL, [("age", ">", 1)] * 9, ["9 terms", "8"]),
    ("second term bad", FULL, [("age", ">", 1), ("zz", "==", 2)], ["'zz'"]),
    ("a term of another shape", FULL, [("age",)], ["term 0"]),
]


@pytest.mark.parametrize("what,schema,where,words", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_start_with_where_and_name_the_field(what, schema, where, words):
    blob = _sound_file(schema)
    last = json.loads(schema)["fields"][-1]["name"]
    calls = [lambda: P.read_container_where(blob, where),
             lambda: P.read_container_where(blob, where, 2, columns=[last]),
             lambda: P.read_container_where_to_device(blob, where, 2),
             lambda: P.filter_container(blob, where),
             lambda: P.filter_container(bytearray(blob), where, inflate="device")]
    for f in calls:
        with pytest.raises(ValueError) as e:      # (raised before any device work: this test has no device)
            f()
        msg = str(e.value)
        assert msg.startswith("where: "), msg
        for w in words:
            assert w in msg, (w, msg)


@pytest.mark.parametrize("where", ["age", 5, {"age": 1}, ("age", "==", 1).__iter__(), None], ids=["str", "int", "dict", "iterator", "none"])
def test_a_where_that_is_no_tuple_or_list_is_a_type_error(where):
    blob = _sound_file()
    for f in (lambda: P.read_container_where(blob, where), lambda: P.read_container_where_to_device(blob, where, 3),
              lambda: P.filter_container(blob, where)):
        with pytest.raises(TypeError):
            f()


def test_the_files_own_errors_come_before_the_predicate():
    blob = _sound_file()
    bad_where = ("nope", "==", 1)
    cut = blob[:len(blob) - 7]                     # the last block's sync marker is cut
    for w in (bad_where, ("age", ">=", 30), "no tuple"):
        for f in (lambda: P.read_container_where(cut, w), lambda: P.read_container_where_to_device(cut, w), lambda: P.filter_container(cut, w)):
            with pytest.raises(ValueError) as e:
                f()
            assert str(e.value).startswith("container: block 2: "), str(e.value)
        with pytest.raises(ValueError, match="^container: bad magic"):
            P.read_container_where(b"PAR1" + bytes(64), w)
        with pytest.raises(ValueError, match="^container: codec 'snappy' is not supported"):
            P.filter_container(CC.header(FULL, "snappy") + CC.block(CC.records_of("full", 3)), w)
    # num_chunks and the schema are _blocks' too
    with pytest.raises(OverflowError):
        P.read_container_where(blob, bad_where, -1)
    with pytest.raises(TypeError):
        P.read_container_where(blob, bad_where, "3")
    with pytest.raises(ValueError) as e:
        P.read_container_where(blob, bad_where, 2, columns=["no_such_column"])
    assert not str(e.value).startswith("where: ")


def test_a_bad_inflate_value_is_refused_first():
    blob = _sound_file()
    for f in (lambda: P.read_container_where(blob, ("nope", "==", 1), inflate="gpu"),
              lambda: P.read_container_where_to_device(b"not a file", ("age", ">", 1), inflate="gpu"),
              lambda: P.filter_container(blob, "no tuple", inflate=""),
              lambda: P.filter_container(blob, ("age", ">", 1), inflate="gpu")):
        with pytest.raises(ValueError) as e:
            f()
        assert str(e.value) == "container: inflate must be 'host' or 'device'"


def test_the_build_recipe_runs_container_where_check():
    from pyruhvro_amd import _build
    exe = _build.build_container_where_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("container_where_check: ") and last.endswith(" 0 failures"), last
    assert "build_container_where_check" in open(_build.ROOT + "/__graft_entry__.py").read()
